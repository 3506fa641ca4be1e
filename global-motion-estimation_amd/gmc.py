"""Global motion compensation: the host definition, in the role bipred.py plays for bidirectional prediction.
Pure NumPy, importable without the library; the device path (``k_gmc`` and ``k_predict_gmc`` of ``csrc/bbme_gmc.hip`` behind
``gme_gmc_u8``, ``gme_seq_gmc``, ``gme_seq_read_gmc`` and ``gme_seq_predict_gmc``) computes what ``decide`` and ``predict`` here
do, byte for byte.

* Frames, warp and field: ``ref`` and ``cur`` are uint8[H, W]; ``cur`` is the frame being predicted.  ``h`` is float64[8] in
  direct.py's convention: pixel (u, v) of ``cur`` samples ``ref`` at ``direct.warp(h, u, v)``.  Block (i, j) of ``cur`` has its
  origin at (j B, i B).  ``f`` int32[Hb, Wb, 2] (column, row) says where that block is found in ``ref``: exactly what
  ``bbme.get_motion_field(cur, ref, ...)`` returns (the role of ``f0`` in bipred.py).
* Arguments: ``block_size`` B in 4 .. 64, ``pnorm`` 0 (sum |d|) or 1 (sum d^2), ``penalty`` in 0 .. 2**30, else ValueError.
  Every sum that enters a decision stays below 2**31 (the largest: 2**30 + 64 * 64 * 255^2).
* A warp is usable when it is finite and ``direct.corners_ok(h, H, W)`` holds.  An unusable warp is no error: no block of that
  pair has a global candidate.
* The global predictor pixel g(u, v) = floor(direct.bilinear(ref)(u', v') + 0.5) exists exactly where ``direct.residual`` calls
  the sample point valid (0 <= u' <= W - 1 and 0 <= v' <= H - 1, the far tap clamped): ``direct.compensate``'s pixel, the same
  operations in the same order, one rounding each.
* Costs of a block: cg, the cost of its g pixels against the ``cur`` block, unavailable (-1) unless the warp is usable and all
  B^2 pixels exist; cl, the cost of the ``ref`` block at f, unavailable unless the displaced block lies entirely in the frame
  (``vbs._inside``).
* Decision: the candidates (mode 0 GLOBAL, cg), (mode 1 LOCAL, cl + penalty) in that order, unavailable ones left out; only a
  strictly smaller value replaces the best, so GLOBAL wins ties.  If neither is available the block gets mode 2 (NONE) and
  cost -1.
* ``decide`` -> ``mode`` uint8[Hb, Wb]; ``cost`` int64[Hb, Wb], the chosen value (penalty included) or -1; ``costs``
  int64[Hb, Wb, 2] = (cg, cl) without the penalty, -1 where unavailable.
* ``predict``: a block of mode 0 is its g pixels, of mode 1 the ``ref`` block at f; a block of mode 2 and every pixel beyond the
  last whole block is the co-located pixel of ``ref``.
"""
import numpy as np

import direct
from vbs import _inside, psnr

MAE, MSE = 0, 1
MIN_BLOCK_SIZE, MAX_BLOCK_SIZE, MAX_PENALTY = 4, 64, 1 << 30
GLOBAL, LOCAL, NONE = 0, 1, 2


def check_args(block_size, pnorm, penalty):
    """The argument rules of the definition -> (block_size, pnorm, penalty) as ints, or ValueError."""
    bs, pnorm, penalty = int(block_size), int(pnorm), int(penalty)
    if not MIN_BLOCK_SIZE <= bs <= MAX_BLOCK_SIZE:
        raise ValueError("block_size %d (%d .. %d)" % (bs, MIN_BLOCK_SIZE, MAX_BLOCK_SIZE))
    if pnorm not in (MAE, MSE):
        raise ValueError("pnorm %d (0: MAE, 1: MSE)" % pnorm)
    if not 0 <= penalty <= MAX_PENALTY:
        raise ValueError("penalty %d (0 .. 2**30)" % penalty)
    return bs, pnorm, penalty


def default_penalty(block_size, pnorm):
    """bipred's convention, not a tuned value: a quarter grey level per pixel of the block, B^2 / 4 for MAE and 4 B^2 for
    MSE."""
    bs = int(block_size)
    return bs * bs // 4 if int(pnorm) == MAE else 4 * bs * bs


def usable(h, H, W):
    """True iff the warp is finite and its denominator is positive at the four corners of an H x W frame."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    if h.shape != (8,) or not np.all(np.isfinite(h)):
        return False
    return direct.corners_ok(h, H, W)


def global_pixels(ref, h):
    """-> (g uint8[H, W], exists bool[H, W]): the global predictor pixel of every pixel of the frame and where it exists; g is 0
    where it does not.  An unusable warp has no pixel anywhere."""
    ref = np.asarray(ref)
    H, W = ref.shape
    if not usable(h, H, W):
        return np.zeros((H, W), np.uint8), np.zeros((H, W), bool)
    h = np.asarray(h, dtype=np.float64).reshape(8)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        up, vp, _ = direct.warp(h, u, v)
        exists = (up >= 0.0) & (up <= W - 1.0) & (vp >= 0.0) & (vp <= H - 1.0)
    ups, vps = np.where(exists, up, 0.0), np.where(exists, vp, 0.0)
    val = np.floor(direct.bilinear(ref, ups, vps) + 0.5)
    return np.where(exists, val, 0.0).astype(np.uint8), exists


def _norm(d, pnorm):
    return int(np.abs(d).sum()) if pnorm == MAE else int((d * d).sum())


def _frames(ref, cur):
    ref, cur = np.asarray(ref), np.asarray(cur)
    if cur.ndim != 2 or any(a.dtype != np.uint8 or a.shape != cur.shape for a in (ref, cur)):
        raise TypeError("ref and cur must be 2-D uint8 images of one shape")
    return ref, cur


def _field(f, H, W, bs):
    f = np.asarray(f)
    if f.ndim != 3 or f.shape[:2] != (H // bs, W // bs) or f.shape[2] < 2:
        raise ValueError("f of a %d x %d frame at block size %d is %r, not %r" % (H, W, bs, (H // bs, W // bs, 2), f.shape))
    return f[:, :, :2].astype(np.int32)


def _warp(h):
    h = np.asarray(h, dtype=np.float64)
    if h.shape != (8,):
        raise ValueError("h is float64[8], not %r" % (h.shape,))
    return h


def decide(ref, cur, h, f, block_size, pnorm, penalty):
    """-> (mode uint8[Hb, Wb], cost int64[Hb, Wb], costs int64[Hb, Wb, 2])."""
    bs, pnorm, penalty = check_args(block_size, pnorm, penalty)
    ref, cur = _frames(ref, cur)
    H, W = cur.shape
    Hb, Wb = H // bs, W // bs
    f = _field(f, H, W, bs)
    g, exists = global_pixels(ref, _warp(h))
    mode = np.full((Hb, Wb), NONE, np.uint8)
    cost = np.full((Hb, Wb), -1, np.int64)
    costs = np.full((Hb, Wb, 2), -1, np.int64)
    for i in range(Hb):
        for j in range(Wb):
            y0, x0 = i * bs, j * bs
            blk = cur[y0:y0 + bs, x0:x0 + bs].astype(np.int64)
            vx, vy = int(f[i, j, 0]), int(f[i, j, 1])
            if exists[y0:y0 + bs, x0:x0 + bs].all():
                costs[i, j, 0] = _norm(g[y0:y0 + bs, x0:x0 + bs].astype(np.int64) - blk, pnorm)
            if _inside(H, W, y0, x0, bs, vx, vy):
                costs[i, j, 1] = _norm(ref[y0 + vy:y0 + vy + bs, x0 + vx:x0 + vx + bs].astype(np.int64) - blk, pnorm)
            for m, c in ((GLOBAL, costs[i, j, 0]), (LOCAL, costs[i, j, 1] + penalty)):
                if costs[i, j, m] >= 0 and (mode[i, j] == NONE or c < cost[i, j]):
                    mode[i, j], cost[i, j] = m, c
    return mode, cost, costs


def predict(ref, h, mode, f, block_size):
    """The predicted frame uint8[H, W].  A block whose mode asks for a predictor that is unavailable (mode 0 where some g pixel
    does not exist, mode 1 where the vector points outside) is a ValueError (``decide`` never yields one)."""
    bs = int(block_size)
    ref = np.asarray(ref)
    H, W = ref.shape
    mode = np.asarray(mode)
    f = _field(f, H, W, bs)
    g = exists = None
    out = ref.copy()
    for i in range(H // bs):
        for j in range(W // bs):
            y0, x0, m = i * bs, j * bs, int(mode[i, j])
            if m == GLOBAL:
                if g is None:
                    g, exists = global_pixels(ref, _warp(h))
                if not exists[y0:y0 + bs, x0:x0 + bs].all():
                    raise ValueError("block (%d, %d) of mode 0 has no global predictor" % (i, j))
                out[y0:y0 + bs, x0:x0 + bs] = g[y0:y0 + bs, x0:x0 + bs]
            elif m == LOCAL:
                vx, vy = int(f[i, j, 0]), int(f[i, j, 1])
                if not _inside(H, W, y0, x0, bs, vx, vy):
                    raise ValueError("block (%d, %d) of mode 1 points outside the frame" % (i, j))
                out[y0:y0 + bs, x0:x0 + bs] = ref[y0 + vy:y0 + vy + bs, x0 + vx:x0 + vx + bs]
    return out


def sse(a, b):
    """Exact sum of squared differences of two uint8 images."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


def all_mode(costs, which):
    """The modes that predict every block with one predictor (``which`` 0 GLOBAL or 1 LOCAL) wherever it is available (``costs``
    of ``decide``), mode 2 elsewhere: what ``summary``'s single-predictor predictions use."""
    return np.where(np.asarray(costs)[:, :, which] >= 0, which, NONE).astype(np.uint8)


def summary(mode, sse_global, sse_local, sse_chosen, height, width):
    """What the CLI reports of one pair: the share of blocks per mode, and SSE and PSNR of three predictions of ``cur``: every
    block in mode 0, every block in mode 1, and the chosen modes."""
    mode = np.asarray(mode)
    n = max(mode.size, 1)
    out = {"mode_share": [float((mode == m).sum()) / n for m in range(3)]}
    for name, s in (("global", sse_global), ("local", sse_local), ("chosen", sse_chosen)):
        out["sse_" + name] = int(s)
        out["psnr_" + name] = psnr(int(s), height, width)
    return out


# ---- the device path --------------------------------------------------------------------------------------------------
def _estimate(ref, cur, h):
    if h is not None:
        return _warp(h)
    import roadmap
    return np.asarray(roadmap.refine_projective(ref, cur)[0], dtype=np.float64)


def motion_field(ref, cur, h=None, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, penalty=None):
    """The search from ``cur`` into ``ref`` on the device (bbme.get_motion_field), then the decision on the device (gme_gmc_u8)
    -> (f, mode, cost, costs).  ``h`` None: the direct projective refinement of the pair (roadmap.refine_projective)."""
    import _gme_native as native
    import bbme
    pnorm = int(pnorm_distance) % 2
    penalty = default_penalty(block_size, pnorm) if penalty is None else penalty
    check_args(block_size, pnorm, penalty)
    h = _estimate(ref, cur, h)
    f = np.ascontiguousarray(bbme.get_motion_field(cur, ref, block_size, search_window, searching_procedure, pnorm_distance)[:, :, :2])
    return (f,) + native.default_context().gmc(ref, cur, h, f, block_size, pnorm, penalty)[:3]


def report(ref, cur, h=None, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, penalty=None):
    """One pair on the device: a two-frame sequence, the search, the decision and the prediction (Sequence.gmc, predict_gmc);
    the two single-predictor predictions it is compared with are ``predict`` on the device's field -> ``summary`` plus the
    arrays."""
    import _gme_native as native
    ref, cur = native.as_frame(ref, "ref"), native.as_frame(cur, "cur")
    pnorm = int(pnorm_distance) % 2
    penalty = default_penalty(block_size, pnorm) if penalty is None else penalty
    bs, pnorm, penalty = check_args(block_size, pnorm, penalty)
    h = _estimate(ref, cur, h)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(np.stack([ref, cur])))
    try:
        seq.gmc(1, h.reshape(1, 8), bs, int(search_window), int(searching_procedure), pnorm, penalty)
        f, mode, cost, costs, ok = [a[0] for a in seq.read_gmc()]
        sse_chosen = int(seq.predict_gmc()[0])
    finally:
        seq.close()
    H, W = cur.shape
    # one predictor everywhere, for comparison only: the definition itself on the field the device found
    single = [sse(cur, predict(ref, h, all_mode(costs, which), f, bs)) for which in (GLOBAL, LOCAL)]
    out = summary(mode, single[0], single[1], sse_chosen, H, W)
    out.update(f=f, mode=mode, cost=cost, costs=costs, penalty=penalty, h=h, usable=bool(ok))
    return out
