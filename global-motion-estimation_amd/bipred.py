"""Bidirectional block prediction: the host definition, in the role vbs.py plays for variable block size.
Pure NumPy, importable without the library; everything is integer, and the device path (``k_bipred`` and ``k_predict_bipred``
of ``csrc/bbme_bipred.hip`` behind ``gme_bipred_u8``, ``gme_seq_bipred``, ``gme_seq_read_bipred`` and
``gme_seq_predict_bipred``) computes what ``decide`` and ``predict`` here do, byte for byte.

* Frames and fields: ``past``, ``mid``, ``next`` are uint8[H, W]; ``mid`` is the frame being predicted.  Block (i, j) of
  ``mid`` has its origin at (j B, i B).  ``f0`` int32[Hb, Wb, 2] (column, row) says where that block is found in ``past``:
  exactly what ``bbme.get_motion_field(mid, past, ...)`` returns; ``f1`` the same into ``next``.  A displaced block is inside
  iff it lies entirely in the frame (``vbs._inside``).
* Arguments: ``block_size`` B in 4 .. 64, ``radius`` r in 0 .. 2, ``rounds`` in 0 .. 2, ``pnorm`` 0 (sum |d|) or 1 (sum d^2),
  ``penalty`` in 0 .. 2**30, else ValueError.  Every sum that enters a decision stays below 2**31 (the largest:
  2**30 + 64 * 64 * 255^2).
* Costs of a block: c0, the cost of the ``mid`` block against ``past`` at f0, unavailable (-1) if that block is not inside;
  c1 the same for ``next`` at f1.  The averaged predictor is (p + n + 1) >> 1 per pixel.  cb exists only when both vectors are
  inside and starts as the cost of the averaged predictor at (f0, f1).
* Refinement of cb: each of the ``rounds`` rounds runs two passes.  Pass 1 holds the ``next`` vector and tries the ``past``
  vector at centre + (ox, oy), (ox, oy) in [-r, r]^2 without the centre, the centre being the ``past`` vector at the start of
  the pass; column offset in the outer loop, both ascending; a candidate that is not inside is skipped; only a strictly
  smaller cost replaces the best.  Pass 2 holds the new ``past`` vector and does the same for the ``next`` vector.
* Decision: the candidates (mode 0, c0), (mode 1, c1), (mode 2, cb + penalty) in that order, unavailable ones left out; only a
  strictly smaller value replaces the best.  If none is available the block gets mode 3 and cost -1.
* ``decide`` -> ``mode`` uint8[Hb, Wb]; ``v0``, ``v1`` int32[Hb, Wb, 2], the refined pair where mode is 2 and the inputs
  elsewhere; ``cost`` int64[Hb, Wb], the chosen value (penalty included) or -1; ``costs`` int64[Hb, Wb, 3] = (c0, c1, cb
  without the penalty), -1 where unavailable.
* ``predict``: mode 0 the ``past`` block at v0, mode 1 the ``next`` block at v1, mode 2 their rounded average; mode 3 and every
  pixel beyond the last whole block the co-located pixel of ``past``.
"""
import numpy as np

from vbs import _inside, psnr

MAE, MSE = 0, 1
MIN_BLOCK_SIZE, MAX_BLOCK_SIZE, MAX_RADIUS, MAX_ROUNDS, MAX_PENALTY = 4, 64, 2, 2, 1 << 30
PAST, NEXT, BOTH, NONE = 0, 1, 2, 3


def check_args(block_size, radius, rounds, pnorm, penalty):
    """The argument rules of the definition -> (block_size, radius, rounds, pnorm, penalty) as ints, or ValueError."""
    bs, r, rounds, pnorm, penalty = int(block_size), int(radius), int(rounds), int(pnorm), int(penalty)
    if not MIN_BLOCK_SIZE <= bs <= MAX_BLOCK_SIZE:
        raise ValueError("block_size %d (%d .. %d)" % (bs, MIN_BLOCK_SIZE, MAX_BLOCK_SIZE))
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError("radius %d (0 .. %d)" % (r, MAX_RADIUS))
    if not 0 <= rounds <= MAX_ROUNDS:
        raise ValueError("rounds %d (0 .. %d)" % (rounds, MAX_ROUNDS))
    if pnorm not in (MAE, MSE):
        raise ValueError("pnorm %d (0: MAE, 1: MSE)" % pnorm)
    if not 0 <= penalty <= MAX_PENALTY:
        raise ValueError("penalty %d (0 .. 2**30)" % penalty)
    return bs, r, rounds, pnorm, penalty


def default_penalty(block_size, pnorm):
    """The CLI's convention, not a tuned value: a quarter grey level per pixel of the block, B^2 / 4 for MAE and 4 B^2 for
    MSE."""
    bs = int(block_size)
    return bs * bs // 4 if int(pnorm) == MAE else 4 * bs * bs


def _norm(d, pnorm):
    return int(np.abs(d).sum()) if pnorm == MAE else int((d * d).sum())


def _block(frame, y0, x0, b, v):
    return frame[y0 + v[1]:y0 + v[1] + b, x0 + v[0]:x0 + v[0] + b].astype(np.int64)


def _cost_one(ref, mid, y0, x0, b, v, pnorm):
    return _norm(_block(ref, y0, x0, b, v) - mid[y0:y0 + b, x0:x0 + b].astype(np.int64), pnorm)


def _cost_both(past, mid, nxt, y0, x0, b, v0, v1, pnorm):
    avg = (_block(past, y0, x0, b, v0) + _block(nxt, y0, x0, b, v1) + 1) >> 1
    return _norm(avg - mid[y0:y0 + b, x0:x0 + b].astype(np.int64), pnorm)


def _refine(past, mid, nxt, y0, x0, b, v0, v1, cb, r, rounds, pnorm):
    """The alternating passes on the pair (v0, v1) -> (v0, v1, cb)."""
    H, W = mid.shape
    for _ in range(rounds):
        for side in (0, 1):
            centre = (v0, v1)[side]
            for ox in range(-r, r + 1):
                for oy in range(-r, r + 1):
                    cand = (centre[0] + ox, centre[1] + oy)
                    if (ox, oy) == (0, 0) or not _inside(H, W, y0, x0, b, cand[0], cand[1]):
                        continue
                    pair = (cand, v1) if side == 0 else (v0, cand)
                    c = _cost_both(past, mid, nxt, y0, x0, b, pair[0], pair[1], pnorm)
                    if c < cb:
                        cb, v0, v1 = c, pair[0], pair[1]
    return v0, v1, cb


def _frames(past, mid, nxt):
    past, mid, nxt = np.asarray(past), np.asarray(mid), np.asarray(nxt)
    if mid.ndim != 2 or any(a.dtype != np.uint8 or a.shape != mid.shape for a in (past, mid, nxt)):
        raise TypeError("past, mid and next must be 2-D uint8 images of one shape")
    return past, mid, nxt


def _field(f, name, H, W, bs):
    f = np.asarray(f)
    if f.ndim != 3 or f.shape[:2] != (H // bs, W // bs) or f.shape[2] < 2:
        raise ValueError("%s of a %d x %d frame at block size %d is %r, not %r" % (name, H, W, bs, (H // bs, W // bs, 2), f.shape))
    return f[:, :, :2].astype(np.int32)


def decide(past, mid, next, f0, f1, block_size, radius, rounds, pnorm, penalty):
    """-> (mode uint8[Hb, Wb], v0 int32[Hb, Wb, 2], v1 int32[Hb, Wb, 2], cost int64[Hb, Wb], costs int64[Hb, Wb, 3])."""
    bs, r, rounds, pnorm, penalty = check_args(block_size, radius, rounds, pnorm, penalty)
    past, mid, nxt = _frames(past, mid, next)
    H, W = mid.shape
    Hb, Wb = H // bs, W // bs
    v0, v1 = _field(f0, "f0", H, W, bs), _field(f1, "f1", H, W, bs)
    mode = np.full((Hb, Wb), NONE, np.uint8)
    cost = np.full((Hb, Wb), -1, np.int64)
    costs = np.full((Hb, Wb, 3), -1, np.int64)
    for i in range(Hb):
        for j in range(Wb):
            y0, x0 = i * bs, j * bs
            a, b = (int(v0[i, j, 0]), int(v0[i, j, 1])), (int(v1[i, j, 0]), int(v1[i, j, 1]))
            in0, in1 = _inside(H, W, y0, x0, bs, *a), _inside(H, W, y0, x0, bs, *b)
            if in0:
                costs[i, j, 0] = _cost_one(past, mid, y0, x0, bs, a, pnorm)
            if in1:
                costs[i, j, 1] = _cost_one(nxt, mid, y0, x0, bs, b, pnorm)
            if in0 and in1:
                cb = _cost_both(past, mid, nxt, y0, x0, bs, a, b, pnorm)
                a, b, cb = _refine(past, mid, nxt, y0, x0, bs, a, b, cb, r, rounds, pnorm)
                costs[i, j, 2] = cb
            for m, c in ((PAST, costs[i, j, 0]), (NEXT, costs[i, j, 1]), (BOTH, costs[i, j, 2] + penalty)):
                if costs[i, j, m] >= 0 and (mode[i, j] == NONE or c < cost[i, j]):
                    mode[i, j], cost[i, j] = m, c
            if mode[i, j] == BOTH:
                v0[i, j], v1[i, j] = a, b
    return mode, v0, v1, cost, costs


def predict(past, next, mode, v0, v1, block_size):
    """The predicted frame uint8[H, W].  A block of mode 0 .. 2 whose vector in use does not point inside is a ValueError
    (``decide`` never yields one)."""
    bs = int(block_size)
    past, nxt = np.asarray(past), np.asarray(next)
    H, W = past.shape
    mode = np.asarray(mode)
    v0, v1 = _field(v0, "v0", H, W, bs), _field(v1, "v1", H, W, bs)
    out = past.copy()
    for i in range(H // bs):
        for j in range(W // bs):
            y0, x0, m = i * bs, j * bs, int(mode[i, j])
            a, b = (int(v0[i, j, 0]), int(v0[i, j, 1])), (int(v1[i, j, 0]), int(v1[i, j, 1]))
            if m > BOTH:
                continue
            if (m != NEXT and not _inside(H, W, y0, x0, bs, *a)) or (m != PAST and not _inside(H, W, y0, x0, bs, *b)):
                raise ValueError("block (%d, %d) of mode %d points outside the frame" % (i, j, m))
            if m == PAST:
                blk = _block(past, y0, x0, bs, a)
            elif m == NEXT:
                blk = _block(nxt, y0, x0, bs, b)
            else:
                blk = (_block(past, y0, x0, bs, a) + _block(nxt, y0, x0, bs, b) + 1) >> 1
            out[y0:y0 + bs, x0:x0 + bs] = blk.astype(np.uint8)
    return out


def sse(a, b):
    """Exact sum of squared differences of two uint8 images."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


def summary(mode, f0, f1, v0, v1, sse_past, sse_next, sse_chosen, height, width):
    """What the CLI reports of one triple: the share of blocks per mode, the share whose vectors the refinement moved, and SSE
    and PSNR of three predictions of ``mid``: every block in mode 0, every block in mode 1, and the chosen modes."""
    mode = np.asarray(mode)
    moved = np.any(np.asarray(v0) != np.asarray(f0)[:, :, :2], axis=2) | np.any(np.asarray(v1) != np.asarray(f1)[:, :, :2], axis=2)
    n = max(mode.size, 1)
    out = {"mode_share": [float((mode == m).sum()) / n for m in range(4)], "refined_share": float(moved.sum()) / n}
    for name, s in (("past", sse_past), ("next", sse_next), ("chosen", sse_chosen)):
        out["sse_" + name] = int(s)
        out["psnr_" + name] = psnr(int(s), height, width)
    return out


def all_mode(field, which, H, W, block_size):
    """The modes that predict every block from one reference (``which`` 0 or 1) wherever its vector points inside, mode 3
    elsewhere: what ``summary``'s single-reference predictions use."""
    bs = int(block_size)
    f = np.asarray(field)
    y0, x0 = np.arange(H // bs)[:, None] * bs, np.arange(W // bs)[None, :] * bs
    ok = (x0 + f[:, :, 0] >= 0) & (y0 + f[:, :, 1] >= 0) & (x0 + f[:, :, 0] + bs <= W) & (y0 + f[:, :, 1] + bs <= H)
    return np.where(ok, which, NONE).astype(np.uint8)


# ---- the device path --------------------------------------------------------------------------------------------------
def motion_field(past, mid, next, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, radius=1, rounds=1,
                 penalty=None):
    """Both searches from ``mid`` on the device (bbme.get_motion_field), then the decision on the device (gme_bipred_u8) ->
    (mode, v0, v1, cost, costs)."""
    import _gme_native as native
    import bbme
    pnorm = int(pnorm_distance) % 2
    penalty = default_penalty(block_size, pnorm) if penalty is None else penalty
    check_args(block_size, radius, rounds, pnorm, penalty)
    f0 = bbme.get_motion_field(mid, past, block_size, search_window, searching_procedure, pnorm_distance)
    f1 = bbme.get_motion_field(mid, next, block_size, search_window, searching_procedure, pnorm_distance)
    return native.default_context().bipred(past, mid, next, f0, f1, block_size, radius, rounds, pnorm, penalty)[:5]


def report(past, mid, next, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, radius=1, rounds=1,
           penalty=None):
    """One triple on the device: a three-frame sequence, both searches, the decision and the prediction (Sequence.bipred,
    predict_bipred); the two single-reference predictions it is compared with are ``predict`` on the device's fields ->
    ``summary`` plus the fields."""
    import _gme_native as native
    past, mid, nxt = native.as_frame(past, "past"), native.as_frame(mid, "mid"), native.as_frame(next, "next")
    pnorm = int(pnorm_distance) % 2
    penalty = default_penalty(block_size, pnorm) if penalty is None else penalty
    bs, radius, rounds, pnorm, penalty = check_args(block_size, radius, rounds, pnorm, penalty)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(np.stack([past, mid, nxt])))
    try:
        seq.bipred(1, bs, int(search_window), int(searching_procedure), pnorm, radius, rounds, penalty)
        f0, f1, mode, v0, v1, cost, costs = [a[0] for a in seq.read_bipred()]
        sse_chosen = int(seq.predict_bipred()[0])
    finally:
        seq.close()
    H, W = mid.shape
    # a single reference everywhere, for comparison only: the definition itself on the fields the device found
    single = []
    for which, f in ((PAST, f0), (NEXT, f1)):
        want = all_mode(f, which, H, W, bs)
        single.append(sse(mid, predict(past, nxt, want, f0, f1, bs)))
    out = summary(mode, f0, f1, v0, v1, single[0], single[1], sse_chosen, H, W)
    out.update(f0=f0, f1=f1, mode=mode, v0=v0, v1=v1, cost=cost, costs=costs, penalty=penalty)
    return out
