"""Vector propagation search: the host definition, in the role vbs.py and gmc.py play for their subjects.
Pure NumPy, importable without the library; every decision is integer, and the device path (``k_prop`` of
``csrc/bbme_prop.hip`` behind ``gme_prop_u8``, ``gme_seq_prop`` and ``gme_seq_read_prop``) computes what ``search`` here does,
byte for byte.

Conventions are vbs.py's: the anchor block is taken from ``previous``, a vector (column, row) says where it is found in
``current``, block (i, j) has its origin at (j B, i B); ``vbs._inside`` is the inside test and ``vbs._cost`` the cost.

* Arguments: ``block_size`` B in 4 .. 64, ``pnorm`` 0 (sum |d|) or 1 (sum d^2), ``rounds`` in 1 .. 4, ``steps`` in 0 .. 4, else
  ValueError.  ``f`` int32[Hb, Wb, >= 2] is the prior field of the pair, from any search; ``t`` (optional) the field of the
  previous pair and ``g`` (optional) one camera vector per block, both of the same shape.  Every sum stays below 2**31 (the
  largest: 64 * 64 * 255^2).
* A vector is available iff |vx| <= 2**14, |vy| <= 2**14 and the displaced block is inside; the magnitude is looked at first,
  so no input can overflow the inside test.
* Rounds: F_0 = f; round r = 1 .. rounds reads only F_(r-1) and writes F_r (Jacobi: every block of a round sees the same old
  field, whatever order the blocks run in).  ``t`` and ``g`` are the same in every round.
* Candidates of block (i, j), in this order: OWN (class 0) F_(r-1)[i, j]; SPATIAL (class 1) F_(r-1)[i + di, j + dj] for
  (di, dj) = (-1,-1), (-1,0), (-1,1), (0,-1), (0,1), (1,-1), (1,0), (1,1), neighbours outside the grid left out; TEMPORAL
  (class 2) t[i, j]; CAMERA (class 3) g[i, j]; ZERO (class 4) (0, 0), which is always available, so every block has a result
  and no cost is ever -1.  Unavailable candidates are skipped, the first available one is the initial best, and only a
  strictly smaller cost replaces it.
* Refinement, up to ``steps`` passes: the centre is the best at the start of the pass; the offsets (ox, oy) in [-1, 1]^2
  without the centre, column offset in the outer loop, both ascending (``vbs._child_search``'s order), relative to the pass's
  centre; unavailable positions are skipped; a strictly smaller cost replaces the best; a pass that changes nothing ends the
  refinement.
* Result of the last round: F_r[i, j] the best vector, ``cost`` its cost, ``source`` the class of the winning candidate, plus
  8 (MOVED) if a refinement pass moved it.  OWN is a candidate, so a block's cost never rises from round to round.
"""
import numpy as np

from vbs import _cost, _inside, psnr

MAE, MSE = 0, 1
MIN_BLOCK_SIZE, MAX_BLOCK_SIZE, MAX_ROUNDS, MAX_STEPS, MAX_COMPONENT = 4, 64, 4, 4, 1 << 14
OWN, SPATIAL, TEMPORAL, CAMERA, ZERO, MOVED = 0, 1, 2, 3, 4, 8
CLASS_NAMES = ("own", "spatial", "temporal", "camera", "zero")
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def check_args(block_size, pnorm, rounds, steps):
    """The argument rules of the definition -> (block_size, pnorm, rounds, steps) as ints, or ValueError."""
    bs, pnorm, rounds, steps = int(block_size), int(pnorm), int(rounds), int(steps)
    if not MIN_BLOCK_SIZE <= bs <= MAX_BLOCK_SIZE:
        raise ValueError("block_size %d (%d .. %d)" % (bs, MIN_BLOCK_SIZE, MAX_BLOCK_SIZE))
    if pnorm not in (MAE, MSE):
        raise ValueError("pnorm %d (0: MAE, 1: MSE)" % pnorm)
    if not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError("rounds %d (1 .. %d)" % (rounds, MAX_ROUNDS))
    if not 0 <= steps <= MAX_STEPS:
        raise ValueError("steps %d (0 .. %d)" % (steps, MAX_STEPS))
    return bs, pnorm, rounds, steps


def available(H, W, y0, x0, b, vx, vy):
    """The magnitude first, then the inside test."""
    return abs(vx) <= MAX_COMPONENT and abs(vy) <= MAX_COMPONENT and _inside(H, W, y0, x0, b, vx, vy)


def _field(a, name, Hb, Wb):
    a = np.asarray(a)
    if a.ndim != 3 or a.shape[:2] != (Hb, Wb) or a.shape[2] < 2:
        raise ValueError("%s is %r, not %r" % (name, a.shape, (Hb, Wb, 2)))
    return a[:, :, :2].astype(np.int64)        # the magnitude test sees the value as given


def _block(previous, current, F, t, g, i, j, bs, pnorm, steps):
    """One block of one round -> (vx, vy, cost, source)."""
    H, W = previous.shape
    Hb, Wb = F.shape[:2]
    y0, x0 = i * bs, j * bs
    cands = [(OWN, F[i, j])]
    cands += [(SPATIAL, F[i + di, j + dj]) for di, dj in NEIGHBOURS if 0 <= i + di < Hb and 0 <= j + dj < Wb]
    if t is not None:
        cands.append((TEMPORAL, t[i, j]))
    if g is not None:
        cands.append((CAMERA, g[i, j]))
    cands.append((ZERO, (0, 0)))
    best = None
    for cls, v in cands:
        vx, vy = int(v[0]), int(v[1])
        if not available(H, W, y0, x0, bs, vx, vy):
            continue
        c = _cost(previous, current, y0, x0, bs, vx, vy, pnorm)
        if best is None or c < best[2]:
            best = (vx, vy, c, cls)
    bx, by, bc, src = best
    for _ in range(steps):
        cx, cy, moved = bx, by, False
        for ox in (-1, 0, 1):
            for oy in (-1, 0, 1):
                if (ox, oy) == (0, 0) or not available(H, W, y0, x0, bs, cx + ox, cy + oy):
                    continue
                c = _cost(previous, current, y0, x0, bs, cx + ox, cy + oy, pnorm)
                if c < bc:
                    bx, by, bc, moved = cx + ox, cy + oy, c, True
        if not moved:
            break
        src |= MOVED
    return bx, by, bc, src


def search(previous, current, f, block_size, pnorm, rounds, steps, t=None, g=None):
    """-> (mf int32[Hb, Wb, 2], cost int64[Hb, Wb], source uint8[Hb, Wb]) of the last round."""
    bs, pnorm, rounds, steps = check_args(block_size, pnorm, rounds, steps)
    previous, current = np.asarray(previous), np.asarray(current)
    if previous.ndim != 2 or previous.dtype != np.uint8 or current.dtype != np.uint8 or previous.shape != current.shape:
        raise TypeError("previous and current must be 2-D uint8 images of one shape")
    H, W = previous.shape
    Hb, Wb = H // bs, W // bs
    F = _field(f, "f", Hb, Wb)
    t = None if t is None else _field(t, "t", Hb, Wb)
    g = None if g is None else _field(g, "g", Hb, Wb)
    cost, source = np.zeros((Hb, Wb), np.int64), np.zeros((Hb, Wb), np.uint8)
    for _ in range(rounds):
        new = np.zeros_like(F)
        for i in range(Hb):
            for j in range(Wb):
                new[i, j, 0], new[i, j, 1], cost[i, j], source[i, j] = _block(previous, current, F, t, g, i, j, bs, pnorm, steps)
        F = new
    return F.astype(np.int32), cost, source


def camera_field(h, H, W, block_size):
    """One camera vector per block, int32[Hb, Wb, 2], or None.  ``h`` float64[8] is a warp in roadmap.refine_projective's pair
    convention: a pixel of ``current`` samples ``previous`` at direct.warp(h, u, v).  The camera vector of a ``previous`` block
    is where its centre c = (x0 + (B - 1) / 2, y0 + (B - 1) / 2) lands in ``current``: p = M^-1 c with M = stabilize.matrix(h),
    the vector floor(p - c + 0.5) per component.  None where gmc.usable(h, H, W) is false, where M is singular, where a centre
    gets a non-positive denominator, or where a component exceeds 2**14.  Float64 on the host only: the device receives
    integers."""
    import gmc
    import stabilize
    bs = int(block_size)
    if not gmc.usable(h, H, W):
        return None
    h = np.asarray(h, dtype=np.float64).reshape(8)
    with np.errstate(all="ignore"):
        try:
            inv = np.linalg.inv(stabilize.matrix(h))
        except np.linalg.LinAlgError:
            return None
        if not np.all(np.isfinite(inv)):
            return None
        Hb, Wb = H // bs, W // bs
        cy, cx = np.meshgrid(np.arange(Hb) * bs + (bs - 1) / 2.0, np.arange(Wb) * bs + (bs - 1) / 2.0, indexing="ij")
        d = inv[2, 0] * cx + inv[2, 1] * cy + inv[2, 2]
        if not np.all(np.isfinite(d)) or not np.all(d > 0.0):
            return None
        px = (inv[0, 0] * cx + inv[0, 1] * cy + inv[0, 2]) / d
        py = (inv[1, 0] * cx + inv[1, 1] * cy + inv[1, 2]) / d
        v = np.stack([np.floor(px - cx + 0.5), np.floor(py - cy + 0.5)], axis=-1)
        if not np.all(np.isfinite(v)) or np.any(np.abs(v) > MAX_COMPONENT):
            return None
    return v.astype(np.int32)


def summary(f, cost_prior, mf, cost, source, sse_prior, sse_prop, height, width):
    """What the CLI reports of one pair: the share of blocks whose vector changed, the share per source class (the MOVED flag
    aside) and of moved blocks, the mean block cost before and after (the prior's over the blocks where its vector is available,
    ``cost_prior`` >= 0), and SSE and PSNR of ``current`` against ``subpel.compensate_integer`` with the prior and with the
    propagated field."""
    f, mf, source = np.asarray(f)[:, :, :2], np.asarray(mf), np.asarray(source)
    cost_prior, cost = np.asarray(cost_prior), np.asarray(cost)
    n = max(source.size, 1)
    ok = cost_prior >= 0
    p_prior, p_prop = psnr(int(sse_prior), height, width), psnr(int(sse_prop), height, width)
    return {"changed_share": float(np.any(f != mf, axis=-1).sum()) / n,
            "source_share": {name: float(((source & 7) == k).sum()) / n for k, name in enumerate(CLASS_NAMES)},
            "moved_share": float(((source & MOVED) != 0).sum()) / n,
            "mean_cost_prior": float(cost_prior[ok].mean()) if ok.any() else -1.0,
            "mean_cost_prop": float(cost.mean()) if cost.size else -1.0,
            "sse_prior": int(sse_prior), "sse_prop": int(sse_prop), "psnr_prior": p_prior, "psnr_prop": p_prop}


def prior_cost(previous, current, f, block_size, pnorm):
    """The cost of every block at its vector of ``f``, -1 where that is not available."""
    previous, current = np.asarray(previous), np.asarray(current)
    H, W = previous.shape
    bs = int(block_size)
    f = np.asarray(f)
    out = np.full(f.shape[:2], -1, np.int64)
    for i in range(f.shape[0]):
        for j in range(f.shape[1]):
            vx, vy = int(f[i, j, 0]), int(f[i, j, 1])
            if available(H, W, i * bs, j * bs, bs, vx, vy):
                out[i, j] = _cost(previous, current, i * bs, j * bs, bs, vx, vy, pnorm)
    return out


# ---- the device path --------------------------------------------------------------------------------------------------
def _camera(previous, current, camera, block_size):
    """``camera`` None, a float64[8] warp, "projective" (roadmap.refine_projective) or "affine" (the indirect affine estimate,
    as a warp) -> (g or None, h or None)."""
    if camera is None or (isinstance(camera, str) and camera == "none"):
        return None, None
    if isinstance(camera, str):
        import roadmap
        if camera == "projective":
            h = roadmap.refine_projective(previous, current)[0]
        elif camera == "affine":
            import motion
            h = roadmap.affine_to_projective(roadmap.global_motion_estimation(previous, current), int(motion.BBME_BLOCK_SIZE))
        else:
            raise ValueError("camera %r (None, a warp, 'projective', 'affine' or 'none')" % (camera,))
    else:
        h = camera
    h = np.asarray(h, dtype=np.float64).reshape(8)
    H, W = np.asarray(previous).shape
    return camera_field(h, H, W, block_size), h


def motion_field(previous, current, block_size=16, search_window=16, searching_procedure=3, pnorm_distance=0, rounds=2, steps=1,
                 camera=None):
    """bbme.get_motion_field on the device, then the propagation on the device (gme_prop_u8) -> (mf, cost, source).  ``camera``
    is None, a float64[8] warp, or "projective" for roadmap.refine_projective of the pair; a warp with no camera field
    (``camera_field`` None) gives no camera candidate."""
    import _gme_native as native
    import bbme
    pnorm = int(pnorm_distance) % 2
    check_args(block_size, pnorm, rounds, steps)
    g, _ = _camera(previous, current, camera, block_size)
    f = np.ascontiguousarray(bbme.get_motion_field(previous, current, block_size, search_window, searching_procedure, pnorm_distance)[:, :, :2])
    return native.default_context().prop(previous, current, f, block_size, pnorm, rounds, steps, None, g)


def report(frames, block_size=16, search_window=16, searching_procedure=3, pnorm_distance=0, rounds=2, steps=1, temporal=True,
           camera=None, hier=False, frame_distance=1):
    """The last pair of ``frames`` (uint8[N, H, W], N = fd + 1, or 2 fd + 1 so that the pair has a temporal prior) on the device: a
    resident sequence, the search (hierarchical if ``hier``, with search_window as its coarse window), the propagation
    (Sequence.prop) and both compensations -> ``summary`` plus the arrays."""
    import _gme_native as native
    import subpel
    frames = np.ascontiguousarray(np.stack([native.as_frame(a) for a in frames]))
    pnorm = int(pnorm_distance) % 2
    bs, pnorm, rounds, steps = check_args(block_size, pnorm, rounds, steps)
    fd = int(frame_distance)
    P = len(frames) - fd
    if P < 1:
        raise ValueError("%d frames at frame distance %d" % (len(frames), fd))
    previous, current = frames[P - 1], frames[P - 1 + fd]
    H, W = current.shape
    g, h = _camera(previous, current, camera, bs)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    try:
        if hier:
            seq.hier(fd, bs, int(search_window), 1, pnorm, 3)
        else:
            seq.bbme(fd, bs, int(search_window), int(searching_procedure), pnorm)
        f = seq.read_mv()[P - 1]
        gs = None
        if g is not None:                       # the camera field of the reported pair; the pairs before it get zeros
            gs = np.zeros((P,) + g.shape, np.int32)
            gs[P - 1] = g
        seq.prop(fd, bs, pnorm, rounds, steps, bool(temporal), gs)
        mf, cost, source = [a[0] for a in seq.read_prop(P - 1, 1)]
    finally:
        seq.close()
    cost_prior = prior_cost(previous, current, f, bs, pnorm)
    sse = [int(ctx.sse(current, subpel.compensate_integer(previous, a, bs))) for a in (f, mf)]
    out = summary(f, cost_prior, mf, cost, source, sse[0], sse[1], H, W)
    out.update(f=f, mf=mf, cost=cost, source=source, cost_prior=cost_prior, g=g, h=h, temporal=bool(temporal) and P > 1)
    return out
