"""Variable-block-size motion: the host definition, in the role subpel.py and hier.py play for their
searches.  Pure NumPy, importable without the library; everything is integer, and the device path (``k_vbs`` of
``csrc/bbme_vbs.hip`` behind ``gme_vbs_u8``, ``gme_seq_vbs``, ``gme_seq_read_vbs`` and ``gme_seq_compensate_vbs``) computes
what ``tree`` here does, byte for byte.

Conventions are bbme.py's, subpel.py's and hier.py's: the anchor block is taken from ``previous``, a vector says where it is
found in ``current``, component 0 is the column and component 1 the row displacement; a displaced block is inside iff it lies
entirely in the frame.

* Arguments: ``block_size`` B, the side of the root blocks (the block size of the input field); ``depth`` D in {0, 1, 2};
  ``radius`` r in 0 .. 3; ``pnorm`` 0 (sum |d|) or 1 (sum d^2); ``penalty`` lambda in 0 .. 2**30; B % 2**D == 0, B >> D >= 4 and
  B <= 64, else ValueError.  Every sum that enters a decision stays below 2**31 (the largest: lambda + 4 * 32 * 32 * 255^2).
* Root (i, j) has its origin at (j B, i B) and the vector v = mf[i, j].  If its displaced block is not inside, the root is a
  leaf of depth 0 with tree cost -1 and its cells carry v (the rule of subpel.refine).  Otherwise its own cost c is the cost
  at v.
* Node (origin, side b, vector v, own cost c, depth d): a leaf with F = c if d == D.  Otherwise four children of side b / 2,
  child k at row k >> 1 and column k & 1 of the node.  A child's centre is the parent's v (inside, because the parent's block
  is); the centre is scored first and is the initial best; then the offsets (ox, oy) in [-r, r]^2 without the centre, column
  offset in the outer loop, both ascending; a candidate whose block is not inside is skipped; only a strictly smaller cost
  replaces the best.  Each child is a node of depth d + 1 with its winning vector and cost, resolved first.  With
  S = lambda + sum F_k the node splits iff S < c (a tie does not split), and F = min(c, S).
* Result per pair, g = B >> D the leaf grid: ``leaf`` int32[Hb 2^D, Wb 2^D, 2], every g x g cell carries the vector of the
  leaf that covers it; ``depth`` uint8 of the same grid, the depth of that leaf; ``cost`` int64[Hb, Wb], F of the root
  (penalties included) or -1.
* Compensation is ``subpel.compensate_integer(previous, leaf, g)``: the per-pixel rule of the integer fields at the leaf size.
"""
import numpy as np

MAE, MSE = 0, 1
MAX_BLOCK_SIZE, MAX_DEPTH, MAX_RADIUS, MIN_LEAF, MAX_PENALTY = 64, 2, 3, 4, 1 << 30


def check_args(block_size, depth, radius, pnorm, penalty):
    """The argument rules of the definition -> (block_size, depth, radius, pnorm, penalty) as ints, or ValueError."""
    bs, depth, r, pnorm, penalty = int(block_size), int(depth), int(radius), int(pnorm), int(penalty)
    if depth not in (0, 1, 2):
        raise ValueError("depth %d (0 .. %d)" % (depth, MAX_DEPTH))
    if pnorm not in (MAE, MSE):
        raise ValueError("pnorm %d (0: MAE, 1: MSE)" % pnorm)
    if bs < 1 or bs > MAX_BLOCK_SIZE or bs % (1 << depth) or (bs >> depth) < MIN_LEAF:
        raise ValueError("block_size %d with depth %d: a multiple of %d, at most %d, and leaves of at least %d"
                         % (bs, depth, 1 << depth, MAX_BLOCK_SIZE, MIN_LEAF))
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError("radius %d (0 .. %d)" % (r, MAX_RADIUS))
    if not 0 <= penalty <= MAX_PENALTY:
        raise ValueError("penalty %d (0 .. 2**30)" % penalty)
    return bs, depth, r, pnorm, penalty


def default_penalty(block_size, pnorm):
    """The CLI's convention, not a tuned value: one grey level per pixel of the root, B^2 for MAE and 16 B^2 for MSE."""
    bs = int(block_size)
    return bs * bs if int(pnorm) == MAE else 16 * bs * bs


def _cost(previous, current, y0, x0, b, vx, vy, pnorm):
    d = current[y0 + vy:y0 + vy + b, x0 + vx:x0 + vx + b].astype(np.int64) - previous[y0:y0 + b, x0:x0 + b].astype(np.int64)
    return int(np.abs(d).sum()) if pnorm == MAE else int((d * d).sum())


def _inside(H, W, y0, x0, b, vx, vy):
    return x0 + vx >= 0 and y0 + vy >= 0 and x0 + vx + b <= W and y0 + vy + b <= H


def _child_search(previous, current, y0, x0, b, vx, vy, r, pnorm):
    """The search of one child around its parent's vector -> (vx, vy, cost)."""
    H, W = previous.shape
    best, bx, by = _cost(previous, current, y0, x0, b, vx, vy, pnorm), vx, vy
    for ox in range(-r, r + 1):
        for oy in range(-r, r + 1):
            if (ox, oy) == (0, 0) or not _inside(H, W, y0, x0, b, vx + ox, vy + oy):
                continue
            c = _cost(previous, current, y0, x0, b, vx + ox, vy + oy, pnorm)
            if c < best:
                best, bx, by = c, vx + ox, vy + oy
    return bx, by, best


def _node(previous, current, y0, x0, b, vx, vy, c, d, D, r, pnorm, penalty, g, leaf, depth):
    """Resolves the node bottom-up, writes its cells and returns F."""
    cells = slice(y0 // g, (y0 + b) // g), slice(x0 // g, (x0 + b) // g)
    if d < D:
        h = b // 2
        kept = leaf[cells].copy(), depth[cells].copy()
        S = penalty
        for k in range(4):
            cy, cx = y0 + (k >> 1) * h, x0 + (k & 1) * h
            kx, ky, kc = _child_search(previous, current, cy, cx, h, vx, vy, r, pnorm)
            S += _node(previous, current, cy, cx, h, kx, ky, kc, d + 1, D, r, pnorm, penalty, g, leaf, depth)
        if S < c:
            return S
        leaf[cells], depth[cells] = kept
    leaf[cells] = (vx, vy)
    depth[cells] = d
    return c


def tree(previous, current, mf, block_size, depth, radius, pnorm, penalty):
    """-> (leaf int32[Hb 2^D, Wb 2^D, 2], depth uint8[Hb 2^D, Wb 2^D], cost int64[Hb, Wb]) of the field mf int32[Hb, Wb, 2]."""
    bs, D, r, pnorm, penalty = check_args(block_size, depth, radius, pnorm, penalty)
    previous, current = np.asarray(previous), np.asarray(current)
    if previous.ndim != 2 or previous.dtype != np.uint8 or current.dtype != np.uint8 or previous.shape != current.shape:
        raise TypeError("previous and current must be 2-D uint8 images of one shape")
    H, W = previous.shape
    Hb, Wb = H // bs, W // bs
    mf = np.asarray(mf)
    if mf.shape[:2] != (Hb, Wb) or mf.ndim != 3 or mf.shape[2] < 2:
        raise ValueError("the field of a %d x %d frame at block size %d is %r, not %r" % (H, W, bs, (Hb, Wb, 2), mf.shape))
    n, g = 1 << D, bs >> D
    leaf = np.zeros((Hb * n, Wb * n, 2), np.int32)
    depths = np.zeros((Hb * n, Wb * n), np.uint8)
    cost = np.full((Hb, Wb), -1, np.int64)
    for i in range(Hb):
        for j in range(Wb):
            vx, vy = int(mf[i, j, 0]), int(mf[i, j, 1])
            y0, x0 = i * bs, j * bs
            if not _inside(H, W, y0, x0, bs, vx, vy):
                leaf[i * n:(i + 1) * n, j * n:(j + 1) * n] = (vx, vy)
                continue
            c = _cost(previous, current, y0, x0, bs, vx, vy, pnorm)
            cost[i, j] = _node(previous, current, y0, x0, bs, vx, vy, c, 0, D, r, pnorm, penalty, g, leaf, depths)
    return leaf, depths, cost


def psnr(sse_value, height, width):
    """utils.PSNR from an exact sum of squared errors: -1 where the frames are equal."""
    if sse_value == 0:
        return -1.0
    return float(20.0 * np.log10(255.0 / np.sqrt(float(sse_value) / (height * width))))


def summary(depth_map, tree_depth, sse_root, sse_leaf, height, width):
    """What the CLI reports of one pair: the share of roots split, the leaves per depth, and SSE and PSNR of ``current``
    against the compensations by the root field and by the leaf field."""
    D = int(tree_depth)
    n = 1 << D
    dm = np.asarray(depth_map)
    roots = dm[::n, ::n]
    leaves = [int((dm == d).sum()) >> (2 * (D - d)) for d in range(D + 1)]
    p_root, p_leaf = psnr(int(sse_root), height, width), psnr(int(sse_leaf), height, width)
    return {"split_share": float(np.mean(roots > 0)) if roots.size else 0.0, "leaves": leaves,
            "sse_root": int(sse_root), "sse_leaf": int(sse_leaf), "psnr_root": p_root, "psnr_leaf": p_leaf,
            "psnr_gain": p_leaf - p_root}


# ---- the device path --------------------------------------------------------------------------------------------------
def motion_field(previous, current, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, depth=2, radius=1,
                 penalty=None):
    """bbme.get_motion_field on the device, then the tree on the device (gme_vbs_u8) -> (leaf, depth, cost)."""
    import _gme_native as native
    import bbme
    pnorm = int(pnorm_distance) % 2
    penalty = default_penalty(block_size, pnorm) if penalty is None else penalty
    check_args(block_size, depth, radius, pnorm, penalty)
    mf = bbme.get_motion_field(previous, current, block_size, search_window, searching_procedure, pnorm_distance)
    return native.default_context().vbs(previous, current, mf, block_size, depth, radius, pnorm, penalty)


def report(previous, current, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, depth=2, radius=1,
           penalty=None, hier=False):
    """One pair on the device: the search (hierarchical if ``hier``, with search_window as its coarse window), the tree and both
    compensations -> ``summary`` plus the fields."""
    import _gme_native as native
    import motion
    previous, current = native.as_frame(previous, "previous"), native.as_frame(current, "current")
    pnorm = int(pnorm_distance) % 2
    penalty = default_penalty(block_size, pnorm) if penalty is None else penalty
    bs, depth, radius, pnorm, penalty = check_args(block_size, depth, radius, pnorm, penalty)
    seq = motion._pair_sequence(previous, current)
    if hier:
        seq.hier(1, bs, int(search_window), 1, pnorm, 3)
    else:
        seq.bbme(1, bs, int(search_window), int(searching_procedure), pnorm)
    mf = seq.read_mv()[0]
    seq.vbs(1, bs, depth, radius, pnorm, penalty)
    leaf, depths, cost = seq.read_vbs()
    sse_leaf = int(seq.compensate_vbs(1, bs)[0])
    ctx = native.default_context()
    sse_root = ctx.sse(current, ctx.compensate(previous, mf)) if mf.size else ctx.sse(current, previous)
    out = summary(depths[0], depth, sse_root, sse_leaf, *previous.shape)
    out.update(mf=mf, leaf=leaf[0], depth=depths[0], cost=cost[0], penalty=penalty)
    return out
