"""Hierarchical block matching: the host definition, in the role subpel.py plays for the quarter-pel search.
Pure NumPy, importable without the library; everything is integer, and the device path (``k_hier`` of ``csrc/bbme_hier.hip``
behind ``gme_hier_u8``, ``gme_seq_hier`` and ``gme_seq_read_hier``) computes what ``search`` here does, bit for bit.

Conventions are bbme.py's and subpel.py's: the anchor block (i, j) is taken from ``previous``, a vector says where it is found
in ``current``, component 0 is the column and component 1 the row displacement.  Pyramids are what ``utils.get_pyramids``
returns, ``[level0, level1, level2]``, coarsest first, level 2 the frame; how a pyramid is made is not part of the definition.

* Levels: ``levels`` in {1, 2, 3}; the search starts at level s = 3 - levels and ends at level 2.  The block of level l has
  side b_l = block_size >> (2 - l); block_size % 2**(levels - 1) == 0, b_s >= 4, block_size <= 64, 0 <= coarse_window <= 8 and
  0 <= radius <= 3, else ValueError.
* Grid: Hb = H // block_size, Wb = W // block_size of level 2; block (i, j) of level l has its origin at (i b_l, j b_l) and
  lies inside that level, whose sides are (n + 1) // 2 of the level below.
* Centre: (0, 0) at level s, twice the block's own vector of level l - 1 below it, clamped per component so that the displaced
  block lies inside the level: cx = clip(raw_x, -j b_l, W_l - b_l - j b_l), the same for rows.
* Candidates: radius R = coarse_window at level s, ``radius`` below.  The centre is scored first and is the initial best; then
  the offsets (ox, oy) in [-R, R]^2, column offset in the outer loop, both ascending, without the centre; a candidate whose
  block is not entirely inside the level is skipped; only a strictly smaller cost replaces the best.
* Cost: sum |d| (norm 0) or sum d^2 (norm 1) over the b_l x b_l block, at most 64 * 64 * 255^2 = 266 342 400.
"""
import numpy as np

MAE, MSE = 0, 1
MAX_BLOCK_SIZE, MAX_COARSE_WINDOW, MAX_RADIUS, MIN_TOP_BLOCK = 64, 8, 3, 4


def check_args(block_size, coarse_window, radius, pnorm, levels):
    """The argument rules of the definition -> (block_size, coarse_window, radius, pnorm, levels) as ints, or ValueError."""
    bs, cw, r, pnorm, levels = int(block_size), int(coarse_window), int(radius), int(pnorm), int(levels)
    if levels not in (1, 2, 3):
        raise ValueError("levels %d (1 .. 3)" % levels)
    if pnorm not in (MAE, MSE):
        raise ValueError("pnorm %d (0: MAE, 1: MSE)" % pnorm)
    if bs < 1 or bs > MAX_BLOCK_SIZE or bs % (1 << (levels - 1)) or (bs >> (levels - 1)) < MIN_TOP_BLOCK:
        raise ValueError("block_size %d with %d levels: a multiple of %d, at most %d, and at least %d at the coarsest level"
                         % (bs, levels, 1 << (levels - 1), MAX_BLOCK_SIZE, MIN_TOP_BLOCK))
    if not 0 <= cw <= MAX_COARSE_WINDOW:
        raise ValueError("coarse_window %d (0 .. %d)" % (cw, MAX_COARSE_WINDOW))
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError("radius %d (0 .. %d)" % (r, MAX_RADIUS))
    return bs, cw, r, pnorm, levels


def reach(coarse_window, radius, levels):
    """The largest |component| a level-2 vector can take."""
    top = 2 ** (int(levels) - 1)
    return int(coarse_window) * top + int(radius) * (top - 1)


def _costs(anchor, region, b, pnorm):
    """Costs of the b x b anchor against every b x b block of ``region`` -> int64[rows, columns] of block origins."""
    d = np.lib.stride_tricks.sliding_window_view(region, (b, b)).astype(np.int64) - anchor
    return (np.abs(d) if pnorm == MAE else d * d).sum(axis=(2, 3))


def search(prev_pyr, cur_pyr, block_size, coarse_window, radius, pnorm, levels=3):
    """-> (fields, costs): dicts over the levels used, fields[l] int32[Hb, Wb, 2], costs[l] int64[Hb, Wb]; fields[2] is the
    result in full-resolution pixels."""
    bs, cw, rad, pnorm, levels = check_args(block_size, coarse_window, radius, pnorm, levels)
    if len(prev_pyr) != 3 or len(cur_pyr) != 3:
        raise ValueError("pyramids of three levels, coarsest first")
    for l in range(3):
        p, c = np.asarray(prev_pyr[l]), np.asarray(cur_pyr[l])
        if p.ndim != 2 or p.dtype != np.uint8 or c.dtype != np.uint8 or p.shape != c.shape:
            raise TypeError("level %d: previous and current must be 2-D uint8 images of one shape" % l)
    H, W = np.asarray(prev_pyr[2]).shape
    Hb, Wb = H // bs, W // bs
    start = 3 - levels
    fields, costs = {}, {}
    for l in range(start, 3):
        prev, cur = np.asarray(prev_pyr[l]), np.asarray(cur_pyr[l])
        Hl, Wl = prev.shape
        b = bs >> (2 - l)
        R = cw if l == start else rad
        field = np.zeros((Hb, Wb, 2), np.int32)
        cost = np.zeros((Hb, Wb), np.int64)
        for i in range(Hb):
            for j in range(Wb):
                y0, x0 = i * b, j * b
                anchor = prev[y0:y0 + b, x0:x0 + b].astype(np.int64)
                raw_x, raw_y = (0, 0) if l == start else (2 * int(fields[l - 1][i, j, 0]), 2 * int(fields[l - 1][i, j, 1]))
                cx = min(max(raw_x, -x0), Wl - b - x0)
                cy = min(max(raw_y, -y0), Hl - b - y0)
                # the offsets of [-R, R]^2 whose block lies inside the level: a rectangle that holds the centre
                ox_lo, ox_hi = max(-R, -(x0 + cx)), min(R, Wl - b - (x0 + cx))
                oy_lo, oy_hi = max(-R, -(y0 + cy)), min(R, Hl - b - (y0 + cy))
                region = cur[y0 + cy + oy_lo:y0 + cy + oy_hi + b, x0 + cx + ox_lo:x0 + cx + ox_hi + b]
                by_column = _costs(anchor, region, b, pnorm).T                  # [ox - ox_lo, oy - oy_lo]
                best, bx, by = int(by_column[-ox_lo, -oy_lo]), cx, cy           # the centre first
                # column offset in the outer loop, both ascending: argmin returns the first minimum in that order, and only
                # a strictly smaller cost replaces the centre
                k = int(np.argmin(by_column))
                if int(by_column.flat[k]) < best:
                    kx, ky = divmod(k, by_column.shape[1])
                    best, bx, by = int(by_column.flat[k]), cx + ox_lo + kx, cy + oy_lo + ky
                field[i, j] = (bx, by)
                cost[i, j] = best
        fields[l], costs[l] = field, cost
    return fields, costs


def psnr(sse_value, height, width):
    """utils.PSNR from an exact sum of squared errors: -1 where the frames are equal."""
    if sse_value == 0:
        return -1.0
    return float(20.0 * np.log10(255.0 / np.sqrt(float(sse_value) / (height * width))))


def summary(field, sse_value, height, width, coarse_window, radius, levels):
    """What the CLI reports of one pair: the reach in pixels, the field's median vector and the PSNR of ``current`` against
    the compensation of ``previous`` by the field."""
    v = np.asarray(field).reshape(-1, 2)
    return {"reach": reach(coarse_window, radius, levels),
            "median_vector": [float(np.median(v[:, 0])), float(np.median(v[:, 1]))] if len(v) else [0.0, 0.0],
            "sse": int(sse_value), "psnr": psnr(int(sse_value), height, width)}


# ---- the device path --------------------------------------------------------------------------------------------------
def motion_field(previous, current, block_size=16, coarse_window=8, radius=1, pnorm_distance=0, levels=3):
    """The search of one pair on the device (gme_hier_u8), pyramids included -> (field int32[Hb, Wb, 2], cost int64[Hb, Wb])
    of level 2."""
    import _gme_native as native
    return native.default_context().hier(previous, current, block_size, coarse_window, radius, int(pnorm_distance) % 2, levels)


def report(previous, current, block_size=16, coarse_window=8, radius=1, pnorm_distance=0, levels=3):
    """One pair on the device: the search, then ``ctx.compensate(previous, field)`` against ``current`` -> ``summary`` plus
    the field and its costs."""
    import _gme_native as native
    previous, current = native.as_frame(previous, "previous"), native.as_frame(current, "current")
    field, cost = motion_field(previous, current, block_size, coarse_window, radius, pnorm_distance, levels)
    ctx = native.default_context()
    sse = ctx.sse(current, ctx.compensate(previous, field)) if field.size else ctx.sse(current, previous)
    out = summary(field, sse, previous.shape[0], previous.shape[1], coarse_window, radius, levels)
    out.update(field=field, cost=cost)
    return out
