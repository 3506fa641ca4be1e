"""Quarter-pel block matching: the host definition, in the role stabilize.py and mosaic.py play for their
features.  Pure NumPy, importable without the library; everything is integer, and the device path (``csrc/bbme_subpel.hip``
behind ``gme_subpel_u8``, ``gme_seq_subpel``, ``gme_seq_read_qmv`` and ``gme_seq_compensate_qpel``) computes what ``refine`` and
``compensate`` here do, bit for bit.

Conventions are bbme.py's: the anchor block (i, j) is ``previous[i*bs:(i+1)*bs, j*bs:(j+1)*bs]``, a vector says where it is
found in ``current``, component 0 is the column and component 1 the row displacement.  A quarter-pel field is
int32[Hb, Wb, 2] in units of 1/4 pixel; ``4 * mf`` is the integer field ``mf`` in that unit.

* ``interp_block``: the block of an image at origin (X, Y) in quarter units (column, row): x0 = X >> 2, fx = X & 3 (floor
  semantics, so negative origins work), the same for y; inside iff x0 >= 0, y0 >= 0, x0 + bs - 1 + (fx != 0) <= W - 1 and
  y0 + bs - 1 + (fy != 0) <= H - 1; pixel = ((4-fx)(4-fy) p00 + fx (4-fy) p01 + (4-fx) fy p10 + fx fy p11 + 8) >> 4 with p01
  one column to the right, p10 one row down, p11 both.  A tap of weight zero is not read.
* ``cost``: interpolated block of ``current`` at (4 c0 + X, 4 r0 + Y) against the anchor: sum |d| (norm 0) or sum d^2 (norm 1).
* ``refine``: from 4 mf, eight half-pel candidates, then eight quarter-pel candidates around the half-pel winner; column offset
  in the outer loop, only a strictly smaller cost replaces the best, so the first minimum wins and the centre wins ties.
* ``compensate``: motion.compensate_frame's rule moved to quarter units, block by block.
"""
import numpy as np

MAE, MSE = 0, 1
OFFSETS = tuple((ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1) if (ox, oy) != (0, 0))   # column offset outer


def _frame(a, name):
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise TypeError("%s must be a 2-D uint8 image" % name)
    return a


def interp_block(img, X, Y, bs):
    """The bs x bs block of ``img`` at origin (X, Y) in quarter units -> int32[bs, bs], or None where it is not inside."""
    H, W = img.shape
    X, Y, bs = int(X), int(Y), int(bs)
    x0, fx, y0, fy = X >> 2, X & 3, Y >> 2, Y & 3
    if x0 < 0 or y0 < 0 or x0 + bs - 1 + (fx != 0) > W - 1 or y0 + bs - 1 + (fy != 0) > H - 1:
        return None
    acc = np.full((bs, bs), 8, np.int32)
    for dy, wy in ((0, 4 - fy), (1, fy)):
        for dx, wx in ((0, 4 - fx), (1, fx)):
            if wx * wy:
                acc += (wx * wy) * img[y0 + dy:y0 + dy + bs, x0 + dx:x0 + dx + bs].astype(np.int32)
    return acc >> 4


def _norm(d, pnorm):
    d = d.astype(np.int64)
    return int(np.abs(d).sum()) if pnorm == MAE else int((d * d).sum())


def cost(previous, current, i, j, X, Y, block_size, pnorm):
    """Cost of anchor block (i, j) of ``previous`` against ``current`` displaced by (X, Y) quarter units; None where the
    displaced block is not inside."""
    bs = int(block_size)
    blk = interp_block(current, 4 * j * bs + int(X), 4 * i * bs + int(Y), bs)
    if blk is None:
        return None
    return _norm(blk - previous[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs].astype(np.int32), pnorm)


def refine(previous, current, mf, block_size, pnorm, levels=2):
    """Integer field ``mf`` int32[Hb, Wb, 2] -> (qfield int32[Hb, Wb, 2], cost int64[Hb, Wb]).  A block whose integer match
    is not inside the frame keeps 4 mf and gets cost -1."""
    previous, current = _frame(previous, "previous"), _frame(current, "current")
    if previous.shape != current.shape:
        raise ValueError("previous and current differ in shape")
    levels, pnorm, bs = int(levels), int(pnorm), int(block_size)
    if levels not in (0, 1, 2):
        raise ValueError("levels %d (0: integer, 1: half-pel, 2: quarter-pel)" % levels)
    if pnorm not in (MAE, MSE):
        raise ValueError("pnorm %d (0: MAE, 1: MSE)" % pnorm)
    mf = np.asarray(mf)
    Hb, Wb = mf.shape[:2]
    qfield = (4 * mf[:, :, :2].astype(np.int64)).astype(np.int32)
    costs = np.full((Hb, Wb), -1, np.int64)
    for i in range(Hb):
        for j in range(Wb):
            X, Y = int(qfield[i, j, 0]), int(qfield[i, j, 1])
            best = cost(previous, current, i, j, X, Y, bs, pnorm)
            if best is None:
                continue
            for step in (2, 1)[:levels]:
                cx, cy = X, Y
                for ox, oy in OFFSETS:
                    c = cost(previous, current, i, j, cx + ox * step, cy + oy * step, bs, pnorm)
                    if c is not None and c < best:
                        best, X, Y = c, cx + ox * step, cy + oy * step
            qfield[i, j] = (X, Y)
            costs[i, j] = best
    return qfield, costs


def compensate(previous, qfield, block_size):
    """``previous`` compensated by the quarter-pel field -> uint8[H, W]: block (i, j) is the interpolated block of ``previous``
    at (4 j bs - q0, 4 i bs - q1) where that block is inside; elsewhere, and beyond the last whole block, the copy."""
    previous = _frame(previous, "previous")
    bs = int(block_size)
    out = previous.copy()
    q = np.asarray(qfield)
    for i in range(min(q.shape[0], previous.shape[0] // bs)):
        for j in range(min(q.shape[1], previous.shape[1] // bs)):
            blk = interp_block(previous, 4 * j * bs - int(q[i, j, 0]), 4 * i * bs - int(q[i, j, 1]), bs)
            if blk is not None:
                out[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs] = blk
    return out


def compensate_integer(previous, mf, block_size):
    """motion.compensate_frame (motion.py:289-321) on the host: ``out[a, b] = previous[a - d1, b - d0]`` per pixel of every
    whole block where the source pixel lies in the frame, else the pixel is kept."""
    previous = _frame(previous, "previous")
    H, W = previous.shape
    bs = int(block_size)
    mf = np.asarray(mf)
    Hb, Wb = min(mf.shape[0], H // bs), min(mf.shape[1], W // bs)
    out = previous.copy()
    a, b = np.mgrid[0:Hb * bs, 0:Wb * bs]
    sa = a - np.repeat(np.repeat(mf[:Hb, :Wb, 1], bs, 0), bs, 1)
    sb = b - np.repeat(np.repeat(mf[:Hb, :Wb, 0], bs, 0), bs, 1)
    ok = (sa >= 0) & (sa < H) & (sb >= 0) & (sb < W)
    out[a[ok], b[ok]] = previous[sa[ok], sb[ok]]
    return out


def sse(a, b):
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


def psnr(sse_value, height, width):
    """utils.PSNR from an exact sum of squared errors (sequence.psnr_from_sse): -1 where the frames are equal."""
    if sse_value == 0:
        return -1.0
    return float(20.0 * np.log10(255.0 / np.sqrt(float(sse_value) / (height * width))))


def summary(mf, qfield, sse_integer, sse_qpel, height, width):
    """What the CLI reports of one pair: the field's median vector in pixels, the share of blocks the refinement moved off
    the integer vector, the PSNR of ``current`` against the integer and the quarter-pel compensation, and their difference."""
    q = np.asarray(qfield).reshape(-1, 2)
    moved = np.any(q != 4 * np.asarray(mf)[:, :, :2].reshape(-1, 2), axis=1)
    p_int, p_q = psnr(int(sse_integer), height, width), psnr(int(sse_qpel), height, width)
    return {"median_vector": [float(np.median(q[:, 0])) / 4.0, float(np.median(q[:, 1])) / 4.0] if len(q) else [0.0, 0.0],
            "moved_share": float(np.mean(moved)) if len(q) else 0.0,
            "sse_integer": int(sse_integer), "sse_qpel": int(sse_qpel),
            "psnr_integer": p_int, "psnr_qpel": p_q, "psnr_gain": p_q - p_int}


# ---- the device path --------------------------------------------------------------------------------------------------
def _levels(levels):
    levels = int(levels)
    if levels not in (0, 1, 2):
        raise ValueError("levels %d (0: integer, 1: half-pel, 2: quarter-pel)" % levels)
    return levels


def motion_field(previous, current, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, levels=2):
    """bbme.get_motion_field on the device, then the refinement on the device -> (qfield int32[Hb, Wb, 2], cost
    int64[Hb, Wb])."""
    import _gme_native as native
    import bbme
    levels = _levels(levels)
    mf = bbme.get_motion_field(previous, current, block_size, search_window, searching_procedure, pnorm_distance)
    return native.default_context().subpel(previous, current, mf, block_size, int(pnorm_distance) % 2, levels)


def report(previous, current, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, levels=2):
    """One pair on the device: integer search, refinement, both compensations -> ``summary`` plus the fields."""
    import _gme_native as native
    import motion
    levels = _levels(levels)
    previous, current = native.as_frame(previous, "previous"), native.as_frame(current, "current")
    seq = motion._pair_sequence(previous, current)
    pnorm = int(pnorm_distance) % 2
    seq.bbme(1, int(block_size), int(search_window), int(searching_procedure), pnorm)
    mf = seq.read_mv()[0]
    seq.subpel(1, int(block_size), pnorm, levels)
    qfield, costs = seq.read_qmv()
    sse_q = int(seq.compensate_qpel(1, int(block_size))[0])
    ctx = native.default_context()
    sse_i = ctx.sse(current, ctx.compensate(previous, mf)) if mf.size else sse(current, previous)
    out = summary(mf, qfield[0], sse_i, sse_q, *previous.shape)
    out.update(mf=mf, qfield=qfield[0], cost=costs[0])
    return out
