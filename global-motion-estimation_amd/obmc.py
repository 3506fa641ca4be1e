"""Overlapped block motion compensation: the host definition, in the role subpel.py and interp.py play for their
features.  Pure NumPy, importable without the library; everything is integer, and the device path (``k_obmc`` of
``csrc/bbme_obmc.hip`` behind ``gme_obmc_u8`` and ``gme_seq_obmc``) computes what ``compensate`` here does, byte for byte.

* Inputs: ``previous`` is uint8[H, W]; the field is int32[Hb, Wb, 2] with Hb = H // B and Wb = W // B exactly (else ValueError),
  component 0 the column and component 1 the row, sign and axes subpel.py's.  A quarter field is in units of 1/4 pixel; an integer
  field ``mf`` is the quarter field ``4 * mf`` (formed in 64 bits).  ``block_size`` B in 4 .. 64, H >= B and W >= B, else
  ValueError.
* Sample: P(X, Y) of ``previous`` at the quarter position (X, Y), both 64-bit: x0 = X >> 2, fx = X & 3, y0 = Y >> 2, fy = Y & 3
  (floor semantics); P = ((4-fx)(4-fy) S(y0, x0) + fx (4-fy) S(y0, x0+1) + (4-fx) fy S(y0+1, x0) + fx fy S(y0+1, x0+1) + 8) >> 4 with
  S(y, x) = previous[clamp(y, 0, H-1), clamp(x, 0, W-1)].  This is subpel.interp_block's blend with its block-inside rule replaced
  by the clamp per pixel: the border is replicated, no sample is ever unavailable, and any int32 vector is valid.
* Window: output pixel (u, v), u < Wb B and v < Hb B, lies in block i = v // B, j = u // B at ty = 2 (v - i B) + 1 - B and
  tx = 2 (u - j B) + 1 - B.  The vertical neighbour is i2 = clamp(i + (-1 if ty < 0 else 1), 0, Hb - 1), likewise j2 from tx: a
  neighbour outside the grid is the block itself.  The rows (i, i2) weigh wy = (2B - |ty|, |ty|), the columns (j, j2)
  wx = (2B - |tx|, |tx|); the four products sum to 4 B^2.  For odd B the centre row and column give the neighbour weight 0.
* Pixel: out[v, u] = (sum_{a,b} wy[a] wx[b] P(4u - q[ia, jb, 0], 4v - q[ia, jb, 1]) + 2 B^2) // (4 B^2): each of the four
  predictions is rounded to 8 bits first, then they are blended.  The largest numerator is 255 * 4 * 64^2 + 2 * 64^2 < 2^22.
  Beyond the last whole block the pixel is the copy of ``previous``, as in every other compensation here.
* ``reciprocal`` and ``divide``: the division by 4 B^2 as the device does it, M = ceil(2^37 / (4 B^2)) and (n M) >> 37, exact
  for every numerator there is (tests/test_obmc_host.py checks all of them).
"""
import numpy as np

MIN_BLOCK_SIZE, MAX_BLOCK_SIZE = 4, 64
MAX_INTEGER_VECTOR = 1 << 29       # |component| of an integer field at the device's Python interface


def check_block_size(block_size):
    bs = int(block_size)
    if not MIN_BLOCK_SIZE <= bs <= MAX_BLOCK_SIZE:
        raise ValueError("block_size %d (%d .. %d)" % (bs, MIN_BLOCK_SIZE, MAX_BLOCK_SIZE))
    return bs


def check_shape(H, W, block_size):
    """H >= B and W >= B, or ValueError."""
    if H < block_size or W < block_size:
        raise ValueError("a %d x %d frame holds no block of %d" % (H, W, block_size))


def check_field(field, H, W, block_size):
    """The field of an H x W frame as an integer array of exactly (H // B, W // B, 2), or ValueError."""
    field = np.asarray(field)
    want = (H // block_size, W // block_size, 2)
    if field.shape != want or field.dtype.kind not in "iu":
        raise ValueError("the field of a %d x %d frame at block size %d is integer%r, not %s%r"
                         % (H, W, block_size, want, field.dtype, field.shape))
    return field


def _frame(a, name):
    a = np.asarray(a)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise TypeError("%s must be a 2-D uint8 image" % name)
    return a


def reciprocal(block_size):
    """M = ceil(2^37 / (4 B^2)): fits 32 bits for B >= 4."""
    area = 4 * int(block_size) * int(block_size)
    return ((1 << 37) + area - 1) // area


def divide(n, m):
    """n // (4 B^2) by the reciprocal m: the high word of the 32 x 32 bit product, shifted right by 5."""
    return ((n * m) >> 32) >> 5


def weights(block_size):
    """The window of one block -> int64[2, 2, B, B]: [a, b, y, x] = wy[a] wx[b] at the pixel (x, y) of the block, a and b 0 for
    the block's own row or column and 1 for the neighbour's.  Sums to 4 B^2 over a and b at every pixel."""
    bs = int(block_size)
    t = np.abs(2 * np.arange(bs, dtype=np.int64) + 1 - bs)
    w = np.stack([2 * bs - t, t])
    return w[:, None, :, None] * w[None, :, None, :]


def sample(previous, X, Y):
    """P(X, Y) for int64 arrays of quarter positions -> int64 of their shape."""
    H, W = previous.shape
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    x0, fx, y0, fy = X >> 2, X & 3, Y >> 2, Y & 3
    # x0 + 1 in 64 bits cannot wrap: |X| <= 2^33 + 4 W
    xa, xb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    ya, yb = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    p = previous.astype(np.int64)
    return ((4 - fx) * (4 - fy) * p[ya, xa] + fx * (4 - fy) * p[ya, xb] + (4 - fx) * fy * p[yb, xa] + fx * fy * p[yb, xb] + 8) >> 4


def compensate(previous, field, block_size, quarter=True):
    """``previous`` compensated by the field with overlapped blocks -> uint8[H, W].  ``quarter``: the field is in quarter pixels;
    else in whole pixels."""
    previous = _frame(previous, "previous")
    bs = check_block_size(block_size)
    H, W = previous.shape
    check_shape(H, W, bs)
    q = check_field(field, H, W, bs).astype(np.int64) * (1 if quarter else 4)
    Hb, Wb = H // bs, W // bs
    out = previous.copy()
    v, u = np.mgrid[0:Hb * bs, 0:Wb * bs].astype(np.int64)
    i, j = v // bs, u // bs
    ty, tx = 2 * (v - i * bs) + 1 - bs, 2 * (u - j * bs) + 1 - bs
    i2 = np.clip(i + np.where(ty < 0, -1, 1), 0, Hb - 1)
    j2 = np.clip(j + np.where(tx < 0, -1, 1), 0, Wb - 1)
    wy, wx = (2 * bs - np.abs(ty), np.abs(ty)), (2 * bs - np.abs(tx), np.abs(tx))
    acc = np.full(v.shape, 2 * bs * bs, np.int64)
    for a, ia in enumerate((i, i2)):
        for b, jb in enumerate((j, j2)):
            acc += wy[a] * wx[b] * sample(previous, 4 * u - q[ia, jb, 0], 4 * v - q[ia, jb, 1])
    out[:Hb * bs, :Wb * bs] = acc // (4 * bs * bs)
    return out


def sse(a, b):
    """Exact sum of squared differences of two uint8 images."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


def psnr(sse_value, height, width):
    """subpel.psnr: utils.PSNR from an exact sum of squared errors, -1 where the frames are equal."""
    if sse_value == 0:
        return -1.0
    return float(20.0 * np.log10(255.0 / np.sqrt(float(sse_value) / (height * width))))


def summary(sse_plain, sse_obmc, height, width):
    """What the CLI reports of one field of one pair: squared error and PSNR of ``current`` against the plain and against the
    overlapped compensation, and the gain."""
    p_plain, p_obmc = psnr(int(sse_plain), height, width), psnr(int(sse_obmc), height, width)
    return {"sse_plain": int(sse_plain), "sse_obmc": int(sse_obmc), "psnr_plain": p_plain, "psnr_obmc": p_obmc,
            "psnr_gain": p_obmc - p_plain}


# ---- the device path --------------------------------------------------------------------------------------------------
def frame(previous, field, block_size=16, quarter=True):
    """``compensate`` on the device (gme_obmc_u8) -> uint8[H, W]."""
    import _gme_native as native
    return native.default_context().obmc(previous, field, block_size, quarter)[0]


def report(previous, current, block_size=16, search_window=16, searching_procedure=0, pnorm_distance=0, levels=0, hier=False):
    """One pair on the device: the integer search (hierarchical if ``hier``, with search_window as its coarse window), with
    ``levels`` above 0 the sub-pel refinement, then the plain and the overlapped compensation of each field -> {"integer": summary,
    "qpel": summary (levels > 0), "mf", "qfield" (levels > 0), "frame": the overlapped compensation by the finest field}."""
    import _gme_native as native
    import motion
    levels = int(levels)
    if levels not in (0, 1, 2):
        raise ValueError("levels %d (0: integer, 1: half-pel, 2: quarter-pel)" % levels)
    bs = check_block_size(block_size)
    previous, current = native.as_frame(previous, "previous"), native.as_frame(current, "current")
    check_shape(previous.shape[0], previous.shape[1], bs)
    H, W = previous.shape
    pnorm = int(pnorm_distance) % 2
    ctx = native.default_context()
    seq = motion._pair_sequence(previous, current)
    if hier:
        seq.hier(1, bs, int(search_window), 1, pnorm, 3)
    else:
        seq.bbme(1, bs, int(search_window), int(searching_procedure), pnorm)
    mf = seq.read_mv()[0]
    frames, err = seq.obmc(1, bs, quarter=False)
    out = {"integer": summary(ctx.sse(current, ctx.compensate(previous, mf)), err[0], H, W), "mf": mf, "frame": frames[0]}
    if levels:
        seq.subpel(1, bs, pnorm, levels)
        out["qfield"] = seq.read_qmv()[0][0]
        sse_plain = int(seq.compensate_qpel(1, bs)[0])
        frames, err = seq.obmc(1, bs, quarter=True)
        out["qpel"] = summary(sse_plain, err[0], H, W)
        out["frame"] = frames[0]
    return out
