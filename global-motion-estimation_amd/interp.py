"""Motion-compensated frame interpolation: the host definition, in the role bipred.py plays for bidirectional
prediction.  Pure NumPy, importable without the library; everything is integer, and the device path (``k_interp`` and
``k_interp_frame`` of ``csrc/bbme_interp.hip`` behind ``gme_interp_u8`` and ``gme_seq_interp``) computes what ``search`` and
``interpolate`` here do, byte for byte.

* Frames: ``past`` and ``next`` are uint8[H, W]; the frame being made lies halfway between them and exists nowhere, so there is
  no target block to match against.  ``S(f, x, y) = f[clamp(y, 0, H - 1), clamp(x, 0, W - 1)]``: the border is replicated, and no
  candidate is ever unavailable.  Block (i, j) of the new frame has its origin at (j B, i B); there are H // B x W // B whole
  blocks; H >= B and W >= B, else ValueError.
* Vector: v = (vx, vy), (column, row).  The block is ``past`` at origin - v and ``next`` at origin + v: content moves by 2 v
  between the two frames.  D(v) = sum |S(past, p - v) - S(next, p + v)| (or the sum of the squares) over the block's pixels p,
  and J(v) = D(v) + bias * (|vx| + |vy|).
* Arguments: ``block_size`` B in 4 .. 64, ``search_window`` sw in 0 .. 8, ``pnorm`` 0 (sum |d|) or 1 (sum d^2), ``bias`` in
  0 .. 2**16, else ValueError.  Every J stays below 2**31 (the largest: 64 * 64 * 255^2 + 2**16 * 16).
* Search: the incumbent is v = (0, 0); then every (ox, oy) in [-sw, sw]^2 without the centre, column offset in the outer loop,
  both ascending; only a strictly smaller J replaces the incumbent.
* ``search`` -> ``mv`` int32[Hb, Wb, 2]; ``cost`` int64[Hb, Wb], the winner's J; ``dist`` int64[Hb, Wb], its D.
* ``interpolate``: a pixel p of a whole block is (S(past, p - v) + S(next, p + v) + 1) >> 1 with the block's v; a pixel beyond
  the last whole block is the same expression with v = 0.
* ``default_bias``: B^2 / 16 for MAE and B^2 for MSE, a sixteenth of a grey level (squared) per pixel and unit of |v|: a
  convention of the tool, not a tuned value.
"""
import numpy as np

MAE, MSE = 0, 1
MIN_BLOCK_SIZE, MAX_BLOCK_SIZE, MAX_SEARCH_WINDOW, MAX_BIAS = 4, 64, 8, 1 << 16


def check_args(block_size, search_window, pnorm, bias):
    """The argument rules of the definition -> (block_size, search_window, pnorm, bias) as ints, or ValueError."""
    bs, sw, pnorm, bias = int(block_size), int(search_window), int(pnorm), int(bias)
    if not MIN_BLOCK_SIZE <= bs <= MAX_BLOCK_SIZE:
        raise ValueError("block_size %d (%d .. %d)" % (bs, MIN_BLOCK_SIZE, MAX_BLOCK_SIZE))
    if not 0 <= sw <= MAX_SEARCH_WINDOW:
        raise ValueError("search_window %d (0 .. %d)" % (sw, MAX_SEARCH_WINDOW))
    if pnorm not in (MAE, MSE):
        raise ValueError("pnorm %d (0: MAE, 1: MSE)" % pnorm)
    if not 0 <= bias <= MAX_BIAS:
        raise ValueError("bias %d (0 .. 2**16)" % bias)
    return bs, sw, pnorm, bias


def default_bias(block_size, pnorm):
    """The CLI's convention, not a tuned value: B^2 / 16 for MAE and B^2 for MSE."""
    bs = int(block_size)
    return bs * bs // 16 if int(pnorm) == MAE else bs * bs


def check_shape(H, W, block_size):
    """H >= B and W >= B, or ValueError."""
    if H < block_size or W < block_size:
        raise ValueError("a %d x %d frame holds no block of %d" % (H, W, block_size))


def _pair(past, next):
    past, nxt = np.asarray(past), np.asarray(next)
    if past.ndim != 2 or any(a.dtype != np.uint8 or a.shape != past.shape for a in (past, nxt)):
        raise TypeError("past and next must be 2-D uint8 images of one shape")
    return past, nxt


def _shifted(padded, m, H, W, dx, dy):
    """S(f, x + dx, y + dy) over the frame, |dx|, |dy| <= m, from f padded by m replicated pixels -> int64[H, W]."""
    return padded[m + dy:m + dy + H, m + dx:m + dx + W]


def search(past, next, block_size, search_window, pnorm, bias):
    """-> (mv int32[Hb, Wb, 2], cost int64[Hb, Wb], dist int64[Hb, Wb])."""
    bs, sw, pnorm, bias = check_args(block_size, search_window, pnorm, bias)
    past, nxt = _pair(past, next)
    H, W = past.shape
    check_shape(H, W, bs)
    Hb, Wb = H // bs, W // bs
    pp = np.pad(past.astype(np.int64), sw, mode="edge")
    nn = np.pad(nxt.astype(np.int64), sw, mode="edge")

    def D(vx, vy):
        d = _shifted(pp, sw, H, W, -vx, -vy) - _shifted(nn, sw, H, W, vx, vy)
        d = np.abs(d) if pnorm == MAE else d * d
        return d[:Hb * bs, :Wb * bs].reshape(Hb, bs, Wb, bs).sum(axis=(1, 3))

    dist = D(0, 0)
    cost = dist.copy()
    mv = np.zeros((Hb, Wb, 2), np.int32)
    for ox in range(-sw, sw + 1):
        for oy in range(-sw, sw + 1):
            if (ox, oy) == (0, 0):
                continue
            d = D(ox, oy)
            j = d + bias * (abs(ox) + abs(oy))
            better = j < cost
            cost = np.where(better, j, cost)
            dist = np.where(better, d, dist)
            mv[better] = (ox, oy)
    return mv, cost.astype(np.int64), dist.astype(np.int64)


def interpolate(past, next, mv, block_size):
    """The frame halfway between ``past`` and ``next`` under the field ``mv`` int32[H // B, W // B, 2] -> uint8[H, W]."""
    bs = int(block_size)
    past, nxt = _pair(past, next)
    H, W = past.shape
    Hb, Wb = H // bs, W // bs
    mv = np.asarray(mv)
    if mv.ndim != 3 or mv.shape[:2] != (Hb, Wb) or mv.shape[2] < 2:
        raise ValueError("the field of a %d x %d frame at block size %d is %r, not %r" % (H, W, bs, (Hb, Wb, 2), mv.shape))
    vx, vy = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    vx[:Hb * bs, :Wb * bs] = np.repeat(np.repeat(mv[:, :, 0], bs, axis=0), bs, axis=1)
    vy[:Hb * bs, :Wb * bs] = np.repeat(np.repeat(mv[:, :, 1], bs, axis=0), bs, axis=1)
    y, x = np.mgrid[0:H, 0:W]
    p = past[np.clip(y - vy, 0, H - 1), np.clip(x - vx, 0, W - 1)].astype(np.int64)
    n = nxt[np.clip(y + vy, 0, H - 1), np.clip(x + vx, 0, W - 1)].astype(np.int64)
    return ((p + n + 1) >> 1).astype(np.uint8)


def average(past, next):
    """The rounded plain average of the two frames: what ``interpolate`` gives under the zero field."""
    past, nxt = _pair(past, next)
    return ((past.astype(np.int64) + nxt.astype(np.int64) + 1) >> 1).astype(np.uint8)


def sse(a, b):
    """Exact sum of squared differences of two uint8 images."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


def psnr(sse_value, height, width):
    """PSNR in dB of a squared error over a height x width frame (inf at 0)."""
    if sse_value <= 0:
        return float("inf")
    return float(10.0 * np.log10(255.0 * 255.0 * height * width / float(sse_value)))


def summary(mv, height, width, sse_interp=None, sse_average=None):
    """What the CLI reports of one pair: the median vector, the share of non-zero vectors and, where there is a true middle
    frame, SSE and PSNR of the interpolation and of the plain average against it."""
    mv = np.asarray(mv).reshape(-1, 2)
    out = {"median_vector": [float(np.median(mv[:, 0])), float(np.median(mv[:, 1]))] if len(mv) else [0.0, 0.0],
           "nonzero_share": float(np.any(mv != 0, axis=1).mean()) if len(mv) else 0.0}
    for name, s in (("interp", sse_interp), ("average", sse_average)):
        if s is not None:
            out["sse_" + name] = int(s)
            out["psnr_" + name] = psnr(int(s), height, width)
    return out


# ---- the device path --------------------------------------------------------------------------------------------------
def _device_args(block_size, search_window, pnorm_distance, bias):
    pnorm = int(pnorm_distance) % 2
    bias = default_bias(block_size, pnorm) if bias is None else bias
    return check_args(block_size, search_window, pnorm, bias)


def motion_field(past, next, block_size=16, search_window=8, pnorm_distance=0, bias=None):
    """``search`` on the device (gme_interp_u8) -> (mv, cost, dist)."""
    import _gme_native as native
    bs, sw, pnorm, bias = _device_args(block_size, search_window, pnorm_distance, bias)
    return native.default_context().interp(past, next, bs, sw, pnorm, bias)[:3]


def frame(past, next, block_size=16, search_window=8, pnorm_distance=0, bias=None):
    """``interpolate`` of ``search`` on the device (gme_interp_u8) -> uint8[H, W]."""
    import _gme_native as native
    bs, sw, pnorm, bias = _device_args(block_size, search_window, pnorm_distance, bias)
    return native.default_context().interp(past, next, bs, sw, pnorm, bias)[3]


def _interp_sequence(frames, frame_distance, bs, sw, pnorm, bias):
    """Sequence.interp over every pair of ``frames`` (a resident sequence made for the call) -> (mv, cost, dist, frames, sse)."""
    import _gme_native as native
    seq = native.Sequence.from_frames(native.default_context(), frames)
    try:
        return seq.interp(frame_distance, bs, sw, pnorm, bias)
    finally:
        seq.close()


def upconvert(frames, block_size=16, search_window=8, pnorm_distance=0, bias=None):
    """Frame-rate doubling: uint8[2 N - 1, H, W] with the originals at the even indices and between each two neighbours the
    frame interpolated from them, from one Sequence.interp(1, ...)."""
    frames = np.ascontiguousarray(frames)
    if frames.ndim != 3 or frames.dtype != np.uint8 or len(frames) < 1:
        raise TypeError("frames must be uint8[N, H, W], N >= 1")
    bs, sw, pnorm, bias = _device_args(block_size, search_window, pnorm_distance, bias)
    check_shape(frames.shape[1], frames.shape[2], bs)
    out = np.empty((2 * len(frames) - 1,) + frames.shape[1:], np.uint8)
    out[0::2] = frames
    if len(frames) > 1:
        out[1::2] = _interp_sequence(frames, 1, bs, sw, pnorm, bias)[3]
    return out


def report(past, next, truth=None, block_size=16, search_window=8, pnorm_distance=0, bias=None):
    """One pair on the device (gme_interp_u8): ``summary`` plus the field, its costs, the interpolated frame and the bias.  With
    ``truth``, the true middle frame, the squared error of the interpolation is the device's and that of the plain average is
    computed here."""
    import _gme_native as native
    bs, sw, pnorm, bias = _device_args(block_size, search_window, pnorm_distance, bias)
    mv, cost, dist, made, err = native.default_context().interp(past, next, bs, sw, pnorm, bias, truth=truth)
    H, W = made.shape
    out = summary(mv, H, W, None if truth is None else err, None if truth is None else sse(average(past, next), truth))
    out.update(mv=mv, cost=cost, dist=dist, frame=made, bias=bias)
    return out
