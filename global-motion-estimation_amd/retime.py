"""Frame interpolation at any phase, for rate conversion and slow motion: the host definition, in the role
interp.py plays for the halfway frame.  Pure NumPy, importable without the library; everything is integer, and the device path
(``k_retime`` and ``k_retime_frame`` of ``csrc/bbme_retime.hip`` behind ``gme_retime_u8`` and ``gme_retime_clip_u8``) computes
what ``search`` and ``interpolate`` here do, byte for byte.

* Frames: ``past`` and ``next`` are uint8[H, W], H >= B and W >= B, else ValueError; there are H // B x W // B whole blocks,
  block (i, j) with its origin at (j B, i B).
* Phase: the new frame lies at phase n / d between ``past`` (phase 0) and ``next`` (phase 1), 1 <= n < d <= 64 after
  ``check_phase`` has reduced n / d by their gcd; anything else is ValueError.
* Vector: V = (Vx, Vy), (column, row), in whole pixels, is how far content moves from ``past`` to ``next``; V in [-sw, sw]^2.
* Offsets, per component and in quarter pixels: ``a(V) = -((8 n V + d) // (2 d))`` (floor division: -4 n V / d rounded to the
  nearest quarter, halves up) and ``b(V) = a(V) + 4 V``.  The two sides always differ by exactly V, and both offsets have the
  same fractional part ``a & 3``.
* Samples, with ``obmc.sample`` (quarter positions, each of the four taps clamped to the frame, + 8 >> 4):
  P(p, V) = sample(past, 4 px + a(Vx), 4 py + a(Vy)), and N(p, V) the same on ``next`` with b.
* Cost: D(V) = sum |P - N| over the block (pnorm 0) or sum (P - N)^2 (pnorm 1); J(V) = D(V) + bias (|Vx| + |Vy|).
* Arguments: ``block_size`` 4 .. 64, ``search_window`` 0 .. 16, ``pnorm`` 0 or 1, ``bias`` 0 .. 2**16, else ValueError.  The
  largest J is 64^2 255^2 + 2**16 * 32 < 2**31.
* Search, exactly ``interp.search``'s order: the incumbent is V = (0, 0); then every (ox, oy) in [-sw, sw]^2 without the centre,
  column offset in the outer loop, both ascending; only a strictly smaller J replaces the incumbent.
* ``search`` -> ``mv`` int32[Hb, Wb, 2]; ``cost`` int64[Hb, Wb], the winner's J; ``dist`` int64[Hb, Wb], its D.
* ``interpolate``: a pixel p of a whole block is ((d - n) P(p, V) + n N(p, V) + (d >> 1)) // d with the block's V; beyond the
  last whole block V = 0, a plain cross-fade.
* ``distortion`` -> int64[H, W], the per-pixel P - N of one V: what ties this definition to interp.py in the host tests.
* ``default_bias`` is ``interp.default_bias``: a convention of the tool, not a tuned value.
* ``schedule(n_frames, step_num, step_den)``: output m = 0 .. M - 1, M = ((n_frames - 1) step_den) // step_num + 1, lies at time
  m step_num / step_den in input frames: k = (m step_num) // step_den, r = (m step_num) % step_den; r = 0 is frame k itself,
  otherwise the pair (k, k + 1) at phase r / step_den, reduced -> int32[M, 3] rows (k, n, d), n = 0 and d = 1 for a copy.  The
  step is input rate over output rate: 24 -> 60 fps is 2/5, 4x slow motion is 1/4, 60 -> 24 fps is 5/2.
"""
from math import gcd

import numpy as np

import interp
import obmc

MAE, MSE = 0, 1
MIN_BLOCK_SIZE, MAX_BLOCK_SIZE, MAX_SEARCH_WINDOW, MAX_BIAS, MAX_DENOMINATOR = 4, 64, 16, 1 << 16, 64

default_bias = interp.default_bias
check_shape = interp.check_shape
sse = interp.sse
psnr = interp.psnr


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


def check_phase(n, d):
    """The phase n / d reduced by the gcd -> (n, d) with 1 <= n < d <= 64, or ValueError."""
    n, d = int(n), int(d)
    if d < 1 or n < 1 or n >= d:
        raise ValueError("phase %d/%d (0 < n / d < 1)" % (n, d))
    g = gcd(n, d)
    n, d = n // g, d // g
    if d > MAX_DENOMINATOR:
        raise ValueError("phase %d/%d: denominator above %d" % (n, d, MAX_DENOMINATOR))
    return n, d


def offsets(V, n, d):
    """(a(V), b(V)) in quarter pixels for an int or an int array V, n / d as given (reduced or not: the value is the same)."""
    V = np.asarray(V, np.int64)
    a = -((8 * n * V + d) // (2 * d))
    return a, a + 4 * V


def _pair(past, next):
    past, nxt = np.asarray(past), np.asarray(next)
    if past.ndim != 2 or any(a.dtype != np.uint8 or a.shape != past.shape for a in (past, nxt)):
        raise TypeError("past and next must be 2-D uint8 images of one shape")
    return past, nxt


def _sides(past, nxt, V, n, d, grid):
    """(P, N) int64[H, W] of one vector; ``grid`` = (4 x, 4 y) of the frame's pixels."""
    (ax, bx), (ay, by) = offsets(V[0], n, d), offsets(V[1], n, d)
    return obmc.sample(past, grid[0] + ax, grid[1] + ay), obmc.sample(nxt, grid[0] + bx, grid[1] + by)


def _grid(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    return 4 * x, 4 * y


def distortion(past, next, V, n, d):
    """P(p, V) - N(p, V) at every pixel -> int64[H, W]."""
    past, nxt = _pair(past, next)
    n, d = check_phase(n, d)
    P, N = _sides(past, nxt, (int(V[0]), int(V[1])), n, d, _grid(*past.shape))
    return P - N


def candidates(search_window):
    """The vectors of [-sw, sw]^2 in the order of the search: the centre first, then column offset outer, both ascending."""
    sw = int(search_window)
    return [(0, 0)] + [(ox, oy) for ox in range(-sw, sw + 1) for oy in range(-sw, sw + 1) if (ox, oy) != (0, 0)]


def _columns(frame, X):
    """The horizontal half of ``obmc.sample`` at the quarter columns X int64[W], unrounded: (4 - fx) f[:, xa] + fx f[:, xb]."""
    W = frame.shape[1]
    x0, fx = X >> 2, X & 3
    return (4 - fx) * frame[:, np.clip(x0, 0, W - 1)] + fx * frame[:, np.clip(x0 + 1, 0, W - 1)]


def _rows(columns, Y):
    """The vertical half at the quarter rows Y int64[H] with the rounding: ``obmc.sample`` of the frame ``_columns`` was given."""
    H = columns.shape[0]
    y0, fy = (Y >> 2)[:, None], (Y & 3)[:, None]
    return ((4 - fy) * columns[np.clip(y0[:, 0], 0, H - 1)] + fy * columns[np.clip(y0[:, 0] + 1, 0, H - 1)] + 8) >> 4


def block_distortions(past, next, block_size, search_window, n, d):
    """D(V) of every block for every vector of ``candidates`` -> (sum |P - N|, sum (P - N)^2), each int64[(2 sw + 1)^2, Hb, Wb]:
    the part of ``search`` that depends on neither the norm nor the bias.  The four-tap sample is taken in two halves, columns
    per Vx and rows per Vy; the sum of the four weighted taps is the same integer, rounded once (``distortion`` takes it whole)."""
    bs, sw = check_args(block_size, search_window, MAE, 0)[:2]
    n, d = check_phase(n, d)
    past, nxt = _pair(past, next)
    H, W = past.shape
    check_shape(H, W, bs)
    Hb, Wb = H // bs, W // bs
    p64, n64 = past.astype(np.int64), nxt.astype(np.int64)
    x4, y4 = 4 * np.arange(Wb * bs, dtype=np.int64), 4 * np.arange(Hb * bs, dtype=np.int64)
    order = {V: c for c, V in enumerate(candidates(sw))}
    out = np.zeros((2, len(order), Hb, Wb), np.int64)
    for ox in range(-sw, sw + 1):
        ax, bx = offsets(ox, n, d)
        pc, nc = _columns(p64, x4 + ax), _columns(n64, x4 + bx)
        for oy in range(-sw, sw + 1):
            ay, by = offsets(oy, n, d)
            e = (_rows(pc, y4 + ay) - _rows(nc, y4 + by)).reshape(Hb, bs, Wb, bs)
            out[MAE, order[(ox, oy)]] = np.abs(e).sum(axis=(1, 3))
            out[MSE, order[(ox, oy)]] = (e * e).sum(axis=(1, 3))
    return out[MAE], out[MSE]


def select(D, search_window, bias):
    """The search over the distortions ``D`` int64[(2 sw + 1)^2, Hb, Wb] of one norm (``block_distortions``): the incumbent is
    the centre, only a strictly smaller J replaces it -> (mv, cost, dist)."""
    sw, bias = int(search_window), int(bias)
    dist = D[0].copy()
    cost = dist.copy()
    mv = np.zeros(D.shape[1:] + (2,), np.int32)
    for c, (ox, oy) in enumerate(candidates(sw)):
        if c == 0:
            continue
        j = D[c] + bias * (abs(ox) + abs(oy))
        better = j < cost
        cost = np.where(better, j, cost)
        dist = np.where(better, D[c], dist)
        mv[better] = (ox, oy)
    return mv, cost.astype(np.int64), dist.astype(np.int64)


def search(past, next, block_size, search_window, pnorm, bias, n, d):
    """-> (mv int32[Hb, Wb, 2], cost int64[Hb, Wb], dist int64[Hb, Wb])."""
    bs, sw, pnorm, bias = check_args(block_size, search_window, pnorm, bias)
    return select(block_distortions(past, next, bs, sw, n, d)[pnorm], sw, bias)


def interpolate(past, next, mv, block_size, n, d):
    """The frame at phase n / d between ``past`` and ``next`` under the field ``mv`` int32[H // B, W // B, 2] -> uint8[H, W]."""
    bs = int(block_size)
    n, d = check_phase(n, d)
    past, nxt = _pair(past, next)
    H, W = past.shape
    Hb, Wb = H // bs, W // bs
    mv = np.asarray(mv)
    if mv.ndim != 3 or mv.shape[:2] != (Hb, Wb) or mv.shape[2] < 2:
        raise ValueError("the field of a %d x %d frame at block size %d is %r, not %r" % (H, W, bs, (Hb, Wb, 2), mv.shape))
    V = np.zeros((2, H, W), np.int64)
    for c in (0, 1):
        V[c, :Hb * bs, :Wb * bs] = np.repeat(np.repeat(mv[:, :, c], bs, axis=0), bs, axis=1)
    P, N = _sides(past, nxt, V, n, d, _grid(H, W))
    return (((d - n) * P + n * N + (d >> 1)) // d).astype(np.uint8)


def crossfade(past, next, n, d):
    """The rounded plain blend of the two frames at phase n / d: what ``interpolate`` gives under the zero field."""
    past, nxt = _pair(past, next)
    n, d = check_phase(n, d)
    return (((d - n) * past.astype(np.int64) + n * nxt.astype(np.int64) + (d >> 1)) // d).astype(np.uint8)


def schedule(n_frames, step_num, step_den):
    """The outputs of a clip of ``n_frames`` frames at a step of step_num / step_den input frames -> int32[M, 3] rows (k, n, d):
    frame k itself (n = 0, d = 1) or the pair (k, k + 1) at the reduced phase n / d."""
    N, num, den = int(n_frames), int(step_num), int(step_den)
    if N < 1 or num < 1 or den < 1:
        raise ValueError("schedule of %d frames at step %d/%d" % (N, num, den))
    M = ((N - 1) * den) // num + 1
    rows = np.zeros((M, 3), np.int32)
    for m in range(M):
        k, r = divmod(m * num, den)
        rows[m] = (k, 0, 1) if r == 0 else (k,) + check_phase(r, den)
    return rows


def rate_step(rate_in, rate_out):
    """The step of a conversion from ``rate_in`` to ``rate_out`` frames per second (integers) -> (num, den), reduced."""
    a, b = int(rate_in), int(rate_out)
    if a < 1 or b < 1 or a != rate_in or b != rate_out:
        raise ValueError("rates %r -> %r: positive integers" % (rate_in, rate_out))
    g = gcd(a, b)
    return a // g, b // g


def summary(mv, height, width, sse_made=None, sse_crossfade=None):
    """What the CLI reports of one made frame: the median vector, the share of non-zero vectors and, where there is a true
    frame at that time, SSE and PSNR of the made frame and of the plain cross-fade against it."""
    out = interp.summary(mv, height, width)
    for name, s in (("retime", sse_made), ("crossfade", sse_crossfade)):
        if s is not None:
            out["sse_" + name] = int(s)
            out["psnr_" + name] = psnr(int(s), height, width)
    return out


# ---- the device path --------------------------------------------------------------------------------------------------
def _device_args(block_size, search_window, pnorm_distance, bias):
    pnorm = int(pnorm_distance) % 2
    bias = default_bias(block_size, pnorm) if bias is None else bias
    return check_args(block_size, search_window, pnorm, bias)


def motion_field(past, next, n=1, d=2, block_size=16, search_window=16, pnorm_distance=0, bias=None):
    """``search`` on the device (gme_retime_u8) -> (mv, cost, dist)."""
    import _gme_native as native
    bs, sw, pnorm, bias = _device_args(block_size, search_window, pnorm_distance, bias)
    return native.default_context().retime(past, next, bs, sw, pnorm, bias, n, d)[:3]


def frame(past, next, n=1, d=2, block_size=16, search_window=16, pnorm_distance=0, bias=None):
    """``interpolate`` of ``search`` on the device (gme_retime_u8) -> uint8[H, W]."""
    import _gme_native as native
    bs, sw, pnorm, bias = _device_args(block_size, search_window, pnorm_distance, bias)
    return native.default_context().retime(past, next, bs, sw, pnorm, bias, n, d)[3]


def report(past, next, n=1, d=2, truth=None, block_size=16, search_window=16, pnorm_distance=0, bias=None):
    """One pair on the device (gme_retime_u8): ``summary`` plus the field, its costs, the made frame, the bias and the reduced
    phase.  With ``truth``, the true frame at that time, the squared error of the made frame is the device's and that of the
    plain cross-fade is computed here."""
    import _gme_native as native
    bs, sw, pnorm, bias = _device_args(block_size, search_window, pnorm_distance, bias)
    n, d = check_phase(n, d)
    mv, cost, dist, made, err = native.default_context().retime(past, next, bs, sw, pnorm, bias, n, d, truth=truth)
    H, W = made.shape
    out = summary(mv, H, W, None if truth is None else err, None if truth is None else sse(crossfade(past, next, n, d), truth))
    out.update(mv=mv, cost=cost, dist=dist, frame=made, bias=bias, phase=[n, d])
    return out


def retime_clip(frames, step, block_size=16, search_window=16, pnorm_distance=0, bias=None, first=0, count=None):
    """Outputs first .. first + count - 1 of ``schedule`` on the device (gme_retime_clip_u8) -> (frames uint8[count, H, W], mv
    int32[count, h, w, 2], cost and dist int64[count, h, w])."""
    import _gme_native as native
    bs, sw, pnorm, bias = _device_args(block_size, search_window, pnorm_distance, bias)
    return native.default_context().retime_clip(frames, bs, sw, pnorm, bias, step=step, first=first, count=count)


def convert(frames, rate_in, rate_out, block_size=16, search_window=16, pnorm_distance=0, bias=None):
    """Frame-rate conversion of uint8[N, H, W] from ``rate_in`` to ``rate_out`` frames per second -> uint8[M, H, W], the
    outputs of ``schedule`` at the step rate_in / rate_out."""
    return retime_clip(frames, rate_step(rate_in, rate_out), block_size, search_window, pnorm_distance, bias)[0]


def slow_motion(frames, factor, block_size=16, search_window=16, pnorm_distance=0, bias=None):
    """``factor`` times slow motion of uint8[N, H, W] -> uint8[(N - 1) factor + 1, H, W]: the step 1 / factor."""
    factor = int(factor)
    if factor < 1:
        raise ValueError("slow-motion factor %d" % factor)
    return retime_clip(frames, (1, factor), block_size, search_window, pnorm_distance, bias)[0]
