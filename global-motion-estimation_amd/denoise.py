"""Motion-compensated temporal denoising: the host definition, in the role obmc.py and interp.py play for their
features.  Pure NumPy, importable without the library; everything is integer (int64 throughout), and the device path
(``k_denoise`` of ``csrc/bbme_denoise.hip`` behind ``gme_denoise_u8`` and ``gme_seq_denoise``) computes what ``blend`` and
``frame`` here do, byte for byte.

* Inputs of ``blend``: ``current`` c uint8[H, W]; ``predictions`` p_1 .. p_R uint8[H, W], 1 <= R <= 4; ``strength`` s in
  1 .. 64 grey levels, S = 9 s.  Anything else is a ValueError.
* Window: D_r(v, u) = sum over a, b in {-1, 0, 1} of |p_r(v+a, u+b) - c(v+a, u+b)| with both coordinates clamped into the frame:
  the border is replicated, neither plane is read outside.  D_r lies in 0 .. 2295.
* Weight: w_r = max(0, S - D_r): zero where the mean absolute difference over the 3 x 3 window reaches ``strength``.  The current
  pixel always weighs S.
* Pixel: tot = S + sum w_r, n = S c + sum w_r p_r, out = (n + tot // 2) // tot; tot <= 5 * 576 = 2880 and n + tot // 2 < 2^20.
  Where every w_r is 0, and where every prediction equals ``current``, the output is ``current``; the order of the references
  does not matter.
* ``frame``: ``blend`` over one overlapped prediction per reference (obmc.py).  Field r is int32[H // B, W // B, 2] on the block
  grid of ``current``: block (i, j) of ``current`` is found in ``ref_r`` displaced by field_r[i, j] (column, row), which is what
  ``bbme.get_motion_field(current, ref_r, ...)`` returns and what bipred.py calls f0 and f1.  ``obmc.compensate`` subtracts a
  vector from the output position (its vectors say where a block of the reference went), so the prediction of ``current`` is
  ``obmc.compensate(ref_r, -field_r, B, quarter)`` with the negation formed in 64 bits: pixel (u, v) reads ``ref_r`` at
  (4 u + q0, 4 v + q1) quarter pixels, every tap clamped, so any int32 vector is valid.
* ``reciprocal`` and ``divide``: the division by tot as a device may do it, M = ceil(2^32 / tot) and (n M) >> 32, exact for
  every tot in 9 .. 2880 and every numerator there is (tests/test_denoise_host.py walks them).
* The default strength 24 is a convention of this tool, not a tuned value.
"""
import numpy as np

import obmc

MIN_REFS, MAX_REFS = 1, 4
MIN_STRENGTH, MAX_STRENGTH = 1, 64
MIN_RADIUS, MAX_RADIUS = 1, 2
DEFAULT_STRENGTH = 24              # a convention of the tool, not a tuned value
WINDOW = 9                         # pixels of the 3 x 3 window


def check_args(refs, strength):
    """R in 1 .. 4 and strength in 1 .. 64, or ValueError -> (R, strength)."""
    refs, strength = int(refs), int(strength)
    if not MIN_REFS <= refs <= MAX_REFS:
        raise ValueError("%d references (%d .. %d)" % (refs, MIN_REFS, MAX_REFS))
    if not MIN_STRENGTH <= strength <= MAX_STRENGTH:
        raise ValueError("strength %d (%d .. %d)" % (strength, MIN_STRENGTH, MAX_STRENGTH))
    return refs, strength


def check_radius(radius):
    radius = int(radius)
    if not MIN_RADIUS <= radius <= MAX_RADIUS:
        raise ValueError("radius %d (%d .. %d)" % (radius, MIN_RADIUS, MAX_RADIUS))
    return radius


def reciprocal(tot):
    """M = ceil(2^32 / tot): fits 32 bits for tot >= 9 (any tot >= 2)."""
    tot = int(tot)
    return ((1 << 32) + tot - 1) // tot


def divide(n, m):
    """n // tot by the reciprocal m of tot: the high word of the 32 x 32 bit product."""
    return (n * m) >> 32


def window_sad(a, b):
    """D of two uint8[H, W] planes -> int64[H, W]: the sum of |a - b| over the 3 x 3 window, the border replicated."""
    d = np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64))
    d = np.pad(d, 1, mode="edge")
    H, W = d.shape[0] - 2, d.shape[1] - 2
    return sum(d[1 + a_:1 + a_ + H, 1 + b_:1 + b_ + W] for a_ in (-1, 0, 1) for b_ in (-1, 0, 1))


def blend(current, predictions, strength=DEFAULT_STRENGTH):
    """The filter of one frame -> uint8[H, W]."""
    current = obmc._frame(current, "current")
    predictions = [obmc._frame(p, "prediction") for p in predictions]
    _, strength = check_args(len(predictions), strength)
    if any(p.shape != current.shape for p in predictions):
        raise ValueError("the predictions differ in shape from the current frame")
    S = WINDOW * strength
    c = current.astype(np.int64)
    tot = np.full(c.shape, S, np.int64)
    n = S * c
    for p in predictions:
        w = np.maximum(0, S - window_sad(p, current))
        tot += w
        n += w * p.astype(np.int64)
    return ((n + tot // 2) // tot).astype(np.uint8)


def predict(ref, field, block_size=16, quarter=False):
    """The overlapped prediction of the current frame from ``ref`` by a field anchored at the current frame -> uint8[H, W]."""
    ref = obmc._frame(ref, "reference")
    bs = obmc.check_block_size(block_size)
    obmc.check_shape(ref.shape[0], ref.shape[1], bs)
    field = obmc.check_field(field, ref.shape[0], ref.shape[1], bs)
    return obmc.compensate(ref, -field.astype(np.int64), bs, quarter)


def frame(current, refs, fields, block_size=16, quarter=False, strength=DEFAULT_STRENGTH):
    """``blend`` over ``predict`` of each reference -> uint8[H, W]: the definition of gme_denoise_u8 (Context.denoise)."""
    refs, fields = list(refs), list(fields)
    check_args(len(refs), strength)
    if len(fields) != len(refs):
        raise ValueError("%d references, %d fields" % (len(refs), len(fields)))
    return blend(current, [predict(r, f, block_size, quarter) for r, f in zip(refs, fields)], strength)


def references(t, n_frames, frame_distance=1, radius=1):
    """The frames a target t of a clip of n_frames is filtered with: t -+ d fd, d = 1 .. radius, those that exist, in the order
    (t - fd, t + fd, t - 2 fd, t + 2 fd)."""
    out = []
    for d in range(1, radius + 1):
        for k in (t - d * frame_distance, t + d * frame_distance):
            if 0 <= k < n_frames:
                out.append(k)
    return out


sse, psnr = obmc.sse, obmc.psnr


# ---- the device path --------------------------------------------------------------------------------------------------
def _field(ctx, target, ref, block_size, search_window, procedure, pnorm, levels):
    """The field of one reference of one target on the device -> (field, quarter)."""
    mf = ctx.bbme(target, ref, block_size, search_window, procedure, pnorm)
    if levels:
        return ctx.subpel(target, ref, mf, block_size, pnorm, levels)[0], True
    return mf, False


def clip(frames, frame_distance=1, block_size=16, search_window=8, searching_procedure=0, pnorm_distance=0, radius=1, levels=0,
         strength=DEFAULT_STRENGTH):
    """Every frame of a clip uint8[N, H, W] filtered -> uint8[N, H, W].  An interior target t uses the references t -+ d fd,
    d = 1 .. radius (Sequence.denoise); near the ends a target uses the references that exist, at least one (Context.denoise).
    The fields come from the named search with the target as the anchor, refined by subpel with ``levels`` 1 or 2."""
    import _gme_native as native
    frames = np.asarray(frames)
    if frames.ndim != 3 or frames.dtype != np.uint8:
        raise TypeError("frames must be uint8[N, H, W]")
    fd, radius = int(frame_distance), check_radius(radius)
    levels = int(levels)
    if levels not in (0, 1, 2):
        raise ValueError("levels %d (0: integer, 1: half-pel, 2: quarter-pel)" % levels)
    _, strength = check_args(1, strength)
    bs = obmc.check_block_size(block_size)
    N, H, W = frames.shape
    obmc.check_shape(H, W, bs)
    if fd < 1 or N < 2 * fd:                # with fewer, a frame in the middle has no reference on either side
        raise ValueError("frame_distance %d needs at least %d frames" % (fd, 2 * max(fd, 1)))
    pnorm = int(pnorm_distance) % 2
    ctx = native.default_context()
    out = np.empty_like(frames)
    reach = radius * fd
    interior = range(reach, N - reach)
    if len(interior):
        seq = native.Sequence.from_frames(ctx, frames)
        try:
            out[reach:N - reach] = seq.denoise(fd, bs, int(search_window), int(searching_procedure), pnorm, radius, levels, strength)[0]
        finally:
            seq.close()
    for t in range(N):
        if t in interior:
            continue
        refs = references(t, N, fd, radius)
        made = [_field(ctx, frames[t], frames[k], bs, int(search_window), int(searching_procedure), pnorm, levels) for k in refs]
        out[t] = ctx.denoise(frames[t], [frames[k] for k in refs], [f for f, _ in made], bs, bool(levels), strength)[0]
    return out


def report(frames, clean=None, **options):
    """What the CLI prints of a clip: ``clip`` of the frames -> {"frames": the filtered clip, "change": per frame the squared
    difference between the filtered and the given frame, and with ``clean`` "sse_noisy", "sse_filtered" (per frame, against the
    clean clip), "psnr_noisy" and "psnr_filtered" (of the whole clip)}."""
    frames = np.asarray(frames)
    made = clip(frames, **options)
    out = {"frames": made, "change": [sse(a, b) for a, b in zip(made, frames)]}
    if clean is not None:
        N, H, W = frames.shape
        out["sse_noisy"] = [sse(a, b) for a, b in zip(frames, clean)]
        out["sse_filtered"] = [sse(a, b) for a, b in zip(made, clean)]
        out["psnr_noisy"] = psnr(sum(out["sse_noisy"]), N * H, W)
        out["psnr_filtered"] = psnr(sum(out["sse_filtered"]), N * H, W)
    return out
