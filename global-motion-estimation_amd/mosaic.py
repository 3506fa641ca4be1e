"""Background mosaic and moving-object masks from the estimated camera path: the host definition, in the role
stabilize.py plays for the stabilizer.

The device path (``csrc/gme_mosaic.hip`` behind ``gme_seq_mosaic``, ``gme_seq_read_mosaic``, ``gme_seq_moving_masks`` and
``gme_seq_read_masks_range``) computes what ``build`` and ``moving_masks`` here do, bit for bit;
``sequence.ShardedSequence.mosaic`` drives it.

Conventions are direct.py's and stabilize.py's: image axes (``u`` the column, ``v`` the row); ``h`` float64[8] with [2,2] = 1; a
warp maps a pixel of the thing being built to the point it samples; C_t (stabilize.trajectory) maps frame-t pixels to frame-0
coordinates.

* ``plan``: A_t = C_anchor^-1 C_t maps frame-t pixels to anchor-frame coordinates.  The canvas is the integer bounding box of
  the corners of every usable frame under A_t: origin (ox, oy) = floor of the least corner, size (Hc, Wc) up to the ceiling
  of the greatest.  G_t = params(A_t^-1) is the warp a canvas pixel samples frame t with.  A frame is unusable (FLAG_UNUSABLE)
  where A_t or G_t is non-finite or has d <= 0 at a corner of what it maps.
* ``build``: canvas pixel (x, y) samples usable frame t at direct.warp(G_t, x + ox, y + oy), valid where that point lies in
  the frame, value floor(bilinear + 0.5); count = the valid samples, sprite = their lower median (rank (count - 1) // 2).
* ``moving_masks``: frame pixel (u, v) against the sprite at direct.warp(params(A_t), u, v) - (ox, oy); see there.
"""
import numpy as np

import direct
import stabilize as stab

FLAG_UNUSABLE = 1
MAX_FRAMES = 65535            # the sample counts are uint16
DEFAULT_CANVAS_FACTOR = 16    # max_canvas_pixels defaults to this many frames' worth of pixels


def _frame_corners(H, W):
    return np.array([0.0, W - 1.0, 0.0, W - 1.0]), np.array([0.0, 0.0, H - 1.0, H - 1.0])


def plan(h, H, W, anchor=0, max_canvas_pixels=None):
    """Pair warps float64[P, 8] -> dict(A float64[N, 8], G float64[N, 8], ox, oy, Hc, Wc, flags int32[N], anchor), N = P + 1:
    ``plan_path`` of the path stabilize.trajectory(h)."""
    return plan_path(stab.trajectory(h), H, W, anchor, max_canvas_pixels)


def plan_path(C, H, W, anchor=0, max_canvas_pixels=None):
    """The plan of a camera path C float64[N, 3, 3] (C_t: frame-t pixels -> common coordinates).  Unusable frames carry the
    identity in A and G (they are never sampled).  ValueError where the anchor is outside the video or unusable, or the
    canvas has more than ``max_canvas_pixels`` (default 16 H W) pixels."""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 3, 3)
    N = len(C)
    anchor = int(anchor)
    if not 0 <= anchor < N:
        raise ValueError("anchor %d outside the %d frames" % (anchor, N))
    if N > MAX_FRAMES:
        raise ValueError("%d frames (the sample counts are 16 bits: at most %d)" % (N, MAX_FRAMES))
    u, v = _frame_corners(H, W)
    A = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0]), (N, 1))
    G = A.copy()
    flags = np.zeros(N, np.int32)
    lo = np.array([np.inf, np.inf])
    hi = -lo
    with np.errstate(all="ignore"):
        try:
            base = np.linalg.inv(C[anchor])
        except np.linalg.LinAlgError:
            base = np.full((3, 3), np.nan)
        for t in range(N):
            m = base @ C[t]
            a = (m / m[2, 2]).reshape(9)[:8]
            ok = bool(np.all(np.isfinite(a)))
            if ok:
                up, vp, d = direct.warp(a, u, v)
                ok = bool(np.all(d > 0.0) and np.all(np.isfinite(up)) and np.all(np.isfinite(vp)))
            if ok:
                try:
                    g = np.linalg.inv(stab.matrix(a))
                    g = (g / g[2, 2]).reshape(9)[:8]
                except np.linalg.LinAlgError:
                    g = np.full(8, np.nan)
                ok = bool(np.all(np.isfinite(g)))
                if ok:                                   # the corners of the frame's footprint map back with d > 0
                    ok = bool(np.all(direct.warp(g, up, vp)[2] > 0.0))
            if not ok:
                flags[t] |= FLAG_UNUSABLE
                continue
            A[t], G[t] = a, g
            lo = np.minimum(lo, [up.min(), vp.min()])
            hi = np.maximum(hi, [up.max(), vp.max()])
    if flags[anchor] or not np.all(np.isfinite(lo)):
        raise ValueError("the anchor frame %d is unusable: no canvas" % anchor)
    limit = DEFAULT_CANVAS_FACTOR * H * W if max_canvas_pixels is None else int(max_canvas_pixels)
    span = np.ceil(hi) - np.floor(lo) + 1.0
    if not span[0] * span[1] <= limit:
        raise ValueError("canvas %.0f x %.0f exceeds max_canvas_pixels = %d" % (span[1], span[0], limit))
    return {"A": A, "G": G, "ox": int(np.floor(lo[0])), "oy": int(np.floor(lo[1])), "Hc": int(span[1]), "Wc": int(span[0]),
            "flags": flags, "anchor": anchor}


def _samples(frame, g, ox, oy, Hc, Wc):
    """int16[Hc * Wc]: the rounded bilinear sample of ``frame`` at every canvas pixel under the warp g, -1 where the sample
    point lies outside the frame."""
    H, W = frame.shape
    y, x = np.meshgrid(np.arange(Hc, dtype=np.float64) + float(oy), np.arange(Wc, dtype=np.float64) + float(ox), indexing="ij")
    with np.errstate(all="ignore"):
        up, vp, _ = direct.warp(g, x.ravel(), y.ravel())
        ins = (up >= 0.0) & (up <= W - 1.0) & (vp >= 0.0) & (vp <= H - 1.0)
    val = np.floor(direct.bilinear(frame, np.where(ins, up, 0.0), np.where(ins, vp, 0.0)) + 0.5)
    return np.where(ins, val, -1.0).astype(np.int16)


def build(frames, plan, fill=0):
    """The definition of gme_seq_mosaic: uint8[N, H, W] frames and a ``plan`` -> (sprite uint8[Hc, Wc], count uint16[Hc, Wc])."""
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError("fill %d outside 0 .. 255" % fill)
    frames = np.asarray(frames, dtype=np.uint8)
    N = len(frames)
    G, flags = np.asarray(plan["G"], np.float64).reshape(N, 8), np.asarray(plan["flags"]).reshape(N)
    ox, oy, Hc, Wc = int(plan["ox"]), int(plan["oy"]), int(plan["Hc"]), int(plan["Wc"])
    use = [t for t in range(N) if not flags[t]]
    samples = np.full((max(len(use), 1), Hc * Wc), 256, np.int16)     # 256: sorts behind every sample
    for k, t in enumerate(use):
        s = _samples(frames[t], G[t], ox, oy, Hc, Wc)
        samples[k] = np.where(s >= 0, s, 256)
    count = (samples < 256).sum(axis=0)
    samples.sort(axis=0)
    rank = np.maximum(count - 1, 0) // 2
    med = samples[rank, np.arange(Hc * Wc)]
    sprite = np.where(count > 0, med, fill).astype(np.uint8)
    return sprite.reshape(Hc, Wc), count.astype(np.uint16).reshape(Hc, Wc)


def residuals(frame, a, sprite, count, ox, oy, min_count=3):
    """(known bool[H, W], r int64[H, W]) of one frame: the background prediction b = floor(bilinear(sprite, x', y') + 0.5) at
    (x', y') = direct.warp(a, u, v) - (ox, oy) is known where the point lies in [0, Wc-1] x [0, Hc-1] and all four taps (the
    far one clamped as direct.py does) have count >= min_count; r = |frame - b| there, 0 elsewhere.  ``b`` is returned too."""
    H, W = frame.shape
    Hc, Wc = sprite.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        up, vp, _ = direct.warp(a, u.ravel(), v.ravel())
        xp, yp = up - float(ox), vp - float(oy)
        ins = (xp >= 0.0) & (xp <= Wc - 1.0) & (yp >= 0.0) & (yp <= Hc - 1.0)
    xp, yp = np.where(ins, xp, 0.0), np.where(ins, yp, 0.0)
    xi, yi, x1, y1, _, _ = direct._taps(sprite, xp, yp)
    c = np.asarray(count, np.int64)
    known = ins & (c[yi, xi] >= min_count) & (c[yi, x1] >= min_count) & (c[y1, xi] >= min_count) & (c[y1, x1] >= min_count)
    b = np.floor(direct.bilinear(sprite, xp, yp) + 0.5).astype(np.int64)
    r = np.where(known, np.abs(frame.astype(np.int64).ravel() - b), 0)
    return known.reshape(H, W), r.reshape(H, W), np.where(known, b, 0).reshape(H, W)


def _box3(a):
    """Sum over the 3x3 neighbourhood inside the frame."""
    p = np.pad(a, 1)
    H, W = a.shape
    return sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))


def moving_masks(frames, plan, sprite, count, threshold=16, min_count=3):
    """The definition of gme_seq_moving_masks -> (masks uint8[N, H, W] of 0 / 1, known int64[N], moving int64[N]): mask = 1
    where the pixel is known (``residuals``) and the residuals of the known pixels of its 3x3 neighbourhood inside the frame
    (n of them, itself included) sum to more than threshold * n.  Unusable frames: zero mask, known = 0."""
    threshold, min_count = int(threshold), int(min_count)
    if not 0 <= threshold <= 255:
        raise ValueError("threshold %d outside 0 .. 255" % threshold)
    if min_count < 1:
        raise ValueError("min_count %d < 1" % min_count)
    frames = np.asarray(frames, dtype=np.uint8)
    N = len(frames)
    A, flags = np.asarray(plan["A"], np.float64).reshape(N, 8), np.asarray(plan["flags"]).reshape(N)
    masks = np.zeros(frames.shape, np.uint8)
    known, moving = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(N):
        if flags[t]:
            continue
        k, r, _ = residuals(frames[t], A[t], sprite, count, int(plan["ox"]), int(plan["oy"]), min_count)
        m = k & (_box3(r) > threshold * _box3(k.astype(np.int64)))
        masks[t] = m
        known[t], moving[t] = int(k.sum()), int(m.sum())
    return masks, known, moving


def mosaic(frames, estimator="projective", anchor=0, threshold=16, min_count=3, fill=0, masks=True, max_canvas_pixels=None,
           procedure=3, search_window=2, outlier_fraction=0.1, max_iters=10):
    """One call for a video in host memory (uint8[N, H, W] or a list of frames) -> (sprite uint8[Hc, Wc], masks uint8[N, H, W]
    of 0 / 1 or None, result).  ``result`` (dict): pair ``h`` and ``pair_flags``, the plan (``A``, ``G``, ``ox``, ``oy``,
    ``Hc``, ``Wc``, frame ``flags``), ``count`` and, with masks, ``known`` and ``moving``."""
    import sequence
    frames = np.ascontiguousarray(np.stack([np.asarray(f, dtype=np.uint8) for f in frames])
                                  if not isinstance(frames, np.ndarray) else frames, dtype=np.uint8)
    N, H, W = frames.shape
    sh = sequence.ShardedSequence(H, W, N, 1)
    try:
        sh.load(frames)
        res = sh.mosaic(estimator=estimator, anchor=anchor, threshold=threshold, min_count=min_count, fill=fill, masks=masks,
                        max_canvas_pixels=max_canvas_pixels, procedure=procedure, search_window=search_window,
                        outlier_fraction=outlier_fraction, max_iters=max_iters)
        sprite, res["count"] = sh.read_mosaic()
        out = sh.read_masks_range(0, N) if masks else None
    finally:
        sh.close()
    return sprite, out, res
