"""Video stabilization from the estimated camera path: the host definition, in the role direct.py plays for
the projective refinement.

The device path (``csrc/gme_stab.hip`` behind ``gme_seq_warp_frames``, ``gme_seq_read_warped_range`` and
``gme_seq_frame_sse``) warps the frames as ``warp_frames`` here does, bit for bit; ``sequence.ShardedSequence.stabilize`` drives
it over the lanes of a shard.

Conventions are direct.py's: image axes (``u`` the column, ``v`` the row); ``h`` float64[8] with
M(h) = [[h0 h1 h2] [h3 h4 h5] [h6 h7 1]]; a warp maps a pixel of the frame being built to the point it samples.

* Pair warps: for frame distance 1, ``h_p`` of the pair (p, p+1) maps a pixel of frame p+1 to frame-p coordinates (what
  ``gme_seq_refine_projective`` returns; the indirect affine estimate enters as ``affine_to_projective``).
* ``trajectory``: C_0 = I, C_t = C_{t-1} M(h_{t-1}) with C_t[2,2] = 1; C_t maps frame-t pixels to frame-0 coordinates.
* ``smooth``: S_t, the Gaussian average of C_{t-r_t} .. C_{t+r_t}, r_t = min(radius, t, N-1-t) (symmetric at the ends).
* Correction of frame t: W_t = C_t^-1 S_t Z(crop), [2,2] = 1, where Z zooms by s = 1 - crop about the frame centre.  Output
  pixel (u, v) of stabilized frame t samples source frame t at direct.warp(W_t, u, v).
* Full-frame form: frame s sees output pixel (u, v) of stabilized frame t at C_s^-1 S_t Z (u, v), so what
  W_t misses of frame t is taken from frames t-1, t+1, t-2, ... (``fill_candidates``) by ``warp_fill``, the definition of
  ``gme_seq_warp_fill`` (``csrc/gme_stab_fill.hip``): per pixel, the first candidate whose point lies in its frame.
* Frame flags: FLAG_FALLBACK (1) -- W_t was non-finite or had d <= 0 at an output corner and was replaced by Z;
  FLAG_BORDER (2) -- an output corner maps outside the frame, so the frame has border pixels (informational).
"""
import math

import numpy as np

import direct

FLAG_FALLBACK, FLAG_BORDER = 1, 2
CORNER_MARGIN = 1e-3          # auto_crop: every output corner must map into [m, W-1-m] x [m, H-1-m]
CROP_TOL = 1e-4               # auto_crop: bisection tolerance
BORDERS = {"constant": 0, "replicate": 1}
ESTIMATORS = ("projective", "affine")


def matrix(h):
    """float64[..., 8] -> float64[..., 3, 3] = M(h)."""
    h = np.asarray(h, dtype=np.float64)
    m = np.ones(h.shape[:-1] + (9,))
    m[..., :8] = h
    return m.reshape(h.shape[:-1] + (3, 3))


def params(m):
    """float64[..., 3, 3] -> float64[..., 8], each matrix divided by its [2,2] entry first."""
    m = np.asarray(m, dtype=np.float64)
    m = m / m[..., 2:3, 2:3]
    return m.reshape(m.shape[:-2] + (9,))[..., :8].copy()


def trajectory(h):
    """Pair warps float64[P, 8] -> the camera path C float64[P+1, 3, 3] (C_t: frame-t pixels -> frame-0 coordinates)."""
    h = np.asarray(h, dtype=np.float64).reshape(-1, 8)
    C = np.empty((len(h) + 1, 3, 3))
    C[0] = np.eye(3)
    M = matrix(h)
    for t in range(1, len(C)):
        c = C[t - 1] @ M[t - 1]
        C[t] = c / c[2, 2]
    return C


def smooth(C, radius=15, sigma=None):
    """Gaussian average of the path: S_t = sum_k w_k C_{t+k} / sum_k w_k over k in [-r_t, r_t], r_t = min(radius, t, N-1-t),
    w_k = exp(-k^2 / (2 sigma^2)), sigma = radius / 3 by default.  radius 0 gives S = C."""
    C = np.asarray(C, dtype=np.float64)
    radius = int(radius)
    if radius < 0:
        raise ValueError("radius %d < 0" % radius)
    if radius == 0:
        return C.copy()
    sigma = radius / 3.0 if sigma is None else float(sigma)
    if not sigma > 0:
        raise ValueError("sigma %r must be positive" % sigma)
    N = len(C)
    S = np.empty_like(C)
    for t in range(N):
        r = min(radius, t, N - 1 - t)
        k = np.arange(-r, r + 1)
        w = np.exp(-(k * k) / (2.0 * sigma * sigma))
        S[t] = np.tensordot(w, C[t - r:t + r + 1], axes=1) / w.sum()
    return S


def zoom(crop, H, W):
    """Z(crop): the zoom by s = 1 - crop about the frame centre ((W-1)/2, (H-1)/2)."""
    s = 1.0 - float(crop)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([[s, 0.0, (1.0 - s) * cx], [0.0, s, (1.0 - s) * cy], [0.0, 0.0, 1.0]])


def _corners(H, W):
    return np.array([0.0, W - 1.0, 0.0, W - 1.0]), np.array([0.0, 0.0, H - 1.0, H - 1.0])


def _relative(C, S):
    """C_t^-1 S_t per frame; exactly I where S_t == C_t (radius 0, and the ends of the path)."""
    A = np.empty_like(C)
    for t in range(len(C)):
        if np.array_equal(S[t], C[t]):
            A[t] = np.eye(3)
        else:
            with np.errstate(all="ignore"):
                try:
                    A[t] = np.linalg.solve(C[t], S[t])
                except np.linalg.LinAlgError:
                    A[t] = np.nan
    return A


def _corrections(A, H, W, crop, margin=0.0):
    """(W float64[N, 8], flags int32[N], inside bool[N]) at one crop; ``inside``: every output corner maps into the frame
    shrunk by ``margin``."""
    Z = zoom(crop, H, W)
    u, v = _corners(H, W)
    out = np.empty((len(A), 8))
    flags = np.zeros(len(A), np.int32)
    ins = np.zeros(len(A), bool)
    for t in range(len(A)):
        with np.errstate(all="ignore"):
            m = A[t] @ Z
            m = m / m[2, 2]
            w = m.reshape(9)[:8]
            up, vp, d = direct.warp(w, u, v)
        if not (np.all(np.isfinite(w)) and np.all(d > 0.0)):
            flags[t] |= FLAG_FALLBACK
            w = params(Z)
            up, vp, d = direct.warp(w, u, v)
        out[t] = w
        if not (np.all(up >= 0.0) and np.all(up <= W - 1.0) and np.all(vp >= 0.0) and np.all(vp <= H - 1.0)):
            flags[t] |= FLAG_BORDER
        ins[t] = bool(np.all(up >= margin) and np.all(up <= W - 1.0 - margin) and np.all(vp >= margin)
                      and np.all(vp <= H - 1.0 - margin))
    return out, flags, ins


def corrections(C, S, H, W, crop=0.0):
    """W_t = C_t^-1 S_t Z(crop) with [2,2] = 1 -> (W float64[N, 8], frame flags int32[N])."""
    w, flags, _ = _corrections(_relative(np.asarray(C, np.float64), np.asarray(S, np.float64)), H, W, crop)
    return w, flags


def auto_crop(C, S, H, W, max_crop=0.25):
    """The smallest crop in [0, max_crop] (to within CROP_TOL, by bisection) at which every output corner of every frame maps
    into [m, W-1-m] x [m, H-1-m], m = CORNER_MARGIN; ``max_crop`` when even that does not suffice."""
    A = _relative(np.asarray(C, np.float64), np.asarray(S, np.float64))

    def ok(c):
        return bool(np.all(_corrections(A, H, W, c, CORNER_MARGIN)[2]))
    max_crop = float(max_crop)
    if ok(0.0):
        return 0.0
    if not ok(max_crop):
        return max_crop
    lo, hi = 0.0, max_crop
    while hi - lo > CROP_TOL:
        mid = 0.5 * (lo + hi)
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return hi


def corners_inside(w, H, W, margin=CORNER_MARGIN):
    """Every output corner of the warp ``w`` maps into the frame shrunk by ``margin``."""
    u, v = _corners(H, W)
    up, vp, _ = direct.warp(np.asarray(w, np.float64), u, v)
    return bool(np.all(up >= margin) and np.all(up <= W - 1.0 - margin) and np.all(vp >= margin) and np.all(vp <= H - 1.0 - margin))


def border_id(border):
    if border not in BORDERS:
        raise ValueError("border %r (choose from %r)" % (border, tuple(BORDERS)))
    return BORDERS[border]


def warp_frames(frames, warps, border="constant", fill=0):
    """The definition of gme_seq_warp_frames: uint8[N, H, W] frames, float64[N, 8] warps -> (uint8[N, H, W], valid int64[N]).
    Output pixel (u, v) of frame t samples frame t at (u', v') = direct.warp(W_t, u, v): where 0 <= u' <= W-1 and
    0 <= v' <= H-1 (a valid pixel) it is floor(bilinear + 0.5) with direct's taps; elsewhere ``fill`` (constant) or the
    point clamped into the frame first (replicate; a NaN coordinate clamps to 0)."""
    bid = border_id(border)
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError("fill %d outside 0 .. 255" % fill)
    frames = np.asarray(frames, dtype=np.uint8)
    N, H, W = frames.shape
    warps = np.asarray(warps, dtype=np.float64).reshape(N, 8)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = u.ravel(), v.ravel()
    out = np.empty_like(frames)
    valid = np.zeros(N, np.int64)
    for t in range(N):
        with np.errstate(all="ignore"):
            up, vp, _ = direct.warp(warps[t], u, v)
            ins = (up >= 0.0) & (up <= W - 1.0) & (vp >= 0.0) & (vp <= H - 1.0)
        valid[t] = int(ins.sum())
        if bid == 1:
            up = np.where(up > 0.0, np.where(up < W - 1.0, up, W - 1.0), 0.0)
            vp = np.where(vp > 0.0, np.where(vp < H - 1.0, vp, H - 1.0), 0.0)
            val = np.floor(direct.bilinear(frames[t], up, vp) + 0.5)
        else:
            val = np.floor(direct.bilinear(frames[t], np.where(ins, up, 0.0), np.where(ins, vp, 0.0)) + 0.5)
            val = np.where(ins, val, float(fill))
        out[t] = val.astype(np.uint8).reshape(H, W)
    return out, valid


MAX_NEIGHBOURS = 8            # fill_candidates: neighbours a side
MAX_CANDIDATES = 2 * MAX_NEIGHBOURS + 1
NO_SOURCE = 255               # warp_fill's `source` where no candidate gave the pixel


def warp_fill(frames, sources, warps, border="constant", fill=0):
    """The definition of gme_seq_warp_fill: uint8[N, H, W] frames, int32[N, n] candidate frames and
    float64[N, n, 8] candidate warps, 1 <= n <= 17 -> (out uint8[N, H, W], source uint8[N, H, W], valid int64[N],
    filled int64[N], sse int64[N-1]).  Output pixel (u, v) of frame t walks its candidates j = 0 .. n-1 in order; a candidate
    with sources[t, j] == -1 is skipped; the first one whose point direct.warp(warps[t, j], u, v) is valid in frame
    sources[t, j] (warp_frames' test) gives the pixel, floor(bilinear + 0.5).  Where none is valid the pixel follows
    ``border`` as warp_frames does for candidate 0 (which must be a frame).  ``source``: the winning j, NO_SOURCE where there
    is none; ``valid`` / ``filled``: the pixels won by candidate 0 / by a later one; sse[k] = sum (out[k+1] - out[k])^2."""
    bid = border_id(border)
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError("fill %d outside 0 .. 255" % fill)
    frames = np.asarray(frames, dtype=np.uint8)
    N, H, W = frames.shape
    sources = np.asarray(sources)
    if sources.ndim != 2 or len(sources) != N or not 1 <= sources.shape[1] <= MAX_CANDIDATES:
        raise ValueError("sources of shape %r: need [%d, n] with n in 1 .. %d" % (sources.shape, N, MAX_CANDIDATES))
    n = sources.shape[1]
    if N and (sources.min() < -1 or sources.max() >= N):
        raise ValueError("a source outside -1 .. %d" % (N - 1))
    if np.any(sources[:, 0] < 0):
        raise ValueError("candidate 0 must be a frame")
    sources = sources.astype(np.int32)
    warps = np.asarray(warps, dtype=np.float64).reshape(N, n, 8)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = u.ravel(), v.ravel()
    out = np.empty_like(frames)
    source = np.empty_like(frames)
    valid, filled = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for t in range(N):
        val = np.full(H * W, float(fill))
        who = np.full(H * W, NO_SOURCE, np.uint8)
        if bid == 1:
            with np.errstate(all="ignore"):
                up, vp, _ = direct.warp(warps[t, 0], u, v)
            up = np.where(up > 0.0, np.where(up < W - 1.0, up, W - 1.0), 0.0)
            vp = np.where(vp > 0.0, np.where(vp < H - 1.0, vp, H - 1.0), 0.0)
            val = np.floor(direct.bilinear(frames[sources[t, 0]], up, vp) + 0.5)
        for j in range(n):
            s = int(sources[t, j])
            if s < 0:
                continue
            with np.errstate(all="ignore"):
                up, vp, _ = direct.warp(warps[t, j], u, v)
                ins = (up >= 0.0) & (up <= W - 1.0) & (vp >= 0.0) & (vp <= H - 1.0)
            win = ins & (who == NO_SOURCE)
            if not np.any(win):
                continue
            val[win] = np.floor(direct.bilinear(frames[s], up[win], vp[win]) + 0.5)
            who[win] = j
        out[t] = val.astype(np.uint8).reshape(H, W)
        source[t] = who.reshape(H, W)
        valid[t] = int((who == 0).sum())
        filled[t] = int(((who != 0) & (who != NO_SOURCE)).sum())
    d = out[1:].astype(np.int64) - out[:-1].astype(np.int64)
    return out, source, valid, filled, (d * d).sum(axis=(1, 2))


def fill_candidates(C, S, H, W, crop=0.0, neighbours=1):
    """The candidates of warp_fill for a stabilization -> (sources int32[N, 2K+1], warps float64[N, 2K+1, 8], flags int32[N]),
    K = ``neighbours`` in 0 .. MAX_NEIGHBOURS.  Candidate 0 is frame t itself with corrections(C, S, H, W, crop)'s W_t and
    flags, exactly; candidates 1, 2, 3, 4, ... are frames t-1, t+1, t-2, t+2, ..., frame s under
    params(C_s^-1 S_t Z(crop)): where frame s saw what the stabilized pose of frame t looks at.  A neighbour is dropped
    (source -1; the slots do not move) where s is outside [0, N), its warp is non-finite or has d <= 0 at an output corner, or
    frame t carries FLAG_FALLBACK (its own warp is no longer the stabilized pose)."""
    K = int(neighbours)
    if not 0 <= K <= MAX_NEIGHBOURS:
        raise ValueError("neighbours %d outside 0 .. %d" % (K, MAX_NEIGHBOURS))
    C, S = np.asarray(C, np.float64), np.asarray(S, np.float64)
    N = len(C)
    w0, flags = corrections(C, S, H, W, crop)
    sources = np.full((N, 2 * K + 1), -1, np.int32)
    warps = np.zeros((N, 2 * K + 1, 8))
    sources[:, 0] = np.arange(N)
    warps[:, 0] = w0
    Z = zoom(crop, H, W)
    u, v = _corners(H, W)
    for t in range(N):
        if flags[t] & FLAG_FALLBACK:
            continue
        for j in range(1, 2 * K + 1):
            s = t - (j + 1) // 2 if j % 2 else t + j // 2
            if not 0 <= s < N:
                continue
            with np.errstate(all="ignore"):
                try:
                    w = params(np.linalg.solve(C[s], S[t] @ Z))
                except np.linalg.LinAlgError:
                    continue
                d = direct.warp(w, u, v)[2]
            if np.all(np.isfinite(w)) and np.all(d > 0.0):
                sources[t, j] = s
                warps[t, j] = w
    return sources, warps, flags


def itf(sse, H, W):
    """Inter-frame transformation fidelity: the mean PSNR of consecutive frames from their squared errors
    (sequence.psnr_from_sse on full frames)."""
    import sequence
    sse = np.asarray(sse, dtype=np.int64)
    return float(np.mean(sequence.psnr_from_sse(sse, H, W))) if len(sse) else 0.0


def plan(h, H, W, radius=15, sigma=None, crop="auto", max_crop=0.25, neighbours=0):
    """The host half of a stabilization from the pair warps float64[P, 8] -> dict(C, S, crop, W, flags).  With
    ``neighbours`` >= 1 (the border filled from that many frames a side, fill_candidates) nothing has to be cropped away, so
    crop "auto" means 0.0, and the dict gains ``neighbours``, ``sources`` and ``fill_warps``; W is candidate 0's warp."""
    K = int(neighbours)
    if not 0 <= K <= MAX_NEIGHBOURS:
        raise ValueError("neighbours %d outside 0 .. %d" % (K, MAX_NEIGHBOURS))
    C = trajectory(h)
    S = smooth(C, radius, sigma)
    if crop == "auto":
        c = auto_crop(C, S, H, W, max_crop) if K == 0 else 0.0
    else:
        c = float(crop)
        if not 0.0 <= c < 1.0:
            raise ValueError("crop %r outside [0, 1)" % crop)
    if K == 0:
        w, flags = corrections(C, S, H, W, c)
        return {"C": C, "S": S, "crop": c, "W": w, "flags": flags}
    sources, warps, flags = fill_candidates(C, S, H, W, c, K)
    return {"C": C, "S": S, "crop": c, "W": warps[:, 0].copy(), "flags": flags, "neighbours": K, "sources": sources,
            "fill_warps": warps}


def stabilize(frames, estimator="projective", radius=15, sigma=None, crop="auto", max_crop=0.25, border="constant", fill=0,
              procedure=3, search_window=2, outlier_fraction=0.1, max_iters=10, neighbours=0):
    """One call for a video in host memory (uint8[N, H, W] or a list of frames) -> (uint8[N, H, W], result).  ``result``
    (dict): pair ``h`` and ``pair_flags``, ``C``, ``S``, ``W``, ``crop``, frame ``flags``, ``valid`` and ``itf_before`` /
    ``itf_after``.  ``estimator``: "projective" (the direct refinement) or "affine" (the reference's indirect estimate).
    ``neighbours`` K >= 1 fills what the corrected view of frame t misses from frames t-1, t+1, .. t-K, t+K (plan;
    ``border`` / ``fill`` decide what none of them reaches) and adds ``neighbours``, ``sources``, ``filled`` and ``unfilled``
    per frame to the result."""
    import sequence
    frames = np.ascontiguousarray(np.stack([np.asarray(f, dtype=np.uint8) for f in frames])
                                  if not isinstance(frames, np.ndarray) else frames, dtype=np.uint8)
    N, H, W = frames.shape
    sh = sequence.ShardedSequence(H, W, N, 1)
    try:
        sh.load(frames)
        res = sh.stabilize(estimator=estimator, radius=radius, sigma=sigma, crop=crop, max_crop=max_crop, border=border,
                           fill=fill, procedure=procedure, search_window=search_window, outlier_fraction=outlier_fraction,
                           max_iters=max_iters, neighbours=neighbours)
        out = sh.read_stabilized_range(0, N)
    finally:
        sh.close()
    return out, res
