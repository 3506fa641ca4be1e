"""Direct projective refinement: the host definition, in the role synth.py plays for the synthetic frames.

The device path (``csrc/gme_direct.hip`` behind ``gme_seq_direct_eval``, ``gme_seq_refine_projective`` and
``gme_seq_compensate_projective``) computes what this module computes; the tests compare the two.

Parameters are ``float64[8] h``, H = [[h0 h1 h2] [h3 h4 h5] [h6 h7 1]].  A pixel of the CURRENT frame at column ``u``,
row ``v`` samples the PREVIOUS frame at

    u' = (h0 u + h1 v + h2) / d,   v' = (h3 u + h4 v + h5) / d,   d = h6 u + h7 v + 1

(OpenCV's ``warpPerspective(prev, H, INTER_LINEAR | WARP_INVERSE_MAP)``).  These are image axes, (column, row) -- not the
reference's "x = row" convention of motion.py.  The identity is ``[1 0 0 0 1 0 0 0]``.

Every operation of the warp, the bilinear weights and the residual is one float64 operation rounded on its own, in the
order written here; the library builds with ``-ffp-contract=off``, so host and device residuals are bit-identical for
identical parameters.
"""
import math

import numpy as np

IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
HIST_BINS = 4096              # histogram of |e| at the start of each level: bins of width 1 / HIST_SCALE
HIST_SCALE = 16.0
MAX_HALVINGS = 4              # a step that raises the cost is retried at half length at most this often
CONVERGED_PX = 1e-3           # a level ends when a step moves no corner further than this (level pixels, per axis)
FLAG_SINGULAR, FLAG_FEW_VALID, FLAG_DENOMINATOR, FLAG_NO_GAIN, FLAG_MAX_ITERS = 1, 2, 4, 8, 16
N_SUMS = 44                   # JtJ upper triangle (36, row by row) | Jte (8)


def affine_to_projective(params, block_size=16):
    """The indirect affine estimate (float64[..., 6] = [a0 a1 a2 b0 b1 b2], or the 12 of a second-order model, of which
    the first six are used) -> float64[..., 8].  The reference displaces block (i, j) by d0 = a0 + a1 i + a2 j columns and
    d1 = b0 + b1 i + b2 j rows (motion.py:139-157, 289-321); at the fractional block coordinates i = (v - c) / bs,
    j = (u - c) / bs with c = (bs - 1) / 2 that is the warp u' = u - d0, v' = v - d1."""
    p = np.asarray(params, dtype=np.float64)
    a0, a1, a2, b0, b1, b2 = (p[..., k] for k in range(6))
    bs = float(block_size)
    c = (bs - 1.0) / 2.0
    h = np.zeros(p.shape[:-1] + (8,))
    h[..., 0] = 1.0 - a2 / bs
    h[..., 1] = -a1 / bs
    h[..., 2] = -a0 + (a1 + a2) * c / bs
    h[..., 3] = -b2 / bs
    h[..., 4] = 1.0 - b1 / bs
    h[..., 5] = -b0 + (b1 + b2) * c / bs
    return h


def projective_to_level(h, level):
    """Full-resolution parameters -> those of pyramid level ``level`` (2 = full resolution): S H S^-1 with
    S = diag(s, s, 1), s = 2^-(2 - level) (cv2.pyrDown puts level pixel k at full-resolution pixel 2k).  h2, h5 scale by s,
    h6, h7 by 1 / s; powers of two, so exact in float64.  Returns a new array."""
    q = np.array(h, dtype=np.float64)
    s = 2.0 ** -(2 - int(level))
    q[..., 2] = q[..., 2] * s
    q[..., 5] = q[..., 5] * s
    q[..., 6] = q[..., 6] * (1.0 / s)
    q[..., 7] = q[..., 7] * (1.0 / s)
    return q


def finer(h):
    """Level L parameters -> level L + 1: h2, h5 doubled, h6, h7 halved."""
    return projective_to_level(projective_to_level(h, 2), 3)


def warp(h, u, v):
    """(u', v', d) of the pixels (u, v) of the current frame (float64 arrays)."""
    d = (h[6] * u + h[7] * v) + 1.0
    up = ((h[0] * u + h[1] * v) + h[2]) / d
    vp = ((h[3] * u + h[4] * v) + h[5]) / d
    return up, vp, d


def _corners(h, H, W):
    u = np.array([0.0, W - 1.0, 0.0, W - 1.0])
    v = np.array([0.0, 0.0, H - 1.0, H - 1.0])
    return u, v


def corners_ok(h, H, W):
    """d > 0 at the four corners of an H x W frame (then everywhere in it: d is affine in (u, v))."""
    u, v = _corners(h, H, W)
    return bool(np.all((h[6] * u + h[7] * v) + 1.0 > 0.0))


def corner_shift(a, b, H, W):
    """The largest per-axis move of a frame corner from the warp ``a`` to the warp ``b``."""
    u, v = _corners(a, H, W)
    ua, va, _ = warp(a, u, v)
    ub, vb, _ = warp(b, u, v)
    return float(max(np.max(np.abs(ub - ua)), np.max(np.abs(vb - va))))


def _taps(img, up, vp):
    """Integer taps and weights of the bilinear sample at (up, vp), which must lie inside the frame: the far tap of a
    coordinate on the last row / column is clamped."""
    H, W = img.shape
    x0 = np.floor(up)
    y0 = np.floor(vp)
    ax = up - x0
    ay = vp - y0
    xi = x0.astype(np.int64)
    yi = y0.astype(np.int64)
    return xi, yi, np.minimum(xi + 1, W - 1), np.minimum(yi + 1, H - 1), ax, ay


def _blend(g00, g01, g10, g11, ax, ay):
    top = (1.0 - ax) * g00 + ax * g01
    bot = (1.0 - ax) * g10 + ax * g11
    return (1.0 - ay) * top + ay * bot


def bilinear(img, up, vp):
    """img (2-D) sampled bilinearly at in-frame points (up, vp), float64."""
    p = np.asarray(img, dtype=np.float64)
    xi, yi, x1, y1, ax, ay = _taps(p, up, vp)
    return _blend(p[yi, xi], p[yi, x1], p[y1, xi], p[y1, x1], ax, ay)


def gradients(img):
    """Central-difference images Gx = (p[v, u+1] - p[v, u-1]) / 2 and Gy likewise, edges replicated."""
    p = np.asarray(img, dtype=np.float64)
    gx = np.empty_like(p)
    gy = np.empty_like(p)
    gx[:, 1:-1] = p[:, 2:] - p[:, :-2]
    gx[:, 0] = p[:, min(1, p.shape[1] - 1)] - p[:, 0]
    gx[:, -1] = p[:, -1] - p[:, max(p.shape[1] - 2, 0)]
    gy[1:-1, :] = p[2:, :] - p[:-2, :]
    gy[0, :] = p[min(1, p.shape[0] - 1), :] - p[0, :]
    gy[-1, :] = p[-1, :] - p[max(p.shape[0] - 2, 0), :]
    return gx * 0.5, gy * 0.5


def residual(prev, cur, h):
    """-> (e, valid, up, vp, d, u, v) over all pixels of the level (flattened, row-major); e = cur - bilinear(prev)(u', v')
    where the sample point lies in the frame, 0 elsewhere."""
    H, W = prev.shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    u, v = u.ravel(), v.ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        up, vp, d = warp(np.asarray(h, dtype=np.float64), u, v)
        valid = (up >= 0.0) & (up <= W - 1.0) & (vp >= 0.0) & (vp <= H - 1.0)
    ups, vps = np.where(valid, up, 0.0), np.where(valid, vp, 0.0)
    e = np.asarray(cur, dtype=np.float64).ravel() - bilinear(prev, ups, vps)
    return np.where(valid, e, 0.0), valid, ups, vps, d, u, v


def threshold(abs_e, outlier_fraction):
    """Upper edge of the first histogram bin (4096 bins of 1/16) at which the cumulative count of |e| reaches
    ceil((1 - f) n_valid); 0 when nothing is valid."""
    n = len(abs_e)
    if n == 0:
        return 0.0
    bins = np.minimum(np.floor(abs_e * HIST_SCALE), HIST_BINS - 1).astype(np.int64)
    cum = np.cumsum(np.bincount(bins, minlength=HIST_BINS))
    k = max(1, int(math.ceil((1.0 - float(outlier_fraction)) * float(n))))
    return (int(np.searchsorted(cum, k)) + 1) / HIST_SCALE


def cost_of(n_valid, n_in, se2, t):
    """(sum over inliers of e^2 + (n_valid - n_in) t^2) / n_valid; infinite when nothing is valid."""
    if n_valid == 0:
        return math.inf
    return (se2 + float(n_valid - n_in) * (t * t)) / float(n_valid)


def sums(prev, cur, h, t, gx=None, gy=None):
    """One pass at ``h`` under the threshold ``t`` -> (n_valid, n_in, cost, sums float64[44] = JtJ upper triangle | Jte)
    over the inliers |e| < t.  J is the derivative of the prediction: [gx u, gx v, gx, gy u, gy v, gy, -q u, -q v] / d,
    q = gx u' + gy v', (gx, gy) the bilinear samples of the central-difference images."""
    h = np.asarray(h, dtype=np.float64)
    e, valid, up, vp, d, u, v = residual(prev, cur, h)
    inl = valid & (np.abs(e) < t)
    n_valid, n_in = int(valid.sum()), int(inl.sum())
    if gx is None:
        gx, gy = gradients(prev)
    e, up, vp, d, u, v = e[inl], up[inl], vp[inl], d[inl], u[inl], v[inl]
    xi, yi, x1, y1, ax, ay = _taps(gx, up, vp)
    sx = _blend(gx[yi, xi], gx[yi, x1], gx[y1, xi], gx[y1, x1], ax, ay)
    sy = _blend(gy[yi, xi], gy[yi, x1], gy[y1, xi], gy[y1, x1], ax, ay)
    q = sx * up + sy * vp
    r = 1.0 / d
    J = np.stack([(sx * u) * r, (sx * v) * r, sx * r, (sy * u) * r, (sy * v) * r, sy * r, -(q * u) * r, -(q * v) * r], axis=1)
    out = np.empty(N_SUMS)
    k = 0
    for a in range(8):
        for b in range(a, 8):
            out[k] = np.dot(J[:, a], J[:, b])
            k += 1
    out[36:] = J.T @ e
    return n_valid, n_in, cost_of(n_valid, n_in, float(np.dot(e, e)), t), out


def evaluate(prev, cur, h, outlier_fraction=0.1):
    """gme_seq_direct_eval for one pair at one level (``h`` in that level's coordinates): a fresh threshold at ``h``, then
    one pass -> dict(threshold, n_valid, n_in, cost, sums float64[44])."""
    e, valid = residual(prev, cur, h)[:2]
    t = threshold(np.abs(e[valid]), outlier_fraction)
    n_valid, n_in, cost, s = sums(prev, cur, h, t)
    return {"threshold": t, "n_valid": n_valid, "n_in": n_in, "cost": cost, "sums": s}


eval = evaluate   # noqa: A001 -- the name the contract uses


def normal_matrix(s):
    """float64[44] sums -> (JtJ 8x8, Jte 8)."""
    N = np.zeros((8, 8))
    k = 0
    for a in range(8):
        for b in range(a, 8):
            N[a, b] = N[b, a] = s[k]
            k += 1
    return N, np.array(s[36:44], dtype=np.float64)


def solve(s):
    """JtJ delta = Jte by the device's elimination (gme_internal.h: Jacobi equilibration, then Gaussian elimination with
    partial pivoting, first largest pivot) -> (delta float64[8], ok); not ok for a non-positive diagonal, a zero pivot or a
    pivot ratio below 1e-12 (the criteria of k_direct_state, gme_direct.hip)."""
    N, rhs = normal_matrix(s)
    n = 8
    if not all(N[k, k] > 0.0 for k in range(n)):
        return np.zeros(n), False
    dsc = [1.0 / math.sqrt(N[k, k]) for k in range(n)]
    a = [[(N[r, c] * dsc[r]) * dsc[c] for c in range(n)] + [rhs[r] * dsc[r]] for r in range(n)]
    pmin, pmax = math.inf, 0.0
    with np.errstate(all="ignore"):                   # a zero pivot fails the test below, as on the device
        return _eliminate(a, dsc, n, pmin, pmax)


def _eliminate(a, dsc, n, pmin, pmax):
    for k in range(n):
        piv, big = k, abs(a[k][k])
        for r in range(k + 1, n):
            if abs(a[r][k]) > big:
                big, piv = abs(a[r][k]), r
        pmin, pmax = min(pmin, big), max(pmax, big)
        a[k], a[piv] = a[piv], a[k]
        for r in range(k + 1, n):
            f = a[r][k] / a[k][k]
            for c in range(k + 1, n + 1):
                a[r][c] = a[r][c] - f * a[k][c]
    if pmin == 0.0 or not (pmin / pmax >= 1e-12):
        return np.zeros(n), False
    z = [0.0] * n
    for k in range(n - 1, -1, -1):
        acc = a[k][n]
        for c in range(k + 1, n):
            acc = acc - a[k][c] * z[c]
        z[k] = acc / a[k][k]
    return np.array([z[k] * dsc[k] for k in range(n)]), True


def refine(prev, cur, init, outlier_fraction=0.1, max_iters=10, info=None):
    """gme_seq_refine_projective for one pair -> (h float64[8], flags).  ``prev`` / ``cur`` are the 3-level pyramids of the
    two frames ([level 0, level 1, level 2], cv2.pyrDown as utils.get_pyramids builds them); ``init`` the full-resolution start (affine_to_projective of the
    indirect estimate).  Gauss-Newton with step halving per level 0 -> 1 -> 2 under a truncated quadratic whose threshold
    is fixed at each level's start; see DESIGN.md §7b for the flags.  ``info`` (a dict) receives the iterations per level."""
    pp, cp = prev, cur
    init = np.array(init, dtype=np.float64).reshape(8)
    flags = 0
    h = projective_to_level(init, 0)
    iters = []
    t = cost = 0.0
    for L in range(3):
        P = np.asarray(pp[L], dtype=np.float64)
        C = np.asarray(cp[L], dtype=np.float64)
        Hl, Wl = P.shape
        if L > 0:
            h = finer(h)
        if not corners_ok(h, Hl, Wl):
            return init, flags | FLAG_DENOMINATOR
        e, valid = residual(P, C, h)[:2]
        n_valid = int(valid.sum())
        if 4 * n_valid < Hl * Wl:
            return init, flags | FLAG_FEW_VALID
        t = threshold(np.abs(e[valid]), outlier_fraction)
        gx, gy = gradients(P)

        def passes(hh):
            if not corners_ok(hh, Hl, Wl):
                return math.inf, None
            nv, _, c, s = sums(P, C, hh, t, gx, gy)
            return (math.inf if 4 * nv < Hl * Wl else c), s

        cost, S = passes(h)
        it = 0
        while True:
            delta, ok = solve(S)
            if not ok:
                return init, flags | FLAG_SINGULAR
            step, halvings = delta, 0
            while True:
                trial = h + step
                c, St = passes(trial)
                if c <= cost:
                    break
                halvings += 1
                if halvings > MAX_HALVINGS:
                    trial = None
                    break
                step = step * 0.5
            if trial is None:
                break
            moved = corner_shift(h, trial, Hl, Wl)
            h, cost, S = trial, c, St
            it += 1
            if moved <= CONVERGED_PX:
                break
            if it >= max_iters:
                if L == 2:
                    flags |= FLAG_MAX_ITERS
                break
        iters.append(it)
    P = np.asarray(pp[2], dtype=np.float64)
    c_init = math.inf
    if corners_ok(init, *P.shape):
        nv, _, c_init, _ = sums(P, np.asarray(cp[2], dtype=np.float64), init, t)
        if 4 * nv < P.size:
            c_init = math.inf
    if info is not None:
        info.update(iters=iters, t=t, cost=cost, cost_init=c_init)
    if not (cost < c_init):
        return init, flags | FLAG_NO_GAIN
    return h, flags


def full_cost(prev, cur, h, t):
    """The level-2 objective of ``h`` under the threshold ``t``."""
    return sums(np.asarray(prev, dtype=np.float64), np.asarray(cur, dtype=np.float64), h, t)[2]


def compensate(prev, cur, h):
    """gme_seq_compensate_projective for one pair -> (uint8 frame, sse): floor(bilinear(prev)(u', v') + 0.5) where the
    sample point lies in the frame, prev[v, u] elsewhere (the reference keeps the previous frame's pixel, motion.py:289-321)."""
    prev = np.asarray(prev, dtype=np.uint8)
    H, W = prev.shape
    _, valid, up, vp = residual(prev, cur, np.asarray(h, dtype=np.float64))[:4]
    val = np.floor(bilinear(prev, up, vp) + 0.5)
    out = np.where(valid, val, prev.ravel().astype(np.float64)).astype(np.uint8).reshape(H, W)
    diff = np.asarray(cur, dtype=np.int64) - out.astype(np.int64)
    return out, int((diff * diff).sum())
