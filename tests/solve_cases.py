"""The affine device solve (k_solve3, gme_kernels.hip) restated in float64 scalars, an exact rational reference, a seeded
catalogue of normal-equation systems, the search for rounding traps and the predicates of the device-solve contract.  Shared
by tests/test_solve3_host.py, tests/test_gpu_solve3.py and tools/solve3_traps.py.

Layout: sums15 = F (9, row-major) | Sx (3) | Sy (3); params = [a0 a1 a2 b0 b1 b2], d_x(i, j) = (a0 + a2 j) + a1 i at the
raw block indices of an h x w field; the fit sees x = 4 i, y = 4 j and the weight 1 / (H W), H, W = 16 h, 16 w."""
import math
from fractions import Fraction

import numpy as np

BS = 16
SHAPES = [(3, 5), (30, 45), (67, 120), (135, 240)]
TRANSLATIONS = [0.7, 12.3, 63.4, 200.7, 500.3]
FAMILIES = ["all", "random70", "band", "last2cols", "last2rows", "corner4x4", "three"]
WELL_SPREAD = ("all", "random70", "band")
SINGULAR = ["column", "row", "block", "collinear", "none"]
NEAR_SINGULAR = ["column_off", "row_off"]        # one block column / row away from the origin: rank 2 up to rounding
COND_LIMIT = 3e-5                                 # k_solve3's flag 8: min / max |pivot| of the equilibrated system below this
TIE_REL = 1e-9                                    # k_solve3's tie flag: within TIE_REL max(1, S) of k + 0.5
DX, DY = [0, 1, 2], [3, 4, 5]


# ---------------------------------------------------------------------------------------------------------------------
# k_solve3, operation for operation (Python floats: every product, difference and quotient rounded on its own)
# ---------------------------------------------------------------------------------------------------------------------
def solve3_np(F, S, equilibrate=True):
    """solve3 of gme_kernels.hip -> (x or None when a pivot is zero / a diagonal entry is not positive, min |pivot|,
    max |pivot|): Jacobi equilibration D F D z = D S with D = 1 / sqrt(diag F), Gaussian elimination with partial pivoting
    (strict > on fabs, so the first largest), back substitution, x = z D.  Without `equilibrate`: the plain elimination the
    kernel had before."""
    F = [float(v) for v in np.asarray(F, dtype=np.float64).reshape(9)]
    S = [float(v) for v in np.asarray(S, dtype=np.float64).reshape(3)]
    if not equilibrate:
        dsc = None
        a = [[F[3 * r + c] for c in range(3)] + [S[r]] for r in range(3)]
    else:
        dsc = [0.0, 0.0, 0.0]
        for k in range(3):
            d = F[4 * k]
            if not d > 0.0:
                return None, 0.0, 0.0
            dsc[k] = 1.0 / math.sqrt(d)
        a = [[(F[3 * r + c] * dsc[r]) * dsc[c] for c in range(3)] + [S[r] * dsc[r]] for r in range(3)]
    pmin, pmax = math.inf, 0.0
    for k in range(3):
        piv = k
        for r in range(k + 1, 3):
            if abs(a[r][k]) > abs(a[piv][k]):
                piv = r
        if a[piv][k] == 0.0:
            return None, 0.0, 0.0
        if piv != k:
            a[k], a[piv] = a[piv], a[k]
        big = abs(a[k][k])
        pmin = big if big < pmin else pmin            # fmin / fmax: a NaN pivot leaves the other operand
        pmax = big if big > pmax else pmax
        for r in range(k + 1, 3):
            m = a[r][k] / a[k][k]
            for c in range(k, 4):
                a[r][c] = a[r][c] - m * a[k][c]
    z = [0.0, 0.0, 0.0]
    for k in (2, 1, 0):
        t = a[k][3]
        for c in range(k + 1, 3):
            t = t - a[k][c] * z[c]
        z[k] = t / a[k][k]
    return (z if dsc is None else [z[k] * dsc[k] for k in range(3)]), pmin, pmax


def params_np(sums15, project=False):
    """Thread 0 of k_solve3 -> (params float64[6], flags 0 / 4 / 8): both systems, the doubling under `project`, flag 4 for a
    singular system (both solutions stay 0), flag 8 for pivots that span more than 1 / COND_LIMIT."""
    s = np.asarray(sums15, dtype=np.float64).reshape(15)
    ax, pmin, pmax = solve3_np(s[:9], s[9:12])
    ay = solve3_np(s[:9], s[12:15])[0] if ax is not None else None
    bad = 0 if ay is not None else 4
    if bad == 0 and not pmin >= COND_LIMIT * pmax:
        bad |= 8
    ax = [0.0, 0.0, 0.0] if ax is None else ax
    ay = [0.0, 0.0, 0.0] if ay is None else ay
    if project:
        ax[0], ay[0] = ax[0] * 2.0, ay[0] * 2.0
    return np.array(ax + ay, dtype=np.float64), bad


def _grid(h, w):
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return i.ravel(), j.ravel()


def field_values(params, h, w):
    """The displacements before rounding, float64[2, h w]: (p0 + p2 j) + p1 i, each product and sum rounded on its own
    (model_component, gme_kernels.hip; affine_field of the NumPy oracle)."""
    p = np.asarray(params, dtype=np.float64).reshape(6)
    i, j = _grid(h, w)
    return np.stack([(p[3 * c] + p[3 * c + 2] * j) + p[3 * c + 1] * i for c in (0, 1)])


def rounded_field(params, h, w):
    """Round-half-even of field_values: what every stage behind a solve sees of the parameters."""
    with np.errstate(invalid="ignore"):
        return np.rint(field_values(params, h, w))


def tie_scale(params, h, w):
    """max(1, S) per component, S = |p0| + |p1| (h - 1) + |p2| (w - 1), summed in that order (fmax: NaN gives 1)."""
    p = [float(v) for v in np.asarray(params, dtype=np.float64).reshape(6)]
    hm, wm = float(h - 1), float(w - 1)
    out = []
    for c in (0, 1):
        s = (abs(p[3 * c]) + abs(p[3 * c + 1]) * hm) + abs(p[3 * c + 2]) * wm
        out.append(s if s > 1.0 else 1.0)
    return out


def tie_flag(params, h, w, fixed_margin=None):
    """The field scan of k_solve3 -> True when the pair is flagged: a displacement within TIE_REL max(1, S) of k + 0.5
    (<=), or not |d| < 30000 (NaN included).  `fixed_margin` restates the rule the kernel had before: < margin, unscaled."""
    with np.errstate(invalid="ignore"):
        d = field_values(params, h, w)
        gap = np.abs((d - np.floor(d)) - 0.5)
        wide = ~(np.abs(d) < 30000.0)
        if fixed_margin is not None:
            return bool(np.any((gap < fixed_margin) | wide))
        scale = tie_scale(params, h, w)
        return bool(any(np.any((gap[c] <= TIE_REL * scale[c]) | wide[c]) for c in (0, 1)))


def flags_np(params, h, w, solve_flags=0, flag_bit=1, fixed_margin=None):
    """The flag word k_solve3 leaves for a pair whose thread 0 returned (params, solve_flags)."""
    return int(solve_flags) | (flag_bit if tie_flag(params, h, w, fixed_margin) else 0)


def device_np(sums15, h, w, project=False, fixed_margin=None):
    """params_np + flags_np -> (params, flags): the whole kernel for one pair."""
    p, bad = params_np(sums15, project)
    return p, flags_np(p, h, w, bad, 1, fixed_margin)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def solve3_exact(F, S):
    """The same system in exact rational arithmetic, rounded once at the end -> float64[3], or None if det F = 0."""
    a = [[Fraction(float(v)) for v in row] for row in np.asarray(F, dtype=np.float64).reshape(3, 3)]
    b = [Fraction(float(v)) for v in np.asarray(S, dtype=np.float64).reshape(3)]

    def det(m):
        return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    d = det(a)
    if d == 0:
        return None
    x = []
    for k in range(3):                                     # Cramer's rule
        m = [[b[r] if c == k else a[r][c] for c in range(3)] for r in range(3)]
        x.append(float(det(m) / d))
    return np.array(x)


def params_exact(sums15, project=False):
    s = np.asarray(sums15, dtype=np.float64).reshape(15)
    ax, ay = solve3_exact(s[:9], s[9:12]), solve3_exact(s[:9], s[12:15])
    if ax is None:
        return None
    p = np.concatenate([ax, ay])
    return p * [2, 1, 1, 2, 1, 1] if project else p


def params_host(sums15, project=False):
    """The host path: oracle.solve_parameters (inv(F) @ S through LAPACK) and the projection.  Raises LinAlgError as it does."""
    from oracle import gme_oracle
    s = np.asarray(sums15, dtype=np.float64).reshape(15)
    p = np.asarray(gme_oracle.solve_parameters(s[:9].reshape(3, 3), s[9:12].copy(), s[12:15].copy()), dtype=np.float64)
    return gme_oracle.project_parameters(p) if project else p


# ---------------------------------------------------------------------------------------------------------------------
# contract predicates
# ---------------------------------------------------------------------------------------------------------------------
def m_k(h, w):
    return np.array([1.0, h - 1, w - 1])


def scaled_errors(dev, host, h, w):
    """|dev - host| m_k / max(1, sum_k |host_k| m_k), float64[6]."""
    dev, host = np.asarray(dev, np.float64).reshape(6), np.asarray(host, np.float64).reshape(6)
    m = m_k(h, w)
    out = np.empty(6)
    for slots in (DX, DY):
        scale = max(1.0, float((np.abs(host[slots]) * m).sum()))
        out[slots] = np.abs(dev[slots] - host[slots]) * m / scale
    return out


def contract_violations(dev, host, h, w):
    """Pairs / slots where |dev - host| m_k > 1e-10 max(1, sum over the displacement's three terms of |host| m_k)."""
    dev, host = np.atleast_2d(dev), np.atleast_2d(host)
    bad = []
    for p in range(len(dev)):
        e = scaled_errors(dev[p], host[p], h, w)
        bad += [(p, int(k), float(e[k])) for k in np.nonzero(~(e <= 1e-10))[0]]
    return bad


def clear_of_ties(params, h, w, rel=1e-8):
    """The h x w field of `params` keeps rel max(1, S) away from every k + 0.5: there an unflagged device solve is required;
    closer, a flag is legitimate."""
    d = field_values(params, h, w)
    scale = tie_scale(params, h, w)
    gap = np.abs((d - np.floor(d)) - 0.5)
    return bool(all(gap[c].min() > rel * scale[c] for c in (0, 1)))


# ---------------------------------------------------------------------------------------------------------------------
# systems
# ---------------------------------------------------------------------------------------------------------------------
def inliers(family, h, w, rng):
    """bool[h, w]: the blocks that enter the sums."""
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    keep = np.zeros((h, w), bool)
    if family == "all":
        keep[:] = True
    elif family == "random70":
        keep.ravel()[rng.permutation(h * w)[:max(3, int(0.7 * h * w))]] = True
        keep[0, 0] = keep[h - 1, 0] = keep[0, w - 1] = True
    elif family == "band":
        keep = np.abs(j - i * (w - 1) / max(h - 1, 1)) <= 1.5
    elif family == "last2cols":
        keep = j >= w - 2
    elif family == "last2rows":
        keep = i >= h - 2
    elif family == "corner4x4":
        keep = (i >= h - 4) & (j >= w - 4)
    elif family == "three":
        while True:
            pts = [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(3)]
            (a, b), (c, d), (e, f) = pts
            if (c - a) * (f - b) - (d - b) * (e - a) != 0:
                break
        for pt in pts:
            keep[pt] = True
    elif family == "column":
        keep = j == 0
    elif family == "row":
        keep = i == 0
    elif family == "block":
        keep[0, 0] = True
    elif family == "collinear":
        keep[:3, 0] = True
    elif family == "column_off":
        keep = j == w - 2
    elif family == "row_off":
        keep = i == h - 2
    elif family != "none":
        raise ValueError(family)
    return keep


def _seq_sum(terms):
    """A sequential float64 sum, first term first (k_fit_level's chains)."""
    return float(np.cumsum(np.asarray(terms, dtype=np.float64))[-1]) if len(terms) else 0.0


def moments(keep, h, w):
    """F of the inliers in k_fit_level's discipline (helpers.COracle.fit_level, oracle.normal_sums): row-major inlier order,
    F[a][b] += (v_a v_b) weight with v = (1, 4 i, 4 j)."""
    i, j = np.nonzero(keep)
    v = [np.ones(len(i)), 4.0 * i, 4.0 * j]
    wgt = 1 / ((h * BS) * (w * BS))
    return np.array([[_seq_sum((v[a] * v[b]) * wgt) for b in range(3)] for a in range(3)])


def sums_of_params(F, p):
    """S = F p, the products of a row summed left to right -> sums15."""
    F = np.asarray(F, dtype=np.float64)
    p = [float(v) for v in p]
    rows = [[float(v) for v in r] for r in F]
    s = [(r[0] * p[o] + r[1] * p[o + 1]) + r[2] * p[o + 2] for o in (0, 3) for r in rows]
    return np.concatenate([F.reshape(9), s])


def sums_of_vectors(keep, h, w, p, rng):
    """k_fit_level's sums over integer vectors rint(field(p)) + {-1, 0, 1} on the inliers -> sums15."""
    i, j = np.nonzero(keep)
    v = [np.ones(len(i)), 4.0 * i, 4.0 * j]
    wgt = 1 / ((h * BS) * (w * BS))
    gt = rounded_field(p, h, w).reshape(2, h, w)[:, i, j] + rng.integers(-1, 2, (2, len(i)))
    s = [_seq_sum((v[a] * gt[c]) * wgt) for c in (0, 1) for a in range(3)]
    return np.concatenate([moments(keep, h, w).reshape(9), s])


class System:
    __slots__ = ("name", "family", "h", "w", "project", "sums", "translation", "form")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    @property
    def well_spread(self):
        return self.family in WELL_SPREAD


def _draw_params(rng, t):
    slopes = rng.normal(0.0, 0.02, 4)
    return np.array([t + rng.uniform(-0.2, 0.2), slopes[0], slopes[1], -0.8 * t + rng.uniform(-0.2, 0.2), slopes[2], slopes[3]])


_catalogue = None


def catalogue():
    """The seeded systems, built once: every shape x family x signed translation x the two ways to form the sums, then the
    singular and the near-singular sets.  Every second system is solved under `project`.  A well-spread system is redrawn (up
    to 40 times, same generator) until its exact solution keeps 4e-8 max(1, S) away from every tie, so that at least nine in
    ten are clear of ties whatever the LAPACK build; the ill-conditioned families are taken as they come."""
    global _catalogue
    if _catalogue is not None:
        return _catalogue
    out = []
    n = 0
    for h, w in SHAPES:
        for family in FAMILIES + SINGULAR + NEAR_SINGULAR:
            rng = np.random.default_rng([h, w, (FAMILIES + SINGULAR + NEAR_SINGULAR).index(family)])
            keep = inliers(family, h, w, rng)
            F = moments(keep, h, w)
            plain = family in FAMILIES
            for t in (TRANSLATIONS if plain else TRANSLATIONS[1:2]):
                for sign in (1.0, -1.0):
                    for form in ("Fp", "vectors"):
                        project = n % 2 == 1
                        n += 1
                        for _ in range(40):
                            p = _draw_params(rng, sign * t)
                            sums = sums_of_params(F, p) if form == "Fp" else sums_of_vectors(keep, h, w, p, rng)
                            if family not in WELL_SPREAD:
                                break
                            exact = params_exact(sums, project)
                            if clear_of_ties(exact, h, w, 4e-8):
                                break
                        out.append(System(name="%dx%d-%s-%+.1f-%s%s" % (h, w, family, sign * t, form, "-proj" if project else ""),
                                          family=family, h=h, w=w, project=project, sums=sums, translation=sign * t, form=form))
    _catalogue = out
    return out


def groups(systems):
    """{(h, w, project): [systems]} in first-seen order: one device call each."""
    out = {}
    for s in systems:
        out.setdefault((s.h, s.w, s.project), []).append(s)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rounding traps
# ---------------------------------------------------------------------------------------------------------------------
TRAP_FAMILIES = [                      # (name, h, w, inlier family, translation)
    ("2160p-last2cols-20", 135, 240, "last2cols", 20.0),
    ("1080p-last2cols-500", 67, 120, "last2cols", 500.3),
    ("1080p-corner4x4-500", 67, 120, "corner4x4", 500.3),
    ("480x720-last2cols-500", 30, 45, "last2cols", 500.3),
]


def trap_search(h, w, family, translation, tries, seed, solve=None, fixed_margin=1e-9):
    """Systems S = F p whose p0 was moved so that the block where the device and the host fields differ most sits on a
    rounding tie between the two.  Yields a dict per try: sums, the restated parameters, `differs` (the rounded fields of the
    restated and the host solution differ), `old_flags` (the flag word under the fixed margin, without flag 8), `spread`
    (that block's |d_dev - d_host|).  A trap is a try with differs and old_flags == 0.  `solve(sums15)` restates the device
    (default: the plain elimination the kernel had when the fixed margin shipped)."""
    rng = np.random.default_rng(seed)
    keep = inliers(family, h, w, rng)
    F = moments(keep, h, w)
    solve = solve or (lambda s: _params_plain(s))
    for _ in range(tries):
        p = _draw_params(rng, translation if rng.integers(0, 2) else -translation)
        sums = sums_of_params(F, p)
        try:
            dd, dh = field_values(solve(sums), h, w), field_values(params_host(sums), h, w)
        except np.linalg.LinAlgError:
            continue
        c, b = np.unravel_index(np.argmax(np.abs(dd - dh)), dd.shape)
        mid = 0.5 * (dd[c, b] + dh[c, b])
        p[3 * c] += (math.floor(mid) + 0.5) - mid
        sums = sums_of_params(F, p)
        dev = solve(sums)
        try:
            host = params_host(sums)
        except np.linalg.LinAlgError:
            continue
        dd, dh = field_values(dev, h, w), field_values(host, h, w)
        yield dict(sums=sums, params=dev, differs=not np.array_equal(np.rint(dd), np.rint(dh)),
                   old_flags=flags_np(dev, h, w, 0, 1, fixed_margin), spread=float(np.abs(dd - dh)[c, b]))


def _params_plain(sums15):
    """k_solve3 as it was with the fixed margin: the elimination of solve3_np without the equilibration."""
    s = np.asarray(sums15, dtype=np.float64).reshape(15)
    ax, ay = solve3_np(s[:9], s[9:12], False)[0], solve3_np(s[:9], s[12:15], False)[0]
    return np.zeros(6) if ax is None or ay is None else np.array(ax + ay)


# ---------------------------------------------------------------------------------------------------------------------
# second-order sums over any inlier set, and the frames of the end-to-end test
# ---------------------------------------------------------------------------------------------------------------------
def sums_of_field2(params12, h, w, keep):
    """sums_of_field of tests/test_gpu_models2_solve.py (the 27 order-2 sums of a field with the float64 displacements of
    `params12`, x = 4 i, y = 4 j, weight 1 / (H W)) over the blocks of the mask `keep` instead of whole block columns."""
    from test_gpu_models2_solve import DX as DX2, DY as DY2, MOMENTS, PHI
    i, j = np.nonzero(keep)
    x, y = 4.0 * i, 4.0 * j
    wgt = 1.0 / (h * BS * w * BS)
    phi = np.stack([x ** a * y ** b for a, b in PHI], axis=1)
    p = np.asarray(params12, np.float64)
    dx, dy = phi @ p[DX2], phi @ p[DY2]
    mono = np.stack([x ** a * y ** b for a, b in MOMENTS], axis=1)
    return np.concatenate([(mono * wgt).sum(0), (phi * dx[:, None] * wgt).sum(0), (phi * dy[:, None] * wgt).sum(0)])


LARGE_SHIFTS = ((13, -9), (-18, 7))


def large_motion_frames(shift, count=4, H=96, W=128):
    """uint8[count, H, W]: hier_cases.pair's texture moving by `shift` (column, row) per frame, cut with the smallest margin
    that holds count - 1 steps of either of LARGE_SHIFTS.  The level-1 fit of so small a frame has 3 x 4 blocks of integer
    vectors and its doubled solution often lands on a tie exactly, a legitimate flag: test_solve3_host.py checks that these
    frames have none."""
    import hier_cases
    margin = (count - 1) * max(abs(v) for s in LARGE_SHIFTS for v in s)
    return np.stack([hier_cases.pair(H, W, (t * shift[0], t * shift[1]), margin=margin)[1] for t in range(count)])
