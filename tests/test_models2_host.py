"""Second-order motion models (roadmap.py: bilinear, pseudo_perspective, quadratic) on the host: the solves against
np.linalg.lstsq on the block vectors, the reduction of the 27 order-2 sums to the 15 affine sums, batch == per-pair,
errors, the projection rule, the CLI and the new kernels' resource remarks.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (p, q) of the 15 moments in the order of the 27 sums
MOMENTS = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3), (4, 0), (3, 1), (2, 2), (1, 3), (0, 4)]
PHI = [(0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2)]


def sums27(x, y, dx, dy, w):
    """The 27 sums as the device forms them: each term (exact integer) * w rounded once, each entry a sequential float64
    sum (np.cumsum) in list order."""
    x, y, dx, dy = (np.asarray(a, np.float64) for a in (x, y, dx, dy))
    cols = [x ** p * y ** q for p, q in MOMENTS]
    cols += [x ** p * y ** q * dx for p, q in PHI]
    cols += [x ** p * y ** q * dy for p, q in PHI]
    out = np.zeros(27)
    for k, c in enumerate(cols):
        out[k] = np.cumsum(c * w)[-1] if len(c) else 0.0
    return out


def affine15(x, y, dx, dy, w):
    """The 15 sums of k_fit_level (F 3x3 | Sx | Sy), same discipline."""
    x, y, dx, dy = (np.asarray(a, np.float64) for a in (x, y, dx, dy))
    va = [np.ones_like(x), x, y]
    out = [np.cumsum(va[a] * va[b] * w)[-1] for a in range(3) for b in range(3)]
    out += [np.cumsum(va[a] * dx * w)[-1] for a in range(3)]
    out += [np.cumsum(va[a] * dy * w)[-1] for a in range(3)]
    return np.array(out)


def field(h, w, seed, coef, noise=0.7, keep=0.8):
    """Block vectors of an h x w grid that follow the quadratic field `coef` (params12 layout, fit coordinates x = 4 i,
    y = 4 j) plus rounding and noise; a random subset plays the inliers."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x, y = 4.0 * i.ravel(), 4.0 * j.ravel()
    phi = np.stack([x ** p * y ** q for p, q in PHI], 1)
    c = np.asarray(coef, np.float64)
    dx = np.rint(phi @ c[[0, 1, 2, 6, 7, 8]] + rng.normal(0, noise, len(x)))
    dy = np.rint(phi @ c[[3, 4, 5, 9, 10, 11]] + rng.normal(0, noise, len(x)))
    sel = rng.random(len(x)) < keep
    return x[sel], y[sel], dx[sel], dy[sel]


COEF = [3.0, 0.02, -0.015, -2.0, 0.01, 0.03, 2e-5, -1.5e-5, 1e-5, -1e-5, 2.5e-5, -2e-5]
GRIDS = {"720p": (45, 80, 1.0 / (720 * 1280)), "1080p": (67, 120, 1.0 / (1080 * 1920))}


def design(model, x, y):
    """Rows of the least-squares problem for [dx; dy] and the map from its unknowns to params12."""
    one, z = np.ones_like(x), np.zeros_like(x)
    if model == "quadratic":
        Ax = np.stack([one, x, y, x * x, x * y, y * y], 1)
        return Ax, [0, 1, 2, 6, 7, 8]
    if model == "bilinear":
        Ax = np.stack([one, x, y, x * y], 1)
        return Ax, [0, 1, 2, 7]
    raise AssertionError(model)


def lstsq_params(model, x, y, dx, dy):
    out = np.zeros(12)
    if model == "pseudo_perspective":
        rx = np.stack([np.ones_like(x), x, y, 0 * x, 0 * x, 0 * x, y * y, x * y], 1)
        ry = np.stack([0 * x, 0 * x, 0 * x, np.ones_like(x), x, y, x * y, x * x], 1)
        th = np.linalg.lstsq(np.concatenate([rx, ry]), np.concatenate([dx, dy]), rcond=None)[0]
        out[:6] = th[:6]
        out[7] = out[9] = th[7]
        out[8] = out[10] = th[6]
        return out
    A, slots = design(model, x, y)
    tx = np.linalg.lstsq(A, dx, rcond=None)[0]
    ty = np.linalg.lstsq(A, dy, rcond=None)[0]
    for c, s in enumerate(slots):
        out[s], out[s + 3] = tx[c], ty[c]
    return out


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("model", ["bilinear", "pseudo_perspective", "quadratic"])
def test_second_order_solves_equal_lstsq(grid, model):
    import roadmap
    h, w, wgt = GRIDS[grid]
    rows, vecs = [], []
    for seed in range(3):
        v = field(h, w, seed, COEF)
        vecs.append(v)
        rows.append(sums27(*v, wgt))
    got = roadmap.solve_model(np.array(rows), model)
    assert got.shape == (3, 12)
    for k, v in enumerate(vecs):
        want = lstsq_params(model, *v)
        np.testing.assert_allclose(got[k], want, rtol=1e-8, atol=1e-12 * np.abs(want).max())
    if model == "bilinear":
        assert np.all(got[:, [6, 8, 9, 11]] == 0)
    if model == "pseudo_perspective":
        assert np.all(got[:, 6] == 0) and np.all(got[:, 11] == 0)
        assert np.array_equal(got[:, 7], got[:, 9]) and np.array_equal(got[:, 8], got[:, 10])


def test_quadratic_recovers_noise_free_field():
    import roadmap
    h, w, wgt = GRIDS["720p"]
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x, y = 4.0 * i.ravel(), 4.0 * j.ravel()
    c = np.array([2.0, 0.25, -0.5, -1.0, 0.5, 0.25, 1 / 16, -1 / 32, 1 / 64, 1 / 32, 1 / 16, -1 / 64])
    dx = c[0] + c[1] * x + c[2] * y + c[6] * x * x + c[7] * x * y + c[8] * y * y          # exact dyadic values
    dy = c[3] + c[4] * x + c[5] * y + c[9] * x * x + c[10] * x * y + c[11] * y * y
    got = roadmap.solve_model(sums27(x, y, dx, dy, wgt), "quadratic")[0]
    np.testing.assert_allclose(got, c, rtol=1e-7, atol=1e-10)


def test_affine_sums_reduce_exactly():
    import motion
    import roadmap
    for grid, (h, w, wgt) in GRIDS.items():
        s27, s15 = [], []
        for seed in range(4):
            v = field(h, w, 10 + seed, COEF)
            s27.append(sums27(*v, wgt))
            s15.append(affine15(*v, wgt))
        s27, s15 = np.array(s27), np.array(s15)
        red = roadmap.affine_sums(s27)
        assert red.shape == (4, 15) and np.array_equal(red, s15), grid
        want = motion._solve_batch(s15)
        assert np.array_equal(roadmap.solve_model(red, "affine"), want)
        assert np.array_equal(roadmap.solve_model(s27, "affine"), want)          # 27-wide sums reduce on their own
        for m in ("translation", "similarity"):
            assert np.array_equal(roadmap.solve_model(s27, m), roadmap.solve_model(s15, m))


@pytest.mark.parametrize("model", ["bilinear", "pseudo_perspective", "quadratic"])
def test_batch_solve_equals_per_pair(model):
    import roadmap
    h, w, wgt = GRIDS["1080p"]
    rows = np.array([sums27(*field(h, w, 20 + k, COEF, keep=0.5 + 0.05 * k), wgt) for k in range(7)])
    batch = roadmap.solve_model(rows, model)
    for k in range(len(rows)):
        assert np.array_equal(batch[k], roadmap.solve_model(rows[k:k + 1], model)[0])
        assert np.array_equal(batch[k], roadmap.solve_model(rows[k], model)[0])


def test_second_order_errors():
    import roadmap
    h, w, wgt = GRIDS["720p"]
    s27 = sums27(*field(h, w, 3, COEF), wgt)[None]
    for m in ("bilinear", "pseudo_perspective", "quadratic"):
        with pytest.raises(ValueError):
            roadmap.solve_model(roadmap.affine_sums(s27), m)          # 15-wide sums cannot determine second-order terms
        with pytest.raises(np.linalg.LinAlgError):
            roadmap.solve_model(np.zeros((1, 27)), m)                  # no inlier
        one = sums27([8.0], [12.0], [1.0], [2.0], wgt)[None]           # one inlier: rank 1
        with pytest.raises(np.linalg.LinAlgError):
            roadmap.solve_model(one, m)
    with pytest.raises(ValueError):
        roadmap.solve_model(s27, "perspective")                        # the projective model is not offered


def test_projection_rule():
    import roadmap
    rng = np.random.default_rng(5)
    p = rng.normal(size=(4, 12))
    q = roadmap.project(p)
    assert q is not p and np.array_equal(p, p)
    assert np.array_equal(q[:, [0, 3]], 2 * p[:, [0, 3]])
    assert np.array_equal(q[:, [1, 2, 4, 5]], p[:, [1, 2, 4, 5]])
    assert np.array_equal(q[:, 6:], p[:, 6:] / 2)
    # the affine layout: motion.parameter_projection
    import motion
    a = rng.normal(size=6)
    assert np.array_equal(roadmap.project(a), motion.parameter_projection(a.copy()))
    # a field at level 2 evaluated on the doubled coordinates of level 1 (x -> 2x) is the projected field: exact
    x, y = 4.0 * np.arange(7.0), 4.0 * np.arange(5.0)[:, None]
    c = np.array([1.5, 0.25, -0.5, -1.0, 0.5, 0.125, 1 / 16, -1 / 32, 1 / 64, 1 / 32, 1 / 16, -1 / 64])
    f = lambda c, x, y: c[0] + c[1] * x + c[2] * y + c[6] * x * x + c[7] * x * y + c[8] * y * y     # noqa: E731
    assert np.array_equal(f(roadmap.project(c), 2 * x, 2 * y), 2 * f(c, x, y))


def test_cli_accepts_second_order_models(capsys):
    import gme_cli
    import roadmap
    ap = gme_cli._parser()
    for m in ("bilinear", "pseudo_perspective", "quadratic", "affine", "similarity"):
        assert ap.parse_args(["results", "-v", "clip", "--model", m]).model == m
    with pytest.raises(SystemExit):
        ap.parse_args(["results", "-v", "clip", "--model", "perspective"])
    assert set(("bilinear", "pseudo_perspective", "quadratic")) <= set(roadmap.MODELS)
    gme_cli.main(["info"])
    out = capsys.readouterr().out
    for m in ("bilinear", "pseudo_perspective", "quadratic"):
        assert m in out


def test_second_order_kernels_do_not_spill():
    """The compiler's resource remarks (build/*.remarks) for the order-2 kernels: no VGPR spill, no scratch, and LDS that
    leaves room for two workgroups per CU beside the 40 KB inlier list (160 KiB per CU)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = {r["name"]: r for r in resource_table.kernels()}
    assert rows, "no build/*.remarks: make -C global-motion-estimation_amd/csrc"
    hits = [r for k, r in rows.items() if k.startswith("k_fit_level2") or k.startswith("k_model2_field")]
    assert {r["name"].split("<")[0] for r in hits} == {"k_fit_level2", "k_model2_field"}, sorted(rows)
    for r in hits:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    fit2 = [r for r in hits if r["name"].startswith("k_fit_level2")][0]
    assert 2 * (fit2["lds"] + 40 * 1024) <= 160 * 1024, fit2
