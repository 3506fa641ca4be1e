"""The host definition of global motion compensation (gmc.py): argument rules, the global predictor against direct.compensate,
the translation identity, ties, saturated content, unusable warps, the zoom scene and the mode coverage of the noise cases.
No GPU."""
import numpy as np
import pytest

import direct
import gmc
import gmc_cases as gc


def test_check_args():
    assert gmc.check_args(16, 0, 64) == (16, 0, 64)
    assert gmc.check_args(4, 1, 0) == (4, 1, 0)
    assert gmc.check_args(64, 1, 1 << 30) == (64, 1, 1 << 30)
    for bad in ((3, 0, 0), (65, 0, 0), (0, 0, 0), (16, 2, 0), (16, -1, 0), (16, 0, -1), (16, 0, (1 << 30) + 1)):
        with pytest.raises(ValueError):
            gmc.check_args(*bad)
    z = np.zeros((16, 16), np.uint8)
    f = np.zeros((1, 1, 2), np.int32)
    with pytest.raises(ValueError):
        gmc.decide(z, z, direct.IDENTITY, f, 16, 2, 0)
    with pytest.raises(ValueError):
        gmc.decide(z, z, direct.IDENTITY, np.zeros((2, 1, 2), np.int32), 16, 0, 0)
    with pytest.raises(ValueError):
        gmc.decide(z, z, np.zeros(6), f, 16, 0, 0)
    with pytest.raises(TypeError):
        gmc.decide(z, z.astype(np.int16), direct.IDENTITY, f, 16, 0, 0)
    # the largest sum of a decision
    assert (1 << 30) + 64 * 64 * 255 * 255 < 1 << 31
    assert gmc.default_penalty(16, 0) == 64 and gmc.default_penalty(16, 1) == 1024 and gmc.default_penalty(8, 0) == 16
    # a mode that asks for an unavailable predictor
    with pytest.raises(ValueError):
        gmc.predict(z, gc.warp_of("far", 16, 16), np.zeros((1, 1), np.uint8), f, 16)
    with pytest.raises(ValueError):
        gmc.predict(z, direct.IDENTITY, np.ones((1, 1), np.uint8), np.full((1, 1, 2), 1, np.int32), 16)


def brute(ref, cur, h, f, bs, pnorm, penalty, i, j):
    """One block straight from the issue's wording, pixel by pixel in Python floats, written apart from gmc.decide ->
    (mode, cost, [cg, cl])."""
    H, W = cur.shape
    y, x = i * bs, j * bs

    def norm(d):
        return abs(d) if pnorm == 0 else d * d
    cg = -1
    if bool(np.all(np.isfinite(h))) and all((h[6] * u + h[7] * v) + 1.0 > 0.0 for u in (0.0, W - 1.0) for v in (0.0, H - 1.0)):
        cg = 0
        for v in range(y, y + bs):
            for u in range(x, x + bs):
                d = (h[6] * u + h[7] * v) + 1.0
                up, vp = ((h[0] * u + h[1] * v) + h[2]) / d, ((h[3] * u + h[4] * v) + h[5]) / d
                if not (0.0 <= up <= W - 1.0 and 0.0 <= vp <= H - 1.0):
                    cg = -1
                    break
                x0, y0 = int(np.floor(up)), int(np.floor(vp))
                ax, ay, x1, y1 = up - x0, vp - y0, min(x0 + 1, W - 1), min(y0 + 1, H - 1)
                top = (1.0 - ax) * float(ref[y0, x0]) + ax * float(ref[y0, x1])
                bot = (1.0 - ax) * float(ref[y1, x0]) + ax * float(ref[y1, x1])
                cg += norm(int(np.floor(((1.0 - ay) * top + ay * bot) + 0.5)) - int(cur[v, u]))
            if cg < 0:
                break
    cl = -1
    vx, vy = int(f[i, j, 0]), int(f[i, j, 1])
    if x + vx >= 0 and y + vy >= 0 and x + vx + bs <= W and y + vy + bs <= H:
        cl = sum(norm(int(ref[v + vy, u + vx]) - int(cur[v, u])) for v in range(y, y + bs) for u in range(x, x + bs))
    mode, best = 2, -1
    if cg >= 0:
        mode, best = 0, cg
    if cl >= 0 and (mode == 2 or cl + penalty < best):
        mode, best = 1, cl + penalty
    return mode, best, [cg, cl]


@pytest.mark.parametrize("case", gc.NOISE)
def test_noise(case):
    """Under every warp and both norms: the modes the warp must produce occur (gmc_cases.required_modes), shapes and types are
    the documented ones, cost and costs agree with mode; under three of the warps every block equals a second writing of the
    definition."""
    (H, W), bs = case
    hb, wb = H // bs, W // bs
    ref, cur, _ = gc.noise_pair(case)
    for name in gc.WARPS:
        h, f = gc.noise_field(case, name)
        for pnorm in (0, 1):
            penalty = gmc.default_penalty(bs, pnorm)
            mode, cost, costs = gc.noise_result(case, name, pnorm)
            assert (mode.dtype, cost.dtype, costs.dtype) == (np.uint8, np.int64, np.int64)
            assert mode.shape == cost.shape == (hb, wb) and costs.shape == (hb, wb, 2)
            gc.check_modes(name, mode)
            assert np.all((cost == -1) == (mode == 2)) and np.all((mode == 2) == np.all(costs == -1, axis=2))
            assert np.all(cost[mode == 0] == costs[mode == 0, 0]) and np.all(cost[mode == 1] == costs[mode == 1, 1] + penalty)
            if name in ("far", "unusable", "nan"):
                assert np.all(costs[:, :, 0] == -1)
            if name in ("identity", "rotzoom", "projective") and bs <= 24:
                for i in range(hb):
                    for j in range(wb):
                        assert brute(ref, cur, h, f, bs, pnorm, penalty, i, j) == (mode[i, j], cost[i, j], list(costs[i, j])), (name, i, j)


@pytest.mark.parametrize("name", ("identity", "fractional", "rotzoom", "projective"))
def test_global_pixels_are_compensate(name):
    """g on fully valid blocks is direct.compensate's output there; where g does not exist compensate keeps the ref pixel."""
    case = gc.NOISE[3]
    (H, W), bs = case
    ref, cur, _ = gc.noise_pair(case)
    h = gc.warp_of(name, H, W)
    g, exists = gmc.global_pixels(ref, h)
    comp = direct.compensate(ref, cur, h)[0]
    assert np.array_equal(g[exists], comp[exists]) and np.array_equal(comp[~exists], ref[~exists])
    mode, cost, costs = gmc.decide(ref, cur, h, np.zeros((H // bs, W // bs, 2), np.int32), bs, 1, 0)
    pred = gmc.predict(ref, h, gmc.all_mode(costs, 0), np.zeros((H // bs, W // bs, 2), np.int32), bs)
    seen = 0
    for i in range(H // bs):
        for j in range(W // bs):
            win = (slice(i * bs, (i + 1) * bs), slice(j * bs, (j + 1) * bs))
            assert (costs[i, j, 0] >= 0) == bool(exists[win].all())
            if costs[i, j, 0] >= 0:
                seen += 1
                assert np.array_equal(pred[win], comp[win]) and costs[i, j, 0] == gmc.sse(comp[win], cur[win])
            else:
                assert np.array_equal(pred[win], ref[win])
    assert seen > 0


@pytest.mark.parametrize("tx,ty", ((0, 0), (3, -2), (-5, 4)))
def test_translation_identity(tx, ty):
    """With h = [1, 0, tx, 0, 1, ty, 0, 0] for integers tx, ty and f = (tx, ty) everywhere, cg == cl wherever both exist, and the
    all-global and the all-local prediction agree on those blocks."""
    case = gc.NOISE[3]
    (H, W), bs = case
    ref, cur, _ = gc.noise_pair(case)
    h = np.array([1.0, 0.0, tx, 0.0, 1.0, ty, 0.0, 0.0])
    f = np.empty((H // bs, W // bs, 2), np.int32)
    f[:] = (tx, ty)
    for pnorm in (0, 1):
        mode, cost, costs = gmc.decide(ref, cur, h, f, bs, pnorm, 0)
        both = (costs[:, :, 0] >= 0) & (costs[:, :, 1] >= 0)
        assert both.any() and np.array_equal(costs[both, 0], costs[both, 1]) and np.all(mode[both] == 0)
        pg = gmc.predict(ref, h, gmc.all_mode(costs, 0), f, bs)
        pl = gmc.predict(ref, h, gmc.all_mode(costs, 1), f, bs)
        for i, j in np.argwhere(both):
            win = (slice(i * bs, (i + 1) * bs), slice(j * bs, (j + 1) * bs))
            assert np.array_equal(pg[win], pl[win])


def test_ties():
    """Constant frames at penalty 0: every block with both candidates is GLOBAL."""
    ref, cur = gc.ties_frames()
    rng = np.random.default_rng(5)
    for bs in (8, 16):
        f = rng.integers(-2, 3, size=(37 // bs, 53 // bs, 2)).astype(np.int32)
        for name in ("identity", "fractional", "rotzoom"):
            for pnorm in (0, 1):
                mode, cost, costs = gmc.decide(ref, cur, gc.warp_of(name, 37, 53), f, bs, pnorm, 0)
                both = (costs[:, :, 0] >= 0) & (costs[:, :, 1] >= 0)
                assert both.any() and np.all(mode[both] == 0) and np.array_equal(costs[both, 0], costs[both, 1])
                assert np.all(mode[(costs[:, :, 0] < 0) & (costs[:, :, 1] >= 0)] == 1)


def test_saturated():
    """Blocks of 64 on frames of 0 and 255 under MSE at penalty 2^30: no sum reaches 2^31, and the values are those of a plain
    int64 evaluation."""
    lo, hi = np.zeros((130, 135), np.uint8), np.full((130, 135), 255, np.uint8)
    f = np.zeros((2, 2, 2), np.int32)
    top = 64 * 64 * 255 * 255
    assert top + (1 << 30) < 1 << 31
    mode, cost, costs = gmc.decide(lo, hi, direct.IDENTITY, f, 64, 1, 1 << 30)
    assert np.all(mode == 0) and np.all(cost == top) and np.all(costs == top)
    mode, cost, costs = gmc.decide(lo, hi, gc.warp_of("far", 130, 135), f, 64, 1, 1 << 30)
    assert np.all(mode == 1) and np.all(cost == top + (1 << 30)) and np.all(costs == (-1, top))
    mode, cost, costs = gmc.decide(lo, hi, direct.IDENTITY, f, 64, 0, 1 << 30)
    assert np.all(mode == 0) and np.all(cost == 64 * 64 * 255)


@pytest.mark.parametrize("name", ("unusable", "nan", "inf"))
def test_unusable_warp(name):
    """No global candidate, no exception: the decision is the local one or none, and predict with those modes works."""
    case = gc.NOISE[2]
    (H, W), bs = case
    ref, cur, f = gc.noise_pair(case)
    h = np.array([1.0, 0.0, 0.0, 0.0, float("inf"), 0.0, 0.0, 0.0]) if name == "inf" else gc.warp_of(name, H, W)
    assert not gmc.usable(h, H, W) and gmc.usable(direct.IDENTITY, H, W)
    mode, cost, costs = gmc.decide(ref, cur, h, f, bs, 0, 64)
    assert np.all(costs[:, :, 0] == -1) and set(np.unique(mode).tolist()) <= {1, 2} and np.all((mode == 1) == (costs[:, :, 1] >= 0))
    pred = gmc.predict(ref, h, mode, f, bs)
    assert pred.shape == ref.shape and pred.dtype == np.uint8


@pytest.mark.parametrize("pnorm", (0, 1))
def test_zoom_scene(pnorm):
    """The mode map, the blocks without a global candidate and the patch's vector (gmc_cases.check_scene); the chosen prediction
    is no worse than either single-predictor one under MSE costs."""
    ref, cur, h = gc.zoom_scene()
    f, mode, cost, costs = gc.scene_result(pnorm)
    assert gmc.default_penalty(16, pnorm) == (64, 1024)[pnorm]
    gc.check_scene(f, mode, costs)
    H, W = cur.shape
    s = [gmc.sse(cur, gmc.predict(ref, h, gmc.all_mode(costs, which), f, 16)) for which in (0, 1)]
    chosen = gmc.sse(cur, gmc.predict(ref, h, mode, f, 16))
    rep = gmc.summary(mode, s[0], s[1], chosen, H, W)
    assert abs(sum(rep["mode_share"]) - 1.0) < 1e-12 and rep["mode_share"][0] == 40.0 / 48.0 and rep["mode_share"][2] == 0.0
    assert rep["psnr_chosen"] > rep["psnr_global"]
