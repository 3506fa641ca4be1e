"""The host definition of bidirectional block prediction (bipred.py): argument rules, noise with arbitrary fields, the cases
without refinement, the identity that ties decide to predict, and the occlusion scene.  No GPU."""
import numpy as np
import pytest

import bipred
import bipred_cases as bc


def test_check_args():
    assert bipred.check_args(16, 1, 1, 0, 64) == (16, 1, 1, 0, 64)
    assert bipred.check_args(4, 0, 0, 1, 0) == (4, 0, 0, 1, 0)
    assert bipred.check_args(64, 2, 2, 1, 1 << 30) == (64, 2, 2, 1, 1 << 30)
    for bad in ((3, 1, 1, 0, 0), (65, 1, 1, 0, 0), (0, 1, 1, 0, 0), (16, -1, 1, 0, 0), (16, 3, 1, 0, 0), (16, 1, -1, 0, 0),
                (16, 1, 3, 0, 0), (16, 1, 1, 2, 0), (16, 1, 1, -1, 0), (16, 1, 1, 0, -1), (16, 1, 1, 0, (1 << 30) + 1)):
        with pytest.raises(ValueError):
            bipred.check_args(*bad)
    z = np.zeros((16, 16), np.uint8)
    f = np.zeros((1, 1, 2), np.int32)
    with pytest.raises(ValueError):
        bipred.decide(z, z, z, f, f, 16, 3, 1, 0, 0)
    with pytest.raises(ValueError):
        bipred.decide(z, z, z, np.zeros((2, 1, 2), np.int32), f, 16, 1, 1, 0, 0)
    with pytest.raises(TypeError):
        bipred.decide(z, z.astype(np.int16), z, f, f, 16, 1, 1, 0, 0)
    # the largest sum of a decision
    assert (1 << 30) + 64 * 64 * 255 * 255 < 1 << 31
    assert bipred.default_penalty(16, 0) == 64 and bipred.default_penalty(16, 1) == 1024 and bipred.default_penalty(8, 0) == 16


def brute(past, mid, nxt, f0, f1, bs, r, rounds, pnorm, penalty, i, j):
    """One block straight from the issue's wording, written apart from bipred.decide -> (mode, v0, v1, cost, costs)."""
    H, W = mid.shape
    y, x = i * bs, j * bs
    blk = mid[y:y + bs, x:x + bs].astype(np.int64)

    def at(frame, v):
        if x + v[0] < 0 or y + v[1] < 0 or x + v[0] + bs > W or y + v[1] + bs > H:
            return None
        return frame[y + v[1]:y + v[1] + bs, x + v[0]:x + v[0] + bs].astype(np.int64)

    def norm(d):
        return int(np.abs(d).sum()) if pnorm == 0 else int((d ** 2).sum())
    a, b = tuple(int(t) for t in f0[i, j]), tuple(int(t) for t in f1[i, j])
    pa, nb = at(past, a), at(nxt, b)
    c = [-1, -1, -1]
    if pa is not None:
        c[0] = norm(pa - blk)
    if nb is not None:
        c[1] = norm(nb - blk)
    if pa is not None and nb is not None:
        c[2] = norm(((pa + nb + 1) >> 1) - blk)
        for _ in range(rounds):
            for side in (0, 1):
                centre = a if side == 0 else b
                for ox in range(-r, r + 1):
                    for oy in range(-r, r + 1):
                        if ox == 0 and oy == 0:
                            continue
                        v = (centre[0] + ox, centre[1] + oy)
                        pa2, nb2 = (at(past, v), at(nxt, b)) if side == 0 else (at(past, a), at(nxt, v))
                        if pa2 is None or nb2 is None:
                            continue
                        cost = norm(((pa2 + nb2 + 1) >> 1) - blk)
                        if cost < c[2]:
                            c[2] = cost
                            if side == 0:
                                a = v
                            else:
                                b = v
    mode, best = 3, -1
    for m, value in ((0, c[0]), (1, c[1]), (2, c[2] + penalty)):
        if c[m] >= 0 and (mode == 3 or value < best):
            mode, best = m, value
    if mode != 2:
        a, b = tuple(int(t) for t in f0[i, j]), tuple(int(t) for t in f1[i, j])
    return mode, a, b, best, c


@pytest.mark.parametrize("case", bc.NOISE)
def test_noise(case):
    """Every mode occurs at the case's penalty in both norms, the listed cases move some pair, the radius-0 and rounds-0 cases
    move none, every block equals a second writing of the definition, and shapes and types are the documented ones."""
    shape, bs, r, rounds = case
    past, mid, nxt, f0, f1 = bc.noise_triple(case)
    hb, wb = shape[0] // bs, shape[1] // bs
    for pnorm in (0, 1):
        penalty = bc.PENALTY[case, pnorm]
        mode, v0, v1, cost, costs = bc.noise_result(case, pnorm)
        assert (mode.dtype, v0.dtype, v1.dtype, cost.dtype, costs.dtype) == (np.uint8, np.int32, np.int32, np.int64, np.int64)
        assert mode.shape == (hb, wb) and v0.shape == v1.shape == (hb, wb, 2) and cost.shape == (hb, wb) and costs.shape == (hb, wb, 3)
        assert set(np.unique(mode).tolist()) == {0, 1, 2, 3}, np.unique(mode)
        moved = np.any(v0 != f0, axis=2) | np.any(v1 != f1, axis=2)
        assert not moved[mode != 2].any()
        if case in bc.REFINED:
            assert moved.any()
        if r == 0 or rounds == 0:
            assert not moved.any()
        assert np.all((cost == -1) == (mode == 3)) and np.all((costs[:, :, 2] >= 0) == ((costs[:, :, 0] >= 0) & (costs[:, :, 1] >= 0)))
        for i in range(hb):
            for j in range(wb):
                m, a, b, best, c = brute(past, mid, nxt, f0, f1, bs, r, rounds, pnorm, penalty, i, j)
                assert (m, a, b, best, c) == (mode[i, j], tuple(v0[i, j]), tuple(v1[i, j]), cost[i, j], list(costs[i, j])), (i, j)


def test_refinement_moves_pairs_without_penalty():
    """What the two listed cases were first seen to do: at penalty 0 some refined pair differs from the input."""
    for case in bc.REFINED:
        shape, bs, r, rounds = case
        past, mid, nxt, f0, f1 = bc.noise_triple(case)
        mode, v0, v1, cost, costs = bipred.decide(past, mid, nxt, f0, f1, bs, r, rounds, 0, 0)
        assert np.any(v0 != f0) or np.any(v1 != f1)
        plain = bipred.decide(past, mid, nxt, f0, f1, bs, 0, rounds, 0, 0)
        assert np.all(costs[:, :, 2] <= plain[4][:, :, 2]) and np.any(costs[:, :, 2] < plain[4][:, :, 2])


@pytest.mark.parametrize("r,rounds", ((0, 0), (0, 2), (2, 0)))
def test_no_refinement(r, rounds):
    case = bc.NOISE[5]
    past, mid, nxt, f0, f1 = bc.noise_triple(case)
    for pnorm in (0, 1):
        mode, v0, v1, cost, costs = bipred.decide(past, mid, nxt, f0, f1, case[1], r, rounds, pnorm, 0)
        assert np.array_equal(v0, f0) and np.array_equal(v1, f1)


@pytest.mark.parametrize("case", bc.NOISE)
def test_decide_and_predict_agree(case):
    """Under MSE the squared error of predict over the whole blocks is the sum over the blocks of mode <= 2 of cost minus the
    penalty where the mode is 2, plus the co-located past error of the blocks of mode 3; beyond the last whole block the
    predicted frame is the past one."""
    shape, bs, r, rounds = case
    past, mid, nxt, f0, f1 = bc.noise_triple(case)
    penalty = bc.PENALTY[case, 1]
    mode, v0, v1, cost, costs = bc.noise_result(case, 1)
    pred = bipred.predict(past, nxt, mode, v0, v1, bs)
    assert pred.dtype == np.uint8 and pred.shape == mid.shape
    hb, wb = shape[0] // bs, shape[1] // bs
    want = 0
    for i in range(hb):
        for j in range(wb):
            if mode[i, j] <= 2:
                want += int(cost[i, j]) - (penalty if mode[i, j] == 2 else 0)
            else:
                want += bipred.sse(past[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs], mid[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs])
    assert bipred.sse(pred[:hb * bs, :wb * bs], mid[:hb * bs, :wb * bs]) == want
    assert np.array_equal(pred[hb * bs:], past[hb * bs:]) and np.array_equal(pred[:, wb * bs:], past[:, wb * bs:])
    with pytest.raises(ValueError):                              # a vector in use must point inside
        bipred.predict(past, nxt, np.zeros_like(mode), np.full_like(v0, -1), v1, bs)


@pytest.mark.parametrize("pnorm", (0, 1))
def test_occlusion_scene(pnorm):
    """The uncovered blocks choose the frame in which they are visible, the others the average (bipred_cases.check_scene), and
    the chosen prediction is better than either single-reference one."""
    past, mid, nxt = bc.occlusion_scene()
    f0, f1, mode, v0, v1, cost, costs = bc.scene_result(pnorm)
    assert bipred.default_penalty(16, pnorm) == (64, 1024)[pnorm]
    bc.check_scene(mode)
    H, W = mid.shape
    s = [bipred.sse(mid, bipred.predict(past, nxt, m, f0, f1, 16)) for m in (bipred.all_mode(f0, 0, H, W, 16), bipred.all_mode(f1, 1, H, W, 16))]
    chosen = bipred.sse(mid, bipred.predict(past, nxt, mode, v0, v1, 16))
    assert chosen < min(s)
    rep = bipred.summary(mode, f0, f1, v0, v1, s[0], s[1], chosen, H, W)
    assert abs(sum(rep["mode_share"]) - 1.0) < 1e-12 and rep["mode_share"][2] > 0.5 and 0.0 <= rep["refined_share"] <= 1.0
    assert rep["psnr_chosen"] > max(rep["psnr_past"], rep["psnr_next"])
