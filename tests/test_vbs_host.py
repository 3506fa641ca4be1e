"""The host definition of variable-block-size motion (vbs.py): the argument rules, the properties of the
tree, the order of children and candidates, the two-motion scene, and that the penalties of the noise cases the GPU tests use
exercise every depth.  Runs without a GPU."""
import numpy as np
import pytest

import subpel
import vbs
import vbs_cases as vc


def test_argument_rules():
    assert vbs.check_args(16, 2, 1, 0, 256) == (16, 2, 1, 0, 256)
    assert vbs.check_args(64, 2, 3, 1, 1 << 30) == (64, 2, 3, 1, 1 << 30)
    assert vbs.check_args(4, 0, 0, 0, 0) == (4, 0, 0, 0, 0) and vbs.check_args(12, 1, 1, 0, 0)[0] == 12
    for bad in ((16, 3, 1, 0, 0), (16, -1, 1, 0, 0), (16, 2, 4, 0, 0), (16, 2, -1, 0, 0), (16, 2, 1, 2, 0), (16, 2, 1, 0, -1),
                (16, 2, 1, 0, (1 << 30) + 1), (68, 2, 1, 0, 0), (128, 2, 1, 0, 0), (12, 2, 1, 0, 0), (18, 2, 1, 0, 0), (6, 1, 1, 0, 0),
                (0, 0, 1, 0, 0)):
        with pytest.raises(ValueError):
            vbs.check_args(*bad)
    p = np.zeros((32, 32), np.uint8)
    with pytest.raises(ValueError):
        vbs.tree(p, p, np.zeros((2, 3, 2), np.int32), 16, 1, 1, 0, 0)
    with pytest.raises(TypeError):
        vbs.tree(p.astype(np.int32), p, np.zeros((2, 2, 2), np.int32), 16, 1, 1, 0, 0)
    assert vbs.default_penalty(16, 0) == 256 and vbs.default_penalty(16, 1) == 4096


def root_costs(previous, current, mf, bs, pnorm):
    """The cost at every root's own vector, -1 where the displaced block is not inside."""
    H, W = previous.shape
    out = np.full(mf.shape[:2], -1, np.int64)
    for i in range(mf.shape[0]):
        for j in range(mf.shape[1]):
            vx, vy = int(mf[i, j, 0]), int(mf[i, j, 1])
            if vbs._inside(H, W, i * bs, j * bs, bs, vx, vy):
                out[i, j] = vbs._cost(previous, current, i * bs, j * bs, bs, vx, vy, pnorm)
    return out


@pytest.mark.parametrize("case", vc.NOISE)
def test_noise_properties(case):
    """On every noise case of the GPU tests, both norms: the penalty of vbs_cases makes every depth 0 .. D occur (at radius 0
    nothing can split, see vbs_cases.PENALTY); F_root <= c_root; roots that point outside give -1, depth 0 and keep their
    vector; depths form whole leaves; depth 0 returns the input; penalty 2^30 never splits."""
    shape, bs, D, r = case
    previous, current, mf = vc.noise_pair(*case)
    n = 1 << D
    for pnorm in (0, 1):
        leaf, depth, cost = vc.noise_result(case, pnorm)
        assert leaf.shape == (mf.shape[0] * n, mf.shape[1] * n, 2) and leaf.dtype == np.int32
        assert depth.shape == leaf.shape[:2] and depth.dtype == np.uint8 and cost.dtype == np.int64
        if r == 0:
            assert not depth.any()
        else:
            assert set(np.unique(depth).tolist()) == set(range(D + 1)), np.unique(depth)
        c_root = root_costs(previous, current, mf, bs, pnorm)
        outside = c_root < 0
        assert outside.any() and not outside.all()
        assert np.array_equal(cost < 0, outside) and np.all(cost[outside] == -1) and np.all(cost <= c_root)
        big = np.repeat(np.repeat(outside, n, 0), n, 1)
        assert not depth[big].any() and np.array_equal(leaf[big], np.repeat(np.repeat(mf, n, 0), n, 1)[big])
        assert vc.whole_leaves(depth, D)
        # a root that did not split keeps its own cost and vector
        kept = np.repeat(np.repeat((depth[::n, ::n] == 0), n, 0), n, 1)
        assert np.array_equal(leaf[kept], np.repeat(np.repeat(mf, n, 0), n, 1)[kept])
        assert np.array_equal(cost[depth[::n, ::n] == 0], c_root[depth[::n, ::n] == 0])
        l0, d0, c0 = vbs.tree(previous, current, mf, bs, 0, r, pnorm, 0)
        assert np.array_equal(l0, mf) and not d0.any() and np.array_equal(c0, c_root)
        lm, dm, cm = vbs.tree(previous, current, mf, bs, D, r, pnorm, 1 << 30)
        assert np.array_equal(lm, np.repeat(np.repeat(mf, n, 0), n, 1)) and not dm.any() and np.array_equal(cm, c_root)


def test_constant_frames_never_split():
    """Grey difference 7 everywhere: every child's best cost is its share of the parent's, S = c at penalty 0, and a tie does
    not split."""
    previous, current = np.full((48, 80), 90, np.uint8), np.full((48, 80), 97, np.uint8)
    mf = np.random.default_rng(3).integers(-2, 3, size=(3, 5, 2)).astype(np.int32)
    for pnorm, per_pixel in ((0, 7), (1, 49)):
        leaf, depth, cost = vbs.tree(previous, current, mf, 16, 2, 2, pnorm, 0)
        assert not depth.any() and np.array_equal(leaf, np.repeat(np.repeat(mf, 4, 0), 4, 1))
        inside = cost >= 0
        assert inside.any() and np.all(cost[inside] == 256 * per_pixel)


def test_root_outside():
    previous, current = np.zeros((32, 48), np.uint8), np.full((32, 48), 9, np.uint8)
    mf = np.zeros((2, 3, 2), np.int32)
    mf[0, 0], mf[1, 2], mf[0, 1] = (-1, 0), (0, 1), (2 ** 31 - 1, -2 ** 31)
    leaf, depth, cost = vbs.tree(previous, current, mf, 16, 2, 1, 0, 0)
    assert cost.tolist() == [[-1, -1, 2304], [2304, 2304, -1]] and not depth.any()
    assert np.array_equal(leaf, np.repeat(np.repeat(mf, 4, 0), 4, 1))


ORDER_CASES = ((1, ((-1, 1), (1, -1)), (-1, 1)),                  # column offset in the outer loop
               (2, ((0, 1), (0, -1)), (0, -1)),                    # row offset ascending
               (0, ((1, -1), (0, 1)), (0, 1)),
               (3, ((-1, 0), (0, 0)), (0, 0)))                     # the centre is scored first and keeps a tie


def order_pair(child, offsets):
    """24 x 24 frames, root (1, 1) of side 8: child k of its four 4 x 4 children has rows 10 + 20 k, 17 + 20 k, 10 + 20 k,
    17 + 20 k in ``previous`` (period 2, so copies two rows apart agree where they overlap); ``current`` is 200 but for copies
    of child ``child`` at the given offsets from its place, so exactly those candidates cost 0."""
    previous = np.full((24, 24), 200, np.uint8)
    current = previous.copy()
    rows = np.array([0, 7, 0, 7], np.uint8)[:, None]
    for k in range(4):
        previous[8 + 4 * (k >> 1):12 + 4 * (k >> 1), 8 + 4 * (k & 1):12 + 4 * (k & 1)] = 10 + 20 * k + rows
    y, x = 8 + 4 * (child >> 1), 8 + 4 * (child & 1)
    for ox, oy in offsets:
        current[y + oy:y + oy + 4, x + ox:x + ox + 4] = previous[y:y + 4, x:x + 4]
    return previous, current


@pytest.mark.parametrize("child,offsets,want", ORDER_CASES)
def test_order_of_children_and_candidates(child, offsets, want):
    """Hand-built equal minima: two candidates of one child cost 0, the first in the definition's order must win (the centre
    before every offset), and the winner lands in the cell at row child >> 1, column child & 1 of the root."""
    previous, current = order_pair(child, offsets)
    y, x = 8 + 4 * (child >> 1), 8 + 4 * (child & 1)
    zero = [(ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1) if vbs._cost(previous, current, y, x, 4, ox, oy, 0) == 0]
    assert sorted(zero) == sorted(offsets)                        # the equal minima are exactly the two that were built
    for pnorm in (0, 1):
        leaf, depth, cost = vbs.tree(previous, current, np.zeros((3, 3, 2), np.int32), 8, 1, 1, pnorm, 0)
        assert depth[2:4, 2:4].all()
        cells = leaf[2:4, 2:4].reshape(4, 2)
        assert cells[child].tolist() == list(want), cells
        best = [min(vbs._cost(previous, current, 8 + 4 * (k >> 1), 8 + 4 * (k & 1), 4, ox, oy, pnorm)
                    for ox in (-1, 0, 1) for oy in (-1, 0, 1)) for k in range(4)]
        assert best[child] == 0 and cost[1, 1] == sum(best)


def test_two_motion_scene():
    """96 x 128 frames of a smoothed-noise canvas, columns left of 72 move by (2, -1), the rest by (0, 1); roots of 16, depth 2,
    radius 2, MAE, penalty 256 on the field of an exhaustive +-6 search: the four interior roots of the straddling column
    split, no interior root away from it does, and every leaf cell of the straddling roots carries the motion of its side."""
    previous, current = vc.two_motion_scene()
    mf, leaf, depth, cost = vc.scene_result()
    vc.check_scene(mf, leaf, depth)
    assert vc.whole_leaves(depth, 2)
    # the leaf field compensates better than the root field
    g = 4
    sse_root = subpel.sse(current, subpel.compensate_integer(previous, mf, 16))
    sse_leaf = subpel.sse(current, subpel.compensate_integer(previous, leaf, g))
    assert sse_leaf < sse_root
    s = vbs.summary(depth, 2, sse_root, sse_leaf, *previous.shape)
    assert s["split_share"] == float(np.mean(depth[::4, ::4] > 0)) and sum(s["leaves"][d] * 4 ** (2 - d) for d in range(3)) == depth.size
    assert s["psnr_leaf"] > s["psnr_root"] and s["sse_leaf"] == sse_leaf
