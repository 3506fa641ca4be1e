"""hier.py, the host definition of hierarchical block matching: against an independent restatement, its
argument rules, the tie and clamp rules, and what the definition achieves on frames whose shift is known.  Runs without a GPU."""
import numpy as np
import pytest

import hier
import hier_cases as hc

# test_known_shifts_larger_frame: interior hit rates of hier.search on hc.pair(160, 192, shift), cw 4, r 1, levels 3, measured
# on the CPU (48 interior blocks at bs 16, 8 at bs 32); each case is asserted at its rate less 0.05.
#   shift       bs 16 MAE  bs 16 MSE  bs 32 MAE  bs 32 MSE
#   (13, -9)    0.979      1.000      1.000      1.000
#   (-18, 7)    0.833      0.958      1.000      1.000
#   (3, 2)      0.938      0.938      1.000      1.000
#   (0, 0)      1.000      1.000      1.000      1.000
LARGER_RATES = {(16, 0): (0.979, 0.833, 0.937, 1.0), (16, 1): (1.0, 0.958, 0.937, 1.0),
                (32, 0): (1.0, 1.0, 1.0, 1.0), (32, 1): (1.0, 1.0, 1.0, 1.0)}


def restated(prev_pyr, cur_pyr, bs, cw, r, pnorm, levels):
    """The definition once more, written on its own: per block, every candidate of a level goes into a list of (cost, order,
    vector) with order 0 for the centre and 1, 2, ... for the offsets in column-major order, and the smallest tuple wins."""
    H, W = prev_pyr[2].shape
    Hb, Wb = H // bs, W // bs
    first = 3 - levels
    fields = {l: np.zeros((Hb, Wb, 2), np.int32) for l in range(first, 3)}
    costs = {l: np.zeros((Hb, Wb), np.int64) for l in range(first, 3)}
    for i in range(Hb):
        for j in range(Wb):
            vec = (0, 0)
            for l in range(first, 3):
                P, C = prev_pyr[l].astype(np.int64), cur_pyr[l].astype(np.int64)
                Hl, Wl = P.shape
                b = bs // (1 << (2 - l))
                R = cw if l == first else r
                top, left = i * b, j * b
                want = (0, 0) if l == first else (2 * vec[0], 2 * vec[1])
                centre = (int(np.clip(want[0], -left, Wl - b - left)), int(np.clip(want[1], -top, Hl - b - top)))
                offsets = [(0, 0)] + [(ox, oy) for ox in range(-R, R + 1) for oy in range(-R, R + 1) if (ox, oy) != (0, 0)]
                listed = []
                for order, (ox, oy) in enumerate(offsets):
                    x, y = left + centre[0] + ox, top + centre[1] + oy
                    if 0 <= x <= Wl - b and 0 <= y <= Hl - b:
                        d = C[y:y + b, x:x + b] - P[top:top + b, left:left + b]
                        listed.append((int(np.abs(d).sum() if pnorm == 0 else (d ** 2).sum()), order, (centre[0] + ox, centre[1] + oy)))
                cost, _, vec = min(listed)
                fields[l][i, j] = vec
                costs[l][i, j] = cost
    return fields, costs


def same(a, b):
    fa, ca = a
    fb, cb = b
    assert sorted(fa) == sorted(fb) == sorted(ca) == sorted(cb)
    for l in fa:
        assert fa[l].dtype == np.int32 and ca[l].dtype == np.int64
        assert np.array_equal(ca[l], cb[l]), (l, np.argwhere(ca[l] != cb[l])[:4])
        assert np.array_equal(fa[l], fb[l]), (l, np.argwhere(np.any(fa[l] != fb[l], axis=2))[:4])


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(37)
    prev, cur = rng.integers(0, 256, size=(2, 37, 53), dtype=np.uint8)
    return hc.pyramid(prev), hc.pyramid(cur)


@pytest.mark.parametrize("bs,levels,cw,r", [(8, 2, 8, 1), (8, 2, 3, 3), (4, 1, 8, 0), (4, 1, 0, 2)])
def test_equals_restatement(noise, bs, levels, cw, r):
    for pnorm in (0, 1):
        got = hier.search(noise[0], noise[1], bs, cw, r, pnorm, levels)
        assert sorted(got[0]) == list(range(3 - levels, 3)) and got[0][2].shape == (37 // bs, 53 // bs, 2)
        same(got, restated(noise[0], noise[1], bs, cw, r, pnorm, levels))


def test_argument_rules_and_reach(noise):
    for bs, cw, r, pnorm, levels in ((16, 8, 1, 0, 3), (64, 0, 0, 1, 3), (4, 8, 3, 0, 1), (8, 8, 3, 1, 2), (12, 1, 1, 0, 2), (20, 4, 2, 0, 3)):
        assert hier.check_args(bs, cw, r, pnorm, levels) == (bs, cw, r, pnorm, levels)
    for bs, cw, r, pnorm, levels in ((16, 8, 1, 0, 0), (16, 8, 1, 0, 4), (18, 8, 1, 0, 3), (8, 8, 1, 0, 3), (6, 8, 1, 0, 2), (3, 8, 1, 0, 1),
                                     (68, 8, 1, 0, 3), (128, 8, 1, 0, 3), (16, 9, 1, 0, 3), (16, -1, 1, 0, 3), (16, 8, 4, 0, 3),
                                     (16, 8, -1, 0, 3), (16, 8, 1, 2, 3), (0, 8, 1, 0, 1)):
        with pytest.raises(ValueError):
            hier.check_args(bs, cw, r, pnorm, levels)
        with pytest.raises(ValueError):
            hier.search(noise[0], noise[1], bs, cw, r, pnorm, levels)
    assert hier.reach(8, 1, 3) == 35 and hier.reach(8, 1, 2) == 17 and hier.reach(8, 3, 1) == 8 and hier.reach(4, 1, 3) == 19
    assert hier.reach(0, 3, 3) == 9 and hier.reach(0, 0, 3) == 0
    # the reach is attained: a lone dot that moves by the reach along the diagonal
    prev, cur = np.zeros((2, 96, 96), np.uint8)
    prev[40:48, 40:48] = 255
    cur[40 + 17:48 + 17, 40 + 17:48 + 17] = 255
    fields, costs = hier.search(hc.pyramid(prev), hc.pyramid(cur), 8, 8, 1, 0, 2)
    assert tuple(fields[2][5, 5]) == (17, 17) and costs[2][5, 5] == 0
    assert max(abs(int(fields[2].min())), int(fields[2].max())) <= 17


def test_ties(noise):
    """Constant frames: every cost of a block is equal, the centre wins at every level.  Vertical stripes of period 2 against
    the same stripes one column on: every odd column offset costs nothing, whatever the row offset, and the first of them
    in the definition's order that lies inside the frame wins."""
    flat = hc.pyramid(np.full((37, 53), 90, np.uint8)), hc.pyramid(np.full((37, 53), 97, np.uint8))
    for bs, levels in ((8, 2), (16, 3), (4, 1)):
        for pnorm in (0, 1):
            fields, costs = hier.search(flat[0], flat[1], bs, 8, 3, pnorm, levels)
            for l in fields:
                b = bs >> (2 - l)
                assert not fields[l].any() and np.all(costs[l] == b * b * (7, 49)[pnorm])
    stripes = np.tile(np.array([0, 255], np.uint8), (37, 27))[:, :53]
    prev, cur = hc.pyramid(stripes), hc.pyramid(255 - stripes)
    for bs, cw in ((4, 3), (4, 2), (8, 8)):
        for pnorm in (0, 1):
            fields, costs = hier.search(prev, cur, bs, cw, 1, pnorm, 1)
            assert not costs[2].any()
            for i in range(37 // bs):
                for j in range(53 // bs):
                    ox = next(o for o in range(-cw, cw + 1) if o % 2 and 0 <= j * bs + o <= 53 - bs)
                    oy = max(-cw, -i * bs)
                    assert tuple(fields[2][i, j]) == (ox, oy), (bs, cw, i, j)
    for bs, levels in ((8, 2), (16, 3)):                        # their pyramids are nearly flat: ties at every level
        for pnorm in (0, 1):
            same(hier.search(prev, cur, bs, 8, 1, pnorm, levels), restated(prev, cur, bs, 8, 1, pnorm, levels))


def test_clamp(noise):
    """On noise the coarse vectors are large everywhere, so at the frame edges (and at the odd level sizes 19 x 27 of 37 x 53)
    twice the parent vector points outside and is clamped."""
    fields, _ = hier.search(noise[0], noise[1], 8, 8, 1, 0, 2)
    assert hc.clamped_blocks(fields, hc.level_shapes(37, 53), 8) > 0
    assert hc.level_shapes(37, 53) == {0: (10, 14), 1: (19, 27), 2: (37, 53)}
    assert [p.shape for p in noise[0]] == [(10, 14), (19, 27), (37, 53)]
    for l in fields:                                            # every vector keeps its block inside its level
        Hl, Wl = hc.level_shapes(37, 53)[l]
        b = 8 >> (2 - l)
        i, j = np.mgrid[0:37 // 8, 0:53 // 8]
        x, y = j * b + fields[l][:, :, 0], i * b + fields[l][:, :, 1]
        assert x.min() >= 0 and y.min() >= 0 and (x + b).max() <= Wl and (y + b).max() <= Hl


@pytest.mark.parametrize("bs", [16, 32])
def test_known_shifts(bs):
    """96 x 128, cw 4, r 1, levels 3: every interior block (8 at bs 16, 2 at bs 32) finds the shift, both norms; (-18, 7) lies
    outside what an exhaustive search of window 16 can find."""
    assert hier.reach(4, 1, 3) == 19
    for shift in hc.SHIFTS:
        prev, cur = hc.pair(96, 128, shift)
        for pnorm in (0, 1):
            fields, _ = hier.search(hc.pyramid(prev), hc.pyramid(cur), bs, 4, 1, pnorm, 3)
            assert hc.interior_hits(fields[2], shift, bs) >= 1.0 - 0.05, (shift, pnorm)


@pytest.mark.parametrize("bs", [16, 32])
def test_known_shifts_larger_frame(bs):
    """160 x 192, 48 interior blocks at bs 16 and 8 at bs 32.  Measured rates (LARGER_RATES above): 1.0 in every case at bs 32;
    at bs 16 the lowest is 0.833 ((-18, 7), MAE), then 0.938 ((3, 2), both norms), 0.958 and 0.979.  Each case is asserted at
    its measured rate less 0.05."""
    for k, shift in enumerate(hc.SHIFTS):
        prev, cur = hc.pair(160, 192, shift)
        for pnorm in (0, 1):
            fields, _ = hier.search(hc.pyramid(prev), hc.pyramid(cur), bs, 4, 1, pnorm, 3)
            rate = hc.interior_hits(fields[2], shift, bs)
            print("160x192 bs %d shift %r norm %d: interior hit rate %.3f" % (bs, shift, pnorm, rate))
            assert rate >= LARGER_RATES[(bs, pnorm)][k] - 0.05, (shift, pnorm, rate)
