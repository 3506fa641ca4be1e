"""The content families and case lists of tests/saturated_cases.py, checked without a GPU: every family reaches the extreme
it is named for (by NumPy int64 block costs written in saturated_cases.py, not the oracles' cost routine), the large-block
cases separate NumPy's float32 summation order from integer order for every block size and search, the C oracle the GPU
tests compare against equals the NumPy oracle on the cases, and three plausibly wrong cost functions each move a vector."""
import numpy as np
import pytest

import saturated_cases as sc
from helpers import c_oracle, np_oracle

BS16_CASES = [(H, W, sw) for sw in sc.BS16_SWS for (H, W) in sc.BS16_SHAPES[sw]]


def _blocks(H, W, bs):
    return [(r, c) for r in range(H // bs) for c in range(W // bs)]


# ---------------------------------------------------------------------------
# every family reaches its extreme
# ---------------------------------------------------------------------------
def test_case_lists_are_the_listed_shapes():
    assert sc.BS16_SHAPES[0] == sc.BS16_SHAPES[8] == sc.BS16_SHAPES[16] == ((48, 80), (50, 83))
    assert sc.BS16_SHAPES[24] == sc.BS16_SHAPES[32] == ((80, 112), (81, 115))
    assert [(2 * sw + 31) // 16 for sw in sc.BS16_SWS] == [1, 2, 3, 4, 5]              # the size classes R of the elimination kernels
    for H, W, sw in BS16_CASES:                    # one block sees every offset -sw .. sw, the frame's other blocks touch each edge
        r, c = sc.full_window_block(H, W, 16, sw)
        assert (H // 16, W // 16) in ((3, 5), (5, 7)) and 0 < r < H // 16 - 1 and 0 < c < W // 16 - 1
    assert sc.full_window_block(48, 80, 16, 24) is None and sc.full_window_block(64, 112, 16, 32) is None      # nothing smaller would do
    assert sc.WALKQ_SIZES == (4, 8, 12, 20, 24, 28, 32) and sc.WALK_SIZES == (6, 10) and sc.OTHER_SWS == (7, 2)
    assert sc.other_shape(32) == (97, 131)
    H, W = sc.DENSE_SHAPE                          # level 1 ((H + 1) // 2) holds a 16 x 16 block with a row and a column to spare
    assert (H + 1) // 2 == 17 and (W + 1) // 2 == 17
    for variant in sc.VARIANTS:
        st = sc.stack(variant, 50, 83)
        assert st.shape == (3, 50, 83) and st.dtype == np.uint8 and np.array_equal(st[0], st[2])
        assert np.array_equal(st, sc.stack(variant, 50, 83))                             # deterministic
    assert set(sc.FAMILIES) == {v for f in sc.FAMILIES for v in sc.variants_of(f)} - {"half_split_rows"}


@pytest.mark.parametrize("bs", (16, 2, 4, 6, 10, 12, 20, 32))
def test_opposite_every_candidate_costs_the_maximum(bs):
    cases = BS16_CASES if bs == 16 else [sc.other_shape(bs) + (sw,) for sw in sc.OTHER_SWS]
    for H, W, sw in cases:
        lo, hi = sc.opposite(H, W, bs)
        for prev, cur in ((lo, hi), (hi, lo)):
            for r, c in _blocks(H, W, bs):
                mae, _ = sc.candidate_costs(prev, cur, bs, sw, r, c, sc.sad)
                mse, _ = sc.candidate_costs(prev, cur, bs, sw, r, c, sc.ssd)
                assert len(mae) >= 1 and (mae == 255 * bs * bs).all() and (mse == 65025 * bs * bs).all(), (H, W, sw, r, c)
    assert 255 * 16 * 16 == 65280 and 65025 * 16 * 16 == 16646400 < 2 ** 24


def _near_max_holds(seed, step):
    """What the issue asks of near_max at bs 16, for every shape, window and norm: every block's minimum is at least 65000
    (MAE) / 2^23 (MSE), the winner is unique in at least half of the blocks, and in the block that sees every offset -sw .. sw
    the winner is not the first candidate in scan order."""
    ok = True
    for H, W, sw in BS16_CASES:
        prev, cur = sc.near_max(H, W, 16, seed, step)
        for pnorm, floor in ((0, 65000), (1, 2 ** 23)):
            unique = 0
            for r, c in _blocks(H, W, 16):
                costs, _ = sc.candidate_costs(prev, cur, 16, sw, r, c, sc.norm_cost(pnorm))
                s = np.sort(costs)
                ok &= bool(s[0] >= floor)
                unique += len(s) == 1 or s[0] < s[1]
            ok &= 2 * unique >= len(_blocks(H, W, 16))
            r, c = sc.full_window_block(H, W, 16, sw)
            costs, _ = sc.candidate_costs(prev, cur, 16, sw, r, c, sc.norm_cost(pnorm))
            ok &= int(np.argmin(costs)) != 0
    return ok


def test_near_max_reaches_its_extreme():
    assert _near_max_holds(sc.NEAR_MAX_SEED, sc.NEAR_MAX_STEP)
    assert not _near_max_holds(0, 24)              # the check tells seeds apart: this one has a window whose full block's first candidate wins
    prev, cur = sc.pair("near_max", 48, 80)
    assert np.array_equal(cur, sc.near_max(48, 80, 16, sc.NEAR_MAX_SEED, sc.NEAR_MAX_STEP)[1]) and not prev.any()
    assert set(np.unique(cur)) == {252, 253, 254, 255}
    # the costs differ in their lowest bits only: within 2^8 (MAE) and 2^17 (MSE) of the maximum
    costs, _ = sc.candidate_costs(prev, cur, 16, 16, 1, 2, sc.sad)
    assert costs.max() <= 65280 and costs.min() > 65280 - 256 and len(np.unique(costs)) > 16
    costs, _ = sc.candidate_costs(prev, cur, 16, 16, 1, 2, sc.ssd)
    assert costs.max() <= 16646400 and costs.min() > 16646400 - 2 ** 17 and len(np.unique(costs)) > 64


def test_half_split_reaches_both_signed_extremes_in_one_candidate():
    both = clamp = 0
    for variant in sc.variants_of("half_split"):
        for H, W, sw in BS16_CASES:
            prev, cur = sc.pair(variant, H, W)
            assert set(np.unique(prev)) == {0, 255} and np.array_equal(cur, 255 - prev)
            for r, c in _blocks(H, W, 16):
                d = sc.quadrant_differences(prev, cur, 16, sw, r, c)
                assert np.abs(d).max() <= 16320
                hit = ((d == 16320).any(axis=1) & (d == -16320).any(axis=1)).any()
                both += bool(hit)
                # lower_bounds_mse sums the squares of twice the differences into 32 bits with a clamp at 2^31 - 1
                clamp += bool((((2 * d) ** 2).sum(axis=1) >= 2 ** 31).any())
                assert np.abs(2 * d).max() <= 32640 < 2 ** 15
            # the zero vector meets the maximum, a shift by half a block (inside the window at every sw) matches exactly
            costs, offs = sc.candidate_costs(prev, cur, 16, sw, 1, 2, sc.sad)
            assert costs.max() == 65280 and costs.min() == 0, (variant, H, W, sw)
        assert both > 0 and clamp > 0, variant
    assert 4 * (2 * 16320) ** 2 >= 2 ** 31         # what "4 LBx" reaches with four quadrants at the extreme


def test_cell_pan_has_an_exact_match_beside_the_maximum():
    for bs, cases in [(16, BS16_CASES)] + [(bs, [sc.other_shape(bs) + (7,)]) for bs in sc.WALKQ_SIZES + sc.WALK_SIZES]:
        dx, dy = sc.cell_pan_vector(bs)
        assert dx % 4 and dy % 4 and 0 < dx < bs and 0 < dy < bs
        top = 0
        for H, W, sw in cases:
            prev, cur = sc.pair("cell_pan", H, W, bs)
            assert set(np.unique(prev)) == {0, 255}
            inside = 0
            for r, c in _blocks(H, W, bs):
                for pnorm in (0, 1):
                    costs, offs = sc.candidate_costs(prev, cur, bs, sw, r, c, sc.norm_cost(pnorm))
                    top = max(top, int(costs.max()) if pnorm == 0 else 0)
                    if r * bs + dy + bs <= H and c * bs + dx + bs <= W:          # the match lies inside the frame
                        k = int(np.argmin(costs))
                        assert costs[k] == 0, (bs, H, W, sw, r, c)
                        inside += pnorm
            assert inside >= (H // bs - 1) * (W // bs - 1)
        assert top == 255 * bs * bs, (bs, top)


def test_bits_sits_at_half_of_the_maximum():
    for H, W, sw in BS16_CASES:
        prev, cur = sc.pair("bits", H, W)
        assert set(np.unique(prev)) == set(np.unique(cur)) == {0, 255}
        costs, _ = sc.candidate_costs(prev, cur, 16, sw, 1, 2, sc.ssd)
        assert 2 ** 22 < costs.min() and costs.max() < 3 * 2 ** 22 and (costs % 65025 == 0).all()


# ---------------------------------------------------------------------------
# float32 order against integer order at bs > 16
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bs", sc.F32_BLOCK_SIZES)
@pytest.mark.parametrize("procedure", (0, 1, 2, 3))
def test_large_blocks_separate_float32_order_from_integer_order(bs, procedure):
    co = c_oracle()
    assert 65025 * bs * bs >= 2 ** 24
    prev, cur = sc.f32_pair(bs, procedure)
    assert prev.shape == sc.other_shape(bs)
    f32 = co.bbme(prev, cur, bs, sc.F32_SW, procedure, 1, allow_inexact=0)
    exact = co.bbme(prev, cur, bs, sc.F32_SW, procedure, 1, allow_inexact=1)
    assert (f32 != exact).any(axis=-1).sum() >= 1, (bs, procedure)
    assert np.array_equal(f32, np_oracle().get_motion_field(prev, cur, bs, sc.F32_SW, procedure, 1)), (bs, procedure)
    if procedure == 0:                             # ... and "integer order" is what the int64 restatement gives
        assert np.array_equal(exact, sc.exhaustive_field(prev, cur, bs, sc.F32_SW, sc.ssd)), bs


# ---------------------------------------------------------------------------
# the C oracle against the NumPy oracle
# ---------------------------------------------------------------------------
def _np_field(prev, cur, bs, sw, procedure, pnorm, block_rows=None):
    o = np_oracle()
    H, W = prev.shape
    mf = np.zeros((H // bs, W // bs, 2), np.int32)
    if procedure == 0:
        return o.search_exhaustive(prev, cur, mf, H, W, pnorm, bs, sw, block_rows=block_rows)
    return o.SEARCHES[procedure](prev, cur, mf, H, W, pnorm, bs, sw)


def _oracles_agree(variant, H, W, bs, sw, rows=None):
    """All four searches, both norms, the pair in both directions and prev against itself (frame distance 2).  `rows`: the
    block rows the exhaustive NumPy search visits (its Python loops are the slow part)."""
    co = c_oracle()
    st = sc.stack(variant, H, W, bs)
    for a, b in ((0, 1), (1, 2), (0, 2)):
        for pnorm in (0, 1):
            for procedure in (1, 2, 3):
                assert np.array_equal(co.bbme(st[a], st[b], bs, sw, procedure, pnorm), _np_field(st[a], st[b], bs, sw, procedure, pnorm)), (
                    variant, H, W, bs, sw, a, b, procedure, pnorm)
            want = co.bbme(st[a], st[b], bs, sw, 0, pnorm)
            for row in (rows if rows is not None else [None]):
                br = None if row is None else (row, row + 1)
                got = _np_field(st[a], st[b], bs, sw, 0, pnorm, br)
                sl = slice(None) if row is None else slice(row, row + 1)
                assert np.array_equal(got[sl], want[sl]), (variant, H, W, bs, sw, a, b, pnorm, row)


@pytest.mark.slow
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_oracles_agree_at_bs16(variant):
    """Every bs 16 case.  From sw 24 on the exhaustive NumPy search visits the interior block row (2) and one edge row (0)."""
    for H, W, sw in BS16_CASES:
        _oracles_agree(variant, H, W, 16, sw, rows=(0, 2) if sw >= 24 else None)


@pytest.mark.parametrize("bs", (4, 12, pytest.param(32, marks=pytest.mark.slow)))
def test_oracles_agree_at_other_block_sizes(bs):
    """bs 32 under MSE is the float32-order path of the C oracle (pairwise_f32) against NumPy's own float32 sums."""
    H, W = sc.other_shape(bs)
    for variant in sc.VARIANTS:
        for sw in sc.OTHER_SWS:
            _oracles_agree(variant, H, W, bs, sw)


# ---------------------------------------------------------------------------
# plausible mutants
# ---------------------------------------------------------------------------
def _moved(variant, H, W, bs, sw, exact, mutant):
    prev, cur = sc.pair(variant, H, W, bs)
    want = sc.exhaustive_field(prev, cur, bs, sw, exact)
    assert np.array_equal(want, c_oracle().bbme(prev, cur, bs, sw, 0, int(exact is sc.ssd))), (variant, H, W, bs, sw)
    return int((sc.exhaustive_field(prev, cur, bs, sw, mutant) != want).any(axis=-1).sum())


def test_sad_saturating_at_15_bits_moves_a_vector():
    mutant = lambda d: np.minimum(sc.sad(d), 2 ** 15 - 1)
    assert _moved("near_max", 48, 80, 16, 16, sc.sad, mutant) > 0


def test_ssd_modulo_2_23_moves_a_vector():
    mutant = lambda d: sc.ssd(d) % 2 ** 23
    assert _moved("bits", 48, 80, 16, 8, sc.ssd, mutant) > 0           # 129 and 130 differing pixels lie on either side of 2^23


def test_integer_order_at_large_blocks_moves_a_vector():
    o = np_oracle()
    for bs in sc.F32_BLOCK_SIZES:
        prev, cur = sc.f32_pair(bs, 0)
        want = o.get_motion_field(prev, cur, bs, sc.F32_SW, 0, 1)       # NumPy's own float32 sums
        assert (sc.exhaustive_field(prev, cur, bs, sc.F32_SW, sc.ssd) != want).any(), bs
