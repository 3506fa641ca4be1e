"""Exhaustive MSE at bs 16 on both sides of every geometry limit of the matrix-core kernel (csrc/bbme_mfma.hip,
bbme_mfma_takes): at most 65535 block rows (grid.y), at most 65535 groups of 8 pairs in one launch (grid.z), and table
offsets that fit 32 bits ((H + 64) * pitch * 4 < 2^31).  Inside a limit k_exh_mfma16 runs on the signed box-sum table
(kind 2); outside it the elimination kernels run on the plain one (kind 1).  The box-sum table is built for the kernel
that reads it; a kind-2 table read as kind 1 is off by a candidate-dependent term and moves the argmin.

Each geometry is checked three ways: the launch plan names the expected kernel; windows of blocks match the C oracle
(run on a crop that holds every candidate of those blocks, so its answer is the full frame's); the whole field matches a
GME_EXH_MFMA=0 run (kind-1 table, elimination kernels).  sw 8 runs at the default settings, sw 32 with GME_EXH_MFMA=1,
whose declined geometries go to the R = 5 two-level elimination path.  Needs an MI355X."""
import os
import re

import numpy as np
import pytest

from helpers import c_oracle

pytestmark = pytest.mark.gpu

MFMA_ROWS = 65535                       # grid.y
PAIR_FRAMES = 65535 * 8 + 2             # fd 2: 65535 groups of 8 pairs; fd 1: one pair more
WIDE_W = 32768                          # (16304 + 64) * 32768 * 4 < 2^31 <= (16320 + 64) * 32768 * 4
WIDE_H = {"inside": 16304, "outside": 16320}
SW_MODES = [pytest.param(8, None, id="sw8"), pytest.param(32, "1", id="sw32-mfma")]


def _vector_plan(sw):
    """the elimination kernel's plan for this window: k_exh_sea16p_mse<R,NV> (persistent) or k_exh_sea16_mse<R>"""
    return re.compile(r"k_exh_sea16p?_mse<%d[,>]" % ((2 * sw + 31) // 16))


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


class _env:
    """set (str) or remove (None) environment variables for the duration of a block"""
    def __init__(self, **kv):
        self.kv = kv
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _noise(rng, *shape):
    return np.frombuffer(rng.bytes(int(np.prod(shape))), np.uint8).reshape(shape)


def _pan_pair(rng, H, W):
    """previous / current frame: independent noise in the left half, the right half a pan of the previous frame by
    (3, -5) -- blocks with a true vector next to blocks where only the cost decides"""
    prev = _noise(rng, H, W)
    cur = _noise(rng, H, W).copy()
    h = W // 2
    cur[:H - 3, h:] = prev[3:, h - 5:W - 5]
    return prev, cur


def _check_plan(ctx, side, sw):
    plan = ctx.last_bbme_info()["plan"]
    if side == "inside":
        assert plan.startswith("k_exh_mfma16<%d>" % ((2 * sw + 16) // 16)), plan
    else:
        assert _vector_plan(sw).match(plan), plan
    return plan


def _check_windows(co, prev, cur, mv, sw, windows, what):
    """blocks [r0, r1) x [c0, c1) of the device field `mv` against the oracle on a crop holding all their candidates
    (offsets -sw .. sw + 15 along each axis, bbme.py's window; or the real frame edge)"""
    H, W = prev.shape
    nbr, nbc = H // 16, W // 16
    m = (sw + 15 + 15) // 16                 # whole block rows / columns that hold a candidate reaching sw + 15 past the block
    for r0, r1, c0, c1 in windows:
        r0, c0, r1, c1 = max(0, r0), max(0, c0), min(nbr, r1), min(nbc, c1)
        y0, y1, x0, x1 = max(0, r0 - m), min(nbr, r1 + m), max(0, c0 - m), min(nbc, c1 + m)
        ys = slice(16 * y0, H if y1 == nbr else 16 * y1)
        xs = slice(16 * x0, W if x1 == nbc else 16 * x1)
        want = co.bbme(prev[ys, xs], cur[ys, xs], 16, sw, 0, 1)[r0 - y0:r1 - y0, c0 - x0:c1 - x0]
        got = mv[r0:r1, c0:c1]
        bad = np.argwhere((got != want).any(axis=-1))
        assert bad.size == 0, "%s: %d of %d blocks in rows [%d, %d) cols [%d, %d) differ from the C oracle, first %s: %s vs %s" % (
            what, len(bad), got.shape[0] * got.shape[1], r0, r1, c0, c1, bad[0] + (r0, c0),
            got[tuple(bad[0])], want[tuple(bad[0])])


def _same_as_vector_unit(ctx, run, mv, sw, what):
    """the whole field against a GME_EXH_MFMA=0 run of the same input (kind-1 table, elimination kernels)"""
    with _env(GME_EXH_MFMA="0"):
        vec = run()
        plan = ctx.last_bbme_info()["plan"]
    assert _vector_plan(sw).match(plan), plan
    diff = (mv != vec).any(axis=-1)
    assert not diff.any(), "%s: %d blocks differ from the vector-unit run, first %s" % (what, int(diff.sum()), np.argwhere(diff)[0])


# ---- block rows: nbr = 65535 / 65536 at W = 32 ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tall_pair():
    return _pan_pair(np.random.default_rng(65535), 16 * (MFMA_ROWS + 1), 32)


@pytest.mark.parametrize("sw,mfma", SW_MODES)
@pytest.mark.parametrize("side", ["inside", "outside"])
def test_block_row_limit(native, tall_pair, side, sw, mfma):
    """H = 16 * 65535 (k_exh_mfma16) and 16 * 65536 (elimination), W = 32: the one-shot entry point and a Sequence"""
    import bbme
    co = c_oracle()
    ctx = native.default_context()
    nbr = MFMA_ROWS + (side == "outside")
    prev, cur = tall_pair[0][:16 * nbr], tall_pair[1][:16 * nbr]
    windows = [(0, 4, 0, 2), (nbr // 2 - 2, nbr // 2 + 2, 0, 2), (65528, nbr, 0, 2)] + [(r, r + 2, 0, 2) for r in range(4, nbr - 8, 1021)]
    with _env(GME_EXH_MFMA=mfma):
        one = bbme.get_motion_field(prev, cur, block_size=16, search_window=sw, searching_procedure=0, pnorm_distance=1)
        _check_plan(ctx, side, sw)
        assert one.shape == (nbr, 2, 2)
        _check_windows(co, prev, cur, one, sw, windows, "one-shot %s sw %d" % (side, sw))
        seq = native.Sequence(ctx, 2, 16 * nbr, 32)
        try:
            seq.upload(0, prev[None])
            seq.upload(1, cur[None])

            def run():
                seq.bbme(1, 16, sw, 0, 1)
                return seq.read_mv()[0]
            mv = run()
            _check_plan(ctx, side, sw)
            _check_windows(co, prev, cur, mv, sw, windows, "Sequence %s sw %d" % (side, sw))
            assert np.array_equal(mv, one)
            _same_as_vector_unit(ctx, run, mv, sw, "Sequence %s sw %d" % (side, sw))
        finally:
            seq.close()


# ---- pairs per launch: 524 280 / 524 281 pairs of 32 x 32 (nblk 4: one launch) -----------------------------------------

@pytest.fixture(scope="module")
def many_frames():
    """524 282 frames of noise; every odd frame is its predecessor panned by (2, -3) (wrapping), so the fd 1 pairs
    alternate between a pan and independent noise"""
    fr = _noise(np.random.default_rng(524282), PAIR_FRAMES, 32, 32).copy()
    fr[1::2] = np.roll(fr[0:-1:2], (2, -3), axis=(1, 2))
    return fr


@pytest.mark.parametrize("sw,mfma", SW_MODES)
@pytest.mark.parametrize("side", ["inside", "outside"])
def test_pairs_per_launch_limit(native, many_frames, side, sw, mfma):
    """fd 2 -> 524 280 pairs = 65535 groups of 8 (k_exh_mfma16), fd 1 -> 524 281 (elimination), in one launch"""
    co = c_oracle()
    ctx = native.default_context()
    fd = 2 if side == "inside" else 1
    P = PAIR_FRAMES - fd
    pairs = sorted(set(list(range(8)) + list(range(65535 * 8 - 16, P)) + list(range(8, P - 8, 4093))))
    seq = native.Sequence.from_frames(ctx, many_frames)
    try:
        def run():
            seq.bbme(fd, 16, sw, 0, 1)
            return seq.read_mv()
        with _env(GME_EXH_MFMA=mfma):
            mv = run()
            _check_plan(ctx, side, sw)
            assert mv.shape == (P, 2, 2, 2)
            for p in pairs:
                want = co.bbme(many_frames[p], many_frames[p + fd], 16, sw, 0, 1)
                assert np.array_equal(mv[p], want), "%s sw %d: pair %d of %d differs from the C oracle: %s vs %s" % (
                    side, sw, p, P, mv[p].tolist(), want.tolist())
            _same_as_vector_unit(ctx, run, mv, sw, "%s sw %d" % (side, sw))
    finally:
        seq.close()


# ---- 32-bit table offsets: 16304 / 16320 x 32768 ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide_pair():
    return _pan_pair(np.random.default_rng(32768), WIDE_H["outside"], WIDE_W)


@pytest.mark.parametrize("sw,mfma", SW_MODES)
@pytest.mark.parametrize("side", ["inside", "outside"])
def test_table_offset_limit(native, wide_pair, side, sw, mfma):
    """(H + 64) * pitch * 4 just under 2^31 (k_exh_mfma16) and at 2^31 (elimination), one pair"""
    co = c_oracle()
    ctx = native.default_context()
    H, W = WIDE_H[side], WIDE_W
    prev, cur = wide_pair[0][:H], wide_pair[1][:H]
    nbr, nbc = H // 16, W // 16
    windows = [(r, r + 3, c, c + 8) for r in (0, nbr // 2, nbr - 3) for c in (0, nbc // 2 - 4, nbc - 8)]
    windows += [(nbr - 2, nbr, c, c + 4) for c in range(64, nbc - 8, 127)]
    seq = native.Sequence(ctx, 2, H, W)
    try:
        seq.upload(0, prev[None])
        seq.upload(1, cur[None])

        def run():
            seq.bbme(1, 16, sw, 0, 1)
            return seq.read_mv()[0]
        with _env(GME_EXH_MFMA=mfma):
            mv = run()
            _check_plan(ctx, side, sw)
            _check_windows(co, prev, cur, mv, sw, windows, "%dx%d sw %d" % (H, W, sw))
            _same_as_vector_unit(ctx, run, mv, sw, "%dx%d sw %d" % (H, W, sw))
    finally:
        seq.close()
