"""Every block-search kernel on saturated content (tests/saturated_cases.py: frames near 0 against frames near 255), where
the hand-derived value ranges of the kernels are tight -- 16-bit SADs at 65280, 24-bit SSDs at 16 646 400, packed u16 pairs,
penalised bounds, the clamp of the squared bound, biased MSE costs of the walks, float32-order sums above 2^24 (DESIGN.md
§4, "Value ranges at saturated content").  tests/test_saturated_cases_host.py holds the cases to the extremes they claim.
Needs an MI355X.

Every motion field is compared with the C oracle bit for bit, and the kernel that answered is asserted through
last_bbme_info()["plan"].  One test id covers one kernel family; a case is three frames [prev, cur, prev] searched at frame
distance 1 (the pair in both directions) and 2."""
import functools
import re

import numpy as np
import pytest

import saturated_cases as sc
from helpers import c_oracle

pytestmark = pytest.mark.gpu

def _sw_id(sw):
    return "sw%d" % sw


def _bs_id(bs):
    return "bs%d" % bs


def _norm_id(pnorm):
    return "mse" if pnorm else "mae"


def _proc_id(procedure):
    return ("exhaustive", "three-step", "2d-log", "diamond")[procedure]


R_OF = {sw: (2 * sw + 31) // 16 for sw in sc.BS16_SWS}                        # size class of the elimination kernels


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


@functools.lru_cache(maxsize=None)
def _stack(variant, H, W, bs):
    st = sc.stack(variant, H, W, bs)
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def _want(variant, H, W, bs, sw, procedure, pnorm, fd):
    """The C oracle's fields of every pair of one case at one frame distance, computed once."""
    co = c_oracle()
    st = _stack(variant, H, W, bs)
    out = []
    for p in range(len(st) - fd):
        mf = co.bbme(st[p], st[p + fd], bs, sw, procedure, pnorm)
        mf.setflags(write=False)
        out.append(mf)
    return tuple(out)


def _search(native, frames, fd, bs, sw, procedure, pnorm):
    """(fields int32[pairs, h, w, 2], last_bbme_info()) of Sequence.bbme on a resident stack."""
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(frames))
    try:
        seq.bbme(fd, bs, sw, procedure, pnorm)
        return seq.read_mv(), ctx.last_bbme_info()
    finally:
        seq.close()


def _check_case(native, variant, H, W, bs, sw, procedure, pnorm, plan, distances=sc.BS16_DISTANCES):
    """One case at every frame distance: the plan names the kernel, every pair equals the oracle.  Returns the infos."""
    infos = []
    for fd in distances:
        mv, info = _search(native, _stack(variant, H, W, bs), fd, bs, sw, procedure, pnorm)
        what = (variant, H, W, bs, sw, procedure, pnorm, fd, info["plan"])
        assert re.match(plan, info["plan"]), what
        want = _want(variant, H, W, bs, sw, procedure, pnorm, fd)
        assert mv.shape[0] == len(want), what
        for p, w in enumerate(want):
            bad = np.argwhere((mv[p] != w).any(axis=-1))
            assert bad.size == 0, "%s pair %d: %d blocks differ, first (row, column) %s: %s, oracle %s" % (
                what, p, len(bad), bad[0], mv[p][tuple(bad[0])], w[tuple(bad[0])])
        infos.append(info)
    return infos


def _tiles(info, H, W, pairs):
    """tiles of one elimination launch, from the plan's "tiles TRxTC" """
    tr, tc = map(int, re.search(r"tiles (\d+)x(\d+)", info["plan"]).groups())
    return pairs * -(-(H // 16) // tr) * -(-(W // 16) // tc)


# ---------------------------------------------------------------------------
# elimination search at bs 16: k_exh_sea16 / k_exh_sea16p (MAE), k_exh_sea16_mse / k_exh_sea16p_mse, k_exh_redo16
# ---------------------------------------------------------------------------
# persistent: GME_SEA_PERSIST=2 (dynamic schedule) wherever the norm's fits() admits the tile shape plan() picks for these
# frames; the small frames would otherwise all take the one-tile kernel.  redo-all: a threshold of 0 hands every tile with
# a listed patch to k_exh_redo16<R, MSE>.  quota0 (MAE only: the MSE kernels have no phase C2) against default.
SEA_SETTINGS = {
    "one-tile": {"GME_SEA_PERSIST": "0"},
    "persistent": {"GME_SEA_PERSIST": "2"},
    "no-redo": {"GME_SEA_REDO": "0"},
    "redo-all": {"GME_SEA_REDO_FRAC": "0"},
    "quota0": {"GME_SEA_QUOTA": "0"},
    "default": {},
}


def _sea(native, monkeypatch, sw, setting, pnorm):
    monkeypatch.setenv("GME_EXH_MFMA", "0")        # MSE at sw <= 16 would otherwise take the matrix-core kernel
    for k, v in SEA_SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    name = "k_exh_sea16%s" + ("_mse" if pnorm else "")
    R = R_OF[sw]
    # three pairs of 15 or 35 blocks never fill the device: without GME_SEA_PERSIST=2 the launcher takes the one-tile kernel
    if setting == "persistent":
        plan = re.escape(name % "p") + r"<%d,\d+> tiles \d+x\d+ persistent-dynamic" % R
    else:
        plan = re.escape(name % "") + r"<%d> tiles \d+x\d+ one-tile " % R
    redo = 0
    for H, W in sc.BS16_SHAPES[sw]:
        for variant in sc.VARIANTS:
            infos = _check_case(native, variant, H, W, 16, sw, 0, pnorm, plan)
            for fd, info in zip(sc.BS16_DISTANCES, infos):
                print(variant, (H, W), "sw", sw, "fd", fd, info)
                if setting == "no-redo":
                    assert info["redo_tiles"] == 0, info
                if setting == "no-redo" and variant == "opposite" and fd == 1:
                    # Every bound equals the upper bound, 65280 / 16 646 400, so no later, tighter upper bound can take a
                    # listed patch away: what the first upper bound left is what gets scored.  (Under MAE that is little or
                    # nothing: a key carries the scan index, and only patches in front of the upper bound's own candidate can
                    # still undercut it.  Under MSE the bounds travel rounded down, and a tie stays listed.)
                    assert info["surviving"] == info["listed"], info
                    assert info["listed"] > 0 or pnorm == 0, info
                if setting == "redo-all" and fd == 1:
                    assert info["redo_tiles"] <= _tiles(info, H, W, 2), info
                    if variant in ("near_max", "bits", "cell_pan"):
                        assert info["redo_tiles"] > 0, info
                    redo += info["redo_tiles"]
    if setting == "redo-all":
        assert redo > 0


@pytest.mark.parametrize("setting", list(SEA_SETTINGS))
@pytest.mark.parametrize("sw", sc.BS16_SWS, ids=_sw_id)
def test_elimination_mae(native, monkeypatch, sw, setting):
    """k_exh_sea16<R> / k_exh_sea16p<R,.>, R = 1 .. 5 (R <= 3: penalty-seeded bounds for edge blocks, R >= 4: the guarded
    form), and k_exh_redo16<R,false> behind them: SADs and L1 bounds at 65280, keys sad << 13 | index, packed u16 sums."""
    _sea(native, monkeypatch, sw, setting, 0)


@pytest.mark.parametrize("setting", [s for s in SEA_SETTINGS if s != "quota0"])
@pytest.mark.parametrize("sw", sc.BS16_SWS, ids=_sw_id)
def test_elimination_mse_vector_unit(native, monkeypatch, sw, setting):
    """k_exh_sea16_mse<R> / k_exh_sea16p_mse<R,.> with GME_EXH_MFMA=0 (R >= 4: lower_bounds_l1 and bounds2_patch), and
    k_exh_redo16<R,true>: doubled quadrant differences at +-32640, the clamp of the squared bound, 37-bit keys."""
    _sea(native, monkeypatch, sw, setting, 1)


# ---------------------------------------------------------------------------
# matrix-core MSE and brute force
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sw,forced", [(0, None), (8, None), (16, None), (24, "1"), (32, "1")], ids=lambda v: _sw_id(v) if isinstance(v, int) else "forced" if v else "default")
def test_matrix_core_mse(native, monkeypatch, sw, forced):
    """k_exh_mfma16<NT>: the default at sw <= 16, GME_EXH_MFMA=1 beyond; whole blocks at 0 against whole blocks at 255."""
    if forced:
        monkeypatch.setenv("GME_EXH_MFMA", forced)
    for H, W in sc.BS16_SHAPES[sw]:
        for variant in sc.VARIANTS:
            _check_case(native, variant, H, W, 16, sw, 0, 1, r"k_exh_mfma16<%d> " % ((2 * sw + 16) // 16))


@pytest.mark.parametrize("pnorm", [0, 1], ids=_norm_id)
@pytest.mark.parametrize("sw", [8, 16], ids=_sw_id)
def test_brute_force(native, monkeypatch, sw, pnorm):
    """GME_EXH_BRUTE=1: k_exh_qsad16<R> (MAE) and k_exh_dot16<R> (MSE)."""
    monkeypatch.setenv("GME_EXH_BRUTE", "1")
    for H, W in sc.BS16_SHAPES[sw]:
        for variant in sc.VARIANTS:
            _check_case(native, variant, H, W, 16, sw, 0, pnorm, r"%s<%d> " % ("k_exh_dot16" if pnorm else "k_exh_qsad16", R_OF[sw]))


# ---------------------------------------------------------------------------
# geometry-fixed persistent instances
# ---------------------------------------------------------------------------
FIXED_FRAMES = ((64, 128), (112, 176))


@pytest.mark.parametrize("pnorm", [0, 1], ids=_norm_id)
@pytest.mark.parametrize("sw", [16, 32], ids=_sw_id)
def test_geometry_fixed_persistent(native, monkeypatch, sw, pnorm):
    """k_exh_sea16p[_mse]<3,5> with 2x4 tiles (sw 16) and <5,7> with 2x6 tiles (sw 32), both norms on the vector unit, under
    GME_SEA_PERSIST=2.  Frames needed: 64x128 already gives both instances (the geometry follows from the tile shape plan()
    picks, and it picks 2x4 / 2x6 from 3 x 5 blocks on -- the "persistent" ids of the elimination tests run them as well);
    112x176 adds tiles with neighbours on every side at sw 16."""
    monkeypatch.setenv("GME_SEA_PERSIST", "2")
    monkeypatch.setenv("GME_EXH_MFMA", "0")
    R, NV, tiles = {16: (3, 5, "2x4"), 32: (5, 7, "2x6")}[sw]
    plan = r"k_exh_sea16p%s<%d,%d> tiles %s persistent-dynamic geometry-fixed " % ("_mse" if pnorm else "", R, NV, tiles)
    for H, W in FIXED_FRAMES:
        for variant in ("near_max",) + sc.variants_of("half_split"):
            _check_case(native, variant, H, W, 16, sw, 0, pnorm, plan, distances=(1,))


# ---------------------------------------------------------------------------
# walks at bs 16
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pnorm", [0, 1], ids=_norm_id)
def test_diamond_bs16(native, pnorm):
    """k_walk16<PNORM>: MSE costs carry MSE_BIAS and must order like the SSD up to 16 646 400."""
    for H, W in sc.WALK16_SHAPES[16]:
        for variant in sc.VARIANTS:
            _check_case(native, variant, H, W, 16, 2, 3, pnorm, r"k_walk16<%d> \(diamond\)" % pnorm)


@pytest.mark.parametrize("pnorm", [0, 1], ids=_norm_id)
@pytest.mark.parametrize("procedure", [1, 2], ids=_proc_id)
@pytest.mark.parametrize("sw", sc.WALK16_SWS, ids=_sw_id)
def test_step_walks_bs16(native, sw, procedure, pnorm):
    """k_walk16s<PNORM,PROC,FITS>: three-step and 2-D log; the widest round fits the cached window at sw 4 and 16, not at 32."""
    plan = r"k_walk16s<%d,%d,%s> " % (pnorm, procedure, "true" if sw <= 16 else "false")
    for H, W in sc.WALK16_SHAPES[sw]:
        for variant in sc.VARIANTS:
            _check_case(native, variant, H, W, 16, sw, procedure, pnorm, plan)


# ---------------------------------------------------------------------------
# other block sizes
# ---------------------------------------------------------------------------
def _other_sizes(native, bs, shape, walk_plan):
    """Every search and norm at one block size: `walk_plan(pnorm)` is the walks' kernel, the exhaustive search is k_exh_generic."""
    H, W = shape
    for sw in sc.OTHER_SWS:
        for variant in sc.VARIANTS:
            for pnorm in (0, 1):
                f32 = " \\(float32-order costs\\)" if pnorm == 1 and 65025 * bs * bs >= 2 ** 24 else ""
                _check_case(native, variant, H, W, bs, sw, 0, pnorm, r"k_exh_generic%s grid" % f32, distances=(1,))
                for procedure in (1, 2, 3):
                    _check_case(native, variant, H, W, bs, sw, procedure, pnorm, walk_plan(pnorm), distances=(1,))


@pytest.mark.parametrize("bs", sc.WALKQ_SIZES, ids=_bs_id)
def test_walkq_block_sizes(native, bs):
    """k_walkq<BS,PNORM> (32-bit group sums of up to BS^2 * 65025, per-lane aa + bb - 2ab); MSE above bs 16 leaves it for
    k_walk<1> in float32 order; k_exh_generic for the exhaustive search."""
    def plan(pnorm):
        if pnorm == 1 and bs > 16:
            return r"k_walk<1> \(float32-order costs\)"
        return r"k_walkq<%d,%d> " % (bs, pnorm)
    _other_sizes(native, bs, sc.other_shape(bs), plan)


@pytest.mark.parametrize("bs", sc.WALK_SIZES, ids=_bs_id)
def test_walk_single_bytes(native, bs):
    """k_walk<G> at block sizes that are no multiple of 4 (16 lanes per block at bs 6, 64 at bs 10)."""
    G = 16 if bs * bs <= 64 else 64
    _other_sizes(native, bs, sc.other_shape(bs), lambda pnorm: r"k_walk<%d> grid" % G)


@pytest.mark.parametrize("bs", [16, 2], ids=_bs_id)
def test_generic_kernels_at_bs16_and_bs2(native, monkeypatch, bs):
    """GME_FORCE_GENERIC=1 routes bs 16 and bs 2 through k_walk<G> and k_exh_generic."""
    monkeypatch.setenv("GME_FORCE_GENERIC", "1")
    G = 64 if bs == 16 else 1
    _other_sizes(native, bs, (48, 80) if bs == 16 else sc.DENSE_SHAPE, lambda pnorm: r"k_walk<%d> grid" % G)


# ---------------------------------------------------------------------------
# float32-order costs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("procedure", [0, 1, 2, 3], ids=_proc_id)
@pytest.mark.parametrize("bs", sc.F32_BLOCK_SIZES, ids=_bs_id)
def test_float32_order_costs(native, bs, procedure):
    """MSE above bs 16 on the case of F32_CASES at which the float32-order field differs from the integer-order one: the
    device must give the float32-order field (pairwise_f32 of bbme_kernels.hip against NumPy's summation order)."""
    import bbme
    co = c_oracle()
    ctx = native.default_context()
    prev, cur = sc.f32_pair(bs, procedure)
    want = co.bbme(prev, cur, bs, sc.F32_SW, procedure, 1, allow_inexact=0)
    exact = co.bbme(prev, cur, bs, sc.F32_SW, procedure, 1, allow_inexact=1)
    assert not np.array_equal(want, exact)
    got = bbme.get_motion_field(prev, cur, bs, sc.F32_SW, procedure, 1)
    plan = ctx.last_bbme_info()["plan"]
    assert plan.startswith("k_exh_generic (float32-order costs)" if procedure == 0 else "k_walk<1> (float32-order costs)"), plan
    assert np.array_equal(got, want), (bs, procedure, int((got != want).any(axis=-1).sum()), int((got != exact).any(axis=-1).sum()))
    mv, info = _search(native, np.stack([prev, cur]), 1, bs, sc.F32_SW, procedure, 1)
    assert info["plan"] == plan and np.array_equal(mv[0], want), (bs, procedure)


# ---------------------------------------------------------------------------
# dense field
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["opposite", "near_max", "bits"])
def test_dense_field(native, variant):
    """k_dense2<1> as gme_begin reaches it (bs 2, sw 2, diamond, MSE on pyramid level 0) on the smallest frames gme_begin
    accepts, and k_dense2 of both norms on the full-resolution frames."""
    co = c_oracle()
    ctx = native.default_context()
    H, W = sc.DENSE_SHAPE
    st = _stack(variant, H, W, 2)
    l0 = [co.pyrdown(co.pyrdown(f)) for f in st]
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(st))
    try:
        seq.gme_begin(1, 16)
        for p in range(2):
            assert np.array_equal(seq.read_frame(p, 0), l0[p]), (variant, p)
            assert np.array_equal(seq.gme_read_stage(0, p)["gt"], co.bbme(l0[p], l0[p + 1], 2, 2, 3, 1)), (variant, p)
    finally:
        seq.close()
    mv, info = _search(native, np.stack(l0), 1, 2, 2, 3, 1)                    # the same search, asked for directly: names its kernel
    assert info["plan"].startswith("k_dense2<1> "), info["plan"]
    for p in range(2):
        assert np.array_equal(mv[p], co.bbme(l0[p], l0[p + 1], 2, 2, 3, 1)), (variant, p)
    for pnorm in (0, 1):
        _check_case(native, variant, H, W, 2, 2, 3, pnorm, r"k_dense2<%d> " % pnorm)
