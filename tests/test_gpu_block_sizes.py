"""The seven one-wave-per-block passes (k_interp, k_retime, k_bipred, k_gmc, k_prop, k_hier, k_vbs: the scaffold of
csrc/bbme_wave_lds.h) at every block size their argument rules admit, 4 .. 64, through the one-shot entry points against the
host definitions, byte for byte and with no tolerance: odd sides (one and three live bytes in a row's last dword), 17 .. 31 and
33 .. 63 (rows of 5 .. 15 dwords, LDS slices of every size, rows-per-lane splits with a remainder), children and coarse blocks
of odd side, and the per-pixel frame kernels at block edges that are no multiple of four.  The cases, and the host results that
several tests share, are tests/block_size_cases.py's; tests/test_block_size_cases_host.py shows on the CPU that they reach every
output.  Every call also asserts the kernel instance that served it.  Needs an MI355X."""
import numpy as np
import pytest

import block_size_cases as bs

pytestmark = pytest.mark.gpu

NAMES = {"interp": ("mv", "cost", "dist", "frame", "sse"), "retime": ("mv", "cost", "dist", "frame", "sse"),
         "bipred": ("mode", "v0", "v1", "cost", "costs", "predicted", "sse"), "gmc": ("mode", "cost", "costs", "predicted", "sse"),
         "prop": ("mf", "cost", "source"), "vbs": ("leaf", "depth", "cost"), "hier": ("field", "cost")}


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def same(what, names, got, want):
    """Every output of a call against the definition's; a failure names the run, the output and the first differing indices."""
    assert len(got) == len(want) == len(names), (what, len(got), len(want))
    for name, g, w in zip(names, got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
            assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())
        else:
            assert g == w, (what, name, g, w)


_pyramids = {}


def pyramids(ctx, B):
    """The device's own pyramids of a size's first two frames, [level0, level1, frame] each, made once."""
    if B not in _pyramids:
        out = []
        for f in bs.content(B)[:2]:
            l1 = ctx.pyrdown(f)
            out.append([ctx.pyrdown(l1), l1, f])
        _pyramids[B] = out
    return _pyramids[B]


def call(ctx, name, B, pnorm, args):
    """One run through the pass's one-shot entry point -> its outputs in the order of block_size_cases.want."""
    f0, f1, f2, fa, fb = bs.content(B)
    if name == "interp":
        return ctx.interp(f0, f2, B, args[0], pnorm, args[1], truth=f1)
    if name == "retime":
        return ctx.retime(f0, f2, B, args[0], pnorm, args[1], args[2], args[3], truth=f1)
    if name == "bipred":
        return ctx.bipred(f0, f1, f2, fa, fb, B, args[0], args[1], pnorm, args[2])
    if name == "gmc":
        return ctx.gmc(f0, f1, np.array(bs.WARP), fa, B, pnorm, args[0])
    if name == "prop":
        return ctx.prop(f0, f1, fa, B, pnorm, args[0], args[1], fb if args[2] else None, bs.camera_field(B) if args[2] else None)
    if name == "hier":
        return ctx.hier(f0, f1, B, args[1], args[2], pnorm, args[0])
    if name == "vbs":
        return ctx.vbs(f0, f1, fa, B, args[0], args[1], pnorm, args[2])
    raise KeyError(name)


def check_levels(native, B, pnorm, args):
    """The levels below the frame, which gme_hier_u8 does not return: gme_seq_hier on the same pair, every level's field and
    cost against hier.search on the sequence's own pyramids."""
    import hier
    ctx = native.default_context()
    levels, cw, r = args
    seq = native.Sequence.from_frames(ctx, np.stack(bs.content(B)[:2]))
    seq.hier(1, B, cw, r, pnorm, levels)
    plan = ctx.last_bbme_info()["plan"]
    pyr = [[seq.read_frame(k, l) for l in range(3)] for k in range(2)]
    got = {l: seq.read_hier(l) for l in range(3 - levels, 3)}
    seq.close()
    assert plan.startswith(bs.plan("hier", B, args) + " "), ("hier", B, pnorm, args, plan)
    want_f, want_c = hier.search(pyr[0], pyr[1], B, cw, r, pnorm, levels)
    for l in want_f:
        same(("gme_seq_hier", B, pnorm, args, "level %d" % l), NAMES["hier"], (got[l][0][0], got[l][1][0]), (want_f[l], want_c[l]))


def sweep(native, name, which):
    ctx = native.default_context()
    for B, pnorm, args in bs.runs(name, which):
        what = (name, B, pnorm, args)
        got = call(ctx, name, B, pnorm, args)
        plan = ctx.last_bbme_info()["plan"]
        assert plan.startswith(bs.plan(name, B, args) + " "), (what, plan)
        if name == "hier":
            prev, cur = pyramids(ctx, B)
            same(what, NAMES[name], got, bs.hier_want(prev, cur, B, pnorm, args)[:2])
            if args[0] > 1:
                check_levels(native, B, pnorm, args)
        else:
            same(what, NAMES[name], got, bs.want(name, B, pnorm, args))


def test_interp_all(native):
    """k_interp and k_interp_frame at every side 4 .. 64: window 2, both norms, without a bias and at the tool's default one,
    the interpolated plane and its squared error against the middle frame included."""
    sweep(native, "interp", "all")


def test_interp_corners(native):
    """The same at the largest window, 8, at 5, 7, 13, 15, 17, 31, 33, 47 and 63."""
    sweep(native, "interp", "corners")


def test_retime_all(native):
    """k_retime and k_retime_frame at every side: window 2, phase 2/5, both norms, without a bias and at the default one."""
    sweep(native, "retime", "all")


def test_retime_corners(native):
    """The same at the largest window, 16, and the phases 7/12 and 63/64, at the nine corner sizes."""
    sweep(native, "retime", "corners")


def test_bipred_all(native):
    """k_bipred and k_predict_bipred at every side: radius 1, one round, both norms, penalty 0 and the tool's default one; both
    fields hold vectors that point outside the frame, so all four modes occur."""
    sweep(native, "bipred", "all")


def test_bipred_corners(native):
    """The same at radius 2 and two rounds, at the nine corner sizes."""
    sweep(native, "bipred", "corners")


def test_gmc_all(native):
    """k_gmc and k_predict_gmc at every side under a quarter-pel translation whose sample points all lie inside the frame (the
    global predictor's bilinear taps straddle every dword boundary), both norms, penalty 0."""
    sweep(native, "gmc", "all")


def test_gmc_corners(native):
    """The same at penalty 0 and the default penalty, at the nine corner sizes (gmc has no window to enlarge)."""
    sweep(native, "gmc", "corners")


def test_prop_all(native):
    """k_prop at every side: two rounds, one refinement step, both norms, without and with the temporal and camera fields."""
    sweep(native, "prop", "all")


def test_prop_corners(native):
    """The same at four rounds and four steps, at the nine corner sizes."""
    sweep(native, "prop", "corners")


def test_hier_all(native):
    """k_hier at every side, at one level and at the most levels the side admits (odd coarse blocks at 10, 14, 20, 28, ...):
    coarse window 2, radius 1, both norms, gme_hier_u8 against hier.search on ctx.pyrdown's pyramids; with more than one
    level also every level's field and cost of gme_seq_hier."""
    sweep(native, "hier", "all")


def test_hier_corners(native):
    """The same at coarse window 8 and radius 3, at 10, 14, 20, 28, 30, 34, 36, 44, 52, 60 and 62 with their most levels."""
    sweep(native, "hier", "corners")


def test_vbs_all(native):
    """k_vbs at every side, at depth 0 and at the largest depth the side admits (children that start at odd byte offsets at
    10, 14, 20, 28, ...): radius 1, penalty 0, both norms; most roots split to the full depth."""
    sweep(native, "vbs", "all")


def test_vbs_corners(native):
    """The same at radius 3, penalty 0 and the default penalty, at the eleven corner sizes with their largest depth."""
    sweep(native, "vbs", "corners")


@pytest.mark.parametrize("B", (13, 20))
def test_sequence(native, monkeypatch, B):
    """A resident sequence of a size's three frames, one pair per launch (GME_MAX_GRID_PAIRS=1): the exhaustive search, the
    tree at the largest depth on its field, k_compensate_vbs on the leaf cells (13 pixels at depth 0; 5 pixels for 20 at depth
    2, which no other test reaches) and gme_seq_interp, every pair against vbs.tree, subpel.compensate_integer and
    interp.search / interp.interpolate."""
    import interp
    import subpel
    import vbs
    monkeypatch.setenv("GME_MAX_GRID_PAIRS", "1")
    ctx = native.default_context()
    frames = np.stack(bs.content(B)[:3])
    D = bs.max_depth(B)
    for pnorm in bs.NORMS:
        seq = native.Sequence.from_frames(ctx, frames)
        seq.bbme(1, B, 6, 0, pnorm)
        mv = seq.read_mv()
        seq.vbs(1, B, D, 1, pnorm, 0)
        plan = ctx.last_bbme_info()["plan"]
        assert plan.startswith(bs.plan("vbs", B, (D, 1, 0)) + " "), (B, pnorm, plan)
        tree = seq.read_vbs()
        sse = seq.compensate_vbs(1, B)
        comp = seq.read_compensated_range(0, 2)
        bias = interp.default_bias(B, pnorm)
        made = seq.interp(1, B, 2, pnorm, bias)
        plan = ctx.last_bbme_info()["plan"]
        assert plan.startswith(bs.plan("interp", B, (2, bias)) + " "), (B, pnorm, plan)
        seq.close()
        assert mv.shape == (2, 2, 5, 2) and mv.any()
        for k in (0, 1):
            want = vbs.tree(frames[k], frames[k + 1], mv[k], B, D, 1, pnorm, 0)
            same(("gme_seq_vbs", B, pnorm, k), NAMES["vbs"], [a[k] for a in tree], want)
            want_comp = subpel.compensate_integer(frames[k], want[0], B >> D)
            same(("gme_seq_compensate_vbs", B, pnorm, k), ("compensated", "sse"), (comp[k], int(sse[k])),
                 (want_comp, subpel.sse(frames[k + 1], want_comp)))
            want = interp.search(frames[k], frames[k + 1], B, 2, pnorm, bias)
            want = want + (interp.interpolate(frames[k], frames[k + 1], want[0], B), -1)
            same(("gme_seq_interp", B, pnorm, k), NAMES["interp"], [a[k] for a in made[:4]] + [int(made[4][k])], want)
