"""The cases of tests/block_size_cases.py on the host alone: what keeps tests/test_gpu_block_sizes.py from passing vacuously.
The seed table is what find_seed yields and the fields have blocks inside and outside; the searches leave the centre, the trees
split to their full depth, the decisions use every mode and source; and the argument tables hold exactly the sizes the
definitions' own check_args admit.  Host arrays and host definitions only."""
import numpy as np

import block_size_cases as bs
import bipred
import gmc
import hier
import interp
import propagate
import retime
import vbs


def test_seed_table():
    """The committed table is find_seed's, no size needs more than s = 1, and at it every size's two fields hold a displaced
    block inside and one outside each, one block with both inside and one with both outside."""
    assert bs.SEED == {B: bs.find_seed(B) for B in bs.ALL}
    assert max(bs.SEED.values()) <= 1
    for B in bs.ALL:
        f0, f1, f2, fa, fb = bs.content(B)
        assert f0.shape == f1.shape == f2.shape == (2 * B + 1, 5 * B + 3) and fa.shape == fb.shape == (2, 5, 2)
        assert max(np.abs(fa).max(), np.abs(fb).max()) <= 6
        m = bs.inside_maps(B, (fa, fb))
        for k in (0, 1):
            assert m[k].any() and not m[k].all(), (B, k)
        assert (m[0] & m[1]).any() and (~m[0] & ~m[1]).any(), B
    assert bs.shape(64) == (129, 323)


def test_searches_move():
    """interp, retime and hier at the light arguments: at least half of the ten blocks take a vector other than the centre, at
    every size and under both norms (on noise the centre is one candidate of 25; the bias makes it likelier)."""
    worst = {}
    for name in ("interp", "retime", "hier"):
        for B, pnorm, args in bs.runs(name, "all"):
            if name == "hier":
                f0, f1 = bs.content(B)[:2]
                mv = bs.hier_want(bs.host_pyramid(f0), bs.host_pyramid(f1), B, pnorm, args)[0]
            else:
                mv = bs.want(name, B, pnorm, args)[0]
            moved = int(np.any(mv != 0, axis=2).sum())
            assert mv.shape == (2, 5, 2) and moved >= 5, (name, B, pnorm, args, moved)
            worst[name] = min(worst.get(name, 10), moved)
    print("blocks of ten that leave the centre, worst case per pass:", worst)


def full_depth_roots(depth_map, D):
    """bool[2, 5]: the roots that split all the way down: every cell is a leaf of depth D."""
    n = 1 << D
    return (depth_map.reshape(2, n, 5, n) == D).all(axis=(1, 3))


def test_trees_split():
    """vbs at penalty 0, every (B, depth >= 1) under both norms: at least half of the roots whose vector lies inside split to
    the full depth, so the children's arithmetic reaches the outputs; a root whose vector lies outside has cost -1."""
    worst = None
    for B, pnorm, args in bs.runs("vbs", "all"):
        D = args[0]
        leaf, depth, cost = bs.want("vbs", B, pnorm, args)
        inside = bs.inside_maps(B, bs.content(B)[3:4])[0]
        assert np.array_equal(cost >= 0, inside), (B, pnorm, args)
        if D == 0:
            assert not depth.any()
            continue
        full = full_depth_roots(depth, D) & inside
        assert 2 * full.sum() >= inside.sum(), (B, pnorm, args, int(full.sum()), int(inside.sum()))
        if worst is None or full.sum() * worst[1] < worst[0] * inside.sum():
            worst = (int(full.sum()), int(inside.sum()), B, D, pnorm)
    print("roots split to the full depth, worst case: %d of %d at B %d, depth %d, norm %d" % worst)


def test_modes_are_spread():
    """bipred, gmc and prop at every size: in some block the candidates' costs differ (bipred's three and gmc's two columns of
    ``costs``; for prop, whose cost array has one column, some block ends at another vector than its prior one), and over the sweep every mode and source class occurs.  prop's
    ``source`` tells of the last round, where a block's own vector already is the best of the temporal, camera and zero
    candidates, which never change; so those three classes are looked for in the sweep's first round, which the device runs
    the same way before the rounds that follow.  gmc's NONE cannot: WARP keeps every sample point of every
    whole block inside the frame (the last one at column 5 B + 1.5 <= W - 1 and row 2 B - 0.25 <= H - 1), so the global
    candidate always exists; its absence is tests/test_gpu_gmc.py's subject."""
    seen = {"bipred": set(), "gmc": set(), "prop": set()}
    for which in ("all", "corners"):
        for B, pnorm, args in bs.runs("bipred", which):
            mode, _, _, _, costs = bs.want("bipred", B, pnorm, args)[:5]
            seen["bipred"] |= set(mode.ravel().tolist())
            both = (costs >= 0).all(axis=2)
            assert both.any() and any(len(set(c.tolist())) == 3 for c in costs[both]), (B, pnorm, args)
        for B, pnorm, args in bs.runs("gmc", which):
            mode, _, costs = bs.want("gmc", B, pnorm, args)[:3]
            seen["gmc"] |= set(mode.ravel().tolist())
            assert (costs[:, :, 0] >= 0).all(), (B, pnorm, args)
            both = costs[:, :, 1] >= 0
            assert both.any() and (costs[both][:, 0] != costs[both][:, 1]).any(), (B, pnorm, args)
        for B, pnorm, args in bs.runs("prop", which):
            f0, f1, _, fa, fb = bs.content(B)
            first = propagate.search(f0, f1, fa, B, pnorm, 1, args[1], fb if args[2] else None, bs.camera_field(B) if args[2] else None)[2]
            for source in (first, bs.want("prop", B, pnorm, args)[2]):
                seen["prop"] |= set((source & 7).ravel().tolist()) | set((source & propagate.MOVED).ravel().tolist())
            assert np.any(bs.want("prop", B, pnorm, args)[0] != bs.content(B)[3]), (B, pnorm, args)
    assert seen["bipred"] == {bipred.PAST, bipred.NEXT, bipred.BOTH, bipred.NONE}
    assert seen["gmc"] == {gmc.GLOBAL, gmc.LOCAL}
    assert seen["prop"] == {propagate.OWN, propagate.SPATIAL, propagate.TEMPORAL, propagate.CAMERA, propagate.ZERO, propagate.MOVED}


def admitted(check, *rest):
    """The sizes of 1 .. 70 that a definition's check_args takes with the other arguments ``rest``."""
    out = []
    for B in range(1, 71):
        try:
            check(B, *rest)
            out.append(B)
        except ValueError:
            pass
    return out


def test_tables_admit_what_the_library_admits():
    """Every size a definition's check_args accepts is in the pass's sweep and nothing else is: 4 .. 64 for the five passes
    without a divisibility rule; for hier and vbs every size at one level / depth 0 and at the largest levels / depth its rule
    admits, which no size exceeds.  Every run of both sweeps passes check_args, and the corner sizes are swept sizes."""
    sweep = list(bs.ALL)
    assert admitted(interp.check_args, 2, 0, 0) == sweep
    assert admitted(retime.check_args, 2, 0, 0) == sweep
    assert admitted(bipred.check_args, 1, 1, 0, 0) == sweep
    assert admitted(gmc.check_args, 0, 0) == sweep
    assert admitted(propagate.check_args, 0, 2, 1) == sweep
    by_levels = {levels: admitted(lambda B: hier.check_args(B, 2, 1, 0, levels)) for levels in (1, 2, 3)}
    by_depth = {depth: admitted(lambda B: vbs.check_args(B, depth, 1, 0, 0)) for depth in (0, 1, 2)}
    assert by_levels[1] == sweep and by_depth[0] == sweep
    for B in sweep:
        assert bs.max_levels(B) == max(l for l in by_levels if B in by_levels[l])
        assert bs.max_depth(B) == max(d for d in by_depth if B in by_depth[d])
    assert set(bs.HIER_ALL) == {(B, 1) for B in sweep} | {(B, bs.max_levels(B)) for B in sweep}
    assert set(bs.VBS_ALL) == {(B, 0) for B in sweep} | {(B, bs.max_depth(B)) for B in sweep}
    checks = {"interp": lambda B, p, a: interp.check_args(B, a[0], p, a[1]),
              "retime": lambda B, p, a: retime.check_args(B, a[0], p, a[1]) + retime.check_phase(a[2], a[3]),
              "bipred": lambda B, p, a: bipred.check_args(B, a[0], a[1], p, a[2]),
              "gmc": lambda B, p, a: gmc.check_args(B, p, a[0]),
              "prop": lambda B, p, a: propagate.check_args(B, p, a[0], a[1]),
              "hier": lambda B, p, a: hier.check_args(B, a[1], a[2], p, a[0]),
              "vbs": lambda B, p, a: vbs.check_args(B, a[0], a[1], p, a[2])}
    for name in bs.PASSES:
        assert sorted({B for B, _, _ in bs.runs(name, "all")}) == sweep, name
        assert {p for _, p, _ in bs.runs(name, "all")} == {0, 1}
        for which in ("all", "corners"):
            for B, pnorm, args in bs.runs(name, which):
                checks[name](B, pnorm, args)
        assert set(bs.sizes(name, "corners")) <= set(sweep)
    assert {(B, a[0]) for B, _, a in bs.runs("hier", "all")} == set(bs.HIER_ALL)
    assert {(B, a[0]) for B, _, a in bs.runs("vbs", "all")} == set(bs.VBS_ALL)
    assert {(B, a[0]) for B, _, a in bs.runs("hier", "corners")} == set(bs.HIER_CORNERS)
    assert {(B, a[0]) for B, _, a in bs.runs("vbs", "corners")} == set(bs.VBS_CORNERS)


def test_plans():
    """The instance a run is served by: compiled at 16 and 32 (64 too for hier at three levels), run-time everywhere else."""
    assert bs.plan("interp", 16, (2, 0)) == "k_interp<16>" and bs.plan("gmc", 32, (0,)) == "k_gmc<32>"
    assert bs.plan("prop", 17, (2, 1, False)) == "k_prop<0>" and bs.plan("retime", 64, (2, 0, 2, 5)) == "k_retime<0>"
    assert [bs.plan("hier", B, (bs.max_levels(B), 2, 1)) for B in (16, 32, 64, 20)] == ["k_hier<16,3>", "k_hier<32,3>", "k_hier<64,3>", "k_hier<0,0>"]
    assert bs.plan("hier", 16, (1, 2, 1)) == "k_hier<0,0>" and bs.plan("vbs", 64, (2, 1, 0)) == "k_vbs<0,0>"
    assert bs.plan("vbs", 16, (2, 1, 0)) == "k_vbs<16,2>" and bs.plan("vbs", 32, (0, 1, 0)) == "k_vbs<0,0>"
    compiled = {name: sorted({B for B, _, a in bs.runs(name, "all") if "<0" not in bs.plan(name, B, a)}) for name in bs.PASSES}
    assert compiled == {name: [16, 32, 64] if name == "hier" else [16, 32] for name in bs.PASSES}
