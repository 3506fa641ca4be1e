"""CPU-side checks of the affine device solve's contract (k_solve3 through gme_solve_fit_sums / gme_seq_gme_device_solve):
an unflagged pair is bit-equal to the host path downstream of the solve, a flagged pair goes to the host path.  Everything
here runs on tests/solve_cases.py's restatement of the kernel; tests/test_gpu_solve3.py pins the device to that restatement
bit for bit, so these tests speak for the device.

Regression: with the rule the kernel had before (plain elimination, a fixed margin of 1e-9, no conditioning flag) 25 of the 40
records of tests/golden/solve3_traps.npz were left unflagged (`old_unflagged` in the file, written by tools/solve3_traps.py)
although the device and the host field differ in one block there.  The shipped rule flags all 40."""
import numpy as np
import pytest

import solve_cases as sc
from helpers import GOLDEN_DIR, oracle_gme

EPS = 2.0 ** -53
# The restatement against the exact solution: the largest scaled error / (cond(F) 2^-53) measured over the non-singular
# catalogue is 0.024 (3 x 5, three blocks); DESIGN.md, "Opt-in device solve".  Ten times that bounds the growth with cond(F).
SLOPE_BOUND = 0.24


@pytest.fixture(scope="module")
def solved():
    """[(system, restated params, restated flags, host params or None where inv raises)] for the whole catalogue."""
    out = []
    for s in sc.catalogue():
        p, flags = sc.device_np(s.sums, s.h, s.w, s.project)
        try:
            host = sc.params_host(s.sums, s.project)
        except np.linalg.LinAlgError:
            host = None
        out.append((s, p, flags, host))
    return out


@pytest.fixture(scope="module")
def traps():
    return np.load(GOLDEN_DIR + "/solve3_traps.npz")


def test_catalogue_is_what_the_issue_lists():
    cat = sc.catalogue()
    plain = [s for s in cat if s.family in sc.FAMILIES]
    assert len(plain) == len(sc.SHAPES) * len(sc.FAMILIES) * len(sc.TRANSLATIONS) * 2 * 2
    assert {(s.h, s.w) for s in cat} == set(sc.SHAPES)
    assert {s.family for s in cat} == set(sc.FAMILIES + sc.SINGULAR + sc.NEAR_SINGULAR)
    sc._catalogue = None                                # seeded: a rebuild gives the same bits
    again = sc.catalogue()
    assert len(again) == len(cat) and all(np.array_equal(a.sums, b.sums) and a.name == b.name for a, b in zip(cat, again))


def test_well_spread_systems_are_clear_of_ties_on_the_host(solved):
    """The guard's premise, for the host solution alone: at least nine in ten well-spread systems keep 1e-8 max(1, S) away
    from every tie, at every shape."""
    for shape in sc.SHAPES:
        ws = [(s, host) for s, _, _, host in solved if s.well_spread and (s.h, s.w) == shape]
        clear = [sc.clear_of_ties(host, s.h, s.w, 1e-8) for s, host in ws]
        assert len(ws) == 60 and np.mean(clear) >= 0.9, (shape, np.mean(clear))


def test_restatement_against_exact_solution(solved):
    """Scaled error of the restated solve against the rational one, per family; it grows with cond(F) no faster than
    SLOPE_BOUND cond(F) 2^-53."""
    worst, slope = {}, {}
    for s, p, flags, _ in solved:
        if s.family not in sc.FAMILIES:
            continue
        exact = sc.params_exact(s.sums, s.project)
        assert exact is not None and not flags & 4, s.name
        err = sc.scaled_errors(p, exact, s.h, s.w).max()
        cond = np.linalg.cond(s.sums[:9].reshape(3, 3))
        worst[s.family] = max(worst.get(s.family, 0.0), err)
        slope[s.family] = max(slope.get(s.family, 0.0), err / (cond * EPS))
        assert err <= SLOPE_BOUND * cond * EPS, (s.name, err, cond)
    print("worst scaled error per family:", {k: "%.1e" % v for k, v in worst.items()})
    print("worst error / (cond 2^-53) per family:", {k: "%.3f" % v for k, v in slope.items()})
    assert max(worst[f] for f in sc.WELL_SPREAD) < 1e-11


def test_singular_families(solved):
    seen = set()
    for s, p, flags, host in solved:
        if s.family not in sc.SINGULAR:
            continue
        seen.add(s.family)
        assert flags & 4 and not np.any(p), (s.name, flags)
        assert sc.solve3_np(s.sums[:9], s.sums[9:12])[0] is None and sc.solve3_exact(s.sums[:9], s.sums[9:12]) is None
        assert host is None or not np.all(np.isfinite(host)), (s.name, host)
    assert seen == set(sc.SINGULAR)
    # rank 2 up to rounding: whatever the host returns, the device does not vouch for it
    near = [(s, flags) for s, _, flags, _ in solved if s.family in sc.NEAR_SINGULAR]
    assert len(near) == 4 * 2 * 4 and all(flags & 12 for _, flags in near), [s.name for s, f in near if not f & 12]


def _check_unflagged(name, h, w, dev, host):
    assert host is not None and np.all(np.isfinite(host)), name
    assert np.array_equal(sc.rounded_field(dev, h, w), sc.rounded_field(host, h, w)), name
    assert sc.contract_violations(dev, host, h, w) == [], name


def test_unflagged_systems_equal_the_host_path(solved, traps):
    """The shipped rule over the catalogue and the trap file: flag 0 means the host's rounded field and the parameter
    contract."""
    import roadmap
    unflagged = 0
    for s, p, flags, host in solved:
        if flags == 0:
            unflagged += 1
            _check_unflagged(s.name, s.h, s.w, p, host)
            batch = roadmap.solve_model(s.sums[None], "affine")                  # the package's own host path (stacked inv)
            _check_unflagged(s.name, s.h, s.w, p, (roadmap.project(batch) if s.project else batch)[0])
    assert unflagged >= 216                             # not by flagging everything: see the next test
    for k in range(len(traps["h"])):
        h, w, project = int(traps["h"][k]), int(traps["w"][k]), bool(traps["project"][k])
        p, flags = sc.device_np(traps["sums"][k], h, w, project)
        if flags == 0:
            _check_unflagged("trap %d" % k, h, w, p, sc.params_host(traps["sums"][k], project))


def test_clear_well_spread_systems_stay_on_the_device(solved):
    ws = [(s, flags, sc.clear_of_ties(host, s.h, s.w, 1e-8)) for s, _, flags, host in solved if s.well_spread]
    assert len(ws) == 240 and sum(c for _, _, c in ws) >= 0.9 * len(ws)
    wrong = [(s.name, flags) for s, flags, c in ws if c and flags]
    assert wrong == []
    assert {(s.h, s.w, abs(s.translation)) for s, flags, c in ws if c and not flags} == {
        (h, w, t) for h, w in sc.SHAPES for t in sc.TRANSLATIONS}


def test_every_trap_is_flagged(traps):
    n = len(traps["h"])
    assert n == 40 and set(traps["family"].tolist()) == {f[0] for f in sc.TRAP_FAMILIES}
    assert int(traps["old_unflagged"]) == int(np.sum(traps["old_flags"] == 0)) == 25
    for k in range(n):
        h, w, project = int(traps["h"][k]), int(traps["w"][k]), bool(traps["project"][k])
        p, flags = sc.device_np(traps["sums"][k], h, w, project)
        assert np.array_equal(p.view(np.uint64), traps["params"][k].view(np.uint64)), k       # the file is the restatement's
        assert flags == traps["flags"][k] and flags != 0, (k, flags)
        # the rule the kernel had: the fixed margin on the plain elimination's solution
        old = sc.flags_np(sc._params_plain(traps["sums"][k]), h, w, 0, 1, 1e-9)
        assert old == traps["old_flags"][k], k


def test_trap_search_is_deterministic():
    a = list(sc.trap_search(30, 45, "last2cols", 500.3, 5, [2024, 3]))
    b = list(sc.trap_search(30, 45, "last2cols", 500.3, 5, [2024, 3]))
    assert len(a) == 5 and all(np.array_equal(x["sums"], y["sums"]) for x, y in zip(a, b))
    for t in a:                                                          # the moved p0 put a tie between the two fields
        assert t["spread"] > 0 and sc.flags_np(t["params"], 30, 45) & 1


def _stage_flags(stages, h, w):
    """The two solves of gme_seq_gme_device_solve on one pair's CPU sums: level 1 projected and checked on the level-2
    field (bit 1), level 2 on the final field (bit 2)."""
    s1 = np.concatenate([stages[0]["F"].ravel(), stages[0]["Sx"], stages[0]["Sy"]])
    s2 = np.concatenate([stages[1]["F"].ravel(), stages[1]["Sx"], stages[1]["Sy"]])
    p1, b1 = sc.params_np(s1, True)
    p2, b2 = sc.params_np(s2, False)
    return sc.flags_np(p1, h, w, b1, 1) | sc.flags_np(p2, h, w, b2, 2)


def test_bench_content_keeps_the_device_path(golden):
    """The first 8 pairs of the benchmark's 480 x 720 content and of the reference's real frames (g9) at both settings:
    no flag, so gme720dev does not fall back."""
    import synth
    frames = synth.sequence(1234, 0, 9, 480, 720)
    for p in range(8):
        _, stages = oracle_gme(frames[p], frames[p + 1], bs=16)
        assert _stage_flags(stages, 30, 45) == 0, p
    g9 = golden("g9_pan240seq")["frames"]
    for bs, fd in ((16, 1), (12, 5)):
        for p in range(8):
            _, stages = oracle_gme(g9[p], g9[p + fd], bs=bs)
            assert _stage_flags(stages, 240 // bs, 320 // bs) == 0, (bs, fd, p)


def test_large_motion_frames_are_unflagged():
    """The premise of test_gpu_solve3.py's end-to-end test, on the CPU: exhaustive search at window 24 on the moving
    texture, both solves restated, no pair flagged."""
    for shift in sc.LARGE_SHIFTS:
        frames = sc.large_motion_frames(shift)
        assert frames.shape == (4, 96, 128)
        for p in range(3):
            _, stages = oracle_gme(frames[p], frames[p + 1], procedure=0, sw=24, bs=16)
            assert _stage_flags(stages, 6, 8) == 0, (shift, p)
