"""The affine device solve (k_solve3 through gme_solve_fit_sums and gme_seq_gme_device_solve) on the device: bit-equal to
tests/solve_cases.py's restatement, and under the contract "unflagged means bit-equal to the host path downstream of the
solve" on ill-conditioned, singular and large-motion systems; the second-order solve (k_solve_model2) under the same stress.
The inputs are sums, except in the last test.  Needs an MI355X."""
import numpy as np
import pytest

import solve_cases as sc
from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


class Case:
    def __init__(self, name, family, h, w, project, sums):
        self.name, self.family, self.h, self.w, self.project, self.sums = name, family, h, w, project, sums
        self.well_spread = family in sc.WELL_SPREAD


@pytest.fixture(scope="module")
def cases():
    """The catalogue and the trap file as one list."""
    out = [Case(s.name, s.family, s.h, s.w, s.project, s.sums) for s in sc.catalogue()]
    t = np.load(GOLDEN_DIR + "/solve3_traps.npz")
    out += [Case("trap %d" % k, "trap", int(t["h"][k]), int(t["w"][k]), bool(t["project"][k]), t["sums"][k]) for k in range(len(t["h"]))]
    return out


@pytest.fixture(scope="module")
def device(native, cases):
    """{case name: (params, flags)}: one gme_solve_fit_sums call per (h, w, project) group."""
    ctx = native.default_context()
    out = {}
    for (h, w, project), group in sc.groups(cases).items():
        params, flags = ctx.solve_fit_sums(np.stack([c.sums for c in group]), h, w, project=project)
        for c, p, f in zip(group, params, flags):
            out[c.name] = (p.copy(), int(f))
    assert len(out) == len(cases)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _host(sums, project):
    """The package's host path: roadmap.solve_model (stacked inv / matmul) and roadmap.project; None where it raises."""
    import roadmap
    try:
        p = roadmap.solve_model(np.asarray(sums)[None], "affine")
    except np.linalg.LinAlgError:
        return None
    return (roadmap.project(p) if project else p)[0]


def test_device_equals_restatement(cases, device):
    """Parameters bit for bit, flags equal: pins the operation order on the device, so that tests/test_solve3_host.py
    speaks for it."""
    for c in cases:
        want_p, want_f = sc.device_np(c.sums, c.h, c.w, c.project)
        got_p, got_f = device[c.name]
        assert np.array_equal(_bits(got_p), _bits(want_p)), (c.name, got_p, want_p)
        assert got_f == want_f, (c.name, got_f, want_f)


def test_contract_against_host(native, cases, device):
    ctx = native.default_context()
    unflagged = clear = 0
    for c in cases:
        dev, flags = device[c.name]
        if c.family in sc.SINGULAR:
            assert flags & 4, (c.name, flags)
        if c.family == "trap" or c.family in sc.NEAR_SINGULAR:
            assert flags != 0, c.name
        host = _host(c.sums, c.project)
        if flags == 0:
            unflagged += 1
            assert host is not None and np.all(np.isfinite(host)), c.name
            assert np.array_equal(ctx.affine_field(dev, c.h, c.w), ctx.affine_field(host, c.h, c.w)), c.name
            assert sc.contract_violations(dev, host, c.h, c.w) == [], c.name
        if c.well_spread and sc.clear_of_ties(host, c.h, c.w, 1e-8):
            clear += 1
            assert flags == 0, (c.name, flags)
    assert clear >= 216 and unflagged >= clear                   # nine in ten of the 240 well-spread systems


def test_edges_of_the_call(native):
    import roadmap
    ctx = native.default_context()
    params, flags = ctx.solve_fit_sums(np.zeros((0, 15)), 30, 45)
    assert params.shape == (0, 6) and flags.shape == (0,)

    def one(h, w, p, project=False):
        """S = F p over the whole h x w field through the device, checked against the restatement."""
        sums = sc.sums_of_params(sc.moments(np.ones((h, w), bool), h, w), p)
        got_p, got_f = ctx.solve_fit_sums(sums[None], h, w, project=project)
        want_p, want_f = sc.device_np(sums, h, w, project)
        assert np.array_equal(_bits(got_p[0]), _bits(want_p)) and got_f[0] == want_f, (h, w, p, got_p, want_p, got_f, want_f)
        return got_p[0], int(got_f[0])

    # h w = 1: a single block determines no plane
    assert one(1, 1, [1.25, 0, 0, -2.25, 0, 0])[1] & 4
    # h w = 257, one block past the 256-thread stride of the field scan: only block 256 sits on a tie (the sums are a
    # 30 x 45 grid's: the field the flag scans is the caller's choice)
    F = sc.moments(np.ones((30, 45), bool), 30, 45)
    for h, w in ((1, 257), (257, 1)):
        slope = [0.0, 1.0 / 1024] if h == 1 else [1.0 / 1024, 0.0]
        sums = sc.sums_of_params(F, [0.25, slope[0], slope[1], 0.125, 0.0, 0.0])       # 0.25 + 256 / 1024 = 0.5
        got_p, got_f = ctx.solve_fit_sums(sums[None], h, w)
        want_p, want_f = sc.device_np(sums, h, w)
        assert np.array_equal(_bits(got_p[0]), _bits(want_p)) and got_f[0] == want_f == 1, (h, w, got_f, want_f)
        _, got_f = ctx.solve_fit_sums(sums[None], *((1, 256) if h == 1 else (256, 1)))      # the same parameters, 256 blocks
        assert got_f[0] == 0, (h, w, got_f)
    # ... and on a field with both extents: 3 x 86 = 258 blocks, the tie at block 256 = (2, 84)
    h, w = 3, 86
    tie = [0.25, 1.0 / 16, 1.0 / 672, -3.3, 0.001, 0.002]                # 0.25 + 2 / 16 + 84 / 672 = 0.5
    got_p, got_f = one(h, w, tie)
    d = sc.field_values(got_p, h, w)
    near = np.abs((d - np.floor(d)) - 0.5) <= 1e-9
    assert got_f == 1 and np.array_equal(np.argwhere(near), [[0, 256]]), (got_f, np.argwhere(near))
    # 1000 systems in one call: every row equals the restatement, a sample equals its single-system call
    rng = np.random.default_rng(11)
    many = np.stack([sc.sums_of_params(F, sc._draw_params(rng, rng.uniform(-300, 300))) for _ in range(1000)])
    params, flags = ctx.solve_fit_sums(many, 30, 45)
    for k in range(1000):
        want_p, want_f = sc.device_np(many[k], 30, 45)
        assert np.array_equal(_bits(params[k]), _bits(want_p)) and flags[k] == want_f, k
    for k in rng.integers(0, 1000, 16):
        p1, f1 = ctx.solve_fit_sums(many[k][None], 30, 45)
        assert np.array_equal(_bits(p1[0]), _bits(params[k])) and f1[0] == flags[k], k
    # NaN and inf anywhere in the sums: flagged, beside healthy neighbours that are not
    bad = np.stack([many[0]] * 32)
    where = [(r, c) for r, c in zip(range(1, 31), list(range(15)) * 2)]
    for r, c in where:
        bad[r, c] = np.nan if r <= 15 else np.inf
    params, flags = ctx.solve_fit_sums(bad, 30, 45)
    assert flags[0] == 0 and flags[31] == 0 and np.array_equal(_bits(params[0]), _bits(params[31]))
    for r, c in where:
        assert flags[r] != 0, (r, c, flags[r], params[r])
        assert flags[r] == sc.device_np(bad[r], 30, 45)[1], (r, c)
    # project: the host's doubling of p0 and p3 on the unprojected device solution, bit for bit
    plain, _ = ctx.solve_fit_sums(many[:64], 30, 45)
    proj, _ = ctx.solve_fit_sums(many[:64], 30, 45, project=True)
    assert np.array_equal(_bits(proj), _bits(roadmap.project(plain)))


ORDER2 = [("bilinear", 3), ("pseudo_perspective", 4), ("quadratic", 4)]       # (model, block columns of its "cols" inlier set)


def _order2_keep(kind, n, h, w, rng):
    keep = np.zeros((h, w), bool)
    if kind == "cols":
        keep[:, w - n:] = True
    elif kind == "corner4x4":
        keep[h - 4:, w - 4:] = True
    else:
        keep = sc.inliers(kind, h, w, rng)
    return keep


def test_second_order_models_under_the_same_stress(native):
    import roadmap
    from test_gpu_models2_solve import clear_of_ties, contract_violations, sums_of_field
    ctx = native.default_context()
    rng = np.random.default_rng(5)
    assert np.array_equal(sc.sums_of_field2(np.arange(12) * 1e-3, 30, 45, _order2_keep("cols", 3, 30, 45, rng)),
                          sums_of_field(np.arange(12) * 1e-3, 30, 45, 16, cols=[42, 43, 44]))
    unflagged = 0
    for h, w in ((30, 45), (135, 240)):
        for model, ncols in ORDER2:
            names, sums = [], []
            for kind in ("cols", "corner4x4", "random70", "all"):
                keep = _order2_keep(kind, ncols, h, w, rng)
                for t in (12.3, 200.7, -12.3, -200.7):
                    p = np.zeros(12)
                    p[:6] = sc._draw_params(rng, t)
                    p[6:] = rng.normal(0, 2e-4, 6)
                    if model == "bilinear":
                        p[[6, 8, 9, 11]] = 0
                    if model == "pseudo_perspective":
                        p[6] = p[11] = 0
                        p[9], p[10] = p[7], p[8]
                    names.append((h, model, kind, t))
                    sums.append(sc.sums_of_field2(p, h, w, keep) if kind != "cols" else
                                sums_of_field(p, h, w, 16, cols=list(range(w - ncols, w))))
            dev, flags = ctx.solve_model2_sums(np.stack(sums), model, h, w)
            for k, name in enumerate(names):
                try:
                    host = roadmap.solve_model(sums[k], model)[0]
                except np.linalg.LinAlgError:
                    assert flags[k] & 12, (name, flags[k])
                    continue
                if name[2] == "all" and clear_of_ties(host, h, w)[0]:
                    assert flags[k] == 0, (name, flags[k])
                if flags[k] == 0:
                    unflagged += 1
                    assert contract_violations(dev[k], host, h, w) == [], name
                    assert np.array_equal(ctx.model2_field(dev[k], h, w), ctx.model2_field(host, h, w)), name
    assert unflagged >= 24                                        # at least half of the full and the 70 % grids


def test_end_to_end_at_large_motion(native):
    """Exhaustive search at window 24 on a moving texture: gme_seq_gme_device_solve against the staged host path."""
    import motion
    frac = float(motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE)
    assert int(motion.BBME_BLOCK_SIZE) == 16
    for shift in sc.LARGE_SHIFTS:
        frames = sc.large_motion_frames(shift)
        seq = native.Sequence.from_frames(native.default_context(), frames)
        try:
            host = motion.estimate_sequence(seq, 1, procedure=0, search_window=24)
            sse_h = np.array(seq.compensate(1, 16, host))
            comp_h = [seq.read_compensated(i) for i in range(3)]
            params, sse, flags = seq.gme_device_solve(1, 16, frac, 0, 24)
            params, sse, flags = np.array(params), np.array(sse), np.array(flags)
            assert params.shape == (3, 6) and not np.any(flags), (shift, flags)
            assert np.max(np.abs(host[:, [0, 3]])) > 5                  # large motion indeed
            assert np.allclose(params, host, rtol=1e-10, atol=0), (shift, params - host)
            assert sc.contract_violations(params, host, 6, 8) == [], shift
            assert np.array_equal(sse, sse_h), shift
            for i in range(3):
                assert np.array_equal(seq.read_compensated(i), comp_h[i]), (shift, i)
        finally:
            seq.close()
