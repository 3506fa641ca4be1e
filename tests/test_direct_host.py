"""Direct projective refinement, host side (direct.py): the affine start, the level scaling, the link of the
dense compensation to the reference's block compensation, recovery of known warps, the Python / CLI surface and the new
kernels' resource remarks.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

from helpers import corner_error

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def warp_canvas(h, H, W, seed=7, y0=300, x0=500):
    """(prev, cur): an H x W crop of synth.canvas(seed) and the frame whose pixel (u, v) is the canvas sampled bilinearly
    (float64) at the crop's point warp(h, u, v), rounded to the nearest integer."""
    import direct
    import synth
    T = synth.canvas(seed).astype(np.float64)
    prev = T[y0:y0 + H, x0:x0 + W].astype(np.uint8)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    up, vp, _ = direct.warp(np.asarray(h, np.float64), u.ravel(), v.ravel())
    cur = np.floor(direct.bilinear(T, up + x0, vp + y0) + 0.5).astype(np.uint8).reshape(H, W)
    return prev, cur


def known_warps(width=160):
    """A sub-pixel translation, a 2 % zoom with 0.5 degrees of rotation, and a perspective with h6 = 2e-4 on a 160 px wide
    frame (scaled by 160 / width on wider ones, so that d spans the same 1 .. 1.03 across the frame)."""
    th, z = np.deg2rad(0.5), 1.02
    return {"subpixel_shift": np.array([1, 0, 1.3, 0, 1, -0.7, 0, 0], np.float64),
            "zoom_rotation": np.array([z * np.cos(th), -z * np.sin(th), 2.0, z * np.sin(th), z * np.cos(th), -1.5, 0, 0]),
            "perspective": np.array([1, 0, 0.5, 0, 1, 0.3, 2e-4 * 160 / width, 0], np.float64)}


def flag_cases(H=99, W=131):
    """Inputs that reach each outcome of direct.refine on an odd-sized frame: name -> (prev, cur, init,
    refine keyword arguments, flags).  prev / cur is a 2 % zoom with 0.5 degrees of rotation rendered by warp_canvas.

    FLAG_NO_GAIN is reached by identical frames at the identity: the cost is 0 at the start and at the end, and 0 < 0 fails.
    The exact warp of a rendered pair does not reach it: rounding the rendering to uint8 leaves a warp near the exact one
    whose cost is a little lower, and the refinement finds it."""
    import direct
    prev, cur = warp_canvas(known_warps(W)["zoom_rotation"], H, W)
    flat = np.full((H, W), 128, np.uint8)
    ident = direct.IDENTITY
    return {
        "singular": (flat, flat, ident, {}, direct.FLAG_SINGULAR),                           # no gradient: JtJ = 0
        "denominator": (prev, cur, np.array([1, 0, 0, 0, 1, 0, -2.0 / W, 0]), {}, direct.FLAG_DENOMINATOR),  # d < 0 at u = W-1
        "few_valid": (prev, cur, np.array([1, 0, 0.8 * W, 0, 1, 0, 0, 0]), {}, direct.FLAG_FEW_VALID),  # ~20 % samples inside
        "max_iters_1": (prev, cur, ident, {"max_iters": 1}, direct.FLAG_MAX_ITERS),
        "max_iters_2": (prev, cur, ident, {"max_iters": 2, "outlier_fraction": 0.3}, direct.FLAG_MAX_ITERS),
        "no_gain": (prev, prev, ident, {}, direct.FLAG_NO_GAIN),
        "converged": (prev, cur, ident, {}, 0),
        "converged_f0": (prev, cur, ident, {"outlier_fraction": 0.0, "max_iters": 20}, 0),
        "converged_f05": (prev, cur, ident, {"outlier_fraction": 0.5, "max_iters": 60}, 0),         # 42 iterations at level 2
    }


def full_hd_case():
    """A 1080 x 1920 rendering of the perspective warp (h6 scaled to the width) and a start 1.5 px / 0.2 % off it: the
    refinement ends without a flag."""
    w = known_warps(1920)["perspective"]
    prev, cur = warp_canvas(w, 1080, 1920, seed=7, y0=300, x0=500)
    init = w + np.array([0.002, 0, -1.5, 0, -0.002, 1.0, 0, 0])
    return prev, cur, init, {}, 0


def test_flag_cases_reach_their_flags():
    """Each constructed case reaches exactly its flag; a flagged result is the start itself."""
    import direct
    from oracle import gme_oracle
    for name, (prev, cur, init, kw, want) in flag_cases().items():
        h, flags = direct.refine(gme_oracle.get_pyramids(prev), gme_oracle.get_pyramids(cur), init, **kw)
        assert flags == want, (name, flags, want)
        if flags & ~direct.FLAG_MAX_ITERS:
            assert np.array_equal(h, init), name
        else:
            assert np.all(np.isfinite(h)) and not np.array_equal(h, init), name


@pytest.mark.slow
def test_full_hd_case_converges():
    import direct
    from oracle import gme_oracle
    prev, cur, init, kw, want = full_hd_case()
    h, flags = direct.refine(gme_oracle.get_pyramids(prev), gme_oracle.get_pyramids(cur), init, **kw)
    assert flags == want and corner_error(h, known_warps(1920)["perspective"], 1080, 1920) < 0.05, (flags, h)


def test_affine_start_matches_block_field():
    """At every block centre the warp's displacement is the affine block field's pre-rounding displacement
    (d0 columns, d1 rows at block (i, j), motion.py:139-157)."""
    import direct
    import roadmap
    rng = np.random.default_rng(3)
    for bs in (16, 12, 8):
        for _ in range(5):
            p = rng.normal(size=6) * np.array([4, 0.05, 0.05, 4, 0.05, 0.05])
            h = roadmap.affine_to_projective(p, bs)
            assert h.shape == (8,) and h[6] == 0 and h[7] == 0
            i, j = np.meshgrid(np.arange(30.0), np.arange(45.0), indexing="ij")
            c = (bs - 1) / 2.0
            u, v = j * bs + c, i * bs + c
            up, vp, _ = direct.warp(h, u, v)
            assert np.allclose(u - up, p[0] + p[1] * i + p[2] * j, rtol=0, atol=1e-12)
            assert np.allclose(v - vp, p[3] + p[4] * i + p[5] * j, rtol=0, atol=1e-12)
    # a batch and the 12-wide second-order layout (its first six entries)
    P = rng.normal(size=(4, 12))
    assert np.array_equal(roadmap.affine_to_projective(P), np.stack([roadmap.affine_to_projective(q[:6]) for q in P]))
    assert np.array_equal(roadmap.affine_to_projective(np.zeros(6)), [1, 0, 0, 0, 1, 0, 0, 0])


def test_level_projection_is_exact():
    import direct
    import roadmap
    rng = np.random.default_rng(4)
    h = rng.normal(size=(6, 8))
    assert np.array_equal(roadmap.projective_to_level(h, 2), h)
    for L in range(3):
        q = roadmap.projective_to_level(h, L)
        for _ in range(2 - L):
            q = direct.finer(q)
        assert np.array_equal(q, h)                                   # the round trip is exact
    q = roadmap.projective_to_level(h, 1)
    assert np.array_equal(q[:, [0, 1, 3, 4]], h[:, [0, 1, 3, 4]])
    assert np.array_equal(q[:, [2, 5]], h[:, [2, 5]] / 2) and np.array_equal(q[:, [6, 7]], h[:, [6, 7]] * 2)
    # S H S^-1: level pixel k is full-resolution pixel 2k (level 1)
    hp = np.array([1.01, 0.02, 3.0, -0.01, 0.99, -2.0, 1e-4, -2e-4])
    u, v = np.array([0.0, 13.0, 200.0]), np.array([0.0, 77.0, 150.0])
    uf, vf, _ = direct.warp(hp, 2 * u, 2 * v)
    ul, vl, _ = direct.warp(roadmap.projective_to_level(hp, 1), u, v)
    assert np.allclose(2 * ul, uf, rtol=0, atol=1e-12) and np.allclose(2 * vl, vf, rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape,bs,shift", [((96, 128), 16, (3, -2)), ((96, 128), 16, (-7, 5)), ((48, 64), 16, (0, 0)),
                                            ((72, 96), 12, (20, 11)), ((64, 64), 16, (-64, 1))])
def test_integer_translation_equals_block_compensation(shape, bs, shift):
    """Under h = [1 0 -d0 0 1 -d1 0 0] the dense compensation is the reference's block compensation of the constant field
    (d0, d1), frame borders included (oracle compensate_frame, motion.py:289-321)."""
    import direct
    import synth
    from oracle import gme_oracle
    H, W = shape
    prev, cur = synth.frame(11, 0, H, W), synth.frame(11, 1, H, W)
    d0, d1 = shift
    mf = np.zeros((H // bs, W // bs, 2), np.int32)
    mf[..., 0], mf[..., 1] = d0, d1
    want = gme_oracle.compensate_frame(prev, mf)
    got, sse = direct.compensate(prev, cur, np.array([1, 0, -d0, 0, 1, -d1, 0, 0], np.float64))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert sse == int(((cur.astype(np.int64) - want) ** 2).sum())


@pytest.mark.parametrize("name", sorted(known_warps()))
def test_refine_recovers_known_warps(name):
    """A 160 x 120 crop of the synthetic canvas and its warp: the four corners come back within 0.05 px from the identity."""
    import direct
    from oracle import gme_oracle
    h_true = known_warps()[name]
    prev, cur = warp_canvas(h_true, 120, 160)
    info = {}
    h, flags = direct.refine(gme_oracle.get_pyramids(prev), gme_oracle.get_pyramids(cur), direct.IDENTITY, info=info)
    assert flags & ~direct.FLAG_MAX_ITERS == 0, (flags, info)
    assert corner_error(h, h_true, 120, 160) < 0.05, (h, h_true, info)


def test_refine_flags_and_fallbacks():
    """Unrelated frames and degenerate starts come back flagged with their initial parameters and no NaN."""
    import direct
    import synth
    from oracle import gme_oracle
    prev = warp_canvas(direct.IDENTITY, 120, 160)[0]
    noise = (synth.hash64(99, np.arange(120 * 160, dtype=np.uint64)) & np.uint64(0xFF)).astype(np.uint8).reshape(120, 160)
    pp, cp = gme_oracle.get_pyramids(prev), gme_oracle.get_pyramids(noise)
    h, flags = direct.refine(pp, cp, direct.IDENTITY)
    assert np.all(np.isfinite(h)) and (flags != 0 or np.array_equal(h, direct.IDENTITY))
    far = np.array([1, 0, 5000.0, 0, 1, 0, 0, 0])                   # every sample point outside: fewer than 1/4 valid
    h, flags = direct.refine(pp, pp, far)
    assert flags == direct.FLAG_FEW_VALID and np.array_equal(h, far)
    flip = np.array([1, 0, 0, 0, 1, 0, -0.05, 0])                    # d <= 0 inside the frame
    h, flags = direct.refine(pp, pp, flip)
    assert flags == direct.FLAG_DENOMINATOR and np.array_equal(h, flip)


def test_elimination_matches_lapack():
    import direct
    rng = np.random.default_rng(8)
    J = rng.normal(size=(500, 8)) * np.array([300, 200, 1, 300, 200, 1, 1e5, 5e4])
    e = rng.normal(size=500)
    N = J.T @ J
    s = np.concatenate([N[np.triu_indices(8)], J.T @ e])
    delta, ok = direct.solve(s)
    assert ok and np.allclose(delta, np.linalg.solve(N, J.T @ e), rtol=1e-8, atol=0)
    assert not direct.solve(np.zeros(44))[1]
    s1 = np.concatenate([np.outer(J[0], J[0])[np.triu_indices(8)], J[0] * e[0]])          # rank 1
    assert not direct.solve(s1)[1]


def test_threshold_and_cost_definition():
    import direct
    e = np.array([0.0, 0.01, 0.5, 1.0, 1.0625, 3.0, 100.0, 300.0])
    t = direct.threshold(e, 0.25)                     # ceil(0.75 * 8) = 6 values at or below the 6th smallest
    assert t == (np.floor(3.0 * 16) + 1) / 16
    assert direct.threshold(np.zeros(0), 0.1) == 0.0
    assert direct.cost_of(10, 7, 2.0, 0.5) == (2.0 + 3 * 0.25) / 10


def test_surface_keeps_the_indirect_models():
    """The projective estimator is separate: roadmap.MODELS and the rejection of model="projective" stay as they are; the
    CLI has a projective subcommand."""
    import gme_cli
    import roadmap
    assert "projective" not in roadmap.MODELS and len(roadmap.MODELS) == 6
    with pytest.raises(ValueError):
        roadmap.solve_model(np.zeros((1, 15)), "projective")
    a = gme_cli._parser().parse_args(["projective", "-p", "clip", "-fi", "3"])
    assert (a.command, a.path, a.fi, a.fd, a.outlier_fraction, a.max_iters) == ("projective", "clip", 3, 1, 0.1, 10)
    import sequence
    assert hasattr(sequence.ShardedSequence, "estimate_projective")


def test_direct_kernels_do_not_spill():
    """The compiler's resource remarks (build/*.remarks) for every kernel of gme_direct.hip: no VGPR spill, no scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "gme_direct.hip"]
    assert {r["name"] for r in rows} == {"k_direct_hist", "k_direct_sums", "k_direct_state", "k_compensate_proj"}, rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
