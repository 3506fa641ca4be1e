"""Video stabilization, host side (stabilize.py): the camera path and its smoothing, the corrections and the
auto crop, the host definition of the device warp, the CLI, the lanes' frame ownership and the new kernels' resource
remarks.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def camera_path(n, H, W, seed=11, pan=(1.5, 0.5), shift_sigma=2.0, rot_sigma_deg=0.2, zoom_sigma=0.003):
    """G float64[n, 3, 3]: frame-t pixels -> canvas coordinates, a constant-velocity pan plus seeded jitter (translation,
    rotation and zoom about the frame centre)."""
    rng = np.random.default_rng(seed)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    G = np.empty((n, 3, 3))
    for t in range(n):
        th = np.deg2rad(rng.normal(scale=rot_sigma_deg))
        z = 1.0 + rng.normal(scale=zoom_sigma)
        tx, ty = pan[0] * t + rng.normal(scale=shift_sigma), pan[1] * t + rng.normal(scale=shift_sigma)
        R = np.array([[z * np.cos(th), -z * np.sin(th), 0], [z * np.sin(th), z * np.cos(th), 0], [0, 0, 1.0]])
        Tc = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
        G[t] = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]]) @ Tc @ R @ np.linalg.inv(Tc)
    return G


def pair_warps(G):
    """The true pair warps G_{t-1}^-1 G_t as float64[n-1, 8]."""
    import stabilize
    return np.stack([stabilize.params(np.linalg.solve(G[t - 1], G[t])) for t in range(1, len(G))])


def second_difference(G, Wt, H, W):
    """RMS second difference over t of the output corners in canvas coordinates (G_t W_t applied to the frame corners)."""
    import stabilize
    u = np.array([0.0, W - 1.0, 0.0, W - 1.0])
    v = np.array([0.0, 0.0, H - 1.0, H - 1.0])
    pts = []
    for t in range(len(G)):
        m = G[t] if Wt is None else G[t] @ stabilize.matrix(Wt[t])
        q = m @ np.stack([u, v, np.ones(4)])
        pts.append(np.concatenate([q[0] / q[2], q[1] / q[2]]))
    pts = np.array(pts)
    d2 = pts[2:] - 2 * pts[1:-1] + pts[:-2]
    return float(np.sqrt(np.mean(d2 * d2)))


def test_trajectory_chains_pair_warps():
    import direct
    import stabilize
    rng = np.random.default_rng(1)
    h = np.tile(direct.IDENTITY, (12, 1)) + rng.normal(scale=[1e-3, 1e-3, 1.0, 1e-3, 1e-3, 1.0, 1e-6, 1e-6], size=(12, 8))
    C = stabilize.trajectory(h)
    assert C.shape == (13, 3, 3) and np.array_equal(C[0], np.eye(3)) and np.allclose(C[:, 2, 2], 1.0, rtol=0, atol=1e-15)
    pts = rng.uniform(0, 300, size=(2, 7))
    for t in range(1, 13):
        u, v = pts
        for p in range(t - 1, -1, -1):                       # frame t -> t-1 -> ... -> 0
            u, v, _ = direct.warp(h[p], u, v)
        q = C[t] @ np.stack([pts[0], pts[1], np.ones(7)])
        assert np.allclose(q[0] / q[2], u, rtol=1e-9) and np.allclose(q[1] / q[2], v, rtol=1e-9)


def test_constant_velocity_pan_is_left_unchanged():
    import stabilize
    H, W = 120, 160
    h = np.tile(np.array([1, 0, -2.5, 0, 1, 0.75, 0, 0], np.float64), (30, 1))
    C = stabilize.trajectory(h)
    S = stabilize.smooth(C, 15)
    assert np.allclose(S, C, rtol=0, atol=1e-9)
    crop = stabilize.auto_crop(C, S, H, W)
    assert 0 < crop < 1e-3
    w, flags = stabilize.corrections(C, S, H, W, crop)
    assert np.allclose(w, stabilize.params(stabilize.zoom(crop, H, W)), rtol=0, atol=1e-9)
    assert not np.any(flags)


def test_radius_zero_is_the_identity():
    import direct
    import stabilize
    rng = np.random.default_rng(2)
    h = np.tile(direct.IDENTITY, (9, 1)) + rng.normal(scale=[1e-3, 1e-3, 2.0, 1e-3, 1e-3, 2.0, 1e-6, 1e-6], size=(9, 8))
    C = stabilize.trajectory(h)
    S = stabilize.smooth(C, 0)
    assert np.array_equal(S, C)
    w, flags = stabilize.corrections(C, S, 90, 120, 0.0)
    assert np.array_equal(w, np.tile(direct.IDENTITY, (10, 1))) and not np.any(flags)
    p = stabilize.plan(h, 90, 120, radius=0, crop=0.0)
    assert p["crop"] == 0.0 and np.array_equal(p["W"], w)


def test_auto_crop():
    import stabilize
    H, W = 120, 160
    G = camera_path(40, H, W)
    C = stabilize.trajectory(pair_warps(G))
    S = stabilize.smooth(C, 10)
    crop = stabilize.auto_crop(C, S, H, W)
    assert 0 < crop < 0.25
    w, flags = stabilize.corrections(C, S, H, W, crop)
    assert all(stabilize.corners_inside(x, H, W) for x in w)
    assert not np.any(flags)
    below, _ = stabilize.corrections(C, S, H, W, crop - 2e-4)
    assert not all(stabilize.corners_inside(x, H, W) for x in below)
    # a cap that binds: returned as is, bit 2 on the frames that keep border pixels
    capped = stabilize.auto_crop(C, S, H, W, max_crop=crop / 4)
    assert capped == crop / 4
    w, flags = stabilize.corrections(C, S, H, W, capped)
    assert np.any(flags & stabilize.FLAG_BORDER) and not np.any(flags & stabilize.FLAG_FALLBACK)
    for x, f in zip(w, flags):
        assert bool(f & stabilize.FLAG_BORDER) == (not stabilize.corners_inside(x, H, W, 0.0))


def test_fallback_flag():
    import stabilize
    C = np.tile(np.eye(3), (3, 1, 1))
    S = C.copy()
    S[1] = [[1, 0, 0], [0, 1, 0], [-0.05, 0, 1]]                # d <= 0 at the right-hand corners of a 160 px frame
    S[2, 0, 0] = np.nan
    w, flags = stabilize.corrections(C, S, 120, 160, 0.1)
    assert list(flags & stabilize.FLAG_FALLBACK) == [0, 1, 1]
    assert np.array_equal(w[1], stabilize.params(stabilize.zoom(0.1, 120, 160)))


def test_smoothing_steadies_a_known_jittered_path():
    """True pair warps of a jittered pan over 48 frames: the RMS second difference of the output corners in canvas
    coordinates drops to at most 0.3x that of the input."""
    import stabilize
    H, W = 240, 320
    G = camera_path(48, H, W)
    p = stabilize.plan(pair_warps(G), H, W)
    assert p["crop"] < 0.25 and not np.any(p["flags"])
    before, after = second_difference(G, None, H, W), second_difference(G, p["W"], H, W)
    assert after <= 0.3 * before, (before, after)


def test_warp_frames_host_definition():
    import direct
    import stabilize
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, size=(3, 37, 53), dtype=np.uint8)
    ident = np.tile(direct.IDENTITY, (3, 1))
    for border in ("constant", "replicate"):
        out, valid = stabilize.warp_frames(f, ident, border)
        assert np.array_equal(out, f) and list(valid) == [37 * 53] * 3
    dx, dy = 3, -2                                              # output (u, v) samples (u + 3, v - 2)
    shift = np.tile(np.array([1, 0, dx, 0, 1, dy, 0, 0], np.float64), (3, 1))
    out, valid = stabilize.warp_frames(f, shift, "constant", fill=17)
    want = np.full_like(f, 17)
    want[:, -dy:, :53 - dx] = f[:, :37 + dy, dx:]
    assert np.array_equal(out, want)
    assert list(valid) == [(37 + dy) * (53 - dx)] * 3
    out, valid = stabilize.warp_frames(f, shift, "replicate")
    rows = np.clip(np.arange(37) + dy, 0, 36)
    cols = np.clip(np.arange(53) + dx, 0, 52)
    assert np.array_equal(out, f[:, rows][:, :, cols])
    assert list(valid) == [(37 + dy) * (53 - dx)] * 3
    with pytest.raises(ValueError):
        stabilize.warp_frames(f, ident, "wrap")
    with pytest.raises(ValueError):
        stabilize.warp_frames(f, ident, "constant", fill=256)


def test_cli_parses_stabilize():
    import gme_cli
    a = gme_cli._parser().parse_args(["stabilize", "-p", "clip", "-o", "out"])
    assert (a.command, a.path, a.outdir, a.estimator, a.radius, a.sigma, a.crop, a.max_crop, a.border, a.fill) == \
        ("stabilize", "clip", "out", "projective", 15, None, "auto", 0.25, "constant", 0)
    a = gme_cli._parser().parse_args(["stabilize", "-p", "c", "-o", "o", "--estimator", "affine", "--crop", "0.1",
                                      "--border", "replicate", "--fill", "9", "--sigma", "2.5", "--radius", "4"])
    assert (a.estimator, a.crop, a.border, a.fill, a.sigma, a.radius) == ("affine", 0.1, "replicate", 9, 2.5, 4)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("streams", [1, 2, 4])
def test_frame_ownership_covers_every_frame_once(world, streams):
    import sequence
    for n in (2, 3, 5, 9, 17, 51):
        owned = []
        for rank in range(world):
            ranges = sequence.stabilized_owners(n, rank, world, streams)
            start, stop = sequence.shard_range(n - 1, rank, world)
            # the ranges of lanes that exist: one per lane the shard builds (sequence.lane_ranges)
            assert len(ranges) == (len(sequence.lane_ranges(stop - start, streams)) if stop > start else 0)
            for a, b in ranges:
                owned.extend(range(a, b))
        assert sorted(owned) == list(range(n)), (n, world, streams)


def test_stab_kernels_do_not_spill():
    """The compiler's resource remarks (build/*.remarks) for the kernels of gme_stab.hip: no VGPR or SGPR spill, no scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "gme_stab.hip"]
    assert {r["name"] for r in rows} == {"k_warp_frames", "k_frame_sse"}, rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
