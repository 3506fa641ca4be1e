"""Video stabilization on the device (k_warp_frames / k_frame_sse of gme_stab.hip through gme_seq_warp_frames,
gme_seq_read_warped_range and gme_seq_frame_sse) against the host definition stabilize.py: the warp bit for bit, the
squared errors, a known jittered camera path, real frames through the sharded surface, the error paths and the CLI.
Needs an MI355X."""
import json

import numpy as np
import pytest

from test_direct_host import corner_error, warp_canvas
from test_stabilize_host import camera_path, pair_warps, second_difference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


@pytest.fixture(scope="module")
def g9(golden):
    return np.ascontiguousarray(golden("g9_pan240seq")["frames"])


def sequence_of(native, frames):
    return native.Sequence.from_frames(native.default_context(), np.ascontiguousarray(frames, dtype=np.uint8))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def random_warps(rng, n, H, W, far=False):
    """Near-identity warps (a few pixels of shift, ~1 % zoom / shear, a little perspective); ``far`` shifts by up to half
    the frame, so that half of the output samples outside it."""
    h = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64), (n, 1))
    h[:, [0, 1, 3, 4]] += rng.normal(scale=0.01, size=(n, 4))
    h[:, 2] += rng.normal(scale=3.0, size=n) + (rng.uniform(-0.5, 0.5, size=n) * W if far else 0)
    h[:, 5] += rng.normal(scale=3.0, size=n) + (rng.uniform(-0.5, 0.5, size=n) * H if far else 0)
    h[:, 6] += rng.normal(scale=1.0 / (W * W), size=n) * 2
    h[:, 7] += rng.normal(scale=1.0 / (H * H), size=n) * 2
    return h


@pytest.mark.parametrize("shape,n", [((37, 53), 6), ((480, 720), 4), ((1080, 1918), 2)])
def test_warp_equals_host(native, shape, n):
    import stabilize
    import synth
    rng = np.random.default_rng(shape[1])
    H, W = shape
    frames = synth.sequence(99, 0, n, H, W) if H > 100 else rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
    seq = sequence_of(native, frames)
    warps = np.concatenate([random_warps(rng, n - n // 2, H, W), random_warps(rng, n // 2, H, W, far=True)])
    for border, fill in (("constant", 0), ("constant", 201), ("replicate", 0)):
        valid = seq.warp_frames(0, warps, stabilize.border_id(border), fill)
        want, want_valid = stabilize.warp_frames(frames, warps, border, fill)
        assert np.array_equal(seq.read_warped_range(0, n), want), (shape, border, fill)
        assert np.array_equal(valid, want_valid)
    # a sub-range: only frames first .. first+count-1 are rewritten
    first, count = 1, n - 1 if n > 2 else 1
    valid = seq.warp_frames(first, warps[:count], 0, 7)
    want, want_valid = stabilize.warp_frames(frames[first:first + count], warps[:count], "constant", 7)
    assert np.array_equal(seq.read_warped_range(first, count), want) and np.array_equal(valid, want_valid)
    seq.close()


def degenerate_warps(H, W):
    """name -> (warp, branch) for the warps random_warps never makes.  branch names what the warp must reach on an H x W
    frame: "edge" a valid sample point exactly on u' = W-1 or v' = H-1 (the far tap clamped), "horizon" pixels with d <= 0,
    "behind" valid samples where d < 0, "d0" d == 0 exactly on a row, "nonfinite" non-finite coordinates."""
    nan, inf = float("nan"), float("inf")
    return {
        "shift_small": ([1, 0, 3, 0, 1, -2, 0, 0], "edge"),
        "shift_half": ([1, 0, -(W // 2), 0, 1, H // 3, 0, 0], "edge"),
        "shift_to_last_column": ([1, 0, W - 1, 0, 1, 0, 0, 0], "edge"),            # only u = 0 samples, on u' = W-1
        "mirror_horizontal": ([-1, 0, W - 1, 0, 1, 0, 0, 0], "edge"),
        "mirror_vertical": ([1, 0, 0, 0, -1, H - 1, 0, 0], "edge"),
        "horizon_behind": ([1, 0, -W, 0, 1, -H, -2.0 / W, 0], "behind"),         # d < 0 past u = W/2, and u', v' land inside
        "horizon_tilted": ([1, 0.1, 2.0, -0.05, 1, 1.0, -2.5 / W, 0.3 / H], "horizon"),
        "d_zero_row": ([1, 0, 0, 0, 1, 0, 0, -1.0 / 32], "d0"),                     # d = 1 - v / 32: exactly 0 on row 32
        "nan_shift": ([1, 0, nan, 0, 1, 0, 0, 0], "nonfinite"),
        "inf_shift": ([1, 0, 0, 0, 1, inf, 0, 0], "nonfinite"),
        "minus_inf_perspective": ([1, 0, 0, 0, 1, 0, -inf, 0], "nonfinite"),        # u' = -0.0, v' = -0.0 for u > 0
    }


def reaches(h, branch, H, W):
    import direct
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        up, vp, d = direct.warp(np.asarray(h, np.float64), u.ravel(), v.ravel())
        ins = (up >= 0.0) & (up <= W - 1.0) & (vp >= 0.0) & (vp <= H - 1.0)
    if branch == "edge":
        return bool(np.any(ins & ((up == W - 1.0) | (vp == H - 1.0))))
    if branch == "horizon":
        return bool(np.any(d <= 0.0))
    if branch == "behind":
        return bool(np.any(ins & (d < 0.0)))
    if branch == "d0":
        return bool(np.any(d == 0.0))
    return not bool(np.all(np.isfinite(up)) and np.all(np.isfinite(vp)))


@pytest.mark.parametrize("shape", [(41, 53), (96, 131), (540, 1918)])
def test_degenerate_warps_equal_host(native, shape):
    """Integer shifts onto the last column / row, mirror flips, horizons crossing the frame, d == 0 on a row, NaN and +-inf
    parameters: warped frames and valid counts bit for bit with stabilize.warp_frames in the three
    border / fill modes, and frame_sse of the warped planes (width not a multiple of 64: the padding must stay zero)
    equal to the int64 squared errors of the host frames."""
    import stabilize
    import synth
    H, W = shape
    warps = degenerate_warps(H, W)
    names = sorted(warps)
    for n in names:
        assert reaches(warps[n][0], warps[n][1], H, W), (shape, n)
    h = np.array([warps[n][0] for n in names], np.float64)
    N = len(names)
    frames = synth.sequence(77, 0, N, H, W) if H > 64 else np.random.default_rng(W).integers(0, 256, (N, H, W), dtype=np.uint8)
    seq = sequence_of(native, frames)
    for border, fill in (("constant", 0), ("constant", 201), ("replicate", 0)):
        valid = seq.warp_frames(0, h, stabilize.border_id(border), fill)
        want, want_valid = stabilize.warp_frames(frames, h, border, fill)
        got = seq.read_warped_range(0, N)
        for k, n in enumerate(names):
            assert np.array_equal(got[k], want[k]), (shape, border, fill, n)
            assert valid[k] == want_valid[k], (shape, border, fill, n, valid[k], want_valid[k])
        w = want.astype(np.int64)
        assert np.array_equal(seq.frame_sse(1, 0, N - 1), ((w[1:] - w[:-1]) ** 2).sum(axis=(1, 2))), (shape, border, fill)
    seq.close()


def test_grid_chunks_give_the_same_bytes(native, monkeypatch):
    import stabilize
    import synth
    rng = np.random.default_rng(8)
    frames = synth.sequence(5, 0, 7, 96, 131)
    warps = random_warps(rng, 7, 96, 131, far=True)
    seq = sequence_of(native, frames)
    valid = seq.warp_frames(0, warps, 1, 0)
    whole, sse = seq.read_warped_range(0, 7), seq.frame_sse(1, 0, 6)
    monkeypatch.setenv("GME_MAX_GRID_PAIRS", "2")
    assert np.array_equal(seq.warp_frames(0, warps, 1, 0), valid)
    assert np.array_equal(seq.read_warped_range(0, 7), whole)
    assert np.array_equal(seq.frame_sse(1, 0, 6), sse)
    d = frames[1:].astype(np.int64) - frames[:-1].astype(np.int64)
    assert np.array_equal(seq.frame_sse(0, 0, 6), (d * d).sum(axis=(1, 2)))
    assert np.array_equal(whole, stabilize.warp_frames(frames, warps, "replicate")[0])
    seq.close()


def test_identity_and_frame_sse(native, g9):
    import direct
    import stabilize
    frames = g9[:12]
    seq = sequence_of(native, frames)
    valid = seq.warp_frames(0, np.tile(direct.IDENTITY, (12, 1)))
    assert np.array_equal(seq.read_warped_range(0, 12), frames) and np.all(valid == 240 * 320)
    d = frames[1:].astype(np.int64) - frames[:-1].astype(np.int64)
    want = (d * d).sum(axis=(1, 2))
    assert np.array_equal(seq.frame_sse(0, 0, 11), want) and np.array_equal(seq.frame_sse(1, 0, 11), want)
    assert np.array_equal(seq.frame_sse(0, 3, 4), want[3:7])
    rng = np.random.default_rng(4)
    warps = random_warps(rng, 12, 240, 320, far=True)
    seq.warp_frames(0, warps, 0, 50)
    w = stabilize.warp_frames(frames, warps, "constant", 50)[0].astype(np.int64)
    assert np.array_equal(seq.frame_sse(1, 0, 11), ((w[1:] - w[:-1]) ** 2).sum(axis=(1, 2)))
    seq.close()
    out, res = stabilize.stabilize(frames, radius=0, crop=0.0)
    assert np.array_equal(out, frames) and res["crop"] == 0.0 and np.array_equal(res["W"], np.tile(direct.IDENTITY, (12, 1)))


def test_known_jitter(native):
    """A jittered pan (camera_path: translation sigma 2 px, rotation 0.2 deg, zoom 0.3 %) rendered on synth.canvas, 320x240,
    48 frames, projective estimator.  Bounds: the estimated C_t within 1 px (corner error) of G_0^-1 G_t for every t; the
    stabilized true path at most 0.3x the input's RMS second difference; ITF up; every output pixel valid under the auto
    crop.  First measured on the MI355X: max corner error 0.470 px, second-difference ratio 0.069, auto crop 0.036,
    ITF 23.05 -> 28.05 dB, pair flags 0 and 16 (max_iters reached, informational); both bounds kept as set."""
    import stabilize
    H, W, n = 240, 320, 48
    G = camera_path(n, H, W)
    frames = np.stack([warp_canvas(stabilize.params(G[t]), H, W)[1] for t in range(n)])
    out, res = stabilize.stabilize(frames)
    true_C = stabilize.trajectory(pair_warps(G))
    err = max(corner_error(stabilize.params(res["C"][t]), stabilize.params(true_C[t]), H, W) for t in range(n))
    ratio = second_difference(G, res["W"], H, W) / second_difference(G, None, H, W)
    print("known jitter: max corner error %.4f px, second-difference ratio %.4f, crop %.4f, itf %.3f -> %.3f dB, pair flags %s"
          % (err, ratio, res["crop"], res["itf_before"], res["itf_after"], np.unique(res["pair_flags"])))
    assert err <= 1.0
    assert ratio <= 0.3
    assert res["itf_after"] > res["itf_before"]
    assert res["crop"] < 0.25 and np.all(res["valid"] == H * W) and not np.any(res["flags"])
    assert out.shape == frames.shape


def test_real_frames_sharded(native, g9):
    """g9 (51 frames of the pan240 clip): streams 1 and 3 give the same stabilized bytes and W, and so does a second run;
    the affine estimator runs."""
    import sequence
    runs = []
    for streams in (1, 3, 1):
        sh = sequence.ShardedSequence(240, 320, len(g9), 1, streams=streams)
        sh.load(g9)
        res = sh.stabilize()
        frames = np.stack([sh.read_stabilized(t) for t in range(len(g9))])
        assert np.array_equal(sh.read_stabilized_range(0, len(g9)), frames)
        runs.append((frames, res))
        sh.close()
    for frames, res in runs[1:]:
        assert np.array_equal(frames, runs[0][0])
        assert np.array_equal(bits(res["W"]), bits(runs[0][1]["W"])) and np.array_equal(res["valid"], runs[0][1]["valid"])
        assert res["itf_after"] == runs[0][1]["itf_after"]
    import stabilize
    out, res = stabilize.stabilize(g9, estimator="affine")
    print("g9: projective crop %.4f itf %.3f -> %.3f dB, flags %s; affine crop %.4f itf -> %.3f dB, flags %s"
          % (runs[0][1]["crop"], runs[0][1]["itf_before"], runs[0][1]["itf_after"], np.unique(runs[0][1]["flags"]),
             res["crop"], res["itf_after"], np.unique(res["flags"])))
    assert out.shape == g9.shape and res["flags"].shape == (51,) and res["pair_flags"].shape == (50,)
    assert np.all(np.isfinite(res["W"]))


def test_error_paths(native, g9):
    import sequence
    seq = sequence_of(native, g9[:4])
    with pytest.raises(IndexError, match="never warped"):
        seq.read_warped_range(0, 1)
    with pytest.raises(IndexError, match="never warped"):
        seq.frame_sse(1, 0, 2)
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64), (2, 1))
    with pytest.raises(IndexError, match="outside"):
        seq.warp_frames(3, ident)
    with pytest.raises(IndexError, match="outside"):
        seq.warp_frames(-1, ident)
    with pytest.raises(IndexError, match="border"):
        seq.warp_frames(0, ident, 2, 0)
    with pytest.raises(IndexError, match="fill"):
        seq.warp_frames(0, ident, 0, 256)
    with pytest.raises(IndexError, match="outside"):
        seq.frame_sse(0, 2, 2)
    seq.warp_frames(0, ident)
    with pytest.raises(IndexError, match="never warped"):
        seq.read_warped_range(1, 2)
    assert seq.read_warped_range(0, 2).shape == (2, 240, 320)
    seq.close()
    sh = sequence.ShardedSequence(240, 320, 6, 2)
    with pytest.raises(ValueError, match="frame_distance"):
        sh.stabilize()
    sh.close()


def test_cli_stabilize(native, g9, tmp_path, capsys):
    import gme_cli
    import stabilize
    np.save(tmp_path / "clip.npy", g9)
    res = gme_cli.main(["stabilize", "-p", str(tmp_path / "clip.npy"), "-o", str(tmp_path / "out")])
    assert "itf before" in capsys.readouterr().out
    pngs = sorted((tmp_path / "out" / "stabilized").glob("*.png"))
    assert len(pngs) == 51 and pngs[0].name == "0000.png"
    rec = json.loads((tmp_path / "out" / "stabilize.json").read_text())
    _, api = stabilize.stabilize(g9)
    assert rec["itf_before"] == api["itf_before"] and rec["itf_after"] == api["itf_after"] == res["itf_after"]
    assert rec["frames"] == 51 and len(rec["W"]) == 51 and len(rec["pair_flags"]) == 50
