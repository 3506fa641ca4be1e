"""Direct projective refinement on the device (k_direct_hist / k_direct_sums / k_direct_state / k_compensate_proj of
gme_direct.hip through gme_seq_direct_eval, gme_seq_refine_projective and gme_seq_compensate_projective) against the host
definition direct.py: compensation bit for bit, one evaluation, recovery of known warps, parity of the whole refinement,
determinism, real frames, the sharded surface and the CLI.  Needs an MI355X."""
import numpy as np
import pytest

from test_direct_host import corner_error, known_warps, warp_canvas

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sequence_of(native, frames):
    return native.Sequence.from_frames(native.default_context(), np.ascontiguousarray(frames, dtype=np.uint8))


def pyramids(seq, index):
    return [seq.read_frame(index, level=l) for l in range(3)]


def random_warps(rng, n, H, W):
    """Valid warps near the identity: a few pixels of shift, ~1 % zoom / shear, a perspective term of up to ~1 px."""
    h = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64), (n, 1))
    h[:, [0, 1, 3, 4]] += rng.normal(scale=0.01, size=(n, 4))
    h[:, [2, 5]] += rng.normal(scale=3.0, size=(n, 2))
    h[:, 6] += rng.normal(scale=1.0 / (W * W), size=n) * 2
    h[:, 7] += rng.normal(scale=1.0 / (H * H), size=n) * 2
    return h


@pytest.fixture(scope="module")
def g9(golden):
    return np.ascontiguousarray(golden("g9_pan240seq")["frames"])


@pytest.mark.parametrize("source", ["g9", "synth720"])
def test_compensation_equals_host(native, g9, source):
    import direct
    import synth
    frames = g9[:9] if source == "g9" else synth.sequence(1234, 3, 5, 480, 720)
    seq = sequence_of(native, frames)
    P, (H, W) = len(frames) - 1, frames.shape[1:]
    h = random_warps(np.random.default_rng(17), P, H, W)
    h[0] = [1, 0, 0, 0, 1, 0, 0, 0]
    h[1] = [1, 0, -3, 0, 1, 2, 0, 0]
    sse = seq.compensate_projective(1, h)
    comp = seq.read_compensated_range(0, P)
    for p in range(P):
        want, want_sse = direct.compensate(frames[p], frames[p + 1], h[p])
        assert np.array_equal(comp[p], want), (source, p)
        assert sse[p] == want_sse, (source, p)
    seq.close()


def test_eval_equals_host(native, g9):
    """Threshold, n_valid and n_in bit-equal; cost and sums within the documented tolerance (1e-9 of the sums of
    absolute values, bounded by Cauchy-Schwarz from the diagonal)."""
    import direct
    import synth
    for frames in (g9[20:25], synth.sequence(77, 0, 3, 480, 720)):
        seq = sequence_of(native, frames)
        P = len(frames) - 1
        for level in range(3):
            H, W = seq.level_shape(level)
            h = random_warps(np.random.default_rng(level), P, H, W)
            for f in (0.1, 0.3):
                got = seq.direct_eval(1, level, h, f)
                for p in range(P):
                    prev, cur = seq.read_frame(p, level), seq.read_frame(p + 1, level)
                    want = direct.evaluate(prev, cur, h[p], f)
                    assert got["threshold"][p] == want["threshold"]
                    assert tuple(got["counts"][p]) == (want["n_valid"], want["n_in"])
                    assert abs(got["cost"][p] - want["cost"]) <= 1e-9 * want["cost"]
                    N, rhs = direct.normal_matrix(want["sums"])
                    d = np.sqrt(np.diag(N))
                    se2 = want["cost"] * want["n_valid"]               # >= sum of e^2 over the inliers
                    scale = np.concatenate([np.outer(d, d)[np.triu_indices(8)], d * np.sqrt(se2)])
                    assert np.all(np.abs(got["sums"][p] - want["sums"]) <= 1e-9 * scale), (level, p)
        seq.close()


def test_recovers_known_warps_full_size(native):
    warps = known_warps(720)
    names = sorted(warps)
    pairs = [warp_canvas(warps[n], 480, 720, seed=5, y0=600, x0=1000) for n in names]
    frames = np.stack([f for pair in pairs for f in pair])
    seq = sequence_of(native, frames)
    init = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64), (len(frames) - 1, 1))
    h, flags = seq.refine_projective(1, init)
    for k, n in enumerate(names):
        assert flags[2 * k] == 0, (n, flags[2 * k])
        assert corner_error(h[2 * k], warps[n], 480, 720) < 0.05, (n, h[2 * k])
    seq.close()


def test_real_frames_parity_cost_and_psnr(native, g9):
    """g9 (the reference's own clip), fd 1, from the indirect affine estimate: the device refinement against direct.refine
    (corners within 0.01 px, identical flags) on a subset, and on every pair a full-resolution cost no worse than the
    start's and a median PSNR gain of the projective over the block-affine compensation above 0 dB."""
    import direct
    import motion
    import roadmap
    import sequence
    seq = sequence_of(native, g9)
    P, (H, W) = len(g9) - 1, g9.shape[1:]
    affine = motion.estimate_sequence(seq, 1)
    init = roadmap.affine_to_projective(affine, 16)
    h, flags = seq.refine_projective(1, init)
    assert np.all(np.isfinite(h))
    sse_affine = seq.compensate(1, 16, affine)
    sse_proj = seq.compensate_projective(1, h)
    gain = sequence.psnr_from_sse(sse_proj, H, W) - sequence.psnr_from_sse(sse_affine, H, W)
    print("g9 fd1: median PSNR gain %.3f dB (min %.3f, max %.3f), flags %s" % (np.median(gain), gain.min(), gain.max(),
                                                                           np.bincount(flags, minlength=32).nonzero()[0].tolist()))
    assert np.median(gain) > 0
    for p in range(P):
        pp, cp = pyramids(seq, p), pyramids(seq, p + 1)
        info = {}
        want, want_flags = direct.refine(pp, cp, init[p], info=info)
        assert flags[p] == want_flags, (p, flags[p], want_flags)
        assert corner_error(h[p], want, H, W) < 0.01, (p, h[p], want)
        if flags[p] & (direct.FLAG_SINGULAR | direct.FLAG_FEW_VALID | direct.FLAG_DENOMINATOR | direct.FLAG_NO_GAIN):
            assert np.array_equal(h[p], init[p])
            continue
        # the full-resolution objective of the result under the level-2 threshold is no worse than the start's
        t = info["t"]
        assert direct.full_cost(pp[2], cp[2], h[p], t) <= direct.full_cost(pp[2], cp[2], init[p], t) * (1 + 1e-12), p
    seq.close()


def test_determinism_batch_and_grid_chunks(native, monkeypatch):
    import synth
    frames = synth.sequence(4321, 0, 65, 480, 720)
    seq = sequence_of(native, frames)
    init = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64), (64, 1))
    init[:, 2] += np.linspace(-6, 6, 64)                               # synth pans (-5, +3) per frame
    a, fa = seq.refine_projective(1, init)
    b, fb = seq.refine_projective(1, init)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(fa, fb)
    monkeypatch.setenv("GME_MAX_GRID_PAIRS", "7")
    c, fc = seq.refine_projective(1, init)
    assert np.array_equal(bits(a), bits(c)) and np.array_equal(fa, fc)
    monkeypatch.delenv("GME_MAX_GRID_PAIRS")
    seq.close()
    one = native.Sequence(native.default_context(), 2, 480, 720)
    for p in range(64):
        one.upload(0, frames[p:p + 2])
        h, f = one.refine_projective(1, init[p:p + 1])
        assert np.array_equal(bits(h[0]), bits(a[p])) and f[0] == fa[p], p
    one.close()


def test_unrelated_frames_fall_back(native):
    import direct
    import synth
    prev = synth.frame(5, 0, 480, 720)
    noise = (synth.hash64(99, np.arange(480 * 720, dtype=np.uint64)) & np.uint64(0xFF)).astype(np.uint8).reshape(480, 720)
    seq = sequence_of(native, np.stack([prev, noise, prev]))
    init = np.array([[1, 0, 0, 0, 1, 0, 0, 0], [1, 0, 5000.0, 0, 1, 0, 0, 0]], np.float64)
    h, flags = seq.refine_projective(1, init)
    assert np.all(np.isfinite(h))
    assert flags[0] != 0 or np.array_equal(h[0], init[0]), (h[0], flags[0])
    assert flags[1] == direct.FLAG_FEW_VALID and np.array_equal(h[1], init[1])
    seq.close()


def test_sharded_estimate_projective_lanes(native):
    import synth
    from sequence import ShardedSequence
    frames = synth.sequence(99, 0, 9, 480, 720)
    out = []
    for streams in (1, 2):
        sh = ShardedSequence(480, 720, len(frames), 1, streams=streams)
        sh.load(frames)
        h, flags, psnr = sh.estimate_projective()
        assert h.shape == (8, 8) and flags.shape == (8,) and psnr.shape == (8,)
        assert np.array_equal(sh.gather(h), h)                           # world 1: the rows as they are
        out.append((h, flags, psnr))
        sh.close()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0]))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_cli_projective(native, g9, tmp_path, capsys):
    import gme_cli
    from PIL import Image
    d = tmp_path / "clip"
    d.mkdir()
    for i in range(3):
        Image.fromarray(g9[10 + i]).save(d / ("f%d.png" % i))
    res = gme_cli.main(["projective", "-p", str(d), "-fi", "2"])
    out = capsys.readouterr().out
    assert "psnr block-affine" in out and "psnr projective" in out and "flags" in out
    assert res["h"].shape == (8,) and np.all(np.isfinite(res["h"]))
