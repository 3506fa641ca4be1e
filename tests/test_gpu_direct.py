"""Direct projective refinement on the device (k_direct_hist / k_direct_sums / k_direct_state / k_compensate_proj of
gme_direct.hip through gme_seq_direct_eval, gme_seq_refine_projective and gme_seq_compensate_projective) against the host
definition direct.py: compensation bit for bit, one evaluation, recovery of known warps, parity of the whole refinement,
determinism, real frames, the sharded surface and the CLI.  Needs an MI355X."""
import numpy as np
import pytest

from helpers import check_eval, check_refine
from test_direct_host import corner_error, flag_cases, full_hd_case, known_warps, warp_canvas

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
    """Threshold, n_valid and n_in bit-equal; cost and sums within the documented tolerance (check_eval)."""
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
                    check_eval(got, p, want, (level, p))
        seq.close()


DIRECT_TILE = 256 * 32                 # gme_direct.hip: pixels per hist / sums workgroup
# odd and ragged sizes (odd level widths from (n + 1) / 2; level 0 of 37 x 53 is 10 x 14), full-resolution levels of
# 2 DIRECT_TILE + 1 and 2 DIRECT_TILE - 1 pixels, and full HD (254 tiles per pass)
EDGE_SHAPES = [(37, 53), (101, 203), (479, 719), (113, 145), (127, 129), (1080, 1920)]


def edge_frames(H, W, n):
    import synth
    return synth.sequence(2024, 1, n, H, W)


def test_edge_shapes_reach_their_geometry():
    assert 113 * 145 == 2 * DIRECT_TILE + 1 and 127 * 129 == 2 * DIRECT_TILE - 1
    assert (37 + 3) // 4 * ((53 + 3) // 4) < 200                          # level 0 of 37 x 53: 10 x 14 pixels
    assert all(W % 2 for _, W in EDGE_SHAPES[:3])
    assert -(-1080 * 1920 // DIRECT_TILE) == 254


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_eval_edge_shapes(native, shape):
    """direct_eval against direct.evaluate on every level of the edge shapes, fractions 0.0, 0.1 and 0.5."""
    import direct
    H, W = shape
    frames = edge_frames(H, W, 3)
    seq = sequence_of(native, frames)
    for level in range(3):
        h_l, w_l = seq.level_shape(level)
        h = random_warps(np.random.default_rng(level + W), 2, h_l, w_l)
        h[1, [2, 5]] = [0.3 * w_l, -0.2 * h_l]                           # part of the frame pushed out
        prev = None
        for f in (0.0, 0.1, 0.5):
            got = seq.direct_eval(1, level, h, f)
            prev = prev or [seq.read_frame(p, level) for p in range(3)]          # the pyramid exists after the first call
            for p in range(2):
                want = direct.evaluate(prev[p], prev[p + 1], h[p], f)
                assert want["n_valid"] > 0
                check_eval(got, p, want, (shape, level, f, p))
    seq.close()


def edge_compensation_warps(H, W):
    """name -> warp: near-identity, part of the frame pushed out (the previous pixel is kept there), a horizon crossing the
    frame (d <= 0 on its right part)."""
    return {"near": random_warps(np.random.default_rng(W), 1, H, W)[0],
            "pushed_out": np.array([1.01, 0.02, 0.4 * W, -0.01, 0.99, -0.3 * H, 0, 0]),
            "horizon": np.array([1, 0.05, 1.5, 0.02, 1, -2.0, -1.6 / W, 0.2 / H])}


@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_compensation_edge_shapes(native, shape):
    """compensate_projective against direct.compensate bit for bit, frames and SSE, on the edge shapes."""
    import direct
    H, W = shape
    warps = edge_compensation_warps(H, W)
    names = sorted(warps)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        d = direct.warp(warps["horizon"], u, v)[2]
    assert np.any(d <= 0.0) and np.any(d > 0.0), shape                     # the horizon crosses the frame
    _, valid = direct.residual(np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8), warps["pushed_out"])[:2]
    assert 0 < valid.sum() < H * W, shape
    frames = edge_frames(H, W, len(names) + 1)
    seq = sequence_of(native, frames)
    h = np.stack([warps[n] for n in names])
    sse = seq.compensate_projective(1, h)
    comp = seq.read_compensated_range(0, len(names))
    for p, n in enumerate(names):
        want, want_sse = direct.compensate(frames[p], frames[p + 1], h[p])
        assert np.array_equal(comp[p], want), (shape, n)
        assert sse[p] == want_sse, (shape, n)
    seq.close()


def refine_parity(native, cases):
    """Device refinement against direct.refine on the device's own pyramids for cases name -> (prev, cur, init, kwargs,
    flags): the host reaches the case's flag, the flags are identical, the corners within 0.01 px, a flagged start comes
    back unchanged.  One sequence of pairs (2k, 2k + 1); one call per distinct set of keyword arguments."""
    import direct
    names = sorted(cases)
    frames = np.stack([f for n in names for f in cases[n][:2]])
    H, W = frames.shape[1:]
    seq = sequence_of(native, frames)
    init = np.tile(direct.IDENTITY, (len(frames) - 1, 1))
    for k, n in enumerate(names):
        init[2 * k] = cases[n][2]
    groups = {}
    for k, n in enumerate(names):
        groups.setdefault(tuple(sorted(cases[n][3].items())), []).append(k)
    for kw, ks in groups.items():
        h, flags = seq.refine_projective(1, init, **dict(kw))
        for k in ks:
            n = names[k]
            want, want_flags = direct.refine(pyramids(seq, 2 * k), pyramids(seq, 2 * k + 1), init[2 * k], **dict(kw))
            assert want_flags == cases[n][4], (n, want_flags)
            check_refine(h[2 * k], flags[2 * k], want, want_flags, init[2 * k], H, W, n)
    seq.close()


def test_refine_flag_paths(native):
    """Every outcome of the state machine on an odd-sized pair (test_direct_host.flag_cases): FLAG_SINGULAR, FLAG_DENOMINATOR,
    FLAG_FEW_VALID, FLAG_MAX_ITERS at max_iters 1 and 2, FLAG_NO_GAIN and no flag at fractions 0.0, 0.1 and 0.5."""
    refine_parity(native, flag_cases())


def test_refine_full_hd(native):
    """One 1080 x 1920 pair (254 slabs per pass through k_direct_state's ordered reduction) ends without a flag, as on the
    host, and recovers the rendered warp."""
    refine_parity(native, {"full_hd": full_hd_case()})


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
