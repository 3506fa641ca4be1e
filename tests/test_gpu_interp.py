"""Motion-compensated frame interpolation on the device (k_interp and k_interp_frame of bbme_interp.hip through gme_interp_u8
and gme_seq_interp) against the host definition interp.py: byte for byte on noise at the shapes where the kernel takes another
path, the stripes, constant and pan scenes, saturated content, a batched sequence and real frames, plus the error paths and the
CLI.  Needs an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import interp_cases as ic

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mv", "cost", "dist", "frame")


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def instance(bs):
    return "k_interp<%d>" % (bs if bs in (16, 32) else 0)


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4])


def check_pair(native, past, nxt, bs, sw, pnorm, bias, want=None, truth=None):
    """gme_interp_u8 on host buffers against interp.search and interp.interpolate (``want``: their result where a test has it
    already), the squared error against interp.sse where there is a true middle frame, -1 where there is none -> the host's
    result."""
    import interp
    ctx = native.default_context()
    if want is None:
        want = interp.search(past, nxt, bs, sw, pnorm, bias)
        want = want + (interp.interpolate(past, nxt, want[0], bs),)
    got = ctx.interp(past, nxt, bs, sw, pnorm, bias, truth=truth)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    what = ("gme_interp_u8", past.shape, bs, sw, pnorm, bias)
    same(got[:4], want, what)
    assert got[4] == (-1 if truth is None else interp.sse(want[3], truth)), what
    return want


@pytest.mark.parametrize("case", ic.NOISE)
def test_noise(native, case):
    """Noise pairs at the shapes of interp_cases, both norms, without a bias and at the tool's default one, with the middle
    noise frame as the truth."""
    shape, bs, sw = case
    past, mid, nxt = ic.noise_pair(case)
    for pnorm in (0, 1):
        for bias in ic.noise_biases(case, pnorm):
            check_pair(native, past, nxt, bs, sw, pnorm, bias, ic.result(case, pnorm, bias), truth=mid)


@pytest.mark.parametrize("pnorm", (0, 1))
def test_scenes(native, pnorm):
    """The scenes of tests/test_interp_host.py on the device: the stripes (scan order at bias 0, the bias at 1), constant frames
    (every candidate ties with the centre) and the pan."""
    import interp
    past, nxt = ic.stripes()
    for bias in (0, 1):
        mv = check_pair(native, past, nxt, ic.STRIPES_BLOCK, ic.STRIPES_WINDOW, pnorm, bias, ic.result("stripes", pnorm, bias))[0]
        assert np.all(mv[:, 1:5] == ((-7, -8) if bias == 0 else (1, 0)))
    flat = np.full((37, 53), 90, np.uint8), np.full((37, 53), 97, np.uint8)
    for bs, sw in ((8, 4), (16, 8)):
        for bias in (0, 5):
            mv, cost, dist, made = check_pair(native, flat[0], flat[1], bs, sw, pnorm, bias)
            assert not mv.any() and np.array_equal(cost, dist) and np.all(made == 94)
    past, mid, nxt = ic.pan_scene()
    bias = interp.default_bias(ic.PAN_BLOCK, pnorm)
    mv = check_pair(native, past, nxt, ic.PAN_BLOCK, ic.PAN_WINDOW, pnorm, bias, ic.result("pan", pnorm, bias), truth=mid)[0]
    assert np.all(mv == ic.PAN_MOVE)


def test_saturated(native):
    """Blocks of 64 with `past` 0 and `next` 255: D is 64^2 * 255 (MAE) or 64^2 * 255^2 = 266 342 400 (MSE), the largest there
    is, in every block and for every candidate, so the centre stays; the frame is 128 everywhere.  With the largest bias, 2^16,
    the largest J a candidate can have is scored beside it.  Nothing wraps."""
    lo, hi = np.zeros((130, 135), np.uint8), np.full((130, 135), 255, np.uint8)
    for pnorm, top in ((0, 64 * 64 * 255), (1, 64 * 64 * 255 * 255)):
        for bias in (0, 1 << 16):
            for past, nxt in ((lo, hi), (hi, lo)):
                mv, cost, dist, made = check_pair(native, past, nxt, 64, 8, pnorm, bias, truth=lo)
                assert not mv.any() and np.all(cost == top) and np.all(dist == top) and np.all(made == 128)
    # a far candidate at the largest bias: `past` is 255 in its first 60 columns only and `next` 255 everywhere, so the first
    # block column matches at vx = 4 at the price of 4 * 2^16, which the centre's four wrong columns exceed under MSE only
    past = lo.copy()
    past[:, :60] = 255
    assert np.all(check_pair(native, past, hi, 64, 8, 1, 1 << 16)[0][:, 0] == (4, 0))
    assert not check_pair(native, past, hi, 64, 8, 0, 1 << 16)[0][:, 0].any()


def check_sequence(native, frames, fd, bs, sw, pnorm, bias):
    """gme_seq_interp over a resident sequence that holds a motion field, a variable-block-size tree and compensated planes:
    every pair against the host, the squared error against the true middle frame for an even distance and -1 for an odd one,
    and the sequence's other results byte-equal after the call -> the device's five arrays."""
    import interp
    ctx = native.default_context()
    P = len(frames) - fd
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(frames))
    seq.bbme(1, 8, 3, 0, pnorm)
    mv = seq.read_mv()
    seq.vbs(1, 8, 1, 1, pnorm, 400)
    tree = seq.read_vbs()
    seq.compensate_vbs(1, 8)
    comp = seq.read_compensated_range(0, len(frames) - 1)
    got = seq.interp(fd, bs, sw, pnorm, bias)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    assert np.array_equal(seq.read_mv(), mv)
    for a, b in zip(seq.read_vbs(), tree):
        assert np.array_equal(a, b)
    assert np.array_equal(seq.read_compensated_range(0, len(frames) - 1), comp)
    seq.close()
    assert all(len(a) == P for a in got)
    for k in range(P):
        want = interp.search(frames[k], frames[k + fd], bs, sw, pnorm, bias)
        want = want + (interp.interpolate(frames[k], frames[k + fd], want[0], bs),)
        same([a[k] for a in got[:4]], want, ("gme_seq_interp", fd, k))
        assert got[4][k] == (interp.sse(want[3], frames[k + fd // 2]) if fd % 2 == 0 else -1), (fd, k)
    return got


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
h = hashlib.sha256()
for fd in (1, 2, 3):
    for a in seq.interp(fd, 8, 3, 0, 4):
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_sequence(native, tmp_path):
    """Seven noise frames of 40 x 72, frame distances 1, 2 and 3, blocks of 8: every pair against the host, the sequence's other
    results untouched, a partial range against the full one, each output alone, the same bytes with two pairs per launch
    (GME_MAX_GRID_PAIRS=2, a fresh process), and the range, frame-count and argument errors."""
    rng = np.random.default_rng(72)
    frames = rng.integers(0, 256, size=(7, 40, 72), dtype=np.uint8)
    ctx = native.default_context()
    h = hashlib.sha256()
    full = {}
    for fd in (1, 2, 3):
        full[fd] = check_sequence(native, frames, fd, 8, 3, 0, 4)
        for a in full[fd]:
            h.update(np.ascontiguousarray(a).tobytes())
    check_sequence(native, frames, 2, 16, 2, 1, 256)
    seq = native.Sequence.from_frames(ctx, frames)
    for fd in (1, 2, 3):
        P = 7 - fd
        part = seq.interp(fd, 8, 3, 0, 4, 1, min(2, P - 1))
        for a, b in zip(part, full[fd]):
            assert np.array_equal(a, b[1:1 + min(2, P - 1)])
        assert all(len(a) == 0 for a in seq.interp(fd, 8, 3, 0, 4, P, 0))
        for first, count in ((P - 1, 2), (-1, 1), (0, P + 1), (0, -1)):
            with pytest.raises(IndexError, match="outside"):
                seq.interp(fd, 8, 3, 0, 4, first, count)
    # any output may be NULL: each one alone, and none at all
    mv, cost, dist, made, sse = (np.zeros_like(a) for a in full[2])
    i32, i64, u8 = native._c_i32p, native._c_i64p, native._c_u8p
    call = seq.lib.gme_seq_interp
    assert call(seq.handle, 2, 8, 3, 0, 4, 0, 5, native._p(mv, i32), None, None, None, None) == 0 and np.array_equal(mv, full[2][0])
    assert call(seq.handle, 2, 8, 3, 0, 4, 0, 5, None, native._p(cost, i64), None, None, None) == 0 and np.array_equal(cost, full[2][1])
    assert call(seq.handle, 2, 8, 3, 0, 4, 0, 5, None, None, native._p(dist, i64), None, None) == 0 and np.array_equal(dist, full[2][2])
    assert call(seq.handle, 2, 8, 3, 0, 4, 0, 5, None, None, None, native._p(made, u8), None) == 0 and np.array_equal(made, full[2][3])
    assert call(seq.handle, 2, 8, 3, 0, 4, 0, 5, None, None, None, None, native._p(sse, i64)) == 0 and np.array_equal(sse, full[2][4])
    assert call(seq.handle, 2, 8, 3, 0, 4, 0, 5, None, None, None, None, None) == 0
    sse[:] = 0
    assert call(seq.handle, 3, 8, 3, 0, 4, 0, 4, None, None, None, None, native._p(sse, i64)) == 0 and np.all(sse[:4] == -1)
    # also in split-phase mode the call computes and returns
    seq.set_split_phase(True)
    for a, b in zip(seq.interp(2, 8, 3, 0, 4), full[2]):
        assert np.array_equal(a, b)
    seq.set_split_phase(False)
    # too few frames for the distance
    with pytest.raises(IndexError, match="needs at least 8 frames"):
        seq.interp(7, 8, 3, 0, 4)
    assert call(seq.handle, 0, 8, 3, 0, 4, 0, 1, None, None, None, None, None) == native.ERR_ARG
    # arguments (block_size, search_window, pnorm, bias): the host rules raise ValueError, the library's own checks GME_ERR_ARG
    p = np.zeros((40, 72), np.uint8)
    for args in ((3, 1, 0, 0), (68, 1, 0, 0), (8, 9, 0, 0), (8, -1, 0, 0), (8, 1, 2, 0), (8, 1, 0, -1), (8, 1, 0, (1 << 16) + 1), (48, 1, 0, 0)):
        with pytest.raises(ValueError):
            seq.interp(1, *args)
        assert call(seq.handle, 1, *args, 0, 1, None, None, None, None, None) == native.ERR_ARG
        with pytest.raises(ValueError):
            ctx.interp(p, p, *args)
        assert seq.lib.gme_interp_u8(ctx.handle, native._p(p, u8), native._p(p, u8), None, 40, 72, 72, *args, None, None, None, None,
                                     None) == native.ERR_ARG
    assert seq.lib.gme_interp_u8(ctx.handle, None, native._p(p, u8), None, 40, 72, 72, 8, 1, 0, 0, None, None, None, None, None) == native.ERR_ARG
    # every output of gme_interp_u8 may be NULL
    mv1 = np.zeros_like(full[2][0][0])
    assert seq.lib.gme_interp_u8(ctx.handle, native._p(frames[0], u8), native._p(frames[2], u8), None, 40, 72, 72, 8, 3, 0, 4,
                                 native._p(mv1, i32), None, None, None, None) == 0
    assert np.array_equal(mv1, full[2][0][0])
    assert seq.lib.gme_interp_u8(ctx.handle, native._p(frames[0], u8), native._p(frames[2], u8), None, 40, 72, 72, 8, 3, 0, 4, None, None,
                                 None, None, None) == 0
    seq.close()
    np.save(tmp_path / "frames.npy", frames)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd")})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy")], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


def test_real_frames(native, golden):
    """g9 frames 10 .. 14 at frame distance 2, blocks of 16, window 8, the default biases: device equal to host, and the PSNR of
    the interpolation and of the plain average against the true middle frames (printed; nothing is asserted about them)."""
    import interp
    g9 = np.ascontiguousarray(golden("g9_pan240seq")["frames"][10:15])
    H, W = g9.shape[1:]
    for pnorm in (0, 1):
        bias = interp.default_bias(16, pnorm)
        mv, cost, dist, made, sse = check_sequence(native, g9, 2, 16, 8, pnorm, bias)
        for k in range(3):
            s = interp.summary(mv[k], H, W, int(sse[k]), interp.sse(interp.average(g9[k], g9[k + 2]), g9[k + 1]))
            print("g9 frame %d from %d and %d, norm %d bias %d: interpolation %.4f dB, plain average %.4f dB, median vector %s, %.1f %% non-zero"
                  % (11 + k, 10 + k, 12 + k, pnorm, bias, s["psnr_interp"], s["psnr_average"], s["median_vector"], 100.0 * s["nonzero_share"]))


def test_upconvert(native):
    """interp.upconvert on the device: the originals at the even indices, the host's interpolated frames between them."""
    import interp
    frames = np.random.default_rng(9).integers(0, 256, size=(4, 24, 40), dtype=np.uint8)
    out = interp.upconvert(frames, block_size=8, search_window=2, pnorm_distance=1)
    assert out.shape == (7, 24, 40) and np.array_equal(out[0::2], frames)
    for k in range(3):
        mv = interp.search(frames[k], frames[k + 1], 8, 2, 1, 64)[0]
        assert np.array_equal(out[2 * k + 1], interp.interpolate(frames[k], frames[k + 1], mv, 8))
        assert np.array_equal(interp.frame(frames[k], frames[k + 1], 8, 2, 1), out[2 * k + 1])
        assert np.array_equal(interp.motion_field(frames[k], frames[k + 1], 8, 2, 1)[0], mv)


def test_cli_interp(native, golden, tmp_path, capsys):
    import gme_cli
    import interp
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(5):
        Image.fromarray(np.ascontiguousarray(g9[10 + k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["interp", "-p", str(d), "-fi", "2", "-o", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "bias 16" in out and "median vector: (" in out and "non-zero vectors: " in out
    assert "psnr interpolation: " in out and "psnr plain average: " in out
    rec = json.loads((tmp_path / "out" / "interp.json").read_text())
    assert set(rec) >= {"median_vector", "nonzero_share", "sse_interp", "sse_average", "psnr_interp", "psnr_average", "options", "shape"}
    assert rec["options"]["bias"] == 16 and rec["shape"] == list(res["mv"].shape[:2])
    mv = interp.search(g9[10], g9[12], 16, 8, 0, 16)[0]
    want = interp.interpolate(g9[10], g9[12], mv, 16)
    assert np.array_equal(res["frame"], want) and rec["sse_interp"] == interp.sse(want, g9[11])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "interp.png")), want)
    assert not (tmp_path / "out" / "upconverted").exists()
    res = gme_cli.main(["interp", "-p", str(d), "-fi", "1", "-fd", "1", "-pn", "1", "-bs", "32", "-sw", "4", "--upconvert", "-o", str(tmp_path / "up")])
    out = capsys.readouterr().out
    assert "blocks of 32, window 4, bias 1024" in out and "psnr" not in out and "up-converted: 9 frames" in out
    names = sorted(os.listdir(tmp_path / "up" / "upconverted"))
    assert names == ["%04d.png" % k for k in range(9)]
    for k in range(5):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "up" / "upconverted" / ("%04d.png" % (2 * k)))), g9[10 + k])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "up" / "upconverted" / "0001.png")), res["frame"])
    with pytest.raises(IndexError):
        gme_cli.main(["interp", "-p", str(d), "-fi", "1"])
    gme_cli.main(["info"])
    assert "frame interpolation" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_interp.remarks, as the compiler wrote them: no instance of the kernels spills or uses scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_interp.hip"]
    assert sorted(r["name"].replace(" ", "") for r in rows) == ["k_interp<0>", "k_interp<16>", "k_interp<32>", "k_interp_frame"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
