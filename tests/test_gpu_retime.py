"""Frame interpolation at any phase on the device (k_retime and k_retime_frame of bbme_retime.hip through gme_retime_u8 and
gme_retime_clip_u8) against the host definition retime.py: byte for byte on noise at the shapes and phases where the kernel
takes another path, the pan, constant, striped and saturated scenes, a clip under every kind of step, real frames, plus the
error paths and the CLI.  Needs an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import retime_cases as rc

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
    return "k_retime<%d>" % (bs if bs in (16, 32) else 0)


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4])


def check_pair(native, past, nxt, bs, sw, pnorm, bias, n, d, want=None, truth=None):
    """gme_retime_u8 on host buffers against retime.search and retime.interpolate (``want``: their result where a test has it
    already), the squared error against interp.sse where there is a true frame, -1 where there is none -> the host's result."""
    import interp
    ctx = native.default_context()
    if want is None:
        want = rc.host_result(past, nxt, bs, sw, pnorm, bias, n, d)
    got = ctx.retime(past, nxt, bs, sw, pnorm, bias, n, d, truth=truth)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    what = ("gme_retime_u8", past.shape, bs, sw, pnorm, bias, n, d)
    same(got[:4], want, what)
    assert got[4] == (-1 if truth is None else interp.sse(want[3], truth)), what
    return want


@pytest.mark.parametrize("case", rc.NOISE, ids=rc.noise_id)
def test_noise(native, case):
    """Noise pairs at the shapes and phases of retime_cases, both norms, without a bias and at the tool's default one, with a
    third noise frame as the truth."""
    (H, W, bs, sw), (n, d) = case
    past, mid, nxt = rc.noise_pair(case[0])
    for pnorm in (0, 1):
        for bias in rc.noise_biases(case[0], pnorm):
            check_pair(native, past, nxt, bs, sw, pnorm, bias, n, d, rc.noise_result(case, pnorm, bias), truth=mid)


@pytest.mark.parametrize("phase", rc.PAN_PHASES)
def test_pan(native, phase):
    """The pan of tests/test_retime_host.py on the device, with the true intermediate frame as `truth`."""
    truth = rc.pan_frame(*phase)
    mv, _, _, made = check_pair(native, rc.pan_frame(0, 1), rc.pan_frame(1, 1), rc.PAN_BLOCK, rc.PAN_WINDOW, 0, rc.PAN_BIAS, *phase,
                                want=rc.pan_result(phase, 0), truth=truth)
    assert np.all(mv[1:4, 1:6] == rc.PAN_MOVE) and np.array_equal(made[rc.PAN_INTERIOR], truth[rc.PAN_INTERIOR])


@pytest.mark.parametrize("pnorm", (0, 1))
def test_scenes(native, pnorm):
    """The other scenes of tests/test_retime_host.py on the device: the stripes (scan order at bias 0, the bias at 1) and constant
    frames (every candidate ties with the centre)."""
    past, nxt = rc.stripes()
    for bias, vector in ((0, (-14, -16)), (1, (2, 0))):
        mv = check_pair(native, past, nxt, rc.STRIPES_BLOCK, rc.STRIPES_WINDOW, pnorm, bias, *rc.STRIPES_PHASE)[0]
        assert np.all(mv[:, 2:4] == vector)
    for bs, sw, (n, d) in ((8, 4, (1, 3)), (16, 16, (5, 6)), (16, 16, (1, 2))):
        for bias in (0, 5):
            mv, cost, dist, made = check_pair(native, rc.flat(90), rc.flat(97), bs, sw, pnorm, bias, n, d)
            assert not mv.any() and np.array_equal(cost, dist) and np.all(made == ((d - n) * 90 + n * 97 + d // 2) // d)


def test_saturated(native):
    """Blocks of 64 with `past` 0 and `next` 255 (and the reverse): D is 64^2 * 255 (MAE) or 64^2 * 255^2 (MSE), the largest there
    is, in every block and for every candidate, so the centre stays; the frame is the rounded blend.  With the largest bias, 2^16,
    and the largest window the largest J a candidate can have is scored beside it.  Nothing wraps."""
    lo, hi = rc.flat(0, (64, 70)), rc.flat(255, (64, 70))
    import retime
    for n, d in ((1, 2), (63, 64)):
        for past, nxt in ((lo, hi), (hi, lo)):
            D = retime.block_distortions(past, nxt, 64, 16, n, d)          # once for both norms and biases
            level = ((d - n) * int(past[0, 0]) + n * int(nxt[0, 0]) + d // 2) // d
            for pnorm, top in ((0, 64 * 64 * 255), (1, 64 * 64 * 255 * 255)):
                for bias in (0, 1 << 16):
                    want = retime.select(D[pnorm], 16, bias)
                    want = want + (retime.interpolate(past, nxt, want[0], 64, n, d),)
                    mv, cost, dist, made = check_pair(native, past, nxt, 64, 16, pnorm, bias, n, d, want=want, truth=lo)
                    assert not mv.any() and np.all(cost == top) and np.all(dist == top) and np.all(made == level)


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
h = hashlib.sha256()
for step in %(steps)r:
    for a in native.default_context().retime_clip(frames, %(bs)d, %(sw)d, 0, %(bias)d, step=step):
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_clip(native, tmp_path):
    """Seven noise frames of 40 x 72, blocks of 8, the steps 2/5, 1/4, 5/2 and 1/1: every output against the host under
    retime.schedule, copies equal to their frames with zero vectors, a partial range against the full one, an empty range, each
    output alone and none, the range and argument errors, retime.convert and retime.slow_motion, and the same bytes with two
    outputs per launch (GME_MAX_GRID_PAIRS=2, a fresh process)."""
    import retime
    frames = rc.clip()
    N, H, W = frames.shape
    ctx = native.default_context()
    bs, sw, bias = rc.CLIP_BLOCK, rc.CLIP_WINDOW, rc.CLIP_BIAS
    h = hashlib.sha256()
    full = {}
    for step in rc.CLIP_STEPS:
        want = rc.clip_result(step)
        rows = retime.schedule(N, *step)
        got = full[step] = ctx.retime_clip(frames, bs, sw, 0, bias, step=step)
        for name, g, w in zip(("frames", "mv", "cost", "dist"), got, want):
            assert g.dtype == w.dtype and g.shape == w.shape, (step, name, g.shape, w.shape)
            assert np.array_equal(g, w), (step, name, np.argwhere(g != w)[:4])
        for m, (k, n, d) in enumerate(rows):
            if n == 0:
                assert np.array_equal(got[0][m], frames[k]) and not got[1][m].any() and not got[2][m].any() and not got[3][m].any()
        for a in got:
            h.update(np.ascontiguousarray(a).tobytes())
        M = len(rows)
        if any(rows[:, 1]):
            assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " ")
        first, count = min(1, M - 1), min(4, M - 1)
        for a, b in zip(ctx.retime_clip(frames, bs, sw, 0, bias, step=step, first=first, count=count), got):
            assert np.array_equal(a, b[first:first + count])
        assert all(len(a) == 0 for a in ctx.retime_clip(frames, bs, sw, 0, bias, step=step, first=M, count=0))
        for first, count in ((M - 1, 2), (-1, 1), (0, M + 1), (0, -1)):
            with pytest.raises(IndexError, match="outside"):
                ctx.retime_clip(frames, bs, sw, 0, bias, step=step, first=first, count=count)
    # the other norm
    got = ctx.retime_clip(frames, bs, sw, 1, 64, step=(2, 5), first=0, count=6)
    for m, (k, n, d) in enumerate(retime.schedule(N, 2, 5)[:6]):
        if n:
            same([a[m] for a in (got[1], got[2], got[3], got[0])], rc.host_result(frames[k], frames[k + 1], bs, sw, 1, 64, n, d), ("mse", m))
    # the tools over it
    assert np.array_equal(retime.convert(frames, 24, 60, bs, sw, 0, bias), full[(2, 5)][0])
    assert np.array_equal(retime.convert(frames, 60, 24, bs, sw, 0, bias), full[(5, 2)][0])
    assert np.array_equal(retime.slow_motion(frames, 4, bs, sw, 0, bias), full[(1, 4)][0])
    assert np.array_equal(retime.slow_motion(frames, 1, bs, sw, 0, bias), frames)
    # any output may be NULL: each one alone, and none at all; the library's own range and argument checks
    want = full[(2, 5)]
    M = len(want[0])
    made, mv, cost, dist = (np.zeros_like(a) for a in want)
    i32, i64, u8 = native._c_i32p, native._c_i64p, native._c_u8p
    call = ctx.lib.gme_retime_clip_u8
    head = (ctx.handle, native._p(frames, u8), N, H, W, W, bs, sw, 0, bias, 2, 5, 0, M)
    assert call(*head, native._p(made, u8), None, None, None) == 0 and np.array_equal(made, want[0])
    assert call(*head, None, native._p(mv, i32), None, None) == 0 and np.array_equal(mv, want[1])
    assert call(*head, None, None, native._p(cost, i64), None) == 0 and np.array_equal(cost, want[2])
    assert call(*head, None, None, None, native._p(dist, i64)) == 0 and np.array_equal(dist, want[3])
    assert call(*head, None, None, None, None) == 0
    for first, count in ((M - 1, 2), (-1, 1), (0, M + 1), (0, -1)):
        assert call(*head[:12], first, count, None, None, None, None) == native.ERR_ARG
    assert call(ctx.handle, None, N, H, W, W, bs, sw, 0, bias, 2, 5, 0, 1, None, None, None, None) == native.ERR_ARG
    assert call(ctx.handle, native._p(frames, u8), 0, H, W, W, bs, sw, 0, bias, 2, 5, 0, 0, None, None, None, None) == native.ERR_ARG
    for step in ((0, 5), (2, 0), (1, 65), (1001, 30000)):
        assert call(*head[:10], *step, 0, 1, None, None, None, None) == native.ERR_ARG
        with pytest.raises(ValueError):
            ctx.retime_clip(frames, bs, sw, 0, bias, step=step)
    # arguments (block_size, search_window, pnorm, bias) and phases: the host rules raise ValueError, the library's own checks
    # GME_ERR_ARG
    p = np.zeros((40, 72), np.uint8)
    one = ctx.lib.gme_retime_u8
    for args in ((3, 1, 0, 0), (68, 1, 0, 0), (8, 17, 0, 0), (8, -1, 0, 0), (8, 1, 2, 0), (8, 1, 0, -1), (8, 1, 0, (1 << 16) + 1), (48, 1, 0, 0)):
        with pytest.raises(ValueError):
            ctx.retime_clip(frames, *args)
        assert call(ctx.handle, native._p(frames, u8), N, H, W, W, *args, 2, 5, 0, 1, None, None, None, None) == native.ERR_ARG
        with pytest.raises(ValueError):
            ctx.retime(p, p, *args)
        assert one(ctx.handle, native._p(p, u8), native._p(p, u8), None, 40, 72, 72, *args, 1, 2, None, None, None, None, None) == native.ERR_ARG
    for phase in ((0, 2), (2, 2), (3, 2), (1, 65), (1, 0)):
        with pytest.raises(ValueError):
            ctx.retime(p, p, 8, 1, 0, 0, *phase)
        assert one(ctx.handle, native._p(p, u8), native._p(p, u8), None, 40, 72, 72, 8, 1, 0, 0, *phase, None, None, None, None, None) == native.ERR_ARG
    assert one(ctx.handle, None, native._p(p, u8), None, 40, 72, 72, 8, 1, 0, 0, 1, 2, None, None, None, None, None) == native.ERR_ARG
    # every output of gme_retime_u8 may be NULL, and a phase is reduced
    mv1 = np.zeros_like(want[1][1])
    assert one(ctx.handle, native._p(frames[0], u8), native._p(frames[1], u8), None, H, W, W, bs, sw, 0, bias, 4, 10, native._p(mv1, i32), None, None,
               None, None) == 0
    assert np.array_equal(mv1, want[1][1])
    assert one(ctx.handle, native._p(frames[0], u8), native._p(frames[1], u8), None, H, W, W, bs, sw, 0, bias, 2, 5, None, None, None, None, None) == 0
    np.save(tmp_path / "frames.npy", frames)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd"), "steps": rc.CLIP_STEPS, "bs": bs, "sw": sw,
                                "bias": bias})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy")], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


def test_real_frames(native, golden):
    """g9 frames 10 .. 13: the pair (10, 13) at the phases 1/3 and 2/3, blocks of 16, window 16, both norms at the default biases:
    device equal to host, and the PSNR of the made frames and of the plain cross-fade against frames 11 and 12 (printed; nothing
    is asserted about them)."""
    import retime
    g9 = np.ascontiguousarray(golden("g9_pan240seq")["frames"][10:14])
    H, W = g9.shape[1:]
    for n in (1, 2):
        D = retime.block_distortions(g9[0], g9[3], 16, 16, n, 3)            # once for both norms
        for pnorm in (0, 1):
            bias = retime.default_bias(16, pnorm)
            want = retime.select(D[pnorm], 16, bias)
            want = want + (retime.interpolate(g9[0], g9[3], want[0], 16, n, 3),)
            mv, _, _, made = check_pair(native, g9[0], g9[3], 16, 16, pnorm, bias, n, 3, want=want, truth=g9[n])
            s = retime.summary(mv, H, W, retime.sse(made, g9[n]), retime.sse(retime.crossfade(g9[0], g9[3], n, 3), g9[n]))
            print("g9 frame %d from 10 and 13 at phase %d/3, norm %d bias %d: retimed %.4f dB, plain cross-fade %.4f dB, median vector %s, "
                  "%.1f %% non-zero" % (10 + n, n, pnorm, bias, s["psnr_retime"], s["psnr_crossfade"], s["median_vector"],
                                        100.0 * s["nonzero_share"]))


def test_cli_retime(native, golden, tmp_path, capsys):
    import gme_cli
    import retime
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(4):
        Image.fromarray(np.ascontiguousarray(g9[10 + k])).save(d / ("%04d.png" % k))
    clip = np.ascontiguousarray(g9[10:14])
    # the clip form: 4x8 blocks keep the host side of this test short
    res = gme_cli.main(["retime", "-p", str(d), "-o", str(tmp_path / "out"), "--rate-in", "24", "--rate-out", "60", "-bs", "32", "-sw", "4"])
    out = capsys.readouterr().out
    assert "step 2/5" in out and "8 frames" in out and "blocks of 32, window 4, bias 64" in out
    rec = json.loads((tmp_path / "out" / "retime.json").read_text())
    assert set(rec) >= {"schedule", "options", "step", "frames", "shape"}
    rows = retime.schedule(4, 2, 5)
    assert rec["schedule"] == rows.tolist() and rec["step"] == [2, 5] and rec["options"]["bias"] == 64
    assert len(rec["frames"]) == 8 and set(rec["frames"][1]) >= {"median_vector", "nonzero_share"} and rec["frames"][0] == {"copy_of": 0}
    names = sorted(os.listdir(tmp_path / "out" / "retimed"))
    assert names == ["%04d.png" % m for m in range(8)]
    for m, (k, n, dd) in enumerate(rows):
        want = clip[k] if n == 0 else rc.host_result(clip[k], clip[k + 1], 32, 4, 0, 64, n, dd)[3]
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "retimed" / ("%04d.png" % m))), want), m
        assert np.array_equal(res["frames"][m], want)
    res = gme_cli.main(["retime", "-p", str(d), "-o", str(tmp_path / "slow"), "--slow", "2", "-bs", "32", "-sw", "2", "-pn", "1"])
    assert "step 1/2" in capsys.readouterr().out and len(os.listdir(tmp_path / "slow" / "retimed")) == 7
    assert np.array_equal(res["frames"][1], rc.host_result(clip[0], clip[1], 32, 2, 1, 1024, 1, 2)[3])
    # one pair: frames 0 and 3 at phase 1/3, with the true frame 1 in the clip
    res = gme_cli.main(["retime", "-p", str(d), "-fi", "0", "--phase", "1/3", "-bs", "32", "-sw", "6", "-o", str(tmp_path / "one")])
    out = capsys.readouterr().out
    assert "phase 1/3" in out and "psnr retimed: " in out and "psnr plain cross-fade: " in out and "median vector: (" in out
    want = rc.host_result(clip[0], clip[3], 32, 6, 0, 64, 1, 3)[3]
    assert np.array_equal(res["frame"], want) and res["sse_retime"] == retime.sse(want, clip[1])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "one" / "retime.png")), want)
    with pytest.raises(IndexError):
        gme_cli.main(["retime", "-p", str(d), "-fi", "2", "--phase", "1/3"])
    gme_cli.main(["info"])
    assert "retime" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_retime.remarks, as the compiler wrote them: no instance of the kernels spills or uses scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_retime.hip"]
    assert sorted(r["name"].replace(" ", "") for r in rows) == ["k_retime<0>", "k_retime<16>", "k_retime<32>", "k_retime_frame"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
