"""Bidirectional block prediction on the device (k_bipred and k_predict_bipred of bbme_bipred.hip through gme_bipred_u8,
gme_seq_bipred, gme_seq_read_bipred and gme_seq_predict_bipred) against the host definition bipred.py: byte for byte on noise
with arbitrary input fields, ties, saturated content, the occlusion scene, a batched sequence and real frames, plus the error
paths and the CLI.  Needs an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bipred_cases as bc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mode", "v0", "v1", "cost", "costs")


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def instance(bs):
    return "k_bipred<%d>" % (bs if bs in (16, 32) else 0)


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4])


def check_triple(native, past, mid, nxt, f0, f1, bs, r, rounds, pnorm, penalty, want=None):
    """gme_bipred_u8 on host buffers against bipred.decide (``want``: its result where a test has it already), the predicted
    frame against bipred.predict and its squared error against subpel.sse -> the host's result."""
    import bipred
    import subpel
    ctx = native.default_context()
    if want is None:
        want = bipred.decide(past, mid, nxt, f0, f1, bs, r, rounds, pnorm, penalty)
    got = ctx.bipred(past, mid, nxt, f0, f1, bs, r, rounds, pnorm, penalty)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    what = ("gme_bipred_u8", mid.shape, bs, r, rounds, pnorm, penalty)
    same(got[:5], want, what)
    pred = bipred.predict(past, nxt, *want[:3], bs)
    assert got[5].dtype == np.uint8 and np.array_equal(got[5], pred), (what, np.argwhere(got[5] != pred)[:4])
    assert got[6] == subpel.sse(mid, pred), what
    return want


@pytest.mark.parametrize("case", bc.NOISE)
def test_noise(native, case):
    """Noise triples of sizes that are no multiple of the block, with random input fields whose vectors lie in [-6, 6] (some
    blocks have one vector outside, some both), both norms, at the penalty of bipred_cases at which all four modes occur on the
    host."""
    shape, bs, r, rounds = case
    past, mid, nxt, f0, f1 = bc.noise_triple(case)
    for pnorm in (0, 1):
        check_triple(native, past, mid, nxt, f0, f1, bs, r, rounds, pnorm, bc.PENALTY[case, pnorm], bc.noise_result(case, pnorm))


def test_ties(native):
    """Constant frames (c0 = c1 = cb: mode 0 at penalty 0, and every candidate of every pass ties with the incumbent) and
    vertical stripes of period 2 against their complement (many equal costs: the definition's order decides), blocks of 8 and
    16, both norms."""
    flat = (np.full((37, 53), 90, np.uint8), np.full((37, 53), 97, np.uint8), np.full((37, 53), 90, np.uint8))
    s = np.tile(np.array([0, 255], np.uint8), (37, 27))[:, :53]
    stripes = (s, 255 - s, s)
    rng = np.random.default_rng(5)
    for frames in (flat, stripes):
        for bs, r, rounds in ((8, 1, 2), (16, 2, 2), (16, 1, 1)):
            f = rng.integers(-2, 3, size=(2, 37 // bs, 53 // bs, 2)).astype(np.int32)
            for pnorm in (0, 1):
                for penalty in (0, 64):
                    mode, v0, v1, cost, costs = check_triple(native, *frames, f[0], f[1], bs, r, rounds, pnorm, penalty)
                    if frames is flat:
                        assert np.array_equal(v0, f[0]) and np.array_equal(v1, f[1])
                        both = costs[:, :, 2] >= 0
                        assert np.all(mode[both] == 0) and np.all(costs[both, 0] == costs[both, 2]) and np.all(costs[both, 1] == costs[both, 2])


def test_saturated(native):
    """Blocks of 64 on frames of 0 and 255: past 0, mid 255, next 255 (c0 the largest cost there is, 64 * 64 * 255^2 =
    266 342 400 under MSE; cb = 64 * 64 * 127^2 with the average 128; c1 = 0), the mirror image, and both references 0 (all
    three costs the largest, and cb + 2^30 the largest sum of a decision).  Nothing wraps."""
    lo, hi = np.zeros((130, 135), np.uint8), np.full((130, 135), 255, np.uint8)
    f = np.zeros((2, 2, 2), np.int32)
    for pnorm, top, half in ((1, 266342400, 64 * 64 * 127 * 127), (0, 64 * 64 * 255, 64 * 64 * 127)):
        for penalty in (0, 1 << 30):
            for r, rounds in ((2, 2), (1, 1)):
                mode, v0, v1, cost, costs = check_triple(native, lo, hi, hi, f, f, 64, r, rounds, pnorm, penalty)
                assert np.all(mode == 1) and np.all(cost == 0) and np.all(costs == (top, 0, half)) and not v0.any() and not v1.any()
                mode, v0, v1, cost, costs = check_triple(native, hi, hi, lo, f, f, 64, r, rounds, pnorm, penalty)
                assert np.all(mode == 0) and np.all(cost == 0) and np.all(costs == (0, top, half))
                mode, v0, v1, cost, costs = check_triple(native, lo, hi, lo, f, f, 64, r, rounds, pnorm, penalty)
                assert np.all(mode == 0) and np.all(cost == top) and np.all(costs == (top, top, top))


@pytest.mark.parametrize("pnorm", (0, 1))
def test_occlusion_scene(native, pnorm):
    """The scene of tests/test_bipred_host.py on the device: equal to the host, hence the uncovered blocks choose the frame in
    which they are visible and the others the average."""
    import bipred
    past, mid, nxt = bc.occlusion_scene()
    want = bc.scene_result(pnorm)
    check_triple(native, past, mid, nxt, want[0], want[1], pnorm=pnorm, penalty=bipred.default_penalty(bc.SCENE_BLOCK, pnorm),
                 want=want[2:], bs=bc.SCENE_ARGS["block_size"], r=bc.SCENE_ARGS["radius"], rounds=bc.SCENE_ARGS["rounds"])
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(np.stack([past, mid, nxt])))
    seq.bipred(1, bc.SCENE_BLOCK, bc.SCENE_WINDOW, 0, pnorm, 1, 1, bipred.default_penalty(bc.SCENE_BLOCK, pnorm))
    got = seq.read_bipred()
    seq.close()
    same([a[0] for a in got[2:]], bipred.decide(past, mid, nxt, got[0][0], got[1][0], pnorm=pnorm,
                                               penalty=bipred.default_penalty(bc.SCENE_BLOCK, pnorm), **bc.SCENE_ARGS), "the sequence's own fields")
    bc.check_scene(got[2][0])


def check_sequence(native, frames, fd, bs, sw, pnorm, r, rounds, penalty):
    """gme_seq_bipred over a resident sequence: both fields against the searches they are defined by, every target against
    bipred.decide on those fields, the predicted frames and their SSE against bipred.predict -> (the seven arrays, sse,
    predicted frames) of the device."""
    import bbme
    import bipred
    import subpel
    ctx = native.default_context()
    N = len(frames)
    T = N - 2 * fd
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(frames))
    seq.bbme(fd, bs, sw, 0, pnorm)
    mv = seq.read_mv()
    seq.vbs(fd, bs, 1, 1, pnorm, 400)
    tree = seq.read_vbs()
    seq.bipred(fd, bs, sw, 0, pnorm, r, rounds, penalty)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    got = seq.read_bipred()
    assert len(got[0]) == T
    # the call leaves the sequence's other results as they were
    assert np.array_equal(seq.read_mv(), mv)
    for a, b in zip(seq.read_vbs(), tree):
        assert np.array_equal(a, b)
    sse = seq.predict_bipred()
    comp = seq.read_compensated_range(0, T)
    seq.close()
    for k in range(T):
        t = fd + k
        assert np.array_equal(got[1][k], mv[t]), ("f1", k)
        assert np.array_equal(got[0][k], bbme.get_motion_field(frames[t], frames[t - fd], bs, sw, 0, pnorm)[:, :, :2]), ("f0", k)
        want = bipred.decide(frames[t - fd], frames[t], frames[t + fd], got[0][k], got[1][k], bs, r, rounds, pnorm, penalty)
        same([a[k] for a in got[2:]], want, ("gme_seq_bipred", fd, k))
        pred = bipred.predict(frames[t - fd], frames[t + fd], *want[:3], bs)
        assert np.array_equal(comp[k], pred), (k, np.argwhere(comp[k] != pred)[:4])
        assert sse[k] == subpel.sse(frames[t], pred)
    return got, sse, comp


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
h = hashlib.sha256()
for fd in (1, 3):
    seq.bipred(fd, 8, 3, 0, 0, 1, 2, 300)
    for a in seq.read_bipred():
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.ascontiguousarray(seq.predict_bipred()).tobytes())
    h.update(np.ascontiguousarray(seq.read_compensated_range(0, 7 - 2 * fd)).tobytes())
print("digest", h.hexdigest())
"""


def test_sequence(native, tmp_path):
    """Seven frames of 40 x 72, frame distances 1 and 3, blocks of 8: the fields, every target, the predicted frames and their
    SSE against the host, a partial read against the full one, the sequence's other results untouched, the same bytes with two
    targets per launch (GME_MAX_GRID_PAIRS=2, a fresh process), and the state and argument errors."""
    rng = np.random.default_rng(72)
    frames = rng.integers(0, 256, size=(7, 40, 72), dtype=np.uint8)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    with pytest.raises(native.GmeError, match="before gme_seq_bipred"):
        seq.read_bipred()
    with pytest.raises(native.GmeError, match="before gme_seq_bipred"):
        seq.predict_bipred()
    h = hashlib.sha256()
    for fd in (1, 3):
        T = 7 - 2 * fd
        got, sse, comp = check_sequence(native, frames, fd, 8, 3, 0, 1, 2, 300)
        seq.bipred(fd, 8, 3, 0, 0, 1, 2, 300)
        full = seq.read_bipred()
        for a, b in zip(full, got):
            assert np.array_equal(a, b)
        part = seq.read_bipred(1, min(2, T - 1))
        for a, b in zip(part, full):
            assert np.array_equal(a, b[1:1 + min(2, T - 1)])
        for first, count in ((T - 1, 2), (-1, 1), (0, T + 1)):
            with pytest.raises(IndexError, match="outside"):
                seq.read_bipred(first, count)
        assert np.array_equal(seq.predict_bipred(), sse)
        for a in full:
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(np.ascontiguousarray(sse).tobytes())
        h.update(np.ascontiguousarray(seq.read_compensated_range(0, T)).tobytes())
        # any output may be NULL
        mode = np.zeros_like(full[2])
        assert seq.lib.gme_seq_read_bipred(seq.handle, 0, T, None, None, native._p(mode, native._c_u8p), None, None, None, None) == 0
        assert np.array_equal(mode, full[2])
        costs = np.zeros_like(full[6])
        assert seq.lib.gme_seq_read_bipred(seq.handle, 0, T, None, None, None, None, None, None, native._p(costs, native._c_i64p)) == 0
        assert np.array_equal(costs, full[6])
        assert seq.lib.gme_seq_predict_bipred(seq.handle, None) == 0
    # too few frames for the distance: 7 < 2 * 4 + 1, and a sequence cut to 2 frames at distance 1
    with pytest.raises(IndexError, match="needs at least 9 frames"):
        seq.bipred(4, 8, 3, 0, 0, 1, 1, 0)
    assert seq.lib.gme_seq_bipred(seq.handle, 0, 8, 3, 0, 0, 1, 1, 0) == native.ERR_ARG
    # the refused calls left the result valid; new frame data ends the validity
    assert np.array_equal(seq.read_bipred()[2], full[2])
    seq.upload(0, frames[:1])
    with pytest.raises(native.GmeError, match="before gme_seq_bipred"):
        seq.read_bipred()
    with pytest.raises(native.GmeError, match="before gme_seq_bipred"):
        seq.predict_bipred()
    # arguments (block_size, radius, rounds, pnorm, penalty): the host rules raise ValueError, the library's own checks GME_ERR_ARG
    p = np.zeros((40, 72), np.uint8)
    for args in ((3, 1, 1, 0, 0), (68, 1, 1, 0, 0), (8, 3, 1, 0, 0), (8, -1, 1, 0, 0), (8, 1, 3, 0, 0), (8, 1, -1, 0, 0), (8, 1, 1, 2, 0),
                 (8, 1, 1, 0, -1), (8, 1, 1, 0, (1 << 30) + 1)):
        bs, r, rounds, pnorm, penalty = args
        with pytest.raises(ValueError):
            seq.bipred(1, bs, 3, 0, pnorm, r, rounds, penalty)
        assert seq.lib.gme_seq_bipred(seq.handle, 1, bs, 3, 0, pnorm, r, rounds, penalty) == native.ERR_ARG
        f = np.zeros((max(1, 40 // bs), max(1, 72 // bs), 2), np.int32)
        mode = np.zeros(f.shape[:2], np.uint8)
        with pytest.raises(ValueError):
            ctx.bipred(p, p, p, f, f, *args)
        u8 = native._c_u8p
        assert seq.lib.gme_bipred_u8(ctx.handle, native._p(p, u8), native._p(p, u8), native._p(p, u8), 40, 72, 72, *args,
                                     native._p(f, native._c_i32p), native._p(f, native._c_i32p), native._p(mode, u8), None, None, None,
                                     None, None, None) == native.ERR_ARG
    assert seq.lib.gme_seq_bipred(seq.handle, 1, 8, 3, 4, 0, 1, 1, 0) == native.ERR_ARG          # the search's own rules
    # every output of gme_bipred_u8 but mode_out may be NULL
    f0, f1 = np.ascontiguousarray(full[0][0]), np.ascontiguousarray(full[1][0])
    want = ctx.bipred(frames[0], frames[3], frames[6], f0, f1, 8, 1, 2, 0, 300)
    mode = np.zeros_like(want[0])
    u8 = native._c_u8p
    assert seq.lib.gme_bipred_u8(ctx.handle, native._p(frames[0], u8), native._p(frames[3], u8), native._p(frames[6], u8), 40, 72, 72, 8, 1,
                                 2, 0, 300, native._p(f0, native._c_i32p), native._p(f1, native._c_i32p), native._p(mode, u8), None, None,
                                 None, None, None, None) == 0
    assert np.array_equal(mode, want[0]) and np.array_equal(mode, full[2][0])
    seq.close()
    np.save(tmp_path / "frames.npy", frames)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd")})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy")], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


def test_real_frames(native, golden):
    """Three triples of g9 (the pan240 clip), blocks of 16, window 16, radius 1, one round, the CLI's default penalties: device
    equal to host, and the PSNR of the past-only, the next-only and the chosen prediction (printed; nothing is asserted about
    them)."""
    import bipred
    g9 = np.ascontiguousarray(golden("g9_pan240seq")["frames"][:5])
    H, W = g9.shape[1:]
    for pnorm in (0, 1):
        penalty = bipred.default_penalty(16, pnorm)
        got, sse, comp = check_sequence(native, g9, 1, 16, 16, pnorm, 1, 1, penalty)
        for k in range(3):
            f0, f1, mode, v0, v1 = (a[k] for a in got[:5])
            single = [bipred.sse(g9[k + 1], bipred.predict(g9[k], g9[k + 2], bipred.all_mode(f, which, H, W, 16), f0, f1, 16))
                      for which, f in ((0, f0), (1, f1))]
            s = bipred.summary(mode, f0, f1, v0, v1, single[0], single[1], int(sse[k]), H, W)
            print("g9 target %d norm %d penalty %d: psnr past only %.4f dB, next only %.4f dB, chosen %.4f dB, modes %s, refined %.2f %%"
                  % (k + 1, pnorm, penalty, s["psnr_past"], s["psnr_next"], s["psnr_chosen"],
                     " ".join("%.1f%%" % (100.0 * v) for v in s["mode_share"]), 100.0 * s["refined_share"]))


def test_cli_bipred(native, golden, tmp_path, capsys):
    import gme_cli
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(5):
        Image.fromarray(np.ascontiguousarray(g9[k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["bipred", "-p", str(d), "-fi", "2", "-fd", "2", "-o", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "penalty 64" in out and "modes: past " in out and "refined blocks: " in out
    assert "psnr past only: " in out and "psnr next only: " in out and "psnr chosen: " in out
    rec = json.loads((tmp_path / "out" / "bipred.json").read_text())
    assert set(rec) >= {"mode_share", "refined_share", "sse_past", "sse_next", "sse_chosen", "psnr_past", "psnr_next", "psnr_chosen",
                        "options", "shape"}
    assert rec["options"]["penalty"] == 64 and rec["shape"] == list(res["mode"].shape) and len(rec["mode_share"]) == 4
    assert rec["mode_share"][2] == float(np.mean(res["mode"] == 2))
    gme_cli.main(["bipred", "-p", str(d), "-fi", "1", "-pn", "1", "-r", "2", "--rounds", "2", "-sw", "4"])
    out = capsys.readouterr().out
    assert "radius 2, rounds 2, penalty 1024" in out
    with pytest.raises(IndexError):
        gme_cli.main(["bipred", "-p", str(d), "-fi", "4"])
    gme_cli.main(["info"])
    assert "bidirectional prediction" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_bipred.remarks, as the compiler wrote them: no instance of the kernels spills or uses scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_bipred.hip"]
    assert sorted(r["name"].replace(" ", "") for r in rows) == ["k_bipred<0>", "k_bipred<16>", "k_bipred<32>", "k_predict_bipred"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
