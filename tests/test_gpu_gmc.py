"""Global motion compensation on the device (k_gmc and k_predict_gmc of bbme_gmc.hip through gme_gmc_u8, gme_seq_gmc,
gme_seq_read_gmc and gme_seq_predict_gmc) against the host definition gmc.py: byte for byte on noise under every warp of
gmc_cases, ties, saturated content, the zoom scene, a padded stride, a batched sequence and real frames, plus the error paths and
the CLI.  Needs an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gmc_cases as gc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mode", "cost", "costs")


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def instance(bs):
    return "k_gmc<%d>" % (bs if bs in (16, 32) else 0)


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4])


def check_pair(native, ref, cur, h, f, bs, pnorm, penalty, want=None):
    """gme_gmc_u8 on host buffers against gmc.decide (``want``: its result where a test has it already), the predicted frame
    against gmc.predict and its squared error against gmc.sse -> the host's result."""
    import gmc
    ctx = native.default_context()
    if want is None:
        want = gmc.decide(ref, cur, h, f, bs, pnorm, penalty)
    got = ctx.gmc(ref, cur, h, f, bs, pnorm, penalty)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    what = ("gme_gmc_u8", cur.shape, bs, pnorm, penalty, [float(v) for v in h])
    same(got[:3], want, what)
    pred = gmc.predict(ref, h, want[0], f, bs)
    assert got[3].dtype == np.uint8 and np.array_equal(got[3], pred), (what, np.argwhere(got[3] != pred)[:4])
    assert got[4] == gmc.sse(cur, pred), what
    return want


@pytest.mark.parametrize("case", gc.NOISE)
def test_noise(native, case):
    """Noise pairs of sizes that are no multiple of the block, half of the blocks copied from where their vector points, with
    vectors in [-6, 6] (some outside), under every warp of gmc_cases (identity with its clamped far tap, integer and fractional
    translations, rotation with zoom, projective, everything outside, unusable, NaN), both norms, at the default penalty."""
    import gmc
    (H, W), bs = case
    ref, cur, _ = gc.noise_pair(case)
    for name in gc.WARPS:
        h, f = gc.noise_field(case, name)
        for pnorm in (0, 1):
            want = check_pair(native, ref, cur, h, f, bs, pnorm, gmc.default_penalty(bs, pnorm), gc.noise_result(case, name, pnorm))
            gc.check_modes(name, want[0])


def test_ties(native):
    """Constant frames: cg = cl wherever both exist, and GLOBAL wins at penalty 0."""
    ref, cur = gc.ties_frames()
    rng = np.random.default_rng(5)
    for bs in (8, 16):
        f = rng.integers(-2, 3, size=(37 // bs, 53 // bs, 2)).astype(np.int32)
        for name in ("identity", "fractional", "rotzoom"):
            for pnorm in (0, 1):
                for penalty in (0, 64):
                    mode, cost, costs = check_pair(native, ref, cur, gc.warp_of(name, 37, 53), f, bs, pnorm, penalty)
                    both = (costs[:, :, 0] >= 0) & (costs[:, :, 1] >= 0)
                    assert both.any() and np.all(mode[both] == 0) and np.array_equal(costs[both, 0], costs[both, 1])


def test_saturated(native):
    """Blocks of 64 on frames of 0 and 255: the largest cost there is, 64 * 64 * 255^2 under MSE, and with the penalty 2^30 the
    largest sum of a decision.  Nothing wraps."""
    import direct
    lo, hi = np.zeros((130, 135), np.uint8), np.full((130, 135), 255, np.uint8)
    f = np.zeros((2, 2, 2), np.int32)
    for pnorm, top in ((1, 64 * 64 * 255 * 255), (0, 64 * 64 * 255)):
        for penalty in (0, 1 << 30):
            mode, cost, costs = check_pair(native, lo, hi, direct.IDENTITY, f, 64, pnorm, penalty)
            assert np.all(mode == 0) and np.all(cost == top) and np.all(costs == top)
            mode, cost, costs = check_pair(native, lo, hi, gc.warp_of("far", 130, 135), f, 64, pnorm, penalty)
            assert np.all(mode == 1) and np.all(cost == top + penalty) and np.all(costs == (-1, top))
            mode, cost, costs = check_pair(native, hi, hi, gc.warp_of("fractional", 130, 135), f, 64, pnorm, penalty)
            assert np.all(mode < 2) and np.all(costs[costs >= 0] == 0) and np.all(cost == np.where(mode == 0, 0, penalty))


@pytest.mark.parametrize("pnorm", (0, 1))
def test_zoom_scene(native, pnorm):
    """The scene of tests/test_gmc_host.py on the device: equal to the host on the host's field, and through a sequence on the
    device's own field, where the conditions of the scene hold as well."""
    import gmc
    ref, cur, h = gc.zoom_scene()
    f, mode, cost, costs = gc.scene_result(pnorm)
    penalty = gmc.default_penalty(gc.SCENE_BLOCK, pnorm)
    check_pair(native, ref, cur, h, f, gc.SCENE_BLOCK, pnorm, penalty, want=(mode, cost, costs))
    gc.check_scene(f, mode, costs)
    seq = native.Sequence.from_frames(native.default_context(), np.ascontiguousarray(np.stack([ref, cur])))
    seq.gmc(1, h.reshape(1, 8), gc.SCENE_BLOCK, gc.SCENE_WINDOW, 0, pnorm, penalty)
    got = [a[0] for a in seq.read_gmc()]
    seq.close()
    assert np.array_equal(got[0], f) and got[4] == 1
    same(got[1:4], gmc.decide(ref, cur, h, got[0], gc.SCENE_BLOCK, pnorm, penalty), "the sequence's own field")
    gc.check_scene(got[0], got[1], got[3])


def test_padded_stride(native):
    """Rows 7 and 11 bytes longer than the frame is wide: views into wider arrays of other content."""
    import gmc
    case = gc.NOISE[3]
    (H, W), bs = case
    ref, cur, _ = gc.noise_pair(case)
    h, f = gc.noise_field(case, "projective")
    rng = np.random.default_rng(9)
    ctx = native.default_context()
    for pad in (7, 11):
        wide = rng.integers(0, 256, size=(2, H, W + pad), dtype=np.uint8)
        wide[0, :, :W], wide[1, :, :W] = ref, cur
        for pnorm in (0, 1):
            penalty = gmc.default_penalty(bs, pnorm)
            got = ctx.gmc(wide[0, :, :W], wide[1, :, :W], h, f, bs, pnorm, penalty)
            want = gc.noise_result(case, "projective", pnorm)
            same(got[:3], want, ("stride", W + pad, pnorm))
            pred = gmc.predict(ref, h, want[0], f, bs)
            assert np.array_equal(got[3], pred) and got[4] == gmc.sse(cur, pred)


SEQ_SHAPE, SEQ_WINDOW = (5, 48, 80), 4
SEQ_WARPS = ("rotzoom", "unusable", "fractional", "projective")


def seq_frames():
    rng = np.random.default_rng(48)
    base = rng.integers(0, 256, size=(SEQ_SHAPE[1] + 8, SEQ_SHAPE[2] + 8), dtype=np.uint8)
    # a pan of one pixel per frame with fresh noise of +-6 on every frame: the searches find real vectors
    frames = np.stack([np.clip(base[4:-4, k:k + SEQ_SHAPE[2]].astype(np.int64) + rng.integers(-6, 7, size=SEQ_SHAPE[1:]), 0, 255)
                       for k in range(SEQ_SHAPE[0])]).astype(np.uint8)
    return np.ascontiguousarray(frames)


def seq_warps(pairs):
    return np.stack([gc.warp_of(SEQ_WARPS[k % len(SEQ_WARPS)], SEQ_SHAPE[1], SEQ_SHAPE[2]) for k in range(pairs)])


def check_sequence(native, seq, frames, fd, bs, sw, procedure, pnorm, penalty, h):
    """gme_seq_gmc over a resident sequence: the field against the search it is defined by, every pair against gmc.decide on
    that field, the predicted frames and their SSE against gmc.predict -> (the five arrays, sse, predicted frames)."""
    import bbme
    import gmc
    ctx = native.default_context()
    P = len(frames) - fd
    seq.gmc(fd, h, bs, sw, procedure, pnorm, penalty)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    got = seq.read_gmc()
    assert len(got[0]) == P
    sse = seq.predict_gmc()
    comp = seq.read_compensated_range(0, P)
    for k in range(P):
        ref, cur = frames[k], frames[k + fd]
        assert got[4][k] == int(gmc.usable(h[k], *cur.shape)), ("usable", k)
        assert np.array_equal(got[0][k], bbme.get_motion_field(cur, ref, bs, sw, procedure, pnorm)[:, :, :2]), ("f", k)
        want = gmc.decide(ref, cur, h[k], got[0][k], bs, pnorm, penalty)
        same([a[k] for a in got[1:4]], want, ("gme_seq_gmc", fd, bs, procedure, pnorm, k))
        pred = gmc.predict(ref, h[k], want[0], got[0][k], bs)
        assert np.array_equal(comp[k], pred), (k, np.argwhere(comp[k] != pred)[:4])
        assert sse[k] == gmc.sse(cur, pred)
    return got, sse, comp


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
h = hashlib.sha256()
for fd in (1, 2):
    seq.gmc(fd, np.load(sys.argv[2])[:len(frames) - fd], 8, 4, 0, 0, 16)
    for a in seq.read_gmc():
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.ascontiguousarray(seq.predict_gmc()).tobytes())
    h.update(np.ascontiguousarray(seq.read_compensated_range(0, len(frames) - fd)).tobytes())
print("digest", h.hexdigest())
"""


def test_sequence(native, tmp_path):
    """Five frames of 48 x 80, frame distances 1 and 2, blocks of 16 and 8, window 4, the exhaustive and the diamond search, both
    norms, per-pair warps of which one is unusable: the field, every pair, the predicted frames and their SSE against the host; the
    motion field and the quarter-pel, variable-block-size and bidirectional results untouched; a partial read; the same bytes
    with two pairs per launch (GME_MAX_GRID_PAIRS=2, a fresh process); the state and argument errors."""
    import gmc
    frames = seq_frames()
    N = len(frames)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    for call in (seq.read_gmc, seq.predict_gmc):
        with pytest.raises(native.GmeError, match="before gme_seq_gmc"):
            call()
    digest = hashlib.sha256()
    for fd in (1, 2):
        P = N - fd
        h = seq_warps(P)
        for bs in (16, 8):
            # what the sequence holds besides: a motion field with its quarter-pel field and tree, and a bidirectional result
            seq.bbme(fd, bs, SEQ_WINDOW, 0, 0)
            seq.subpel(fd, bs, 0, 2)
            seq.vbs(fd, bs, 1, 1, 0, 400)
            seq.bipred(1, bs, SEQ_WINDOW, 0, 0, 1, 1, 64)
            held = [seq.read_mv()] + list(seq.read_qmv()) + list(seq.read_vbs()) + list(seq.read_bipred())
            for procedure in (0, 3):
                for pnorm in (0, 1):
                    penalty = gmc.default_penalty(bs, pnorm)
                    got, sse, comp = check_sequence(native, seq, frames, fd, bs, SEQ_WINDOW, procedure, pnorm, penalty, h)
                    now = [seq.read_mv()] + list(seq.read_qmv()) + list(seq.read_vbs()) + list(seq.read_bipred())
                    for a, b in zip(now, held):
                        assert np.array_equal(a, b)
                    if (bs, procedure, pnorm) == (8, 0, 0):
                        for a in got:
                            digest.update(np.ascontiguousarray(a).tobytes())
                        digest.update(np.ascontiguousarray(sse).tobytes())
                        digest.update(np.ascontiguousarray(comp).tobytes())
        # the last call's result: a partial read, range errors, NULL outputs
        full = seq.read_gmc()
        part = seq.read_gmc(1, 2)
        for a, b in zip(part, full):
            assert np.array_equal(a, b[1:3])
        for first, count in ((P - 1, 2), (-1, 1), (0, P + 1)):
            with pytest.raises(IndexError, match="outside"):
                seq.read_gmc(first, count)
        mode = np.zeros_like(full[1])
        assert seq.lib.gme_seq_read_gmc(seq.handle, 0, P, None, native._p(mode, native._c_u8p), None, None, None) == 0
        assert np.array_equal(mode, full[1])
        costs = np.zeros_like(full[3])
        assert seq.lib.gme_seq_read_gmc(seq.handle, 0, P, None, None, None, native._p(costs, native._c_i64p), None) == 0
        assert np.array_equal(costs, full[3])
        assert seq.lib.gme_seq_predict_gmc(seq.handle, None) == 0
    # too few frames for the distance
    with pytest.raises(IndexError):
        seq.gmc(N, np.zeros((0, 8)), 8, SEQ_WINDOW, 0, 0, 0)
    hp = native._p(np.ascontiguousarray(seq_warps(N)), native._c_f64p)
    assert seq.lib.gme_seq_gmc(seq.handle, 0, 8, SEQ_WINDOW, 0, 0, 0, hp) == native.ERR_ARG
    assert seq.lib.gme_seq_gmc(seq.handle, N, 8, SEQ_WINDOW, 0, 0, 0, hp) == native.ERR_ARG
    assert seq.lib.gme_seq_gmc(seq.handle, 1, 8, SEQ_WINDOW, 0, 0, 0, None) == native.ERR_ARG
    # arguments (block_size, pnorm, penalty): the host rules raise ValueError, the library's own checks GME_ERR_ARG
    p = np.zeros(SEQ_SHAPE[1:], np.uint8)
    u8 = native._c_u8p
    for args in ((3, 0, 0), (68, 0, 0), (8, 2, 0), (8, -1, 0), (8, 0, -1), (8, 0, (1 << 30) + 1)):
        bs, pnorm, penalty = args
        with pytest.raises(ValueError):
            seq.gmc(1, seq_warps(N - 1), bs, SEQ_WINDOW, 0, pnorm, penalty)
        assert seq.lib.gme_seq_gmc(seq.handle, 1, bs, SEQ_WINDOW, 0, pnorm, penalty, hp) == native.ERR_ARG
        f = np.zeros((max(1, p.shape[0] // bs), max(1, p.shape[1] // bs), 2), np.int32)
        mode = np.zeros(f.shape[:2], np.uint8)
        with pytest.raises(ValueError):
            ctx.gmc(p, p, seq_warps(1)[0], f, *args)
        assert seq.lib.gme_gmc_u8(ctx.handle, native._p(p, u8), native._p(p, u8), p.shape[0], p.shape[1], p.shape[1], *args, hp,
                                  native._p(f, native._c_i32p), native._p(mode, u8), None, None, None, None) == native.ERR_ARG
    assert seq.lib.gme_seq_gmc(seq.handle, 1, 8, SEQ_WINDOW, 4, 0, 0, hp) == native.ERR_ARG             # the search's own rules
    # the refused calls left the result valid; new frame data ends the validity
    assert np.array_equal(seq.read_gmc()[1], full[1])
    seq.upload(0, frames[:1])
    for call in (seq.read_gmc, seq.predict_gmc):
        with pytest.raises(native.GmeError, match="before gme_seq_gmc"):
            call()
    seq.close()
    # every output of gme_gmc_u8 but mode_out may be NULL
    h1 = np.ascontiguousarray(seq_warps(1)[0])
    f = np.ascontiguousarray(full[0][0])
    want = ctx.gmc(frames[0], frames[2], h1, f, 8, 1, 1024)
    mode = np.zeros_like(want[0])
    assert seq.lib.gme_gmc_u8(ctx.handle, native._p(frames[0], u8), native._p(frames[2], u8), p.shape[0], p.shape[1], p.shape[1], 8, 1, 1024,
                              native._p(h1, native._c_f64p), native._p(f, native._c_i32p), native._p(mode, u8), None, None, None,
                              None) == 0
    assert np.array_equal(mode, want[0])
    np.save(tmp_path / "frames.npy", frames)
    np.save(tmp_path / "warps.npy", seq_warps(N - 1))
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd")})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy"), str(tmp_path / "warps.npy")],
                         env=dict(os.environ, GME_MAX_GRID_PAIRS="2"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == digest.hexdigest()


def test_real_frames(native, golden):
    """Pairs 0 .. 2 of g9 (the pan240 clip), blocks of 16, window 16, the warps of the direct projective refinement, both norms:
    device equal to host at the default penalty, and under MSE at penalty 0 with the exhaustive search the chosen prediction's
    squared error is at most the global-only and the local-only one (vector 0 is a search candidate, so cl is never above the
    co-located cost that the local-only prediction falls back on, and a chosen block costs the smaller of what exists).  The PSNR
    figures are printed; nothing else is asserted about them."""
    import gmc
    import roadmap
    g9 = np.ascontiguousarray(golden("g9_pan240seq")["frames"][:4])
    H, W = g9.shape[1:]
    seq = native.Sequence.from_frames(native.default_context(), g9)
    h = roadmap.refine_sequence(seq, 1)[0]
    for pnorm in (0, 1):
        for penalty in (gmc.default_penalty(16, pnorm), 0):
            got, sse, comp = check_sequence(native, seq, g9, 1, 16, 16, 0, pnorm, penalty, h)
            for k in range(3):
                f, mode, cost, costs = (a[k] for a in got[:4])
                single = [gmc.sse(g9[k + 1], gmc.predict(g9[k], h[k], gmc.all_mode(costs, which), f, 16)) for which in (0, 1)]
                s = gmc.summary(mode, single[0], single[1], int(sse[k]), H, W)
                print("g9 pair %d norm %d penalty %d: psnr global only %.4f dB, local only %.4f dB, chosen %.4f dB, modes %s"
                      % (k, pnorm, penalty, s["psnr_global"], s["psnr_local"], s["psnr_chosen"],
                         " ".join("%.1f%%" % (100.0 * v) for v in s["mode_share"])))
                if pnorm == 1 and penalty == 0:
                    assert int(sse[k]) <= single[0] and int(sse[k]) <= single[1], (k, int(sse[k]), single)
    seq.close()


def test_cli_gmc(native, golden, tmp_path, capsys):
    import gme_cli
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(4):
        Image.fromarray(np.ascontiguousarray(g9[k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["gmc", "-p", str(d), "-fi", "2", "-fd", "2", "-o", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "penalty 64" in out and "modes: global " in out
    assert "psnr global only: " in out and "psnr local only: " in out and "psnr chosen: " in out
    rec = json.loads((tmp_path / "out" / "gmc.json").read_text())
    assert set(rec) >= {"mode_share", "sse_global", "sse_local", "sse_chosen", "psnr_global", "psnr_local", "psnr_chosen", "options",
                        "shape", "h", "usable"}
    assert rec["options"]["penalty"] == 64 and rec["options"]["estimator"] == "projective"
    assert rec["shape"] == list(res["mode"].shape) and len(rec["mode_share"]) == 3 and len(rec["h"]) == 8
    assert rec["mode_share"][0] == float(np.mean(res["mode"] == 0))
    img = np.asarray(Image.open(tmp_path / "out" / "modes.png"))
    assert img.shape[:2] == g9.shape[1:] and set(np.unique(img).tolist()) <= {0, 128, 255}
    assert np.array_equal(img[:res["mode"].shape[0] * 16:16, :res["mode"].shape[1] * 16:16], np.array([0, 128, 255], np.uint8)[res["mode"]])
    gme_cli.main(["gmc", "-p", str(d), "-fi", "1", "-pn", "1", "-sw", "4", "--estimator", "affine"])
    out = capsys.readouterr().out
    assert "affine warp" in out and "penalty 1024" in out
    with pytest.raises(IndexError):
        gme_cli.main(["gmc", "-p", str(d), "-fi", "4"])
    gme_cli.main(["info"])
    assert "global motion compensation" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_gmc.remarks, as the compiler wrote them: no instance of the kernels spills or uses scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_gmc.hip"]
    assert sorted(r["name"].replace(" ", "") for r in rows) == ["k_gmc<0>", "k_gmc<16>", "k_gmc<32>", "k_predict_gmc"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
