"""Motion-compensated temporal denoising on the device (k_denoise of bbme_denoise.hip through gme_denoise_u8 and gme_seq_denoise)
against the host definition denoise.py: byte for byte on the cases of denoise_cases with every number of references, strength and
unit, strided input, saturated content, a resident sequence and what it must leave alone, the whole clip, the error paths and the
CLI.  Needs an MI355X."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_cases as dc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("quarter", dc.UNITS)
@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_cases(native, case, quarter):
    """gme_denoise_u8 byte-equal to denoise.frame for R = 1 .. 4 and strength 1, 24, 64; the squared error against a noise frame
    exact, -1 without one."""
    import denoise
    ctx = native.default_context()
    cur, refs, fields, truth = dc.current(case), dc.refs(case), dc.fields(case, quarter), dc.truth(case)
    for R in dc.REFS:
        for strength in dc.STRENGTHS:
            want = dc.want(case, R, strength, quarter)
            got, err = ctx.denoise(cur, refs[:R], fields[:R], case[1], quarter, strength, truth=truth)
            assert ctx.last_bbme_info()["plan"].startswith("k_denoise "), ctx.last_bbme_info()["plan"]
            same(got, want, (case, quarter, R, strength))
            assert err == denoise.sse(want, truth)
    got, err = ctx.denoise(cur, refs[:2], fields[:2], case[1], quarter, 24)
    same(got, dc.want(case, 2, 24, quarter), (case, quarter, "no truth"))
    assert err == -1
    same(dc.want(case, 2, 24, quarter), denoise.frame(cur, refs[:2], fields[:2], case[1], quarter, 24), "the shared reference is denoise.frame")


def test_outputs_stride_and_errors(native):
    """Each output alone may be NULL; a view with a row stride above W; the GME_ERR_ARG cases and the host rules in front of them."""
    import denoise
    ctx = native.default_context()
    lib, u8, i32 = ctx.lib, native._c_u8p, native._c_i32p
    case = dc.CASES[3]
    (H, W), B = case
    cur, refs, truth = dc.current(case), dc.refs(case), dc.truth(case)
    fields = [np.ascontiguousarray(f) for f in dc.fields(case, True)]
    want = dc.want(case, 3, 24, True)
    c, t = native._p(np.ascontiguousarray(cur), u8), native._p(np.ascontiguousarray(truth), u8)
    held = [np.ascontiguousarray(r) for r in refs]

    def ptrs(R, drop=None):
        return ((u8 * max(R, 1))(*[None if k == drop else native._p(held[k % 4], u8) for k in range(R)]),
                (i32 * max(R, 1))(*[native._p(fields[k % 4], i32) for k in range(R)]))

    rp, fp = ptrs(3)
    made, err = np.zeros((H, W), np.uint8), ctypes.c_int64(0)
    assert lib.gme_denoise_u8(ctx.handle, c, rp, fp, 3, H, W, W, B, 1, 24, t, native._p(made, u8), None) == 0
    same(made, want, "frame alone")
    assert lib.gme_denoise_u8(ctx.handle, c, rp, fp, 3, H, W, W, B, 1, 24, t, None, ctypes.byref(err)) == 0
    assert err.value == denoise.sse(want, truth)
    assert lib.gme_denoise_u8(ctx.handle, c, rp, fp, 3, H, W, W, B, 1, 24, None, None, ctypes.byref(err)) == 0 and err.value == -1
    assert lib.gme_denoise_u8(ctx.handle, c, rp, fp, 3, H, W, W, B, 1, 24, t, None, None) == 0
    # rows 64 bytes apart
    wide = np.full((5, H, 64), 255, np.uint8)
    for k, a in enumerate((cur, refs[0], refs[1], refs[2], truth)):
        wide[k, :, :W] = a
    got, e = ctx.denoise(wide[0, :, :W], [wide[1, :, :W], wide[2, :, :W], wide[3, :, :W]], fields[:3], B, True, 24, truth=wide[4, :, :W])
    same(got, want, "strided")
    assert e == denoise.sse(want, truth)
    # GME_ERR_ARG: R outside 1 .. 4, strength outside 1 .. 64, B outside 4 .. 64, H < B, W < B, unit not in {1, 4}, null pointers
    for R, h, w, b, unit, strength in ((0, H, W, B, 1, 24), (5, H, W, B, 1, 24), (-1, H, W, B, 1, 24), (3, H, W, B, 1, 0), (3, H, W, B, 1, 65),
                                       (3, H, W, 3, 1, 24), (3, H, W, 65, 1, 24), (3, 7, W, B, 1, 24), (3, H, 7, B, 1, 24), (3, H, W, B, 0, 24),
                                       (3, H, W, B, 2, 24), (3, H, W, B, -4, 24)):
        rp, fp = ptrs(max(R, 0))
        assert lib.gme_denoise_u8(ctx.handle, c, rp, fp, R, h, w, W, b, unit, strength, t, native._p(made, u8), None) == native.ERR_ARG, \
            (R, h, w, b, unit, strength)
    rp, fp = ptrs(3)
    assert lib.gme_denoise_u8(ctx.handle, None, rp, fp, 3, H, W, W, B, 1, 24, t, native._p(made, u8), None) == native.ERR_ARG
    assert lib.gme_denoise_u8(ctx.handle, c, None, fp, 3, H, W, W, B, 1, 24, t, native._p(made, u8), None) == native.ERR_ARG
    assert lib.gme_denoise_u8(ctx.handle, c, rp, None, 3, H, W, W, B, 1, 24, t, native._p(made, u8), None) == native.ERR_ARG
    rp, fp = ptrs(3, drop=1)
    assert lib.gme_denoise_u8(ctx.handle, c, rp, fp, 3, H, W, W, B, 1, 24, t, native._p(made, u8), None) == native.ERR_ARG
    # the host rules raise ValueError before the call
    for R in (0, 5):
        with pytest.raises(ValueError):
            ctx.denoise(cur, [refs[0]] * R, [fields[0]] * R, B)
    for strength in (0, 65):
        with pytest.raises(ValueError):
            ctx.denoise(cur, refs[:1], fields[:1], B, True, strength)
    for b in (3, 65):
        with pytest.raises(ValueError):
            ctx.denoise(cur, refs[:1], fields[:1], b)
    with pytest.raises(ValueError):
        ctx.denoise(cur[:7], [refs[0][:7]], [np.zeros((0, 6, 2), np.int32)], B)
    with pytest.raises(ValueError):
        ctx.denoise(cur, refs[:1], [fields[0][:, :-1]], B)
    with pytest.raises(ValueError):
        ctx.denoise(cur, refs[:2], fields[:1], B)
    # any int32 vector is valid, INT32_MIN included: the negation is formed in 64 bits
    wild = np.array(fields[0])
    wild[0, 0], wild[-1, -1] = (-(1 << 31), (1 << 31) - 1), ((1 << 31) - 1, -(1 << 31))
    same(ctx.denoise(cur, refs[:1], [wild], B, True, 64)[0], denoise.frame(cur, refs[:1], [wild], B, True, 64), "int32 extremes")


def test_saturated(native):
    """The target has alternating 0 / 255 columns.  References equal to it at strength 64 and R = 4: the largest tot (2880) and the
    largest numerator (255 * 2880 + 1440).  References equal to its inverse: D = 2295 and every weight is 0.  A one-pixel vector
    turns the one into the other inside the frame.  Nothing wraps."""
    import denoise
    ctx = native.default_context()
    target = np.zeros((20, 300), np.uint8)
    target[:, 1::2] = 255
    inverse = 255 - target
    zero = np.zeros((1, 18, 2), np.int32)
    one = np.zeros((1, 18, 2), np.int32)
    one[..., 0] = 1
    for refs, field in (([target] * 4, zero), ([inverse] * 4, zero), ([target] * 4, one), ([target, inverse, target, inverse], zero)):
        for strength in (1, 64):
            want = denoise.frame(target, refs, [field] * 4, 16, False, strength)
            got, err = ctx.denoise(target, refs, [field] * 4, 16, False, strength, truth=inverse)
            same(got, want, "saturated")
            assert err == denoise.sse(want, inverse)
            if field is zero:
                same(got, target, "equal or fully rejected references leave the target")
    assert denoise.window_sad(inverse, target).min() == 2295
    grey = np.full((20, 300), 128, np.uint8)
    got = ctx.denoise(target, [grey] * 4, [zero] * 4, 16, False, 64)[0]            # D = 9 * 127 or 9 * 128 >= 576: rejected
    same(got, target, "grey references")
    same(ctx.denoise(grey, [target] * 4, [zero] * 4, 16, False, 64)[0], grey, "grey target")


# ---- a resident sequence ------------------------------------------------------------------------------------------------
SEQ_ARGS = dict(block_size=8, search_window=3, procedure=0, pnorm=0)
SEQ_STRENGTH = 24
SEQ_MODES = ((1, 0), (1, 2), (2, 0), (2, 2))         # (radius, levels)


@functools.lru_cache(maxsize=None)
def seq_frames():
    """Seven frames of 40 x 72: a noise canvas seen through a window that moves by (1, 1) a frame, plus noise within +-3."""
    rng = np.random.default_rng(4072)
    canvas = rng.integers(0, 256, size=(60, 90), dtype=np.uint8)
    frames = np.stack([canvas[4 + t:44 + t, 4 + t:76 + t] for t in range(7)]).astype(np.int64)
    frames = np.clip(frames + rng.integers(-3, 4, size=frames.shape), 0, 255).astype(np.uint8)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def host_field(t, k, levels):
    """The field of target t into reference k by the host-side search of SEQ_ARGS, refined on the host where levels > 0."""
    import subpel
    from oracle import gme_oracle
    frames = seq_frames()
    mf = np.asarray(gme_oracle.get_motion_field(frames[t], frames[k], 8, 3, 0, 0), np.int32)
    return subpel.refine(frames[t], frames[k], mf, 8, 0, levels)[0] if levels else mf


@functools.lru_cache(maxsize=None)
def host_target(t, radius, levels, ends=False):
    """denoise.frame of target t with the references a clip of seven frames gives it."""
    import denoise
    frames = seq_frames()
    refs = denoise.references(t, 7, 1, radius)
    assert len(refs) == 2 * radius or ends
    out = denoise.frame(frames[t], [frames[k] for k in refs], [host_field(t, k, levels) for k in refs], 8, levels > 0, SEQ_STRENGTH)
    out.setflags(write=False)
    return out


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
h = hashlib.sha256()
for radius, levels in %(modes)r:
    for a in seq.denoise(1, 8, 3, 0, 0, radius, levels, %(strength)d):
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_sequence(native, tmp_path):
    """gme_seq_denoise at radius 1 and 2, levels 0 and 2: every target against denoise.frame built from host-side searches, `change`
    exact, ranges, split-phase mode, the kept results of a search, a refinement and a compensation byte-equal before and after,
    the argument errors, and the same bytes with two planes per launch (GME_MAX_GRID_PAIRS=2, a fresh process)."""
    import denoise
    ctx = native.default_context()
    frames = seq_frames()
    seq = native.Sequence.from_frames(ctx, frames)
    call, u8, i64 = seq.lib.gme_seq_denoise, native._c_u8p, native._c_i64p
    seq.bbme(1, 8, 3, 0, 0)
    seq.subpel(1, 8, 0, 2)
    sse_q = seq.compensate_qpel(1, 8)
    mv, qmv, comp = seq.read_mv(), seq.read_qmv(), seq.read_compensated_range(0, 6)
    h = hashlib.sha256()
    for radius, levels in SEQ_MODES:
        T = 7 - 2 * radius
        full = seq.denoise(1, radius=radius, levels=levels, strength=SEQ_STRENGTH, **SEQ_ARGS)
        assert ctx.last_bbme_info()["plan"].startswith("k_denoise R %d strength %d" % (2 * radius, SEQ_STRENGTH)), ctx.last_bbme_info()["plan"]
        assert full[0].shape == (T, 40, 72) and full[1].shape == (T,)
        for k in range(T):
            want = host_target(radius + k, radius, levels)
            same(full[0][k], want, ("gme_seq_denoise", radius, levels, k))
            assert full[1][k] == denoise.sse(want, frames[radius + k]), (radius, levels, k)
        assert full[1].min() > 0
        for a in full:
            h.update(np.ascontiguousarray(a).tobytes())
        # it keeps nothing: every kept result reads back byte-identical
        assert np.array_equal(seq.read_mv(), mv)
        for a, b in zip(seq.read_qmv(), qmv):
            assert np.array_equal(a, b)
        assert np.array_equal(seq.read_compensated_range(0, 6), comp)
        # a partial range, an empty one, ranges outside the targets
        part = seq.denoise(1, radius=radius, levels=levels, strength=SEQ_STRENGTH, first=1, count=T - 2, **SEQ_ARGS)
        assert np.array_equal(part[0], full[0][1:T - 1]) and np.array_equal(part[1], full[1][1:T - 1])
        assert all(len(a) == 0 for a in seq.denoise(1, radius=radius, levels=levels, strength=SEQ_STRENGTH, first=T, count=0, **SEQ_ARGS))
        for first, count in ((T - 1, 2), (-1, 1), (0, T + 1), (0, -1), (T + 1, 0)):
            with pytest.raises(IndexError, match="outside"):
                seq.denoise(1, radius=radius, levels=levels, strength=SEQ_STRENGTH, first=first, count=count, **SEQ_ARGS)
        # either output may be NULL
        made, change = np.zeros((T, 40, 72), np.uint8), np.zeros(T, np.int64)
        args = (seq.handle, 1, 8, 3, 0, 0, radius, levels, SEQ_STRENGTH, 0, T)
        assert call(*args, native._p(made, u8), None) == 0 and np.array_equal(made, full[0])
        assert call(*args, None, native._p(change, i64)) == 0 and np.array_equal(change, full[1])
        assert call(*args, None, None) == 0
        # also in split-phase mode the call computes and returns
        seq.set_split_phase(True)
        for a, b in zip(seq.denoise(1, radius=radius, levels=levels, strength=SEQ_STRENGTH, **SEQ_ARGS), full):
            assert np.array_equal(a, b)
        seq.set_split_phase(False)
    assert np.array_equal(seq.compensate_qpel(1, 8), sse_q)
    # GME_ERR_ARG: radius, too few frames for the distance, strength, block size, window, procedure, norm, levels
    for fd, bs, sw, sp, pn, radius, levels, strength in ((1, 8, 3, 0, 0, 0, 0, 24), (1, 8, 3, 0, 0, 3, 0, 24), (0, 8, 3, 0, 0, 1, 0, 24),
                                                        (4, 8, 3, 0, 0, 1, 0, 24), (2, 8, 3, 0, 0, 2, 0, 24), (1, 8, 3, 0, 0, 1, 0, 0),
                                                        (1, 8, 3, 0, 0, 1, 0, 65), (1, 3, 3, 0, 0, 1, 0, 24), (1, 65, 3, 0, 0, 1, 0, 24),
                                                        (1, 48, 3, 0, 0, 1, 0, 24), (1, 8, 3, 4, 0, 1, 0, 24), (1, 8, 3, 0, 2, 1, 0, 24),
                                                        (1, 8, 3, 0, 0, 1, 3, 24), (1, 8, 3, 0, 0, 1, -1, 24)):
        assert call(seq.handle, fd, bs, sw, sp, pn, radius, levels, strength, 0, 1, None, None) == native.ERR_ARG, \
            (fd, bs, sw, sp, pn, radius, levels, strength)
    assert call(seq.handle, 3, 8, 3, 0, 0, 1, 0, 24, 0, 1, None, None) == 0           # seven frames are just enough
    assert call(None, 1, 8, 3, 0, 0, 1, 0, 24, 0, 1, None, None) == native.ERR_ARG
    for radius in (0, 3):
        with pytest.raises(ValueError):
            seq.denoise(1, radius=radius, **SEQ_ARGS)
    for strength in (0, 65):
        with pytest.raises(ValueError):
            seq.denoise(1, strength=strength, **SEQ_ARGS)
    for bs in (3, 65, 48):
        with pytest.raises(ValueError):
            seq.denoise(1, bs)
    seq.close()
    np.save(tmp_path / "frames.npy", frames)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd"), "modes": SEQ_MODES, "strength": SEQ_STRENGTH})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy")], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


@pytest.mark.parametrize("radius,levels", SEQ_MODES)
def test_clip(native, radius, levels):
    """denoise.clip on the sequence: the ends, which use the references that exist, included; each frame against the host
    composition."""
    import denoise
    frames = seq_frames()
    got = denoise.clip(frames, 1, 8, 3, 0, 0, radius, levels, SEQ_STRENGTH)
    assert got.shape == frames.shape and got.dtype == np.uint8
    for t in range(7):
        same(got[t], host_target(t, radius, levels, ends=True), ("denoise.clip", radius, levels, t))


def test_cli_denoise(native, golden, tmp_path, capsys):
    import denoise
    import gme_cli
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(5):
        Image.fromarray(np.ascontiguousarray(g9[10 + k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["denoise", "-p", str(d), "-o", str(tmp_path / "out"), "--noise", "10", "--seed", "3"])
    out = capsys.readouterr().out
    assert "5 frames of" in out and "psnr against the clean clip: noisy " in out and "filtered " in out
    print("psnr noisy %.4f dB, filtered %.4f dB" % (res["psnr_noisy"], res["psnr_filtered"]))
    assert res["psnr_filtered"] > res["psnr_noisy"]
    clean = np.stack([np.ascontiguousarray(g9[10 + k]) for k in range(5)])
    rng = np.random.default_rng(3)
    noisy = np.clip(np.rint(clean + rng.normal(scale=10.0, size=clean.shape)), 0, 255).astype(np.uint8)
    assert np.array_equal(res["noisy"], noisy)
    rec = json.loads((tmp_path / "out" / "denoise.json").read_text())
    assert rec["frames"] == 5 and rec["shape"] == list(clean.shape[1:])
    assert rec["options"]["strength"] == 24 and rec["options"]["radius"] == 1 and rec["options"]["noise"] == 10.0 and rec["options"]["seed"] == 3
    assert rec["change"] == [denoise.sse(a, b) for a, b in zip(res["frames"], noisy)]
    assert rec["sse_noisy"] == [denoise.sse(a, b) for a, b in zip(noisy, clean)]
    assert rec["sse_filtered"] == [denoise.sse(a, b) for a, b in zip(res["frames"], clean)]
    assert rec["psnr_noisy"] == res["psnr_noisy"] and rec["psnr_filtered"] == res["psnr_filtered"]
    assert sum(rec["sse_filtered"]) < sum(rec["sse_noisy"])
    for k in range(5):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "denoised" / ("%04d.png" % k))), res["frames"][k])
    # without --noise there is no PSNR to report
    res = gme_cli.main(["denoise", "-p", str(d), "-o", str(tmp_path / "plain"), "-sp", "3", "--radius", "2", "--subpel", "2", "--strength", "8"])
    out = capsys.readouterr().out
    assert "psnr against" not in out and "strength 8, radius 2" in out and "psnr_noisy" not in res
    assert np.array_equal(res["frames"], denoise.clip(clean, 1, 16, 8, 3, 0, 2, 2, 8))
    gme_cli.main(["info"])
    assert "temporal denoising" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_denoise.remarks, as the compiler wrote them: the kernel does not spill and uses no scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_denoise.hip"]
    assert [r["name"].replace(" ", "") for r in rows] == ["k_denoise"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
