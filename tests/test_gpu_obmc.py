"""Overlapped block motion compensation on the device (k_obmc of bbme_obmc.hip through gme_obmc_u8 and gme_seq_obmc) against the
host definition obmc.py: byte for byte on the cases of obmc_cases with both units, strided input, saturated content, a resident
sequence with its lifetimes, the fields of the other searches, the error paths and the CLI.  Needs an MI355X."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import obmc_cases as oc

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


@pytest.mark.parametrize("quarter", oc.UNITS)
@pytest.mark.parametrize("case", oc.CASES, ids=oc.case_id)
def test_cases(native, case, quarter):
    """gme_obmc_u8 byte-equal to obmc.compensate, the squared error against a noise frame exact, -1 without one."""
    import obmc
    ctx = native.default_context()
    previous, current = oc.frames(case)
    want = oc.want(case, quarter)
    got, err = ctx.obmc(previous, oc.field(case, quarter), case[1], quarter, cur=current)
    assert ctx.last_bbme_info()["plan"].startswith("k_obmc "), ctx.last_bbme_info()["plan"]
    same(got, want, (case, quarter))
    assert err == obmc.sse(want, current)
    got, err = ctx.obmc(previous, oc.field(case, quarter), case[1], quarter)
    same(got, want, (case, quarter, "no current"))
    assert err == -1


def test_outputs_stride_and_errors(native):
    """Each output alone may be NULL; a view with a row stride above W; the GME_ERR_ARG cases and the host rules in front of them."""
    import obmc
    ctx = native.default_context()
    lib, u8, i32 = ctx.lib, native._c_u8p, native._c_i32p
    case = oc.CASES[2]
    (H, W), B = case
    previous, current = oc.frames(case)
    f, want = np.ascontiguousarray(oc.field(case, True)), oc.want(case, True)
    p, c = native._p(np.ascontiguousarray(previous), u8), native._p(np.ascontiguousarray(current), u8)
    made, err = np.zeros((H, W), np.uint8), ctypes.c_int64(0)
    assert lib.gme_obmc_u8(ctx.handle, p, c, H, W, W, B, native._p(f, i32), 1, native._p(made, u8), None) == 0
    same(made, want, "frame alone")
    assert lib.gme_obmc_u8(ctx.handle, p, c, H, W, W, B, native._p(f, i32), 1, None, ctypes.byref(err)) == 0
    assert err.value == obmc.sse(want, current)
    assert lib.gme_obmc_u8(ctx.handle, p, None, H, W, W, B, native._p(f, i32), 1, None, ctypes.byref(err)) == 0 and err.value == -1
    assert lib.gme_obmc_u8(ctx.handle, p, c, H, W, W, B, native._p(f, i32), 1, None, None) == 0
    # rows 64 bytes apart
    wide = np.zeros((2, H, 64), np.uint8)
    wide[0, :, :W], wide[1, :, :W] = previous, current
    wide[:, :, W:] = 255
    got, e = ctx.obmc(wide[0, :, :W], f, B, True, cur=wide[1, :, :W])
    same(got, want, "strided")
    assert e == obmc.sse(want, current)
    # GME_ERR_ARG: null prev or field, B outside 4 .. 64, H < B, W < B, unit not in {1, 4}
    bad = ((None, native._p(f, i32), H, W, B, 1), (p, None, H, W, B, 1), (p, native._p(f, i32), H, W, 3, 1), (p, native._p(f, i32), H, W, 65, 1),
           (p, native._p(f, i32), 7, W, B, 1), (p, native._p(f, i32), H, 7, B, 1), (p, native._p(f, i32), H, W, B, 0),
           (p, native._p(f, i32), H, W, B, 2), (p, native._p(f, i32), H, W, B, -4))
    for pp, ff, h, w, b, unit in bad:
        assert lib.gme_obmc_u8(ctx.handle, pp, c, h, w, W, b, ff, unit, native._p(made, u8), None) == native.ERR_ARG, (h, w, b, unit)
    # the host rules raise ValueError before the call
    for b in (3, 65):
        with pytest.raises(ValueError):
            ctx.obmc(previous, f, b)
    with pytest.raises(ValueError):
        ctx.obmc(previous[:7], np.zeros((0, 6, 2), np.int32), B)
    with pytest.raises(ValueError):
        ctx.obmc(previous, f[:, :-1], B)
    whole = np.zeros_like(f)
    whole[1, 1, 0] = (1 << 29) + 1
    with pytest.raises(ValueError):
        ctx.obmc(previous, whole, B, quarter=False)
    whole[1, 1, 0] = -(1 << 29) - 1
    with pytest.raises(ValueError):
        ctx.obmc(previous, whole, B, quarter=False)
    same(ctx.obmc(previous, whole, B, quarter=True)[0], obmc.compensate(previous, whole, B), "the quarter field is unrestricted")
    same(obmc.frame(previous, f, B), want, "obmc.frame")
    # the C ABI itself takes any int32 at unit 4 too: the product is formed in 64 bits
    whole = np.array(oc.field(case, False))
    whole[0, 0], whole[-1, -1], whole[0, -1] = (oc.INT32_MIN, oc.INT32_MAX), (oc.INT32_MAX, oc.INT32_MIN), (oc.INT32_MAX, oc.INT32_MAX)
    assert lib.gme_obmc_u8(ctx.handle, p, c, H, W, W, B, native._p(whole, i32), 4, native._p(made, u8), None) == 0
    same(made, obmc.compensate(previous, whole, B, quarter=False), "int32 extremes in whole pixels")


def test_saturated(native):
    """`previous` alternating 0 / 255 columns at B = 64 with quarter vectors: predictions of 0 and 255 side by side under every
    weight, the largest numerators there are (255 * 4 * 64^2 + 2 * 64^2).  Nothing wraps."""
    import obmc
    ctx = native.default_context()
    previous = np.zeros((130, 200), np.uint8)
    previous[:, 1::2] = 255
    rng = np.random.default_rng(64)
    f = rng.integers(-40, 41, size=(2, 3, 2)).astype(np.int32)
    for field in (f, np.zeros_like(f), np.full_like(f, 4)):
        want = obmc.compensate(previous, field, 64)
        got, err = ctx.obmc(previous, field, 64, cur=previous)
        same(got, want, "saturated")
        assert err == obmc.sse(want, previous)
    assert want.max() == 255 and want.min() == 0
    white = np.full((64, 64), 255, np.uint8)
    same(ctx.obmc(white, np.array([[[7, -9]]], np.int32), 64)[0], white, "all 255")


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
seq.bbme(1, 8, 3, 0, 0)
seq.subpel(1, 8, 0, 2)
h = hashlib.sha256()
for quarter in (False, True):
    for a in seq.obmc(1, 8, quarter):
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_sequence(native, tmp_path):
    """Six noise frames of 40 x 72, bbme(1, 8, ...) then subpel, at unit 4 and 1: every pair against the host, the kept results
    byte-equal before and after, ranges, split-phase mode, the states that refuse, and the same bytes with two pairs per launch
    (GME_MAX_GRID_PAIRS=2, a fresh process)."""
    import obmc
    ctx = native.default_context()
    rng = np.random.default_rng(4072)
    frames = rng.integers(0, 256, size=(6, 40, 72), dtype=np.uint8)
    seq = native.Sequence.from_frames(ctx, frames)
    call, u8, i64 = seq.lib.gme_seq_obmc, native._c_u8p, native._c_i64p
    # before any search there is no field
    for unit in (4, 1):
        assert call(seq.handle, 1, 8, unit, 0, 1, None, None) == native.ERR_STATE
    with pytest.raises(native.GmeError):
        seq.obmc(1, 8)
    seq.bbme(1, 8, 3, 0, 0)
    assert call(seq.handle, 1, 8, 1, 0, 1, None, None) == native.ERR_STATE          # unit 1 before subpel
    seq.subpel(1, 8, 0, 2)
    sse_q = seq.compensate_qpel(1, 8)
    mv, qmv, comp = seq.read_mv(), seq.read_qmv(), seq.read_compensated_range(0, 5)
    h = hashlib.sha256()
    full = {}
    for quarter in (False, True):
        field = qmv[0] if quarter else mv
        full[quarter] = seq.obmc(1, 8, quarter)
        assert ctx.last_bbme_info()["plan"].startswith("k_obmc "), ctx.last_bbme_info()["plan"]
        assert full[quarter][0].shape == (5, 40, 72) and full[quarter][1].shape == (5,)
        for k in range(5):
            want = obmc.compensate(frames[k], field[k], 8, quarter)
            same(full[quarter][0][k], want, ("gme_seq_obmc", quarter, k))
            assert full[quarter][1][k] == obmc.sse(want, frames[k + 1]), (quarter, k)
        for a in full[quarter]:
            h.update(np.ascontiguousarray(a).tobytes())
        # it keeps nothing: every kept result reads back byte-identical
        assert np.array_equal(seq.read_mv(), mv)
        for a, b in zip(seq.read_qmv(), qmv):
            assert np.array_equal(a, b)
        assert np.array_equal(seq.read_compensated_range(0, 5), comp)
        # a partial range, an empty one, ranges outside the pairs
        part = seq.obmc(1, 8, quarter, 1, 3)
        assert np.array_equal(part[0], full[quarter][0][1:4]) and np.array_equal(part[1], full[quarter][1][1:4])
        assert all(len(a) == 0 for a in seq.obmc(1, 8, quarter, 5, 0))
        for first, count in ((4, 2), (-1, 1), (0, 6), (0, -1)):
            with pytest.raises(IndexError, match="outside"):
                seq.obmc(1, 8, quarter, first, count)
        # either output may be NULL
        made, err = np.zeros((5, 40, 72), np.uint8), np.zeros(5, np.int64)
        unit = 1 if quarter else 4
        assert call(seq.handle, 1, 8, unit, 0, 5, native._p(made, u8), None) == 0 and np.array_equal(made, full[quarter][0])
        assert call(seq.handle, 1, 8, unit, 0, 5, None, native._p(err, i64)) == 0 and np.array_equal(err, full[quarter][1])
        assert call(seq.handle, 1, 8, unit, 0, 5, None, None) == 0
        # also in split-phase mode the call computes and returns
        seq.set_split_phase(True)
        for a, b in zip(seq.obmc(1, 8, quarter), full[quarter]):
            assert np.array_equal(a, b)
        seq.set_split_phase(False)
    assert np.array_equal(seq.compensate_qpel(1, 8), sse_q)
    # another block size or distance than the field's, and the arguments
    for fd, bs in ((2, 8), (1, 16), (1, 4)):
        for unit in (4, 1):
            assert call(seq.handle, fd, bs, unit, 0, 1, None, None) == native.ERR_STATE, (fd, bs, unit)
    for fd, bs, unit in ((0, 8, 4), (6, 8, 4), (1, 3, 4), (1, 65, 4), (1, 48, 4), (1, 8, 0), (1, 8, 2)):
        assert call(seq.handle, fd, bs, unit, 0, 1, None, None) == native.ERR_ARG, (fd, bs, unit)
    for bs in (3, 65, 48):
        with pytest.raises(ValueError):
            seq.obmc(1, bs)
    # new frame data: the quarter-pel field is gone, the motion field stays as a prior and is applied to the frames that are there
    seq.invalidate_pyramids()                                       # gme_seq_invalidate
    assert call(seq.handle, 1, 8, 1, 0, 1, None, None) == native.ERR_STATE
    for a, b in zip(seq.obmc(1, 8), full[False]):
        assert np.array_equal(a, b)
    other = rng.integers(0, 256, size=(6, 40, 72), dtype=np.uint8)
    seq.upload(0, other)
    assert call(seq.handle, 1, 8, 1, 0, 1, None, None) == native.ERR_STATE
    made, err = seq.obmc(1, 8)
    for k in range(5):
        want = obmc.compensate(other[k], mv[k], 8, quarter=False)
        same(made[k], want, ("after invalidate", k))
        assert err[k] == obmc.sse(want, other[k + 1])
    seq.close()
    np.save(tmp_path / "frames.npy", frames)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd")})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy")], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


def test_fields_of_other_searches(native):
    """The fields of gme_seq_hier and gme_seq_prop as the sequence's field, one pair each, whole pixels and refined."""
    import obmc
    ctx = native.default_context()
    frames = np.random.default_rng(5).integers(0, 256, size=(3, 48, 80), dtype=np.uint8)
    seq = native.Sequence.from_frames(ctx, frames)
    for search in (lambda: seq.hier(1, 16, 4, 1, 0, 3), lambda: (seq.bbme(1, 16, 4, 3, 0), seq.prop(1, 16, 0, 1, 1))):
        search()
        mv = seq.read_mv()
        made, err = seq.obmc(1, 16, False, 1, 1)
        want = obmc.compensate(frames[1], mv[1], 16, quarter=False)
        same(made[0], want, "integer field")
        assert err[0] == obmc.sse(want, frames[2])
        seq.subpel(1, 16, 0, 2)
        qmv = seq.read_qmv()[0]
        made, err = seq.obmc(1, 16, True, 0, 1)
        want = obmc.compensate(frames[0], qmv[0], 16)
        same(made[0], want, "refined field")
        assert err[0] == obmc.sse(want, frames[1])
    seq.close()


def test_cli_obmc(native, golden, tmp_path, capsys):
    import gme_cli
    import obmc
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(5):
        Image.fromarray(np.ascontiguousarray(g9[10 + k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["obmc", "-p", str(d), "-fi", "2", "-sp", "3", "--subpel", "2", "-o", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "blocks of 16" in out and "psnr integer field: plain " in out and "psnr refined field: plain " in out and "overlapped " in out
    rec = json.loads((tmp_path / "out" / "obmc.json").read_text())
    assert set(rec) >= {"integer", "qpel", "options", "shape"} and rec["shape"] == list(res["mf"].shape[:2])
    for key in ("integer", "qpel"):
        assert set(rec[key]) >= {"sse_plain", "sse_obmc", "psnr_plain", "psnr_obmc"}
    assert rec["options"]["subpel"] == 2 and rec["options"]["block_size"] == 16
    want = obmc.compensate(g9[11], res["qfield"], 16)
    assert rec["qpel"]["sse_obmc"] == obmc.sse(want, g9[12])
    assert rec["integer"]["sse_obmc"] == obmc.sse(obmc.compensate(g9[11], res["mf"], 16, quarter=False), g9[12])
    assert rec["qpel"]["sse_obmc"] < rec["qpel"]["sse_plain"] and rec["integer"]["sse_obmc"] < rec["integer"]["sse_plain"]
    assert np.array_equal(res["frame"], want)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "obmc.png")), want)
    res = gme_cli.main(["obmc", "-p", str(d), "-fi", "1", "-bs", "32", "--hier"])
    out = capsys.readouterr().out
    assert "blocks of 32" in out and "psnr integer field: plain " in out and "refined" not in out
    assert np.array_equal(res["frame"], obmc.compensate(g9[10], res["mf"], 32, quarter=False))
    with pytest.raises(IndexError):
        gme_cli.main(["obmc", "-p", str(d), "-fi", "5"])
    gme_cli.main(["info"])
    assert "overlapped block" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_obmc.remarks, as the compiler wrote them: the kernel does not spill and uses no scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_obmc.hip"]
    assert [r["name"].replace(" ", "") for r in rows] == ["k_obmc"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
