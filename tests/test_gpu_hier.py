"""Hierarchical block matching on the device (k_hier of bbme_hier.hip through gme_hier_u8, gme_seq_hier and gme_seq_read_hier)
against the host definition hier.py fed the device's own pyramids: byte for byte at every level on noise, ties, saturated
content, known shifts, a batched sequence and real frames, plus the composition with the quarter-pel calls, the error paths and
the CLI.  Needs an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hier_cases as hc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def instance(bs, levels):
    return "k_hier<%d,3>" % bs if levels == 3 and bs in (16, 32, 64) else "k_hier<0,0>"


def check_sequence(native, frames, fd, bs, cw, r, pnorm, levels):
    """gme_seq_hier over a resident sequence: every level's field and cost of every pair against hier.search on the pyramid
    read back from the sequence; the level-2 field is the sequence's motion field.  -> (fields, costs) of the device."""
    import hier
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(frames))
    seq.hier(fd, bs, cw, r, pnorm, levels)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs, levels) + " "), ctx.last_bbme_info()["plan"]
    pyr = [[seq.read_frame(k, l) for l in range(3)] for k in range(len(frames))]
    got = {l: seq.read_hier(l) for l in range(3 - levels, 3)}
    mv = seq.read_mv()
    for l in range(3 - levels):
        with pytest.raises(IndexError, match="level"):
            seq.read_hier(l)
    seq.close()
    assert np.array_equal(mv, got[2][0])
    for k in range(len(frames) - fd):
        assert np.array_equal(pyr[k][2], frames[k])
        want_f, want_c = hier.search(pyr[k], pyr[k + fd], bs, cw, r, pnorm, levels)
        for l in want_f:
            f, c = got[l][0][k], got[l][1][k]
            assert f.dtype == np.int32 and c.dtype == np.int64
            assert np.array_equal(c, want_c[l]), (k, l, bs, pnorm, np.argwhere(c != want_c[l])[:4])
            assert np.array_equal(f, want_f[l]), (k, l, bs, pnorm, np.argwhere(np.any(f != want_f[l], axis=2))[:4])
    return {l: got[l][0] for l in got}, {l: got[l][1] for l in got}


def check_pair(native, prev, cur, bs, cw, r, pnorm, levels):
    """gme_hier_u8 on host buffers against hier.search on the pyramids of ctx.pyrdown."""
    import hier
    ctx = native.default_context()
    field, cost = ctx.hier(prev, cur, bs, cw, r, pnorm, levels)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs, levels) + " ")
    pyrs = []
    for f in (prev, cur):
        l1 = ctx.pyrdown(f)
        pyrs.append([ctx.pyrdown(l1), l1, f])
    want_f, want_c = hier.search(pyrs[0], pyrs[1], bs, cw, r, pnorm, levels)
    assert np.array_equal(cost, want_c[2]) and np.array_equal(field, want_f[2]), (bs, pnorm, levels)
    return field, cost


NOISE = [((37, 53), 4, 1, 8, 0), ((37, 53), 4, 1, 0, 3), ((37, 53), 8, 2, 8, 1), ((37, 53), 8, 2, 3, 3), ((37, 53), 12, 2, 8, 1),
         ((48, 80), 16, 3, 8, 1), ((48, 80), 16, 3, 3, 0), ((70, 101), 16, 3, 8, 3), ((70, 101), 32, 3, 8, 1),
         ((70, 101), 32, 3, 0, 3), ((70, 101), 24, 3, 3, 1), ((130, 135), 64, 3, 8, 3), ((130, 135), 64, 3, 0, 0)]


@pytest.mark.parametrize("shape,bs,levels,cw,r", NOISE)
def test_noise(native, shape, bs, levels, cw, r):
    """Frame sizes that are no multiple of the block size (48 x 80 at bs 16 is: its last blocks touch the last row and column),
    odd level sizes, the compiled instances (16, 32, 64 at three levels) and the run-time one; blocks start at the frame edge,
    so many candidates fall outside."""
    rng = np.random.default_rng(100 + bs + cw)
    frames = rng.integers(0, 256, size=(2,) + shape, dtype=np.uint8)
    for pnorm in (0, 1):
        check_sequence(native, frames, 1, bs, cw, r, pnorm, levels)
        check_pair(native, frames[0], frames[1], bs, cw, r, pnorm, levels)


def test_clamp(native):
    """The noise pair of tests/test_hier_host.py::test_clamp (37 x 53, level sizes 19 x 27 and 10 x 14, bs 8 at two levels): the
    device equals the host, where at MAE a doubled parent vector points outside its level and is clamped."""
    rng = np.random.default_rng(37)
    frames = rng.integers(0, 256, size=(2, 37, 53), dtype=np.uint8)
    for pnorm in (0, 1):
        fields, _ = check_sequence(native, frames, 1, 8, 8, 1, pnorm, 2)
        if pnorm == 0:
            assert hc.clamped_blocks({l: f[0] for l, f in fields.items()}, hc.level_shapes(37, 53), 8) > 0


def test_ties(native):
    """Constant frames (the centre wins every tie: the zero field at every level) and vertical stripes of period 2 against the
    same stripes one column on (many zero costs: the first in the definition's order wins), bs 8 and 16, both norms."""
    flat = np.stack([np.full((37, 53), 90, np.uint8), np.full((37, 53), 97, np.uint8)])
    stripes = np.tile(np.array([0, 255], np.uint8), (37, 27))[:, :53]
    stripes = np.stack([stripes, 255 - stripes])
    for frames in (flat, stripes):
        for bs, levels in ((8, 2), (16, 3), (8, 1), (16, 1)):
            for pnorm in (0, 1):
                fields, costs = check_sequence(native, frames, 1, bs, 8, 1, pnorm, levels)
                if frames is flat:
                    assert all(not f.any() for f in fields.values())
                elif levels == 1:
                    assert not costs[2].any() and tuple(fields[2][0, 1, 1]) == (-7, -8)


def test_saturated(native):
    """previous all 0, current all 255 at bs 64: every level-2 cost is the largest there is, 64 * 64 * 255^2 at MSE, and the
    centre wins everywhere."""
    frames = np.stack([np.zeros((130, 135), np.uint8), np.full((130, 135), 255, np.uint8)])
    for pnorm, top in ((1, 266342400), (0, 64 * 64 * 255)):
        fields, costs = check_sequence(native, frames, 1, 64, 8, 3, pnorm, 3)
        assert np.all(costs[2] == top) and not fields[2].any()
        field, cost = check_pair(native, frames[0], frames[1], 64, 8, 3, pnorm, 3)
        assert np.all(cost == top) and not field.any()


@pytest.mark.parametrize("bs", [16, 32])
def test_known_shifts(native, bs):
    """The 96 x 128 frames of tests/test_hier_host.py on the device: equal to the host, hence every interior block finds the
    shift, (-18, 7) beyond an exhaustive window of 16 included."""
    for shift in hc.SHIFTS:
        prev, cur = hc.pair(96, 128, shift)
        for pnorm in (0, 1):
            fields, _ = check_sequence(native, np.stack([prev, cur]), 1, bs, 4, 1, pnorm, 3)
            assert hc.interior_hits(fields[2][0], shift, bs) >= 1.0 - 0.05


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
h = hashlib.sha256()
for fd in (1, 3):
    seq.hier(fd, 8, 8, 1, 0, 2)
    for level in (1, 2):
        for a in seq.read_hier(level):
            h.update(np.ascontiguousarray(a).tobytes())
    seq.subpel(fd, 8, 0, 2)
    for a in seq.read_qmv():
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_batched(native, tmp_path):
    """Seven frames of 40 x 72, frame distances 1 and 3, bs 8 at two levels: every pair against the host, a partial read against
    the full one, the same bytes with two pairs per launch (GME_MAX_GRID_PAIRS=2, a fresh process), the quarter-pel chain on
    the field, and the call-order and argument errors."""
    import subpel
    rng = np.random.default_rng(72)
    frames = rng.integers(0, 256, size=(7, 40, 72), dtype=np.uint8)
    for fd in (1, 3):
        fields, _ = check_sequence(native, frames, fd, 8, 8, 1, 0, 2)
        assert len(fields[2]) == 7 - fd
    seq = native.Sequence.from_frames(native.default_context(), frames)
    with pytest.raises(native.GmeError, match="before gme_seq_hier"):
        seq.read_hier(2)
    h = hashlib.sha256()
    for fd in (1, 3):
        seq.bbme(fd, 8, 3, 0, 0)
        seq.subpel(fd, 8, 0, 2)
        seq.hier(fd, 8, 8, 1, 0, 2)
        with pytest.raises(native.GmeError, match="before gme_seq_subpel"):          # the earlier quarter-pel result is gone
            seq.read_qmv()
        full = {level: seq.read_hier(level) for level in (1, 2)}
        for level in (1, 2):
            f12, c12 = seq.read_hier(level, 1, 2)
            assert np.array_equal(f12, full[level][0][1:3]) and np.array_equal(c12, full[level][1][1:3])
            for a in full[level]:
                h.update(np.ascontiguousarray(a).tobytes())
        mv = seq.read_mv()
        assert np.array_equal(mv, full[2][0]) and np.array_equal(seq.read_mv(1, 2), mv[1:3])
        with pytest.raises(IndexError, match="level"):
            seq.read_hier(0)
        with pytest.raises(IndexError, match="level"):
            seq.read_hier(3)
        with pytest.raises(IndexError, match="outside"):
            seq.read_hier(2, 7 - fd - 1, 2)
        with pytest.raises(native.GmeError, match="block size"):
            seq.subpel(fd, 4, 0)
        seq.subpel(fd, 8, 0, 2)
        q, qc = seq.read_qmv()
        for k in range(7 - fd):
            want_q, want_c = subpel.refine(frames[k], frames[k + fd], mv[k], 8, 0, 2)
            assert np.array_equal(q[k], want_q) and np.array_equal(qc[k], want_c)
        sse = seq.compensate_qpel(fd, 8)
        comp = seq.read_compensated_range(0, 7 - fd)
        assert all(sse[k] == subpel.sse(frames[k + fd], comp[k]) for k in range(7 - fd))
        for a in (q, qc):
            h.update(np.ascontiguousarray(a).tobytes())
    # what ends the validity of the levels: another block-matching call, new frame data
    seq.bbme(1, 8, 3, 0, 0)
    with pytest.raises(native.GmeError, match="before gme_seq_hier"):
        seq.read_hier(2)
    seq.hier(1, 8, 8, 1, 0, 2)
    seq.read_hier(1)
    seq.upload(0, frames[:1])
    with pytest.raises(native.GmeError, match="before gme_seq_hier"):
        seq.read_hier(2)
    # arguments: the host rules raise ValueError, the library's own checks GME_ERR_ARG
    for args in ((1, 8, 8, 1, 0, 3), (1, 6, 8, 1, 0, 2), (1, 16, 9, 1, 0, 3), (1, 16, 8, 4, 0, 3), (1, 16, 8, 1, 0, 0), (1, 68, 8, 1, 0, 3)):
        with pytest.raises(ValueError):
            seq.hier(*args)
        assert seq.lib.gme_seq_hier(seq.handle, *args) == native.ERR_ARG
        p = np.zeros((40, 72), np.uint8)
        mf = np.zeros((40 // args[1], 72 // args[1], 2), np.int32)
        assert seq.lib.gme_hier_u8(seq.ctx.handle, native._p(p, native._c_u8p), native._p(p, native._c_u8p), 40, 72, 72, *args[1:],
                                   native._p(mf, native._c_i32p), None) == native.ERR_ARG
    with pytest.raises(IndexError, match="frame_distance"):
        seq.hier(7, 8, 8, 1, 0, 2)
    field, _ = native.default_context().hier(frames[0], frames[1], 8, 8, 1, 0, 2)
    mf = np.zeros_like(field)
    assert seq.lib.gme_hier_u8(seq.ctx.handle, native._p(frames[0], native._c_u8p), native._p(frames[1], native._c_u8p), 40, 72, 72,
                               8, 8, 1, 0, 2, native._p(mf, native._c_i32p), None) == 0          # cost_out may be NULL
    assert np.array_equal(mf, field)
    seq.close()
    np.save(tmp_path / "frames.npy", frames)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd")})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy")], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


def test_sharded_lanes(native):
    """ShardedSequence.motion_fields_hier: two lanes give what one gives, and what a plain sequence gives."""
    import sequence
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(6, 40, 72), dtype=np.uint8)
    got = []
    for streams in (1, 2):
        sh = sequence.ShardedSequence(40, 72, 6, 1, streams=streams)
        sh.load(frames)
        got.append(sh.motion_fields_hier(8, 8, 1, 1, 1, levels=2))
        with pytest.raises(ValueError):
            sh.motion_fields_hier(8, 8, 1, 1, 2)
        sh.close()
    assert got[0][0].shape == (5, 5, 9, 2) and got[0][1].shape == (5, 5, 9)
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    seq = native.Sequence.from_frames(native.default_context(), frames)
    seq.hier(1, 8, 8, 1, 1, 2)
    assert np.array_equal(seq.read_mv(), got[0][0])
    seq.close()


def test_real_frames(native, golden):
    """Three pairs of g9 (the pan240 clip), bs 16: device equal to host at every level, and the PSNR of the compensation next
    to that of the exhaustive search at window 16 and of the diamond search on the same pairs (DESIGN.md section 7f records the
    figures; nothing is asserted about them, the search is a heuristic)."""
    import sequence
    g9 = np.ascontiguousarray(golden("g9_pan240seq")["frames"][:4])
    H, W = g9.shape[1:]
    ctx = native.default_context()

    def psnr(mf):
        return sequence.psnr_from_sse(np.array([ctx.sse(g9[k + 1], ctx.compensate(g9[k], mf[k])) for k in range(3)]), H, W)
    for pnorm in (0, 1):
        fields, _ = check_sequence(native, g9, 1, 16, 8, 1, pnorm, 3)
        seq = native.Sequence.from_frames(ctx, g9)
        others = []
        for procedure in (0, 3):
            seq.bbme(1, 16, 16, procedure, pnorm)
            others.append(psnr(seq.read_mv()))
        seq.close()
        p_h = psnr(fields[2])
        for k in range(3):
            print("g9 pair %d norm %d: psnr hierarchical %.4f dB, exhaustive sw 16 %.4f dB, diamond %.4f dB, median vector (%g, %g)"
                  % (k, pnorm, p_h[k], others[0][k], others[1][k], np.median(fields[2][k, :, :, 0]), np.median(fields[2][k, :, :, 1])))


def test_cli_hier(native, golden, tmp_path, capsys):
    import gme_cli
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(3):
        Image.fromarray(np.ascontiguousarray(g9[k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["hier", "-p", str(d), "-fi", "2", "-fd", "2", "--subpel", "2", "-o", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "reach: +-35 px" in out and "median vector" in out and "psnr: " in out and "psnr quarter-pel" in out
    rec = json.loads((tmp_path / "out" / "hier.json").read_text())
    assert set(rec) >= {"reach", "median_vector", "sse", "psnr", "sse_qpel", "psnr_qpel", "options", "shape"}
    assert rec["reach"] == 35 and rec["shape"] == list(res["field"].shape[:2])
    assert rec["median_vector"] == [float(np.median(res["field"][:, :, 0])), float(np.median(res["field"][:, :, 1]))]
    assert np.array_equal(res["qfield"] >> 2, res["field"]) or rec["psnr_qpel"] > 0
    gme_cli.main(["hier", "-p", str(d), "-fi", "1", "-bs", "8", "--levels", "2", "-cw", "4", "-r", "2", "-pn", "1"])
    out = capsys.readouterr().out
    assert "reach: +-10 px" in out and "psnr quarter-pel" not in out
    gme_cli.main(["info"])
    assert "hierarchical search" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_hier.remarks, as the compiler wrote them: no instance of the kernel spills or uses scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_hier.hip"]
    assert sorted(r["name"].replace(" ", "") for r in rows) == ["k_hier<0,0>", "k_hier<16,3>", "k_hier<32,3>", "k_hier<64,3>"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
