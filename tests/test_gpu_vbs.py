"""Variable-block-size motion on the device (k_vbs and k_compensate_vbs of bbme_vbs.hip through gme_vbs_u8, gme_seq_vbs,
gme_seq_read_vbs and gme_seq_compensate_vbs) against the host definition vbs.py and subpel.compensate_integer: byte for byte on
noise with arbitrary input fields, ties, saturated content, the two-motion scene, a batched sequence and real frames, plus the
error paths, the sharded lanes and the CLI.  Needs an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vbs_cases as vc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def instance(bs, depth):
    return "k_vbs<%d,2>" % bs if depth == 2 and bs in (16, 32) else "k_vbs<0,0>"


def same(got, want, what):
    for name, g, w in zip(("leaf", "depth", "cost"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4])


def check_pair(native, prev, cur, mf, bs, D, r, pnorm, penalty, want=None):
    """gme_vbs_u8 on host buffers with the field ``mf`` against vbs.tree (``want``: its result where a test has it already)
    -> the host's result."""
    import vbs
    ctx = native.default_context()
    if want is None:
        want = vbs.tree(prev, cur, mf, bs, D, r, pnorm, penalty)
    got = ctx.vbs(prev, cur, mf, bs, D, r, pnorm, penalty)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs, D) + " "), ctx.last_bbme_info()["plan"]
    same(got, want, ("gme_vbs_u8", prev.shape, bs, D, r, pnorm, penalty))
    return want


def check_sequence(native, frames, fd, bs, D, r, pnorm, penalty, search):
    """gme_seq_vbs over a resident sequence after ``search(seq)``: every pair against vbs.tree on the sequence's own motion
    field, which the call leaves as it was; the compensated frames and their SSE against subpel.compensate_integer at the leaf
    size -> (leaf, depth, cost, sse) of the device."""
    import subpel
    import vbs
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(frames))
    search(seq)
    mv = seq.read_mv()
    seq.vbs(fd, bs, D, r, pnorm, penalty)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs, D) + " "), ctx.last_bbme_info()["plan"]
    got = seq.read_vbs()
    assert np.array_equal(seq.read_mv(), mv)
    sse = seq.compensate_vbs(fd, bs)
    comp = seq.read_compensated_range(0, len(frames) - fd)
    seq.close()
    for k in range(len(frames) - fd):
        want = vbs.tree(frames[k], frames[k + fd], mv[k], bs, D, r, pnorm, penalty)
        same([a[k] for a in got], want, ("gme_seq_vbs", k, bs, D, r, pnorm))
        want_comp = subpel.compensate_integer(frames[k], want[0], bs >> D)
        assert np.array_equal(comp[k], want_comp), (k, np.argwhere(comp[k] != want_comp)[:4])
        assert sse[k] == subpel.sse(frames[k + fd], want_comp)
    return got + (sse,)


@pytest.mark.parametrize("case", vc.NOISE)
def test_noise(native, case):
    """Noise pairs of sizes that are no multiple of the root, with a random input field whose vectors lie in [-6, 6] (some
    roots point outside, many children sit at the frame edge), both norms, at the penalty of vbs_cases that makes every depth
    occur on the host: gme_vbs_u8 on that field; gme_seq_vbs, gme_seq_read_vbs and gme_seq_compensate_vbs on the field an
    exhaustive +-6 search of the same pair leaves in the sequence (no call sets a sequence's field to arbitrary values)."""
    shape, bs, D, r = case
    prev, cur, mf = vc.noise_pair(*case)
    for pnorm in (0, 1):
        penalty = vc.PENALTY[case, pnorm]
        check_pair(native, prev, cur, mf, bs, D, r, pnorm, penalty, vc.noise_result(case, pnorm))
        check_sequence(native, np.stack([prev, cur]), 1, bs, D, r, pnorm, penalty, lambda seq: seq.bbme(1, bs, 6, 0, pnorm))


def test_ties(native):
    """Constant frames with a grey difference (every S equals c at penalty 0: nothing splits) and vertical stripes of period 2
    against the same stripes one column on (many equal costs: the first in the definition's order wins), roots of 8 and 16,
    both norms, through both entry points."""
    flat = np.stack([np.full((37, 53), 90, np.uint8), np.full((37, 53), 97, np.uint8)])
    stripes = np.tile(np.array([0, 255], np.uint8), (37, 27))[:, :53]
    stripes = np.stack([stripes, 255 - stripes])
    rng = np.random.default_rng(5)
    for frames in (flat, stripes):
        for bs, D in ((8, 1), (16, 2), (16, 1)):
            mf = rng.integers(-2, 3, size=(37 // bs, 53 // bs, 2)).astype(np.int32)
            for pnorm in (0, 1):
                for penalty in (0, 64):
                    leaf, depth, cost = check_pair(native, frames[0], frames[1], mf, bs, D, 1, pnorm, penalty)
                    if frames is flat:
                        assert not depth.any() and np.array_equal(leaf, np.repeat(np.repeat(mf, 1 << D, 0), 1 << D, 1))
                got = check_sequence(native, frames, 1, bs, D, 1, pnorm, 0, lambda seq: seq.bbme(1, bs, 3, 0, pnorm))
                if frames is flat:
                    assert not got[1].any()


def test_saturated(native):
    """previous all 0, current all 255 at roots of 64 and MSE: the largest cost there is.  At penalty 0 every S equals c, a tie:
    no split and cost 64 * 64 * 255^2 = 266 342 400; at penalty 2^30 likewise no split, and nothing wraps."""
    frames = np.stack([np.zeros((130, 135), np.uint8), np.full((130, 135), 255, np.uint8)])
    mf = np.zeros((2, 2, 2), np.int32)
    for pnorm, top in ((1, 266342400), (0, 64 * 64 * 255)):
        for penalty in (0, 1 << 30):
            for D, r in ((2, 3), (1, 1)):
                leaf, depth, cost = check_pair(native, frames[0], frames[1], mf, 64, D, r, pnorm, penalty)
                assert np.all(cost == top) and not depth.any() and not leaf.any()
            got = check_sequence(native, frames, 1, 64, 2, 3, pnorm, penalty, lambda seq: seq.hier(1, 64, 8, 3, pnorm, 3))
            assert np.all(got[2] == top) and not got[1].any()


def test_two_motion_scene(native):
    """The scene of tests/test_vbs_host.py on the device: equal to the host, hence the straddling roots split, the others do
    not, and the leaves carry the motion of their side."""
    prev, cur = vc.two_motion_scene()
    mf, leaf, depth, cost = vc.scene_result()
    a = vc.SCENE_ARGS
    check_pair(native, prev, cur, mf, a["block_size"], a["depth"], a["radius"], a["pnorm"], a["penalty"], (leaf, depth, cost))
    got = check_sequence(native, np.stack([prev, cur]), 1, a["block_size"], a["depth"], a["radius"], a["pnorm"], a["penalty"],
                         lambda seq: seq.bbme(1, a["block_size"], vc.SCENE_WINDOW, 0, a["pnorm"]))
    vc.check_scene(mf, got[0][0], got[1][0])


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
h = hashlib.sha256()
for fd in (1, 3):
    for search in ("bbme", "hier"):
        if search == "bbme":
            seq.bbme(fd, 8, 3, 0, 0)
        else:
            seq.hier(fd, 8, 8, 1, 0, 2)
        seq.vbs(fd, 8, 1, 1, 0, 400)
        for a in seq.read_vbs():
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(np.ascontiguousarray(seq.compensate_vbs(fd, 8)).tobytes())
        h.update(np.ascontiguousarray(seq.read_compensated_range(0, 7 - fd)).tobytes())
print("digest", h.hexdigest())
"""


def test_batched(native, tmp_path):
    """Seven frames of 40 x 72, frame distances 1 and 3, roots of 8 at depth 1, after seq.bbme and after seq.hier: every pair
    against the host, a partial read against the full one, the compensated frames and their SSE, the same bytes with two pairs
    per launch (GME_MAX_GRID_PAIRS=2, a fresh process), and the state and argument errors."""
    rng = np.random.default_rng(72)
    frames = rng.integers(0, 256, size=(7, 40, 72), dtype=np.uint8)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    with pytest.raises(native.GmeError, match="before gme_seq_bbme"):             # no field yet
        seq.vbs(1, 8, 1, 1, 0, 400)
    with pytest.raises(native.GmeError, match="before gme_seq_vbs"):
        seq.read_vbs()
    with pytest.raises(native.GmeError, match="before gme_seq_vbs"):
        seq.compensate_vbs(1, 8)
    h = hashlib.sha256()
    for fd in (1, 3):
        for search in (lambda s: s.bbme(fd, 8, 3, 0, 0), lambda s: s.hier(fd, 8, 8, 1, 0, 2)):
            got = check_sequence(native, frames, fd, 8, 1, 1, 0, 400, search)
            assert len(got[0]) == 7 - fd and set(np.unique(got[1]).tolist()) == {0, 1}
            search(seq)
            with pytest.raises(native.GmeError, match="before gme_seq_vbs"):      # a new search ends the validity
                seq.read_vbs()
            seq.vbs(fd, 8, 1, 1, 0, 400)
            full = seq.read_vbs()
            same(full, got[:3], "second sequence")
            part = seq.read_vbs(1, 2)
            same(part, [a[1:3] for a in full], "partial read")
            with pytest.raises(IndexError, match="outside"):
                seq.read_vbs(7 - fd - 1, 2)
            with pytest.raises(native.GmeError, match="block size"):
                seq.vbs(fd, 16, 1, 1, 0, 400)
            with pytest.raises(native.GmeError, match="frame distance"):
                seq.vbs(fd + 1, 8, 1, 1, 0, 400)
            with pytest.raises(native.GmeError, match="block size"):
                seq.compensate_vbs(fd, 4)
            same(seq.read_vbs(), full, "after the refused calls")
            sse = seq.compensate_vbs(fd, 8)
            assert np.array_equal(sse, got[3])
            for a in full:
                h.update(np.ascontiguousarray(a).tobytes())
            h.update(np.ascontiguousarray(sse).tobytes())
            h.update(np.ascontiguousarray(seq.read_compensated_range(0, 7 - fd)).tobytes())
            # any output may be NULL
            leaf = np.zeros_like(full[0])
            assert seq.lib.gme_seq_read_vbs(seq.handle, 0, 7 - fd, native._p(leaf, native._c_i32p), None, None) == 0
            assert np.array_equal(leaf, full[0])
            cost = np.zeros_like(full[2])
            assert seq.lib.gme_seq_read_vbs(seq.handle, 0, 7 - fd, None, None, native._p(cost, native._c_i64p)) == 0
            assert np.array_equal(cost, full[2])
            assert seq.lib.gme_seq_compensate_vbs(seq.handle, fd, 8, None) == 0
    # new frame data ends the validity
    seq.upload(0, frames[:1])
    with pytest.raises(native.GmeError, match="before gme_seq_vbs"):
        seq.read_vbs()
    with pytest.raises(native.GmeError, match="before gme_seq_vbs"):
        seq.compensate_vbs(3, 8)
    # arguments: the host rules raise ValueError, the library's own checks GME_ERR_ARG
    seq.bbme(1, 8, 3, 0, 0)
    p = np.zeros((40, 72), np.uint8)
    for args in ((8, 3, 1, 0, 0), (8, 2, 1, 0, 0), (6, 1, 1, 0, 0), (8, 1, 4, 0, 0), (8, 1, 1, 2, 0), (8, 1, 1, 0, -1),
                 (8, 1, 1, 0, (1 << 30) + 1), (68, 2, 1, 0, 0), (8, -1, 1, 0, 0)):
        with pytest.raises(ValueError):
            seq.vbs(1, *args)
        assert seq.lib.gme_seq_vbs(seq.handle, 1, *args) == native.ERR_ARG
        mf = np.zeros((max(1, 40 // max(args[0], 1)), max(1, 72 // max(args[0], 1)), 2), np.int32)
        leaf = np.zeros((mf.shape[0] * 4, mf.shape[1] * 4, 2), np.int32)
        with pytest.raises(ValueError):
            ctx.vbs(p, p, mf, *args)
        assert seq.lib.gme_vbs_u8(ctx.handle, native._p(p, native._c_u8p), native._p(p, native._c_u8p), 40, 72, 72, *args,
                                  native._p(mf, native._c_i32p), native._p(leaf, native._c_i32p), None, None) == native.ERR_ARG
    want = ctx.vbs(frames[0], frames[1], seq.read_mv()[0], 8, 1, 1, 0, 400)
    leaf = np.zeros_like(want[0])
    mf = np.ascontiguousarray(seq.read_mv()[0])
    assert seq.lib.gme_vbs_u8(ctx.handle, native._p(frames[0], native._c_u8p), native._p(frames[1], native._c_u8p), 40, 72, 72, 8, 1, 1,
                              0, 400, native._p(mf, native._c_i32p), native._p(leaf, native._c_i32p), None, None) == 0
    assert np.array_equal(leaf, want[0])                          # depth_out and cost_out may be NULL
    seq.close()
    np.save(tmp_path / "frames.npy", frames)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd")})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy")], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


def test_sharded_lanes(native):
    """ShardedSequence.motion_fields_vbs: two lanes give what one gives, and what a plain sequence gives."""
    import sequence
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(6, 40, 72), dtype=np.uint8)
    got = []
    for streams in (1, 2):
        sh = sequence.ShardedSequence(40, 72, 6, 1, streams=streams)
        sh.load(frames)
        got.append(sh.motion_fields_vbs(8, 3, 0, 0, depth=1, radius=1, penalty=150, compensate=True))
        with pytest.raises(ValueError):
            sh.motion_fields_vbs(8, 3, 0, 0, depth=2)
        sh.close()
    assert got[0][0].shape == (5, 10, 18, 2) and got[0][1].shape == (5, 10, 18) and got[0][2].shape == (5, 5, 9)
    assert got[0][3].shape == (5,)
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    seq = native.Sequence.from_frames(native.default_context(), frames)
    seq.bbme(1, 8, 3, 0, 0)
    seq.vbs(1, 8, 1, 1, 0, 150)
    same(seq.read_vbs(), got[0][:3], "plain sequence")
    assert np.array_equal(seq.compensate_vbs(1, 8), got[0][3])
    seq.close()


def test_real_frames(native, golden):
    """Three pairs of g9 (the pan240 clip), roots of 16 at depth 2, radius 1, the CLI's default penalties, on the field of the
    exhaustive search at window 16: device equal to host, and the PSNR of the root-field and the leaf-field compensation
    (printed; nothing is asserted about them, the search is a heuristic)."""
    import sequence
    import vbs
    g9 = np.ascontiguousarray(golden("g9_pan240seq")["frames"][:4])
    H, W = g9.shape[1:]
    ctx = native.default_context()
    for pnorm in (0, 1):
        penalty = vbs.default_penalty(16, pnorm)
        leaf, depth, cost, sse = check_sequence(native, g9, 1, 16, 2, 1, pnorm, penalty, lambda seq: seq.bbme(1, 16, 16, 0, pnorm))
        seq = native.Sequence.from_frames(ctx, g9)
        seq.bbme(1, 16, 16, 0, pnorm)
        mv = seq.read_mv()
        seq.close()
        p_root = sequence.psnr_from_sse(np.array([ctx.sse(g9[k + 1], ctx.compensate(g9[k], mv[k])) for k in range(3)]), H, W)
        p_leaf = sequence.psnr_from_sse(sse, H, W)
        for k in range(3):
            s = vbs.summary(depth[k], 2, 0, 0, H, W)
            print("g9 pair %d norm %d penalty %d: psnr root field %.4f dB, leaf field %.4f dB, roots split %.2f %%, leaves %s"
                  % (k, pnorm, penalty, p_root[k], p_leaf[k], 100.0 * s["split_share"], s["leaves"]))


def test_cli_vbs(native, golden, tmp_path, capsys):
    import gme_cli
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(3):
        Image.fromarray(np.ascontiguousarray(g9[k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["vbs", "-p", str(d), "-fi", "2", "-fd", "2", "-o", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "penalty 256" in out and "roots split: " in out and "leaves per depth: " in out
    assert "psnr root field: " in out and "psnr leaf field: " in out
    rec = json.loads((tmp_path / "out" / "vbs.json").read_text())
    assert set(rec) >= {"split_share", "leaves", "sse_root", "sse_leaf", "psnr_root", "psnr_leaf", "psnr_gain", "options", "shape"}
    assert rec["options"]["penalty"] == 256 and rec["shape"] == list(res["mf"].shape[:2]) and len(rec["leaves"]) == 3
    assert rec["split_share"] == float(np.mean(res["depth"][::4, ::4] > 0))
    gme_cli.main(["vbs", "-p", str(d), "-fi", "1", "-pn", "1", "--depth", "1", "-r", "2", "--hier", "-sw", "4"])
    out = capsys.readouterr().out
    assert "depth 1, radius 2, penalty 4096" in out
    gme_cli.main(["info"])
    assert "variable block size" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_vbs.remarks, as the compiler wrote them: no instance of the kernels spills or uses scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_vbs.hip"]
    assert sorted(r["name"].replace(" ", "") for r in rows) == ["k_compensate_vbs", "k_vbs<0,0>", "k_vbs<16,2>", "k_vbs<32,2>"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
