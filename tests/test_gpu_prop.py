"""The vector propagation search on the device (k_prop of bbme_prop.hip through gme_prop_u8, gme_seq_prop and gme_seq_read_prop)
against the host definition propagate.py: byte for byte on noise with every class of candidate, the wavefront and camera scenes,
ties, saturated content, a padded stride, a batched sequence and real frames, plus the error paths and the CLI.  Needs an
MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import prop_cases as pc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mf", "cost", "source")


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def instance(bs):
    return "k_prop<%d>" % (bs if bs in (16, 32) else 0)


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4])


def check_pair(native, previous, current, f, bs, pnorm, rounds, steps, t=None, g=None, want=None):
    """gme_prop_u8 on host buffers against propagate.search (``want``: its result where a test has it already) -> the host's
    result."""
    import propagate
    ctx = native.default_context()
    if want is None:
        want = propagate.search(previous, current, f, bs, pnorm, rounds, steps, t, g)
    got = ctx.prop(previous, current, f, bs, pnorm, rounds, steps, t, g)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    same(got, want, ("gme_prop_u8", current.shape, bs, pnorm, rounds, steps, t is not None, g is not None))
    return want


@pytest.mark.parametrize("pnorm", (0, 1))
@pytest.mark.parametrize("case", pc.NOISE)
def test_noise(native, case, pnorm):
    """Noise pairs of sizes that are no multiple of the block, random f, t and g in [-6, 6] (some unavailable), half of the blocks
    found where one of their candidates points, every (rounds, steps) of prop_cases, with and without t and g.  That every class and
    the MOVED flag occur in these results is asserted on the host (test_prop_host.test_noise_sources)."""
    previous, current, f, t, g = pc.noise_pair(case)
    for rounds, steps in pc.ROUNDS_STEPS:
        for with_t, with_g in pc.GIVEN:
            want = pc.noise_result(case, pnorm, rounds, steps, with_t, with_g)
            check_pair(native, previous, current, f, case[1], pnorm, rounds, steps, t if with_t else None, g if with_g else None, want)
            if not with_t:
                assert not np.any((want[2] & 7) == 2)
            if not with_g:
                assert not np.any((want[2] & 7) == 3)


@pytest.mark.parametrize("pnorm", (0, 1))
def test_scenes(native, pnorm):
    """The wavefront, camera, temporal and refinement scenes of tests/test_prop_host.py on the device."""
    import propagate
    previous, current = pc.pan_scene()
    ok = pc.available_mask(pc.PAN_SHAPE, pc.PAN_BLOCK, pc.PAN_MOVE)
    for rounds in (1, 2, 3, 4):
        mf, _, _ = check_pair(native, previous, current, pc.wavefront_prior(), pc.PAN_BLOCK, pnorm, rounds, 0,
                              want=pc.wavefront_result(pnorm, rounds))
        assert np.array_equal(np.all(mf == pc.PAN_MOVE, axis=-1), pc.reached(ok, pc.PAN_START, rounds))
    for which, cls in (("g", propagate.CAMERA), ("t", propagate.TEMPORAL)):
        field = {which: pc.constant_field(pc.PAN_MOVE)}
        mf, _, source = check_pair(native, previous, current, pc.constant_field((0, 0)), pc.PAN_BLOCK, pnorm, 1, 0,
                                   want=pc.inherit_result(pnorm, which), **field)
        assert np.all(mf[ok] == pc.PAN_MOVE) and np.all(source[ok] == cls) and np.all(source[~ok] == 0)
    for off in pc.REFINE_OFFSETS:
        v = (pc.PAN_MOVE[0] + off[0], pc.PAN_MOVE[1] + off[1])
        both = ok & pc.available_mask(pc.PAN_SHAPE, pc.PAN_BLOCK, v)
        mf, _, source = check_pair(native, previous, current, pc.constant_field(v), pc.PAN_BLOCK, pnorm, 1, 1)
        assert np.all(mf[both] == pc.PAN_MOVE) and np.all(source[both] == (propagate.OWN | propagate.MOVED))


def test_ties(native):
    """Constant frames: every block keeps its own vector with source 0 and no MOVED; block (0, 0), whose own vector points
    outside, takes its first available candidate in list order."""
    import propagate
    previous, current = pc.ties_frames()
    for bs in (8, 16):
        f, t, g = pc.ties_fields(bs)
        for pnorm in (0, 1):
            for rounds, steps in ((1, 2), (2, 4)):
                mf, cost, source = check_pair(native, previous, current, f, bs, pnorm, rounds, steps, t, g)
                assert not np.any(source & propagate.MOVED) and np.all(cost == bs * bs * (7 if pnorm == 0 else 49))
                if rounds == 1:
                    own = propagate.prior_cost(previous, current, f, bs, pnorm) >= 0
                    assert np.all(mf[own] == f[own]) and np.all(source[own] == 0)
                    assert tuple(mf[0, 0]) == (1, 2) and source[0, 0] == propagate.SPATIAL


def test_saturated_and_hostile(native):
    """Blocks of 64 on frames of 0 against 255: the largest cost there is, 64 * 64 * 255^2 under MSE, does not wrap, and every
    block keeps its own vector.  Vectors of +-2^30 in f, t and g are unavailable and no error."""
    lo, hi = np.zeros((130, 135), np.uint8), np.full((130, 135), 255, np.uint8)
    f = np.array([[[1, 0], [2, 1]], [[0, 1], [3, -1]]], np.int32)
    for pnorm, top in ((1, 64 * 64 * 255 * 255), (0, 64 * 64 * 255)):
        mf, cost, source = check_pair(native, lo, hi, f, 64, pnorm, 2, 2, f[::-1].copy(), f[:, ::-1].copy())
        assert np.array_equal(mf, f) and np.all(cost == top) and np.all(source == 0)
    case = pc.NOISE[0]
    previous, current, f, t, g = pc.noise_pair(case)
    big = 1 << 30
    hostile = []
    for k, a in enumerate((f, t, g)):
        a = a.copy()
        a[0, 0] = (big, -big)
        a[1, k] = (-big, 3)
        a[2, 2 + k] = (2, big)
        a[3, 5 - k] = (-(1 << 31), (1 << 31) - 1)
        hostile.append(a)
    for pnorm in (0, 1):
        check_pair(native, previous, current, hostile[0], case[1], pnorm, 2, 1, hostile[1], hostile[2])


def test_padded_stride(native):
    """Rows 7 and 11 bytes longer than the frame is wide: views into wider arrays of other content."""
    case = pc.NOISE[3]
    (H, W), bs = case
    previous, current, f, t, g = pc.noise_pair(case)
    rng = np.random.default_rng(9)
    ctx = native.default_context()
    for pad in (7, 11):
        wide = rng.integers(0, 256, size=(2, H, W + pad), dtype=np.uint8)
        wide[0, :, :W], wide[1, :, :W] = previous, current
        for pnorm in (0, 1):
            got = ctx.prop(wide[0, :, :W], wide[1, :, :W], f, bs, pnorm, 2, 1, t, g)
            same(got, pc.noise_result(case, pnorm, 2, 1, True, True), ("stride", W + pad, pnorm))


def check_sequence(native, seq, frames, fd, bs, pnorm, rounds, steps, temporal, g):
    """gme_seq_prop on the sequence's current field: every pair against propagate.search with t = the prior field of pair k - 1
    -> (prior, the three arrays)."""
    import propagate
    ctx = native.default_context()
    P = len(frames) - fd
    prior = seq.read_mv()
    seq.prop(fd, bs, pnorm, rounds, steps, temporal, g)
    assert ctx.last_bbme_info()["plan"].startswith(instance(bs) + " "), ctx.last_bbme_info()["plan"]
    got = seq.read_prop()
    assert len(got[0]) == P
    for k in range(P):
        want = propagate.search(frames[k], frames[k + fd], prior[k], bs, pnorm, rounds, steps,
                                prior[k - 1] if temporal and k else None, None if g is None else g[k])
        same([a[k] for a in got], want, ("gme_seq_prop", fd, bs, pnorm, rounds, steps, temporal, g is not None, k))
    assert np.array_equal(seq.read_mv(), got[0])
    return prior, got


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
h = hashlib.sha256()
for fd in (1, 2):
    seq.bbme(fd, 8, 4, 3, 0)
    seq.prop(fd, 8, 0, 3, 1, True, np.load(sys.argv[2])[:len(frames) - fd])
    for a in seq.read_prop():
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_sequence(native, tmp_path):
    """Five frames of 48 x 80, frame distances 1 and 2, blocks of 16 and 8, the diamond search and the hierarchical one as
    priors, temporal on and off, g given and NULL: every pair against the host; the result is the sequence's field (read_mv,
    subpel, vbs and a second prop work on it); bipred and gmc results untouched; a partial read, NULL outputs, range, state and
    argument errors; the same bytes with two pairs per launch (GME_MAX_GRID_PAIRS=2, a fresh process)."""
    import propagate
    import subpel
    import vbs
    frames = pc.seq_frames()
    N = len(frames)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    with pytest.raises(native.GmeError, match="before gme_seq_bbme"):              # no field yet
        seq.prop(1, 8)
    with pytest.raises(native.GmeError, match="before gme_seq_prop"):
        seq.read_prop()
    digest = hashlib.sha256()
    for fd in (1, 2):
        P = N - fd
        for bs in (16, 8):
            cam = pc.seq_camera(P, bs)
            searches = (lambda: seq.bbme(fd, bs, pc.SEQ_WINDOW, 3, 0), lambda: seq.hier(fd, bs, pc.SEQ_WINDOW, 1, 0, 3 if bs == 16 else 2))
            # what the sequence holds besides: a bidirectional and a global-motion-compensation result
            seq.bipred(1, bs, pc.SEQ_WINDOW, 0, 0, 1, 1, 64)
            seq.gmc(fd, np.tile(np.array([1.0, 0, 0.5, 0, 1.0, 0, 0, 0]), (P, 1)), bs, pc.SEQ_WINDOW, 0, 0, 16)
            held = list(seq.read_bipred()) + list(seq.read_gmc())
            for search in searches:
                for temporal in (True, False):
                    for g in (cam, None):
                        pnorm = int(temporal) ^ int(g is None)            # both norms over the four combinations
                        search()
                        with pytest.raises(native.GmeError, match="before gme_seq_prop"):      # a new search ends the validity
                            seq.read_prop()
                        check_sequence(native, seq, frames, fd, bs, pnorm, 2, 1, temporal, g)
                for a, b in zip(list(seq.read_bipred()) + list(seq.read_gmc()), held):
                    assert np.array_equal(a, b)
            # the propagated field is the sequence's field: the quarter-pel refinement and the tree run on it ...
            mf = seq.read_mv()
            seq.subpel(fd, bs, 0, 2)
            q, qcost = seq.read_qmv()
            seq.vbs(fd, bs, 1, 1, 0, 400)
            leaf, dmap, vcost = seq.read_vbs()
            for k in range(P):
                wq = subpel.refine(frames[k], frames[k + fd], mf[k], bs, 0, 2)
                assert np.array_equal(q[k], wq[0]) and np.array_equal(qcost[k], wq[1]), ("subpel", k)
                wv = vbs.tree(frames[k], frames[k + fd], mf[k], bs, 1, 1, 0, 400)
                assert all(np.array_equal(a[k], b) for a, b in zip((leaf, dmap, vcost), wv)), ("vbs", k)
            # ... and so does a second propagation, which ends their validity
            check_sequence(native, seq, frames, fd, bs, 1, 1, 2, True, cam)
            for call in (seq.read_qmv, seq.read_vbs):
                with pytest.raises(native.GmeError, match="before gme_seq_"):
                    call()
            with pytest.raises(native.GmeError, match="block size"):
                seq.prop(fd, 32 if bs == 16 else 16)
            with pytest.raises(native.GmeError, match="frame distance"):
                seq.prop(fd + 1, bs)
        # bs 8, the diamond prior, temporal, with g: what the child process repeats
        seq.bbme(fd, 8, pc.SEQ_WINDOW, 3, 0)
        seq.prop(fd, 8, 0, 3, 1, True, pc.seq_camera(P, 8))
        full = seq.read_prop()
        for a in full:
            digest.update(np.ascontiguousarray(a).tobytes())
        # a partial read, range errors, NULL outputs
        part = seq.read_prop(1, 2)
        for a, b in zip(part, full):
            assert np.array_equal(a, b[1:3])
        for first, count in ((P - 1, 2), (-1, 1), (0, P + 1)):
            with pytest.raises(IndexError, match="outside"):
                seq.read_prop(first, count)
        cost, source = np.zeros_like(full[1]), np.zeros_like(full[2])
        assert seq.lib.gme_seq_read_prop(seq.handle, 0, P, None, native._p(cost, native._c_i64p), None) == 0
        assert seq.lib.gme_seq_read_prop(seq.handle, 0, P, None, None, native._p(source, native._c_u8p)) == 0
        assert np.array_equal(cost, full[1]) and np.array_equal(source, full[2])
        assert seq.lib.gme_seq_read_prop(seq.handle, 0, P, None, None, None) == 0
    # arguments (block_size, pnorm, rounds, steps): the host rules raise ValueError, the library's own checks GME_ERR_ARG
    p = np.zeros(pc.SEQ_SHAPE[1:], np.uint8)
    u8, i32 = native._c_u8p, native._c_i32p
    for args in ((3, 0, 1, 0), (68, 0, 1, 0), (8, 2, 1, 0), (8, -1, 1, 0), (8, 0, 0, 0), (8, 0, 5, 0), (8, 0, 1, -1), (8, 0, 1, 5)):
        bs = args[0]
        with pytest.raises(ValueError):
            seq.prop(2, *args)
        assert seq.lib.gme_seq_prop(seq.handle, 2, *args, 1, None) == native.ERR_ARG
        f = np.zeros((max(1, p.shape[0] // bs), max(1, p.shape[1] // bs), 2), np.int32)
        with pytest.raises(ValueError):
            ctx.prop(p, p, f, *args)
        assert seq.lib.gme_prop_u8(ctx.handle, native._p(p, u8), native._p(p, u8), p.shape[0], p.shape[1], p.shape[1], *args,
                                   native._p(f, i32), None, None, native._p(f.copy(), i32), None, None) == native.ERR_ARG
    with pytest.raises(ValueError):                                                 # a camera field of another shape
        seq.prop(2, 8, 0, 1, 0, True, np.zeros((N - 2, 3, 3, 2), np.int32))
    f = np.zeros((p.shape[0] // 8, p.shape[1] // 8, 2), np.int32)
    assert seq.lib.gme_prop_u8(ctx.handle, native._p(p, u8), native._p(p, u8), p.shape[0], p.shape[1], p.shape[1], 8, 0, 1, 0, None, None,
                               None, native._p(f, i32), None, None) == native.ERR_ARG
    # the refused calls left the result valid; new frame data ends the validity
    same(seq.read_prop(), full, "after the refused calls")
    seq.upload(0, frames[:1])
    with pytest.raises(native.GmeError, match="before gme_seq_prop"):
        seq.read_prop()
    seq.close()
    # cost_out and source_out of gme_prop_u8 may be NULL
    f = np.ascontiguousarray(full[0][0])
    want = ctx.prop(frames[0], frames[2], f, 8, 1, 2, 1)
    mf = np.zeros_like(f)
    assert seq.lib.gme_prop_u8(ctx.handle, native._p(frames[0], u8), native._p(frames[2], u8), p.shape[0], p.shape[1], p.shape[1], 8, 1, 2, 1,
                               native._p(f, i32), None, None, native._p(mf, i32), None, None) == 0
    assert np.array_equal(mf, want[0])
    same(want, propagate.search(frames[0], frames[2], f, 8, 1, 2, 1), "gme_prop_u8 without t and g")
    np.save(tmp_path / "frames.npy", frames)
    np.save(tmp_path / "camera.npy", pc.seq_camera(N - 1, 8))
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd")})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy"), str(tmp_path / "camera.npy")],
                         env=dict(os.environ, GME_MAX_GRID_PAIRS="2"), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == digest.hexdigest()


def test_sharded(native):
    """ShardedSequence.motion_fields_prop: one lane equals the resident sequence; with two lanes the first pair of the second
    lane has no temporal prior, and with ``temporal`` off the lanes do not matter."""
    import sequence
    frames = pc.seq_frames()
    N = len(frames)
    cam = pc.seq_camera(N - 1, 8)
    seq = native.Sequence.from_frames(native.default_context(), frames)
    want = {}
    for temporal in (True, False):
        seq.bbme(1, 8, pc.SEQ_WINDOW, 3, 0)
        seq.prop(1, 8, 0, 2, 1, temporal, cam)
        want[temporal] = seq.read_prop()
    seq.close()
    for streams in (1, 2):
        sh = sequence.ShardedSequence(frames.shape[1], frames.shape[2], N, 1, streams=streams)
        sh.load(frames)
        for temporal in (True, False):
            got = sh.motion_fields_prop(8, pc.SEQ_WINDOW, 3, 0, 2, 1, temporal, cam)
            if streams == 1 or not temporal:
                same(got, want[temporal], ("sharded", streams, temporal))
            else:
                assert not np.any((got[2][sh.lanes[1].lo] & 7) == 2) and np.array_equal(got[0][0], want[True][0][0])
        sh.close()


def test_real_frames(native, golden):
    """Pairs 0 .. 2 of g9 (the pan240 clip), blocks of 16, the diamond search at window 16 as the prior, the camera field of the
    direct projective refinement, both norms: device equal to host, and no block costs more than under the prior.  The PSNR
    figures are printed; nothing is asserted about them."""
    import propagate
    import roadmap
    import subpel
    import vbs
    g9 = np.ascontiguousarray(golden("g9_pan240seq")["frames"][:4])
    H, W = g9.shape[1:]
    seq = native.Sequence.from_frames(native.default_context(), g9)
    h = roadmap.refine_sequence(seq, 1)[0]
    fields = [propagate.camera_field(h[k], H, W, 16) for k in range(3)]
    assert all(a is not None for a in fields)
    g = np.stack(fields)
    for pnorm in (0, 1):
        seq.bbme(1, 16, 16, 3, pnorm)
        prior, got = check_sequence(native, seq, g9, 1, 16, pnorm, 2, 1, True, g)
        for k in range(3):
            before = propagate.prior_cost(g9[k], g9[k + 1], prior[k], 16, pnorm)
            assert np.all(got[1][k][before >= 0] <= before[before >= 0]), k
            sse = [int(((g9[k + 1].astype(np.int64) - subpel.compensate_integer(g9[k], a, 16)) ** 2).sum()) for a in (prior[k], got[0][k])]
            print("g9 pair %d norm %d: psnr prior %.4f dB, propagated %.4f dB, vectors changed %.1f%%, camera source %.1f%%"
                  % (k, pnorm, vbs.psnr(sse[0], H, W), vbs.psnr(sse[1], H, W), 100.0 * np.mean(np.any(prior[k] != got[0][k], axis=-1)),
                     100.0 * np.mean((got[2][k] & 7) == 3)))
    seq.close()


def test_motion_field(native):
    """propagate.motion_field: the search, then the propagation, equal to the definition on the search's field."""
    import bbme
    import propagate
    previous, current = pc.pan_scene()
    h = np.array([1.0, 0.0, -float(pc.PAN_MOVE[0]), 0.0, 1.0, -float(pc.PAN_MOVE[1]), 0.0, 0.0])
    f = bbme.get_motion_field(previous, current, 16, 16, 3, 0)[:, :, :2]
    for camera in (None, h):
        got = propagate.motion_field(previous, current, camera=camera)
        g = None if camera is None else propagate.camera_field(h, *pc.PAN_SHAPE, 16)
        same(got, propagate.search(previous, current, f, 16, 0, 2, 1, None, g), ("motion_field", camera is not None))
    assert np.all(g == pc.PAN_MOVE)
    with pytest.raises(ValueError):
        propagate.motion_field(previous, current, rounds=5)


def test_cli_prop(native, golden, tmp_path, capsys):
    import gme_cli
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(4):
        Image.fromarray(np.ascontiguousarray(g9[k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["prop", "-p", str(d), "-fi", "2", "-o", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "rounds 2, steps 1, temporal prior yes, camera projective" in out
    assert "vectors changed: " in out and "sources: own " in out and "mean block cost: prior " in out
    assert "psnr prior field: " in out and "psnr propagated field: " in out
    rec = json.loads((tmp_path / "out" / "prop.json").read_text())
    assert set(rec) >= {"changed_share", "source_share", "moved_share", "mean_cost_prior", "mean_cost_prop", "sse_prior", "sse_prop",
                        "psnr_prior", "psnr_prop", "options", "shape", "h", "camera_field"}
    assert rec["options"]["rounds"] == 2 and rec["options"]["camera"] == "projective" and rec["options"]["temporal"] is True
    assert rec["shape"] == list(res["mf"].shape[:2]) and set(rec["source_share"]) == {"own", "spatial", "temporal", "camera", "zero"}
    assert rec["changed_share"] == float(np.mean(np.any(res["f"] != res["mf"], axis=-1)))
    gme_cli.main(["prop", "-p", str(d), "-fi", "1", "-pn", "1", "--camera", "none", "--rounds", "1", "--steps", "0", "--hier"])
    out = capsys.readouterr().out
    assert "temporal prior no, camera none" in out and "camera 0.00 %" in out
    gme_cli.main(["prop", "-p", str(d), "-fi", "3", "-fd", "1", "--no-temporal", "--camera", "affine"])
    assert "temporal prior no, camera affine" in capsys.readouterr().out
    with pytest.raises(IndexError):
        gme_cli.main(["prop", "-p", str(d), "-fi", "4"])
    gme_cli.main(["info"])
    assert "vector propagation search" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_prop.remarks, as the compiler wrote them: no instance of the kernel spills or uses scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_prop.hip"]
    assert sorted(r["name"].replace(" ", "") for r in rows) == ["k_prop<0>", "k_prop<16>", "k_prop<32>"], rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
