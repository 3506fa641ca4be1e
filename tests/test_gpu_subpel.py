"""Quarter-pel block matching on the device (k_subpel_refine / k_compensate_qpel of bbme_subpel.hip through gme_subpel_u8,
gme_seq_subpel, gme_seq_read_qmv and gme_seq_compensate_qpel) against the host definition subpel.py: byte for byte on noise,
ties, known shifts, a batched sequence and real frames, plus the error paths and the CLI.  Needs an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import subpel_cases as sc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def pair_on_device(native, prev, cur, mf, bs, pnorm, levels):
    """Field and cost of an arbitrary integer field through the single-pair entry (a sequence only refines its own search)."""
    return native.default_context().subpel(prev, cur, mf, bs, pnorm, levels)


def check_pair(native, prev, cur, mf, bs, pnorm, levels):
    import subpel
    want_q, want_c = subpel.refine(prev, cur, mf, bs, pnorm, levels)
    got_q, got_c = pair_on_device(native, prev, cur, mf, bs, pnorm, levels)
    assert got_q.dtype == np.int32 and got_c.dtype == np.int64
    assert np.array_equal(got_c, want_c), (bs, pnorm, levels, np.argwhere(got_c != want_c)[:4])
    assert np.array_equal(got_q, want_q), (bs, pnorm, levels, np.argwhere(got_q != want_q)[:4])
    return want_q, want_c


def check_sequence(native, frames, fd, bs, sw, procedure, pnorm, levels):
    """Search, refinement, compensation and squared error of a resident sequence against subpel.py fed the device's field."""
    import subpel
    seq = native.Sequence.from_frames(native.default_context(), np.ascontiguousarray(frames))
    seq.bbme(fd, bs, sw, procedure, pnorm)
    mf = seq.read_mv()
    seq.subpel(fd, bs, pnorm, levels)
    q, cost = seq.read_qmv()
    sse = seq.compensate_qpel(fd, bs)
    comp = seq.read_compensated_range(0, len(mf))
    seq.close()
    for k in range(len(mf)):
        want_q, want_c = subpel.refine(frames[k], frames[k + fd], mf[k], bs, pnorm, levels)
        assert np.array_equal(cost[k], want_c) and np.array_equal(q[k], want_q), (k, bs, pnorm, levels)
        want = subpel.compensate(frames[k], want_q, bs)
        assert np.array_equal(comp[k], want), (k, bs, pnorm, levels)
        assert sse[k] == subpel.sse(frames[k + fd], want)
    return mf, q, cost, sse


@pytest.mark.parametrize("shape,bs", [((37, 53), 4), ((37, 53), 8), ((37, 53), 12), ((48, 80), 16)])
def test_noise(native, shape, bs):
    """Frame sizes that are no multiple of the block size (48 x 80 at bs 16 is: its last blocks touch the last row and column);
    the device's own search and a random field in [-bs, bs], where many edge blocks start outside or lose candidates."""
    rng = np.random.default_rng(100 + bs)
    frames = rng.integers(0, 256, size=(2,) + shape, dtype=np.uint8)
    rand = rng.integers(-bs, bs + 1, size=(shape[0] // bs, shape[1] // bs, 2)).astype(np.int32)
    outside = 0
    for pnorm in (0, 1):
        for levels in (0, 1, 2):
            check_sequence(native, frames, 1, bs, 3, 0, pnorm, levels)
            _, cost = check_pair(native, frames[0], frames[1], rand, bs, pnorm, levels)
            outside += int((cost < 0).sum())
    assert outside > 0 and (cost >= 0).any()
    # the compensation of the random field's refinement, whose edge blocks keep the copy
    import subpel
    q, _ = subpel.refine(frames[0], frames[1], rand, bs, 0, 2)
    assert not np.array_equal(subpel.compensate(frames[0], q, bs), frames[0])


@pytest.mark.parametrize("bs,shape", [(1, (5, 7)), (3, (10, 11)), (5, (17, 23)), (64, (130, 135)), (65, (132, 140))])
def test_other_block_sizes(native, bs, shape):
    """The sizes at which the launcher takes another instance: below 4 (four blocks to a wave, run-time size), between the
    compiled sizes, the largest block staged in LDS (64) and the first that is read from global memory with 64-bit sums (65)."""
    rng = np.random.default_rng(bs)
    prev, cur = rng.integers(0, 256, size=(2,) + shape, dtype=np.uint8)
    mf = rng.integers(-1, 2, size=(shape[0] // bs, shape[1] // bs, 2)).astype(np.int32)
    mf[0, 0] = 0
    for pnorm in (0, 1):
        _, cost = check_pair(native, prev, cur, mf, bs, pnorm, 2)
        assert cost[0, 0] >= 0


def test_ties(native):
    """Constant frames (the centre wins every tie) and vertical stripes of period 2 (many equal costs: the first in the
    definition's order wins), both norms, both through a sequence and with a random field."""
    rng = np.random.default_rng(2)
    flat = np.stack([np.full((37, 53), 90, np.uint8), np.full((37, 53), 97, np.uint8)])
    stripes = np.stack([np.full((37, 53), 128, np.uint8), np.tile(np.array([0, 255], np.uint8), (37, 27))[:, :53]])
    for frames in (flat, stripes):
        for bs in (4, 8):
            rand = rng.integers(-2, 3, size=(37 // bs, 53 // bs, 2)).astype(np.int32)
            for pnorm in (0, 1):
                mf, q, _, _ = check_sequence(native, frames, 1, bs, 2, 0, pnorm, 2)
                if frames is flat:
                    assert np.array_equal(q[0], 4 * mf[0])
                check_pair(native, frames[0], frames[1], rand, bs, pnorm, 2)
                check_pair(native, frames[0], frames[1], rand, bs, pnorm, 1)


@pytest.mark.parametrize("shape,bs", [((64, 96), 8), ((96, 128), 16)])
def test_known_shifts(native, shape, bs):
    """The device equals the host on the frames of subpel_cases, hence recovers the shift: every interior block of 96 x 128 at
    bs 16, and the rates of tests/test_subpel_host.py at 64 x 96 (lowest 0.933, asserted less 0.05)."""
    for shift in sc.SHIFTS:
        prev, cur = sc.shifted_pair(shape[0], shape[1], shift, bs)
        for pnorm in (0, 1):
            _, q, _, _ = check_sequence(native, np.stack([prev, cur]), 1, bs, 3, 0, pnorm, 2)
            assert sc.interior_hits(q[0], shift) >= 0.933 - 0.05


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r]
import _gme_native as native
frames = np.load(sys.argv[1])
seq = native.Sequence.from_frames(native.default_context(), frames)
h = hashlib.sha256()
for fd in (1, 3):
    seq.bbme(fd, 8, 3, 0, 0)
    seq.subpel(fd, 8, 0, 2)
    q, cost = seq.read_qmv()
    sse = seq.compensate_qpel(fd, 8)
    for a in (q, cost, sse, seq.read_compensated_range(0, len(q))):
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_batched(native, tmp_path):
    """Seven frames of 40 x 72, frame distances 1 and 3, bs 8: every pair against the host, a partial read against the full
    one, the same bytes with two pairs per launch (GME_MAX_GRID_PAIRS=2, a fresh process), and the call-order errors."""
    rng = np.random.default_rng(72)
    frames = rng.integers(0, 256, size=(7, 40, 72), dtype=np.uint8)
    h = hashlib.sha256()
    for fd in (1, 3):
        _, q, cost, sse = check_sequence(native, frames, fd, 8, 3, 0, 0, 2)
        assert len(q) == 7 - fd
    seq = native.Sequence.from_frames(native.default_context(), frames)
    with pytest.raises(native.GmeError, match="before gme_seq_bbme"):
        seq.subpel(1, 8, 0)
    for fd in (1, 3):
        seq.bbme(fd, 8, 3, 0, 0)
        with pytest.raises(native.GmeError, match="before gme_seq_subpel"):
            seq.read_qmv()
        with pytest.raises(native.GmeError, match="before gme_seq_subpel"):
            seq.compensate_qpel(fd, 8)
        with pytest.raises(native.GmeError, match="block size"):
            seq.subpel(fd, 4, 0)
        with pytest.raises(native.GmeError, match="frame distance"):
            seq.subpel(fd + 1, 8, 0)
        with pytest.raises(ValueError):
            seq.subpel(fd, 8, 0, 3)
        seq.subpel(fd, 8, 0, 2)
        q, cost = seq.read_qmv()
        q12, cost12 = seq.read_qmv(1, 2)
        assert np.array_equal(q12, q[1:3]) and np.array_equal(cost12, cost[1:3])
        with pytest.raises(IndexError, match="outside"):
            seq.read_qmv(7 - fd - 1, 2)
        with pytest.raises(native.GmeError, match="block size"):
            seq.compensate_qpel(fd, 4)
        sse = seq.compensate_qpel(fd, 8)
        for a in (q, cost, sse, seq.read_compensated_range(0, len(q))):
            h.update(np.ascontiguousarray(a).tobytes())
    seq.close()
    np.save(tmp_path / "frames.npy", frames)
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd")})
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "frames.npy")], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


def test_sharded_lanes(native):
    """ShardedSequence.motion_fields_subpel: two lanes give what one gives."""
    import sequence
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, size=(6, 40, 72), dtype=np.uint8)
    got = []
    for streams in (1, 2):
        sh = sequence.ShardedSequence(40, 72, 6, 1, streams=streams)
        sh.load(frames)
        got.append(sh.motion_fields_subpel(8, 3, 0, 1, levels=2, compensate=True))
        assert len(sh.motion_fields_subpel(8, 3, 0, 1, levels=1)) == 2
        sh.close()
    assert got[0][0].shape == (5, 5, 9, 2) and got[0][1].shape == (5, 5, 9) and got[0][2].shape == (5,)
    for a, b in zip(*got):
        assert np.array_equal(a, b)


def test_real_frames(native, golden):
    """Three pairs of g9 (the pan240 clip), bs 16, diamond search: device equal to host, and the PSNR of the quarter-pel
    compensation against that of the integer compensation of the same search (DESIGN.md section 7e records the figures)."""
    import sequence
    import subpel
    g9 = np.ascontiguousarray(golden("g9_pan240seq")["frames"][:4])
    H, W = g9.shape[1:]
    ctx = native.default_context()
    for pnorm in (0, 1):
        mf, q, cost, sse_q = check_sequence(native, g9, 1, 16, 16, 3, pnorm, 2)
        sse_i = np.array([ctx.sse(g9[k + 1], ctx.compensate(g9[k], mf[k])) for k in range(3)])
        p_i, p_q = sequence.psnr_from_sse(sse_i, H, W), sequence.psnr_from_sse(sse_q, H, W)
        for k in range(3):
            print("g9 pair %d norm %d: psnr integer %.4f dB, quarter-pel %.4f dB (gain %+.4f), moved %.1f %% of the blocks"
                  % (k, pnorm, p_i[k], p_q[k], p_q[k] - p_i[k], 100.0 * np.mean(np.any(q[k] != 4 * mf[k], axis=2))))
        assert np.all(cost >= 0) or np.all(cost[cost < 0] == -1)
        assert np.all(p_q >= p_i), (p_i, p_q)


def test_cli_subpel(native, golden, tmp_path, capsys):
    import gme_cli
    from PIL import Image
    g9 = golden("g9_pan240seq")["frames"]
    d = tmp_path / "clip"
    d.mkdir()
    for k in range(3):
        Image.fromarray(np.ascontiguousarray(g9[k])).save(d / ("%04d.png" % k))
    res = gme_cli.main(["subpel", "-p", str(d), "-fi", "2", "-fd", "2", "-sp", "3", "-o", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "median vector" in out and "psnr quarter-pel" in out
    rec = json.loads((tmp_path / "out" / "subpel.json").read_text())
    assert set(rec) >= {"median_vector", "moved_share", "psnr_integer", "psnr_qpel", "psnr_gain", "options", "shape"}
    assert rec["shape"] == list(res["mf"].shape[:2]) and 0.0 <= rec["moved_share"] <= 1.0
    assert rec["median_vector"] == [float(np.median(res["qfield"][:, :, 0])) / 4, float(np.median(res["qfield"][:, :, 1])) / 4]
    assert abs(rec["psnr_gain"] - (rec["psnr_qpel"] - rec["psnr_integer"])) < 1e-12
    gme_cli.main(["subpel", "-p", str(d), "-fi", "1", "--levels", "0", "-pn", "1"])
    assert "moved off the integer vector: 0.00 %" in capsys.readouterr().out


def test_no_spill():
    """csrc/build/bbme_subpel.remarks, as the compiler wrote them: no instance of either kernel spills or uses scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_subpel.hip"]
    assert {r["name"].split("<")[0] for r in rows} == {"k_subpel_refine", "k_compensate_qpel"}, rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
