"""Full-frame stabilization on the device (k_warp_fill of gme_stab_fill.hip through gme_seq_warp_fill) against the host
definition stabilize.warp_fill, byte for byte: shapes and candidate counts, degenerate candidates, sub-ranges and launch chunks,
NULL outputs, what the sequence keeps, the whole stabilization with neighbours, the error paths and the CLI.  Needs an
MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stabfill_cases as cases
from test_direct_host import warp_canvas
from test_gpu_stabilize import random_warps, reaches, sequence_of
from test_stabfill_host import assert_coverage
from test_stabilize_host import camera_path

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("frames", "source", "valid", "filled", "sse")


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def same(got, want, what):
    for a, b, name in zip(got, want, NAMES):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, name)


@pytest.mark.parametrize("shape", cases.SHAPES)
@pytest.mark.parametrize("n", cases.CANDIDATES)
def test_warp_fill_equals_host(native, shape, n):
    """Every output in the three border / fill modes.  The coverage condition is asserted on the host's `source` map first:
    every j < n wins somewhere, 255 occurs, a row is all candidate 0's (the early exit), a wave has lanes resolved at
    different j; the lists hold a -1 in the middle, a frame twice and frames out of temporal order."""
    import stabilize
    case = cases.case(shape, n)
    assert_coverage(case, n)
    seq = sequence_of(native, case["frames"])
    for (border, fill), want in case["want"].items():
        got = seq.warp_fill(0, case["sources"], case["warps"], stabilize.border_id(border), fill, want_source=True)
        same(got, want, (shape, n, border, fill))
    seq.close()


@pytest.mark.parametrize("border,fill", [("constant", 201), ("replicate", 0)])
def test_degenerate_candidates_equal_host(native, border, fill):
    """The degenerate warps of test_gpu_stabilize.py (last column / row, mirrors, horizons, d == 0 on a row, NaN and +-inf) as
    candidates 1 .. 11 behind a far candidate 0, each first in line in some frame."""
    import stabilize
    frames, sources, warps, names, table = cases.degenerate_case()
    H, W = cases.DEGENERATE_SHAPE
    for name in names:
        assert reaches(table[name][0], table[name][1], H, W), name
    want = stabilize.warp_fill(frames, sources, warps, border, fill)
    assert len(set(np.unique(want[1]).tolist()) - {0, 255}) >= 6          # the degenerate candidates do win pixels
    seq = sequence_of(native, frames)
    same(seq.warp_fill(0, sources, warps, stabilize.border_id(border), fill, want_source=True), want, (border, fill))
    seq.close()


_CHILD = """
import hashlib, sys
import numpy as np
sys.path[:0] = [%(pkg)r, %(tests)r]
import _gme_native as native
import stabfill_cases as cases
case = cases.case(%(shape)r, %(n)d)
seq = native.Sequence.from_frames(native.default_context(), case["frames"])
h = hashlib.sha256()
for first, count in %(ranges)r:
    for a in seq.warp_fill(first, case["sources"][first:first + count], case["warps"][first:first + count], 1, 0, want_source=True):
        h.update(np.ascontiguousarray(a).tobytes())
print("digest", h.hexdigest())
"""


def test_sub_range_and_chunks(native, tmp_path):
    """A sub-range (first > 0) whose sources point outside it, and the same bytes with two planes per launch
    (GME_MAX_GRID_PAIRS=2, a fresh process)."""
    shape, n = (41, 131), 3
    case = cases.case(shape, n)
    want = case["want"][("replicate", 0)]
    ranges = ((0, cases.N_FRAMES), (2, 5), (3, 1))
    seq = sequence_of(native, case["frames"])
    h = hashlib.sha256()
    for first, count in ranges:
        src = case["sources"][first:first + count]
        assert count == cases.N_FRAMES or np.any((src >= 0) & ((src < first) | (src >= first + count)))
        got = seq.warp_fill(first, src, case["warps"][first:first + count], 1, 0, want_source=True)
        same(got, tuple(w[first:first + count] for w in want[:4]) + (want[4][first:first + count - 1],), (first, count))
        for a in got:
            h.update(np.ascontiguousarray(a).tobytes())
    empty = seq.warp_fill(cases.N_FRAMES, case["sources"][:0], case["warps"][:0])
    assert empty[0].shape == (0,) + shape and empty[1] is None and all(len(a) == 0 for a in empty[2:])
    seq.close()
    script = tmp_path / "child.py"
    script.write_text(_CHILD % {"pkg": os.path.join(REPO, "global-motion-estimation_amd"), "tests": os.path.join(REPO, "tests"),
                                "shape": shape, "n": n, "ranges": ranges})
    out = subprocess.run([sys.executable, str(script)], env=dict(os.environ, GME_MAX_GRID_PAIRS="2"), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-1] == h.hexdigest()


def test_null_outputs(native):
    """Each output NULL in turn, all of them NULL, and the frames without the source map."""
    shape, n = (37, 53), 3
    case = cases.case(shape, n)
    want = case["want"][("constant", 201)]
    N, (H, W) = cases.N_FRAMES, shape
    seq = sequence_of(native, case["frames"])
    types = (native._c_u8p, native._c_u8p, native._c_i64p, native._c_i64p, native._c_i64p)
    src, w = np.ascontiguousarray(case["sources"]), np.ascontiguousarray(case["warps"])
    head = (seq.handle, 0, N, n, native._p(src, native._c_i32p), native._p(w, native._c_f64p), 0, 201)
    for skip in (None, 0, 1, 2, 3, 4, "all"):
        outs = [np.zeros((N, H, W), np.uint8), np.zeros((N, H, W), np.uint8), np.zeros(N, np.int64), np.zeros(N, np.int64),
                np.zeros(N - 1, np.int64)]
        ptrs = [None if skip == "all" or skip == k else native._p(a, t) for k, (a, t) in enumerate(zip(outs, types))]
        assert seq.lib.gme_seq_warp_fill(*head, *ptrs) == 0, skip
        for k, (a, b) in enumerate(zip(outs, want)):
            assert np.array_equal(a, b if ptrs[k] is not None else np.zeros_like(a)), (skip, NAMES[k])
    got = seq.warp_fill(0, src, w, 0, 201)
    assert got[1] is None and np.array_equal(got[0], want[0])
    seq.close()


def test_keeps_nothing(native):
    """After warp_frames, bbme and a subpel, a warp_fill leaves read_warped_range, read_mv and read_qmv byte-identical;
    in split-phase mode the call computes and returns the same bytes."""
    rng = np.random.default_rng(72)
    N, H, W, n = 7, 40, 72, 3
    frames = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    sources = rng.integers(0, N, size=(N, n)).astype(np.int32)
    sources[3, 1] = -1
    warps = random_warps(rng, N * n, H, W, far=True).reshape(N, n, 8)
    import stabilize
    want = stabilize.warp_fill(frames, sources, warps, "replicate")
    seq = sequence_of(native, frames)
    seq.warp_frames(0, warps[:, 1], 0, 9)
    seq.bbme(1, 8, 3, 0, 0)
    seq.subpel(1, 8, 0, 2)
    warped, mv, qmv = seq.read_warped_range(0, N), seq.read_mv(), seq.read_qmv()
    same(seq.warp_fill(0, sources, warps, 1, 0, want_source=True), want, "blocking")
    seq.set_split_phase(True)
    same(seq.warp_fill(0, sources, warps, 1, 0, want_source=True), want, "split-phase")
    seq.set_split_phase(False)
    assert np.array_equal(seq.read_warped_range(0, N), warped) and np.array_equal(seq.read_mv(), mv)
    for a, b in zip(seq.read_qmv(), qmv):
        assert np.array_equal(a, b)
    assert np.array_equal(warped, stabilize.warp_frames(frames, warps[:, 1], "constant", 9)[0])
    seq.close()


def test_end_to_end(native):
    """test_known_jitter's clip (320 x 240, 48 frames) through stabilize.stabilize(frames, neighbours=2): crop 0, every pixel
    accounted for, pixels filled, ITF above the input's and above that of the cropless constant-border output, the frames
    those of the host definition, and a second run the same bytes."""
    import stabilize
    H, W, n = 240, 320, 48
    G = camera_path(n, H, W)
    frames = np.stack([warp_canvas(stabilize.params(G[t]), H, W)[1] for t in range(n)])
    out, res = stabilize.stabilize(frames, neighbours=2)
    _, plain = stabilize.stabilize(frames, crop=0.0)
    print("known jitter, 2 neighbours a side: itf %.3f -> %.3f dB (crop 0 with a constant border: %.3f dB); filled %.3f %%, unfilled "
          "%.4f %% of the pixels" % (res["itf_before"], res["itf_after"], plain["itf_after"],
                                      100.0 * res["filled"].sum() / (n * H * W), 100.0 * res["unfilled"].sum() / (n * H * W)))
    assert res["crop"] == 0.0 and res["neighbours"] == 2 and res["sources"].shape == (n, 5)
    assert np.array_equal(res["valid"] + res["filled"] + res["unfilled"], np.full(n, H * W))
    assert res["filled"].sum() > 0 and res["unfilled"].min() >= 0
    assert res["itf_after"] > res["itf_before"]
    assert res["itf_after"] > plain["itf_after"]
    want = stabilize.warp_fill(frames, res["sources"], res["fill_warps"], "constant", 0)
    assert np.array_equal(out, want[0]) and np.array_equal(res["valid"], want[2]) and np.array_equal(res["filled"], want[3])
    assert res["itf_after"] == stabilize.itf(want[4], H, W)
    again, res2 = stabilize.stabilize(frames, neighbours=2)
    assert np.array_equal(again, out) and res2["itf_after"] == res["itf_after"] and np.array_equal(res2["filled"], res["filled"])


def test_error_paths(native):
    """GME_ERR_ARG: a range outside [0, N), n_cand outside 1 .. 17, a source outside -1 .. N-1, candidate 0 not a frame, a bad
    border or fill; the sharded surface refuses neighbours with more than one lane."""
    import sequence
    N, H, W = 4, 24, 40
    frames = np.random.default_rng(1).integers(0, 256, size=(N, H, W), dtype=np.uint8)
    seq = sequence_of(native, frames)
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64)

    def call(first, sources, border=0, fill=0):
        sources = np.asarray(sources, np.int32)
        return seq.warp_fill(first, sources, np.tile(ident, sources.shape + (1,)), border, fill)
    assert np.array_equal(call(2, [[2, 0], [3, -1]])[0], frames[2:])
    for first, rows in ((3, 2), (-1, 1), (4, 1), (0, 5)):
        with pytest.raises(IndexError, match="outside"):
            call(first, [[0]] * rows)
    with pytest.raises(IndexError, match="candidates"):
        call(0, [[0] * 18])
    with pytest.raises(IndexError, match="candidates"):
        call(0, np.zeros((1, 0), np.int32))
    assert call(0, [[0] * 17])[0].shape == (1, H, W)
    for bad in (4, -2):
        with pytest.raises(IndexError, match="source"):
            call(0, [[0, bad]])
    with pytest.raises(IndexError, match="candidate 0"):
        call(0, [[0, 1], [-1, 1]])
    with pytest.raises(IndexError, match="border"):
        call(0, [[0]], 2)
    for fill in (-1, 256):
        with pytest.raises(IndexError, match="fill"):
            call(0, [[0]], 0, fill)
    src = np.zeros((1, 1), np.int32)
    assert seq.lib.gme_seq_warp_fill(None, 0, 1, 1, native._p(src, native._c_i32p), native._p(ident, native._c_f64p), 0, 0,
                                     None, None, None, None, None) == native.ERR_ARG
    assert seq.lib.gme_seq_warp_fill(seq.handle, 0, 1, 1, None, native._p(ident, native._c_f64p), 0, 0, None, None, None, None,
                                     None) == native.ERR_ARG
    seq.close()
    sh = sequence.ShardedSequence(H, W, 6, 1, streams=2)
    with pytest.raises(ValueError, match="whole video in one sequence"):
        sh.stabilize(neighbours=1)
    sh.close()


def test_cli_neighbours(native, golden, tmp_path, capsys):
    import gme_cli
    clip = np.ascontiguousarray(golden("g9_pan240seq")["frames"][:12])
    np.save(tmp_path / "clip.npy", clip)
    res = gme_cli.main(["stabilize", "-p", str(tmp_path / "clip.npy"), "-o", str(tmp_path / "out"), "--neighbours", "2", "--radius", "4"])
    assert "itf after" in capsys.readouterr().out
    rec = json.loads((tmp_path / "out" / "stabilize.json").read_text())
    assert rec["neighbours"] == 2 and rec["options"]["neighbours"] == 2 and rec["crop"] == 0.0
    assert len(rec["filled"]) == len(rec["unfilled"]) == len(rec["valid"]) == 12
    assert [a + b + c for a, b, c in zip(rec["valid"], rec["filled"], rec["unfilled"])] == [240 * 320] * 12
    assert rec["filled"] == res["filled"].tolist() and rec["itf_after"] == res["itf_after"]
    assert len(sorted((tmp_path / "out" / "stabilized").glob("*.png"))) == 12
