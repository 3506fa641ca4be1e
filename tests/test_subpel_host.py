"""subpel.py, the host definition of quarter-pel block matching: the interpolation formula, the edge
rules, the selection order and what the definition achieves on frames whose shift is known.  Runs without a GPU."""
import os
import sys

import numpy as np
import pytest

import subpel
import subpel_cases as sc
from helpers import c_oracle
from oracle import gme_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test_known_shift: the definition on sc.shifted_pair(64, 96, shift, 8) after the C oracle's exhaustive search at sw 3, measured
# on the CPU.  Interior hit rate (MAE / MSE) and squared error of the integer -> the quarter-pel compensation (MAE; MSE within
# 2 % of it):
#   (5, -3)  0.983 / 0.983   140189 -> 16422
#   (-6, 2)  0.933 / 0.950   384483 -> 29342
#   (1, 1)   0.983 / 0.983   138921 -> 16417
#   (9, 7)   0.983 / 0.983   106898 -> 16520
#   (0, 0)   1.000 / 1.000        0 -> 0
# The field median is the true shift in every case.  The floor below is the lowest rate less 0.05.
HIT_RATE_MIN = 0.933


def float_bilinear(img, X, Y, bs):
    """The block at (X / 4, Y / 4) by float64 bilinear interpolation, rounded half up."""
    x, y = X / 4.0, Y / 4.0
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    ax, ay = x - x0, y - y0
    p = np.pad(img.astype(np.float64), ((0, 1), (0, 1)))         # a tap of weight zero may lie outside: any value does
    b = lambda dy, dx: p[y0 + dy:y0 + dy + bs, x0 + dx:x0 + dx + bs]
    v = (1 - ax) * (1 - ay) * b(0, 0) + ax * (1 - ay) * b(0, 1) + (1 - ax) * ay * b(1, 0) + ax * ay * b(1, 1)
    return np.floor(v + 0.5).astype(np.int32)


def test_interpolation_all_phases():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(19, 23), dtype=np.uint8)
    for fy in range(4):
        for fx in range(4):
            for x0, y0, bs in ((0, 0, 5), (3, 2, 8), (23 - 6 - (fx != 0), 19 - 6 - (fy != 0), 6)):
                got = subpel.interp_block(img, 4 * x0 + fx, 4 * y0 + fy, bs)
                assert got is not None and np.array_equal(got, float_bilinear(img, 4 * x0 + fx, 4 * y0 + fy, bs)), (fx, fy, x0)
    a, b, c, d = (img[2:7, 3:8].astype(np.int32), img[2:7, 4:9].astype(np.int32), img[3:8, 3:8].astype(np.int32),
                  img[3:8, 4:9].astype(np.int32))
    assert np.array_equal(subpel.interp_block(img, 14, 8, 5), (a + b + 1) >> 1)
    assert np.array_equal(subpel.interp_block(img, 12, 10, 5), (a + c + 1) >> 1)
    assert np.array_equal(subpel.interp_block(img, 14, 10, 5), (a + b + c + d + 2) >> 2)


def test_inside_rule():
    img = np.zeros((16, 24), np.uint8)
    assert subpel.interp_block(img, 0, 0, 8) is not None
    assert subpel.interp_block(img, -1, 0, 8) is None and subpel.interp_block(img, 0, -1, 8) is None     # floor: x0 = -1
    assert subpel.interp_block(img, 4 * 16, 4 * 8, 8) is not None                                        # the last whole position
    assert subpel.interp_block(img, 4 * 16 + 1, 4 * 8, 8) is None and subpel.interp_block(img, 4 * 16, 4 * 8 + 1, 8) is None
    assert subpel.interp_block(img, 4 * 15 + 3, 4 * 7 + 3, 8) is not None


@pytest.mark.parametrize("pnorm", [0, 1])
def test_level_zero_is_the_integer_cost(pnorm):
    rng = np.random.default_rng(11)
    prev, cur = rng.integers(0, 256, size=(2, 37, 53), dtype=np.uint8)
    bs = 8
    mf = c_oracle().bbme(prev, cur, bs, 4, 0, pnorm)
    q, cost = subpel.refine(prev, cur, mf, bs, pnorm, levels=0)
    assert q.dtype == np.int32 and cost.dtype == np.int64 and np.array_equal(q, 4 * mf)
    for i in range(mf.shape[0]):
        for j in range(mf.shape[1]):
            r, c = i * bs + mf[i, j, 1], j * bs + mf[i, j, 0]
            want = gme_oracle.block_cost(prev[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs], cur[r:r + bs, c:c + bs], pnorm)
            assert cost[i, j] == int(want)
    # more levels never cost more, and a refined vector stays within 3/4 pixel of the integer one
    q2, cost2 = subpel.refine(prev, cur, mf, bs, pnorm, levels=2)
    q1, cost1 = subpel.refine(prev, cur, mf, bs, pnorm, levels=1)
    assert np.all(cost2 <= cost1) and np.all(cost1 <= cost) and np.abs(q2 - 4 * mf).max() <= 3 and np.all((q1 - 4 * mf) % 2 == 0)
    assert np.any(q2 != 4 * mf)
    with pytest.raises(ValueError):
        subpel.refine(prev, cur, mf, bs, pnorm, levels=3)
    with pytest.raises(ValueError):
        subpel.refine(prev, cur, mf, bs, pnorm, levels=-1)


def test_constant_frames_keep_the_centre():
    prev, cur = np.full((32, 48), 90, np.uint8), np.full((32, 48), 97, np.uint8)
    mf = np.zeros((4, 6, 2), np.int32)
    mf[1:3, 1:5] = (1, -1)
    for pnorm in (0, 1):
        q, cost = subpel.refine(prev, cur, mf, 8, pnorm)
        assert np.array_equal(q, 4 * mf) and np.all(cost == 64 * (7 if pnorm == 0 else 49))


def test_first_minimum_wins():
    """Vertical stripes of period 2: every half-pel candidate with a horizontal offset sees the same grey block, so many costs
    tie, and the first in the definition's order (column offset outer, then row offset) must be the one kept."""
    prev = np.full((16, 24), 128, np.uint8)
    cur = np.tile(np.array([0, 255], np.uint8), (16, 12))
    mf = np.zeros((2, 3, 2), np.int32)
    q, cost = subpel.refine(prev, cur, mf, 8, 0, levels=1)
    # block (0, 0): ox = -2 is outside; ox = 0 keeps the stripes (cost 64 * 127.5); the first grey candidate is (2, -2), outside
    # for the first block row, then (2, 0)
    assert tuple(q[0, 0]) == (2, 0) and tuple(q[1, 1]) == (-2, -2) and tuple(q[1, 0]) == (2, -2)
    assert cost[1, 1] == 0 and cost[0, 0] == 0


def test_vector_pointing_outside_is_left_alone():
    rng = np.random.default_rng(5)
    prev, cur = rng.integers(0, 256, size=(2, 24, 40), dtype=np.uint8)
    mf = np.zeros((3, 5, 2), np.int32)
    mf[0, 0] = (-1, 0)
    mf[2, 4] = (0, 1)
    mf[1, 2] = (40, 0)
    q, cost = subpel.refine(prev, cur, mf, 8, 0)
    for ij in ((0, 0), (2, 4), (1, 2)):
        assert cost[ij] == -1 and np.array_equal(q[ij], 4 * mf[ij])
    assert np.all(cost[(cost >= 0)] > 0) and (cost >= 0).sum() == 12
    # block (0, 1) starts inside, its candidates above the frame are skipped: the row component never goes negative
    assert q[0, 1, 1] >= 0


def test_compensate_matches_the_integer_rule():
    rng = np.random.default_rng(8)
    prev = rng.integers(0, 256, size=(35, 53), dtype=np.uint8)     # 35 // 4 == 8: the oracle takes the block size from the shapes
    bs = 8
    mf = rng.integers(-3, 4, size=(4, 6, 2)).astype(np.int32)
    mf[0, :, 1] = np.minimum(mf[0, :, 1], 0)                     # every displaced block inside: source = block - vector
    mf[:, 0, 0] = np.minimum(mf[:, 0, 0], 0)
    mf[3, :, 1] = np.maximum(mf[3, :, 1], 0)
    mf[:, 5, 0] = np.maximum(mf[:, 5, 0], 0)
    out = subpel.compensate(prev, 4 * mf, bs)
    assert np.array_equal(out, gme_oracle.compensate_frame(prev, mf))
    assert np.array_equal(out, subpel.compensate_integer(prev, mf, bs))
    assert np.array_equal(out[32:], prev[32:]) and np.array_equal(out[:, 48:], prev[:, 48:])
    mf[0, 0] = (1, 0)                                            # a block whose source leaves the frame keeps the copy, whole
    out = subpel.compensate(prev, 4 * mf, bs)
    assert np.array_equal(out[:8, :8], prev[:8, :8])
    assert np.array_equal(subpel.compensate_integer(prev, mf, bs), gme_oracle.compensate_frame(prev, mf))


@pytest.mark.parametrize("shift", sc.SHIFTS)
def test_known_shift(shift):
    H, W, bs = 64, 96, 8
    prev, cur = sc.shifted_pair(H, W, shift, bs)
    for pnorm in (0, 1):
        mf = c_oracle().bbme(prev, cur, bs, 3, 0, pnorm)
        q, cost = subpel.refine(prev, cur, mf, bs, pnorm)
        median = (int(np.median(q[:, :, 0])), int(np.median(q[:, :, 1])))
        hits = sc.interior_hits(q, shift)
        sse_i = subpel.sse(cur, subpel.compensate_integer(prev, mf, bs))
        sse_q = subpel.sse(cur, subpel.compensate(prev, q, bs))
        print("shift %r norm %d: median %r, interior hits %.3f, sse %d -> %d" % (shift, pnorm, median, hits, sse_i, sse_q))
        assert median == tuple(shift)
        assert hits >= HIT_RATE_MIN - 0.05
        if shift != (0, 0):
            assert sse_q < sse_i
        else:
            assert sse_q == 0 and sse_i == 0
        s = subpel.summary(mf, q, sse_i, sse_q, H, W)
        assert s["median_vector"] == [shift[0] / 4.0, shift[1] / 4.0] and (s["psnr_gain"] > 0) == (shift != (0, 0))


def test_abi_declares_the_subpel_entries():
    import _gme_native
    lib = _gme_native.load_library()
    header = open(os.path.join(REPO, "include", "gme_hip.h")).read()
    for name in ("gme_subpel_u8", "gme_seq_subpel", "gme_seq_read_qmv", "gme_seq_compensate_qpel"):
        assert name in _gme_native.exported_symbols() and hasattr(lib, name) and name + "(" in header


def test_subpel_kernels_do_not_spill():
    """The compiler's resource remarks for bbme_subpel.hip: every instance of both kernels, no VGPR or SGPR spill, no scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "bbme_subpel.hip"]
    names = {r["name"] for r in rows}
    assert "k_compensate_qpel" in names and {n.split("<")[0] for n in names} == {"k_subpel_refine", "k_compensate_qpel"}, names
    assert len(rows) == 8, names                                 # seven instances of the refinement
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
