"""obmc.py, the host definition of overlapped block motion compensation: a scalar restatement of it, its
three properties, the exact reciprocal the device divides with, the argument rules, what it gains on real frames, and the two
entries of the C ABI.  Runs without a GPU."""
import os

import numpy as np
import pytest

import obmc
import obmc_cases as oc
import subpel
from oracle import gme_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scalar(previous, field, B, quarter):
    """The definition pixel by pixel in Python integers, written out from the text of the issue rather than from obmc.py."""
    H, W = previous.shape
    Hb, Wb = H // B, W // B
    unit = 1 if quarter else 4

    def S(y, x):
        return int(previous[min(max(y, 0), H - 1), min(max(x, 0), W - 1)])

    def P(X, Y):
        x0, fx, y0, fy = X >> 2, X & 3, Y >> 2, Y & 3
        return ((4 - fx) * (4 - fy) * S(y0, x0) + fx * (4 - fy) * S(y0, x0 + 1) + (4 - fx) * fy * S(y0 + 1, x0)
                + fx * fy * S(y0 + 1, x0 + 1) + 8) >> 4

    out = previous.copy()
    for v in range(Hb * B):
        for u in range(Wb * B):
            i, j = v // B, u // B
            ty, tx = 2 * (v - i * B) + 1 - B, 2 * (u - j * B) + 1 - B
            rows = (i, min(max(i + (-1 if ty < 0 else 1), 0), Hb - 1))
            cols = (j, min(max(j + (-1 if tx < 0 else 1), 0), Wb - 1))
            wy, wx = (2 * B - abs(ty), abs(ty)), (2 * B - abs(tx), abs(tx))
            n = 2 * B * B
            for a in range(2):
                for b in range(2):
                    q = field[rows[a], cols[b]]
                    n += wy[a] * wx[b] * P(4 * u - unit * int(q[0]), 4 * v - unit * int(q[1]))
            out[v, u] = n // (4 * B * B)
    return out


@pytest.mark.parametrize("quarter", oc.UNITS)
@pytest.mark.parametrize("case", oc.SMALL, ids=oc.case_id)
def test_scalar_restatement(case, quarter):
    previous = oc.frames(case)[0]
    got = oc.want(case, quarter)
    assert got.dtype == np.uint8 and got.shape == previous.shape
    assert np.array_equal(got, scalar(previous, oc.field(case, quarter), case[1], quarter))
    (H, W), B = case
    assert np.array_equal(got[H // B * B:], previous[H // B * B:]) and np.array_equal(got[:, W // B * B:], previous[:, W // B * B:])


@pytest.mark.parametrize("B", (4, 5, 8, 12, 16))
def test_zero_field_is_the_frame(B):
    previous = np.random.default_rng(B).integers(0, 256, size=(37, 53), dtype=np.uint8)
    zero = np.zeros((37 // B, 53 // B, 2), np.int32)
    for quarter in oc.UNITS:
        assert np.array_equal(obmc.compensate(previous, zero, B, quarter), previous)


@pytest.mark.parametrize("B", (4, 5, 8, 12, 16))
def test_uniform_field_costs_nothing(B):
    """Under a uniform field every block whose displaced block subpel.interp_block finds inside the frame equals that block."""
    previous = np.random.default_rng(100 + B).integers(0, 256, size=(37, 53), dtype=np.uint8)
    Hb, Wb = 37 // B, 53 // B
    for q in ((0, 0), (5, -7), (-9, 6), (4, 4), (-4 * B, 3), (1, 4 * B - 2)):
        got = obmc.compensate(previous, np.tile(np.array(q, np.int32), (Hb, Wb, 1)), B)
        inside = 0
        for i in range(Hb):
            for j in range(Wb):
                blk = subpel.interp_block(previous, 4 * j * B - q[0], 4 * i * B - q[1], B)
                if blk is not None:
                    inside += 1
                    assert np.array_equal(got[i * B:(i + 1) * B, j * B:(j + 1) * B], blk), (B, q, i, j)
        assert inside > 0, (B, q)
    whole = np.tile(np.array((2, -1), np.int32), (Hb, Wb, 1))
    assert np.array_equal(obmc.compensate(previous, whole, B, quarter=False), obmc.compensate(previous, 4 * whole, B))


def test_weights_sum():
    for B in range(obmc.MIN_BLOCK_SIZE, obmc.MAX_BLOCK_SIZE + 1):
        w = obmc.weights(B)
        assert w.shape == (2, 2, B, B) and w.min() >= 0
        assert np.all(w.sum(axis=(0, 1)) == 4 * B * B)
        if B % 2:
            assert not w[1, :, B // 2, :].any() and not w[:, 1, :, B // 2].any()      # the zero-weight centre row and column


def test_reciprocal_is_exact():
    """(mulhi(n, M)) >> 5 == n // (4 B^2) for every B in 4 .. 64 and every numerator up to 255 * 4 B^2 + 2 B^2, with obmc.py's copy
    of the formula (the library exports no helper of its own)."""
    for B in range(obmc.MIN_BLOCK_SIZE, obmc.MAX_BLOCK_SIZE + 1):
        M = obmc.reciprocal(B)
        assert 0 < M < 1 << 32
        n = np.arange(255 * 4 * B * B + 2 * B * B + 1, dtype=np.int64)
        assert n[-1] < 1 << 22
        assert np.array_equal(obmc.divide(n, M), n // (4 * B * B)), B


def test_argument_and_shape_errors():
    p = np.zeros((20, 30), np.uint8)
    f = np.zeros((2, 3, 2), np.int32)
    assert obmc.compensate(p, f, 8).shape == (20, 30)
    for B in (3, 65, 0, -8):
        with pytest.raises(ValueError):
            obmc.compensate(p, f, B)
    for shape in ((3, 7), (7, 40)):                                 # H < B, W < B
        with pytest.raises(ValueError):
            obmc.compensate(np.zeros(shape, np.uint8), np.zeros((0, 0, 2), np.int32), 8)
    for bad in (np.zeros((2, 3), np.int32), np.zeros((2, 3, 3), np.int32), np.zeros((3, 3, 2), np.int32), np.zeros((2, 2, 2), np.int32),
                np.zeros((1, 2, 3, 2), np.int32), np.zeros((2, 3, 2), np.float32)):
        with pytest.raises(ValueError):
            obmc.compensate(p, bad, 8)
    with pytest.raises(TypeError):
        obmc.compensate(p.astype(np.int16), f, 8)
    with pytest.raises(TypeError):
        obmc.compensate(np.zeros((2, 20, 30), np.uint8), f, 8)
    s = obmc.summary(200, 100, 10, 10)
    assert s["sse_plain"] == 200 and s["sse_obmc"] == 100 and abs(s["psnr_gain"] - 10 * np.log10(2)) < 1e-9
    assert obmc.sse(p, p + 2) == 4 * p.size and obmc.psnr(0, 4, 4) == -1.0


def test_g9_overlapping_lowers_the_error(golden):
    """g9 pairs (10, 11), (11, 12), (12, 13), the reference's diamond search at bs 16 under MAE with subpel.refine on top: the
    overlapped squared error is strictly below the plain one, for the integer field and for the quarter-pel field.  Measured on
    the CPU: 8.81 M against 10.19 M, 9.01 M against 10.71 M and 8.87 M against 10.27 M for the integer field; 8.08 M against
    12.20 M, 8.29 M against 12.92 M and 8.28 M against 12.32 M for the quarter-pel field."""
    g9 = golden("g9_pan240seq")["frames"]
    H, W = g9.shape[1:]
    for k in (10, 11, 12):
        prev, cur = np.ascontiguousarray(g9[k]), np.ascontiguousarray(g9[k + 1])
        mf = gme_oracle.get_motion_field(prev, cur, 16, 16, 3, 0)
        qf = subpel.refine(prev, cur, mf, 16, 0)[0]
        rows = (("integer", obmc.sse(subpel.compensate_integer(prev, mf, 16), cur), obmc.sse(obmc.compensate(prev, mf, 16, quarter=False), cur)),
                ("quarter-pel", obmc.sse(subpel.compensate(prev, qf, 16), cur), obmc.sse(obmc.compensate(prev, qf, 16), cur)))
        for name, plain, lapped in rows:
            print("g9 pair (%d, %d), %s field: plain %d (%.2f dB), overlapped %d (%.2f dB)"
                  % (k, k + 1, name, plain, obmc.psnr(plain, H, W), lapped, obmc.psnr(lapped, H, W)))
        for name, plain, lapped in rows:
            assert lapped < plain, (k, name, lapped, plain)


def test_abi_declares_the_obmc_entries():
    import _gme_native
    lib = _gme_native.load_library()
    header = open(os.path.join(REPO, "include", "gme_hip.h")).read()
    for name in ("gme_obmc_u8", "gme_seq_obmc"):
        assert name in _gme_native.exported_symbols() and hasattr(lib, name) and name + "(" in header
    assert len(_gme_native._SIGNATURES["gme_obmc_u8"][1]) == 11 and len(_gme_native._SIGNATURES["gme_seq_obmc"][1]) == 8
