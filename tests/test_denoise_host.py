"""denoise.py, the host definition of motion-compensated temporal denoising: a scalar restatement of it,
its three properties, the exact reciprocal, the argument rules, what it achieves on a moving noisy scene, and the two entries of
the C ABI.  Runs without a GPU."""
import os

import numpy as np
import pytest

import denoise
import denoise_cases as dc
import obmc
from oracle import gme_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scalar(current, predictions, strength):
    """The definition pixel by pixel in Python integers, written out from the text of the issue rather than from denoise.py."""
    H, W = current.shape
    S = 9 * strength
    out = np.zeros((H, W), np.uint8)
    for v in range(H):
        for u in range(W):
            tot, n = S, S * int(current[v, u])
            for p in predictions:
                D = 0
                for a in (-1, 0, 1):
                    for b in (-1, 0, 1):
                        y, x = min(max(v + a, 0), H - 1), min(max(u + b, 0), W - 1)
                        D += abs(int(p[y, x]) - int(current[y, x]))
                assert 0 <= D <= 2295
                w = max(0, S - D)
                tot += w
                n += w * int(p[v, u])
            assert tot <= 2880 and n + tot // 2 < 1 << 20
            out[v, u] = (n + tot // 2) // tot
    return out


@pytest.mark.parametrize("quarter", dc.UNITS)
@pytest.mark.parametrize("case", dc.SMALL, ids=dc.case_id)
def test_scalar_restatement(case, quarter):
    cur, preds = dc.current(case), dc.predictions(case, quarter)
    moved = 0
    for R in dc.REFS:
        for strength in dc.STRENGTHS:
            got = dc.want(case, R, strength, quarter)
            assert got.dtype == np.uint8 and got.shape == cur.shape
            assert np.array_equal(got, scalar(cur, preds[:R], strength)), (R, strength)
            moved += int((got != cur).sum())
    assert moved > 0, "the case never weighs a reference"
    # frame is blend over the overlapped predictions by the negated fields
    assert np.array_equal(denoise.frame(cur, dc.refs(case)[:3], dc.fields(case, quarter)[:3], case[1], quarter, 24), dc.want(case, 3, 24, quarter))
    f = dc.fields(case, quarter)[0]
    assert np.array_equal(dc.predictions(case, quarter)[0], obmc.compensate(dc.refs(case)[0], -f.astype(np.int64), case[1], quarter))


def test_prediction_follows_a_field_anchored_at_the_current_frame():
    """A reference that is the current frame moved by (3, 2): the search from the current frame finds (3, 2) (column, row), and the
    prediction by that field gives the blocks of the current frame back (40 x 56 frames: every displaced block lies inside)."""
    canvas = np.random.default_rng(5).integers(0, 256, size=(60, 80), dtype=np.uint8)
    cur, ref = np.ascontiguousarray(canvas[10:50, 10:66]), np.ascontiguousarray(canvas[8:48, 7:63])      # cur(y, x) = ref(y + 2, x + 3)
    f = np.asarray(gme_oracle.get_motion_field(cur, ref, 16, 4, 0, 0), np.int32)
    assert np.all(f == (3, 2))
    pred = denoise.predict(ref, f, 16)
    assert np.array_equal(pred[:32, :48], cur[:32, :48])
    assert np.array_equal(denoise.predict(ref, 4 * f, 16, quarter=True), pred)


def test_properties():
    case = dc.CASES[3]
    cur, preds = dc.current(case), dc.predictions(case, False)
    for strength in dc.STRENGTHS:
        S = 9 * strength
        # out = current where every weight is 0
        got = dc.want(case, 4, strength, False)
        dead = np.ones(cur.shape, bool)
        for p in preds:
            dead &= denoise.window_sad(p, cur) >= S
        assert dead.any() and np.array_equal(got[dead], cur[dead])
        # out = current where every prediction equals current
        for R in dc.REFS:
            assert np.array_equal(denoise.blend(cur, [cur] * R, strength), cur)
        # the order of the references does not matter
        for order in ((3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1)):
            assert np.array_equal(denoise.blend(cur, [preds[k] for k in order], strength), got)
    assert not np.array_equal(dc.want(case, 4, 64, False), cur)
    inverse = 255 - cur
    assert np.array_equal(denoise.blend(cur, [inverse] * 4, 1), cur)


def test_reciprocal_is_exact():
    """(n M) >> 32 == n // tot with M = ceil(2^32 / tot) for every tot in 9 .. 2880, at n = k tot and n = k tot - 1 for k = 1 .. 256,
    at n = 0 and at the largest numerator 255 tot + tot // 2, with denoise.py's copy of the formula (the library exports no helper
    of its own)."""
    k = np.arange(1, 257, dtype=np.int64)
    for tot in range(9, 2881):
        M = denoise.reciprocal(tot)
        assert 0 < M < 1 << 32
        n = np.concatenate([k * tot, k * tot - 1, [0, 255 * tot + tot // 2]])
        assert n.max() < 1 << 20
        assert np.array_equal(denoise.divide(n, M), n // tot), tot


def test_argument_and_shape_errors():
    c = np.zeros((20, 30), np.uint8)
    f = np.zeros((2, 3, 2), np.int32)
    assert denoise.blend(c, [c], 1).shape == (20, 30) and denoise.frame(c, [c] * 4, [f] * 4, 8, False, 64).shape == (20, 30)
    for R in (0, 5):
        with pytest.raises(ValueError):
            denoise.blend(c, [c] * R, 24)
        with pytest.raises(ValueError):
            denoise.frame(c, [c] * R, [f] * R, 8)
    for strength in (0, 65, -1):
        with pytest.raises(ValueError):
            denoise.blend(c, [c], strength)
        with pytest.raises(ValueError):
            denoise.frame(c, [c], [f], 8, False, strength)
    with pytest.raises(ValueError):
        denoise.blend(c, [c[:10]], 24)
    with pytest.raises(ValueError):
        denoise.frame(c, [c, c], [f], 8)
    for B in (3, 65):                                               # the block and shape rules of obmc.py
        with pytest.raises(ValueError):
            denoise.frame(c, [c], [f], B)
    with pytest.raises(ValueError):
        denoise.frame(c[:7], [c[:7]], [np.zeros((0, 3, 2), np.int32)], 8)
    for bad in (np.zeros((2, 3), np.int32), np.zeros((3, 3, 2), np.int32), np.zeros((2, 3, 2), np.float32)):
        with pytest.raises(ValueError):
            denoise.frame(c, [c], [bad], 8)
    with pytest.raises(TypeError):
        denoise.blend(c.astype(np.int16), [c], 24)
    for radius in (0, 3):
        with pytest.raises(ValueError):
            denoise.check_radius(radius)
        with pytest.raises(ValueError):
            denoise.clip(np.zeros((5, 20, 30), np.uint8), radius=radius)
    for n, fd in ((1, 1), (3, 2), (5, 0)):                          # a frame without any reference; no distance
        with pytest.raises(ValueError):
            denoise.clip(np.zeros((n, 20, 30), np.uint8), frame_distance=fd)
    assert denoise.references(0, 5, 1, 2) == [1, 2] and denoise.references(2, 5, 1, 2) == [1, 3, 0, 4]
    assert denoise.references(4, 5, 2, 1) == [2] and denoise.references(1, 5, 1, 2) == [0, 2, 3]
    assert denoise.DEFAULT_STRENGTH == 24 and "not a tuned value" in denoise.__doc__


def scene(seed=2026, frames=5, shape=(96, 128), step=(3, 2), sigma=10.0):
    """A smooth textured canvas (low-pass filtered noise, stretched to 16 .. 239) seen through a window that moves by `step`
    (columns, rows) a frame -> (clean uint8[frames, H, W], noisy: clean plus seeded Gaussian noise, rounded and clipped)."""
    rng = np.random.default_rng(seed)
    H, W = shape
    ch, cw = H + step[1] * frames + 8, W + step[0] * frames + 8
    fy, fx = np.fft.fftfreq(ch)[:, None], np.fft.fftfreq(cw)[None, :]
    canvas = np.real(np.fft.ifft2(np.fft.fft2(rng.normal(size=(ch, cw))) * np.exp(-(fx * fx + fy * fy) * 300.0)))
    canvas = 16.0 + (canvas - canvas.min()) / (canvas.max() - canvas.min()) * 223.0
    clean = np.stack([np.rint(canvas[4 + step[1] * t:4 + step[1] * t + H, 4 + step[0] * t:4 + step[0] * t + W]) for t in range(frames)])
    noisy = np.clip(np.rint(clean + rng.normal(scale=sigma, size=clean.shape)), 0, 255)
    return clean.astype(np.uint8), noisy.astype(np.uint8)


def test_what_it_achieves():
    """A scene that moves by (3, 2) pixels a frame, five frames of 96 x 128, Gaussian noise of sigma 10, exhaustive MAE at B 16 and
    sw 8, strength 32, the middle frame as the target.  Squared error against the clean frame, strictly ordered: noisy > one
    reference > two > four; the filter on the two uncompensated neighbours lands strictly above the two-reference result.
    Measured on the CPU: 1.236 M, 0.679 M, 0.466 M, 0.324 M, and 0.787 M uncompensated.  The orderings are the conditions; the
    values are printed, not pinned."""
    clean, noisy = scene()
    t = 2
    order = (1, 3, 0, 4)
    fields = [np.asarray(gme_oracle.get_motion_field(noisy[t], noisy[k], 16, 8, 0, 0), np.int32) for k in order]
    err = {"noisy": denoise.sse(noisy[t], clean[t])}
    for R in (1, 2, 4):
        err[R] = denoise.sse(denoise.frame(noisy[t], [noisy[k] for k in order[:R]], fields[:R], 16, False, 32), clean[t])
    err["uncompensated"] = denoise.sse(denoise.blend(noisy[t], [noisy[1], noisy[3]], 32), clean[t])
    print("squared error against the clean frame: noisy %d, one reference %d, two %d, four %d; two uncompensated %d"
          % (err["noisy"], err[1], err[2], err[4], err["uncompensated"]))
    assert err["noisy"] > err[1] > err[2] > err[4], err
    assert err["uncompensated"] > err[2], err


def test_abi_declares_the_denoise_entries():
    import _gme_native
    lib = _gme_native.load_library()
    header = open(os.path.join(REPO, "include", "gme_hip.h")).read()
    for name in ("gme_denoise_u8", "gme_seq_denoise"):
        assert name in _gme_native.exported_symbols() and hasattr(lib, name) and name + "(" in header
    assert len(_gme_native._SIGNATURES["gme_denoise_u8"][1]) == 14 and len(_gme_native._SIGNATURES["gme_seq_denoise"][1]) == 13
