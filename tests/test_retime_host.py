"""The host definition of frame interpolation at any phase (retime.py) against interp.py where the two meet, its offsets, the
pan whose intermediate frames are known exactly, constant, saturated and striped content, the schedule of a rate conversion,
the argument rules and the ABI.  No device."""
import os
from math import gcd

import numpy as np
import pytest

import interp
import retime
import retime_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_halfway_distortion_is_interp_at_half_the_vector():
    """At phase 1/2 an even displacement V = 2 v reads whole pixels: `past` at p - v and `next` at p + v, the difference
    interp.search scores at v."""
    rng = np.random.default_rng(11)
    past, nxt = rng.integers(0, 256, size=(2, 37, 53), dtype=np.uint8)
    H, W = past.shape
    y, x = np.mgrid[0:H, 0:W]
    for vx, vy in ((0, 0), (1, -2), (-3, 2), (4, 4)):
        want = (past[np.clip(y - vy, 0, H - 1), np.clip(x - vx, 0, W - 1)].astype(np.int64)
                - nxt[np.clip(y + vy, 0, H - 1), np.clip(x + vx, 0, W - 1)].astype(np.int64))
        got = retime.distortion(past, nxt, (2 * vx, 2 * vy), 1, 2)
        assert got.dtype == np.int64 and np.array_equal(got, want), (vx, vy)
        # ... which is what interp.search sums: one block over the whole frame's whole blocks, that vector alone
        d8 = np.abs(want)[:32, :48].reshape(4, 8, 6, 8).sum(axis=(1, 3))
        pp, nn = np.pad(past.astype(np.int64), 8, mode="edge"), np.pad(nxt.astype(np.int64), 8, mode="edge")
        ref = np.abs(interp._shifted(pp, 8, H, W, -vx, -vy) - interp._shifted(nn, 8, H, W, vx, vy))[:32, :48].reshape(4, 8, 6, 8).sum(axis=(1, 3))
        assert np.array_equal(d8, ref)


def test_halfway_frame_is_interp_under_the_halved_field():
    rng = np.random.default_rng(12)
    past, nxt = rng.integers(0, 256, size=(2, 37, 53), dtype=np.uint8)
    half = rng.integers(-8, 9, size=(4, 6, 2)).astype(np.int32)
    assert np.array_equal(retime.interpolate(past, nxt, 2 * half, 8, 1, 2), interp.interpolate(past, nxt, half, 8))
    assert np.array_equal(retime.interpolate(past, nxt, 2 * half, 8, 3, 6), interp.interpolate(past, nxt, half, 8))
    assert np.array_equal(retime.crossfade(past, nxt, 1, 2), interp.average(past, nxt))
    assert np.array_equal(retime.interpolate(past, nxt, 0 * half, 8, 2, 5), retime.crossfade(past, nxt, 2, 5))


def test_offsets():
    V = np.arange(-16, 17)
    for d in range(2, 65):
        for n in range(1, d):
            if gcd(n, d) != 1:
                continue
            a, b = retime.offsets(V, n, d)
            assert np.array_equal(b - a, 4 * V) and np.array_equal(a & 3, b & 3), (n, d)
            # -4 n V / d rounded to the nearest quarter, halves up
            assert np.array_equal(a, -np.floor(4.0 * n * V / d + 0.5).astype(np.int64)), (n, d)
    assert [int(retime.offsets(v, 1, 3)[0]) for v in range(-3, 4)] == [4, 3, 1, 0, -1, -3, -4]
    assert [int(retime.offsets(v, 2, 5)[0]) for v in range(-3, 4)] == [5, 3, 2, 0, -2, -3, -5]
    assert retime.check_phase(2, 4) == (1, 2) and retime.check_phase(63, 64) == (63, 64) and retime.check_phase(130, 260) == (1, 2)
    for bad in ((0, 2), (2, 2), (3, 2), (1, 0), (-1, 2), (1, 65), (2, 130 + 1)):
        with pytest.raises(ValueError):
            retime.check_phase(*bad)


@pytest.mark.parametrize("phase", rc.PAN_PHASES)
def test_pan(phase):
    """Noise panned by (12, -6): every interior block takes that vector, and the interior of the made frame is the true
    intermediate frame, byte for byte.  Border blocks clamp and are left out by construction."""
    mv, cost, dist, made = rc.pan_result(phase, 0)
    assert np.all(mv[1:4, 1:6] == rc.PAN_MOVE)
    assert np.all(dist[1:4, 1:6] == 0) and np.all(cost[1:4, 1:6] == rc.PAN_BIAS * 18)
    truth = rc.pan_frame(*phase)
    assert np.array_equal(made[rc.PAN_INTERIOR], truth[rc.PAN_INTERIOR])


def test_constant_frames():
    """Every candidate ties with the centre: V = 0 everywhere, cost == dist, and the frame is the blend of the two levels."""
    past, nxt = rc.flat(90), rc.flat(97)
    for (n, d) in ((1, 2), (1, 3), (5, 6), (63, 64)):
        for pnorm in (0, 1):
            for bias in (0, 5):
                mv, cost, dist, made = rc.host_result(past, nxt, 8, 4, pnorm, bias, n, d)
                assert not mv.any() and np.array_equal(cost, dist) and np.all(dist == 64 * (7 if pnorm == 0 else 49))
                assert np.all(made == ((d - n) * 90 + n * 97 + d // 2) // d)


def test_saturated():
    """Blocks of 64 with 0 against 255 at the largest bias: D is 64^2 255 or 64^2 255^2, the frame the rounded n 255 / d."""
    lo, hi = rc.flat(0, (64, 70)), rc.flat(255, (64, 70))
    for (n, d) in ((1, 2), (2, 5), (63, 64)):
        for pnorm, top in ((0, 64 * 64 * 255), (1, 64 * 64 * 255 * 255)):
            for past, nxt, level in ((lo, hi, (n * 255 + d // 2) // d), (hi, lo, ((d - n) * 255 + d // 2) // d)):
                mv, cost, dist, made = rc.host_result(past, nxt, 64, 2, pnorm, 1 << 16, n, d)
                assert not mv.any() and np.all(cost == top) and np.all(dist == top) and np.all(made == level)
                assert cost.dtype == np.int64 and made.dtype == np.uint8
    assert 64 * 64 * 255 * 255 + (1 << 16) * 32 < 1 << 31


def test_stripes():
    """Vertical stripes of period 8 that move two columns: Vx = 2 + 8 k ties at D = 0 for every Vy where nothing clamps.  Without
    a bias the first of them in scan order wins, (-14, -16); at bias 1 the smallest |V|, (2, 0)."""
    past, nxt = rc.stripes()
    for pnorm in (0, 1):
        mv, cost, dist, _ = rc.host_result(past, nxt, rc.STRIPES_BLOCK, rc.STRIPES_WINDOW, pnorm, 0, *rc.STRIPES_PHASE)
        assert np.all(mv[:, 2:4] == (-14, -16)) and not dist[:, 2:4].any()
        mv, cost, dist, _ = rc.host_result(past, nxt, rc.STRIPES_BLOCK, rc.STRIPES_WINDOW, pnorm, 1, *rc.STRIPES_PHASE)
        assert np.all(mv[:, 1:5] == (2, 0)) and np.all(cost[:, 1:5] == 2) and not dist[:, 1:5].any()


def test_schedule():
    rows = retime.schedule(5, 2, 5)
    assert rows.dtype == np.int32 and rows.shape == (11, 3)
    assert rows.tolist() == [[0, 0, 1], [0, 2, 5], [0, 4, 5], [1, 1, 5], [1, 3, 5], [2, 0, 1], [2, 2, 5], [2, 4, 5], [3, 1, 5], [3, 3, 5],
                             [4, 0, 1]]
    assert retime.schedule(3, 1, 4).tolist() == [[0, 0, 1], [0, 1, 4], [0, 1, 2], [0, 3, 4], [1, 0, 1], [1, 1, 4], [1, 1, 2], [1, 3, 4],
                                                 [2, 0, 1]]
    assert retime.schedule(7, 5, 2).tolist() == [[0, 0, 1], [2, 1, 2], [5, 0, 1]]
    assert retime.schedule(4, 1, 1).tolist() == [[k, 0, 1] for k in range(4)]
    assert retime.schedule(4, 3, 3).tolist() == [[k, 0, 1] for k in range(4)]
    assert retime.schedule(1, 2, 5).tolist() == [[0, 0, 1]]
    assert retime.schedule(3, 2, 128).tolist()[1] == [0, 1, 64]
    for bad in ((3, 1, 65), (3, 1001, 30000), (0, 1, 2), (3, 0, 2), (3, 1, 0)):
        with pytest.raises(ValueError):
            retime.schedule(*bad)
    assert retime.rate_step(24, 60) == (2, 5) and retime.rate_step(25, 30) == (5, 6) and retime.rate_step(60, 24) == (5, 2)
    with pytest.raises(ValueError):
        retime.rate_step(0, 30)


def test_check_args():
    assert retime.check_args(16, 16, 0, 16) == (16, 16, 0, 16)
    assert retime.check_args(4, 0, 1, 0) == (4, 0, 1, 0) and retime.check_args(64, 16, 1, 1 << 16) == (64, 16, 1, 1 << 16)
    z = np.zeros((64, 64), np.uint8)
    for bad in ((3, 1, 0, 0), (65, 1, 0, 0), (0, 1, 0, 0), (16, -1, 0, 0), (16, 17, 0, 0), (16, 1, 2, 0), (16, 1, -1, 0), (16, 1, 0, -1),
                (16, 1, 0, (1 << 16) + 1)):
        with pytest.raises(ValueError):
            retime.check_args(*bad)
        with pytest.raises(ValueError):
            retime.search(z, z, *bad, 1, 2)
    for phase in ((0, 2), (2, 2), (1, 65)):
        with pytest.raises(ValueError):
            retime.search(z, z, 16, 1, 0, 0, *phase)
        with pytest.raises(ValueError):
            retime.interpolate(z, z, np.zeros((4, 4, 2), np.int32), 16, *phase)
    for small in (np.zeros((15, 20), np.uint8), np.zeros((20, 15), np.uint8)):           # H >= B and W >= B
        with pytest.raises(ValueError):
            retime.search(small, small, 16, 1, 0, 0, 1, 2)
    with pytest.raises(TypeError):
        retime.search(z, z.astype(np.int16), 16, 1, 0, 0, 1, 2)
    with pytest.raises(TypeError):
        retime.search(z, z[:, :32], 16, 1, 0, 0, 1, 2)
    with pytest.raises(ValueError):
        retime.interpolate(z, z, np.zeros((2, 1, 2), np.int32), 16, 1, 2)
    assert retime.default_bias(16, 0) == 16 and retime.default_bias(16, 1) == 256
    # the split the tests share is the search itself
    rng = np.random.default_rng(5)
    past, nxt = rng.integers(0, 256, size=(2, 24, 40), dtype=np.uint8)
    mae, mse = retime.block_distortions(past, nxt, 8, 3, 2, 5)
    assert mae.shape == (49, 3, 5) and len(retime.candidates(3)) == 49 and retime.candidates(3)[:2] == [(0, 0), (-3, -3)]
    for got, want in zip(retime.search(past, nxt, 8, 3, 1, 7, 2, 5), retime.select(mse, 3, 7)):
        assert np.array_equal(got, want)
    # ... and its distortions are the block sums of `distortion`, the four-tap sample taken whole
    for c, V in enumerate(retime.candidates(3)):
        e = retime.distortion(past, nxt, V, 2, 5).reshape(3, 8, 5, 8)
        assert np.array_equal(mae[c], np.abs(e).sum(axis=(1, 3))) and np.array_equal(mse[c], (e * e).sum(axis=(1, 3))), V


def test_abi_declares_the_retime_entries():
    import _gme_native
    lib = _gme_native.load_library()
    header = open(os.path.join(REPO, "include", "gme_hip.h")).read()
    for name in ("gme_retime_u8", "gme_retime_clip_u8"):
        assert name in _gme_native.exported_symbols() and hasattr(lib, name) and name + "(" in header
    assert len(_gme_native._SIGNATURES["gme_retime_u8"][1]) == 18 and len(_gme_native._SIGNATURES["gme_retime_clip_u8"][1]) == 18
    assert "gme_seq_retime" not in header
    if lib.gme_device_count() == 0:                                # no device: the calls fail loudly, there is no CPU path
        f = np.zeros((3, 32, 32), np.uint8)
        with pytest.raises(_gme_native.GmeError):
            retime.frame(f[0], f[1], 1, 3)
        with pytest.raises(_gme_native.GmeError):
            retime.slow_motion(f, 2)
        with pytest.raises(_gme_native.GmeError):
            retime.convert(f, 24, 60)
