"""The host definition of motion-compensated frame interpolation (interp.py): argument rules, the definition against a block
written straight from its wording, the pan scene, the stripes that pin scan order and bias, constant frames, window 0, the
interleaving of upconvert, and a real pair.  No GPU."""
import numpy as np
import pytest

import interp
import interp_cases as ic


def test_check_args():
    assert interp.check_args(16, 8, 0, 16) == (16, 8, 0, 16)
    assert interp.check_args(4, 0, 1, 0) == (4, 0, 1, 0)
    assert interp.check_args(64, 8, 1, 1 << 16) == (64, 8, 1, 1 << 16)
    for bad in ((3, 1, 0, 0), (65, 1, 0, 0), (0, 1, 0, 0), (16, -1, 0, 0), (16, 9, 0, 0), (16, 1, 2, 0), (16, 1, -1, 0), (16, 1, 0, -1),
                (16, 1, 0, (1 << 16) + 1)):
        with pytest.raises(ValueError):
            interp.check_args(*bad)
        with pytest.raises(ValueError):
            interp.search(np.zeros((64, 64), np.uint8), np.zeros((64, 64), np.uint8), *bad)
    z = np.zeros((16, 20), np.uint8)
    for small in (np.zeros((15, 20), np.uint8), np.zeros((20, 15), np.uint8)):           # H >= B and W >= B
        with pytest.raises(ValueError):
            interp.search(small, small, 16, 1, 0, 0)
    with pytest.raises(TypeError):
        interp.search(z, z.astype(np.int16), 16, 1, 0, 0)
    with pytest.raises(TypeError):
        interp.search(z, z[:, :16], 16, 1, 0, 0)
    with pytest.raises(ValueError):
        interp.interpolate(z, z, np.zeros((2, 1, 2), np.int32), 16)
    # the largest J
    assert 64 * 64 * 255 * 255 + (1 << 16) * (8 + 8) < 1 << 31
    assert interp.default_bias(16, 0) == 16 and interp.default_bias(16, 1) == 256 and interp.default_bias(8, 0) == 4


def brute(past, nxt, bs, sw, pnorm, bias, i, j):
    """One block straight from the definition's wording, written apart from interp.search -> (v, J, D)."""
    H, W = past.shape

    def S(f, x, y):
        return int(f[min(max(y, 0), H - 1), min(max(x, 0), W - 1)])

    def D(vx, vy):
        total = 0
        for y in range(i * bs, i * bs + bs):
            for x in range(j * bs, j * bs + bs):
                d = S(past, x - vx, y - vy) - S(nxt, x + vx, y + vy)
                total += abs(d) if pnorm == 0 else d * d
        return total
    best = ((0, 0), D(0, 0), D(0, 0))
    for ox in range(-sw, sw + 1):
        for oy in range(-sw, sw + 1):
            if (ox, oy) != (0, 0):
                d = D(ox, oy)
                if d + bias * (abs(ox) + abs(oy)) < best[1]:
                    best = ((ox, oy), d + bias * (abs(ox) + abs(oy)), d)
    return best


@pytest.mark.parametrize("case", (ic.NOISE[0], ic.NOISE[1], ic.NOISE[8]))
def test_search_is_the_definition(case):
    """interp.search (whole-frame array arithmetic) against the block-by-block wording on small noise cases, and interpolate
    against its per-pixel wording: border blocks clamp on every side."""
    shape, bs, sw = case
    past, _, nxt = ic.noise_pair(case)
    H, W = shape
    for pnorm in (0, 1):
        for bias in ic.noise_biases(case, pnorm):
            mv, cost, dist, made = ic.result(case, pnorm, bias)
            assert mv.dtype == np.int32 and cost.dtype == np.int64 and dist.dtype == np.int64 and made.dtype == np.uint8
            assert mv.shape == (H // bs, W // bs, 2) and cost.shape == dist.shape == mv.shape[:2] and made.shape == shape
            for i in range(H // bs):
                for j in range(W // bs):
                    v, J, D = brute(past, nxt, bs, sw, pnorm, bias, i, j)
                    assert (tuple(mv[i, j]), cost[i, j], dist[i, j]) == (v, J, D), (case, pnorm, bias, i, j)
            assert np.array_equal(cost, dist + bias * np.abs(mv).sum(axis=2))
            for y in range(H):
                for x in range(W):
                    vx, vy = mv[y // bs, x // bs] if y // bs < H // bs and x // bs < W // bs else (0, 0)
                    p = int(past[min(max(y - vy, 0), H - 1), min(max(x - vx, 0), W - 1)])
                    n = int(nxt[min(max(y + vy, 0), H - 1), min(max(x + vx, 0), W - 1)])
                    assert made[y, x] == (p + n + 1) >> 1, (case, y, x)


@pytest.mark.parametrize("pnorm", (0, 1))
def test_pan_scene(pnorm):
    """A pan of (3, -2) per frame under noise of +-4, blocks of 16, window 6, the default bias: every block carries the pan
    (the border blocks too: the replicated border costs less than any other vector), and the interpolated frame is closer to
    the true middle frame than the plain average (31.1 against 15.4 dB at the seed in use)."""
    past, mid, nxt = ic.pan_scene()
    bias = interp.default_bias(ic.PAN_BLOCK, pnorm)
    mv, cost, dist, made = ic.result("pan", pnorm, bias)
    assert mv.shape == (5, 7, 2)
    assert np.all(mv[1:-1, 1:-1] == ic.PAN_MOVE), mv[:, :, 0]
    assert np.all(mv == ic.PAN_MOVE), mv[:, :, 0]
    made_sse, average_sse = interp.sse(made, mid), interp.sse(interp.average(past, nxt), mid)
    print("pan scene norm %d: interpolation %.2f dB, average %.2f dB" % (pnorm, interp.psnr(made_sse, *ic.PAN_SHAPE),
                                                                         interp.psnr(average_sse, *ic.PAN_SHAPE)))
    assert made_sse < average_sse


@pytest.mark.parametrize("pnorm", (0, 1))
def test_stripes_pin_order_and_bias(pnorm):
    """Stripes of period 8 moving one column per frame: D is zero at vx = 1 and, the pattern repeating, at vx = -7 for every vy.
    Without a bias the scan order decides: the first zero in it is (-7, -8); in the last block column the clamped border leaves
    (-3, -8), in the first one (1, -8).  A bias of 1 makes (1, 0) the only minimum everywhere."""
    mv, cost, dist, _ = ic.result("stripes", pnorm, 0)
    assert mv.shape == (4, 6, 2) and not cost.any() and not dist.any()
    assert np.all(mv[:, 1:5] == (-7, -8)) and np.all(mv[:, 5] == (-3, -8)) and np.all(mv[:, 0] == (1, -8)), mv
    mv, cost, dist, made = ic.result("stripes", pnorm, 1)
    assert np.all(mv == (1, 0)) and np.all(cost == 1) and not dist.any()
    # the frame between the two over the whole blocks: the stripes moved by one column
    x = np.arange(48)
    assert np.array_equal(made[:32, :48], np.tile(np.where(((x + 1) % 8) < 4, 40, 200), (32, 1)))


def test_constant_frames_and_window_zero():
    past, nxt = np.full((37, 53), 90, np.uint8), np.full((37, 53), 97, np.uint8)
    for pnorm, d in ((0, 7), (1, 49)):
        for bias in (0, 5):
            mv, cost, dist = interp.search(past, nxt, 8, 4, pnorm, bias)
            assert not mv.any() and np.array_equal(cost, dist) and np.all(dist == 64 * d)
            assert np.all(interp.interpolate(past, nxt, mv, 8) == 94)                  # (90 + 97 + 1) >> 1
    past, _, nxt = ic.noise_pair(ic.NOISE[3])
    for pnorm in (0, 1):
        mv, cost, dist, made = ic.result(ic.NOISE[3], pnorm, 16)
        assert ic.NOISE[3][2] == 0 and not mv.any() and np.array_equal(cost, dist)
        d = past.astype(np.int64)[:48, :80] - nxt.astype(np.int64)[:48, :80]
        assert np.array_equal(dist, (np.abs(d) if pnorm == 0 else d * d).reshape(3, 16, 5, 16).sum(axis=(1, 3)))
        assert np.array_equal(made, interp.average(past, nxt))
        assert np.array_equal(made, ((past.astype(np.uint16) + nxt + 1) >> 1).astype(np.uint8))


def test_upconvert_interleaves(monkeypatch):
    """upconvert with the device call replaced by the host functions: the originals at the even indices, between them the
    frame interpolated from the two neighbours, from one call at frame distance 1."""
    frames = np.random.default_rng(9).integers(0, 256, size=(4, 24, 40), dtype=np.uint8)
    calls = []

    def host(frames, fd, bs, sw, pnorm, bias):
        calls.append((fd, bs, sw, pnorm, bias))
        fields = [interp.search(frames[k], frames[k + fd], bs, sw, pnorm, bias) for k in range(len(frames) - fd)]
        made = np.stack([interp.interpolate(frames[k], frames[k + fd], f[0], bs) for k, f in enumerate(fields)])
        return (np.stack([f[0] for f in fields]), np.stack([f[1] for f in fields]), np.stack([f[2] for f in fields]), made,
                np.full(len(fields), -1, np.int64))
    monkeypatch.setattr(interp, "_interp_sequence", host)
    out = interp.upconvert(frames, block_size=8, search_window=2, pnorm_distance=1)
    assert calls == [(1, 8, 2, 1, 64)]
    assert out.dtype == np.uint8 and out.shape == (7, 24, 40) and np.array_equal(out[0::2], frames)
    for k in range(3):
        mv = interp.search(frames[k], frames[k + 1], 8, 2, 1, 64)[0]
        assert np.array_equal(out[2 * k + 1], interp.interpolate(frames[k], frames[k + 1], mv, 8))
    assert np.array_equal(interp.upconvert(frames[:1], block_size=8), frames[:1]) and len(calls) == 1
    with pytest.raises(ValueError):
        interp.upconvert(frames, block_size=8, search_window=9)
    with pytest.raises(ValueError):
        interp.upconvert(frames, block_size=32)


def test_real_pair(golden):
    """g9 frames 10 and 12 interpolate frame 11 at the defaults (blocks of 16, window 8, MAE, bias 16): closer to the true frame
    than the plain average."""
    g9 = golden("g9_pan240seq")["frames"]
    past, mid, nxt = (np.ascontiguousarray(g9[k]) for k in (10, 11, 12))
    mv, cost, dist = interp.search(past, nxt, 16, 8, 0, interp.default_bias(16, 0))
    made_sse, average_sse = interp.sse(interp.interpolate(past, nxt, mv, 16), mid), interp.sse(interp.average(past, nxt), mid)
    s = interp.summary(mv, *mid.shape, made_sse, average_sse)
    print("g9 pair (10, 12): interpolation %.2f dB, average %.2f dB, median vector %s, %.0f %% of the vectors non-zero"
          % (s["psnr_interp"], s["psnr_average"], s["median_vector"], 100.0 * s["nonzero_share"]))
    assert made_sse < average_sse
