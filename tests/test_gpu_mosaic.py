"""Background mosaic and moving-object masks on the device (k_mosaic_median / k_moving_mask of gme_mosaic.hip through
gme_seq_mosaic, gme_seq_read_mosaic, gme_seq_moving_masks and gme_seq_read_masks_range) against the host definition
mosaic.py: bit for bit, a known moving object under the true and the estimated path, real frames, the error paths and the
CLI.  Needs an MI355X."""
import json

import numpy as np
import pytest

from test_direct_host import corner_error
from test_gpu_stabilize import degenerate_warps, random_warps
from test_mosaic_host import IDENT, pan_frames, pan_warps

pytestmark = pytest.mark.gpu

# synth.frame: frame t shows the canvas at (x - 5 t, y + 3 t), so a pixel of frame p + 1 lies at (u - 5, v + 3) in frame p
SYNTH_PAIR = np.array([1, 0, -5, 0, 1, 3, 0, 0], np.float64)
# test_known_object_true_path's floor: mosaic.py on the CPU gave IoU min 0.882424 (frame 39), mean 0.967059; less 0.05
IOU_TRUE_MIN = 0.882424
# test_known_object_estimated_path: what the estimated path lost against the true one when first measured on the MI355X
# (true-path IoU minus estimated-path IoU, mean and minimum over the 40 frames), per estimator; asserted at 1.5 times that
IOU_GAP = {"projective": (0.000447, 0.002916), "affine": (0.002352, 0.002655)}
# test_real_frames: pairs of g9 whose frame the mosaic predicts better than the previous frame does (mosaic.py, CPU, fed the
# device's pair warps): 21 of 50 when first counted, under half, which DESIGN.md section 7d reports as a finding about the
# chained path on this clip; asserted less 3
G9_BEATS = 21


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


@pytest.fixture(scope="module")
def g9(golden):
    return np.ascontiguousarray(golden("g9_pan240seq")["frames"])


def sequence_of(native, frames):
    return native.Sequence.from_frames(native.default_context(), np.ascontiguousarray(frames, dtype=np.uint8))


def device_equals_host(native, frames, pl, fill=0, threshold=16, min_count=3):
    """Sprite, count, masks, known and moving of the device, with and without the cull, against mosaic.py -> the host's."""
    import mosaic
    usable = np.asarray(pl["flags"]) == 0
    sprite, count = mosaic.build(frames, pl, fill)
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count, threshold, min_count)
    seq = sequence_of(native, frames)
    for cull in (True, False):
        seq.mosaic(0, pl["G"], usable, pl["ox"], pl["oy"], pl["Hc"], pl["Wc"], fill, cull)
        s, c = seq.read_mosaic()
        assert c.dtype == np.uint16 and np.array_equal(c, count), "count, cull %d" % cull
        assert np.array_equal(s, sprite), "sprite, cull %d" % cull
    k, m = seq.moving_masks(0, pl["A"], usable, pl["ox"], pl["oy"], threshold, min_count)
    got = seq.read_masks_range(0, len(frames))
    assert np.array_equal(k, known) and np.array_equal(m, moving)
    assert np.array_equal(got, masks)
    assert np.array_equal(seq.read_masks_range(1, 2), masks[1:3])
    seq.close()
    return sprite, count, masks, known, moving


def test_random_frames_random_warps(native):
    """(37, 53) x 9: near-identity and far warps (half a frame away, so most frames miss most of the canvas and the counts run
    from 0 to 9, even and odd); the canvas width is no multiple of 64."""
    import mosaic
    import stabilize
    rng = np.random.default_rng(53)
    H, W, n = 37, 53, 9
    frames = rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
    warps = np.concatenate([IDENT[None], random_warps(rng, 4, H, W), random_warps(rng, 4, H, W, far=True)])
    pl = mosaic.plan_path(stabilize.matrix(warps), H, W)
    assert not pl["flags"].any() and pl["Wc"] % 64 != 0 and pl["Wc"] > W
    for fill, threshold, min_count in ((0, 16, 3), (201, 40, 1)):
        _, count, _, known, _ = device_equals_host(native, frames, pl, fill, threshold, min_count)
    assert count.min() == 0 and count.max() >= 5 and len(np.unique(count)) >= 6 and known.min() > 0


def test_synth_true_path(native):
    import mosaic
    import synth
    n, H, W = 12, 480, 720
    frames = synth.sequence(7, 0, n, H, W)
    pl = mosaic.plan(np.tile(SYNTH_PAIR, (n - 1, 1)), H, W)
    assert (pl["ox"], pl["oy"], pl["Hc"], pl["Wc"]) == (-55, 0, 480 + 33, 720 + 55)
    _, count, masks, _, moving = device_equals_host(native, frames, pl)
    assert count.max() == n and moving.min() > 0


def test_1080_few_frames_subpixel(native):
    """1080 x 1918, four frames under a sub-pixel pan with a little rotation and perspective: real bilinear weights."""
    import mosaic
    import stabilize
    import synth
    n, H, W = 4, 1080, 1918
    frames = synth.sequence(21, 0, n, H, W)
    rng = np.random.default_rng(1918)
    warps = np.concatenate([IDENT[None], random_warps(rng, n - 1, H, W)])
    warps[1:, 2] += [-5.3, -10.6, -15.2]
    warps[1:, 5] += [3.4, 6.1, 9.7]
    pl = mosaic.plan_path(stabilize.matrix(warps), H, W)
    device_equals_host(native, frames, pl, min_count=2)


def test_degenerate_warps_among_usable_ones(native):
    """The warps random_warps never makes (edge taps, mirrors, d <= 0, d == 0 on a row, non-finite entries), each given to
    the device as a usable frame's G and A beside three ordinary frames, on a canvas larger than the frame."""
    H, W = 48, 64
    rng = np.random.default_rng(6)
    deg = degenerate_warps(H, W)
    names = sorted(deg)
    warps = np.array([deg[k][0] for k in names], np.float64)
    n = len(warps) + 3
    frames = rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
    frames[-3:] = frames[-3]                                  # three identical ordinary frames: a background to be known
    G = np.concatenate([warps, np.tile(IDENT, (3, 1))])
    pl = {"A": G.copy(), "G": G, "ox": -9, "oy": -5, "Hc": H + 11, "Wc": W + 20, "flags": np.zeros(n, np.int32)}
    _, count, _, known, _ = device_equals_host(native, frames, pl, fill=9, min_count=3)
    assert count.max() >= 5 and known[-1] > 0
    pl["flags"][[1, 4, n - 1]] = 1                            # and with some of them marked unusable
    _, _, masks, known, _ = device_equals_host(native, frames, pl, fill=9, min_count=2)
    assert not masks[[1, 4, n - 1]].any() and not known[[1, 4, n - 1]].any()


def test_cull_extremes(native):
    """A fast pan of small frames (each frame covers under a tenth of the canvas: the cull drops most frames at most row
    segments) and a standing camera (every frame covers every segment: it drops none); more than 64 frames, so the frame
    loop runs a second batch."""
    import mosaic
    n, H, W = 70, 40, 64
    frames, _ = pan_frames(13, n, H, W, 21, 3)
    pl = mosaic.plan(pan_warps(n, 21, 3), H, W, max_canvas_pixels=10 ** 7)
    assert pl["Wc"] == W + 69 * 21 and H * W * 10 < pl["Hc"] * pl["Wc"]
    _, count, _, _, _ = device_equals_host(native, frames, pl)
    assert count.max() == 4
    rng = np.random.default_rng(2)
    still = rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
    pl = mosaic.plan(np.tile(IDENT, (n - 1, 1)), H, W)
    _, count, _, _, _ = device_equals_host(native, still, pl)
    assert np.all(count == n)


def object_iou(masks, H, W):
    """Per-frame IoU of the masks against the footprint of synth.frame's foreground rectangle (its rows x cols)."""
    out = np.empty(len(masks))
    rh, rw = H // 4, W // 6
    for t in range(len(masks)):
        rows = (H // 3 + 4 * t + np.arange(rh)) % H
        cols = (W // 3 - 7 * t + np.arange(rw)) % W
        truth = np.zeros((H, W), bool)
        truth[rows[:, None], cols[None, :]] = True
        m = masks[t].astype(bool)
        out[t] = float((m & truth).sum()) / float((m | truth).sum())
    return out


@pytest.fixture(scope="module")
def known_object(native):
    """480 x 720 x 40 synth frames of seed 5 and the host definition's masks under the true path."""
    import mosaic
    import synth
    n, H, W = 40, 480, 720
    frames = synth.sequence(5, 0, n, H, W)
    pl = mosaic.plan(np.tile(SYNTH_PAIR, (n - 1, 1)), H, W)
    sprite, count = mosaic.build(frames, pl)
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count, 16, 3)
    return frames, pl, masks, object_iou(masks, H, W)


def test_known_object_true_path(native, known_object):
    """The device's masks under the true integer path equal the host definition's, and so does their IoU against the
    rectangle's known footprint, every frame kept (the wrap-around frames 35 .. 39 too).  The host definition on the CPU:
    IoU min 0.882424 (frame 39, whose object region few frames have seen), mean 0.967059; the floor is that minimum less
    0.05, slack for a later change of the seed or the frame count here, not for the device."""
    import sequence
    frames, pl, masks, iou_host = known_object
    n, H, W = frames.shape
    sh = sequence.ShardedSequence(H, W, n, 1)
    sh.load(frames)
    res = sh.mosaic(h=np.tile(SYNTH_PAIR, (n - 1, 1)), threshold=16, min_count=3)
    got = sh.read_masks_range(0, n)
    sh.close()
    iou = object_iou(got, H, W)
    print("known object, true path: IoU min %.6f (frame %d) mean %.6f; host min %.6f mean %.6f"
          % (iou.min(), iou.argmin(), iou.mean(), iou_host.min(), iou_host.mean()))
    assert (res["ox"], res["oy"], res["Hc"], res["Wc"]) == (pl["ox"], pl["oy"], pl["Hc"], pl["Wc"])
    assert np.array_equal(got, masks)
    assert np.array_equal(iou, iou_host)
    assert iou.min() >= IOU_TRUE_MIN - 0.05


@pytest.mark.parametrize("estimator", ["projective", "affine"])
def test_known_object_estimated_path(native, known_object, estimator):
    """The same video through ShardedSequence.mosaic with the path estimated from the frames.  Measured against the true
    path's IoU (test_known_object_true_path): the estimate may lose what its drift over 39 chained pairs costs and no more.
    The gap first measured on the MI355X is IOU_GAP (DESIGN.md section 7d has the figures and the path's corner error); the
    bound is that gap plus half of it again, for a later harmless change of the estimator's last bits."""
    import sequence
    import stabilize
    frames, pl, _, iou_true = known_object
    n, H, W = frames.shape
    sh = sequence.ShardedSequence(H, W, n, 1)
    sh.load(frames)
    res = sh.mosaic(estimator=estimator, threshold=16, min_count=3)
    got = sh.read_masks_range(0, n)
    sh.close()
    iou = object_iou(got, H, W)
    C, true_C = stabilize.trajectory(res["h"]), stabilize.trajectory(np.tile(SYNTH_PAIR, (n - 1, 1)))
    err = max(corner_error(stabilize.params(C[t]), stabilize.params(true_C[t]), H, W) for t in range(n))
    gap_mean, gap_min = iou_true.mean() - iou.mean(), iou_true.min() - iou.min()
    print("known object, %s path: IoU min %.6f (frame %d) mean %.6f; gap to the true path mean %.6f min %.6f; worst corner "
          "error of the path %.4f px; canvas %d x %d at (%d, %d); unusable frames %d"
          % (estimator, iou.min(), iou.argmin(), iou.mean(), gap_mean, gap_min, err, res["Hc"], res["Wc"], res["ox"], res["oy"],
             int(res["flags"].sum())))
    assert not res["flags"].any()
    assert gap_mean <= 1.5 * IOU_GAP[estimator][0]
    assert gap_min <= 1.5 * IOU_GAP[estimator][1]


def psnr_over(a, b, where):
    d = a.astype(np.float64)[where] - b.astype(np.float64)[where]
    mse = float(np.mean(d * d))
    return 99.0 if mse == 0.0 else 10.0 * np.log10(255.0 * 255.0 / mse)


def test_real_frames(native, g9):
    """g9 (51 frames of the pan240 clip): every frame usable, a canvas wider than the frame, counts within 1 .. 51 on frame
    0's footprint, device equal to the host definition fed the device's pair warps, and the mosaic predicts a frame better
    than the previous frame does (PSNR over the known pixels) on G9_BEATS = 21 of the 50 pairs, asserted less 3.  That is
    fewer than half: on this clip the path chained over 50 pairs does not hold the background still to within a pixel, and
    26.6 % of the known pixels come out as moving; the bound records what is, it is not a target."""
    import mosaic
    import sequence
    n, H, W = g9.shape
    sh = sequence.ShardedSequence(H, W, n, 1)
    sh.load(g9)
    res = sh.mosaic()
    sprite, count = sh.read_mosaic()
    masks = sh.read_masks_range(0, n)
    sh.close()
    assert n == 51 and not res["flags"].any() and res["Wc"] > W
    assert count.max() <= 51
    assert count[-res["oy"]:-res["oy"] + H, -res["ox"]:-res["ox"] + W].min() >= 1
    pl = mosaic.plan(res["h"], H, W)
    s, c = mosaic.build(g9, pl)
    assert np.array_equal(s, sprite) and np.array_equal(c, count)
    m, known, moving = mosaic.moving_masks(g9, pl, s, c)
    assert np.array_equal(m, masks) and np.array_equal(known, res["known"]) and np.array_equal(moving, res["moving"])
    beats = 0
    for t in range(1, n):
        kn, _, b = mosaic.residuals(g9[t], pl["A"][t], s, c, pl["ox"], pl["oy"], 3)
        assert kn.any()
        beats += psnr_over(g9[t], b, kn) > psnr_over(g9[t], g9[t - 1], kn)
    print("g9: canvas %d x %d at (%d, %d), count max %d, known %.1f %% of the pixels, moving %.2f %% of the known; the mosaic "
          "beats the previous frame on %d of 50 pairs"
          % (res["Hc"], res["Wc"], res["ox"], res["oy"], count.max(), 100.0 * known.sum() / (n * H * W),
             100.0 * moving.sum() / max(1, known.sum()), beats))
    assert beats >= G9_BEATS - 3


def test_error_paths(native, g9):
    seq = sequence_of(native, g9[:4])
    ident = np.tile(IDENT, (4, 1))
    with pytest.raises(IndexError, match="no mosaic was built"):
        seq.read_mosaic()
    with pytest.raises(IndexError, match="no mosaic was built"):
        seq.moving_masks(0, ident, None, 0, 0)
    with pytest.raises(IndexError, match="never computed"):
        seq.read_masks_range(0, 1)
    with pytest.raises(IndexError, match="outside"):
        seq.mosaic(2, ident, None, 0, 0, 240, 320)
    with pytest.raises(IndexError, match="outside"):
        seq.mosaic(-1, ident[:2], None, 0, 0, 240, 320)
    with pytest.raises(IndexError, match="canvas"):
        seq.mosaic(0, ident, None, 0, 0, 0, 320)
    with pytest.raises(IndexError, match="canvas"):
        seq.mosaic(0, ident, None, 0, 0, 1 << 16, 1 << 16)
    with pytest.raises(IndexError, match="fill"):
        seq.mosaic(0, ident, None, 0, 0, 240, 320, 256)
    seq.mosaic(0, ident, None, 0, 0, 240, 320)
    with pytest.raises(IndexError, match="threshold"):
        seq.moving_masks(0, ident, None, 0, 0, 256, 3)
    with pytest.raises(IndexError, match="threshold"):
        seq.moving_masks(0, ident, None, 0, 0, -1, 3)
    with pytest.raises(IndexError, match="min_count"):
        seq.moving_masks(0, ident, None, 0, 0, 16, 0)
    with pytest.raises(IndexError, match="outside"):
        seq.moving_masks(1, ident, None, 0, 0)
    seq.moving_masks(0, ident[:2], None, 0, 0)
    with pytest.raises(IndexError, match="never computed"):
        seq.read_masks_range(1, 2)
    with pytest.raises(IndexError, match="outside"):
        seq.read_masks_range(3, 2)
    assert seq.read_masks_range(0, 2).shape == (2, 240, 320)
    sprite, count = seq.read_mosaic()
    assert sprite.shape == (240, 320) and np.all(count == 4)
    seq.close()


def test_cli_mosaic(native, g9, tmp_path, capsys):
    import gme_cli
    from PIL import Image
    np.save(tmp_path / "clip.npy", g9)
    res = gme_cli.main(["mosaic", "-p", str(tmp_path / "clip.npy"), "-o", str(tmp_path / "out")])
    assert "canvas" in capsys.readouterr().out
    rec = json.loads((tmp_path / "out" / "mosaic.json").read_text())
    assert rec["frames"] == 51 and rec["size"] == [res["Hc"], res["Wc"]] and rec["origin"] == [res["ox"], res["oy"]]
    assert len(rec["pair_params"]) == 50 and len(rec["frame_flags"]) == 51 and rec["known"] == res["known"].tolist()
    assert rec["moving"] == res["moving"].tolist()
    sprite = np.asarray(Image.open(tmp_path / "out" / "mosaic.png"))
    assert sprite.shape == (res["Hc"], res["Wc"])
    pngs = sorted((tmp_path / "out" / "masks").glob("*.png"))
    assert len(pngs) == 51 and pngs[0].name == "0000.png"
    m7 = np.asarray(Image.open(pngs[7]))
    assert set(np.unique(m7)) <= {0, 255} and int((m7 == 255).sum()) == rec["moving"][7]
    gme_cli.main(["mosaic", "-p", str(tmp_path / "clip.npy"), "-o", str(tmp_path / "out2"), "--no-masks", "--estimator", "affine"])
    assert not (tmp_path / "out2" / "masks").exists() and json.loads((tmp_path / "out2" / "mosaic.json").read_text())["known"] is None
