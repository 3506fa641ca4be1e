"""The host definition of the background mosaic and the moving-object masks (mosaic.py) on cases with
closed-form answers, the surface around it (CLI, ShardedSequence.mosaic's refusals) and the compiler's resource remarks for
the two kernels.  No GPU."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float64)


def pan_warps(n, dx, dy):
    """Pair warps of a camera whose frame t shows the canvas at offset (t dx, t dy): a pixel of frame p + 1 lies at
    (u + dx, v + dy) in frame p."""
    return np.tile(np.array([1, 0, dx, 0, 1, dy, 0, 0], np.float64), (n - 1, 1))


def pan_frames(seed, n, H, W, dx, dy, x0=200, y0=100):
    """Frames cut from synth.canvas at integer offsets, no foreground, no noise; frame t = canvas[y0 + t dy :, x0 + t dx :]."""
    import synth
    T = synth.canvas(seed)
    return np.stack([T[y0 + t * dy:y0 + t * dy + H, x0 + t * dx:x0 + t * dx + W] for t in range(n)]), T


def test_identity_path():
    import mosaic
    import synth
    f = synth.frame(3, 0, 37, 53)
    frames = np.stack([f] * 5)
    pl = mosaic.plan(np.tile(IDENT, (4, 1)), 37, 53)
    assert (pl["ox"], pl["oy"], pl["Hc"], pl["Wc"]) == (0, 0, 37, 53) and not pl["flags"].any()
    sprite, count = mosaic.build(frames, pl)
    assert count.dtype == np.uint16 and np.all(count == 5) and np.array_equal(sprite, f)
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count)
    assert not masks.any() and np.all(known == 37 * 53) and not moving.any()


@pytest.mark.parametrize("dx,dy", [(5, -3), (-4, 2), (7, 0)])
def test_integer_pan_gives_the_canvas_crop(dx, dy):
    import mosaic
    n, H, W = 9, 48, 64
    frames, T = pan_frames(7, n, H, W, dx, dy)
    pl = mosaic.plan(pan_warps(n, dx, dy), H, W)
    # closed form: frame t covers [t dx, t dx + W - 1] x [t dy, t dy + H - 1] in frame-0 coordinates
    ox, oy = min(0, (n - 1) * dx), min(0, (n - 1) * dy)
    assert (pl["ox"], pl["oy"]) == (ox, oy)
    assert (pl["Hc"], pl["Wc"]) == (H + (n - 1) * abs(dy), W + (n - 1) * abs(dx))
    sprite, count = mosaic.build(frames, pl)
    crop = T[100 + oy:100 + oy + pl["Hc"], 200 + ox:200 + ox + pl["Wc"]]
    assert count.max() <= n and count[-oy:-oy + H, -ox:-ox + W].min() >= 1
    assert np.array_equal(sprite[count >= 1], crop[count >= 1])
    assert np.all(sprite[count == 0] == 0)
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count)
    assert not masks.any() and known.min() > 0


def test_median_removes_the_object_and_a_mean_would_not():
    import mosaic
    n, H, W, dx, dy = 12, 48, 64, 3, 1
    frames, T = pan_frames(11, n, H, W, dx, dy)
    frames = frames.copy()
    # a 10 x 12 rectangle at frame position (8 + 13 t mod 30, 6 + 17 t mod 40): in canvas coordinates it moves by more than
    # its own size every frame, so no canvas pixel is covered twice in a row and none in half of the frames that see it
    boxes = []
    for t in range(n):
        r, c = 6 + (13 * t) % 30, 8 + (17 * t) % 40
        frames[t, r:r + 10, c:c + 12] = 255
        boxes.append((r + t * dy, c + t * dx))
    pl = mosaic.plan(pan_warps(n, dx, dy), H, W)
    sprite, count = mosaic.build(frames, pl)
    covered = np.zeros((pl["Hc"], pl["Wc"]), np.int64)
    for r, c in boxes:
        covered[r - pl["oy"]:r - pl["oy"] + 10, c - pl["ox"]:c - pl["ox"] + 12] += 1
    ok = count >= 3
    assert np.all(2 * covered[ok] < count[ok]), "the test's own premise: every pixel is clean in more than half of its frames"
    crop = T[100 + pl["oy"]:100 + pl["oy"] + pl["Hc"], 200 + pl["ox"]:200 + pl["ox"] + pl["Wc"]]
    assert np.array_equal(sprite[ok], crop[ok])
    # the mean of the same samples is not the background where the rectangle has been
    total = np.zeros(sprite.shape, np.float64)
    for t in range(n):
        total[t * dy - pl["oy"]:t * dy - pl["oy"] + H, t * dx - pl["ox"]:t * dx - pl["ox"] + W] += frames[t]
    mean = np.floor(total / np.maximum(count, 1) + 0.5)
    hit = ok & (covered > 0) & (crop < 200)
    assert hit.any() and np.all(mean[hit] != crop[hit])
    # and the masks find the rectangle: every pixel of its interior, nothing two pixels away from it
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count, threshold=16, min_count=3)
    for t in (3, 6):
        r, c = 6 + (13 * t) % 30, 8 + (17 * t) % 40
        inner = masks[t, r + 1:r + 9, c + 1:c + 11]
        kn = mosaic.residuals(frames[t], pl["A"][t], sprite, count, pl["ox"], pl["oy"], 3)[0][r + 1:r + 9, c + 1:c + 11]
        assert np.all(inner[kn] == 1)
        far = masks[t].copy()
        far[max(0, r - 2):r + 12, max(0, c - 2):c + 14] = 0
        assert not far.any()


def test_lower_median_on_even_counts_fill_and_min_count():
    import mosaic
    H, W = 4, 6
    vals = [10, 200, 30, 40]                              # sorted 10 30 40 200: rank (4 - 1) // 2 = 1 -> 30
    frames = np.stack([np.full((H, W), v, np.uint8) for v in vals])
    pl = {"A": np.tile(IDENT, (4, 1)), "G": np.tile(IDENT, (4, 1)), "ox": -2, "oy": 0, "Hc": H, "Wc": W + 4,
          "flags": np.zeros(4, np.int32)}
    sprite, count = mosaic.build(frames, pl, fill=77)
    assert np.all(count[:, 2:2 + W] == 4) and np.all(sprite[:, 2:2 + W] == 30)
    assert np.all(count[:, :2] == 0) and np.all(sprite[:, :2] == 77) and np.all(sprite[:, 2 + W:] == 77)
    pl["flags"] = np.array([0, 0, 0, 1], np.int32)        # three samples 10 200 30 -> rank 1 -> 30; two -> rank 0
    assert np.all(mosaic.build(frames, pl)[0][:, 2:2 + W] == 30)
    pl["flags"] = np.array([0, 1, 1, 0], np.int32)        # 10 40 -> the lower one
    sprite, count = mosaic.build(frames, pl)
    assert np.all(sprite[:, 2:2 + W] == 10) and np.all(count[:, 2:2 + W] == 2)
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count, threshold=16, min_count=3)
    assert not masks.any() and not known.any()           # count 2 < min_count: nothing is known
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count, threshold=16, min_count=2)
    # the far tap of the last frame column is canvas column W + 2, which no frame covers: that column is not known
    n = H * (W - 1)
    assert list(known) == [n, 0, 0, n] and list(moving) == [0, 0, 0, n]      # |40 - 10| > 16; flagged frames: zero
    with pytest.raises(ValueError):
        mosaic.moving_masks(frames, pl, sprite, count, threshold=256)
    with pytest.raises(ValueError):
        mosaic.moving_masks(frames, pl, sprite, count, min_count=0)
    with pytest.raises(ValueError):
        mosaic.build(frames, pl, fill=-1)


def one_frame_masks(frame, sprite, count, threshold, min_count=1):
    import mosaic
    pl = {"A": IDENT[None], "G": IDENT[None], "ox": 0, "oy": 0, "Hc": 5, "Wc": 5, "flags": np.zeros(1, np.int32)}
    return mosaic.moving_masks(frame[None], pl, sprite, count, threshold, min_count)


def test_three_by_three_rule_at_borders_and_beside_unknown_pixels():
    sprite = np.full((5, 5), 100, np.uint8)
    count = np.full((5, 5), 5, np.uint16)
    # one pixel of residual 100 in the corner: its neighbourhood has 4 pixels, 100 > 16 * 4; the pixel (1, 1) sees it among
    # 9, 100 <= 144; a residual of 145 there would pass
    f = sprite.copy()
    f[0, 0] = 200
    m, known, moving = one_frame_masks(f, sprite, count, 16)
    want = np.zeros((5, 5), np.uint8)
    want[0, 0] = 1                                         # (0, 1) and (1, 0): 6 pixels, 100 > 96 as well
    want[0, 1] = want[1, 0] = 1
    assert np.array_equal(m[0], want) and known[0] == 25 and moving[0] == 3
    # on an edge: (0, 2) with residual 100 has 6 neighbours inside: 100 > 96 -> set; its neighbours on row 0 see 6 too; row 1
    # sees 9: not set
    f = sprite.copy()
    f[0, 2] = 0
    m, _, _ = one_frame_masks(f, sprite, count, 16)
    want = np.zeros((5, 5), np.uint8)
    want[0, 1:4] = 1
    assert np.array_equal(m[0], want)
    # in the middle a single residual of 144 does not pass (144 <= 16 * 9) and 145 does, for all nine pixels around it
    for r, expect in ((144, 0), (145, 1)):
        f = sprite.copy()
        f[2, 2] = 100 + r
        m, _, _ = one_frame_masks(f, sprite, count, 16)
        assert m[0].sum() == 9 * expect and np.all(m[0, 1:4, 1:4] == expect)
    # unknown pixels leave the sum and the number: columns 3 and 4 have count 0, and the far tap of a pixel of column 2 is
    # column 3, so columns 0 and 1 are known and 2 .. 4 are not
    c2 = count.copy()
    c2[:, 3:] = 0
    f = sprite.copy()
    f[2, 1] = 200                                         # residual 100; its known neighbourhood: columns 0, 1 x rows 1..3 = 6
    m, known, moving = one_frame_masks(f, sprite, c2, 16)
    assert known[0] == 10
    want = np.zeros((5, 5), np.uint8)
    want[1:4, 0:2] = 1                                     # each of them has 6 known neighbours: 100 > 96
    assert np.array_equal(m[0], want) and moving[0] == 6
    assert not m[0][:, 2:].any()                           # an unknown pixel is never set, whatever lies beside it
    # threshold 0: any residual marks
    f = sprite.copy()
    f[4, 4] = 101
    m, _, _ = one_frame_masks(f, sprite, count, 0)
    assert m[0].sum() == 4 and np.all(m[0, 3:, 3:] == 1)


def test_unusable_frames_are_flagged_and_left_out():
    import mosaic
    n, H, W = 6, 32, 48
    frames, T = pan_frames(5, n, H, W, 2, 1)
    h = pan_warps(n, 2, 1)
    clean = mosaic.plan(h, H, W)
    C = __import__("stabilize").trajectory(h)
    bad = C.copy()
    bad[2, 0, 2] = np.nan                                   # a NaN warp
    bad[4] = np.array([[1, 0, 8], [0, 1, 4], [-2.0 / W, 0, 1.0]])   # d = 1 - 2 u / W: <= 0 on the right half of the frame
    pl = mosaic.plan_path(bad, H, W)
    assert list(pl["flags"]) == [0, 0, 1, 0, 1, 0]
    assert (pl["ox"], pl["oy"], pl["Hc"], pl["Wc"]) == (clean["ox"], clean["oy"], clean["Hc"], clean["Wc"])
    sprite, count = mosaic.build(frames, pl)
    keep = [0, 1, 3, 5]
    sub = dict(clean, A=clean["A"][keep], G=clean["G"][keep], flags=np.zeros(4, np.int32))
    s2, c2 = mosaic.build(frames[keep], sub)
    assert np.array_equal(sprite, s2) and np.array_equal(count, c2) and count.max() == 4
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count, min_count=1)
    assert not masks[2].any() and not masks[4].any() and known[2] == known[4] == 0 and known[[0, 1, 3, 5]].min() > 0
    with pytest.raises(ValueError, match="anchor"):
        mosaic.plan_path(bad, H, W, anchor=2)
    with pytest.raises(ValueError, match="anchor"):
        mosaic.plan(h, H, W, anchor=n)


def test_max_canvas_pixels_raises_with_the_size():
    import mosaic
    h = pan_warps(9, 5, -3)
    with pytest.raises(ValueError, match="72 x 104"):
        mosaic.plan(h, 48, 64, max_canvas_pixels=72 * 104 - 1)
    assert mosaic.plan(h, 48, 64, max_canvas_pixels=72 * 104)["Wc"] == 104
    with pytest.raises(ValueError, match="max_canvas_pixels"):
        mosaic.plan(pan_warps(40, 64, 0), 48, 64)           # 40 frames side by side: more than 16 frames' worth


def test_anchor_shifts_the_canvas_by_the_closed_form_offset():
    import mosaic
    n, H, W, dx, dy = 9, 48, 64, 5, -3
    frames, _ = pan_frames(7, n, H, W, dx, dy)
    h = pan_warps(n, dx, dy)
    p0, p4 = mosaic.plan(h, H, W), mosaic.plan(h, H, W, anchor=4)
    assert (p4["ox"], p4["oy"]) == (p0["ox"] - 4 * dx, p0["oy"] - 4 * dy) and (p4["Hc"], p4["Wc"]) == (p0["Hc"], p0["Wc"])
    s0, c0 = mosaic.build(frames, p0)
    s4, c4 = mosaic.build(frames, p4)
    assert np.array_equal(s0, s4) and np.array_equal(c0, c4)
    m0 = mosaic.moving_masks(frames, p0, s0, c0)
    m4 = mosaic.moving_masks(frames, p4, s4, c4)
    assert all(np.array_equal(a, b) for a, b in zip(m0, m4))


def test_cli_parses_mosaic():
    import gme_cli
    a = gme_cli._parser().parse_args(["mosaic", "-p", "clip.npy", "-o", "out"])
    assert (a.command, a.path, a.outdir, a.estimator, a.anchor, a.threshold, a.min_count, a.masks) == \
        ("mosaic", "clip.npy", "out", "projective", 0, 16, 3, True)
    a = gme_cli._parser().parse_args(["mosaic", "-p", "x", "-o", "y", "--estimator", "affine", "--anchor", "7", "--threshold", "24",
                                      "--min-count", "5", "--no-masks"])
    assert (a.estimator, a.anchor, a.threshold, a.min_count, a.masks) == ("affine", 7, 24, 5, False)
    with pytest.raises(SystemExit):
        gme_cli._parser().parse_args(["mosaic", "-p", "x"])


class _FakeSequence:
    def __init__(self, ctx, n, H, W):
        self.N = n

    def close(self):
        pass


def test_sharded_mosaic_refuses_more_than_one_rank_or_lane(monkeypatch):
    import _gme_native
    import sequence
    monkeypatch.setattr(_gme_native, "Sequence", _FakeSequence)
    monkeypatch.setattr(_gme_native, "Context", lambda device=0: type("C", (), {"device": device, "close": lambda self: None})())
    ctx = type("C", (), {"device": 0})()
    for kw in ({"rank": 0, "world": 2}, {"rank": 1, "world": 3}, {"streams": 2}):
        sh = sequence.ShardedSequence(32, 48, 12, 1, ctx=ctx, **kw)
        with pytest.raises(ValueError, match="median does not combine"):
            sh.mosaic()
        sh.close()
    sh = sequence.ShardedSequence(32, 48, 12, 2, ctx=ctx)
    with pytest.raises(ValueError, match="frame_distance"):
        sh.mosaic()
    sh.close()


def test_mosaic_kernels_do_not_spill():
    """The compiler's resource remarks (build/*.remarks) for the kernels of gme_mosaic.hip: no VGPR or SGPR spill, no scratch."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_table
    rows = [r for r in resource_table.kernels() if r["file"] == "gme_mosaic.hip"]
    assert {r["name"] for r in rows} == {"k_mosaic_median", "k_moving_mask"}, rows
    for r in rows:
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r.get("sgpr_spill", 0) == 0, r
    med = [r for r in rows if r["name"] == "k_mosaic_median"][0]
    assert med["lds"] == 32768, med                        # 64 pixels x 256 bins of 16 bits


def test_abi_declares_the_mosaic_entries():
    import _gme_native
    lib = _gme_native.load_library()
    for name in ("gme_seq_mosaic", "gme_seq_read_mosaic", "gme_seq_moving_masks", "gme_seq_read_masks_range"):
        assert name in _gme_native.exported_symbols() and hasattr(lib, name)
