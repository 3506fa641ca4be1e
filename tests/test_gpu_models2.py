"""Second-order motion models on the device (k_fit_level2 / k_model2_field of gme_kernels.hip through gme_seq_gme_begin_fit2 /
gme_seq_gme_fit2 / gme_seq_compensate2 / gme_model2_field): reduction to the affine path, the exact order-2 stage against NumPy
restatements, recovery of a known quadratic field, the streamed batch against per-pair calls, and the CLI.  Needs an MI355X."""
import os

import numpy as np
import pytest

from helpers import c_oracle, field2_np, stage_np

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pad12(p):
    p = np.asarray(p, np.float64).reshape(-1, 6)
    return np.concatenate([p, np.zeros_like(p)], axis=1)


def pairs_under_test(golden):
    import synth
    g = golden("g9_pan240seq")["frames"]
    return {"synth720": synth.sequence(1234, 5, 2, 480, 720), "real_g9": np.ascontiguousarray(g[10:12])}


def test_zero_second_order_reduces_to_affine(golden, native):
    """params12 = affine params + zero second-order terms: fields, masks, thresholds equal the order-1 calls', the 27 sums
    reduce to the order-1 sums bit for bit, compensate2 equals compensate -- levels -1, 1 and 2, synthetic and real frames."""
    import motion
    import roadmap
    ctx = native.default_context()
    for name, frames in pairs_under_test(golden).items():
        H, W = frames.shape[1:]
        seq = native.Sequence(ctx, 2, H, W)
        seq.upload(0, frames)
        q0, s15 = seq.gme_begin_fit(1, 16, 0.3)
        s15 = np.array(s15)
        st = seq.gme_read_stage(1, 0)
        r0, s27 = seq.gme_begin_fit2(1, 16, 0.3)
        s27 = np.array(s27)
        st2 = seq.gme_read_stage(1, 0)
        assert np.array_equal(np.array(q0), np.array(r0))
        for k in ("gt", "model", "mask"):
            assert np.array_equal(st[k], st2[k]), (name, 1, k)
        assert st["thr"] == st2["thr"]
        assert np.array_equal(bits(roadmap.affine_sums(s27)), bits(s15)), (name, 1)
        p = motion._solve_batch(s15)
        p[:, 0] *= 2
        p[:, 3] *= 2
        for frac in (0.3, 0.0):
            s15 = np.array(seq.gme_fit(2, p, frac))
            st = seq.gme_read_stage(2, 0)
            s27 = np.array(seq.gme_fit2(2, pad12(p), frac))
            st2 = seq.gme_read_stage(2, 0)
            for k in ("gt", "model", "mask", "thr"):
                assert np.array_equal(st[k], st2[k]), (name, 2, frac, k)
            assert np.array_equal(bits(roadmap.affine_sums(s27)), bits(s15)), (name, 2, frac)
        final = motion._solve_batch(s15)
        sse = np.array(seq.compensate(1, 16, final))
        comp = seq.read_compensated(0)
        sse2 = np.array(seq.compensate2(1, 16, pad12(final)))
        assert np.array_equal(sse, sse2) and np.array_equal(comp, seq.read_compensated(0)), name
        assert np.array_equal(comp, seq.read_compensated_range(0, 1)[0])
        # level -1: the field of the last bbme() call, unmasked and masked
        seq.bbme(1, 16, 2, 3, 1)
        for frac in (-1.0, 0.3):
            s15 = np.array(seq.gme_fit(-1, final, frac))
            st = seq.gme_read_stage(-1, 0)
            s27 = np.array(seq.gme_fit2(-1, pad12(final), frac))
            st2 = seq.gme_read_stage(-1, 0)
            for k in ("gt", "model", "mask", "thr"):
                assert np.array_equal(st[k], st2[k]), (name, -1, frac, k)
            assert np.array_equal(bits(roadmap.affine_sums(s27)), bits(s15)), (name, -1, frac)
        # the single-pair field
        h, w = H // 16, W // 16
        assert np.array_equal(ctx.model2_field(pad12(final)[0], h, w), motion.get_motion_field_affine((h, w), final[0]))
        seq.close()


SECOND = [
    # smooth second-order terms
    np.array([1.25, 0.05, -0.08, -0.75, 0.04, 0.02, 0.004, -0.003, 0.002, -0.002, 0.003, -0.001]),
    # dyadic values: many displacements exactly on .5 ties (round-half-even decides)
    np.array([0.5, 0.25, -0.5, -1.5, 0.5, 0.25, 0.125, -0.0625, 0.03125, 0.25, 0.0625, -0.125]),
    # beyond int16: the store wraps
    np.array([40000.5, 0.0, 0.0, -33000.5, 1.0, 0.0, 30.0, 0.0, 0.0, 0.0, 0.0, -20.0]),
]


def test_exact_second_order_stage(golden, native):
    """Non-zero second-order terms: the device field equals the NumPy restatement of its evaluation order, mask and threshold
    the threshold rule, all 27 sums a sequential sum over the ordered inliers bit for bit, compensated frames the C oracle's
    compensate fed with that field."""
    co = c_oracle()
    ctx = native.default_context()
    for name, frames in pairs_under_test(golden).items():
        H, W = frames.shape[1:]
        h, w = H // 16, W // 16
        seq = native.Sequence(ctx, 2, H, W)
        seq.upload(0, frames)
        seq.gme_begin_fit2(1, 16, 0.3)
        seq.bbme(1, 16, 2, 3, 1)
        for k, p12 in enumerate(SECOND):
            want_field = field2_np(p12, h, w)
            assert np.array_equal(ctx.model2_field(p12, h, w), want_field), (name, k)
            for level, frac in ((2, 0.3), (1, 0.3), (2, 0.0), (-1, -1.0), (-1, 0.3)):
                s27 = np.array(seq.gme_fit2(level, p12[None], frac))[0]
                st = seq.gme_read_stage(level, 0)
                hh, ww = st["gt"].shape[:2]
                model = field2_np(p12, hh, ww)
                assert np.array_equal(st["model"], model), (name, k, level)
                lvl_hw = (H, W) if level != 1 else seq.level_shape(1)
                thr, mask, sums = stage_np(st["gt"], model, frac, lvl_hw)
                assert st["thr"] == thr and np.array_equal(st["mask"], mask), (name, k, level, frac)
                assert np.array_equal(bits(s27), bits(sums)), (name, k, level, frac, s27 - sums)
            sse = int(np.array(seq.compensate2(1, 16, p12[None]))[0])
            comp = seq.read_compensated(0)
            want = co.compensate(frames[0], want_field.astype(np.int32))
            assert np.array_equal(comp, want), (name, k)
            assert sse == co.sse(frames[1], want), (name, k)
        seq.close()


FIT_LIST_LDS_BYTES = 40 * 1024        # gme_internal.h: larger inlier lists (16 bytes per block) live in global memory


def global_list_stages():
    """(name, frames uint8[3, H, W], begin_fit block size or None, [(bbme block size for level -1)]) whose stages all hold
    more than FIT_LIST_LDS_BYTES / 16 = 2560 blocks: full HD and a ragged size at levels 2 and 1 (bs 8) and -1 (bs 16),
    480 x 720 at level -1 after small-block searches."""
    import synth
    return [("hd", synth.sequence(31, 0, 3, 1080, 1920), 8, [16]),
            ("ragged", synth.sequence(32, 4, 3, 1078, 1918), 8, [16]),
            ("synth720", synth.sequence(1234, 5, 3, 480, 720), None, [8, 4])]


def check_stage_pair(seq, order, level, pair, p12, frac, lvl_hw, sums, what):
    """One pair's stage against field2_np / stage_np bit for bit; order 1 against the affine part of the order-2 sums."""
    import roadmap
    st = seq.gme_read_stage(level, pair)
    hh, ww = st["gt"].shape[:2]
    assert hh * ww * 16 > FIT_LIST_LDS_BYTES, (what, hh, ww)                 # the global inlier list
    model = field2_np(p12, hh, ww)
    assert np.array_equal(st["model"], model), what
    thr, mask, want = stage_np(st["gt"], model, frac, lvl_hw)
    assert st["thr"] == thr and np.array_equal(st["mask"], mask), what
    if order == 1:
        want = roadmap.affine_sums(want)[0]
    assert np.array_equal(bits(sums), bits(want)), (what, sums - want)


def test_second_order_stage_global_list(native):
    """test_exact_second_order_stage where the inlier list does not fit in LDS (k_fit_level2 / k_fit_level with the global
    list): field, threshold, mask and all 27 sums bit for bit against the NumPy restatements for every SECOND parameter set
    and fractions 0.3, 0.0 and -1, two pairs with different parameters per call (the per-pair list offset); the order-1
    fit's 15 sums at the same stages against the affine part of the restated 27."""
    ctx = native.default_context()
    for name, frames, fit_bs, mv_bs in global_list_stages():
        H, W = frames.shape[1:]
        seq = native.Sequence(ctx, 3, H, W)
        seq.upload(0, frames)
        stages = []
        if fit_bs:
            seq.gme_begin_fit2(1, fit_bs, 0.3)
            stages += [(2, None), (1, None)]
        stages += [(-1, b) for b in mv_bs]
        for level, bs in stages:
            if bs:
                seq.bbme(1, bs, 2, 3, 1)
            lvl_hw = seq.level_shape(1) if level == 1 else (H, W)
            for k in range(len(SECOND)):
                p12 = np.stack([SECOND[k], SECOND[(k + 1) % len(SECOND)]])
                for frac in (0.3, 0.0, -1.0):
                    s27 = np.array(seq.gme_fit2(level, p12, frac))
                    for pair in range(2):
                        check_stage_pair(seq, 2, level, pair, p12[pair], frac, lvl_hw, s27[pair], (name, level, bs, k, frac, pair))
                    s15 = np.array(seq.gme_fit(level, p12[:, :6], frac))
                    for pair in range(2):
                        check_stage_pair(seq, 1, level, pair, pad12(p12[pair, :6])[0], frac, lvl_hw, s15[pair],
                                         (name, level, bs, k, frac, pair, "order 1"))
        seq.close()


def quad_pair(seed=7, H=240, W=320, bs=16):
    """A frame pair whose block vectors follow a known second-order field: block (i, j) of a noise canvas `previous` is
    pasted into `current` moved by the rounded field (block matching searches each block of `previous` in `current`,
    motion.py:224-229 / bbme.py:146-171); every target lies inside the frame, |d| <= 6 < the search window of 8."""
    rng = np.random.default_rng(seed)
    prev = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    cur = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    h, w = H // bs, W // bs
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ci, cj = (h - 1) / 2.0, (w - 1) / 2.0
    dx = -((j - cj) * (0.25 + 0.01 * i) + 0.01 * (j - cj) ** 2)       # >= 0 at the left edge, <= 0 at the right
    dy = -((i - ci) * (0.25 + 0.01 * j) + 0.02 * (i - ci) ** 2)       # >= 0 at the top, <= 0 at the bottom
    truth = np.stack([np.rint(dx), np.rint(dy)], axis=2).astype(np.int32)
    assert np.abs(truth).max() <= 6
    for a in range(h):
        for b in range(w):
            r, c = a * bs + truth[a, b, 1], b * bs + truth[a, b, 0]
            assert 0 <= r <= H - bs and 0 <= c <= W - bs
            cur[r:r + bs, c:c + bs] = prev[a * bs:(a + 1) * bs, b * bs:(b + 1) * bs]
    return prev, cur, truth, (dx, dy)


def lstsq_inliers(model, gt, mask):
    import importlib
    host = importlib.import_module("test_models2_host")
    h, w = gt.shape[:2]
    k = np.nonzero(~np.asarray(mask, bool).ravel())[0]
    x, y = 4.0 * (k // w), 4.0 * (k % w)
    return host.lstsq_params(model, x, y, gt.reshape(-1, 2)[k, 0].astype(np.float64), gt.reshape(-1, 2)[k, 1].astype(np.float64))


def test_recovery_of_a_known_quadratic_field(native):
    import roadmap
    prev, cur, truth, (dx, dy) = quad_pair()
    ctx = native.default_context()
    seq = native.Sequence(ctx, 2, *prev.shape)
    seq.upload(0, np.stack([prev, cur]))
    seq.bbme(1, 16, 8, 0, 1)                                          # exhaustive, MSE
    s27 = seq.gme_fit2(-1, np.zeros((1, 12)), -1.0)                   # the unmasked fit of motion.py:33-88
    st = seq.gme_read_stage(-1, 0)
    assert np.array_equal(st["gt"], truth) and not st["mask"].any()
    got = roadmap.solve_model(s27, "quadratic")[0]
    np.testing.assert_allclose(got, lstsq_inliers("quadratic", truth, st["mask"]), rtol=1e-6, atol=1e-9)
    # the fitted field (fit coordinates x = 4 i, y = 4 j) stays within the rounding of the true one
    h, w = truth.shape[:2]
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y = 4 * i, 4 * j
    fx = got[0] + got[1] * x + got[2] * y + got[6] * x * x + got[7] * x * y + got[8] * y * y
    fy = got[3] + got[4] * x + got[5] * y + got[9] * x * x + got[10] * x * y + got[11] * y * y
    assert np.abs(fx - dx).max() < 0.5 and np.abs(fy - dy).max() < 0.5
    # the staged two-level estimate: level-2 parameters are the least-squares fit of the device's own inlier stage
    for model in ("pseudo_perspective", "quadratic", "bilinear"):
        params = roadmap.estimate_sequence(seq, 1, model)
        st = seq.gme_read_stage(2, 0)
        np.testing.assert_allclose(params[0], lstsq_inliers(model, st["gt"], st["mask"]), rtol=1e-6, atol=1e-9)
        assert np.array_equal(params[0], roadmap.global_motion_estimation(prev, cur, model))
    seq.close()


def test_stream_batch_equals_per_pair(native):
    """estimate_stream(..., model=m) over 300 pairs in chunks across two lanes == roadmap.global_motion_estimation per pair,
    bit for bit; PSNR from compensate2 == the C oracle's compensation with roadmap.model_field; the default call is today's."""
    import roadmap
    import sequence
    import synth
    frames = synth.sequence(99, 0, 301, 240, 320)
    base_p, base_s = sequence.estimate_stream(frames, 1, chunk_pairs=64, streams=2)
    none_p, none_s = sequence.estimate_stream(frames, 1, chunk_pairs=64, streams=2, model=None)
    aff_p, aff_s = sequence.estimate_stream(frames, 1, chunk_pairs=64, streams=2, model="affine")
    assert np.array_equal(base_p, none_p) and np.array_equal(base_s, none_s)
    assert np.array_equal(base_p, aff_p) and np.array_equal(base_s, aff_s)
    co = c_oracle()
    for model in ("bilinear", "pseudo_perspective", "quadratic"):
        comp = np.empty((300, 240, 320), np.uint8)
        p, psnr = sequence.estimate_stream(frames, 1, chunk_pairs=64, streams=2, model=model, compensated=comp)
        assert p.shape == (300, 12)
        for k in range(300):
            assert np.array_equal(p[k], roadmap.global_motion_estimation(frames[k], frames[k + 1], model)), (model, k)
        for k in (0, 63, 64, 299):
            want = co.compensate(frames[k], roadmap.model_field((15, 20), p[k]).astype(np.int32))
            assert np.array_equal(comp[k], want), (model, k)
            assert psnr[k] == sequence.psnr_from_sse(np.array([co.sse(frames[k + 1], want)]), 240, 320)[0]


@pytest.mark.parametrize("model", ["quadratic", "pseudo_perspective"])
def test_cli_results_second_order(native, tmp_path, monkeypatch, model):
    import gme_cli
    import synth
    from PIL import Image
    monkeypatch.chdir(tmp_path)
    d = tmp_path / "resources" / "videos" / "clip"
    d.mkdir(parents=True)
    frames = synth.sequence(1234, 0, 7, 240, 320)
    for k, f in enumerate(frames):
        Image.fromarray(f).save(str(d / ("%d.png" % k)))
    base = gme_cli.main(["results", "-v", "clip", "-f", "1"])
    rec = gme_cli.main(["results", "-v", "clip", "-f", "1", "--model", model])
    assert sorted(rec, key=int) == [str(k) for k in range(1, 7)]
    for k in base:                                                    # a pure pan: the second-order fit compensates it as well
        assert abs(complex(rec[k]).real - complex(base[k]).real) < 1.0, (k, rec[k], base[k])
    out = tmp_path / "results" / "clip"
    for sub in ("frames", "compensated", "curr_prev_diff", "model_motion_field", "curr_comp_diff"):
        assert len(os.listdir(str(out / sub))) == 6, sub
