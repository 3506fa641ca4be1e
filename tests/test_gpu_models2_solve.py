"""The second-order device solve (k_solve_model2 through gme_solve_model2_sums and gme_seq_gme_device_solve2) and the motion
models of ShardedSequence, against the staged host path (begin_fit2 -> roadmap.solve_model -> roadmap.project -> fit2(2) ->
roadmap.solve_model -> compensate2).  Needs an MI355X."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from helpers import DX, DY, MOMENTS, PHI
from helpers import clear_of_ties2 as clear_of_ties
from helpers import contract_violations2 as contract_violations

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


@contextmanager
def _with_env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def sums_of_field(params, h, w, bs, cols=None):
    """The 27 order-2 sums of the fit (x = 4 i, y = 4 j, uniform weight 1 / (H W)) over the blocks of an h x w field whose
    displacements are the float64 values of `params`; `cols` restricts the inliers to those block columns."""
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if cols is not None:
        keep = np.isin(j, cols)
        i, j = i[keep], j[keep]
    x, y = 4 * i.ravel(), 4 * j.ravel()
    wgt = 1.0 / (h * bs * w * bs)
    phi = np.stack([x ** a * y ** b for a, b in PHI], axis=1)
    p = np.asarray(params, np.float64)
    dx, dy = phi @ p[DX], phi @ p[DY]
    mono = np.stack([x ** a * y ** b for a, b in MOMENTS], axis=1)
    return np.concatenate([(mono * wgt).sum(0), (phi * dx[:, None] * wgt).sum(0), (phi * dy[:, None] * wgt).sum(0)])


def _synthetic_sums(h, w, bs, n, seed):
    rng = np.random.default_rng(seed)
    scale = np.array([3.0, 0.05, 0.05, 3.0, 0.05, 0.05] + [2e-4] * 6)
    return np.stack([sums_of_field(rng.normal(size=12) * scale, h, w, bs) for _ in range(n)])


def _real_sums(native, golden):
    """The order-2 sums gme_fit2 leaves on the reference's real frames (g9, bs 16, fd 1): level 1 and level 2."""
    import roadmap
    frames = golden("g9_pan240seq")["frames"]
    seq = native.Sequence.from_frames(native.default_context(), frames)
    try:
        _, s1 = seq.gme_begin_fit2(1, 16, 0.3)
        s1 = np.array(s1)
        s2 = np.array(seq.gme_fit2(2, roadmap.project(roadmap.solve_model(s1, "quadratic")), 0.3))
    finally:
        seq.close()
    return np.concatenate([s1, s2])


@pytest.mark.parametrize("H,W", [(480, 720), (1080, 1920)])
def test_solve_equals_host_on_known_fields(native, H, W):
    import roadmap
    ctx = native.default_context()
    bs = 16
    h, w = H // bs, W // bs
    sums = _synthetic_sums(h, w, bs, 64, H)
    for model in roadmap.SECOND_ORDER:
        host = roadmap.solve_model(sums, model)
        clear = clear_of_ties(host, h, w)
        assert clear.sum() >= 48, model
        dev, flags = ctx.solve_model2_sums(sums, model, h, w)
        assert not np.any(flags[clear]), (model, np.nonzero(flags)[0], flags[flags != 0])
        assert contract_violations(dev, host, h, w) == [], model
        proj, pflags = ctx.solve_model2_sums(sums, model, h, w, project=True)
        assert not np.any(pflags[clear_of_ties(roadmap.project(host), h, w)]), model
        assert np.array_equal(proj, roadmap.project(dev)), model           # the projection is exact
        if model == "pseudo_perspective":
            assert np.array_equal(dev[:, 7], dev[:, 9]) and np.array_equal(dev[:, 8], dev[:, 10])
            assert not np.any(dev[:, 6]) and not np.any(dev[:, 11])
        if model == "bilinear":
            assert not np.any(dev[:, [6, 8, 9, 11]])


def test_solve_equals_host_on_real_sums(native, golden):
    import roadmap
    ctx = native.default_context()
    sums = _real_sums(native, golden)
    h, w = 240 // 16, 320 // 16
    for model in roadmap.SECOND_ORDER:
        host = roadmap.solve_model(sums, model)
        clear = clear_of_ties(host, h, w)
        assert clear.mean() > 0.9, model
        dev, flags = ctx.solve_model2_sums(sums, model, h, w)
        assert not np.any(flags[clear]), (model, np.nonzero(flags)[0], flags[flags != 0])
        assert contract_violations(dev[clear], host[clear], h, w) == [], model


def test_safety_net(native):
    import roadmap
    ctx = native.default_context()
    h, w, bs = 30, 45, 16
    tie = np.zeros(12)
    tie[0] = 2.5                                                            # dx = 2.5 on every block: a rounding tie
    on_tie = sums_of_field(tie, h, w, bs)[None]
    for model in roadmap.SECOND_ORDER:
        _, flags = ctx.solve_model2_sums(on_tie, model, h, w)
        assert flags[0] & 1, (model, flags)
    apart = tie.copy()
    apart[0], apart[3], apart[1], apart[7] = 2.25, -1.125, 1e-3, 1e-5       # every dx in [2.25, 2.3), dy = -1.125
    _, flags = ctx.solve_model2_sums(sums_of_field(apart, h, w, bs)[None], "quadratic", h, w)
    assert flags[0] == 0, flags
    # every inlier in block column 0: y = 0, so the y, y^2 and xy rows vanish -- roadmap raises LinAlgError
    column = sums_of_field(apart, h, w, bs, cols=[0])[None]
    with pytest.raises(np.linalg.LinAlgError):
        roadmap.solve_model(column, "quadratic")
    _, flags = ctx.solve_model2_sums(column, "quadratic", h, w)
    assert flags[0] & 4, flags
    with pytest.raises(IndexError, match="model 2"):                       # GME_ERR_ARG through _check
        ctx.solve_model2_sums(on_tie, 2, h, w)


@pytest.mark.parametrize("bs,fd", [(16, 1), (12, 5)])
def test_device_estimate_equals_staged_host_path(native, golden, bs, fd):
    import motion
    import roadmap
    frames = golden("g9_pan240seq")["frames"]
    n = len(frames) - fd
    H, W = frames.shape[1:]
    frac = float(motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE)
    seq = native.Sequence.from_frames(native.default_context(), frames)
    try:
        for model in roadmap.SECOND_ORDER:
            _, s1 = seq.gme_begin_fit2(fd, bs, frac)
            s2 = seq.gme_fit2(2, roadmap.project(roadmap.solve_model(s1, model)), frac)
            stage_h = [seq.gme_read_stage(2, i) for i in range(n)]
            host = roadmap.solve_model(s2, model)
            sse_h = np.array(seq.compensate2(fd, bs, host))
            comp_h = [seq.read_compensated(i) for i in range(n)]

            seq.set_split_phase(True)
            try:
                params, sse, flags = seq.gme_device_solve2(model, fd, bs, frac)     # returns once queued
                seq.wait()
                params, sse, flags = np.array(params), np.array(sse), np.array(flags)
            finally:
                seq.set_split_phase(False)
            assert params.shape == (n, 12) and sse.shape == (n,)
            assert not np.any(flags), "flagged pairs of %s at bs %d fd %d: %s" % (
                model, bs, fd, {int(i): int(flags[i]) for i in np.nonzero(flags)[0]})
            assert contract_violations(params, host, H // bs, W // bs) == [], (model, bs, fd)
            assert np.array_equal(sse, sse_h), model
            for i in range(n):
                st = seq.gme_read_stage(2, i)
                assert np.array_equal(st["model"], stage_h[i]["model"]) and np.array_equal(st["mask"], stage_h[i]["mask"]), (model, i)
                assert st["thr"] == stage_h[i]["thr"], (model, i)
                assert np.array_equal(seq.read_compensated(i), comp_h[i]), (model, i)
    finally:
        seq.close()


def _reference(native, frames, fd, model):
    """roadmap.estimate_sequence + compensate2 / compensate on one sequence -> (params, exact PSNR)."""
    import motion
    import roadmap
    import sequence
    seq = native.Sequence.from_frames(native.default_context(), frames)
    try:
        p = roadmap.estimate_sequence(seq, fd, model)
        comp = seq.compensate2 if model in roadmap.SECOND_ORDER else seq.compensate
        sse = np.array(comp(fd, int(motion.BBME_BLOCK_SIZE), p))
    finally:
        seq.close()
    return p, sequence.psnr_from_sse(sse, frames.shape[1], frames.shape[2], exact=True)


@pytest.mark.parametrize("streams", [1, 3])
def test_sharded_sequence_models(native, golden, streams):
    import roadmap
    import sequence
    frames = golden("g9_pan240seq")["frames"]
    fd = 1
    h, w = 240 // 16, 320 // 16
    shard = sequence.ShardedSequence(240, 320, len(frames), fd, streams=streams, interleave=streams > 1)
    try:
        shard.load(frames)
        base_p, base_psnr = shard.estimate_and_compensate(exact_psnr=True)
        for same in (None, "affine"):
            p, psnr = shard.estimate_and_compensate(exact_psnr=True, model=same)
            assert np.array_equal(p, base_p) and np.array_equal(psnr, base_psnr), same
        assert np.array_equal(shard.estimate(model="affine"), shard.estimate())
        for model in roadmap.MODELS:
            want_p, want_psnr = _reference(native, frames, fd, model)
            p, psnr = shard.estimate_and_compensate(exact_psnr=True, model=model)
            assert p.shape == (len(frames) - fd, 12 if model in roadmap.SECOND_ORDER else 6)
            assert np.array_equal(p, want_p), model
            assert np.array_equal(psnr, want_psnr), model
            assert np.array_equal(shard.estimate(model=model), want_p), model

            ran = []
            real = shard._device_solved

            def spy(*a, **k):
                r = real(*a, **k)
                ran.append(r is not None)
                return r
            shard._device_solved = spy
            try:
                with _with_env("GME_DEVICE_SOLVE", "1"):
                    dp, dpsnr = shard.estimate_and_compensate(exact_psnr=True, model=model)
            finally:
                del shard._device_solved
            if model in roadmap.SECOND_ORDER:
                assert ran == [True], "%s: the device path did not run or fell back on real frames" % model
                assert contract_violations(dp, want_p, h, w) == [], model
            elif model == "affine":                                          # the existing 3x3 device solve
                assert ran == [True], model
                assert np.allclose(dp, want_p, rtol=1e-10, atol=1e-12)
            else:
                assert ran == [], model                                      # translation / similarity: the host path
                assert np.array_equal(dp, want_p), model
            assert np.array_equal(dpsnr, want_psnr), model
    finally:
        shard.close()


def test_two_shards_in_one_process_equal_one(native, golden):
    import sequence
    frames = golden("g9_pan240seq")["frames"]
    fd = 1
    whole = sequence.ShardedSequence(240, 320, len(frames), fd)
    try:
        whole.load(frames)
        want_p, want_psnr = whole.estimate_and_compensate(exact_psnr=True, model="quadratic")
    finally:
        whole.close()
    parts = []
    for rank in (0, 1):
        shard = sequence.ShardedSequence(240, 320, len(frames), fd, rank=rank, world=2)
        try:
            shard.load(frames)
            parts.append(shard.estimate_and_compensate(exact_psnr=True, model="quadratic"))
        finally:
            shard.close()
    p = np.concatenate([q for q, _ in parts])
    assert p.shape == (len(frames) - fd, 12)
    assert np.array_equal(p, want_p) and np.array_equal(np.concatenate([s for _, s in parts]), want_psnr)
    # the rows of a second-order model cross the library's RCCL all-gather as they are (one rank: the identity)
    ctx = native.Context(0)
    try:
        sequence.comm_init(ctx, 0, 1)
        got = sequence.gather_parameters_rccl(ctx, want_p, len(want_p), 0, 1)
        assert got.shape == want_p.shape and np.array_equal(got, want_p)
        sequence.comm_destroy(ctx)
    finally:
        ctx.close()
