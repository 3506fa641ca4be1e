"""The frame-plumbing kernels of csrc/gme_kernels.hip at their path boundaries: k_pyrdown_lds / k_pyrdown / k_pyrdown_edge16 /
k_pyrdown_edge, k_compensate16 / k_compensate with their fused squared error, k_sse and k_repack, on the case lists of
tests/frame_kernel_cases.py (which tests/test_frame_kernel_cases_host.py holds to the branches they must reach).  Needs an
MI355X.  Everything here is exact integer arithmetic: every comparison is byte for byte against the C oracle."""
import functools

import numpy as np
import pytest

import frame_kernel_cases as fk
from helpers import c_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


@functools.lru_cache(maxsize=None)
def _pyr_want(H, W, kind):
    """(level 1, level 0) of the C oracle for one single-plane case, computed once."""
    co = c_oracle()
    l1 = co.pyrdown(fk.content(kind, H, W))
    l1.setflags(write=False)
    l0 = co.pyrdown(l1)
    l0.setflags(write=False)
    return l1, l0


@functools.lru_cache(maxsize=None)
def _comp_want():
    """{case id: (frame, compensated frame of the C oracle)}, computed once."""
    co = c_oracle()
    out = {}
    for cid, H, W, bs, mf in fk.comp_cases():
        f = fk.comp_frame(H, W)
        want = co.compensate(f, mf)
        want.setflags(write=False)
        out[cid] = (f, want)
    return out


# ---------------------------------------------------------------------------
# pyramid
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", fk.CONTENTS)
def test_pyramid_single_plane(native, kind, monkeypatch):
    """utils.get_pyramids on every shape of pyr_shapes(): both levels equal the oracle, and with GME_FORCE_GENERIC (read at
    every launch) the fallback kernels give the same bytes on the shapes that take k_pyrdown_lds by default."""
    import utils
    shapes = fk.pyr_shapes()
    for H, W in shapes:
        f = fk.content(kind, H, W)
        l1, l0 = _pyr_want(H, W, kind)
        pyr = utils.get_pyramids(f)
        assert pyr[2] is f and np.array_equal(pyr[1], l1), (H, W, fk.pyr_path(H, W))
        assert np.array_equal(pyr[0], l0), (H, W, fk.pyr_path(*l1.shape))
    monkeypatch.setenv("GME_FORCE_GENERIC", "1")
    ctx = native.default_context()
    for H, W in shapes:
        if fk.pyr_path(H, W) != ("k_pyrdown_lds",):
            continue
        l1, l0 = _pyr_want(H, W, kind)
        assert np.array_equal(ctx.pyrdown(fk.content(kind, H, W)), l1), (H, W, "generic")
        assert np.array_equal(ctx.pyrdown(l1), l0), (H, W, "generic, level 0")


def _batch_frames(H, W):
    kinds = ("noise", "noise", "checker", "border", "noise")
    return np.stack([fk.content(k, H, W, seed=10 + i) for i, k in enumerate(kinds[:fk.PYR_BATCH])])


@pytest.mark.parametrize("chunk", [None, "2"])
def test_pyramid_batched(native, chunk, monkeypatch):
    """More than one plane per launch (blockIdx.z and the plane strides): levels 1 and 0 of every frame of a Sequence after
    gme_begin, in one launch per level and in chunks of two planes (GME_MAX_GRID_PAIRS)."""
    ctx = native.default_context()
    co = c_oracle()
    if chunk:
        monkeypatch.setenv("GME_MAX_GRID_PAIRS", chunk)
    for H, W in fk.PYR_BATCH_SHAPES:
        frames = _batch_frames(H, W)
        seq = native.Sequence.from_frames(ctx, frames)
        seq.gme_begin(1, 16)
        for i in range(len(frames)):
            l1 = co.pyrdown(frames[i])
            assert np.array_equal(seq.read_frame(i, 2), frames[i]), (H, W, i)
            assert np.array_equal(seq.read_frame(i, 1), l1), (H, W, i, fk.pyr_path(H, W))
            assert np.array_equal(seq.read_frame(i, 0), co.pyrdown(l1)), (H, W, i, fk.pyr_path(*l1.shape))
        seq.close()


# ---------------------------------------------------------------------------
# compensation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", fk.COMP_SHAPES, ids=lambda s: "%dx%d-bs%d" % s)
def test_compensate_boundary_fields(native, shape, monkeypatch):
    """motion.compensate_frame on every field of comp_fields(): the default dispatch and GME_FORCE_GENERIC (k_compensate
    on the k_compensate16 shapes too).  The fields are int32 and go through the mf32 entry as they are."""
    import motion
    want = _comp_want()
    cases = [c for c in fk.comp_cases() if c[1:4] == shape]
    assert len(cases) == len(fk.comp_fields(*shape))
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("GME_FORCE_GENERIC", env)
        for cid, H, W, bs, mf in cases:
            f, w = want[cid]
            got = motion.compensate_frame(f, mf)
            assert got.dtype == np.uint8 and np.array_equal(got, w), (cid, env, fk.comp_kernel(H, W, mf.shape[0], bool(env)))


@pytest.mark.parametrize("shape", fk.COMP_SEQ_SHAPES, ids=lambda s: "%dx%d-bs%d" % s)
def test_compensate_batched_translations_and_sse(native, shape, monkeypatch):
    """Sequence.compensate with one pure translation per pair (seq_translations: block columns and rows on the boundaries),
    both dispatches: every compensated frame and every fused squared error equals the oracle."""
    H, W, bs = shape
    ctx = native.default_context()
    co = c_oracle()
    tr = fk.seq_translations(H, W)
    frames = np.stack([fk.content("noise", H, W, seed=20 + i) for i in range(len(tr) + 1)])
    params = np.array([[d0, 0, 0, d1, 0, 0] for d0, d1 in tr], np.float64)
    wants = []
    for p, (d0, d1) in enumerate(tr):
        comp = co.compensate(frames[p], np.tile(np.array([d0, d1], np.int32), (H // bs, W // bs, 1)))
        wants.append((comp, co.sse(frames[p + 1], comp)))
    seq = native.Sequence.from_frames(ctx, frames)
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("GME_FORCE_GENERIC", env)
        sse = seq.compensate(1, bs, params)
        for p, (comp, err) in enumerate(wants):
            assert np.array_equal(seq.read_compensated(p), comp), (shape, env, tr[p])
            assert int(sse[p]) == err, (shape, env, tr[p])
    seq.close()


# ---------------------------------------------------------------------------
# squared error
# ---------------------------------------------------------------------------
def test_sse_pairs(native):
    ctx = native.default_context()
    co = c_oracle()
    for sid, a, b in fk.sse_pairs():
        want = co.sse(a, b)
        if "v" in sid:
            assert want == 255 ** 2 * a.shape[0] * a.shape[1], sid
        assert ctx.sse(a, b) == want, sid


@pytest.mark.parametrize("shape", fk.SSE_SATURATED, ids=lambda s: "%dx%d" % s)
def test_saturated_sse_fused_in_compensation(native, shape, monkeypatch):
    """A frame of 0 against a frame of 255 under zero motion: the per-thread, per-wave and per-tile 32-bit sums of
    k_compensate16 / k_compensate hold 255^2 per pixel (5.3e8 for a full 256 x 32 tile); the total is 255^2 H W exactly."""
    H, W = shape
    ctx = native.default_context()
    lo, hi = fk.content("zeros", H, W), fk.content("full", H, W)
    seq = native.Sequence.from_frames(ctx, np.stack([lo, hi, lo]))          # pairs 0 -> 255 and 255 -> 0
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("GME_FORCE_GENERIC", env)
        sse = seq.compensate(1, 16, np.zeros((2, 6)))
        assert [int(v) for v in sse] == [255 ** 2 * H * W] * 2, (shape, env)
        assert np.array_equal(seq.read_compensated(0), lo) and np.array_equal(seq.read_compensated(1), hi), (shape, env)
    seq.close()


# ---------------------------------------------------------------------------
# repack
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, "2"])
def test_repack_round_trip(native, chunk, monkeypatch):
    """Tight host frames through k_repack into the pitched planes and back: the 16-byte path (W % 16 == 0) and the byte
    path, a whole stack, a single frame behind others, and in chunks of two frames."""
    ctx = native.default_context()
    if chunk:
        monkeypatch.setenv("GME_MAX_GRID_PAIRS", chunk)
    for W in fk.REPACK_WIDTHS:
        H = 9
        frames = np.stack([fk.content("noise", H, W, seed=30 + i) for i in range(5)])
        seq = native.Sequence.from_frames(ctx, frames)
        for i in range(5):
            assert np.array_equal(seq.read_frame(i), frames[i]), (W, i)
        seq.upload(3, frames[1:2])
        assert np.array_equal(seq.read_frame(3), frames[1]) and np.array_equal(seq.read_frame(4), frames[4]), W
        assert np.array_equal(seq.read_frame(2), frames[2]), W
        seq.close()


@pytest.mark.parametrize("pinned", [True, False])
def test_repack_streamed_uploads(native, pinned):
    """bbme_streamed's chunked uploads (page-locked and pageable frames) leave the frames they were given in the planes."""
    ctx = native.default_context()
    co = c_oracle()
    for H, W in fk.REPACK_STREAMED:
        src = np.stack([fk.content("noise", H, W, seed=40 + i) for i in range(5)])
        frames = native.pinned_empty(src.shape) if pinned else np.empty(src.shape, np.uint8)
        frames[...] = src
        seq = native.Sequence(ctx, 5, H, W)
        mv = seq.bbme_streamed(frames, 1, 16, 2, 3, 0, chunk_frames=2).copy()
        for i in range(5):
            assert np.array_equal(seq.read_frame(i), src[i]), (H, W, i)
        assert np.array_equal(mv[3], co.bbme(src[3], src[4], 16, 2, 3, 0)), (H, W)
        seq.close()
