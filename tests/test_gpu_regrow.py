"""One Sequence asked for more than it has allocated: every call that keeps device buffers in the sequence runs first at a
small demand and then at a larger one on the SAME sequence, so its buffers grow, its groups are sized anew and the borrowed
motion field of the level -1 fit moves.  Every output is compared byte for byte with the same call on a freshly created
sequence of the same frames (tests/test_gpu_reuse.py takes every pass through growing and shrinking demands against its
definition; the rest of the suite makes a fresh sequence per shape).  Successful calls only: allocation failures are the
business of tests/test_dev_buf_host.py.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, H, W = 4, 80, 112          # W is no multiple of 64: uploads go through the staging buffer; level 1 = 40 x 56, level 0 = 20 x 28
SW, EXHAUSTIVE, MAE = 8, 0, 0


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


@pytest.fixture(scope="module")
def frames():
    import synth
    return np.ascontiguousarray(synth.sequence(20261, 0, N, H, W))


def same_bytes(got, want, where):
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), where
        for k in want:
            same_bytes(got[k], want[k], where + (k,))
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), where
        for k, (g, w) in enumerate(zip(got, want)):
            same_bytes(g, w, where + (k,))
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), where


def grows(native, frames, step, demands):
    """step(seq, *demand) at each demand in turn on one sequence, each against the same call on a fresh sequence."""
    ctx = native.default_context()
    reused = native.Sequence.from_frames(ctx, frames)
    for demand in demands:
        got = step(reused, *demand)
        fresh = native.Sequence.from_frames(ctx, frames)
        want = step(fresh, *demand)
        fresh.close()
        same_bytes(got, want, (step.__name__,) + tuple(demand))
    reused.close()


def affine(pairs):
    return np.array([[-3.0 + 0.5 * k, 0.02, -0.01, 2.0 - 0.25 * k, 0.015, 0.01] for k in range(pairs)])


def field_steps(seq, fd, bs):
    """Steps 1 - 3: the motion field and its summary, the level -1 fit of it (stage buffers sized anew, gt borrowed from the
    field that has just moved), and the quarter-pel refinement, compensation and read-back."""
    pairs = N - fd
    seq.bbme(fd, bs, SW, EXHAUSTIVE, MAE)
    out = {"mv": seq.read_mv(), "summary": seq.mv_summary()}
    assert out["mv"].shape == (pairs, H // bs, W // bs, 2) and out["mv"].any()
    out["fit"] = np.array(seq.gme_fit(-1, affine(pairs), 0.3))
    out["fit_stage"] = seq.gme_read_stage(-1, pairs - 1)
    seq.subpel(fd, bs, MAE)
    out["qmv"] = seq.read_qmv()
    out["qsse"] = np.array(seq.compensate_qpel(fd, bs))
    out["qcomp"] = seq.read_compensated_range(0, pairs)
    return out


def test_motion_field_fit_and_quarter_pel(native, frames):
    grows(native, frames, field_steps, [(2, 16), (1, 8)])          # more pairs and a larger field


def staged(seq, bs, fd):
    p0, sums1 = seq.gme_begin_fit(fd, bs, 0.3)
    return {"p0": np.array(p0), "sums1": np.array(sums1), "stage": seq.gme_read_stage(1, 0)}


def test_staged_estimate(native, frames):
    grows(native, frames, staged, [(bs, fd) for bs in (16, 8, 16) for fd in (2, 1)])


def compensated(seq, order, fd):
    pairs = N - fd
    if order == 1:
        sse = seq.compensate(fd, 16, affine(pairs))
    else:
        second = np.tile([1e-4, -2e-4, 1e-4, -1e-4, 2e-4, 5e-5], (pairs, 1))
        sse = seq.compensate2(fd, 16, np.concatenate([affine(pairs), second], axis=1))
    out = {"sse": np.array(sse), "frames": seq.read_compensated_range(0, pairs), "last": seq.read_compensated(pairs - 1)}
    assert not np.array_equal(out["frames"][0], seq.read_frame(0))
    return out


def test_compensation(native, frames):
    grows(native, frames, compensated, [(1, 2), (1, 1)])
    grows(native, frames, compensated, [(2, 2), (2, 1)])
    grows(native, frames, compensated, [(1, 2), (2, 2), (2, 1), (1, 1)])       # the order-2 field grows under the shared group


def direct(seq, fd):
    p = np.tile([1, 0, -2.5 * fd, 0, 1, 1.5 * fd, 0, 0], (N - fd, 1)).astype(np.float64)
    return seq.direct_eval(fd, 1, p, 0.1)


def test_direct_evaluation(native, frames):
    grows(native, frames, direct, [(2,), (1,)])


def mosaic_and_masks(seq, grow):
    pan = np.array([[1, 0, -5.0 * k, 0, 1, 3.0 * k, 0, 0] for k in range(N)], np.float64)       # synth.frame's pan
    inv = pan.copy()
    inv[:, 2], inv[:, 5] = -pan[:, 2], -pan[:, 5]
    Hc, Wc = H + grow, W + grow
    seq.mosaic(0, inv, None, 0, 0, Hc, Wc, 0, True)
    sprite, count = seq.read_mosaic()
    assert sprite.shape == (Hc, Wc) and count.max() > 1
    known, moving = seq.moving_masks(0, pan, None, 0, 0, 16, 2)
    return {"sprite": sprite, "count": count, "known": known, "moving": moving, "masks": seq.read_masks_range(0, N)}


def test_mosaic_and_masks(native, frames):
    grows(native, frames, mosaic_and_masks, [(0,), (32,)])
