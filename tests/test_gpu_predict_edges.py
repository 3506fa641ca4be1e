"""The row frame the predict-a-plane kernels share (predict_rows of csrc/bbme_predict.h: k_compensate_qpel, k_compensate_vbs,
k_predict_bipred) and k_predict_gmc beside it, at the edges of that frame: a second workgroup column with a whole block, a partial
four-pixel group and pixels beyond the last whole block (9 x 262, whose rows are no multiple of the four of a workgroup), a frame
that ends on the column boundary (8 x 256), and one lane with a partial group and one remainder row band (6 x 7).  Block size 4,
seeded noise, the predicted plane byte for byte and its squared error against the host definitions subpel.compensate,
subpel.compensate_integer (on the vbs leaf field), bipred.predict and gmc.predict, through the Python entry points.

The one-shot calls (Context.bipred, Context.gmc) take their fields as they are, random in [-6, 6] (vbs_cases.FIELD_REACH), and
host frames whose rows are PAD bytes longer than the frame.  The two compensations exist on a resident sequence only, whose
frames are uploaded tight and whose field is the one a +-6 exhaustive search of the pair leaves (no call sets a sequence's field
to arbitrary values): on noise those vectors fill [-6, 6] as well, and since a compensation reads `previous` at the block MINUS
its vector, blocks near the border point outside although the search kept every candidate inside.

Every case is asserted, from the host arrays alone, not to be vacuous: the host prediction differs from the co-located
reference frame, and at least one whole block falls back to the kept pixel (SEED was chosen on the CPU for that: find_seed).
6 x 7 holds ONE whole block: where a predictor keeps or replaces a block as a whole (bidirectional, global motion) the two
conditions exclude each other there, so that block must be predicted and the kept pixels are the ones beyond it; the integer
compensation keeps single pixels and meets both; the quarter-pel compensation of that one block can only ever give the
co-located frame (not_vacuous says why), so its case checks the frame, the padding and the error sum on a block that falls
back.  Needs an MI355X."""
import numpy as np
import pytest

import vbs_cases as vc

pytestmark = pytest.mark.gpu

SHAPES = ((9, 262), (8, 256), (6, 7))
BS, PAD = 4, 5
WINDOW = vc.FIELD_REACH                                          # the sequence's search: vectors in [-6, 6]
WARP = np.array([1.0, 0.0, 2.5, 0.0, 1.0, 0.75, 0.0, 0.0])       # gmc: right of and below the frame's last blocks there is no sample
PREDICTORS = ("qpel", "vbs", "bipred", "gmc")
# chosen on the CPU (find_seed), with the C oracle's exhaustive search in the place of the sequence's
SEED = {
    ("qpel", (9, 262)): 0, ("qpel", (8, 256)): 0, ("qpel", (6, 7)): 0,
    ("vbs", (9, 262)): 0, ("vbs", (8, 256)): 0, ("vbs", (6, 7)): 0,
    ("bipred", (9, 262)): 0, ("bipred", (8, 256)): 0, ("bipred", (6, 7)): 8,
    ("gmc", (9, 262)): 1, ("gmc", (8, 256)): 0, ("gmc", (6, 7)): 0,
}
CASES = [(p, s) for p in PREDICTORS for s in SHAPES]


def inputs(predictor, shape):
    """(frames uint8[n, H, W] as views of rows PAD bytes longer, fields int32[m, H // BS, W // BS, 2] in [-6, 6]) of a case."""
    H, W = shape
    rng = np.random.default_rng(SEED[predictor, shape])
    frames = rng.integers(0, 256, size=(3, H, W + PAD), dtype=np.uint8)[:, :, :W]
    fields = rng.integers(-vc.FIELD_REACH, vc.FIELD_REACH + 1, size=(2, H // BS, W // BS, 2)).astype(np.int32)
    return frames, fields


def host(predictor, frames, fields):
    """-> (predicted uint8[H, W], the frame it is measured against, the co-located reference, whole blocks that fall back to the
    kept pixel) on the host; ``fields``: the quarter-pel field, the leaf field, (f0, f1) or (f,)."""
    import bipred
    import gmc
    import subpel
    H, W = frames[0].shape
    if predictor == "qpel":
        q = fields[0]
        kept = sum(subpel.interp_block(frames[0], 4 * j * BS - int(q[i, j, 0]), 4 * i * BS - int(q[i, j, 1]), BS) is None
                   for i in range(H // BS) for j in range(W // BS))
        return subpel.compensate(frames[0], q, BS), frames[1], frames[0], kept
    if predictor == "vbs":
        leaf = fields[0]
        a, b = np.mgrid[0:H // BS * BS, 0:W // BS * BS]
        sa, sb = a - np.repeat(np.repeat(leaf[:, :, 1], BS, 0), BS, 1), b - np.repeat(np.repeat(leaf[:, :, 0], BS, 0), BS, 1)
        out = (sa < 0) | (sa >= H) | (sb < 0) | (sb >= W)        # pixels of whole blocks whose source lies outside: kept
        kept = int(out.reshape(H // BS, BS, W // BS, BS).any(axis=(1, 3)).sum())
        return subpel.compensate_integer(frames[0], leaf, BS), frames[1], frames[0], kept
    if predictor == "bipred":
        mode, v0, v1 = bipred.decide(frames[0], frames[1], frames[2], fields[0], fields[1], BS, 1, 1, 0, 0)[:3]
        return bipred.predict(frames[0], frames[2], mode, v0, v1, BS), frames[1], frames[0], int((mode == bipred.NONE).sum())
    mode = gmc.decide(frames[0], frames[1], WARP, fields[0], BS, 0, 0)[0]
    return gmc.predict(frames[0], WARP, mode, fields[0], BS), frames[1], frames[0], int((mode == gmc.NONE).sum())


def not_vacuous(predictor, shape, want, ref, kept):
    """The two conditions of the module's docstring, on host arrays."""
    H, W = shape
    if (H // BS) * (W // BS) == 1 and predictor == "qpel":
        # the block at the origin: the search keeps origin + vector inside, the compensation reads at origin - vector, so a
        # vector other than zero falls back and the prediction is the co-located frame either way; the seed makes it fall back
        assert kept == 1 and np.array_equal(want, ref), (predictor, shape, kept)
        return
    assert not np.array_equal(want, ref), (predictor, shape, "the prediction is the co-located frame")
    if (H // BS) * (W // BS) == 1 and predictor != "vbs":
        assert kept == 0 and (H % BS or W % BS), (predictor, shape, kept)
    else:
        assert kept >= 1, (predictor, shape, "no block falls back")


def find_seed(predictor, shape, start=0):
    """How SEED was chosen (CPU only, not run by the tests): the first seed whose case is not vacuous, the sequence's field
    taken from the C oracle's exhaustive search."""
    import subpel
    from helpers import c_oracle
    for seed in range(start, start + 1000):
        SEED[predictor, shape] = seed
        frames, fields = inputs(predictor, shape)
        if predictor in ("qpel", "vbs"):
            mf = c_oracle().bbme(frames[0], frames[1], BS, WINDOW, 0, 0)
            fields = (subpel.refine(frames[0], frames[1], mf, BS, 0)[0],) if predictor == "qpel" else (mf,)
        want, _, ref, kept = host(predictor, frames, fields)
        try:
            not_vacuous(predictor, shape, want, ref, kept)
            return seed
        except AssertionError:
            pass
    raise ValueError("no seed makes %s at %r a case" % (predictor, shape))


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def device(native, predictor, frames, fields):
    """-> (predicted plane, its squared error, the fields the host prediction takes) of the device."""
    ctx = native.default_context()
    if predictor == "bipred":
        assert frames[1].strides[0] == frames.shape[2] + PAD
        got = ctx.bipred(frames[0], frames[1], frames[2], fields[0], fields[1], BS, 1, 1, 0, 0)
        return got[5], got[6], fields
    if predictor == "gmc":
        assert frames[1].strides[0] == frames.shape[2] + PAD
        got = ctx.gmc(frames[0], frames[1], WARP, fields[0], BS, 0, 0)
        return got[3], got[4], fields[:1]
    seq = native.Sequence.from_frames(ctx, np.ascontiguousarray(frames[:2]))
    try:
        seq.bbme(1, BS, WINDOW, 0, 0)
        if predictor == "qpel":
            seq.subpel(1, BS, 0, 2)
            field = seq.read_qmv()[0][0]
            sse = seq.compensate_qpel(1, BS)
        else:
            seq.vbs(1, BS, 0, 1, 0, 0)                           # depth 0: the leaf field is the searched one, the cell a block
            field = seq.read_vbs()[0][0]
            sse = seq.compensate_vbs(1, BS)
        return seq.read_compensated_range(0, 1)[0], int(sse[0]), (field,)
    finally:
        seq.close()


@pytest.mark.parametrize("predictor,shape", CASES)
def test_predicted_plane_and_sse(native, predictor, shape):
    import subpel
    frames, fields = inputs(predictor, shape)
    pred, sse, fields = device(native, predictor, frames, fields)
    want, against, ref, kept = host(predictor, frames, fields)
    not_vacuous(predictor, shape, want, ref, kept)
    assert pred.shape == want.shape and pred.dtype == np.uint8
    assert np.array_equal(pred, want), (predictor, shape, np.argwhere(pred != want)[:4])
    assert sse == subpel.sse(against, want), (predictor, shape)
