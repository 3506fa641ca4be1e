"""Host frames -> planes: the three host layouts of upload_copies (csrc/gme_api.hip) on both intake paths,
gme_seq_upload and the chunked gme_seq_bbme_streamed.  Needs an MI355X.

Shapes (five frames of noise each), by what a contiguous stack does:
  (33, 50)  rows narrower than the 64-byte plane pitch: linear copy + k_repack (its byte path, W % 4 != 0)
  (32, 64)  pitch == W and 32 * 64 is a multiple of 256: planes back to back, ONE 2-D copy for all frames
  (33, 64)  pitch == W, but 2112 bytes round up to a plane stride of 2304: one 2-D copy per frame
and two strided views of larger arrays: `big` (frame stride != row stride * H: per-frame copies at every shape) and
`wide` (frame stride == row stride * H: the single 2-D copy at (32, 64), per-frame copies otherwise).
Every case: the planes hold the source, the fields are the C oracle's, and a resident search on the same sequence
returns the same fields.
"""
import numpy as np
import pytest

from helpers import c_oracle

pytestmark = pytest.mark.gpu

N, BS = 5, 16
SHAPES = [(33, 50), (32, 64), (33, 64)]
# (search window, procedure, norm): exhaustive MAE; exhaustive MSE with the table of box sums of squares (kind 1) and with
# the signed table of the matrix-core kernel (kind 2, windows that are multiples of 8); diamond
SEARCHES = [(4, 0, 0), (4, 0, 1), (8, 0, 1), (2, 3, 1)]
_stacks, _fields = {}, {}


@pytest.fixture(scope="module")
def native():
    import _gme_native
    ctx = _gme_native.default_context()
    assert "gfx950" in ctx.info()["name"]
    return _gme_native


def stack(shape):
    """uint8[N, H, W] noise, one read-only array per shape."""
    if shape not in _stacks:
        a = np.random.default_rng(1000 * shape[0] + shape[1]).integers(0, 256, (N,) + shape, dtype=np.uint8)
        a.flags.writeable = False
        _stacks[shape] = a
    return _stacks[shape]


def oracle_fields(src, fd, search, key=None):
    """int32[N - fd, h, w, 2] of the C oracle; computed once per key and kept read-only."""
    if key is not None and (key, fd, search) in _fields:
        return _fields[(key, fd, search)]
    sw, proc, pn = search
    out = np.stack([c_oracle().bbme(src[p], src[p + fd], BS, sw, proc, pn) for p in range(len(src) - fd)])
    out.flags.writeable = False
    if key is not None:
        _fields[(key, fd, search)] = out
    return out


def host_layout(src, layout):
    """The frames of `src` as a contiguous stack or as a strided view of a larger array filled with other bytes."""
    n, H, W = src.shape
    if layout == "contiguous":
        return np.array(src)
    hold = np.full((n, H + 3, W + 6) if layout == "big" else (n, H, W + 6), 0xA5, np.uint8)
    view = hold[:, :H, :W]
    view[...] = src
    assert not view.flags.c_contiguous and view.strides[2] == 1 and view.strides[1] == W + 6
    assert (view.strides[0] == view.strides[1] * H) == (layout == "wide")
    return view


def assert_planes(seq, src):
    for i in range(len(src)):
        assert np.array_equal(seq.read_frame(i), src[i]), i


@pytest.mark.parametrize("shape", SHAPES)
def test_upload_whole_stack_and_one_slot(native, shape):
    """Sequence.upload of the whole stack, then of one other frame into slot 3: every plane holds its source (the slot's
    neighbours included) and the resident search gives the oracle's fields both times."""
    src = stack(shape)
    seq = native.Sequence(native.default_context(), N, *shape)
    seq.upload(0, src)
    assert_planes(seq, src)
    for search in SEARCHES:
        seq.bbme(1, BS, *search)
        assert np.array_equal(seq.read_mv(), oracle_fields(src, 1, search, shape)), search
    changed = np.array(src)
    changed[3] = np.random.default_rng(7).integers(0, 256, shape, dtype=np.uint8)
    seq.upload(3, changed[3:4])
    assert_planes(seq, changed)
    for search in SEARCHES:                                  # the tables of the old frame 3 must not be reused
        seq.bbme(1, BS, *search)
        assert np.array_equal(seq.read_mv(), oracle_fields(changed, 1, search)), search
    seq.close()


@pytest.mark.parametrize("layout", ["contiguous", "big", "wide"])
@pytest.mark.parametrize("shape", SHAPES)
def test_streamed_layouts(native, shape, layout):
    """bbme_streamed from each host layout, in chunks of 1, 2 and 8 frames (8: one chunk; 1 with frame distance 2: the
    first two chunks bring no pair) at frame distance 1 and 2."""
    src = stack(shape)
    frames = host_layout(src, layout)
    seq = native.Sequence(native.default_context(), N, *shape)
    for chunk in (1, 2, 8):
        for fd in (1, 2):
            for search in SEARCHES:
                case = (chunk, fd, search)
                got = seq.bbme_streamed(frames, fd, BS, *search, chunk_frames=chunk).copy()
                assert got.shape == (N - fd, shape[0] // BS, shape[1] // BS, 2), case
                assert_planes(seq, src)
                assert np.array_equal(got, oracle_fields(src, fd, search, shape)), case
                seq.bbme(fd, BS, *search)                    # the frames stay resident
                assert np.array_equal(seq.read_mv(), got), case
    seq.close()
