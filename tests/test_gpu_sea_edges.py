"""Edge blocks of the elimination kernels (bbme_sea.hip: lower_bounds with GUARD_ROWS / GUARD_ALL): candidates outside the
frame and the padding candidates of a partial size class are penalised, not skipped -- the row through the start value of
the inner v_sad_u16, the column through a lane mask formed once -- and a patch without valid candidates must still end
as 0xFFFFE000 | index.  Needs an MI355X.

Every case compares the motion field of Sequence.bbme(1, 16, sw, 0, pnorm) with the C oracle bit for bit on 3 frames, with
GME_SEA_REDO=0 so that the elimination kernel itself answers (redo_tiles == 0).

Shapes: 32x48 (2 x 3 blocks) and 48x80 (3 x 5 blocks) -- every block touches the frame's edge in rows or in columns at every
window, most in both.  sw 4 .. 32 covers the size classes R = 2 .. 5; sw 12 (NC = 40 < 48) and sw 20 (NC = 56 < 64) are
the partial classes, where padding candidates and frame edges meet in the guarded body.  MSE at sw 8 and 32: the box
sums are shared.  Contents:
    noise         every bound decides;
    constant 128  every cost ties: the answer is the first valid candidate in scan order, so an invalid one leaking in
                  shows at once;
    0 / 255       frames 0, 255, 0: the zero padding outside the frame matches the all-zero frame exactly, so any invalid
                  candidate that forms a key would win, and valid bounds sit at 65280, the top of the real range -- a
                  penalty that is too small shows here.
One case at 112x176, sw 16 with the persistent kernel forced: plan() picks 2x4 tiles there, i.e. the geometry-fixed
instance of the benchmark, with edge tiles on all four sides.
"""
import numpy as np
import pytest

from helpers import c_oracle

pytestmark = pytest.mark.gpu

SIZES = ((32, 48), (48, 80))                               # (H, W)
SWS = (4, 8, 12, 16, 20, 24, 32)
CONTENTS = ("noise", "const128", "0_255")
CASES = [(h, w, sw, 0, c) for (h, w) in SIZES for sw in SWS for c in CONTENTS]
CASES += [(h, w, sw, 1, c) for (h, w) in SIZES for sw in (8, 32) for c in CONTENTS]


@pytest.fixture(scope="module")
def native():
    import _gme_native
    assert "gfx950" in _gme_native.default_context().info()["name"]
    return _gme_native


def frames_of(content, h, w, seed):
    if content == "noise":
        return np.random.RandomState(seed).randint(0, 256, size=(3, h, w)).astype(np.uint8)
    if content == "const128":
        return np.full((3, h, w), 128, np.uint8)
    f = np.zeros((3, h, w), np.uint8)                       # pair 0: prev 0, cur 255; pair 1 the other way round
    f[1] = 255
    return f


def check(native, monkeypatch, frames, sw, pnorm, persist=None):
    monkeypatch.setenv("GME_SEA_REDO", "0")                 # read per launch: no brute-force redo of hostile tiles
    monkeypatch.setenv("GME_EXH_MFMA", "0")                 # MSE at sw <= 16 would otherwise take the matrix-core kernel
    if persist is not None:
        monkeypatch.setenv("GME_SEA_PERSIST", persist)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    try:
        seq.bbme(1, 16, sw, 0, pnorm)
        mv = seq.read_mv()
        info = ctx.last_bbme_info()
    finally:
        seq.close()
    print(frames.shape, "sw", sw, "pnorm", pnorm, info["plan"])
    assert "k_exh_sea16" in info["plan"], info["plan"]
    assert info["redo_tiles"] == 0, info
    co = c_oracle()
    for p in range(len(frames) - 1):
        assert np.array_equal(mv[p], co.bbme(frames[p], frames[p + 1], 16, sw, 0, pnorm)), (frames.shape, sw, pnorm, p, info["plan"])


@pytest.mark.parametrize("h,w,sw,pnorm,content", CASES)
def test_every_block_an_edge_block(native, monkeypatch, h, w, sw, pnorm, content):
    check(native, monkeypatch, frames_of(content, h, w, 2000 + 11 * sw + h + pnorm), sw, pnorm)


def test_edge_tiles_on_all_sides_persistent(native, monkeypatch):
    check(native, monkeypatch, frames_of("noise", 112, 176, 112176), 16, 0, persist="2")
