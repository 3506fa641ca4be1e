"""Box-sum phase of the elimination kernels (bbme_sea_common.h: box_sums8_ch): one QSAD per lane and window row, the
neighbour quad's half from lane + 1 (DPP wave_shl:1), whole row segments on the lanes of one wave, a donor lane behind a
segment whose last quad is read.  Needs an MI355X.

Every case compares the motion field of Sequence.bbme(1, 16, sw, 0, pnorm) with the C oracle bit for bit, on uniform
noise (nothing prunes, so almost every box sum decides a bound) and with GME_SEA_REDO=0, so that the elimination kernel
itself answers instead of handing hostile tiles to the brute-force kernel.

Tile shapes plan() picks for the cases (tr x tc, box-sum quads per row XQ against the `need` the bound phase reads):
    48x48     sw 0: 2x2 XQ 12 > 10   sw 4, 8: 2x2 XQ 14 == 14   sw 16: 2x2 XQ 20 > 18   sw 24: 2x2 XQ 22 == 22   sw 32: 2x2 XQ 28 > 26
    80x64     sw 0: 4x1 XQ 12 > 6    sw 4, 8: 4x1 XQ 10 == 10   sw 16: 4x2 XQ 20 > 18   sw 24: 4x2 XQ 22 == 22   sw 32: 4x2 XQ 28 > 26
    176x112   sw 0: 1x4 XQ 20 > 18   sw 4, 8: 1x4 XQ 22 == 22   sw 16: 2x4 XQ 28 > 26   sw 24: 2x4 XQ 30 == 30   sw 32: 2x6 XQ 44 > 42
    32x32     sw 32: 2x2 XQ 28 > 26 (most window rows and columns are zero padding)
    256x24    sw 16: 1x16 XQ 76 > 74 -- the only shape plan() picks whose row segment is longer than a wave: two pieces, lane
              63 of the first one only donates its quad, which the second piece starts with
    720x480   sw 16: 2x4 XQ 28 > 26; persistent (GME_SEA_PERSIST=2) it is the geometry-fixed instance, 0 the one-tile kernel
so tr = 1 (176x112 at sw <= 8), tr = 2 and tr = 4 are covered, XQ > need (last lane of a segment is padding) by every
R = 1, 3, 5 case, XQ == need (one more lane per segment computes quad XQ and stores nothing) by every R = 2 and R = 4
case, and segments per wave from 1 (XQ 44) to 5 (XQ 10 + donor, XQ 12), with and without idle lanes behind the last segment.
"""
import numpy as np
import pytest

from helpers import c_oracle

pytestmark = pytest.mark.gpu

SIZES = ((48, 48), (64, 80), (112, 176))                   # (H, W): one tile; a ragged last tile column; several tiles per row
CASES = [(h, w, sw, 0) for (h, w) in SIZES for sw in (0, 4, 8, 16, 24, 32)]
CASES += [(h, w, sw, 1) for (h, w) in SIZES for sw in (8, 32)]
CASES += [(32, 32, 32, 0), (32, 32, 32, 1), (24, 256, 16, 0)]


@pytest.fixture(scope="module")
def native():
    import _gme_native
    assert "gfx950" in _gme_native.default_context().info()["name"]
    return _gme_native


def noise_frames(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, h, w)).astype(np.uint8)


def sea_env(monkeypatch, persist=None):
    monkeypatch.setenv("GME_SEA_REDO", "0")             # read per launch: no brute-force redo of hostile tiles
    monkeypatch.setenv("GME_EXH_MFMA", "0")             # MSE at sw <= 16 would otherwise take the matrix-core kernel
    if persist is not None:
        monkeypatch.setenv("GME_SEA_PERSIST", persist)


def check(native, frames, sw, pnorm, plan_has):
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    try:
        seq.bbme(1, 16, sw, 0, pnorm)
        mv = seq.read_mv()
        info = ctx.last_bbme_info()
    finally:
        seq.close()
    print(frames.shape, "sw", sw, "pnorm", pnorm, info["plan"])
    assert all(s in info["plan"] for s in plan_has), info["plan"]
    assert info["redo_tiles"] == 0, info
    co = c_oracle()
    for p in range(len(frames) - 1):
        assert np.array_equal(mv[p], co.bbme(frames[p], frames[p + 1], 16, sw, 0, pnorm)), (frames.shape, sw, pnorm, p, info["plan"])


@pytest.mark.parametrize("h,w,sw,pnorm", CASES)
def test_noise_field_matches_oracle(native, monkeypatch, h, w, sw, pnorm):
    """Every window size class R = 1 .. 5 and the partial ones (NC < 16 R), MAE everywhere and MSE at sw 8 and 32."""
    sea_env(monkeypatch)
    check(native, noise_frames(4, h, w, 1000 + 7 * sw + h + pnorm), sw, pnorm, ["k_exh_sea16"])


@pytest.mark.parametrize("persist,plan_has", [("2", ["k_exh_sea16p<3,5>", "tiles 2x4", "geometry-fixed"]),
                                              ("0", ["k_exh_sea16<3>", "tiles 2x4", "one-tile"])])
def test_noise_720x480_fixed_geometry_and_one_tile(native, monkeypatch, persist, plan_has):
    """The benchmark's shape: the persistent kernel's geometry-fixed 2x4 instance (the segment length is a compile-time
    constant there) and the one-tile kernel (geometry at run time) on the same frames."""
    sea_env(monkeypatch, persist)
    check(native, noise_frames(9, 480, 720, 720), 16, 0, plan_has)
