"""Persistent elimination kernels (bbme_sea_common.h: persistent_tiles), second and later tiles of a workgroup.  Needs an MI355X.

The tile loop keeps only the tile geometry in registers; planes, frame size, schedule constants, counters and lists are
read from the kernel-argument segment by the block that needs them (launch_args), and what follows from them -- tiles of
the XCD, G / 8, the counter's address, the plane's extent -- is recomputed there.  A wrong offset or a value that goes
stale would show from the second tile on, so every walking case here makes each resident workgroup process several
tiles: `grid` is read from the launch plan and `tiles per XCD >= 3 * grid / 8` is asserted (no CU count assumed).
Every pair's field is compared with the C oracle bit for bit.

Cases:
    112x176, sw 16, 259 synthetic frames      2x4 tiles: the geometry-fixed instance of the benchmark, 12 tiles per pair,
                                              ragged on both sides; 258 pairs = uneven XCD classes (258 % 8 != 0);
                                              MAE with the dynamic and the static schedule, MSE with the dynamic one
    uniform noise, same shape                 hostile tiles: streaks and bursts read redo_list, status and the tile counter
                                              (redo_tiles > 0); once more with the redo kernel switched off
    48x80 (3x5 blocks), sw 0 / 8 / 24         the run-time-geometry instances R = 1, 2, 4
    32x96 (2x6 blocks), sw 32                 the smallest frame for which plan() picks 2x6 tiles: the geometry-fixed R = 5
                                              instance
    5 pairs                                   three XCD classes have no pair and return before their first tile; the
                                              statistics must add up to what the one-tile kernel reports (one tile per
                                              workgroup in both, so the third probe is the zero vector in both)

The small shapes need several hundred pairs for three tiles per workgroup.  Their sequences repeat K = 17 distinct
synthetic frames (frame i = base[i % 17]), so the oracle searches 17 distinct pairs and every pair of the sequence is
compared with the oracle's field for its two frames.  References are computed once per module, on a thread pool (the
oracle is a plain C function; ctypes drops the GIL).
"""
import concurrent.futures
import re

import numpy as np
import pytest

from helpers import c_oracle

pytestmark = pytest.mark.gpu

H0, W0 = 112, 176
PERIOD = 17


@pytest.fixture(scope="module")
def native():
    import _gme_native
    assert "gfx950" in _gme_native.default_context().info()["name"]
    return _gme_native


def oracle_fields(pairs_of_frames, sw, pnorm):
    """C oracle for a list of (prev, cur) -> list of int32[h, w, 2]."""
    co = c_oracle()
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        return list(pool.map(lambda pc: co.bbme(pc[0], pc[1], 16, sw, 0, pnorm), pairs_of_frames))


@pytest.fixture(scope="module")
def synth_frames():
    import synth
    return np.ascontiguousarray(synth.sequence(4711, 0, 259, H0, W0))


@pytest.fixture(scope="module")
def noise_frames():
    return np.random.RandomState(112176).randint(0, 256, size=(259, H0, W0)).astype(np.uint8)


@pytest.fixture(scope="module")
def refs(synth_frames, noise_frames):
    """Lazily computed oracle fields of the 258-pair sequences, keyed by (content, pnorm)."""
    cache = {}

    def get(content, pnorm):
        if (content, pnorm) not in cache:
            f = synth_frames if content == "synth" else noise_frames
            cache[(content, pnorm)] = np.stack(oracle_fields([(f[p], f[p + 1]) for p in range(len(f) - 1)], 16, pnorm))
        return cache[(content, pnorm)]
    return get


def search(native, monkeypatch, frames, sw, pnorm, env):
    monkeypatch.setenv("GME_EXH_MFMA", "0")                 # MSE at sw <= 16 would otherwise take the matrix-core kernel
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    try:
        seq.bbme(1, 16, sw, 0, pnorm)
        mv = seq.read_mv()
        info = ctx.last_bbme_info()
    finally:
        seq.close()
    print(frames.shape, "sw", sw, "pnorm", pnorm, env, info)
    return mv, info


def assert_walks(info, frames):
    """Every resident workgroup gets at least three tiles: tiles per XCD >= 3 * grid / 8, grid from the plan."""
    plan = info["plan"]
    assert "persistent" in plan, plan
    grid = int(re.search(r"grid (\d+)", plan).group(1))
    tr, tc = map(int, re.search(r"tiles (\d+)x(\d+)", plan).groups())
    n, h, w = frames.shape
    tiles_per_pair = -(-(h // 16) // tr) * -(-(w // 16) // tc)
    tiles_per_xcd = -(-(n - 1) // 8) * tiles_per_pair
    print("grid", grid, "tiles per pair", tiles_per_pair, "tiles per XCD", tiles_per_xcd)
    assert grid % 8 == 0 and tiles_per_xcd >= 3 * grid // 8, (plan, tiles_per_xcd)
    return tiles_per_pair


@pytest.mark.parametrize("pnorm,persist", [(0, "2"), (0, "1"), (1, "2")])
def test_fixed_geometry_walk(native, monkeypatch, synth_frames, refs, pnorm, persist):
    mv, info = search(native, monkeypatch, synth_frames, 16, pnorm, {"GME_SEA_PERSIST": persist})
    assert " geometry-fixed" in info["plan"] and ("dynamic" if persist == "2" else "static") in info["plan"], info["plan"]
    assert assert_walks(info, synth_frames) == 12
    assert np.array_equal(mv, refs("synth", pnorm))


@pytest.mark.parametrize("redo", [True, False])
def test_hostile_content_walk(native, monkeypatch, noise_frames, refs, redo):
    mv, info = search(native, monkeypatch, noise_frames, 16, 0, {"GME_SEA_PERSIST": "2", "GME_SEA_REDO": "1" if redo else "0"})
    assert_walks(info, noise_frames)
    assert (info["redo_tiles"] > 0) == redo, info
    assert np.array_equal(mv, refs("noise", 0))


def periodic(h, w, count, seed):
    import synth
    base = np.ascontiguousarray(synth.sequence(seed, 0, PERIOD, h, w))
    return base, np.ascontiguousarray(base[np.arange(count) % PERIOD])


def check_periodic(native, monkeypatch, h, w, sw, pairs, seed):
    base, frames = periodic(h, w, pairs + 1, seed)
    want = np.stack(oracle_fields([(base[k], base[(k + 1) % PERIOD]) for k in range(PERIOD)], sw, 0))
    mv, info = search(native, monkeypatch, frames, sw, 0, {"GME_SEA_PERSIST": "2"})
    assert "k_exh_sea16p" in info["plan"], info["plan"]
    assert_walks(info, frames)
    assert np.array_equal(mv, want[np.arange(pairs) % PERIOD])
    return info


def pairs_for(native, tiles_per_pair, waves_per_tile):
    """Pairs that give three tiles per workgroup even where a CU holds as many workgroups as its 32 wave slots allow
    (an upper bound: LDS may allow fewer); assert_walks checks the launch itself."""
    cus = native.default_context().info()["cu_count"]
    per_xcd = 3 * (32 // waves_per_tile) * cus // 8
    return 8 * -(-per_xcd // tiles_per_pair) + 2            # + 2: uneven XCD classes


@pytest.mark.parametrize("sw", [0, 8, 24])
def test_runtime_geometry_walk(native, monkeypatch, sw):
    # 3 x 5 blocks: plan() picks 2x2 tiles (4 waves, 6 tiles per pair) in all three size classes
    info = check_periodic(native, monkeypatch, 48, 80, sw, pairs_for(native, 6, 4), 100 + sw)
    assert "geometry-fixed" not in info["plan"] and "<%d," % ((2 * sw + 31) // 16) in info["plan"], info["plan"]


def test_fixed_geometry_r5_walk(native, monkeypatch):
    # 2 x 6 blocks: one 2x6 tile (12 waves) per pair
    info = check_periodic(native, monkeypatch, 32, 96, 32, pairs_for(native, 1, 12), 532)
    assert " geometry-fixed" in info["plan"] and "<5,7>" in info["plan"] and "tiles 2x6" in info["plan"], info["plan"]


def test_empty_xcd_classes(native, monkeypatch, synth_frames, refs):
    frames = synth_frames[:6]
    mv, info = search(native, monkeypatch, frames, 16, 0, {"GME_SEA_PERSIST": "2"})
    assert "persistent-dynamic" in info["plan"], info["plan"]
    assert np.array_equal(mv, refs("synth", 0)[:5])
    mv1, one = search(native, monkeypatch, frames, 16, 0, {"GME_SEA_PERSIST": "0"})
    assert "one-tile" in one["plan"], one["plan"]
    assert np.array_equal(mv1, mv)
    for key in ("patches", "surviving", "listed", "redo_tiles"):
        assert info[key] == one[key], (key, info, one)
    assert info["surviving"] > 0
