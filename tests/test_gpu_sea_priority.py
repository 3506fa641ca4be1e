"""Elimination search (bbme_sea.hip, bbme_sea_mse.hip): the paths of a tile on which a wave's priority is raised or
lowered, or on which the phase-stamp variant reads its clock.  Needs an MI355X.

Priority and stamps cannot change a result: every pair of every case is compared with the C oracle bit for bit, and the
statistics of the noise and synthetic cases equal what the PARENT commit's library reported on the same inputs.

Cases (spans: box sums A', phase E's chunks, C2 .. D of a crowded block; exits: the redo return behind phase D's barrier, the
last tile of a workgroup, a workgroup without tiles, the one-tile kernel):
    several chunks        48x80 uniform noise, sw 16, GME_SEA_REDO=0, persistent dynamic: every block is an edge block and a
                          tile's list runs to several phase-E chunks (asserted from `listed`), so a raise and a lower around
                          a chunk repeat inside one tile
    redo return           112x176, 258 pairs of uniform noise, redo on, persistent dynamic and static: tiles leave behind phase
                          D's barrier with a box-sum or C2 span behind them, under the dynamic schedule in streaks and bursts
    empty XCD classes     the same shape on the synthetic generator's frames, 5 pairs: three XCD classes have no tile and
                          their workgroups return before the first one
    C2 engaged            tests/golden/g9_pan240seq.npz, 8 pairs, default quota: `listed` > `surviving`
    R = 5                 32x96 at sw 32 in the geometry-fixed instance; 32x96 at sw 8 with run-time geometry; MSE on the vector
                          unit (GME_EXH_MFMA=0) at sw 16 and sw 32 on 48x80
    statistics            ctx.last_bbme_info()'s patches / surviving / listed / redo_tiles of the noise and synthetic cases in
                          the one-tile kernel and under the static schedule equal tests/golden/sea_priority_stats.json,
                          recorded on an MI355X from the parent commit's library before the change (never recomputed from
                          the code under test); where an input is also in sea_bound_minima_stats.json or
                          sea_list_stats.json the files agree.
"""
import json
import os
import re

import numpy as np
import pytest

from helpers import GOLDEN_DIR
from test_gpu_sea_persistent_walk import PERIOD, oracle_fields, periodic

pytestmark = pytest.mark.gpu

H0, W0 = 112, 176
STAT_KEYS = ("patches", "surviving", "listed", "redo_tiles")
STATS_JSON = os.path.join(GOLDEN_DIR, "sea_priority_stats.json")


@pytest.fixture(scope="module")
def native():
    import _gme_native
    assert "gfx950" in _gme_native.default_context().info()["name"]
    return _gme_native


def small_noise_frames():
    return np.random.RandomState(4880).randint(0, 256, size=(4, 48, 80)).astype(np.uint8)


def noise_frames():
    return np.random.RandomState(112176).randint(0, 256, size=(259, H0, W0)).astype(np.uint8)


def synth_frames():
    import synth
    return np.ascontiguousarray(synth.sequence(4711, 0, 6, H0, W0))


def pan240_frames():
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN_DIR, "g9_pan240seq.npz"))["frames"][:9])


def fields_of(frames, sw, pnorm=0):
    return np.stack(oracle_fields([(frames[p], frames[p + 1]) for p in range(len(frames) - 1)], sw, pnorm))


@pytest.fixture(scope="module")
def cases():
    """name -> (frames, oracle fields at sw 16, MAE), each computed once."""
    made = {}
    makers = {"small_noise": small_noise_frames, "noise": noise_frames, "synth": synth_frames, "pan240": pan240_frames}

    def get(name):
        if name not in made:
            frames = makers[name]()
            made[name] = (frames, fields_of(frames, 16))
        return made[name]
    return get


def search(native, monkeypatch, frames, sw, env, pnorm=0):
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
    assert "k_exh_sea16" in info["plan"] and ("_mse" in info["plan"]) == bool(pnorm), info["plan"]
    return mv, info


def tiles_and_waves(info, frames):
    tr, tc = map(int, re.search(r"tiles (\d+)x(\d+)", info["plan"]).groups())
    n, h, w = frames.shape
    return (n - 1) * -(-(h // 16) // tr) * -(-(w // 16) // tc), tr * tc


# ---- several phase-E chunks per tile ---------------------------------------------------------------------------------
def test_lists_of_several_chunks(native, monkeypatch, cases):
    frames, want = cases("small_noise")
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_REDO": "0", "GME_SEA_PERSIST": "2"})
    assert "persistent-dynamic" in info["plan"], info["plan"]
    assert info["redo_tiles"] == 0, info
    tiles, waves = tiles_and_waves(info, frames)
    # a chunk is 16 entries per wave (four lanes per patch at R = 3).  Half of the tiles of a 3 x 5 block grid are ragged
    # (15 blocks in four 2x4 tiles), so only the mean is asserted: lists that are longer than two chunks on average
    # mean that some tile ran three or more, i.e. a raise and a lower repeated inside it
    assert info["listed"] > 2 * 16 * waves * tiles, (info, tiles, waves)
    assert np.array_equal(mv, want)


# ---- the redo return, streaks and bursts -----------------------------------------------------------------------------
@pytest.mark.parametrize("persist", ["2", "1"])
def test_redo_return(native, monkeypatch, cases, persist):
    frames, want = cases("noise")
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_PERSIST": persist})
    assert ("persistent-dynamic" if persist == "2" else "persistent-static") in info["plan"], info["plan"]
    tiles, _ = tiles_and_waves(info, frames)
    # some tiles leave by the redo return, the others are searched by the elimination kernel itself
    assert 0 < info["redo_tiles"] < tiles, (info, tiles)
    assert np.array_equal(mv, want)


# ---- workgroups that return before their first tile ------------------------------------------------------------------
def test_empty_xcd_classes(native, monkeypatch, cases):
    frames, want = cases("synth")
    assert len(frames) - 1 == 5
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_PERSIST": "2"})
    assert "persistent-dynamic" in info["plan"], info["plan"]
    assert info["surviving"] > 0, info
    assert np.array_equal(mv, want)


# ---- C2 engaged ------------------------------------------------------------------------------------------------------
def test_ordered_evaluation_engaged(native, monkeypatch, cases):
    frames, want = cases("pan240")
    assert frames.shape == (9, 240, 320)
    mv, info = search(native, monkeypatch, frames, 16, {})
    assert info["listed"] > info["surviving"] > 0, info
    assert np.array_equal(mv, want)


# ---- R = 5, run-time geometry, MSE on the vector unit ----------------------------------------------------------------
def test_fixed_r5_instance(native, monkeypatch):
    base, frames = periodic(32, 96, PERIOD + 2, 532)         # 2 x 6 blocks: one 2x6 tile (12 waves) per pair
    want = fields_of(np.concatenate([base, base[:1]]), 32)
    mv, info = search(native, monkeypatch, frames, 32, {"GME_SEA_PERSIST": "2"})
    assert " geometry-fixed" in info["plan"] and "k_exh_sea16p<5,7>" in info["plan"], info["plan"]
    assert np.array_equal(mv, want[np.arange(len(frames) - 1) % PERIOD])


def test_runtime_geometry_sw8(native, monkeypatch):
    base, frames = periodic(32, 96, PERIOD + 2, 508)
    want = fields_of(np.concatenate([base, base[:1]]), 8)
    mv, info = search(native, monkeypatch, frames, 8, {"GME_SEA_PERSIST": "2"})
    assert "k_exh_sea16p<2," in info["plan"] and "geometry-fixed" not in info["plan"], info["plan"]
    assert np.array_equal(mv, want[np.arange(len(frames) - 1) % PERIOD])


@pytest.mark.parametrize("sw", [16, 32])
def test_mse_on_the_vector_unit(native, monkeypatch, sw):
    frames = np.random.RandomState(4880 + sw).randint(0, 256, size=(4, 48, 80)).astype(np.uint8)
    mv, info = search(native, monkeypatch, frames, sw, {"GME_EXH_MFMA": "0", "GME_SEA_PERSIST": "2"}, pnorm=1)
    assert "k_exh_sea16p_mse<%d," % (3 if sw == 16 else 5) in info["plan"], info["plan"]
    assert np.array_equal(mv, fields_of(frames, sw, 1))


# ---- statistics against the parent commit's --------------------------------------------------------------------------
STAT_CASES = {
    # name: (case, environment beside GME_SEA_PERSIST)
    "noise_48x80_3_noredo": ("small_noise", {"GME_SEA_REDO": "0"}),
    "noise_112x176_258": ("noise", {}),
    "synth_112x176_5": ("synth", {}),
}
STAT_MODES = {"one_tile": "0", "static": "1"}               # GME_SEA_PERSIST
STAT_RUNS = [(c, m) for c in sorted(STAT_CASES) for m in sorted(STAT_MODES)]


@pytest.mark.parametrize("case,mode", STAT_RUNS)
def test_statistics_equal_the_parents(native, monkeypatch, cases, case, mode):
    recorded = json.load(open(STATS_JSON))["cases"][case][mode]
    name, env = STAT_CASES[case]
    frames, want = cases(name)
    mv, info = search(native, monkeypatch, frames, 16, dict(env, GME_SEA_PERSIST=STAT_MODES[mode]))
    assert ("one-tile" in info["plan"]) == (mode == "one_tile") and ("static" in info["plan"]) == (mode == "static"), info["plan"]
    assert {k: info[k] for k in STAT_KEYS} == {k: recorded[k] for k in STAT_KEYS}, (case, mode, info, recorded)
    assert np.array_equal(mv, want)


def test_recorded_statistics_agree_with_the_earlier_files():
    mine = json.load(open(STATS_JSON))["cases"]
    shared = 0
    for other in ("sea_bound_minima_stats.json", "sea_list_stats.json"):
        theirs = json.load(open(os.path.join(GOLDEN_DIR, other)))["cases"]
        for case in mine:
            for mode in mine[case]:
                if case in theirs and mode in theirs[case]:
                    shared += 1
                    assert {k: mine[case][mode][k] for k in STAT_KEYS} == {k: theirs[case][mode][k] for k in STAT_KEYS}, (other, case, mode)
    assert shared >= 2                                        # noise_112x176_258, one-tile, is in both
