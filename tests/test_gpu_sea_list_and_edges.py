"""Elimination search (bbme_sea.hip): one list reservation per wave and tile, "interior block" carried in the list entry.
Needs an MI355X.

Phase D reserves the list slots of a wave's R column groups with ONE returning LDS add (ballots, popcounts and
mbcnt give every lane its slot), so the order of the entries inside the list differs from the parent's; an entry's bit 29
says that the patch's block has its whole window inside the frame, and phase E (and C2's own slots) take the window limits
only where it is clear.  Every field of every case is compared with the C oracle bit for bit (MAE).

Cases:
    mixed tiles           112x176, sw 16, 258 synthetic pairs in the geometry-fixed k_exh_sea16p<3, 5, 36>, three tiles per
                          resident workgroup (asserted from the launch plan): border tiles hold interior and edge blocks,
                          whose entries meet in one phase-E wave.  Dynamic schedule, static schedule, one-tile kernel.
    every block an edge   32x48 and 48x80, sw 4 / 12 / 16 / 20 / 32 (the partial size classes among them); uniform noise,
                          constant 128 and all-0 against all-255; the redo kernel is off so that the elimination kernel answers
    long lists            uniform noise at 112x176 with GME_SEA_REDO=0: lists of several phase-E chunks, lanes that push all
                          R entries.  The list's length (`listed`; nothing is scored outside it: == `surviving`) must be what
                          the parent's one-at-a-time reservation counted: `patches` minus what the bound removed, 2 800 848 of
                          3 814 272.  With the redo kernel on the one-tile kernel must hand over the parent's 1294 tiles.
    ties                  constant frames and frames flat in halves, split vertically and horizontally: the first strict
                          minimum in scan order must hold whatever the list order; one-tile and persistent kernel
    C2                    tests/golden/g9_pan240seq.npz with GME_SEA_QUOTA at its default and at 0 (the `own` slots carry
                          the interior bit too)
    R = 5                 the geometry-fixed k_exh_sea16p<5, 7, 38> on 32x96 at sw 32, and run-time geometry at sw 8 and 24
    statistics            ctx.last_bbme_info() (patches, surviving, listed, redo_tiles) equals what the PARENT commit's library
                          reported (tests/golden/sea_list_stats.json, recorded on an MI355X before the change, never
                          recomputed from the code under test), in the one-tile kernel and under the static schedule; where an
                          input is also in tests/golden/sea_bound_minima_stats.json the two files must agree.
"""
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN_DIR
from test_gpu_sea_bound_minima import (STAT_KEYS, assert_exact, guard_frames, noise_frames, pan240_frames, search, synth_frames,
                                       tie_frames, tiles_per_workgroup)
from test_gpu_sea_persistent_walk import PERIOD, oracle_fields, pairs_for, periodic

pytestmark = pytest.mark.gpu

STATS_JSON = os.path.join(GOLDEN_DIR, "sea_list_stats.json")
EARLIER_JSON = os.path.join(GOLDEN_DIR, "sea_bound_minima_stats.json")
MODES = {"one_tile": "0", "static": "1", "dynamic": "2"}       # GME_SEA_PERSIST


@pytest.fixture(scope="module")
def native():
    import _gme_native
    assert "gfx950" in _gme_native.default_context().info()["name"]
    return _gme_native


def fields_of(frames, sw):
    return np.stack(oracle_fields([(frames[p], frames[p + 1]) for p in range(len(frames) - 1)], sw, 0))


@pytest.fixture(scope="module")
def cases():
    """Inputs and their oracle fields, computed once per module and on demand."""
    makers = {"synth": synth_frames, "noise": noise_frames, "pan240": pan240_frames, "ties": lambda: tie_frames(112, 176)}
    cache = {}

    def get(name):
        if name not in cache:
            frames = makers[name]()
            cache[name] = (frames, fields_of(frames, 16))
        return cache[name]
    return get


def edge_frames(content, h, w, seed):
    if content == "128":
        return np.full((3, h, w), 128, np.uint8)
    return guard_frames(content, h, w, seed)


def assert_mode(info, mode):
    plan = info["plan"]
    assert ("one-tile" in plan) == (mode == "one_tile") and ("-static" in plan) == (mode == "static") \
        and ("-dynamic" in plan) == (mode == "dynamic"), plan


# ---- mixed tiles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dynamic", "static", "one_tile"])
def test_mixed_tiles(native, monkeypatch, cases, mode):
    frames, want = cases("synth")
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_PERSIST": MODES[mode]})
    assert_mode(info, mode)
    if mode != "one_tile":
        assert "k_exh_sea16p<3,5>" in info["plan"] and " geometry-fixed" in info["plan"], info["plan"]
        assert tiles_per_workgroup(info, frames) >= 3, info["plan"]
    assert info["redo_tiles"] == 0 and 0 < info["surviving"] < info["patches"], info
    assert np.array_equal(mv, want)


# ---- every block an edge block -------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["noise", "128", "0-255"])
@pytest.mark.parametrize("sw", [4, 12, 16, 20, 32])
@pytest.mark.parametrize("h,w", [(32, 48), (48, 80)])
def test_every_block_an_edge_block(native, monkeypatch, h, w, sw, content):
    frames = edge_frames(content, h, w, 9100 + 17 * sw + w)
    mv, info = search(native, monkeypatch, frames, sw, {"GME_SEA_REDO": "0"})
    assert info["redo_tiles"] == 0, info
    assert_exact(mv, frames, sw, info)


# ---- long lists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dynamic", "static", "one_tile"])
def test_long_lists(native, monkeypatch, cases, mode):
    frames, want = cases("noise")
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_REDO": "0", "GME_SEA_PERSIST": MODES[mode]})
    assert_mode(info, mode)
    assert info["redo_tiles"] == 0, info
    # 8 waves x 64 lanes x 3 patches per tile, 128 list entries per phase-E chunk
    assert info["listed"] / (info["patches"] / (8 * 64 * 3)) > 4 * 128, info
    assert info["listed"] == info["surviving"], info          # nothing is scored outside the list on this content
    if mode != "dynamic":                                      # dynamic: the third probe depends on who drew which tile
        recorded = json.load(open(STATS_JSON))["cases"]["noise_112x176_258_noredo"][mode]
        assert info["patches"] == recorded["patches"] == 3814272 and info["listed"] == recorded["listed"] == 2800848, (info, recorded)
    assert np.array_equal(mv, want)


def test_long_lists_hand_the_same_tiles_over(native, monkeypatch, cases):
    frames, want = cases("noise")
    recorded = json.load(open(STATS_JSON))["cases"]["noise_112x176_258"]["one_tile"]
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_REDO": "1", "GME_SEA_PERSIST": "0"})
    assert info["redo_tiles"] == recorded["redo_tiles"] == 1294, (info, recorded)
    assert np.array_equal(mv, want)
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_REDO": "1", "GME_SEA_PERSIST": "2"})
    assert info["redo_tiles"] > 0, info
    assert np.array_equal(mv, want)


# ---- ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dynamic", "one_tile"])
def test_ties_whatever_the_list_order(native, monkeypatch, cases, mode):
    frames, want = cases("ties")
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_REDO": "0", "GME_SEA_PERSIST": MODES[mode]})
    assert_mode(info, mode)
    assert np.array_equal(mv, want)


def test_ties_every_block_an_edge_block(native, monkeypatch):
    frames = tie_frames(48, 80)
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_REDO": "0", "GME_SEA_PERSIST": "2"})
    assert_exact(mv, frames, 16, info)


# ---- C2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quota", [None, "0"])
@pytest.mark.parametrize("mode", ["static", "one_tile"])
def test_ordered_evaluation_slots(native, monkeypatch, cases, mode, quota):
    frames, want = cases("pan240")
    env = {"GME_SEA_PERSIST": MODES[mode]}
    if quota is not None:
        env["GME_SEA_QUOTA"] = quota
    mv, info = search(native, monkeypatch, frames, 16, env)
    assert_mode(info, mode)
    assert (info["listed"] > info["surviving"]) == (quota is None) and info["surviving"] > 0, info
    assert np.array_equal(mv, want)


# ---- R = 5, and run-time geometry ------------------------------------------------------------------------------------
def test_fixed_r5_instance(native, monkeypatch):
    pairs = pairs_for(native, 1, 12)                          # 2 x 6 blocks: one 2x6 tile (12 waves) per pair
    base, frames = periodic(32, 96, pairs + 1, 9532)
    want = np.stack(oracle_fields([(base[k], base[(k + 1) % PERIOD]) for k in range(PERIOD)], 32, 0))
    mv, info = search(native, monkeypatch, frames, 32, {"GME_SEA_PERSIST": "2"})
    assert " geometry-fixed" in info["plan"] and "k_exh_sea16p<5,7>" in info["plan"], info["plan"]
    assert np.array_equal(mv, want[np.arange(pairs) % PERIOD])


@pytest.mark.parametrize("sw", [8, 24])
@pytest.mark.parametrize("h,w", [(48, 80), (112, 176)])
def test_runtime_geometry(native, monkeypatch, h, w, sw):
    import synth
    frames = np.ascontiguousarray(synth.sequence(900 + sw, 0, 10, h, w))
    mv, info = search(native, monkeypatch, frames, sw, {"GME_SEA_PERSIST": "2"})
    assert "k_exh_sea16p<%d," % ((2 * sw + 31) // 16) in info["plan"] and "geometry-fixed" not in info["plan"], info["plan"]
    assert_exact(mv, frames, sw, info)


# ---- statistics against the parent commit's -------------------------------------------------------------------------
STAT_CASES = {
    # name: (frames, environment beside GME_SEA_PERSIST)
    "synth_112x176_258": (synth_frames, {}),
    "noise_112x176_258": (noise_frames, {}),
    "noise_112x176_258_noredo": (noise_frames, {"GME_SEA_REDO": "0"}),
    "pan240_8": (pan240_frames, {}),
    "pan240_8_quota0": (pan240_frames, {"GME_SEA_QUOTA": "0"}),
    "ties_112x176_6": (lambda: tie_frames(112, 176), {"GME_SEA_REDO": "0"}),
}
STAT_MODES = ("one_tile", "static")
# noise with the redo kernel on is compared in the one-tile kernel only: which tiles a persistent workgroup hands over
# depends on its earlier tiles
STAT_RUNS = [(c, m) for c in sorted(STAT_CASES) for m in STAT_MODES if (c, m) != ("noise_112x176_258", "static")]


@pytest.mark.parametrize("case,mode", STAT_RUNS)
def test_statistics_equal_the_parents(native, monkeypatch, case, mode):
    recorded = json.load(open(STATS_JSON))["cases"][case][mode]
    make, env = STAT_CASES[case]
    _, info = search(native, monkeypatch, make(), 16, dict(env, GME_SEA_PERSIST=MODES[mode]))
    assert_mode(info, mode)
    assert {k: info[k] for k in STAT_KEYS} == {k: recorded[k] for k in STAT_KEYS}, (case, mode, info, recorded)


def test_recorded_statistics_agree_with_the_earlier_file():
    new, old = json.load(open(STATS_JSON))["cases"], json.load(open(EARLIER_JSON))["cases"]
    shared = [(c, m) for c in old for m in old[c] if c in new and m in new[c]]
    assert len(shared) >= 9, shared
    for c, m in shared:
        assert {k: new[c][m][k] for k in STAT_KEYS} == {k: old[c][m][k] for k in STAT_KEYS}, (c, m)
