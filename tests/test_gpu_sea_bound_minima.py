"""Elimination search (bbme_sea.hip), bound phase without per-candidate keys.  Needs an MI355X.

Phase B keeps the smallest BOUND of each patch, not `bound << 13 | local index`; the candidate the first probe scores is
recovered once per wave (smallest bound, then smallest lane, then smallest local index -- the old key's order), and the
bound's operand pairs are built vertically ([S(y, x), S(y + 8, x)]) so that a candidate's right-hand pair is the left-hand
pair of the candidate eight columns on.  Every pair of every case is compared with the C oracle bit for bit (MAE).

Cases:
    ties in the bound     48x80 and 112x176, sw 16 / 8 / 24: constant 128 against constant 128 (every bound is 0: the probe
                          must name local index 0 of lane 0), then two flat halves split vertically and horizontally, the
                          split moving between the frames (many candidates share the minimum across lanes and inside one)
    every guard form      32x48 and 48x80 (every block is an edge block), sw 4 / 12 / 20 (partial size classes with padding
                          candidates), 16 and 32; uniform noise and all-0 against all-255; the redo kernel is off there so
                          that the elimination kernel itself answers; 32x48 at sw 32 once more in k_exh_sea16p<5, 16, 0>,
                          the one instance that keeps horizontal pairs
    later tiles          112x176 with 258 pairs of noise and of the synthetic generator's frames in the geometry-fixed
                          k_exh_sea16p<3, 5, 36>, several tiles per workgroup (asserted from the launch plan); the
                          geometry-fixed R = 5 instance on 32x96
    C2 engaged            tests/golden/g9_pan240seq.npz (320x240, 8 pairs) with the ordered evaluation on (it must have
                          taken patches: `listed` > `surviving`) and with GME_SEA_QUOTA=0 (`listed` == `surviving`)
    statistics            ctx.last_bbme_info() of the noise, synthetic and pan240 cases equals what the PARENT commit's
                          library reported on the same inputs (tests/golden/sea_bound_minima_stats.json, recorded on an
                          MI355X before the change; never recomputed from the code under test).  A difference means the
                          probe or a gate sees another bound than before.  Recorded with the one-tile kernel and with the
                          persistent kernel's static schedule: the third probe is the vector the workgroup's previous tile
                          ended with, so under the dynamic schedule `surviving` depends on which workgroup drew which tile.
"""
import json
import os
import re

import numpy as np
import pytest

from helpers import GOLDEN_DIR, c_oracle
from test_gpu_sea_persistent_walk import PERIOD, oracle_fields, pairs_for, periodic

pytestmark = pytest.mark.gpu

H0, W0 = 112, 176
STAT_KEYS = ("patches", "surviving", "listed", "redo_tiles")
STATS_JSON = os.path.join(GOLDEN_DIR, "sea_bound_minima_stats.json")


@pytest.fixture(scope="module")
def native():
    import _gme_native
    assert "gfx950" in _gme_native.default_context().info()["name"]
    return _gme_native


def synth_frames():
    import synth
    return np.ascontiguousarray(synth.sequence(4711, 0, 259, H0, W0))


def noise_frames():
    return np.random.RandomState(112176).randint(0, 256, size=(259, H0, W0)).astype(np.uint8)


def pan240_frames():
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN_DIR, "g9_pan240seq.npz"))["frames"][:9])


def tie_frames(h, w):
    """constant | constant | vertical split | the split 3 columns on | horizontal split | 5 rows up | vertical split."""
    def halves(split, axis):
        f = np.full((h, w), 60, np.uint8)
        if axis == 1:
            f[:, split:] = 200
        else:
            f[split:, :] = 200
        return f
    return np.stack([np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8), halves(w // 2, 1), halves(w // 2 + 3, 1),
                     halves(h // 2, 0), halves(h // 2 - 5, 0), halves(w // 2, 1)])


def guard_frames(content, h, w, seed):
    if content == "noise":
        return np.random.RandomState(seed).randint(0, 256, size=(4, h, w)).astype(np.uint8)
    f = np.zeros((3, h, w), np.uint8)                       # pair 0: prev 0, cur 255; pair 1 the other way round
    f[1] = 255
    return f


def search(native, monkeypatch, frames, sw, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, frames)
    try:
        seq.bbme(1, 16, sw, 0, 0)
        mv = seq.read_mv()
        info = ctx.last_bbme_info()
    finally:
        seq.close()
    print(frames.shape, "sw", sw, env, info)
    assert "k_exh_sea16" in info["plan"], info["plan"]
    return mv, info


def assert_exact(mv, frames, sw, info):
    want = oracle_fields([(frames[p], frames[p + 1]) for p in range(len(frames) - 1)], sw, 0)
    for p in range(len(frames) - 1):
        assert np.array_equal(mv[p], want[p]), (frames.shape, sw, p, info["plan"])


def tiles_per_workgroup(info, frames):
    """(tiles of the busiest XCD) / (workgroups per XCD), both from the launch plan and the shape."""
    plan = info["plan"]
    grid = int(re.search(r"grid (\d+)", plan).group(1))
    tr, tc = map(int, re.search(r"tiles (\d+)x(\d+)", plan).groups())
    n, h, w = frames.shape
    tiles_per_xcd = -(-(n - 1) // 8) * -(-(h // 16) // tr) * -(-(w // 16) // tc)
    return tiles_per_xcd / (grid / 8)


# ---- ties in the bound ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(48, 80), (112, 176)])
@pytest.mark.parametrize("sw", [16, 8, 24])
def test_ties_in_the_bound(native, monkeypatch, h, w, sw):
    frames = tie_frames(h, w)
    mv, info = search(native, monkeypatch, frames, sw, {})
    assert info["redo_tiles"] == 0, info
    if sw != 16:
        assert "geometry-fixed" not in info["plan"], info["plan"]         # run-time geometry: R = 2 and R = 4
    assert_exact(mv, frames, sw, info)


# ---- every guard form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["noise", "0-255"])
@pytest.mark.parametrize("sw", [4, 12, 20, 16, 32])
@pytest.mark.parametrize("h,w", [(32, 48), (48, 80)])
def test_every_guard_form(native, monkeypatch, h, w, sw, content):
    frames = guard_frames(content, h, w, 7000 + 13 * sw + h)
    mv, info = search(native, monkeypatch, frames, sw, {"GME_SEA_REDO": "0"})
    assert info["redo_tiles"] == 0, info
    assert_exact(mv, frames, sw, info)


@pytest.mark.parametrize("content", ["noise", "0-255", "ties"])
def test_instance_with_horizontal_pairs(native, monkeypatch, content):
    # k_exh_sea16p<5, 16, 0> keeps horizontal pairs (bbme_sea.hip: vertical_pairs); 2x2 tiles of a 32x48 frame launch it
    frames = tie_frames(32, 48) if content == "ties" else guard_frames(content, 32, 48, 7532)
    mv, info = search(native, monkeypatch, frames, 32, {"GME_SEA_REDO": "0", "GME_SEA_PERSIST": "2"})
    assert "k_exh_sea16p<5,16>" in info["plan"], info["plan"]
    assert_exact(mv, frames, 32, info)


# ---- the geometry-fixed instances on their later tiles ---------------------------------------------------------------
@pytest.fixture(scope="module")
def long_cases():
    """258-pair sequences and their oracle fields, computed once."""
    out = {}
    for name, frames in (("noise", noise_frames()), ("synth", synth_frames())):
        out[name] = (frames, np.stack(oracle_fields([(frames[p], frames[p + 1]) for p in range(len(frames) - 1)], 16, 0)))
    return out


@pytest.mark.parametrize("content,redo", [("synth", "1"), ("noise", "1"), ("noise", "0")])
def test_fixed_interior_instance_later_tiles(native, monkeypatch, long_cases, content, redo):
    frames, want = long_cases[content]
    mv, info = search(native, monkeypatch, frames, 16, {"GME_SEA_REDO": redo, "GME_SEA_PERSIST": "2"})
    assert "k_exh_sea16p<3,5>" in info["plan"] and " geometry-fixed" in info["plan"], info["plan"]
    assert tiles_per_workgroup(info, frames) > 1, info["plan"]
    if redo == "0":
        assert info["redo_tiles"] == 0, info
    assert np.array_equal(mv, want)


def test_fixed_r5_instance_later_tiles(native, monkeypatch):
    # 2 x 6 blocks: one 2x6 tile (12 waves) per pair
    pairs = pairs_for(native, 1, 12)
    base, frames = periodic(32, 96, pairs + 1, 532)
    want = np.stack(oracle_fields([(base[k], base[(k + 1) % PERIOD]) for k in range(PERIOD)], 32, 0))
    mv, info = search(native, monkeypatch, frames, 32, {"GME_SEA_PERSIST": "2"})
    assert " geometry-fixed" in info["plan"] and "k_exh_sea16p<5,7>" in info["plan"], info["plan"]
    assert tiles_per_workgroup(info, frames) > 1, info["plan"]
    assert np.array_equal(mv, want[np.arange(pairs) % PERIOD])


# ---- C2 engaged ----------------------------------------------------------------------------------------------------
def test_ordered_evaluation_engaged(native, monkeypatch):
    frames = pan240_frames()
    assert frames.shape == (9, 240, 320)
    mv, info = search(native, monkeypatch, frames, 16, {})
    # listed = phase D's list + what C2 took off it, surviving = the list + what C2 scored itself: they differ only if the
    # ordered evaluation ran (it scores at most the patches it takes off, and prunes with the tighter bound)
    assert info["listed"] > info["surviving"] > 0, info
    assert_exact(mv, frames, 16, info)
    mv0, off = search(native, monkeypatch, frames, 16, {"GME_SEA_QUOTA": "0"})
    assert off["listed"] == off["surviving"] > 0, off
    assert off["listed"] == info["listed"], (off, info)      # what the first upper bounds leave does not depend on C2
    assert np.array_equal(mv0, mv)


# ---- statistics against the parent commit's -------------------------------------------------------------------------
STAT_CASES = {
    # name: (frames, environment beside GME_SEA_PERSIST)
    "synth_112x176_258": (synth_frames, {}),
    "noise_112x176_258": (noise_frames, {}),
    "noise_112x176_258_noredo": (noise_frames, {"GME_SEA_REDO": "0"}),
    "pan240_8": (pan240_frames, {}),
    "pan240_8_quota0": (pan240_frames, {"GME_SEA_QUOTA": "0"}),
}
STAT_MODES = {"one_tile": "0", "static": "1"}               # GME_SEA_PERSIST
# noise with the redo kernel on is compared in the one-tile kernel only: which tiles a persistent workgroup hands over
# depends on its earlier tiles (parent: 1294 tiles one-tile, 1289 static, 1292 - 1293 dynamic)
STAT_RUNS = [(c, m) for c in sorted(STAT_CASES) for m in sorted(STAT_MODES) if (c, m) != ("noise_112x176_258", "static")]


@pytest.mark.parametrize("case,mode", STAT_RUNS)
def test_statistics_equal_the_parents(native, monkeypatch, case, mode):
    recorded = json.load(open(STATS_JSON))["cases"][case][mode]
    make, env = STAT_CASES[case]
    _, info = search(native, monkeypatch, make(), 16, dict(env, GME_SEA_PERSIST=STAT_MODES[mode]))
    assert ("one-tile" in info["plan"]) == (mode == "one_tile") and ("static" in info["plan"]) == (mode == "static"), info["plan"]
    assert {k: info[k] for k in STAT_KEYS} == {k: recorded[k] for k in STAT_KEYS}, (case, mode, info, recorded)
    if "pan240" in case:
        assert (info["listed"] > info["surviving"]) == ("quota0" not in case), info
