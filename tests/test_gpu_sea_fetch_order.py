"""Elimination search (bbme_sea_common.h: persistent_tiles): where in a tile a wave issues the next tile's prefetch.
Needs an MI355X.

The waves that hold chunks of the box-sum pass (holds_box_chunks) run that pass first and fetch the next tile's number
and window behind its barrier; the others fetch in front of it.  The order cannot change a result: every pair of every
case is compared with the C oracle bit for bit, every case asserts from the launch plan that it ran the instance it is
meant for, and the statistics of the synthetic and noise cases equal what the PARENT commit's library reported.

Cases (who holds chunks follows from shape_of's constants: a 2x4 tile at sw 16 has 28 quads per table row, two chunks per
wave, waves 0 .. 3 of 8; a 2x6 tile at sw 32 has 44, one chunk per wave, waves 0 .. 7 of 12 -- eight, not six):
    walk                  112x176, 258 synthetic pairs, sw 16: the geometry-fixed <3,5> instance, 2x4 tiles, ragged last tile
                          row and column, 396 tiles per XCD for 128 resident workgroups: early and late prefetch on every
                          tile but the last, which has none at either site; dynamic and static schedule
    redo                  the same shape, 258 pairs of uniform noise, redo on: the redo return behind phase D's barrier, and
                          the streak and burst code that replaces `drawn` behind wave 0's (now later) draw; both schedules
    5 pairs               three XCD classes return before their first tile, every walking workgroup has one tile
    C2 engaged            tests/golden/g9_pan240seq.npz (`listed` > `surviving`)
    sw 32                 32x96, the geometry-fixed <5,7> instance (2x6 tiles), three tiles per workgroup
    run-time geometry     32x96 at sw 8 (2x2 tiles, waves 0 and 1 of 4 hold chunks); one block row, so
                          tr == 1 and 1x8 tiles whose eight waves all hold chunks: 16x128 at sw 8 (MAE <2,6>) and at sw 16
                          under MSE (<3,6>).  MAE at sw 16 on that frame runs <3,6,0>: the run-time-geometry instances of
                          R = 3 keep every wave's prefetch in front of the pass (bbme_sea.hip: late_prefetch); that case pins
                          the form without the order
    static content        equal frames, and flat ones: the previous vector equals the zero vector
    MSE                   on the vector unit (GME_EXH_MFMA=0), walk and redo, at sw 16 (112x176) and sw 32 (32x96)
    statistics            patches / surviving / listed / redo_tiles of the synthetic and noise cases in the one-tile kernel and
                          under the static schedule equal tests/golden/sea_fetch_order_stats.json, recorded on an MI355X from
                          the parent commit's library before the change (never recomputed from the code under test); shared
                          inputs agree with sea_priority_stats.json.  Under the dynamic schedule the third probe depends on
                          the tile order: those runs are checked against the oracle only.
    stamped build         the first case with a library built with -DSEA_PHASE_STAMPS, in a process of its own (tools/
                          sea_phase_stamps.py --verify): plan, tiles counted by the clock code, fields against the oracle, both
                          schedules.  tools/microbench/libgme_stamps.so is used when it is newer than the three sources, else
                          built once (tools/build_variant.sh: two files, or all of them where the tree's objects are missing)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import GOLDEN_DIR
from test_gpu_sea_persistent_walk import PERIOD, assert_walks, oracle_fields, pairs_for, search

pytestmark = pytest.mark.gpu

H0, W0 = 112, 176
STAT_KEYS = ("patches", "surviving", "listed", "redo_tiles")
STATS_JSON = os.path.join(GOLDEN_DIR, "sea_fetch_order_stats.json")


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


@pytest.fixture(scope="module")
def big():
    """(content, pnorm) -> (frames, oracle fields at sw 16) of the 258-pair sequences, each computed once."""
    frames, fields = {}, {}
    makers = {"synth": synth_frames, "noise": noise_frames}

    def get(content, pnorm=0):
        if content not in frames:
            frames[content] = makers[content]()
        if (content, pnorm) not in fields:
            f = frames[content]
            fields[(content, pnorm)] = np.stack(oracle_fields([(f[p], f[p + 1]) for p in range(len(f) - 1)], 16, pnorm))
        return frames[content], fields[(content, pnorm)]
    return get


def periodic_of(base, count):
    return np.ascontiguousarray(base[np.arange(count) % PERIOD])


def periodic_base(kind, h, w, seed):
    if kind == "noise":
        return np.random.RandomState(seed).randint(0, 256, size=(PERIOD, h, w)).astype(np.uint8)
    import synth
    return np.ascontiguousarray(synth.sequence(seed, 0, PERIOD, h, w))


def check_periodic(native, monkeypatch, kind, h, w, sw, pnorm, tiles_per_pair, waves, seed, env, plan_has, plan_lacks=()):
    """`kind` frames of period 17, as many pairs as give every workgroup three tiles, against the oracle's 17 fields."""
    base = periodic_base(kind, h, w, seed)
    pairs = pairs_for(native, tiles_per_pair, waves)
    frames = periodic_of(base, pairs + 1)
    want = np.stack(oracle_fields([(base[k], base[(k + 1) % PERIOD]) for k in range(PERIOD)], sw, pnorm))
    mv, info = search(native, monkeypatch, frames, sw, pnorm, env)
    for s in plan_has:
        assert s in info["plan"], info["plan"]
    for s in plan_lacks:
        assert s not in info["plan"], info["plan"]
    assert assert_walks(info, frames) == tiles_per_pair
    assert np.array_equal(mv, want[np.arange(pairs) % PERIOD])
    return info


FIXED3 = ("k_exh_sea16p<3,5>", "tiles 2x4", " geometry-fixed")
SCHEDULE = {"2": "persistent-dynamic", "1": "persistent-static"}


# ---- walk: early and late prefetch on every tile but a workgroup's last ----------------------------------------------
@pytest.mark.parametrize("persist", ["2", "1"])
def test_walk(native, monkeypatch, big, persist):
    frames, want = big("synth")
    mv, info = search(native, monkeypatch, frames, 16, 0, {"GME_SEA_PERSIST": persist})
    for s in FIXED3 + (SCHEDULE[persist],):
        assert s in info["plan"], info["plan"]
    assert assert_walks(info, frames) == 12
    assert info["redo_tiles"] == 0, info
    assert np.array_equal(mv, want)


# ---- redo return, streaks and bursts behind wave 0's draw ------------------------------------------------------------
@pytest.mark.parametrize("persist", ["2", "1"])
def test_redo(native, monkeypatch, big, persist):
    frames, want = big("noise")
    mv, info = search(native, monkeypatch, frames, 16, 0, {"GME_SEA_PERSIST": persist})
    for s in FIXED3 + (SCHEDULE[persist],):
        assert s in info["plan"], info["plan"]
    tiles = 12 * (len(frames) - 1)
    assert assert_walks(info, frames) == 12
    assert 0 < info["redo_tiles"] < tiles, (info, tiles)
    assert np.array_equal(mv, want)


# ---- 5 pairs: XCD classes without tiles, one tile per walking workgroup ----------------------------------------------
def test_five_pairs(native, monkeypatch, big):
    frames, want = big("synth")
    mv, info = search(native, monkeypatch, frames[:6], 16, 0, {"GME_SEA_PERSIST": "2"})
    for s in FIXED3 + (SCHEDULE["2"], "grid 96 "):          # 5 pairs x 12 tiles: 60 tiles for 96 workgroups (8 classes x 12)
        assert s in info["plan"], info["plan"]
    assert np.array_equal(mv, want[:5])


# ---- C2 engaged ------------------------------------------------------------------------------------------------------
def test_ordered_evaluation_engaged(native, monkeypatch):
    frames = np.ascontiguousarray(np.load(os.path.join(GOLDEN_DIR, "g9_pan240seq.npz"))["frames"][:9])
    assert frames.shape == (9, 240, 320)
    want = np.stack(oracle_fields([(frames[p], frames[p + 1]) for p in range(8)], 16, 0))
    mv, info = search(native, monkeypatch, frames, 16, 0, {"GME_SEA_PERSIST": "2"})
    for s in FIXED3:
        assert s in info["plan"], info["plan"]
    assert info["listed"] > info["surviving"] > 0, info
    assert np.array_equal(mv, want)


# ---- sw 32: the geometry-fixed <5,7> instance ------------------------------------------------------------------------
def test_fixed_r5(native, monkeypatch):
    check_periodic(native, monkeypatch, "synth", 32, 96, 32, 0, 1, 12, 532, {"GME_SEA_PERSIST": "2"},
                   ("k_exh_sea16p<5,7>", "tiles 2x6", " geometry-fixed"))


# ---- run-time geometry -----------------------------------------------------------------------------------------------
def test_runtime_geometry_sw8(native, monkeypatch):
    check_periodic(native, monkeypatch, "synth", 32, 96, 8, 0, 3, 4, 508, {"GME_SEA_PERSIST": "2"},
                   ("k_exh_sea16p<2,", "tiles 2x2"), ("geometry-fixed",))


@pytest.mark.parametrize("sw,pnorm,kernel", [(8, 0, "k_exh_sea16p<2,6>"), (16, 1, "k_exh_sea16p_mse<3,6>"), (16, 0, "k_exh_sea16p<3,6>")])
def test_runtime_geometry_one_block_row(native, monkeypatch, sw, pnorm, kernel):
    check_periodic(native, monkeypatch, "synth", 16, 128, sw, pnorm, 1, 8, 516, {"GME_SEA_PERSIST": "2"},
                   (kernel, "tiles 1x8"), ("geometry-fixed",))


# ---- static content: the previous vector equals the zero vector ------------------------------------------------------
@pytest.mark.parametrize("content", ["equal", "flat"])
def test_static_content(native, monkeypatch, big, content):
    if content == "equal":
        one = big("synth")[0][3]
    else:
        one = np.full((H0, W0), 128, np.uint8)
    frames = np.ascontiguousarray(np.repeat(one[None], 259, axis=0))
    want = oracle_fields([(one, one)], 16, 0)[0]              # equal: SAD 0 at the zero vector; flat: every cost ties, the first candidate wins
    for persist in ("2", "1"):
        mv, info = search(native, monkeypatch, frames, 16, 0, {"GME_SEA_PERSIST": persist})
        for s in FIXED3 + (SCHEDULE[persist],):
            assert s in info["plan"], info["plan"]
        assert_walks(info, frames)
        assert np.array_equal(mv, np.broadcast_to(want, mv.shape))


# ---- MSE on the vector unit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("persist", ["2", "1"])
@pytest.mark.parametrize("content", ["synth", "noise"])
def test_mse_sw16(native, monkeypatch, big, content, persist):
    frames, want = big(content, 1)
    mv, info = search(native, monkeypatch, frames, 16, 1, {"GME_SEA_PERSIST": persist})
    for s in ("k_exh_sea16p_mse<3,5>", "tiles 2x4", " geometry-fixed", SCHEDULE[persist]):
        assert s in info["plan"], info["plan"]
    assert assert_walks(info, frames) == 12
    assert (info["redo_tiles"] > 0) == (content == "noise"), info
    assert np.array_equal(mv, want)


@pytest.mark.parametrize("persist", ["2", "1"])
@pytest.mark.parametrize("content", ["synth", "noise"])
def test_mse_sw32(native, monkeypatch, content, persist):
    # (no claim about redo_tiles here: a frame two block rows high leaves most of a 80x80 window outside the frame)
    check_periodic(native, monkeypatch, content, 32, 96, 32, 1, 1, 12, 532, {"GME_SEA_PERSIST": persist},
                   ("k_exh_sea16p_mse<5,7>", "tiles 2x6", " geometry-fixed", SCHEDULE[persist]))


# ---- the stamped build -------------------------------------------------------------------------------------------------
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "global-motion-estimation_amd", "csrc")
STAMPED = ("bbme_sea.hip", "bbme_sea_mse.hip")


@pytest.fixture(scope="module")
def stamped_library():
    lib = os.path.join(REPO, "tools", "microbench", "libgme_stamps.so")
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in STAMPED + ("bbme_sea_common.h",))
    if not os.path.exists(lib) or os.path.getmtime(lib) < newest:
        srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))       # as the Makefile's wildcard
        have_objects = all(os.path.exists(os.path.join(CSRC, "build", f[:-4] + ".o")) for f in srcs)
        cmd = ["bash", os.path.join(REPO, "tools", "build_variant.sh"), "stamps", "-DSEA_PHASE_STAMPS"] + ([" ".join(STAMPED)] if have_objects else [])
        subprocess.run(cmd, check=True, cwd=REPO, stdout=subprocess.DEVNULL)
    return lib


@pytest.mark.parametrize("pnorm", [0, 1])
def test_stamped_build(native, stamped_library, pnorm):
    # a second library of the same C ABI cannot share this process with the tree's: a process of its own
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "sea_phase_stamps.py"), "--lib", "stamps", "--pnorm", str(pnorm), "--verify"],
                       cwd=REPO, capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "bit-exact under both schedules" in r.stdout and "persistent-dynamic" in r.stdout and "persistent-static" in r.stdout, r.stdout


# ---- statistics against the parent commit's --------------------------------------------------------------------------
STAT_CASES = {
    # name: (content, pairs, pnorm)
    "synth_112x176_258": ("synth", 258, 0),
    "noise_112x176_258": ("noise", 258, 0),
    "synth_112x176_5": ("synth", 5, 0),
    "mse_synth_112x176_258": ("synth", 258, 1),
    "mse_noise_112x176_258": ("noise", 258, 1),
}
STAT_MODES = {"one_tile": "0", "static": "1"}               # GME_SEA_PERSIST
STAT_RUNS = [(c, m) for c in sorted(STAT_CASES) for m in sorted(STAT_MODES)]


@pytest.mark.parametrize("case,mode", STAT_RUNS)
def test_statistics_equal_the_parents(native, monkeypatch, big, case, mode):
    recorded = json.load(open(STATS_JSON))["cases"][case][mode]
    content, pairs, pnorm = STAT_CASES[case]
    frames, want = big(content, pnorm)
    mv, info = search(native, monkeypatch, frames[:pairs + 1], 16, pnorm, {"GME_SEA_PERSIST": STAT_MODES[mode]})
    assert ("one-tile" in info["plan"]) == (mode == "one_tile") and ("static" in info["plan"]) == (mode == "static"), info["plan"]
    assert ("_mse" in info["plan"]) == bool(pnorm), info["plan"]
    assert {k: info[k] for k in STAT_KEYS} == {k: recorded[k] for k in STAT_KEYS}, (case, mode, info, recorded)
    assert np.array_equal(mv, want[:pairs])


def test_recorded_statistics_agree_with_the_earlier_file():
    mine = json.load(open(STATS_JSON))["cases"]
    theirs = json.load(open(os.path.join(GOLDEN_DIR, "sea_priority_stats.json")))["cases"]
    shared = 0
    for case in mine:
        for mode in mine[case]:
            if case in theirs and mode in theirs[case]:
                shared += 1
                assert {k: mine[case][mode][k] for k in STAT_KEYS} == {k: theirs[case][mode][k] for k in STAT_KEYS}, (case, mode)
    assert shared == 4                                        # noise_112x176_258 and synth_112x176_5, both modes
