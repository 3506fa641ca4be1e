#!/usr/bin/env python3
"""Where a wave's time goes inside a tile of the persistent elimination kernels: runs a library built
with -DSEA_PHASE_STAMPS (csrc/bbme_sea_common.h: PhaseClock) on the `exh720` shape -- 720x480, blocks of 16, window 16,
exhaustive -- with 256 synthetic pairs and 256 `pan240x2` pairs (640x480), and prints cycles per wave and tile by span, for
the waves that hold the box-sum chunks (0-3 of a 2x4 tile) and the others (4-7) separately, with the share of each that is
barrier wait.  The stamps perturb the kernel (every clock reading waits for the wave's outstanding LDS and scalar loads):
the table attributes time, it does not measure it.  Needs an MI355X.

    bash tools/build_variant.sh stamps -DSEA_PHASE_STAMPS "bbme_sea.hip bbme_sea_mse.hip"
    python tools/sea_phase_stamps.py [--lib stamps] [--pnorm 0] [--pairs 256] [--out profiles/<tag>_phase_stamps.txt]
    python tools/sea_phase_stamps.py [--lib stamps] [--pnorm 0] --verify

--verify: no table; the stamped library searches 258 synthetic pairs of 112x176 (2x4 tiles, ragged on both sides, every workgroup
walks several tiles: the first case of tests/test_gpu_sea_fetch_order.py) under the dynamic and the static schedule, and every
field must equal the C oracle's bit for bit -- the clock readings sit on every path of a tile and must not change a result.
"""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

# (name, slot of the ST_* enum in csrc/bbme_sea_common.h), in the order of a tile
SPANS = [("head (registers -> LDS)", 0), ("head barrier", 1), ("prefetch issue", 2), ("A' box sums", 3), ("A' barrier", 4),
         ("B + C", 5), ("C2", 6), ("D", 7), ("D barrier", 8), ("E work", 9), ("E barriers", 10), ("F + tail", 11)]
WAITS = ("head barrier", "A' barrier", "D barrier", "E barriers")
ST_TILES, ST_SLOTS = 12, 16


def resources(lib_name, plan):
    """VGPRs / spills / scratch of the instance the plan names, from the remarks tools/build_variant.sh kept."""
    path = os.path.join(REPO, "tools", "microbench", "libgme_%s.remarks" % lib_name)
    m = re.match(r"(\w+)<(\d+),(\d+)>.*?( geometry-fixed)?", plan)
    fixed = " geometry-fixed" in plan
    tr, tc = map(int, re.search(r"tiles (\d+)x(\d+)", plan).groups())
    want = "%s<%s, %s, %d>" % (m.group(1), m.group(2), m.group(3), (16 * tr + tc + 0 if fixed else 0))
    if not os.path.exists(path):
        return want + ": no remarks beside the library"
    cur, rows = None, {}
    for line in open(path, errors="replace"):
        f = re.search(r"remark: Function Name: (\S+)", line)
        if f:
            cur = rows.setdefault(f.group(1), {})
            continue
        f = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?): (\d+)", line)
        if f and cur is not None:
            cur[f.group(1).strip()] = int(f.group(2))
    names = list(rows)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    for mangled, name in zip(names, plain):
        if want + "(" in name.replace("(anonymous namespace)::", ""):
            r = rows[mangled]
            return "%s: VGPRs %d, VGPR spills %d, SGPR spills %d, scratch %d B/lane, %d waves/SIMD" % (
                want, r.get("VGPRs", -1), r.get("VGPRs Spill", -1), r.get("SGPRs Spill", -1), r.get("ScratchSize [bytes/lane]", -1),
                r.get("Occupancy [waves/SIMD]", -1))
    return want + ": not in the remarks"


def table(tot, nb):
    """tot: uint64[16][ST_SLOTS] -> lines; cycles per wave and tile of waves 0-3 and of the rest."""
    groups = [("waves 0-3", range(0, min(4, nb))), ("waves 4-%d" % (nb - 1), range(4, nb))]
    lines = ["%-26s %s" % ("span", "".join("%14s %7s" % (g, "share") for g, _ in groups))]
    sums, waits, per = [], [], []
    for _, waves in groups:
        tiles = float(sum(tot[w][ST_TILES] for w in waves)) or 1.0
        per.append([sum(float(tot[w][slot]) for w in waves) / tiles for _, slot in SPANS])
        sums.append(sum(per[-1]))
        waits.append(sum(per[-1][s] for s, (name, _) in enumerate(SPANS) if name in WAITS))
    for s, (name, _) in enumerate(SPANS):
        lines.append("%-26s %s" % (name, "".join("%14.0f %6.1f%%" % (per[g][s], 100.0 * per[g][s] / sums[g]) for g in range(2))))
    lines.append("%-26s %s" % ("tile", "".join("%14.0f %7s" % (sums[g], "") for g in range(2))))
    lines.append("%-26s %s" % ("barrier wait, all four", "".join("%14.0f %6.1f%%" % (waits[g], 100.0 * waits[g] / sums[g]) for g in range(2))))
    ia, ie = [n for n, _ in SPANS].index("A' barrier"), [n for n, _ in SPANS].index("E barriers")
    lines.append("%-26s %s" % ("A' + E barriers", "".join("%14.0f %6.1f%%" % (per[g][ia] + per[g][ie], 100.0 * (per[g][ia] + per[g][ie]) / sums[g])
                                                          for g in range(2))))
    return lines


def verify(native, ctx, lib, pnorm):
    import concurrent.futures
    import synth
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from helpers import c_oracle
    frames = np.ascontiguousarray(synth.sequence(4711, 0, 259, 112, 176))
    co = c_oracle()
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
        want = np.stack(list(pool.map(lambda p: co.bbme(frames[p], frames[p + 1], 16, 16, 0, pnorm), range(258))))
    tot = np.zeros((16, ST_SLOTS), np.uint64)
    for persist in ("2", "1"):
        os.environ["GME_SEA_PERSIST"] = persist
        seq = native.Sequence.from_frames(ctx, frames)
        try:
            seq.bbme(1, 16, 16, 0, pnorm)
            mv = seq.read_mv()
            info = ctx.last_bbme_info()
        finally:
            seq.close()
        assert lib.gme_sea_phase_stamps(pnorm, tot.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1) == 0
        tiles = int(tot[0][ST_TILES])
        print(info["plan"], "tiles counted for wave 0:", tiles)
        assert "persistent" in info["plan"] and "geometry-fixed" in info["plan"] and tiles == 258 * 12, (info, tiles)
        assert np.array_equal(mv, want), "the stamped library's fields differ from the oracle's (GME_SEA_PERSIST=%s)" % persist
    print("stamped library: 258 pairs bit-exact under both schedules")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="stamps", help="tools/microbench/libgme_<lib>.so, built with -DSEA_PHASE_STAMPS")
    ap.add_argument("--pnorm", type=int, default=0, help="0: MAE (k_exh_sea16p), 1: MSE on the vector unit (k_exh_sea16p_mse)")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--verify", action="store_true", help="compare the stamped library's fields with the C oracle instead")
    opt = ap.parse_args()
    if opt.pnorm:
        os.environ["GME_EXH_MFMA"] = "0"

    import _gme_native
    _gme_native.LIB_PATH = os.path.join(REPO, "tools", "microbench", "libgme_%s.so" % opt.lib)
    lib = _gme_native.load_library()
    if not hasattr(lib, "gme_sea_phase_stamps"):
        sys.exit("%s was not built with -DSEA_PHASE_STAMPS" % _gme_native.LIB_PATH)
    lib.gme_sea_phase_stamps.restype = ctypes.c_int
    lib.gme_sea_phase_stamps.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    ctx = _gme_native.default_context()
    if opt.verify:
        return verify(_gme_native, ctx, lib, opt.pnorm)
    from bench import host_content

    out = ["# phase stamps, %s, %s, %d pairs per content, library libgme_%s.so" % (ctx.info()["name"], "MSE" if opt.pnorm else "MAE", opt.pairs, opt.lib),
           "# cycles of the shader clock per wave and tile; every reading costs a wait for the wave's LDS and scalar loads"]
    for content in ("synthetic", "pan240x2"):
        if content == "synthetic":
            seq = _gme_native.Sequence(ctx, opt.pairs + 1, 480, 720)
            seq.synth(1234, 0)
        else:
            frames, _, _ = host_content(content, opt.pairs + 1, 480, 720)
            seq = _gme_native.Sequence.from_frames(ctx, np.ascontiguousarray(frames))
        tot = np.zeros((16, ST_SLOTS), np.uint64)
        buf = tot.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        try:
            seq.bbme(1, 16, 16, 0, opt.pnorm)                # warm-up: code object, buffers
            assert lib.gme_sea_phase_stamps(opt.pnorm, buf, 1) == 0, lib.gme_last_error()
            seq.bbme(1, 16, 16, 0, opt.pnorm)
            assert lib.gme_sea_phase_stamps(opt.pnorm, buf, 1) == 0, lib.gme_last_error()
            info = ctx.last_bbme_info()
        finally:
            seq.close()
        nb = int(np.count_nonzero(tot[:, ST_TILES]))
        out.append("")
        out.append("## %s: %s" % (content, info["plan"]))
        out.append("# surviving %d of %d patches, %d tiles per wave slot counted, %s" % (
            info["surviving"], info["patches"], int(tot[0][ST_TILES]), resources(opt.lib, info["plan"])))
        out += table(tot, nb)
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
