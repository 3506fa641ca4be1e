#!/usr/bin/env python3
"""Throughput of the background mosaic and the moving-object masks on one GPU.

* gme_seq_mosaic (k_mosaic_median) over resident synthetic frames under their true integer pan, 720x480 x `--frames` and
  1920x1080 x `--frames-1080`, with the cull and without it: time from a host clock around the blocking call (warm-up, median
  of `--reps`), canvas pixels x frames per second, and nanoseconds per sample actually taken (sum of the counts), to set
  beside k_warp_frames' 0.0104-0.0114 ns per sampled pixel (§7c).
* gme_seq_moving_masks (k_moving_mask) on the same sequences: frames per second.
* the whole ShardedSequence.mosaic at 720x480, split into estimate (projective refinement), host plan, device (mosaic and
  masks) and read-back.
Kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this tool, on its own.  Prints one JSON line.
usage: python tools/mosaic_bench.py [--frames 512] [--frames-1080 128] [--reps 5] [--mosaic-frames 512]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

SYNTH_PAIR = np.array([1, 0, -5, 0, 1, 3, 0, 0], np.float64)      # synth_kernels.hip: frame t shows the canvas at (x - 5 t, y + 3 t)
CANVAS_LIMIT = 1 << 27


def timed(fn, reps):
    fn()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best.append(time.perf_counter() - t0)
    return float(np.median(best))


def kernel_rates(native, H, W, n, reps):
    import mosaic
    seq = native.Sequence(native.default_context(), n, H, W)
    seq.synth(1234, 0)
    pl = mosaic.plan(np.tile(SYNTH_PAIR, (n - 1, 1)), H, W, max_canvas_pixels=CANVAS_LIMIT)
    args = (0, pl["G"], None, pl["ox"], pl["oy"], pl["Hc"], pl["Wc"], 0)
    t_cull = timed(lambda: seq.mosaic(*args, True), reps)
    t_all = timed(lambda: seq.mosaic(*args, False), max(1, reps // 2))
    samples = int(seq.read_mosaic()[1].astype(np.int64).sum())
    t_mask = timed(lambda: seq.moving_masks(0, pl["A"], None, pl["ox"], pl["oy"], 16, 3), reps)
    seq.close()
    cells = float(pl["Hc"]) * pl["Wc"] * n
    return {"shape": [H, W], "frames": n, "canvas": [pl["Hc"], pl["Wc"]], "samples": samples,
            "samples_per_cell": samples / cells, "median_ms": t_cull * 1e3, "median_cells_per_s": cells / t_cull,
            "median_ns_per_sample": t_cull / samples * 1e9, "median_nocull_ms": t_all * 1e3,
            "median_nocull_cells_per_s": cells / t_all, "masks_ms": t_mask * 1e3, "masks_frames_per_s": n / t_mask,
            "masks_ns_per_pixel": t_mask / (n * float(H) * W) * 1e9}


def mosaic_split(native, n, reps):
    import mosaic
    import roadmap
    import sequence
    H, W = 480, 720
    sh = sequence.ShardedSequence(H, W, n, 1)
    sh.synth(1234, 0)
    seq = sh.seq
    parts = {"estimate": [], "host": [], "device": [], "readback": []}
    for _ in range(reps + 1):
        seq.invalidate_pyramids()
        t0 = time.perf_counter()
        h, _ = roadmap.refine_sequence(seq, 1)
        t1 = time.perf_counter()
        p = mosaic.plan(h, H, W, max_canvas_pixels=CANVAS_LIMIT)
        t2 = time.perf_counter()
        use = p["flags"] == 0
        seq.mosaic(0, p["G"], use, p["ox"], p["oy"], p["Hc"], p["Wc"], 0, True)
        seq.moving_masks(0, p["A"], use, p["ox"], p["oy"], 16, 3)
        t3 = time.perf_counter()
        seq.read_mosaic()
        seq.read_masks_range(0, n)
        t4 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            parts[k].append(v)
    sh.close()
    out = {k + "_ms": float(np.median(v[1:])) * 1e3 for k, v in parts.items()}
    out["total_ms"] = sum(out.values())
    out.update(shape=[H, W], frames=n, frames_per_s=n / (out["total_ms"] / 1e3), canvas=[p["Hc"], p["Wc"]],
               unusable=int(p["flags"].sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mosaic-frames", type=int, default=512, help="frames of the whole-mosaic split (0: skip it)")
    args = ap.parse_args()
    import _gme_native as native
    res = {"kernels": [kernel_rates(native, H, W, n, args.reps) for H, W, n in ((480, 720, args.frames), (1080, 1920, args.frames_1080))
                       if n > 1]}
    if args.mosaic_frames:
        res["mosaic_720x480"] = mosaic_split(native, args.mosaic_frames, max(1, args.reps // 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
