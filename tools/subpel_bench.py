#!/usr/bin/env python3
"""Throughput of the quarter-pel refinement and compensation on one GPU.

Resident synthetic frames, 720x480 x `--frames` and 1920x1080 x `--frames-1080`, block size 16, both norms: time of
gme_seq_subpel (k_subpel_refine) and of gme_seq_compensate_qpel (k_compensate_qpel) from a host clock around the blocking
call (warm-up, median of `--reps`), beside the integer search they follow (diamond, and exhaustive at sw 16; gme_seq_bbme plus
a sync).  Refinement in ns per block-candidate (17 per block), compensation in ns per pixel, to set beside k_warp_frames'
0.0104-0.0114 ns per pixel (§7c), and what the refinement adds on top of each search.
Kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this tool, on its own.  Prints one JSON line.
usage: python tools/subpel_bench.py [--frames 512] [--frames-1080 128] [--reps 5]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, SW = 16, 16


def timed(fn, reps):
    fn()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best.append(time.perf_counter() - t0)
    return float(np.median(best))


def rates(native, H, W, n, reps):
    ctx = native.default_context()
    seq = native.Sequence(ctx, n, H, W)
    seq.synth(1234, 0)
    pairs, blocks = n - 1, (H // BS) * (W // BS)
    out = {"shape": [H, W], "frames": n, "pairs": pairs, "blocks_per_pair": blocks}
    for pnorm, norm in ((0, "mae"), (1, "mse")):
        def search(procedure):
            seq.bbme(1, BS, SW, procedure, pnorm)
            ctx.sync()
        t_exh = timed(lambda: search(0), reps)
        t_dia = timed(lambda: search(3), reps)                   # the field the refinement below starts from
        t_ref = timed(lambda: seq.subpel(1, BS, pnorm, 2), reps)
        t_half = timed(lambda: seq.subpel(1, BS, pnorm, 1), reps)
        seq.subpel(1, BS, pnorm, 2)
        q, _ = seq.read_qmv()
        mf = seq.read_mv()
        t_comp = timed(lambda: seq.compensate_qpel(1, BS), reps)
        out[norm] = {"diamond_ms": t_dia * 1e3, "exhaustive_ms": t_exh * 1e3, "subpel_ms": t_ref * 1e3,
                     "subpel_half_only_ms": t_half * 1e3, "compensate_ms": t_comp * 1e3,
                     "subpel_ns_per_block_candidate": t_ref / (pairs * blocks * 17.0) * 1e9,
                     "compensate_ns_per_pixel": t_comp / (pairs * float(H) * W) * 1e9,
                     "subpel_over_diamond": t_ref / t_dia, "subpel_over_exhaustive": t_ref / t_exh,
                     "moved_share": float(np.mean(np.any(q != 4 * mf, axis=3)))}
    seq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import _gme_native as native
    print(json.dumps({"sizes": [rates(native, H, W, n, args.reps) for H, W, n in ((480, 720, args.frames), (1080, 1920, args.frames_1080))
                                if n > 1]}))


if __name__ == "__main__":
    main()
