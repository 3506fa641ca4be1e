#!/usr/bin/env python3
"""Throughput of the hierarchical block search on one GPU.

Resident frames, 720x480 x `--frames` and 1920x1080 x `--frames-1080`, synthetic (gme_seq_synth) and noise: pairs per second of
Sequence.hier at bs 16, cw 8, r 1, levels 3 under both norms, and in the same process, on the same frames, of Sequence.bbme
exhaustive at sw 32 and diamond at sw 32 (bs 16).  Every call is warmed up once, then `--reps` calls are timed together between
gme_timer_start and gme_timer_stop (device events on the launch stream).  The pyramids are built before the window opens: a
resident sequence builds them once, whatever is searched afterwards.  `--only hier` times the hierarchical search alone: the
form to run under `rocprofv3 --kernel-trace --stats` for the kernel's own time,

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/hier_bench.py --only hier

Prints one JSON line.
usage: python tools/hier_bench.py [--frames 256] [--frames-1080 64] [--reps 5] [--only hier]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, CW, RADIUS, LEVELS, SW = 16, 8, 1, 3, 32


def pairs_per_second(ctx, fn, pairs, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    ms = ctx.timer_stop() / reps
    return {"ms": ms, "pairs_per_s": pairs / (ms * 1e-3)}


def rates(native, H, W, n, reps, content, only_hier):
    ctx = native.default_context()
    seq = native.Sequence(ctx, n, H, W)
    if content == "synth":
        seq.synth(1234, 0)
    else:
        rng = np.random.default_rng(5)
        seq.upload(0, rng.integers(0, 256, size=(n, H, W), dtype=np.uint8))
    pairs = n - 1
    out = {"shape": [H, W], "content": content, "frames": n, "pairs": pairs, "blocks_per_pair": (H // BS) * (W // BS)}
    for pnorm, norm in ((0, "mae"), (1, "mse")):
        row = {"hier": pairs_per_second(ctx, lambda: seq.hier(1, BS, CW, RADIUS, pnorm, LEVELS), pairs, reps)}
        row["hier"]["plan"] = ctx.last_bbme_info()["plan"]
        if not only_hier:
            row["exhaustive_sw32"] = pairs_per_second(ctx, lambda: seq.bbme(1, BS, SW, 0, pnorm), pairs, reps)
            row["diamond_sw32"] = pairs_per_second(ctx, lambda: seq.bbme(1, BS, SW, 3, pnorm), pairs, reps)
            row["hier_over_exhaustive"] = row["hier"]["pairs_per_s"] / row["exhaustive_sw32"]["pairs_per_s"]
            row["hier_over_diamond"] = row["hier"]["pairs_per_s"] / row["diamond_sw32"]["pairs_per_s"]
        out[norm] = row
    seq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("hier",), default=None)
    args = ap.parse_args()
    import _gme_native as native
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "cw": CW, "radius": RADIUS, "levels": LEVELS, "sw": SW, "reps": args.reps},
                      "sizes": [rates(native, H, W, n, args.reps, content, args.only == "hier")
                                for H, W, n in sizes if n > 1 for content in ("synth", "noise")]}))


if __name__ == "__main__":
    main()
