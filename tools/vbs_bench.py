#!/usr/bin/env python3
"""Throughput and compensation quality of variable-block-size motion on one GPU.

Resident synthetic frames (gme_seq_synth), 720x480 x `--frames` and 1920x1080 x `--frames-1080`, roots of 16, depth 2, radius 1,
the CLI's default penalty, MAE: pairs per second of
  search        Sequence.bbme at bs 16 (`--procedure`, `--sw`) alone,
  search_tree   the same search followed by Sequence.vbs,
  search_bs4    the same search at bs 4, the fixed-small-block alternative.
Every configuration is warmed up once, then `--reps` calls are timed together between gme_timer_start and gme_timer_stop (device
events on the launch stream).  Then, on the first `--pairs` pairs of the g9 golden frames, the mean PSNR of `current` against
the three compensations: by the root field, by the leaf field and by the bs 4 field.  These figures are recorded, not asserted:
the search is a heuristic.  Prints one JSON line.
usage: python tools/vbs_bench.py [--frames 64] [--frames-1080 16] [--reps 3] [--procedure 0] [--sw 16] [--pairs 8]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, DEPTH, RADIUS, PNORM = 16, 2, 1, 0


def pairs_per_second(ctx, fn, pairs, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    ms = ctx.timer_stop() / reps
    return {"ms": ms, "pairs_per_s": pairs / (ms * 1e-3)}


def rates(native, vbs, H, W, n, reps, procedure, sw):
    ctx = native.default_context()
    seq = native.Sequence(ctx, n, H, W)
    seq.synth(1234, 0)
    pairs, penalty = n - 1, vbs.default_penalty(BS, PNORM)
    out = {"shape": [H, W], "frames": n, "pairs": pairs, "roots_per_pair": (H // BS) * (W // BS)}

    def search_tree():
        seq.bbme(1, BS, sw, procedure, PNORM)
        seq.vbs(1, BS, DEPTH, RADIUS, PNORM, penalty)
    out["search"] = pairs_per_second(ctx, lambda: seq.bbme(1, BS, sw, procedure, PNORM), pairs, reps)
    out["search"]["plan"] = ctx.last_bbme_info()["plan"]
    out["search_tree"] = pairs_per_second(ctx, search_tree, pairs, reps)
    out["search_tree"]["plan"] = ctx.last_bbme_info()["plan"]
    out["search_bs4"] = pairs_per_second(ctx, lambda: seq.bbme(1, BS >> DEPTH, sw, procedure, PNORM), pairs, reps)
    out["search_bs4"]["plan"] = ctx.last_bbme_info()["plan"]
    out["tree_ms"] = out["search_tree"]["ms"] - out["search"]["ms"]
    seq.close()
    return out


def quality(native, vbs, pairs, procedure, sw):
    import sequence
    g9 = np.ascontiguousarray(np.load(os.path.join(REPO, "tests", "golden", "g9_pan240seq.npz"))["frames"][:pairs + 1])
    H, W = g9.shape[1:]
    ctx = native.default_context()
    seq = native.Sequence.from_frames(ctx, g9)
    penalty = vbs.default_penalty(BS, PNORM)

    def field_sse(mv):
        return np.array([ctx.sse(g9[k + 1], ctx.compensate(g9[k], mv[k])) for k in range(pairs)])
    seq.bbme(1, BS >> DEPTH, sw, procedure, PNORM)
    sse_bs4 = field_sse(seq.read_mv())
    seq.bbme(1, BS, sw, procedure, PNORM)
    sse_root = field_sse(seq.read_mv())
    seq.vbs(1, BS, DEPTH, RADIUS, PNORM, penalty)
    depth = seq.read_vbs()[1]
    sse_leaf = seq.compensate_vbs(1, BS)
    seq.close()
    out = {"clip": "g9_pan240seq", "shape": [H, W], "pairs": pairs, "penalty": penalty,
           "split_share": float(np.mean(depth[:, ::1 << DEPTH, ::1 << DEPTH] > 0))}
    for name, sse in (("root", sse_root), ("leaf", sse_leaf), ("bs4", sse_bs4)):
        out["psnr_" + name] = float(np.mean(sequence.psnr_from_sse(np.asarray(sse), H, W)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--procedure", type=int, default=0)
    ap.add_argument("--sw", type=int, default=16)
    ap.add_argument("--pairs", type=int, default=8)
    args = ap.parse_args()
    import _gme_native as native
    import vbs
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "depth": DEPTH, "radius": RADIUS, "pnorm": PNORM, "procedure": args.procedure, "sw": args.sw,
                                 "penalty": vbs.default_penalty(BS, PNORM), "reps": args.reps},
                      "sizes": [rates(native, vbs, H, W, n, args.reps, args.procedure, args.sw) for H, W, n in sizes if n > 1],
                      "quality": quality(native, vbs, args.pairs, args.procedure, args.sw)}))


if __name__ == "__main__":
    main()
