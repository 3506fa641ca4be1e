#!/usr/bin/env python3
"""Throughput and prediction quality of bidirectional block prediction on one GPU.

Resident synthetic frames (gme_seq_synth), 720x480 x `--frames` and 1920x1080 x `--frames-1080`, blocks of 16, radius 1, one
round, the CLI's default penalty, MAE, frame distance 1:
  bipred          Sequence.bipred (both searches from every target and the decision) followed by Sequence.predict_bipred, in
                  targets per second,
  two_searches    two Sequence.bbme calls at the same settings on the same frames (`--procedure`, `--sw`): the searches alone,
                  without decision and prediction.  Each covers N - 1 pairs where bipred's cover N - 2, so the figures beside
                  them are per pair and per target.
Every configuration is warmed up once, then `--reps` calls are timed together between gme_timer_start and gme_timer_stop (device
events on the launch stream).  `decide_predict_share` is what of a target's time is not the two searches.  Then, on the first
`--targets` targets of the g9 golden frames, the mean PSNR of the target against the past-only, the next-only and the chosen
prediction, and the mean mode shares.  These figures are recorded, not asserted.  Prints one JSON line.
usage: python tools/bipred_bench.py [--frames 64] [--frames-1080 16] [--reps 3] [--procedure 0] [--sw 16] [--targets 8]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, RADIUS, ROUNDS, PNORM, FD = 16, 1, 1, 0, 1


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def rates(native, bipred, H, W, n, reps, procedure, sw):
    ctx = native.default_context()
    seq = native.Sequence(ctx, n, H, W)
    seq.synth(1234, 0)
    targets, pairs, penalty = n - 2 * FD, n - FD, bipred.default_penalty(BS, PNORM)
    out = {"shape": [H, W], "frames": n, "targets": targets, "pairs": pairs, "blocks_per_target": (H // BS) * (W // BS)}

    def both():
        seq.bipred(FD, BS, sw, procedure, PNORM, RADIUS, ROUNDS, penalty)
        seq.predict_bipred()

    def searches():
        seq.bbme(FD, BS, sw, procedure, PNORM)
        seq.bbme(FD, BS, sw, procedure, PNORM)
    ms = timed(ctx, searches, reps)
    out["two_searches"] = {"ms": ms, "ms_per_pair": ms / pairs, "pairs_per_s": pairs / (ms * 1e-3), "plan": ctx.last_bbme_info()["plan"]}
    ms = timed(ctx, both, reps)
    out["bipred"] = {"ms": ms, "ms_per_target": ms / targets, "targets_per_s": targets / (ms * 1e-3), "plan": ctx.last_bbme_info()["plan"]}
    out["decide_predict_share"] = 1.0 - out["two_searches"]["ms_per_pair"] / out["bipred"]["ms_per_target"]
    seq.close()
    return out


def quality(native, bipred, targets, procedure, sw):
    g9 = np.ascontiguousarray(np.load(os.path.join(REPO, "tests", "golden", "g9_pan240seq.npz"))["frames"][:targets + 2 * FD])
    H, W = g9.shape[1:]
    penalty = bipred.default_penalty(BS, PNORM)
    seq = native.Sequence.from_frames(native.default_context(), g9)
    seq.bipred(FD, BS, sw, procedure, PNORM, RADIUS, ROUNDS, penalty)
    f0, f1, mode, v0, v1, cost, costs = seq.read_bipred()
    sse = seq.predict_bipred()
    seq.close()
    rows = []
    for k in range(targets):
        single = [bipred.sse(g9[k + FD], bipred.predict(g9[k], g9[k + 2 * FD], bipred.all_mode(f, which, H, W, BS), f0[k], f1[k], BS))
                  for which, f in ((0, f0[k]), (1, f1[k]))]
        rows.append(bipred.summary(mode[k], f0[k], f1[k], v0[k], v1[k], single[0], single[1], int(sse[k]), H, W))
    out = {"clip": "g9_pan240seq", "shape": [H, W], "targets": targets, "penalty": penalty,
           "mode_share": [float(np.mean([r["mode_share"][m] for r in rows])) for m in range(4)],
           "refined_share": float(np.mean([r["refined_share"] for r in rows]))}
    for name in ("past", "next", "chosen"):
        out["psnr_" + name] = float(np.mean([r["psnr_" + name] for r in rows]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--procedure", type=int, default=0)
    ap.add_argument("--sw", type=int, default=16)
    ap.add_argument("--targets", type=int, default=8)
    args = ap.parse_args()
    import _gme_native as native
    import bipred
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "radius": RADIUS, "rounds": ROUNDS, "pnorm": PNORM, "frame_distance": FD,
                                 "procedure": args.procedure, "sw": args.sw, "penalty": bipred.default_penalty(BS, PNORM), "reps": args.reps},
                      "sizes": [rates(native, bipred, H, W, n, args.reps, args.procedure, args.sw) for H, W, n in sizes if n > 2 * FD],
                      "quality": quality(native, bipred, args.targets, args.procedure, args.sw)}))


if __name__ == "__main__":
    main()
