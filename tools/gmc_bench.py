#!/usr/bin/env python3
"""Throughput and prediction quality of global motion compensation on one GPU.

Resident synthetic frames (gme_seq_synth), 720x480 x `--frames` and 1920x1080 x `--frames-1080`, blocks of 16, the default
penalty, MAE, frame distance 1, the warps of the direct projective refinement of the same frames (estimated once, outside the
timed calls):
  gmc             Sequence.gmc (the search from every predicted frame and the decision) followed by Sequence.predict_gmc, in
                  pairs per second,
  search          one Sequence.bbme call at the same settings on the same frames (`--procedure`, `--sw`): the search alone,
  compensate_proj one Sequence.compensate_projective call under the same warps: the same per-pixel warp for whole frames.
  predict_gmc, predict_bipred   the two prediction calls alone (the latter on a bidirectional result of the same frames), per pixel.
Every configuration is warmed up once, then `--reps` calls are timed together between gme_timer_start and gme_timer_stop (device
events on the launch stream).  `decide_predict_share` is what of a pair's time is not the search.  Then, on the first `--pairs`
pairs of the g9 golden frames, the mean PSNR of the global-only, the local-only and the chosen prediction and the mean mode
shares.  These figures are recorded, not asserted.  Prints one JSON line.
usage: python tools/gmc_bench.py [--frames 64] [--frames-1080 16] [--reps 3] [--procedure 0] [--sw 16] [--pairs 8]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, PNORM, FD = 16, 0, 1


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def rates(native, gmc, roadmap, H, W, n, reps, procedure, sw):
    ctx = native.default_context()
    seq = native.Sequence(ctx, n, H, W)
    seq.synth(1234, 0)
    pairs, penalty = n - FD, gmc.default_penalty(BS, PNORM)
    h = roadmap.refine_sequence(seq, FD)[0]
    out = {"shape": [H, W], "frames": n, "pairs": pairs, "blocks_per_pair": (H // BS) * (W // BS),
           "usable_warps": int(sum(gmc.usable(w, H, W) for w in h)), "affine_warps": int(np.sum((h[:, 6] == 0) & (h[:, 7] == 0)))}

    def both():
        seq.gmc(FD, h, BS, sw, procedure, PNORM, penalty)
        seq.predict_gmc()
    ms = timed(ctx, lambda: seq.bbme(FD, BS, sw, procedure, PNORM), reps)
    out["search"] = {"ms": ms, "ms_per_pair": ms / pairs, "pairs_per_s": pairs / (ms * 1e-3), "plan": ctx.last_bbme_info()["plan"]}
    ms = timed(ctx, lambda: seq.compensate_projective(FD, h), reps)
    out["compensate_proj"] = {"ms": ms, "ms_per_pair": ms / pairs, "pairs_per_s": pairs / (ms * 1e-3)}
    ms = timed(ctx, both, reps)
    out["gmc"] = {"ms": ms, "ms_per_pair": ms / pairs, "pairs_per_s": pairs / (ms * 1e-3), "plan": ctx.last_bbme_info()["plan"]}
    out["decide_predict_share"] = 1.0 - out["search"]["ms_per_pair"] / out["gmc"]["ms_per_pair"]
    # the two prediction kernels alone, on the same frames: predict_gmc on the result above, predict_bipred on a bidirectional
    # result at bipred_bench.py's settings (N - 2 targets)
    ms = timed(ctx, seq.predict_gmc, reps)
    out["predict_gmc"] = {"ms": ms, "frames": pairs, "ns_per_pixel": ms * 1e6 / (pairs * H * W)}
    seq.bipred(FD, BS, sw, procedure, PNORM, 1, 1, penalty)
    ms = timed(ctx, seq.predict_bipred, reps)
    out["predict_bipred"] = {"ms": ms, "frames": n - 2 * FD, "ns_per_pixel": ms * 1e6 / ((n - 2 * FD) * H * W)}
    out["mode_share"] = [float(np.mean(seq.read_gmc()[1] == m)) for m in range(3)]
    seq.close()
    return out


def quality(native, gmc, roadmap, pairs, procedure, sw):
    g9 = np.ascontiguousarray(np.load(os.path.join(REPO, "tests", "golden", "g9_pan240seq.npz"))["frames"][:pairs + FD])
    H, W = g9.shape[1:]
    penalty = gmc.default_penalty(BS, PNORM)
    seq = native.Sequence.from_frames(native.default_context(), g9)
    h = roadmap.refine_sequence(seq, FD)[0]
    seq.gmc(FD, h, BS, sw, procedure, PNORM, penalty)
    f, mode, cost, costs, usable = seq.read_gmc()
    sse = seq.predict_gmc()
    seq.close()
    rows = []
    for k in range(pairs):
        single = [gmc.sse(g9[k + FD], gmc.predict(g9[k], h[k], gmc.all_mode(costs[k], which), f[k], BS)) for which in (0, 1)]
        rows.append(gmc.summary(mode[k], single[0], single[1], int(sse[k]), H, W))
    out = {"clip": "g9_pan240seq", "shape": [H, W], "pairs": pairs, "penalty": penalty, "usable_warps": int(usable.sum()),
           "mode_share": [float(np.mean([r["mode_share"][m] for r in rows])) for m in range(3)]}
    for name in ("global", "local", "chosen"):
        out["psnr_" + name] = float(np.mean([r["psnr_" + name] for r in rows]))
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
    import gmc
    import roadmap
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "pnorm": PNORM, "frame_distance": FD, "procedure": args.procedure, "sw": args.sw,
                                 "penalty": gmc.default_penalty(BS, PNORM), "reps": args.reps},
                      "sizes": [rates(native, gmc, roadmap, H, W, n, args.reps, args.procedure, args.sw) for H, W, n in sizes if n > FD],
                      "quality": quality(native, gmc, roadmap, args.pairs, args.procedure, args.sw)}))


if __name__ == "__main__":
    main()
