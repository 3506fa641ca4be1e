#!/usr/bin/env python3
"""Throughput of motion-compensated temporal denoising on one GPU.

Resident frames, 720x480 x `--frames` and 1920x1080 x `--frames-1080`, blocks of 16, exhaustive MAE search at window 8, frame
distance 1, default strength, radius 1 and 2, all figures from one run.  Per size three sets of frames:
  pan     frames cut from one smooth canvas (a noise canvas, box-filtered) that moves by (3, 2) pixels per frame, plus Gaussian
          noise of sigma 10: the case the filter is for; its `quality` is the PSNR of the noisy and of the filtered targets
          against the clean ones on the first `--targets` targets,
  synth   the synthetic frames (gme_seq_synth, the frames of tools/obmc_bench.py),
  noise   independent noise frames: nearly every weight is zero, every vector differs from its neighbours.
Per set and radius, over every interior target,
  change   gme_seq_denoise with change_out only, in targets per second,
  frames   gme_seq_denoise with the frames read back as well (what Sequence.denoise does), in targets per second.
A target costs 2 radius searches, overlapped predictions (k_obmc) and one filter launch (k_denoise); the call is blocking, so a
figure holds the host's wait as well.  The kernels' own times per launch, k_denoise beside the k_obmc launches that feed it on the
same planes, come from a kernel trace in a run of its own: `rocprofv3 --kernel-trace --stats -- python tools/denoise_bench.py
--reps 1`.  Every configuration is warmed up once, then `--reps` calls are timed together between gme_timer_start and
gme_timer_stop (device events on the launch stream).  These figures are recorded, not asserted.  Prints one JSON line.
usage: python tools/denoise_bench.py [--frames 64] [--frames-1080 16] [--reps 3] [--targets 4]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, SW, PROCEDURE, PNORM, FD, SIGMA = 16, 8, 0, 0, 1, 10.0
SETS = ("pan", "synth", "noise")
RADII = (1, 2)


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def fill(seq, name, H, W):
    """The frames of one set into the sequence -> the clean frames of the pan set, else None."""
    if name == "synth":
        seq.synth(1234, 0)
        return None
    rng = np.random.default_rng(len(name))
    if name == "noise":
        for k in range(seq.N):
            seq.upload(k, rng.integers(0, 256, size=(1, H, W), dtype=np.uint8))
        return None
    canvas = rng.integers(0, 256, size=(H + 2 * seq.N + 8, W + 3 * seq.N + 8)).astype(np.float64)
    box = np.cumsum(np.cumsum(np.pad(canvas, ((1, 0), (1, 0))), axis=0), axis=1)
    smooth = (box[8:, 8:] - box[:-8, 8:] - box[8:, :-8] + box[:-8, :-8]) / 64.0
    smooth = np.rint((smooth - smooth.min()) / (smooth.max() - smooth.min()) * 255.0)
    clean = np.stack([smooth[2 * k:2 * k + H, 3 * k:3 * k + W] for k in range(seq.N)])
    noisy = np.clip(np.rint(clean + rng.normal(scale=SIGMA, size=clean.shape)), 0, 255).astype(np.uint8)
    seq.upload(0, noisy)
    return clean.astype(np.uint8), noisy


def one_set(native, denoise, seq, name, H, W, reps, targets):
    ctx = native.default_context()
    pan = fill(seq, name, H, W)
    out = {}
    u8, i64 = native._c_u8p, native._c_i64p
    for radius in RADII:
        T = seq.N - 2 * radius * FD
        if T < 1:
            continue
        frames, change = np.zeros((T, H, W), np.uint8), np.zeros(T, np.int64)

        def run(f, c):
            return lambda: native._check(seq.lib.gme_seq_denoise(seq.handle, FD, BS, SW, PROCEDURE, PNORM, radius, 0, denoise.DEFAULT_STRENGTH,
                                                                 0, T, f, c), seq.lib)

        row = {"targets": T}
        for key, fn in (("change", run(None, native._p(change, i64))), ("frames", run(native._p(frames, u8), native._p(change, i64)))):
            ms = timed(ctx, fn, reps)
            row[key] = {"ms": ms, "ms_per_target": ms / T, "targets_per_s": T / (ms * 1e-3)}
        row["mean_change_per_pixel"] = float(change.mean() / (H * W))
        if pan is not None:
            clean, noisy = pan
            n = min(targets, T)
            t = slice(radius * FD, radius * FD + n)
            row["quality"] = {"targets": n, "psnr_noisy": denoise.psnr(denoise.sse(noisy[t], clean[t]), n * H, W),
                              "psnr_filtered": denoise.psnr(denoise.sse(frames[:n], clean[t]), n * H, W)}
        out["radius%d" % radius] = row
    return out


def size(native, denoise, H, W, n, reps, targets):
    seq = native.Sequence(native.default_context(), n, H, W)
    out = {"shape": [H, W], "frames": n}
    for name in SETS:
        out[name] = one_set(native, denoise, seq, name, H, W, reps, targets)
    seq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--targets", type=int, default=4)
    args = ap.parse_args()
    import _gme_native as native
    import denoise
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "search_window": SW, "searching_procedure": PROCEDURE, "pnorm": PNORM, "frame_distance": FD,
                                 "strength": denoise.DEFAULT_STRENGTH, "sigma": SIGMA, "reps": args.reps},
                      "sizes": [size(native, denoise, H, W, n, args.reps, args.targets) for H, W, n in sizes if n > 2 * FD]}))


if __name__ == "__main__":
    main()
