#!/usr/bin/env python3
"""Throughput of motion-compensated frame interpolation beside the existing block searches, on one GPU.

Resident synthetic frames (gme_seq_synth, the frames of tools/prop_bench.py), 720x480 x `--frames` and 1920x1080 x
`--frames-1080`, blocks of 16, window 8, MAE, the tool's default bias, frame distance 2 (frame k + 1 is the truth the frame made
from k and k + 2 is compared with).  Per size, gme_seq_interp over every pair with
  interp_search   the vectors as the only output: k_interp<16> and the read-back of the field,
  interp_sse      the squared errors as well: plus k_interp_frame, the frames staying on the device,
  interp_frames   every output: plus the read-back of the frames (what Sequence.interp and interp.upconvert do),
and beside them, over the pairs (k, k + 1) of the same frames,
  hier            Sequence.hier, three levels, coarse window 8, radius 1 (k_hier<16, 3>),
  exhaustive      Sequence.bbme, procedure 0 at window 16,
each in pairs per second.  `launch` holds the time per launch (one launch carries every pair): k_interp<16> as interp_search,
k_interp_frame as interp_sse minus interp_search, and the two searches as they are; all of these are blocking calls, so a figure
holds the host's wait and the small read-backs as well (`rocprofv3 --kernel-trace --stats -- python tools/interp_bench.py
--reps 1` for the kernels' own times).  Every configuration is warmed up once, then `--reps` calls are timed together between
gme_timer_start and gme_timer_stop (device events on the launch stream).  `quality` is the mean PSNR of the interpolated frames
and of the plain averages against the true middle frames, on the synthetic frames and on g9.  These figures are recorded, not
asserted.  Prints one JSON line.
usage: python tools/interp_bench.py [--frames 64] [--frames-1080 16] [--reps 3] [--pairs 8]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, SW, PNORM, FD = 16, 8, 0, 2


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def raw_interp(native, seq, bias, outputs):
    """gme_seq_interp over every pair with only the named outputs (buffers made once) -> the call."""
    P, h, w = seq.N - FD, seq.H // BS, seq.W // BS
    bufs = {"mv": (np.zeros((P, h, w, 2), np.int32), native._c_i32p), "cost": (np.zeros((P, h, w), np.int64), native._c_i64p),
            "dist": (np.zeros((P, h, w), np.int64), native._c_i64p), "frames": (np.zeros((P, seq.H, seq.W), np.uint8), native._c_u8p),
            "sse": (np.zeros(P, np.int64), native._c_i64p)}
    ptrs = [native._p(*bufs[name]) if name in outputs else None for name in ("mv", "cost", "dist", "frames", "sse")]

    def call():
        native._check(seq.lib.gme_seq_interp(seq.handle, FD, BS, SW, PNORM, bias, 0, P, *ptrs), seq.lib)
    call.bufs = bufs
    return call


def quality(interp, frames, made):
    """Mean PSNR of the interpolated frames and of the plain averages against the true middle frames."""
    H, W = frames.shape[1:]
    ours = [interp.psnr(interp.sse(made[k], frames[k + 1]), H, W) for k in range(len(made))]
    plain = [interp.psnr(interp.sse(interp.average(frames[k], frames[k + 2]), frames[k + 1]), H, W) for k in range(len(made))]
    return {"psnr_interp": float(np.mean(ours)), "psnr_average": float(np.mean(plain))}


def synthetic(native, interp, H, W, n, pairs, reps):
    ctx = native.default_context()
    seq = native.Sequence(ctx, n, H, W)
    seq.synth(1234, 0)
    bias = interp.default_bias(BS, PNORM)
    out = {"shape": [H, W], "frames": n, "pairs": n - FD, "blocks_per_pair": (H // BS) * (W // BS), "bias": bias}
    runs = {"interp_search": raw_interp(native, seq, bias, ("mv",)), "interp_sse": raw_interp(native, seq, bias, ("mv", "sse")),
            "interp_frames": raw_interp(native, seq, bias, ("mv", "cost", "dist", "frames", "sse")),
            "hier": lambda: seq.hier(1, BS, 8, 1, PNORM, 3), "exhaustive": lambda: seq.bbme(1, BS, 16, 0, PNORM)}
    for name, fn in runs.items():
        ms = timed(ctx, fn, reps)
        P = seq.N - (FD if name.startswith("interp") else 1)
        out[name] = {"ms": ms, "ms_per_pair": ms / P, "pairs_per_s": P / (ms * 1e-3), "plan": ctx.last_bbme_info()["plan"]}
    out["launch"] = {"k_interp<16>": out["interp_search"]["ms"], "k_interp_frame": out["interp_sse"]["ms"] - out["interp_search"]["ms"],
                     "k_hier<16,3>": out["hier"]["ms"], "exhaustive_sw16": out["exhaustive"]["ms"]}
    pairs = min(pairs, n - FD)
    frames = np.stack([seq.read_frame(k) for k in range(pairs + FD)])
    out["quality"] = dict(quality(interp, frames, runs["interp_frames"].bufs["frames"][0][:pairs]), pairs=pairs)
    seq.close()
    return out


def golden(native, interp, pairs):
    g9 = np.ascontiguousarray(np.load(os.path.join(REPO, "tests", "golden", "g9_pan240seq.npz"))["frames"][10:10 + pairs + FD])
    seq = native.Sequence.from_frames(native.default_context(), g9)
    made = seq.interp(FD, BS, SW, PNORM, interp.default_bias(BS, PNORM))[3]
    seq.close()
    return dict(quality(interp, g9, made), clip="g9_pan240seq", first_frame=10, shape=list(g9.shape[1:]), pairs=pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=8)
    args = ap.parse_args()
    import _gme_native as native
    import interp
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "sw": SW, "pnorm": PNORM, "frame_distance": FD,
                                 "hier": {"levels": 3, "coarse_window": 8, "radius": 1, "frame_distance": 1},
                                 "exhaustive": {"sw": 16, "frame_distance": 1}, "reps": args.reps},
                      "sizes": [synthetic(native, interp, H, W, n, args.pairs, args.reps) for H, W, n in sizes if n > FD],
                      "quality": golden(native, interp, args.pairs)}))


if __name__ == "__main__":
    main()
