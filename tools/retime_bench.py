#!/usr/bin/env python3
"""Throughput of frame interpolation at any phase beside the halfway interpolation it extends, on one GPU.

Synthetic frames (gme_seq_synth, the frames of tools/interp_bench.py, read back to the host: gme_retime_clip_u8 takes a host
clip), 720x480 x `--frames` and 1920x1080 x `--frames-1080`, blocks of 16, MAE, the tool's default bias.  Per size,
gme_retime_clip_u8 at window 16 over every output of the schedule, at the step 1/2 (one made frame per pair, at phase 1/2) and at
the step 2/5 (24 -> 60 fps: the phases 2/5, 4/5, 1/5 and 3/5), each with
  search    the vectors as the only output: the upload of the clip, k_retime<16> and the read-back of the fields,
  frames    every output: plus k_retime_frame and the read-back of the frames (what retime.convert and retime.slow_motion do);
the call has no form that makes the frames and leaves them on the device, so "with frames made" is `search` plus the launches
of k_retime_frame in the kernel trace,
and beside them gme_seq_interp at window 8 over the pairs (k, k + 1) of the same frames, resident: vectors only, with the frames
made (frame distance 2, where there is a truth and the frames stay on the device) and with the frames read back.  That is the
same +-16 pixels of reach between the two frames, at whole pixels and even displacements only.  Figures are per
made frame.  All of these are blocking calls, so a figure holds the host's wait, the upload and the read-backs as well; the
kernels' own times come from `rocprofv3 --kernel-trace --stats -- python tools/retime_bench.py --reps 1`.  Every configuration is
warmed up once, then `--reps` calls are timed together between gme_timer_start and gme_timer_stop.  `ratio` is the time per made
frame of the retime search over that of the interp search.  These figures are recorded, not asserted.  Prints one JSON line.
usage: python tools/retime_bench.py [--frames 16] [--frames-1080 6] [--reps 3]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, SW, SW_INTERP, PNORM = 16, 16, 8, 0
STEPS = ((1, 2), (2, 5))


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def raw_clip(native, ctx, clip, bias, step, M, outputs):
    """gme_retime_clip_u8 over every output with only the named outputs (buffers made once) -> the call."""
    N, H, W = clip.shape
    h, w = H // BS, W // BS
    bufs = {"frames": (np.zeros((M, H, W), np.uint8), native._c_u8p), "mv": (np.zeros((M, h, w, 2), np.int32), native._c_i32p),
            "cost": (np.zeros((M, h, w), np.int64), native._c_i64p), "dist": (np.zeros((M, h, w), np.int64), native._c_i64p)}
    ptrs = [native._p(*bufs[name]) if name in outputs else None for name in ("frames", "mv", "cost", "dist")]

    def call():
        native._check(ctx.lib.gme_retime_clip_u8(ctx.handle, native._p(clip, native._c_u8p), N, H, W, W, BS, SW, PNORM, bias, step[0],
                                                 step[1], 0, M, *ptrs), ctx.lib)
    return call


def one_size(native, retime, H, W, n, reps):
    ctx = native.default_context()
    seq = native.Sequence(ctx, n, H, W)
    seq.synth(1234, 0)
    clip = np.ascontiguousarray(np.stack([seq.read_frame(k) for k in range(n)]))
    bias = retime.default_bias(BS, PNORM)
    out = {"shape": [H, W], "frames": n, "blocks_per_frame": (H // BS) * (W // BS), "bias": bias}
    for step in STEPS:
        rows = retime.schedule(n, *step)
        M, made = len(rows), int(np.count_nonzero(rows[:, 1]))
        rec = {"outputs": M, "made": made}
        for name, outputs in (("search", ("mv",)), ("frames", ("frames", "mv", "cost", "dist"))):
            ms = timed(ctx, raw_clip(native, ctx, clip, bias, step, M, outputs), reps)
            rec[name] = {"ms": ms, "ms_per_made_frame": ms / made, "made_frames_per_s": made / (ms * 1e-3)}
        rec["plan"] = ctx.last_bbme_info()["plan"]
        out["retime_%d_%d" % step] = rec
    P = n - 1
    i32, i64, u8 = native._c_i32p, native._c_i64p, native._c_u8p
    mv, frames, sse = np.zeros((P, H // BS, W // BS, 2), np.int32), np.zeros((P, H, W), np.uint8), np.zeros(P, np.int64)
    for name, ptrs in (("search", (native._p(mv, i32), None, None, None, None)),
                       ("made", (native._p(mv, i32), None, None, None, native._p(sse, i64))),
                       ("frames", (native._p(mv, i32), None, None, native._p(frames, u8), None))):
        # frame distance 2 for `made`: only an even distance has a truth, and only with a truth are frames made but not read
        fd = 2 if name == "made" else 1
        ms = timed(ctx, lambda: native._check(seq.lib.gme_seq_interp(seq.handle, fd, BS, SW_INTERP, PNORM, bias, 0, n - fd, *ptrs), seq.lib), reps)
        out.setdefault("interp", {})[name] = {"ms": ms, "ms_per_made_frame": ms / (n - fd), "made_frames_per_s": (n - fd) / (ms * 1e-3)}
    out["interp"]["plan"] = ctx.last_bbme_info()["plan"]
    out["ratio"] = {"retime_%d_%d_over_interp_search" % step: out["retime_%d_%d" % step]["search"]["ms_per_made_frame"]
                    / out["interp"]["search"]["ms_per_made_frame"] for step in STEPS}
    seq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import _gme_native as native
    import retime
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "sw": SW, "pnorm": PNORM, "steps": [list(s) for s in STEPS],
                                 "interp": {"sw": SW_INTERP, "frame_distance": 1}, "reps": args.reps},
                      "sizes": [one_size(native, retime, H, W, n, args.reps) for H, W, n in sizes if n > 2]}))


if __name__ == "__main__":
    main()
