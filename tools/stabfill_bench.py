#!/usr/bin/env python3
"""Cost of filling the stabilizer's border from neighbour frames on one GPU, against k_warp_frames.

`--frames` resident synthetic frames at 720x480 and 1920x1080 under random jitter corrections W_t = J_t at crop 0 (a few
pixels of shift, ~0.3 % zoom, ~0.2 degrees: stabilize_bench.py's, without its 5 % crop).  With a still smoothed path the
neighbour s of any frame sees the output at J_s, so the candidates of frame t are (t, J_t), (t-1, J_{t-1}), (t+1, J_{t+1}), ...
In one run, with a host clock around blocking calls (median of `--reps`):
  warp_frames   gme_seq_warp_frames (the yardstick: the same warps, output kept in the sequence)
  fill1 / fill5 gme_seq_warp_fill with 1 and 5 candidates and every output pointer NULL but the counts: the allocation of
                the call's own planes, their memset and the kernel
  fill5_frames  the same with the frames read back (what Sequence.warp_fill does)
Per-launch kernel times come from a `rocprofv3 --kernel-trace --stats` run of this tool with --no-readback.
Prints one JSON line.
usage: python tools/stabfill_bench.py [--frames 512] [--reps 5] [--no-readback]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO, os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402

from stabilize_bench import timed  # noqa: E402


def jitter(rng, n, H, W):
    import stabilize
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    Tc = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
    out = np.empty((n, 8))
    for t in range(n):
        th = np.deg2rad(rng.normal(scale=0.2))
        z = 1.0 + rng.normal(scale=0.003)
        R = np.array([[z * np.cos(th), -z * np.sin(th), 0], [z * np.sin(th), z * np.cos(th), 0], [0, 0, 1.0]])
        T = np.array([[1, 0, rng.normal(scale=2.0)], [0, 1, rng.normal(scale=2.0)], [0, 0, 1.0]])
        out[t] = stabilize.params(T @ Tc @ R @ np.linalg.inv(Tc))
    return out


def candidates(J, K):
    n = len(J)
    sources = np.full((n, 2 * K + 1), -1, np.int32)
    warps = np.zeros((n, 2 * K + 1, 8))
    for t in range(n):
        for j in range(2 * K + 1):
            s = t if j == 0 else (t - (j + 1) // 2 if j % 2 else t + j // 2)
            if 0 <= s < n:
                sources[t, j], warps[t, j] = s, J[s]
    return sources, warps


def rates(native, H, W, n, reps, rng, readback):
    seq = native.Sequence(native.default_context(), n, H, W)
    seq.synth(1234, 0)
    J = jitter(rng, n, H, W)
    px = float(H) * W * n
    out = {"shape": [H, W], "frames": n}
    t = timed(lambda: seq.warp_frames(0, J, 0, 0), reps)
    out.update(warp_frames_ms=t * 1e3, warp_frames_ns_per_pixel=t / px * 1e9)
    frames = np.empty((n, H, W), np.uint8) if readback else None
    valid, filled = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for K in (0, 2):
        sources, warps = candidates(J, K)
        head = (seq.handle, 0, n, 2 * K + 1, native._p(sources, native._c_i32p), native._p(warps, native._c_f64p), 0, 0)
        tail = (None, native._p(valid, native._c_i64p), native._p(filled, native._c_i64p), None)

        def call(out_frames=None):
            native._check(seq.lib.gme_seq_warp_fill(*head, out_frames, *tail), seq.lib)
        t = timed(call, reps)
        key = "fill%d" % (2 * K + 1)
        out.update({key + "_ms": t * 1e3, key + "_ns_per_pixel": t / px * 1e9, key + "_valid": int(valid.sum()),
                    key + "_filled": int(filled.sum())})
        if K:
            out[key + "_unfilled"] = int(px) - int(valid.sum()) - int(filled.sum())
            if filled.sum():
                out[key + "_extra_ns_per_filled_pixel"] = (t * 1e3 - out["fill1_ms"]) * 1e6 / float(filled.sum())
            if readback:
                t = timed(lambda: call(native._p(frames, native._c_u8p)), max(1, reps // 2))
                out.update({key + "_frames_ms": t * 1e3})
    seq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-readback", action="store_true", help="leave out the calls that read the frames back")
    args = ap.parse_args()
    import _gme_native as native
    rng = np.random.default_rng(7)
    print(json.dumps({"fill": [rates(native, H, W, args.frames, args.reps, rng, not args.no_readback)
                               for H, W in ((480, 720), (1080, 1920))]}))


if __name__ == "__main__":
    main()
