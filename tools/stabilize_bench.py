#!/usr/bin/env python3
"""Throughput of the video stabilizer on one GPU.

* gme_seq_warp_frames alone over `--frames` resident synthetic frames at 720x480 and 1920x1080, random jitter warps (a
  few pixels of shift, ~0.3 % zoom, ~0.2 degrees, 5 % crop): frames/s from a host clock around calls that end in a device
  synchronise, and the effective bandwidth (H*W bytes read + H*W written per frame) against the 6.3 TB/s copy rate.
* gme_seq_compensate_projective (k_compensate_proj, one pixel per thread) under the same warps, as the per-pixel
  baseline: the host clock here; the kernel time itself comes from a `rocprofv3 --kernel-trace --stats` run of this tool.
* the whole ShardedSequence.stabilize at 720x480, split into estimate (projective refinement), host trajectory / crop /
  corrections, warp (+ the two consecutive-frame squared-error passes) and readback.
Prints one JSON line.
usage: python tools/stabilize_bench.py [--frames 512] [--reps 5] [--stabilize-frames 512]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

COPY_TBPS = 6.3


def jitter_warps(rng, n, H, W):
    import stabilize
    Z = stabilize.zoom(0.05, H, W)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    out = np.empty((n, 8))
    for t in range(n):
        th = np.deg2rad(rng.normal(scale=0.2))
        z = 1.0 + rng.normal(scale=0.003)
        R = np.array([[z * np.cos(th), -z * np.sin(th), 0], [z * np.sin(th), z * np.cos(th), 0], [0, 0, 1.0]])
        Tc = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
        T = np.array([[1, 0, rng.normal(scale=2.0)], [0, 1, rng.normal(scale=2.0)], [0, 0, 1.0]])
        out[t] = stabilize.params(T @ Tc @ R @ np.linalg.inv(Tc) @ Z)
    return out


def timed(fn, reps):
    fn()
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best.append(time.perf_counter() - t0)
    return float(np.median(best))


def warp_rates(native, H, W, n, reps, rng):
    seq = native.Sequence(native.default_context(), n, H, W)
    seq.synth(1234, 0)
    warps = jitter_warps(rng, n, H, W)
    t_warp = timed(lambda: seq.warp_frames(0, warps, 0, 0), reps)
    t_comp = timed(lambda: seq.compensate_projective(1, warps[:n - 1]), reps)
    seq.close()
    px = float(H) * W
    return {"shape": [H, W], "frames": n, "warp_ms": t_warp * 1e3, "warp_frames_per_s": n / t_warp,
            "warp_ns_per_pixel": t_warp / (n * px) * 1e9, "warp_tb_per_s": 2 * px * n / t_warp / 1e12,
            "warp_fraction_of_copy": 2 * px * n / t_warp / 1e12 / COPY_TBPS,
            "compensate_proj_ms": t_comp * 1e3, "compensate_proj_ns_per_pixel": t_comp / ((n - 1) * px) * 1e9}


def stabilize_split(native, n, reps):
    import roadmap
    import sequence
    import stabilize
    H, W = 480, 720
    sh = sequence.ShardedSequence(H, W, n, 1)
    sh.synth(1234, 0)
    seq = sh.seq
    parts = {"estimate": [], "host": [], "warp": [], "readback": []}
    for _ in range(reps + 1):
        seq.invalidate_pyramids()
        t0 = time.perf_counter()
        h, _ = roadmap.refine_sequence(seq, 1)
        t1 = time.perf_counter()
        p = stabilize.plan(h, H, W)
        t2 = time.perf_counter()
        seq.warp_frames(0, p["W"], 0, 0)
        seq.frame_sse(0, 0, n - 1)
        seq.frame_sse(1, 0, n - 1)
        t3 = time.perf_counter()
        seq.read_warped_range(0, n)
        t4 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            parts[k].append(v)
    sh.close()
    out = {k + "_ms": float(np.median(v[1:])) * 1e3 for k, v in parts.items()}
    out["total_ms"] = sum(out.values())
    out.update(shape=[H, W], frames=n, frames_per_s=n / (out["total_ms"] / 1e3), crop=p["crop"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stabilize-frames", type=int, default=512, help="frames of the whole-stabilize split (0: skip it)")
    args = ap.parse_args()
    import _gme_native as native
    rng = np.random.default_rng(7)
    res = {"warp": [warp_rates(native, H, W, args.frames, args.reps, rng) for H, W in ((480, 720), (1080, 1920))]}
    if args.stabilize_frames:
        res["stabilize_720x480"] = stabilize_split(native, args.stabilize_frames, max(1, args.reps // 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
