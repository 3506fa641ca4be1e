#!/usr/bin/env python3
"""Throughput of the direct projective refinement beside the existing GME flow, on one GPU.

ShardedSequence.estimate_projective (indirect affine estimate + refinement + compensation) and
ShardedSequence.estimate_and_compensate (the indirect affine flow alone) over `--pairs` pairs of the 720x480 synthetic
sequence, default caps (outlier fraction 0.1, max_iters 10); pairs/s from a host clock around calls that end in a device
synchronise.  Also: the mean Gauss-Newton steps per level of a sample of pairs (host definition direct.refine on the
device's pyramids, which the device refinement follows step for step), and the pixel passes they imply.
usage: python tools/projective_bench.py [--pairs 512] [--reps 3] [--sample 4]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=4, help="pairs whose iterations the host definition counts (0: none)")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=720)
    args = ap.parse_args()
    import direct
    import motion
    import roadmap
    from sequence import ShardedSequence
    H, W, P = args.height, args.width, args.pairs
    sh = ShardedSequence(H, W, P + 1, 1)
    sh.synth(1234, 0)
    out = {"pairs": P, "shape": [H, W], "reps": args.reps}

    def timed(fn):
        fn()                                                   # warm-up: code objects, buffers, pyramids
        ts = []
        for _ in range(args.reps):
            sh.invalidate()                                    # every timed call pays for its pyramids
            t0 = time.perf_counter()
            r = fn()
            sh.sync()
            ts.append(time.perf_counter() - t0)
        return r, ts

    (h, flags, psnr), ts = timed(lambda: sh.estimate_projective())
    out["estimate_projective"] = {"pairs_per_s": P / min(ts), "seconds": ts, "flags": np.bincount(flags, minlength=32).tolist(),
                                  "median_psnr": float(np.median(psnr))}
    (p6, psnr6), ts6 = timed(lambda: sh.estimate_and_compensate())
    out["estimate_and_compensate_affine"] = {"pairs_per_s": P / min(ts6), "seconds": ts6, "median_psnr": float(np.median(psnr6))}
    # refinement alone (the indirect estimate precomputed)
    seq = sh.seq
    init = roadmap.affine_to_projective(motion.estimate_sequence(seq, 1), int(motion.BBME_BLOCK_SIZE))
    _, tr = timed(lambda: seq.refine_projective(1, init))
    out["refine_projective_only"] = {"pairs_per_s": P / min(tr), "seconds": tr}
    if args.sample:
        iters = []
        for p in np.linspace(0, P - 1, args.sample).astype(int):
            info = {}
            direct.refine([seq.read_frame(p, l) for l in range(3)], [seq.read_frame(p + 1, l) for l in range(3)], init[p], info=info)
            iters.append(info["iters"])
        it = np.mean(np.array(iters, dtype=np.float64), axis=0)
        out["mean_steps_per_level"] = it.tolist()
        out["steps_sample"] = [list(map(int, x)) for x in iters]
    sh.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
