#!/usr/bin/env python3
"""Throughput and compensation quality of the vector propagation search beside the existing searches, on one GPU.

Resident synthetic frames (gme_seq_synth, the frames of tools/gmc_bench.py), 720x480 x `--frames` and 1920x1080 x
`--frames-1080`, blocks of 16, MAE, frame distance 1.  The camera field comes from the direct projective refinement of the same
frames (propagate.camera_field of roadmap.refine_sequence), computed once outside the timed calls.  Per size:
  diamond              Sequence.bbme, procedure 3 at window 16,
  diamond_prop         the same followed by Sequence.prop (2 rounds, 1 step, temporal prior, no camera field),
  diamond_prop_camera  ... with the camera field,
  exhaustive           Sequence.bbme, procedure 0 at window 16,
  hier                 Sequence.hier, three levels, coarse window 8, radius 1,
each in pairs per second with the PSNR of ``current`` against the integer compensation by its field (gme_compensate_u8 and
gme_sse_u8 per pair, mean over the first `--pairs` pairs), the share of vectors that differ from the exhaustive field's, and for
the propagated fields the share per source class.  `prop_launch` is one round (one k_prop launch per chunk of pairs) with one
step on the diamond field: the time of search + one round minus the time of the search.  Every configuration is warmed up once,
then `--reps` calls are timed together between gme_timer_start and gme_timer_stop (device events on the launch stream); all of
these are blocking calls, so a figure holds the host's wait as well.  Then the same five on the first `--pairs` pairs of the g9
golden frames, quality only.  These figures are recorded, not asserted.  Prints one JSON line.
usage: python tools/prop_bench.py [--frames 64] [--frames-1080 16] [--reps 3] [--pairs 8]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, PNORM, FD, SW, ROUNDS, STEPS = 16, 0, 1, 16, 2, 1


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def camera(propagate, roadmap, seq, H, W):
    """(g int32[P, h, w, 2], pairs without a camera field: they get zeros)."""
    h = roadmap.refine_sequence(seq, FD)[0]
    fields = [propagate.camera_field(w, H, W, BS) for w in h]
    zero = np.zeros((H // BS, W // BS, 2), np.int32)
    return np.stack([zero if a is None else a for a in fields]), int(sum(a is None for a in fields))


def searches(seq, g):
    return {
        "diamond": lambda: seq.bbme(FD, BS, SW, 3, PNORM),
        "diamond_prop": lambda: (seq.bbme(FD, BS, SW, 3, PNORM), seq.prop(FD, BS, PNORM, ROUNDS, STEPS, True, None)),
        "diamond_prop_camera": lambda: (seq.bbme(FD, BS, SW, 3, PNORM), seq.prop(FD, BS, PNORM, ROUNDS, STEPS, True, g)),
        "exhaustive": lambda: seq.bbme(FD, BS, SW, 0, PNORM),
        "hier": lambda: seq.hier(FD, BS, 8, 1, PNORM, 3),
    }


def quality(ctx, vbs, frames, fields, source, reference):
    """Mean PSNR of the integer compensation over the pairs of ``frames``, vectors that differ from ``reference``'s."""
    H, W = frames.shape[1:]
    sse = [int(ctx.sse(frames[k + FD], ctx.compensate(frames[k], fields[k]))) for k in range(len(fields))]
    out = {"psnr": float(np.mean([vbs.psnr(s, H, W) for s in sse])), "sse": int(np.sum(sse)),
           "differs_from_exhaustive": float(np.mean(np.any(fields != reference, axis=-1)))}
    if source is not None:
        out["source_share"] = [float(np.mean((source & 7) == c)) for c in range(5)]
        out["moved_share"] = float(np.mean((source & 8) != 0))
    return out


def measure(native, propagate, roadmap, vbs, seq, frames, pairs, reps):
    """The five configurations on a resident sequence: quality on its first ``pairs`` pairs (``frames``: those pairs' frames on
    the host) and, with ``reps``, the rates over all of its pairs."""
    ctx = native.default_context()
    H, W = frames.shape[1:]
    g, missing = camera(propagate, roadmap, seq, H, W)
    out = {"camera_fields_missing": missing}
    runs = searches(seq, g)
    runs["exhaustive"]()
    reference = seq.read_mv(0, pairs)
    for name, fn in runs.items():
        row = {}
        if reps:
            ms = timed(ctx, fn, reps)
            P = seq.N - FD
            row.update(ms=ms, ms_per_pair=ms / P, pairs_per_s=P / (ms * 1e-3), plan=ctx.last_bbme_info()["plan"])
        else:
            fn()
        source = seq.read_prop(0, pairs)[2] if "prop" in name else None
        row.update(quality(ctx, vbs, frames, seq.read_mv(0, pairs), source, reference))
        out[name] = row
    if reps:
        one = timed(ctx, lambda: (seq.bbme(FD, BS, SW, 3, PNORM), seq.prop(FD, BS, PNORM, 1, STEPS, True, g)), reps)
        out["prop_launch"] = {"ms": one - out["diamond"]["ms"], "search_ms": out["diamond"]["ms"],
                              "ratio_to_search": (one - out["diamond"]["ms"]) / out["diamond"]["ms"]}
        out["prop_share"] = 1.0 - out["diamond"]["ms"] / out["diamond_prop_camera"]["ms"]
    return out


def synthetic(native, propagate, roadmap, vbs, H, W, n, pairs, reps):
    seq = native.Sequence(native.default_context(), n, H, W)
    seq.synth(1234, 0)
    pairs = min(pairs, n - FD)
    frames = np.stack([seq.read_frame(k) for k in range(pairs + FD)])
    out = {"shape": [H, W], "frames": n, "pairs": n - FD, "quality_pairs": pairs, "blocks_per_pair": (H // BS) * (W // BS)}
    out.update(measure(native, propagate, roadmap, vbs, seq, frames, pairs, reps))
    seq.close()
    return out


def golden(native, propagate, roadmap, vbs, pairs):
    g9 = np.ascontiguousarray(np.load(os.path.join(REPO, "tests", "golden", "g9_pan240seq.npz"))["frames"][:pairs + FD])
    seq = native.Sequence.from_frames(native.default_context(), g9)
    out = {"clip": "g9_pan240seq", "shape": list(g9.shape[1:]), "pairs": pairs}
    out.update(measure(native, propagate, roadmap, vbs, seq, g9, pairs, 0))
    seq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=8)
    args = ap.parse_args()
    import _gme_native as native
    import propagate
    import roadmap
    import vbs
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "pnorm": PNORM, "frame_distance": FD, "sw": SW, "rounds": ROUNDS, "steps": STEPS,
                                 "hier": {"levels": 3, "coarse_window": 8, "radius": 1}, "reps": args.reps},
                      "sizes": [synthetic(native, propagate, roadmap, vbs, H, W, n, args.pairs, args.reps) for H, W, n in sizes if n > FD],
                      "quality": golden(native, propagate, roadmap, vbs, args.pairs)}))


if __name__ == "__main__":
    main()
