#!/usr/bin/env python3
"""Time of overlapped block motion compensation beside the plain quarter-pel compensation, on one GPU.

Resident frames, 720x480 x `--frames` and 1920x1080 x `--frames-1080`, blocks of 16, frame distance 1, all figures from one run.
Per size three fields, each searched and refined to quarter pixels on the device, so that both kernels read the same pairs and
the same field from the sequence:
  pan      frames cut from one noise canvas that moves by (3, 2) pixels per frame, exhaustive search at window 8: one vector in
           (nearly) every block, the case the equal-vector path of k_obmc serves,
  diamond  the synthetic frames (gme_seq_synth, the frames of tools/interp_bench.py) under the diamond search,
  random   independent noise frames under the exhaustive search at window 16: the winner among equally bad candidates is uniform
           within +-16 pixels, +-64 quarter units after the refinement, and no two neighbours agree: the worst case of sixteen
           taps per pixel.
Per field, over every pair,
  k_obmc              gme_seq_obmc on the quarter-pel field without an output: the launch and the wait,
  k_compensate_qpel   gme_seq_compensate_qpel without an output: the launch and the wait,
  obmc_sse            gme_seq_obmc with sse_out only, in pairs per second,
  obmc_frames         gme_seq_obmc with the frames read back as well (what Sequence.obmc does), in pairs per second,
and `ratio`, k_obmc over k_compensate_qpel.  One launch carries every pair; all of these are blocking calls, so a figure holds the
host's wait as well (`rocprofv3 --kernel-trace --stats -- python tools/obmc_bench.py --reps 1` for the kernels' own times).
Every configuration is warmed up once, then `--reps` calls are timed together between gme_timer_start and gme_timer_stop (device
events on the launch stream).  `quality` is the mean PSNR of the plain and of the overlapped compensation by the integer and by
the quarter-pel field on the first `--pairs` pairs; `agree` the share of blocks whose vector equals that of all four direct
neighbours.  These figures are recorded, not asserted.  Prints one JSON line.
usage: python tools/obmc_bench.py [--frames 64] [--frames-1080 16] [--reps 3] [--pairs 4]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "global-motion-estimation_amd"), REPO]

import numpy as np  # noqa: E402

BS, PNORM, FD = 16, 0, 1
FIELDS = {"pan": (8, 0), "diamond": (16, 3), "random": (16, 0)}        # search window, searching procedure


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def fill(seq, name, H, W):
    """The frames of one field into the sequence."""
    if name == "diamond":
        seq.synth(1234, 0)
        return
    rng = np.random.default_rng(len(name))
    if name == "random":
        for k in range(seq.N):
            seq.upload(k, rng.integers(0, 256, size=(1, H, W), dtype=np.uint8))
        return
    canvas = rng.integers(0, 256, size=(H + 2 * seq.N, W + 3 * seq.N), dtype=np.uint8)
    for k in range(seq.N):
        seq.upload(k, canvas[None, 2 * k:2 * k + H, 3 * k:3 * k + W])


def agreement(q):
    """Share of the blocks whose vector equals that of the four direct neighbours (the grid's border counts as agreeing)."""
    same = np.ones(q.shape[:3], bool)
    for axis in (1, 2):
        eq = np.all(np.take(q, range(1, q.shape[axis]), axis) == np.take(q, range(q.shape[axis] - 1), axis), axis=-1)
        pad = [(0, 0)] * 3
        pad[axis] = (1, 0)
        same &= np.pad(eq, pad, constant_values=True)
        pad[axis] = (0, 1)
        same &= np.pad(eq, pad, constant_values=True)
    return float(same.mean())


def one_field(native, obmc, seq, name, H, W, reps, pairs):
    ctx = native.default_context()
    sw, procedure = FIELDS[name]
    fill(seq, name, H, W)
    seq.bbme(FD, BS, sw, procedure, PNORM)
    seq.subpel(FD, BS, PNORM, 2)
    P = seq.N - FD
    frames, err = np.zeros((P, H, W), np.uint8), np.zeros(P, np.int64)
    u8, i64 = native._c_u8p, native._c_i64p

    def lapped(f, e):
        return lambda: native._check(seq.lib.gme_seq_obmc(seq.handle, FD, BS, 1, 0, P, f, e), seq.lib)

    runs = {"k_obmc": lapped(None, None),
            "k_compensate_qpel": lambda: native._check(seq.lib.gme_seq_compensate_qpel(seq.handle, FD, BS, None), seq.lib),
            "obmc_sse": lapped(None, native._p(err, i64)), "obmc_frames": lapped(native._p(frames, u8), native._p(err, i64))}
    out = {}
    for key, fn in runs.items():
        ms = timed(ctx, fn, reps)
        out[key] = {"ms": ms, "ms_per_pair": ms / P, "pairs_per_s": P / (ms * 1e-3)}
    out["ratio"] = out["k_obmc"]["ms"] / out["k_compensate_qpel"]["ms"]
    out["agree"] = agreement(seq.read_qmv()[0])
    n = min(pairs, P)
    plain_q = seq.compensate_qpel(FD, BS)[:n]
    lap_q = seq.obmc(FD, BS, True, 0, n)[1]
    lap_i = seq.obmc(FD, BS, False, 0, n)[1]
    mv = seq.read_mv(0, n)
    plain_i = [ctx.sse(seq.read_frame(k + FD), ctx.compensate(seq.read_frame(k), mv[k])) for k in range(n)]
    mean = lambda v: float(np.mean([obmc.psnr(int(s), H, W) for s in v]))       # noqa: E731
    out["quality"] = {"pairs": n, "psnr_integer_plain": mean(plain_i), "psnr_integer_obmc": mean(lap_i),
                      "psnr_qpel_plain": mean(plain_q), "psnr_qpel_obmc": mean(lap_q)}
    return out


def size(native, obmc, H, W, n, reps, pairs):
    seq = native.Sequence(native.default_context(), n, H, W)
    out = {"shape": [H, W], "frames": n, "pairs": n - FD, "blocks_per_pair": (H // BS) * (W // BS)}
    for name in FIELDS:
        out[name] = one_field(native, obmc, seq, name, H, W, reps, pairs)
    seq.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frames-1080", dest="frames_1080", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4)
    args = ap.parse_args()
    import _gme_native as native
    import obmc
    sizes = [(480, 720, args.frames), (1080, 1920, args.frames_1080)]
    print(json.dumps({"config": {"bs": BS, "pnorm": PNORM, "frame_distance": FD, "reps": args.reps,
                                 "fields": {k: {"search_window": v[0], "searching_procedure": v[1]} for k, v in FIELDS.items()}},
                      "sizes": [size(native, obmc, H, W, n, args.reps, args.pairs) for H, W, n in sizes if n > FD]}))


if __name__ == "__main__":
    main()
