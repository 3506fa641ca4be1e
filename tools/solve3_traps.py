#!/usr/bin/env python3
"""Regenerates tests/golden/solve3_traps.npz: normal-equation systems on which the affine device solve and the host solve
(inv(F) @ S) round one block of the model field differently.

CPU only.  For each family of tests/solve_cases.TRAP_FAMILIES a seeded search draws S = F p over an ill-conditioned inlier set
and moves p0 so that the block where the two solutions differ most sits on a rounding tie between them
(solve_cases.trap_search).  A try is a trap when the rounded fields differ and the rule k_solve3 had before -- plain
elimination, a fixed margin of 1e-9 around k + 0.5, no conditioning flag -- leaves it unflagged.  Per family the file keeps
the first PER_FAMILY traps; where the search finds fewer (480 x 720 yields none) the tries with the largest difference
between the two fields fill the rest.

The host solution decides only which tries are kept.  The file stores what does not depend on the LAPACK build: sums15, h, w,
project, the restated parameters and flags of the shipped kernel (solve_cases.device_np), the flags of the old rule, the
family's name, and `old_unflagged`, the number of records the old rule let through.  The tests recompute host solutions.

usage: python tools/solve3_traps.py [--tries 1200] [--out tests/golden/solve3_traps.npz]"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import solve_cases as sc  # noqa: E402

PER_FAMILY = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tries", type=int, default=1200)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "solve3_traps.npz"))
    args = ap.parse_args()
    rec = dict(sums=[], h=[], w=[], project=[], params=[], flags=[], old_flags=[], family=[])
    for seed, (name, h, w, family, translation) in enumerate(sc.TRAP_FAMILIES):
        tries = list(sc.trap_search(h, w, family, translation, args.tries, [2024, seed]))
        traps = [t for t in tries if t["differs"] and t["old_flags"] == 0]
        rest = sorted((t for t in tries if not (t["differs"] and t["old_flags"] == 0)), key=lambda t: -t["spread"])
        keep = (traps + rest)[:PER_FAMILY]
        print("%-24s %4d tries, %3d traps under the fixed margin, kept %d (%d traps)" % (
            name, len(tries), len(traps), len(keep), min(len(traps), PER_FAMILY)))
        for t in keep:
            p, flags = sc.device_np(t["sums"], h, w)
            rec["sums"].append(t["sums"]); rec["h"].append(h); rec["w"].append(w); rec["project"].append(0)
            rec["params"].append(p); rec["flags"].append(flags); rec["old_flags"].append(t["old_flags"]); rec["family"].append(name)
    old_unflagged = int(sum(1 for f in rec["old_flags"] if f == 0))
    np.savez_compressed(args.out, sums=np.array(rec["sums"]), h=np.array(rec["h"], np.int32), w=np.array(rec["w"], np.int32),
                        project=np.array(rec["project"], np.int32), params=np.array(rec["params"]),
                        flags=np.array(rec["flags"], np.int32), old_flags=np.array(rec["old_flags"], np.int32),
                        family=np.array(rec["family"]), old_unflagged=np.int32(old_unflagged))
    print("%d records, %d unflagged under the fixed margin, %d unflagged under the shipped rule -> %s" % (
        len(rec["h"]), old_unflagged, int(sum(1 for f in rec["flags"] if f == 0)), args.out))


if __name__ == "__main__":
    main()
