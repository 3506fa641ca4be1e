"""The shapes, seeds and fields that tests/test_obmc_host.py and tests/test_gpu_obmc.py share: noise frames, random vectors within
+-40 quarter pixels, and in two corner blocks the extremes of the vector range.  The host results are computed once per process
and handed out read-only."""
import functools

import numpy as np

import obmc

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# (H, W), B: the smallest shapes at which the kernel can go wrong
CASES = (
    ((9, 13), 4),        # tails in both axes; W below one lane group of the row frame
    ((37, 53), 5),       # odd B: the zero-weight centre row and column
    ((37, 53), 8),
    ((37, 53), 12),      # 4 B^2 is not a power of two
    ((20, 300), 16),     # crosses the 256-column workgroup boundary of the row frame; the last whole block ends at 288; H % 4 == 0
    ((33, 261), 32),     # one block row: every vertical neighbour clamps to the block itself
    ((64, 64), 64),      # a single block: every neighbour is the block itself
    ((70, 130), 64),
)
SMALL = CASES[:4]        # what the scalar restatement walks on the host
UNITS = (True, False)    # quarter field, integer field


def case_id(case):
    return "%dx%d-b%d" % (case[0] + (case[1],))


def _rng(case, salt):
    (H, W), B = case
    return np.random.default_rng([H, W, B, salt])


@functools.lru_cache(maxsize=None)
def frames(case):
    """-> (previous, current): two noise frames of the case's shape."""
    rng = _rng(case, 0)
    out = tuple(rng.integers(0, 256, size=case[0], dtype=np.uint8) for _ in range(2))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def field(case, quarter):
    """-> int32[Hb, Wb, 2]: within +-40 quarter pixels, as quarter vectors or as whole pixels; the first and the last block carry
    the extremes of the range (int32 for a quarter field, +-2^29 whole pixels for an integer field) with opposite signs."""
    (H, W), B = case
    Hb, Wb = H // B, W // B
    reach = 40 if quarter else 10
    f = _rng(case, 1 if quarter else 2).integers(-reach, reach + 1, size=(Hb, Wb, 2)).astype(np.int32)
    lo, hi = (INT32_MIN, INT32_MAX) if quarter else (-obmc.MAX_INTEGER_VECTOR, obmc.MAX_INTEGER_VECTOR)
    f[0, 0] = (lo, hi)
    f[Hb - 1, Wb - 1] = (hi, lo)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def want(case, quarter):
    """obmc.compensate of the case -> uint8[H, W], read-only."""
    out = obmc.compensate(frames(case)[0], field(case, quarter), case[1], quarter)
    out.setflags(write=False)
    return out
