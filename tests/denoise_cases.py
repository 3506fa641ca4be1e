"""The shapes, seeds, frames and fields that tests/test_denoise_host.py and tests/test_gpu_denoise.py share.  A case has a noise
frame as the current frame and four references: the first and the third are the current frame plus noise within +-3, so that
weights are non-zero under small vectors, the second and the fourth independent noise, where almost every weight is zero.  The
host results are computed once per process and handed out read-only."""
import functools

import numpy as np

import denoise

# (H, W), B: the smallest shapes at which the kernel can go wrong
CASES = (
    ((4, 4), 4),         # every window pixel clamps
    ((9, 13), 4),        # tails in both axes; W below one lane group of the row frame
    ((37, 53), 5),       # odd B
    ((37, 53), 8),
    ((20, 300), 16),     # crosses the 256-column workgroup boundary: the neighbour columns of a lane lie in another workgroup
    ((33, 261), 32),
    ((5, 257), 4),       # one column past a workgroup; H not a multiple of 4
)
SMALL = CASES[:4]        # what the scalar restatement walks on the host
REFS = (1, 2, 3, 4)
STRENGTHS = (1, 24, 64)
UNITS = (False, True)    # integer field, quarter field


def case_id(case):
    return "%dx%d-b%d" % (case[0] + (case[1],))


def _rng(case, salt):
    (H, W), B = case
    return np.random.default_rng([H, W, B, 7, salt])


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def current(case):
    return _frozen(_rng(case, 0).integers(0, 256, size=case[0], dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def refs(case):
    """-> four uint8[H, W]: current + noise in -3 .. 3 (clipped), noise, current + other noise in -3 .. 3, other noise."""
    out = []
    for r in range(4):
        rng = _rng(case, 1 + r)
        if r % 2 == 0:
            a = np.clip(current(case).astype(np.int64) + rng.integers(-3, 4, size=case[0]), 0, 255).astype(np.uint8)
        else:
            a = rng.integers(0, 256, size=case[0], dtype=np.uint8)
        out.append(_frozen(a))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fields(case, quarter):
    """-> four int32[Hb, Wb, 2]: three blocks in four carry the zero vector (where the near-copies of the current frame weigh),
    the others vectors within +-6 quarter or +-2 whole pixels."""
    (H, W), B = case
    Hb, Wb = H // B, W // B
    reach = 6 if quarter else 2
    out = []
    for r in range(4):
        rng = _rng(case, (20 if quarter else 10) + r)
        f = rng.integers(-reach, reach + 1, size=(Hb, Wb, 2)).astype(np.int32)
        f[rng.integers(0, 4, size=(Hb, Wb)) != 0] = 0
        out.append(_frozen(f))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def truth(case):
    return _frozen(_rng(case, 99).integers(0, 256, size=case[0], dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def predictions(case, quarter):
    return tuple(_frozen(denoise.predict(r, f, case[1], quarter)) for r, f in zip(refs(case), fields(case, quarter)))


@functools.lru_cache(maxsize=None)
def want(case, R, strength, quarter):
    """denoise.frame of the case's first R references -> uint8[H, W], read-only."""
    return _frozen(denoise.blend(current(case), predictions(case, quarter)[:R], strength))
