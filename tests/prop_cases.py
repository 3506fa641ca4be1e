"""Frames, fields and results shared by the vector-propagation tests (host and GPU)."""
import functools

import numpy as np

import gmc_cases
import propagate
import vbs_cases

# ---- the pan scene ------------------------------------------------------------------------------------------------------------
# checked on the CPU with propagate.py itself: with seed 1 the wavefront, camera, temporal and refinement tests of
# test_prop_host.py hold in both norms
PAN_SEED = 1
PAN_SHAPE, PAN_MARGIN, PAN_BLOCK = (80, 112), 8, 16
PAN_MOVE = (5, -3)                                               # (column, row): where the content of `previous` lies in `current`
PAN_NOISE = 4
PAN_START = (2, 3)                                               # the one block of the wavefront's prior that carries PAN_MOVE
REFINE_OFFSETS = ((1, 1), (-1, 0), (1, -1))


@functools.lru_cache(maxsize=None)
def pan_scene(seed=PAN_SEED):
    """(previous, current): a pan of PAN_MOVE over a canvas, independent uniform noise of +-PAN_NOISE on both frames."""
    (H, W), m = PAN_SHAPE, PAN_MARGIN
    c = vbs_cases.canvas(seed, H + 2 * m, W + 2 * m)
    rng = np.random.default_rng(seed + 2000)
    out = []
    for vx, vy in ((0, 0), PAN_MOVE):
        f = c[m - vy:m - vy + H, m - vx:m - vx + W].astype(np.int64)
        f = np.clip(f + rng.integers(-PAN_NOISE, PAN_NOISE + 1, size=(H, W)), 0, 255).astype(np.uint8)
        f.setflags(write=False)
        out.append(f)
    return out[0], out[1]


def grid(shape=PAN_SHAPE, bs=PAN_BLOCK):
    return shape[0] // bs, shape[1] // bs


def available_mask(shape, bs, v):
    """bool[Hb, Wb]: where the vector v is available."""
    H, W = shape
    Hb, Wb = grid(shape, bs)
    return np.array([[propagate.available(H, W, i * bs, j * bs, bs, int(v[0]), int(v[1])) for j in range(Wb)] for i in range(Hb)])


def constant_field(v, shape=PAN_SHAPE, bs=PAN_BLOCK):
    f = np.zeros(grid(shape, bs) + (2,), np.int32)
    f[:, :] = v
    return f


def wavefront_prior():
    f = constant_field((0, 0))
    f[PAN_START] = PAN_MOVE
    return f


def reached(ok, start, steps):
    """bool grid: the blocks reached from ``start`` in at most ``steps`` steps of the 8-neighbourhood through blocks of ``ok``."""
    cur = np.zeros(ok.shape, bool)
    cur[start] = True
    for _ in range(steps):
        p = np.pad(cur, 1)
        grown = np.zeros(ok.shape, bool)
        for di in (0, 1, 2):
            for dj in (0, 1, 2):
                grown |= p[di:di + ok.shape[0], dj:dj + ok.shape[1]]
        cur = cur | (grown & ok)
    return cur


@functools.lru_cache(maxsize=None)
def wavefront_result(pnorm, rounds):
    previous, current = pan_scene()
    return frozen(propagate.search(previous, current, wavefront_prior(), PAN_BLOCK, pnorm, rounds, 0))


@functools.lru_cache(maxsize=None)
def inherit_result(pnorm, which):
    """One round without refinement on a zero prior with PAN_MOVE everywhere in ``t`` (which = "t") or ``g`` ("g")."""
    previous, current = pan_scene()
    field = {which: constant_field(PAN_MOVE)}
    return frozen(propagate.search(previous, current, constant_field((0, 0)), PAN_BLOCK, pnorm, 1, 0, **field))


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


# ---- noise ----------------------------------------------------------------------------------------------------------------------
NOISE = gmc_cases.NOISE                                          # (shape, block_size): see there
FIELD_REACH, COPY_NOISE = 6, 2
ROUNDS_STEPS = ((1, 0), (2, 1), (3, 2), (4, 4))
GIVEN = ((True, True), (True, False), (False, True), (False, False))     # (t given, g given)

# Seed per case, chosen on the CPU (find_seed below): the first seed from 3000 + 1000 * (index of the case) on at which the
# host's sources, over the results of both norms and every entry of ROUNDS_STEPS with t and g given, hold all five classes and
# the MOVED flag.  (The union, not each result: the case of 130 x 135 at 64 has four blocks.)
SEED = {NOISE[0]: 3000, NOISE[1]: 4000, NOISE[2]: 5000, NOISE[3]: 6000, NOISE[4]: 7000, NOISE[5]: 8006, NOISE[6]: 9004,
        NOISE[7]: 10001, NOISE[8]: 11000}


def _noise_pair(case, seed):
    (H, W), bs = case
    Hb, Wb = H // bs, W // bs
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(2, H, W), dtype=np.uint8)
    previous, current = frames[0], frames[1].copy()
    f, t, g = (rng.integers(-FIELD_REACH, FIELD_REACH + 1, size=(Hb, Wb, 2)).astype(np.int32) for _ in range(3))
    # on pure noise every candidate costs about the same: a random half of the blocks is found in `current` where one of its
    # candidates points (own, a neighbour's, temporal, camera, zero, or one pixel beside its own, for the refinement), with
    # noise of +-COPY_NOISE
    for i in range(Hb):
        for j in range(Wb):
            kind, ni, nj, ox, oy = rng.integers(0, 6), rng.integers(-1, 2), rng.integers(-1, 2), rng.integers(-1, 2), rng.integers(-1, 2)
            if rng.random() >= 0.5:
                continue
            ni, nj = min(max(i + ni, 0), Hb - 1), min(max(j + nj, 0), Wb - 1)
            v = (f[i, j], f[ni, nj], t[i, j], g[i, j], (0, 0), (f[i, j, 0] + ox, f[i, j, 1] + oy))[kind]
            vx, vy = int(v[0]), int(v[1])
            y, x = i * bs, j * bs
            if not propagate.available(H, W, y, x, bs, vx, vy):
                continue
            blk = previous[y:y + bs, x:x + bs].astype(np.int64)
            current[y + vy:y + vy + bs, x + vx:x + vx + bs] = np.clip(blk + rng.integers(-COPY_NOISE, COPY_NOISE + 1, size=(bs, bs)), 0, 255)
    return frozen((previous, current, f, t, g))


@functools.lru_cache(maxsize=None)
def noise_pair(case):
    """(previous, current, f, t, g) of a noise case; the same arrays on every call."""
    return _noise_pair(case, SEED[case])


def _noise_search(pair, bs, pnorm, rounds, steps, with_t, with_g):
    previous, current, f, t, g = pair
    return propagate.search(previous, current, f, bs, pnorm, rounds, steps, t if with_t else None, g if with_g else None)


@functools.lru_cache(maxsize=None)
def noise_result(case, pnorm, rounds, steps, with_t, with_g):
    """propagate.search of a noise case, computed once -> (mf, cost, source)."""
    return frozen(_noise_search(noise_pair(case), case[1], pnorm, rounds, steps, with_t, with_g))


def sources_seen(results):
    """The set of classes, and 8 if any block moved, over the source maps of ``results``."""
    seen = set()
    for _, _, source in results:
        seen |= set((np.unique(source) & 7).tolist())
        if np.any(source & propagate.MOVED):
            seen.add(propagate.MOVED)
    return seen


ALL_SOURCES = {0, 1, 2, 3, 4, 8}


def find_seed(case, start):
    """How SEED was chosen (CPU only, not run by the tests)."""
    seed = start
    while True:
        pair = _noise_pair(case, seed)
        res = [_noise_search(pair, case[1], pnorm, r, s, True, True) for pnorm in (0, 1) for r, s in ROUNDS_STEPS]
        if sources_seen(res) == ALL_SOURCES:
            return seed
        seed += 1


# ---- ties and saturated content ---------------------------------------------------------------------------------------------------
def ties_frames():
    """Constant frames: every candidate of a block costs the same."""
    return gmc_cases.ties_frames()


def ties_fields(bs):
    """(f, t, g) for the ties frames (37 x 53): random vectors in [-2, 2], and block (0, 0) with an own vector that points outside,
    an upper-left corner whose first available candidate in list order is its right neighbour's vector."""
    rng = np.random.default_rng(5 + bs)
    f, t, g = (rng.integers(-2, 3, size=(37 // bs, 53 // bs, 2)).astype(np.int32) for _ in range(3))
    f[0, 0] = (-1, -1)
    f[0, 1] = (1, 2)
    return f, t, g


# ---- the sequence -----------------------------------------------------------------------------------------------------------------
SEQ_SHAPE, SEQ_WINDOW = (5, 48, 80), 4


@functools.lru_cache(maxsize=None)
def seq_frames():
    """tests/test_gpu_gmc.py's recipe: a pan of one pixel per frame with fresh noise of +-6 on every frame."""
    rng = np.random.default_rng(48)
    base = rng.integers(0, 256, size=(SEQ_SHAPE[1] + 8, SEQ_SHAPE[2] + 8), dtype=np.uint8)
    frames = np.stack([np.clip(base[4:-4, k:k + SEQ_SHAPE[2]].astype(np.int64) + rng.integers(-6, 7, size=SEQ_SHAPE[1:]), 0, 255)
                       for k in range(SEQ_SHAPE[0])]).astype(np.uint8)
    frames = np.ascontiguousarray(frames)
    frames.setflags(write=False)
    return frames


def seq_camera(pairs, bs):
    """A camera field per pair int32[pairs, Hb, Wb, 2]: the pan's vector, one pixel off on every other pair."""
    g = np.zeros((pairs, SEQ_SHAPE[1] // bs, SEQ_SHAPE[2] // bs, 2), np.int32)
    for k in range(pairs):
        g[k, :, :] = (-1 - (k & 1), k & 1)
    return g
