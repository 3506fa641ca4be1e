"""Frames, fields and penalties shared by the bidirectional-prediction tests (host and GPU)."""
import functools

import numpy as np

import bipred
import vbs_cases

# ---- the occlusion scene --------------------------------------------------------------------------------------------------
# checked on the CPU: of the seeds 1 .. 8 every one but 7 meets check_scene's three conditions in both norms (at 7 one block
# misses them under MAE); the first is taken
SCENE_SEED = 1
SCENE_SHAPE, SCENE_BLOCK, SCENE_WINDOW = (64, 128), 16, 8
SCENE_OBJECT = (16, 48, 32, 6)                                   # first row, first column at t = 0, side, columns moved per frame
SCENE_NOISE = 8
SCENE_ARGS = dict(block_size=SCENE_BLOCK, radius=1, rounds=1)


@functools.lru_cache(maxsize=None)
def occlusion_scene():
    """(past, mid, next): a background panning one column per frame, a patch of another canvas moving six columns per frame
    over it, and independent uniform noise of +-SCENE_NOISE grey levels on every frame."""
    (H, W), m = SCENE_SHAPE, 8
    top, left, side, step = SCENE_OBJECT
    background = vbs_cases.canvas(SCENE_SEED, H, W + 2 * m)
    patch = vbs_cases.canvas(SCENE_SEED + 1000, side, side)
    rng = np.random.default_rng(SCENE_SEED + 2000)
    frames = []
    for t in (-1, 0, 1):
        f = background[:, m + t:m + t + W].astype(np.int64)
        f[top:top + side, left + step * t:left + step * t + side] = patch
        f = np.clip(f + rng.integers(-SCENE_NOISE, SCENE_NOISE + 1, size=(H, W)), 0, 255).astype(np.uint8)
        f.setflags(write=False)
        frames.append(f)
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def scene_result(pnorm):
    """(f0, f1, mode, v0, v1, cost, costs) of the scene on the host at the default penalty, computed once."""
    past, mid, nxt = occlusion_scene()
    f0 = vbs_cases.exhaustive(mid, past, SCENE_BLOCK, SCENE_WINDOW, pnorm)
    f1 = vbs_cases.exhaustive(mid, nxt, SCENE_BLOCK, SCENE_WINDOW, pnorm)
    out = (f0, f1) + bipred.decide(past, mid, nxt, f0, f1, pnorm=pnorm, penalty=bipred.default_penalty(SCENE_BLOCK, pnorm), **SCENE_ARGS)
    for a in out:
        a.setflags(write=False)
    return out


def check_scene(mode):
    """The three conditions of the scene: block rows 1 - 2 of column 2 choose the next frame (the object still hides them in the
    past one), those of column 5 the past frame (the object hides them in the next one), and every other block of columns
    1 .. 6 the average."""
    want = np.full(mode.shape, bipred.BOTH, np.uint8)
    want[1:3, 2] = bipred.NEXT
    want[1:3, 5] = bipred.PAST
    assert np.array_equal(mode[:, 1:7], want[:, 1:7]), mode


# ---- noise ------------------------------------------------------------------------------------------------------------------
# (shape, block_size, radius, rounds): frame sizes that are no multiple of the block (48 x 80 at 16 is), the compiled instances
# (16 and 32) and the run-time one, rows of 12 and 24 bytes, no refinement by radius 0 and by rounds 0, and rows of 10 bytes,
# whose last dword holds bytes beyond the block
NOISE = (((37, 53), 8, 1, 1), ((37, 53), 8, 1, 2), ((37, 53), 12, 1, 2), ((48, 80), 16, 1, 1), ((48, 80), 16, 0, 1),
         ((70, 101), 16, 2, 2), ((70, 101), 32, 1, 1), ((70, 101), 24, 2, 1), ((70, 101), 16, 1, 0), ((130, 135), 64, 2, 2),
         ((37, 53), 10, 1, 2))
FIELD_REACH = 6                                                  # the random input vectors lie in [-6, 6]: some point outside

# Seed per case and penalty per (case, norm), chosen on the CPU so that the host's modes hold every value 0 .. 3: the first
# seed from 2000 + 1000 * (index of the case) on at which some block has both vectors outside and the others spread over the
# three predictors, and the penalty nearest the median of min(c0, c1) - cb over the blocks with both vectors inside at which
# all four modes occur.  (On noise the average beats either reference by about a third of their cost; without a penalty of
# that order every block with both vectors inside would choose it.)
SEED = {NOISE[0]: 2000, NOISE[1]: 3000, NOISE[2]: 4000, NOISE[3]: 5000, NOISE[4]: 6000, NOISE[5]: 7000, NOISE[6]: 8000,
        NOISE[7]: 9000, NOISE[8]: 10000, NOISE[9]: 11017, NOISE[10]: 12000}
PENALTY = {
    (NOISE[0], 0): 1206, (NOISE[0], 1): 268712,
    (NOISE[1], 0): 1234, (NOISE[1], 1): 259417,
    (NOISE[2], 0): 2621, (NOISE[2], 1): 575169,
    (NOISE[3], 0): 3051, (NOISE[3], 1): 662098,
    (NOISE[4], 0): 2334, (NOISE[4], 1): 624660,
    (NOISE[5], 0): 4537, (NOISE[5], 1): 1034701,
    (NOISE[6], 0): 11161, (NOISE[6], 1): 2861505,
    (NOISE[7], 0): 8767, (NOISE[7], 1): 1967729,
    (NOISE[8], 0): 2157, (NOISE[8], 1): 585890,
    (NOISE[9], 0): 45664, (NOISE[9], 1): 11552391,
    (NOISE[10], 0): 1666, (NOISE[10], 1): 343598,
}
# the cases in which some refined pair must differ from the input at the case's penalty (both were seen to at penalty 0 first)
REFINED = (NOISE[1], NOISE[5])


@functools.lru_cache(maxsize=None)
def noise_triple(case):
    """(past, mid, next, f0, f1) of a noise case; the same arrays on every call."""
    shape, bs, radius, rounds = case
    rng = np.random.default_rng(SEED[case])
    frames = rng.integers(0, 256, size=(3,) + tuple(shape), dtype=np.uint8)
    f = rng.integers(-FIELD_REACH, FIELD_REACH + 1, size=(2, shape[0] // bs, shape[1] // bs, 2)).astype(np.int32)
    for a in (frames, f):
        a.setflags(write=False)
    return frames[0], frames[1], frames[2], f[0], f[1]


@functools.lru_cache(maxsize=None)
def noise_result(case, pnorm):
    """bipred.decide of a noise case at its penalty, computed once -> (mode, v0, v1, cost, costs)."""
    shape, bs, radius, rounds = case
    past, mid, nxt, f0, f1 = noise_triple(case)
    out = bipred.decide(past, mid, nxt, f0, f1, bs, radius, rounds, pnorm, PENALTY[case, pnorm])
    for a in out:
        a.setflags(write=False)
    return out
