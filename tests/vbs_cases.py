"""Frames, fields and penalties shared by the variable-block-size tests (host and GPU)."""
import functools

import numpy as np

import vbs

# ---- the two-motion scene -------------------------------------------------------------------------------------------------
SCENE_SEED = 1                                                   # fixed after checking test_two_motion_scene's conditions on the CPU
SCENE_SHAPE, SCENE_EDGE = (96, 128), 72
SCENE_LEFT, SCENE_RIGHT = (2, -1), (0, 1)                        # (column, row): where the content of `previous` lies in `current`
SCENE_ARGS = dict(block_size=16, depth=2, radius=2, pnorm=0, penalty=256)
SCENE_WINDOW = 6


def canvas(seed, H, W):
    """uint8[H, W]: uniform noise smoothed by a 3-tap box along both axes, stretched to 0 .. 255."""
    a = np.random.default_rng(seed).random((H + 2, W + 2))
    for axis in (0, 1):
        a = (np.roll(a, 1, axis) + a + np.roll(a, -1, axis)) / 3.0
    a = a[1:-1, 1:-1]
    return np.floor((a - a.min()) / (a.max() - a.min()) * 255.0 + 0.5).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def two_motion_scene():
    """(previous, current): what lies left of column SCENE_EDGE in ``previous`` moves by SCENE_LEFT, the rest by SCENE_RIGHT;
    the left part moves towards the right one and covers its first two columns."""
    (H, W), m = SCENE_SHAPE, 8
    c = canvas(SCENE_SEED, H + 2 * m, W + 2 * m)

    def moved(v):
        return c[m - v[1]:m - v[1] + H, m - v[0]:m - v[0] + W]
    previous = np.ascontiguousarray(c[m:m + H, m:m + W])
    x = np.arange(W)[None, :]
    current = np.ascontiguousarray(np.where(x < SCENE_EDGE + SCENE_LEFT[0], moved(SCENE_LEFT), moved(SCENE_RIGHT)))
    previous.setflags(write=False)
    current.setflags(write=False)
    return previous, current


def exhaustive(previous, current, block_size, window, pnorm):
    """The integer field of a full search of +-window: column offset in the outer loop, the first minimum wins, blocks that
    are not inside are skipped."""
    H, W = previous.shape
    bs = block_size
    mf = np.zeros((H // bs, W // bs, 2), np.int32)
    for i in range(H // bs):
        for j in range(W // bs):
            best = None
            for dx in range(-window, window + 1):
                for dy in range(-window, window + 1):
                    if vbs._inside(H, W, i * bs, j * bs, bs, dx, dy):
                        c = vbs._cost(previous, current, i * bs, j * bs, bs, dx, dy, pnorm)
                        if best is None or c < best:
                            best, mf[i, j] = c, (dx, dy)
    return mf


@functools.lru_cache(maxsize=None)
def scene_result():
    """(root field, leaf, depth, cost) of the scene on the host, computed once."""
    previous, current = two_motion_scene()
    mf = exhaustive(previous, current, SCENE_ARGS["block_size"], SCENE_WINDOW, SCENE_ARGS["pnorm"])
    out = (mf,) + vbs.tree(previous, current, mf, **SCENE_ARGS)
    for a in out:
        a.setflags(write=False)
    return out


def check_scene(mf, leaf, depth):
    """The three conditions of the scene: the four interior roots of the column that straddles SCENE_EDGE split, no interior
    root away from it does, and every leaf cell of the straddling roots carries the motion of its side."""
    B, D = SCENE_ARGS["block_size"], SCENE_ARGS["depth"]
    n, g = 1 << D, B >> D
    split = depth[::n, ::n] > 0
    j = SCENE_EDGE // B
    rows = np.arange(1, SCENE_SHAPE[0] // B - 1)
    away = [c for c in range(1, SCENE_SHAPE[1] // B - 1) if c != j]
    assert split[rows, j].all(), split
    assert not split[np.ix_(rows, away)].any(), split
    cells = leaf[rows[0] * n:(rows[-1] + 1) * n, j * n:(j + 1) * n]
    left = (j * B + g * np.arange(n)) < SCENE_EDGE
    assert np.all(cells[:, left] == SCENE_LEFT) and np.all(cells[:, ~left] == SCENE_RIGHT), cells


# ---- noise ------------------------------------------------------------------------------------------------------------------
# (shape, block_size, depth, radius): frame sizes that are no multiple of the root (48 x 80 at 16 is), the compiled instances
# (16 and 32 at depth 2) and the run-time one, leaf rows of 6 bytes (12 at depth 1, 24 at depth 2) and 12 bytes
NOISE = (((37, 53), 8, 1, 1), ((37, 53), 12, 1, 1), ((48, 80), 16, 2, 1), ((48, 80), 16, 0, 1), ((70, 101), 16, 2, 3),
         ((70, 101), 32, 2, 1), ((70, 101), 24, 2, 1), ((70, 101), 24, 1, 1), ((130, 135), 64, 2, 3), ((130, 135), 64, 1, 0))
FIELD_REACH = 6                                                  # the random input vectors lie in [-6, 6]: some roots point outside

# penalty per (case, norm), chosen on the CPU so that the host's depth map holds every value 0 .. depth.  At radius 0 a child
# has its parent's vector, the children's costs add up to the parent's, S = penalty + c is never below c and nothing can
# split: those cases run at penalty 0 and the host test asserts that no root splits.
PENALTY = {
    (((37, 53), 8, 1, 1), 0): 196, (((37, 53), 8, 1, 1), 1): 2716,
    (((37, 53), 12, 1, 1), 0): 216, (((37, 53), 12, 1, 1), 1): 3034,
    (((48, 80), 16, 2, 1), 0): 526, (((48, 80), 16, 2, 1), 1): 88289,
    (((48, 80), 16, 0, 1), 0): 0, (((48, 80), 16, 0, 1), 1): 0,
    (((70, 101), 16, 2, 3), 0): 564, (((70, 101), 16, 2, 3), 1): 111439,
    (((70, 101), 32, 2, 1), 0): 1305, (((70, 101), 32, 2, 1), 1): 270114,
    (((70, 101), 24, 2, 1), 0): 1172, (((70, 101), 24, 2, 1), 1): 211585,
    (((70, 101), 24, 1, 1), 0): 318, (((70, 101), 24, 1, 1), 1): 4637,
    (((130, 135), 64, 2, 3), 0): 3239, (((130, 135), 64, 2, 3), 1): 569341,
    (((130, 135), 64, 1, 0), 0): 0, (((130, 135), 64, 1, 0), 1): 0,
}


def noise_pair(shape, block_size, depth, radius):
    """(previous, current, field) of a noise case; the same arrays on every call."""
    return _noise_pair(tuple(shape), block_size, depth, radius)


@functools.lru_cache(maxsize=None)
def _noise_pair(shape, block_size, depth, radius):
    rng = np.random.default_rng(1000 + 100 * block_size + 10 * depth + radius)
    frames = rng.integers(0, 256, size=(2,) + shape, dtype=np.uint8)
    mf = rng.integers(-FIELD_REACH, FIELD_REACH + 1, size=(shape[0] // block_size, shape[1] // block_size, 2)).astype(np.int32)
    for a in (frames, mf):
        a.setflags(write=False)
    return frames[0], frames[1], mf


@functools.lru_cache(maxsize=None)
def noise_result(case, pnorm):
    """vbs.tree of a noise case at its penalty, computed once -> (leaf, depth, cost)."""
    shape, bs, depth, radius = case
    previous, current, mf = noise_pair(*case)
    out = vbs.tree(previous, current, mf, bs, depth, radius, pnorm, PENALTY[case, pnorm])
    for a in out:
        a.setflags(write=False)
    return out


def whole_leaves(depth_map, D):
    """True iff a cell of depth d lies in a 2^(D-d) square of cells of depth d aligned to that size."""
    dm = np.asarray(depth_map)
    for d in range(D + 1):
        s = 1 << (D - d)
        blocks = (dm == d).reshape(dm.shape[0] // s, s, dm.shape[1] // s, s)
        count = blocks.sum(axis=(1, 3))
        if np.any((count != 0) & (count != s * s)):
            return False
    return bool(np.all(dm <= D))
