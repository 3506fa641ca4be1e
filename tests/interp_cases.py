"""Frames and host results shared by the frame-interpolation tests (host and GPU)."""
import functools

import numpy as np

import interp
import vbs_cases

# ---- the pan scene ----------------------------------------------------------------------------------------------------------
# checked on the CPU with the committed definition: at the seeds 1 .. 3 all 35 blocks carry PAN_MOVE in both norms and the
# interpolation beats the plain average by more than 15 dB; the first is taken
PAN_SEED = 1
PAN_SHAPE, PAN_BLOCK, PAN_WINDOW, PAN_MARGIN = (80, 112), 16, 6, 8
PAN_MOVE = (3, -2)                                               # (columns, rows) the content moves per frame
PAN_NOISE = 4


@functools.lru_cache(maxsize=None)
def pan_scene(seed=PAN_SEED):
    """(past, middle, next): a pan of PAN_MOVE per frame over a canvas, independent uniform noise of +-PAN_NOISE grey levels on
    every frame."""
    (H, W), m = PAN_SHAPE, PAN_MARGIN
    c = vbs_cases.canvas(seed, H + 2 * m, W + 2 * m)
    rng = np.random.default_rng(seed + 2000)
    out = []
    for t in (-1, 0, 1):
        vx, vy = t * PAN_MOVE[0], t * PAN_MOVE[1]
        f = c[m - vy:m - vy + H, m - vx:m - vx + W].astype(np.int64)
        f = np.clip(f + rng.integers(-PAN_NOISE, PAN_NOISE + 1, size=(H, W)), 0, 255).astype(np.uint8)
        f.setflags(write=False)
        out.append(f)
    return tuple(out)


# ---- stripes ----------------------------------------------------------------------------------------------------------------
STRIPES_SHAPE, STRIPES_BLOCK, STRIPES_WINDOW = (37, 53), 8, 8


@functools.lru_cache(maxsize=None)
def stripes():
    """(past, next): vertical stripes of period 8 (four columns of 40, four of 200) moving one column per frame, two frames
    apart."""
    H, W = STRIPES_SHAPE
    x = np.arange(W + 2)
    row = np.where((x % 8) < 4, 40, 200).astype(np.uint8)
    past = np.ascontiguousarray(np.tile(row[2:2 + W], (H, 1)))
    nxt = np.ascontiguousarray(np.tile(row[0:W], (H, 1)))
    for f in (past, nxt):
        f.setflags(write=False)
    return past, nxt


# ---- noise ------------------------------------------------------------------------------------------------------------------
# (shape, block_size, search_window): frame sizes that are no multiple of the block (48 x 80 at 16 is), the compiled instances
# (16 and 32) and the run-time one, rows of 12 and 24 bytes, no search at window 0, the largest windows (80 x 80 at 64 and 8),
# a single block whose every window pixel beyond it is clamped, the smallest block there is, and rows of 6 and 10 bytes, whose
# last dword holds bytes beyond the block
NOISE = (((37, 53), 8, 3), ((37, 53), 12, 5), ((48, 80), 16, 8), ((48, 80), 16, 0), ((70, 101), 32, 4), ((70, 101), 24, 8),
         ((130, 135), 64, 8), ((16, 16), 16, 8), ((4, 4), 4, 1), ((37, 53), 6, 3), ((37, 53), 10, 5))


def noise_biases(case, pnorm):
    """The biases a noise case runs at: none, and the tool's default for its block size."""
    return (0, interp.default_bias(case[1], pnorm))


@functools.lru_cache(maxsize=None)
def noise_pair(case):
    """(past, middle, next) of a noise case; the same arrays on every call."""
    frames = np.random.default_rng(3000 + NOISE.index(case)).integers(0, 256, size=(3,) + tuple(case[0]), dtype=np.uint8)
    frames.setflags(write=False)
    return frames[0], frames[1], frames[2]


@functools.lru_cache(maxsize=None)
def result(name, pnorm, bias):
    """(mv, cost, dist, frame) of a named pair on the host, computed once: ``name`` is "pan", "stripes" or a case of NOISE."""
    if name == "pan":
        past, nxt, bs, sw = pan_scene()[0], pan_scene()[2], PAN_BLOCK, PAN_WINDOW
    elif name == "stripes":
        past, nxt, bs, sw = stripes() + (STRIPES_BLOCK, STRIPES_WINDOW)
    else:
        past, nxt, bs, sw = noise_pair(name)[0], noise_pair(name)[2], name[1], name[2]
    out = interp.search(past, nxt, bs, sw, pnorm, bias)
    out = out + (interp.interpolate(past, nxt, out[0], bs),)
    for a in out:
        a.setflags(write=False)
    return out
