"""Frames and host results shared by the frame-retiming tests (host and GPU)."""
import functools

import numpy as np

import interp_cases
import retime

# ---- the pan scene ----------------------------------------------------------------------------------------------------------
# Noise cut from a larger field, so that every frame of the pan is exact: `next` is `past` moved by PAN_MOVE, and the true frame
# at phase n / d is `past` moved by PAN_MOVE n / d, a whole number of pixels at every phase of PAN_PHASES.
PAN_SHAPE, PAN_BLOCK, PAN_WINDOW, PAN_MARGIN, PAN_BIAS = (80, 112), 16, 16, 16, 16
PAN_MOVE = (12, -6)                                              # (columns, rows) the content moves from past to next
PAN_PHASES = ((1, 2), (1, 3), (2, 3), (5, 6))
PAN_INTERIOR = (slice(16, 64), slice(16, 96))                    # the rows and columns of the blocks that never clamp


@functools.lru_cache(maxsize=None)
def pan_field():
    (H, W), m = PAN_SHAPE, PAN_MARGIN
    f = np.random.default_rng(4100).integers(0, 256, size=(H + 2 * m, W + 2 * m), dtype=np.uint8)
    f.setflags(write=False)
    return f


def pan_frame(n, d):
    """The frame of the pan at phase n / d (0 / 1: past, 1 / 1: next); PAN_MOVE n / d must be whole."""
    (H, W), m = PAN_SHAPE, PAN_MARGIN
    assert PAN_MOVE[0] * n % d == 0 and PAN_MOVE[1] * n % d == 0
    vx, vy = PAN_MOVE[0] * n // d, PAN_MOVE[1] * n // d
    f = np.ascontiguousarray(pan_field()[m - vy:m - vy + H, m - vx:m - vx + W])
    f.setflags(write=False)
    return f


# ---- stripes, constant and saturated frames -----------------------------------------------------------------------------------
STRIPES_BLOCK, STRIPES_WINDOW, STRIPES_PHASE = 8, 16, (1, 2)
stripes = interp_cases.stripes            # content moves two columns from past to next, period 8: V = 2 + 8 k ties, any Vy


def flat(value, shape=(37, 53)):
    return np.full(shape, value, np.uint8)


# ---- noise ------------------------------------------------------------------------------------------------------------------
# (H, W, block_size, search_window): one block whose every window pixel beyond it is clamped, run-time block sizes with rows that
# are no multiple of four bytes, both compiled instances, ragged edges, the largest window, and window 0
SHAPES = ((16, 16, 16, 16), (37, 53, 4, 1), (37, 53, 6, 5), (40, 72, 8, 3), (37, 53, 12, 16), (48, 64, 16, 16), (33, 70, 32, 7),
          (130, 135, 64, 16), (37, 53, 16, 0))
ALL_PHASES = ((1, 2), (1, 3), (2, 3), (2, 5), (7, 12), (1, 64), (63, 64))
# every shape with 1/2 and an odd denominator; the two shapes at the largest window with all seven: 1/64 and 63/64 leave
# the fewest classes for that window and make the two windows most lopsided
PHASES = {(16, 16, 16, 16): ((1, 2), (1, 3), (63, 64)), (37, 53, 4, 1): ((1, 2), (2, 5)), (37, 53, 6, 5): ((1, 2), (2, 3), (7, 12)),
          (40, 72, 8, 3): ((1, 2), (2, 5), (1, 64)), (37, 53, 12, 16): ((1, 2), (1, 3), (7, 12)), (48, 64, 16, 16): ALL_PHASES,
          (33, 70, 32, 7): ((1, 2), (2, 5), (63, 64)), (130, 135, 64, 16): ALL_PHASES, (37, 53, 16, 0): ((1, 2), (1, 3))}
NOISE = tuple((shape, phase) for shape in SHAPES for phase in PHASES[shape])


def noise_id(case):
    (H, W, bs, sw), (n, d) = case
    return "%dx%d-b%d-w%d-%d/%d" % (H, W, bs, sw, n, d)


def noise_biases(shape, pnorm):
    """The biases a noise shape runs at: none, and the tool's default for its block size."""
    return (0, retime.default_bias(shape[2], pnorm))


@functools.lru_cache(maxsize=None)
def noise_pair(shape):
    """(past, truth, next) of a noise shape; the same arrays on every call."""
    frames = np.random.default_rng(4000 + SHAPES.index(shape)).integers(0, 256, size=(3,) + tuple(shape[:2]), dtype=np.uint8)
    frames.setflags(write=False)
    return frames[0], frames[1], frames[2]


@functools.lru_cache(maxsize=None)
def noise_distortions(case):
    """retime.block_distortions of a noise case, computed once for both norms and every bias."""
    shape, (n, d) = case
    past, _, nxt = noise_pair(shape)
    out = retime.block_distortions(past, nxt, shape[2], shape[3], n, d)
    for a in out:
        a.setflags(write=False)
    return out


def noise_result(case, pnorm, bias):
    """(mv, cost, dist, frame) of a noise case on the host: retime.select of its distortions (what retime.search does), then
    retime.interpolate."""
    shape, (n, d) = case
    past, _, nxt = noise_pair(shape)
    out = retime.select(noise_distortions(case)[pnorm], shape[3], bias)
    return out + (retime.interpolate(past, nxt, out[0], shape[2], n, d),)


def host_result(past, nxt, bs, sw, pnorm, bias, n, d):
    """(mv, cost, dist, frame) of any pair on the host."""
    out = retime.search(past, nxt, bs, sw, pnorm, bias, n, d)
    return out + (retime.interpolate(past, nxt, out[0], bs, n, d),)


@functools.lru_cache(maxsize=None)
def pan_result(phase, pnorm):
    out = host_result(pan_frame(0, 1), pan_frame(1, 1), PAN_BLOCK, PAN_WINDOW, pnorm, PAN_BIAS, *phase)
    for a in out:
        a.setflags(write=False)
    return out


# ---- a clip -----------------------------------------------------------------------------------------------------------------
CLIP_SHAPE, CLIP_BLOCK, CLIP_WINDOW, CLIP_BIAS = (7, 40, 72), 8, 3, 4
CLIP_STEPS = ((2, 5), (1, 4), (5, 2), (1, 1))


@functools.lru_cache(maxsize=None)
def clip():
    frames = np.random.default_rng(4200).integers(0, 256, size=CLIP_SHAPE, dtype=np.uint8)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def clip_result(step, pnorm=0):
    """(frames, mv, cost, dist) of every output of the clip at a step, on the host under retime.schedule."""
    f = clip()
    rows = retime.schedule(len(f), *step)
    H, W = f.shape[1:]
    h, w = H // CLIP_BLOCK, W // CLIP_BLOCK
    made = np.zeros((len(rows), H, W), np.uint8)
    mv, cost, dist = np.zeros((len(rows), h, w, 2), np.int32), np.zeros((len(rows), h, w), np.int64), np.zeros((len(rows), h, w), np.int64)
    for m, (k, n, d) in enumerate(rows):
        if n == 0:
            made[m] = f[k]
        else:
            mv[m], cost[m], dist[m], made[m] = host_result(f[k], f[k + 1], CLIP_BLOCK, CLIP_WINDOW, pnorm, CLIP_BIAS, n, d)
    for a in (made, mv, cost, dist):
        a.setflags(write=False)
    return made, mv, cost, dist
