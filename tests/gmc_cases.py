"""Frames, warps and fields shared by the global-motion-compensation tests (host and GPU)."""
import functools
import math

import numpy as np

import direct
import gmc
import vbs_cases

# ---- the zoom scene -----------------------------------------------------------------------------------------------------------
# checked on the CPU: the seeds 1 .. 4 all meet check_scene's conditions in both norms; the first is taken
SCENE_SEED = 1
SCENE_SHAPE, SCENE_MARGIN, SCENE_BLOCK, SCENE_WINDOW = (96, 128), 16, 16, 8
SCENE_PATCH = (32, 48, 32)                                       # first row, first column in `ref`, side
SCENE_MOVE = (5, -3)                                             # the patch in `cur`: 5 columns right, 3 rows up
SCENE_NOISE = 4
SCENE_ANGLE, SCENE_ZOOM = 1.5, 1.02
SCENE_MODES = np.array([[1, 1, 0, 0, 0, 0, 0, 0],
                        [0, 0, 0, 0, 0, 0, 0, 0],
                        [0, 0, 0, 1, 1, 0, 0, 0],
                        [0, 0, 0, 1, 1, 0, 0, 0],
                        [0, 0, 0, 0, 0, 0, 0, 0],
                        [0, 0, 0, 0, 0, 0, 1, 1]], np.uint8)


def rotation_zoom(H, W, degrees, zoom):
    """The warp that turns by ``degrees`` and divides by ``zoom`` about the centre of an H x W frame."""
    a = math.radians(degrees)
    c, s = math.cos(a) / zoom, math.sin(a) / zoom
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    return np.array([c, -s, cx - c * cx + s * cy, s, c, cy - s * cx - c * cy, 0.0, 0.0])


@functools.lru_cache(maxsize=None)
def zoom_scene(seed=SCENE_SEED):
    """(ref, cur, h): a camera that turns and zooms over a canvas, a patch of another canvas that moves by SCENE_MOVE on its
    own, and independent uniform noise of +-SCENE_NOISE grey levels on both frames."""
    (H, W), m = SCENE_SHAPE, SCENE_MARGIN
    top, left, side = SCENE_PATCH
    big = vbs_cases.canvas(seed, H + 2 * m, W + 2 * m)
    patch = vbs_cases.canvas(seed + 1000, side, side)
    h = rotation_zoom(H, W, SCENE_ANGLE, SCENE_ZOOM)
    ref = big[m:m + H, m:m + W].astype(np.int64)
    ref[top:top + side, left:left + side] = patch
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    up, vp, _ = direct.warp(h, u, v)
    cur = np.floor(direct.bilinear(big, up + m, vp + m) + 0.5).astype(np.int64)
    top, left = top + SCENE_MOVE[1], left + SCENE_MOVE[0]
    cur[top:top + side, left:left + side] = patch
    rng = np.random.default_rng(seed + 2000)
    out = []
    for f in (ref, cur):
        f = np.clip(f + rng.integers(-SCENE_NOISE, SCENE_NOISE + 1, size=(H, W)), 0, 255).astype(np.uint8)
        f.setflags(write=False)
        out.append(f)
    h.setflags(write=False)
    return out[0], out[1], h


@functools.lru_cache(maxsize=None)
def scene_result(pnorm, seed=SCENE_SEED):
    """(f, mode, cost, costs) of the scene on the host at the default penalty, computed once."""
    ref, cur, h = zoom_scene(seed)
    f = vbs_cases.exhaustive(cur, ref, SCENE_BLOCK, SCENE_WINDOW, pnorm)
    out = (f,) + gmc.decide(ref, cur, h, f, SCENE_BLOCK, pnorm, gmc.default_penalty(SCENE_BLOCK, pnorm))
    for a in out:
        a.setflags(write=False)
    return out


def check_scene(f, mode, costs):
    """The conditions of the scene: the mode map is SCENE_MODES; its four local blocks of the corner rows are exactly the blocks
    without a global candidate; the four patch blocks carry the patch's vector."""
    assert np.array_equal(mode, SCENE_MODES), mode
    none = costs[:, :, 0] == -1
    want = np.zeros(mode.shape, bool)
    want[0, :2] = want[-1, -2:] = True
    assert np.array_equal(none, want), none
    assert np.all(f[2:4, 3:5] == (-SCENE_MOVE[0], -SCENE_MOVE[1])), f[2:4, 3:5]


# ---- noise ----------------------------------------------------------------------------------------------------------------------
# (shape, block_size): frame sizes that are no multiple of the block (48 x 80 at 16 is), the compiled instances (16 and 32) and the
# run-time one, rows of 12 and 24 bytes, and rows of 10 and 6 bytes, whose last dword holds bytes beyond the block
NOISE = (((37, 53), 8), ((37, 53), 12), ((48, 80), 16), ((70, 101), 16), ((70, 101), 24), ((70, 101), 32), ((130, 135), 64),
         ((37, 53), 10), ((37, 53), 6))
FIELD_REACH = 6                                                  # the random input vectors lie in [-6, 6]: some point outside
COPY_NOISE = 2

WARPS = ("identity", "integer", "fractional", "rotzoom", "projective", "far", "unusable", "nan")
# Which modes the host must produce per warp.  The warps of FULL have blocks with and without a global candidate (each makes
# pixel (0, 0) sample outside the frame), so all three modes must occur.  The identity gives every block a global candidate, so
# mode 2 cannot occur; under the last three no block has one, so mode 0 cannot.
FULL = ("integer", "fractional", "rotzoom", "projective")


def warp_of(name, H, W):
    """float64[8] of a named warp for an H x W frame."""
    if name == "identity":                                       # u' = W - 1 on the last column: the clamped far tap
        return direct.IDENTITY.copy()
    if name == "integer":
        return np.array([1.0, 0.0, -3.0, 0.0, 1.0, 2.0, 0.0, 0.0])
    if name == "fractional":
        return np.array([1.0, 0.0, -2.25, 0.0, 1.0, 1.5, 0.0, 0.0])
    if name == "rotzoom":                                        # zooming in keeps the far corners inside; the shift puts (0, 0) outside
        h = rotation_zoom(H, W, 1.0, 1.0 / 1.02)
        h[2] -= 1.5
        h[5] -= 1.0
        return h
    if name == "projective":
        return np.array([0.99, 0.004, -1.5, -0.003, 0.985, 0.75, 1e-5, -1e-5])
    if name == "far":                                            # every sample outside
        return np.array([1.0, 0.0, 2.0 * W, 0.0, 1.0, 0.0, 0.0, 0.0])
    if name == "unusable":                                       # d = 1 - 2 u / (W - 1) <= 0 at the right corners
        return np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -2.0 / (W - 1), 0.0])
    if name == "nan":
        return np.array([1.0, 0.0, float("nan"), 0.0, 1.0, 0.0, 0.0, 0.0])
    raise KeyError(name)


# Seed per case, chosen on the CPU (find_seed below): the first seed from 3000 + 1000 * (index of the case) on at which the host's
# modes hold what required_modes asks under every warp in both norms at the default penalty.
SEED = {NOISE[0]: 3000, NOISE[1]: 4000, NOISE[2]: 5000, NOISE[3]: 6000, NOISE[4]: 7000, NOISE[5]: 8002, NOISE[6]: 9000,
        NOISE[7]: 10000, NOISE[8]: 11000}


def required_modes(name):
    if name in FULL:
        return {0, 1, 2}
    return {0, 1} if name == "identity" else None                # None: no mode 0, see check_modes


def check_modes(name, mode):
    got = set(np.unique(mode).tolist())
    want = required_modes(name)
    if want is None:
        assert got <= {1, 2} and 1 in got, (name, got)
    else:
        assert got == want, (name, got)


def _inside_mask(f, H, W, bs):
    y0, x0 = np.arange(H // bs)[:, None] * bs, np.arange(W // bs)[None, :] * bs
    return (x0 + f[:, :, 0] >= 0) & (y0 + f[:, :, 1] >= 0) & (x0 + f[:, :, 0] + bs <= W) & (y0 + f[:, :, 1] + bs <= H)


def _noise_pair(case, seed):
    (H, W), bs = case
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(2, H, W), dtype=np.uint8)
    ref, cur = frames[0], frames[1].copy()
    f = rng.integers(-FIELD_REACH, FIELD_REACH + 1, size=(H // bs, W // bs, 2)).astype(np.int32)
    # on pure noise the bilinear predictor averages noise and would win every block: a random half of the blocks whose vector
    # points inside is the ref block at f, with noise of +-COPY_NOISE
    copy = _inside_mask(f, H, W, bs) & (rng.random(f.shape[:2]) < 0.5)
    for i, j in np.argwhere(copy):
        y, x = i * bs, j * bs
        blk = ref[y + f[i, j, 1]:y + f[i, j, 1] + bs, x + f[i, j, 0]:x + f[i, j, 0] + bs].astype(np.int64)
        cur[y:y + bs, x:x + bs] = np.clip(blk + rng.integers(-COPY_NOISE, COPY_NOISE + 1, size=(bs, bs)), 0, 255)
    for a in (ref, cur, f):
        a.setflags(write=False)
    return ref, cur, f


@functools.lru_cache(maxsize=None)
def noise_pair(case):
    """(ref, cur, f) of a noise case; the same arrays on every call."""
    return _noise_pair(case, SEED[case])


def _noise_field(case, name, pair):
    (H, W), bs = case
    ref, cur, f = pair
    h = warp_of(name, H, W)
    exists = gmc.global_pixels(ref, h)[1]
    f = f.copy()
    # the first block without a global candidate gets a vector that points outside, so that mode 2 occurs
    for i in range(H // bs):
        for j in range(W // bs):
            if not exists[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs].all():
                f[i, j] = (-W, 0)
                f.setflags(write=False)
                return h, f
    f.setflags(write=False)
    return h, f


@functools.lru_cache(maxsize=None)
def noise_field(case, name):
    """(h, f) of a noise case under a named warp."""
    return _noise_field(case, name, noise_pair(case))


@functools.lru_cache(maxsize=None)
def noise_result(case, name, pnorm):
    """gmc.decide of a noise case under a named warp at the default penalty, computed once -> (mode, cost, costs)."""
    ref, cur, _ = noise_pair(case)
    h, f = noise_field(case, name)
    out = gmc.decide(ref, cur, h, f, case[1], pnorm, gmc.default_penalty(case[1], pnorm))
    for a in out:
        a.setflags(write=False)
    return out


def find_seed(case, start):
    """How SEED was chosen (CPU only, not run by the tests)."""
    seed = start
    while True:
        pair = _noise_pair(case, seed)
        try:
            for name in WARPS:
                h, f = _noise_field(case, name, pair)
                for pnorm in (0, 1):
                    check_modes(name, gmc.decide(pair[0], pair[1], h, f, case[1], pnorm, gmc.default_penalty(case[1], pnorm))[0])
            return seed
        except AssertionError:
            seed += 1


# ---- ties and saturated content ---------------------------------------------------------------------------------------------------
def ties_frames():
    """Constant frames: every candidate of a block costs the same."""
    return np.full((37, 53), 90, np.uint8), np.full((37, 53), 97, np.uint8)
