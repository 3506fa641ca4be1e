"""Frames, fields, argument tables and host results of the block-size sweep over the seven one-wave-per-block passes (k_interp,
k_retime, k_bipred, k_gmc, k_prop, k_hier, k_vbs of csrc/bbme_wave_lds.h's scaffold): every side the argument rules admit in
4 .. 64, shared by tests/test_block_size_cases_host.py (CPU) and tests/test_gpu_block_sizes.py (GPU)."""
import functools

import numpy as np

import bipred
import gmc
import hier
import interp
import propagate
import retime
import vbs

PASSES = ("interp", "retime", "bipred", "gmc", "prop", "hier", "vbs")
NORMS = (0, 1)
ALL = range(4, 65)
# the sizes the CORNERS runs repeat at each pass's largest arguments: odd sides and the neighbours of the compiled instances for
# the passes that take any size; odd tops, leaves and children that start inside a dword for hier and vbs
CORNERS_ANY = (5, 7, 13, 15, 17, 31, 33, 47, 63)
CORNERS_TREE = (10, 14, 20, 28, 30, 34, 36, 44, 52, 60, 62)
FIELD_RANGE = 6
WARP = (1.0, 0.0, 2.5, 0.0, 1.0, 0.75, 0.0, 0.0)      # a quarter-pel translation whose every sample point lies inside the frame


def shape(B):
    """Two block rows of five blocks (the second workgroup of a block row has one working wave), one row and three columns
    beyond the last whole block; 129 x 323 at the largest side."""
    return 2 * B + 1, 5 * B + 3


# ---- content ----------------------------------------------------------------------------------------------------------------
def _content(B, s):
    """(frames uint8[3, H, W] of uniform noise, fields int32[2, 2, 5, 2] with components in [-6, 6])."""
    rng = np.random.default_rng([7700, B, s])
    frames = rng.integers(0, 256, size=(3,) + shape(B), dtype=np.uint8)
    fields = rng.integers(-FIELD_RANGE, FIELD_RANGE + 1, size=(2, 2, 5, 2)).astype(np.int32)
    return frames, fields


def inside_maps(B, fields):
    """bool[2, 2, 5]: per field, the blocks whose displaced block lies entirely in the frame."""
    H, W = shape(B)
    return np.array([[[vbs._inside(H, W, i * B, j * B, B, int(f[i, j, 0]), int(f[i, j, 1])) for j in range(5)] for i in range(2)]
                     for f in fields])


def field_condition(B, fields):
    """Each field has a displaced block inside the frame and one outside; one block has both inside, one both outside."""
    m = inside_maps(B, fields)
    return bool(m[0].any() and (~m[0]).any() and m[1].any() and (~m[1]).any() and (m[0] & m[1]).any() and (~m[0] & ~m[1]).any())


def find_seed(B):
    """How SEED was chosen: the first s of 0, 1, ... at which the field condition holds."""
    s = 0
    while not field_condition(B, _content(B, s)[1]):
        s += 1
    return s


# {B: s}; tests/test_block_size_cases_host.py checks that it equals what find_seed yields
SEED = {B: 1 if B in (10, 25, 42, 44) else 0 for B in ALL}


@functools.lru_cache(maxsize=None)
def content(B):
    """(f[0], f[1], f[2], field0, field1) of a size; the same read-only arrays on every call.  The passes take them as: interp
    and retime past f[0], next f[2], truth f[1]; bipred past, mid, next with field0 into past and field1 into next; gmc, prop,
    hier and vbs previous / ref f[0] and current f[1] with field0; prop's temporal field is field1 and its camera field
    camera_field(B)."""
    frames, fields = _content(B, SEED[B])
    frames.setflags(write=False)
    fields.setflags(write=False)
    return frames[0], frames[1], frames[2], fields[0], fields[1]


def camera_field(B):
    """prop's camera field: field1 turned by half a turn over the block grid (there are two fields per size, and a third
    candidate that repeated one of them could never win on its own)."""
    return np.ascontiguousarray(content(B)[4][::-1, ::-1])


# ---- argument tables --------------------------------------------------------------------------------------------------------
def max_levels(B):
    return 3 if B % 4 == 0 and B >= 16 else 2 if B % 2 == 0 and B >= 8 else 1


def max_depth(B):
    return max_levels(B) - 1


HIER_ALL = tuple(sorted({(B, max_levels(B)) for B in ALL} | {(B, 1) for B in ALL}))
VBS_ALL = tuple(sorted({(B, max_depth(B)) for B in ALL} | {(B, 0) for B in ALL}))
HIER_CORNERS = tuple((B, max_levels(B)) for B in CORNERS_TREE)
VBS_CORNERS = tuple((B, max_depth(B)) for B in CORNERS_TREE)

RETIME_PHASE = (2, 5)
RETIME_CORNER_PHASES = ((7, 12), (63, 64))


def second(name, B, pnorm):
    """The one bias or penalty other than 0 that a pass runs at: the tool's default for the size."""
    if name in ("interp", "retime"):
        return interp.default_bias(B, pnorm)
    return {"bipred": bipred, "gmc": gmc, "vbs": vbs}[name].default_penalty(B, pnorm)


def light(name, B, pnorm):
    """The argument tuples, without the size and the norm, of a pass's light runs (every size): the smallest windows.  For hier
    and vbs the tuple begins with the levels / depth, and every one of HIER_ALL / VBS_ALL of that size is run."""
    if name == "interp":
        return tuple((2, bias) for bias in (0, second(name, B, pnorm)))
    if name == "retime":
        return tuple((2, bias) + RETIME_PHASE for bias in (0, second(name, B, pnorm)))
    if name == "bipred":
        return tuple((1, 1, penalty) for penalty in (0, second(name, B, pnorm)))
    if name == "gmc":
        return ((0,),)
    if name == "prop":
        return ((2, 1, False), (2, 1, True))
    if name == "hier":
        return tuple((levels, 2, 1) for b, levels in HIER_ALL if b == B)
    if name == "vbs":
        return tuple((depth, 1, 0) for b, depth in VBS_ALL if b == B)
    raise KeyError(name)


def corner(name, B, pnorm):
    """The same at a pass's largest arguments (the sizes of CORNERS_ANY, or CORNERS_TREE for hier and vbs), at 0 and at the
    size's default bias / penalty."""
    both = (0, second(name, B, pnorm)) if name not in ("prop", "hier") else ()
    if name == "interp":
        return tuple((8, bias) for bias in both)
    if name == "retime":
        return tuple((16, bias) + phase for phase in RETIME_CORNER_PHASES for bias in both)
    if name == "bipred":
        return tuple((2, 2, penalty) for penalty in both)
    if name == "gmc":
        return tuple((penalty,) for penalty in both)
    if name == "prop":
        return ((4, 4, False), (4, 4, True))
    if name == "hier":
        return ((max_levels(B), 8, 3),)
    if name == "vbs":
        return tuple((max_depth(B), 3, penalty) for penalty in both)
    raise KeyError(name)


def sizes(name, which):
    """The sizes of a pass's sweep, ``which`` "all" or "corners"."""
    if which == "all":
        return tuple(ALL)
    return CORNERS_TREE if name in ("hier", "vbs") else CORNERS_ANY


def runs(name, which):
    """Every (B, pnorm, args) of a pass's sweep."""
    table = light if which == "all" else corner
    return [(B, pnorm, args) for B in sizes(name, which) for pnorm in NORMS for args in table(name, B, pnorm)]


def plan(name, B, args):
    """The kernel instance that serves a run: the compiled one at 16 and 32 (hier at three levels also at 64, vbs at depth 2
    only), the run-time one everywhere else."""
    if name == "hier":
        return "k_hier<%d,3>" % B if args[0] == 3 and B in (16, 32, 64) else "k_hier<0,0>"
    if name == "vbs":
        return "k_vbs<%d,2>" % B if args[0] == 2 and B in (16, 32) else "k_vbs<0,0>"
    return "k_%s<%d>" % (name, B if B in (16, 32) else 0)


# ---- host results -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _retime_distortions(B, sw, n, d):
    """retime.block_distortions of a size: the part of its search that depends on neither the norm nor the bias."""
    f0, _, f2, _, _ = content(B)
    return retime.block_distortions(f0, f2, B, sw, n, d)


def _frozen(out):
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def want(name, B, pnorm, args):
    """The host definition's result of one run, in the order the device's one-shot entry point returns it, computed once:
    interp, retime (mv, cost, dist, frame, sse); bipred (mode, v0, v1, cost, costs, predicted, sse); gmc (mode, cost, costs,
    predicted, sse); prop (mf, cost, source); vbs (leaf, depth, cost).  hier has no entry here: its definition runs on the
    device's own pyramids (hier_want)."""
    f0, f1, f2, fa, fb = content(B)
    if name == "interp":
        sw, bias = args
        out = interp.search(f0, f2, B, sw, pnorm, bias)
        made = interp.interpolate(f0, f2, out[0], B)
        return _frozen(out + (made, interp.sse(made, f1)))
    if name == "retime":
        sw, bias, n, d = args
        retime.check_args(B, sw, pnorm, bias)
        out = retime.select(_retime_distortions(B, sw, n, d)[pnorm], sw, bias)
        made = retime.interpolate(f0, f2, out[0], B, n, d)
        return _frozen(out + (made, interp.sse(made, f1)))
    if name == "bipred":
        r, rounds, penalty = args
        out = bipred.decide(f0, f1, f2, fa, fb, B, r, rounds, pnorm, penalty)
        pred = bipred.predict(f0, f2, out[0], out[1], out[2], B)
        return _frozen(out + (pred, bipred.sse(f1, pred)))
    if name == "gmc":
        out = gmc.decide(f0, f1, np.array(WARP), fa, B, pnorm, args[0])
        pred = gmc.predict(f0, np.array(WARP), out[0], fa, B)
        return _frozen(out + (pred, gmc.sse(f1, pred)))
    if name == "prop":
        rounds, steps, extra = args
        return _frozen(propagate.search(f0, f1, fa, B, pnorm, rounds, steps, fb if extra else None, camera_field(B) if extra else None))
    if name == "vbs":
        depth, r, penalty = args
        return _frozen(vbs.tree(f0, f1, fa, B, depth, r, pnorm, penalty))
    raise KeyError(name)


def hier_want(prev_pyr, cur_pyr, B, pnorm, args):
    """hier.search on the given pyramids -> (field, cost) of level 2, as gme_hier_u8 returns them, plus the per-level dicts."""
    levels, cw, r = args
    fields, costs = hier.search(prev_pyr, cur_pyr, B, cw, r, pnorm, levels)
    return fields[2], costs[2], fields, costs


def host_pyramid(frame):
    """[level0, level1, frame] by the 2 x 2 rounded mean with replicated edges: a pyramid for the host test only, where what
    matters is that hier's search has something to find, not how the levels were made."""
    levels = [np.asarray(frame)]
    for _ in range(2):
        p = levels[0].astype(np.int64)
        p = np.pad(p, ((0, p.shape[0] % 2), (0, p.shape[1] % 2)), mode="edge")
        levels.insert(0, ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return levels
