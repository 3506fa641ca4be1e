"""Result lifetimes of a resident sequence (include/gme_hip.h, "Result lifetimes"): the frames, the producers with their host
definitions, the readers, the events, and the table of what every reader returns after every event.  Shared by
test_lifetimes_host.py (coverage, discrimination, the table against the header) and test_gpu_lifetimes.py (the library against
the table).  Nothing here touches a device: every expected byte comes from the host definitions (subpel, hier, vbs, bipred, gmc,
propagate, direct, stabilize, mosaic, synth) and the C oracle."""
import functools
import hashlib
import os
import re

import numpy as np

import gmc_cases
import prop_cases
from helpers import c_oracle, np_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gme_hip.h")

# ---- frames ---------------------------------------------------------------------------------------------------------------------
N, H, W = prop_cases.SEQ_SHAPE                                   # uint8[5, 48, 80]
N_SHORT = 4                                                      # gme_seq_set_frames(4)
FD, BS, SW = 1, 8, prop_cases.SEQ_WINDOW                         # frame distance, block size, search window
SLOT = 2                                                         # the slot the one-slot upload replaces
SYNTH_SEED, SYNTH_T0 = 77, 3
# How SEED_B was chosen (find_seed_b below, on the CPU): the first seed from 49 on at which test_lifetimes_host.py's
# discrimination check holds -- every family's host result on stack B, on stack A with slot SLOT taken from B, and on the
# synthetic frames differs from its result on stack A.
SEED_B = 49


def _pan_stack(seed, reverse):
    """prop_cases.seq_frames()'s recipe: a pan of one pixel per frame over a noise canvas, fresh noise of +-6 on every frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H + 8, W + 8), dtype=np.uint8)
    cols = [N - 1 - k if reverse else k for k in range(N)]
    frames = np.stack([np.clip(base[4:-4, c:c + W].astype(np.int64) + rng.integers(-6, 7, size=(H, W)), 0, 255) for c in cols]).astype(np.uint8)
    frames = np.ascontiguousarray(frames)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def stack(name, seed_b=SEED_B):
    """The frame stacks by name: "A", "B", "A+B[slot]" (A with slot SLOT from B), "synth"."""
    if name == "A":
        return prop_cases.seq_frames()
    if name == "B":
        return _pan_stack(seed_b, True)
    if name == "A+B[slot]":
        f = stack("A").copy()
        f[SLOT] = stack("B", seed_b)[SLOT]
        f.setflags(write=False)
        return f
    if name == "synth":
        import synth
        f = synth.sequence(SYNTH_SEED, SYNTH_T0, N, H, W)
        f.setflags(write=False)
        return f
    raise KeyError(name)


# ---- arguments --------------------------------------------------------------------------------------------------------------------
# Two sets per call: [0] builds the full state, [1] is what the call uses as an event, so that "fresh" after an event on unchanged
# frames is told apart from "unchanged".
ARGS = {
    "bbme": ((FD, BS, SW, 3, 0), (FD, BS, SW, 0, 1)),                                  # fd, bs, window, procedure, pnorm
    "hier": ((FD, BS, SW, 1, 0, 2), (FD, BS, 2, 2, 1, 2)),                             # fd, bs, coarse window, radius, pnorm, levels
    "prop": ((FD, BS, 0, 2, 1, True), (FD, BS, 1, 1, 2, False)),                       # fd, bs, pnorm, rounds, steps, temporal
    "subpel": ((FD, BS, 0, 2), (FD, BS, 1, 1)),                                        # fd, bs, pnorm, levels
    "vbs": ((FD, BS, 1, 1, 0, 400), (FD, BS, 1, 2, 1, 900)),                           # fd, bs, depth, radius, pnorm, penalty
    # fd, bs, window, procedure, pnorm, radius, rounds, penalty; [2]: frame distance 2, the one family that needs N >= 2 fd + 1
    "bipred": ((1, BS, SW, 0, 0, 1, 1, 64), (1, BS, SW, 3, 1, 1, 2, 0), (2, BS, SW, 0, 0, 1, 1, 64)),
    "gmc": ((FD, BS, SW, 0, 0, 16), (FD, BS, SW, 3, 1, 64)),                           # fd, bs, window, procedure, pnorm, penalty
    "begin_fit": ((FD, BS, 0.3, 3, 2), (FD, BS, 0.25, 3, 3)),                          # fd, bs, outlier fraction, procedure, window
    "warp_frames": ((0, 7), (1, 0)),                                                   # border, fill
    "mosaic": ((0,), (9,)),                                                            # fill
    "moving_masks": ((16, 3), (8, 2)),                                                 # threshold, min_count
}
HIER_LEVELS = (1, 2)                                             # the levels both argument sets of "hier" use
FIT_LEVEL, FIT_FRACTION = 2, 0.3                                 # the reader gme_fit
MOSAIC_FRAMES = N_SHORT                                          # the mosaic and the masks cover frames [0, 4): valid at both counts
RANGE = (1, 3)                                                   # frames the warped-frame and mask readers read (first, count)
GMC_WARPS = (("rotzoom", "unusable", "fractional", "projective"), ("projective", "fractional", "identity", "rotzoom"))
PROJ_WARPS = (("fractional", "projective", "rotzoom", "integer"), ("integer", "rotzoom", "projective", "fractional"))


def named_warps(names, pairs):
    return np.stack([gmc_cases.warp_of(names[k % len(names)], H, W) for k in range(pairs)])


def _rows(seed, pairs, width, scale):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=(N, width))[:pairs] * np.asarray(scale)


def comp_params(v, pairs):
    """float64[pairs, 6] for gme_seq_compensate: shifts of up to two pixels, a small affine part."""
    return _rows(100 + v, pairs, 6, [2.0, 0.05, 0.05, 2.0, 0.05, 0.05])


def comp2_params(v, pairs):
    """float64[pairs, 12] for gme_seq_compensate2."""
    return _rows(200 + v, pairs, 12, [2.0, 0.05, 0.05, 2.0, 0.05, 0.05] + [0.01] * 6)


def fit_params(pairs):
    """float64[pairs, 6] the reader gme_fit hands to level 2."""
    return _rows(300, pairs, 6, [1.5, 0.02, 0.02, 1.5, 0.02, 0.02])


def frame_warps(v, count):
    """float64[count, 8] for gme_seq_warp_frames: fractional shifts (v 0), a slight projective warp on top (v 1)."""
    w = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0]), (count, 1))
    w[:, 2] = 0.5 * np.arange(count) + 0.25
    w[:, 5] = -0.75 * np.arange(count)
    if v:
        w[:, 0], w[:, 4], w[:, 6] = 0.99, 1.01, 1e-5
    return w


def mosaic_plan(v):
    """mosaic.plan of MOSAIC_FRAMES frames under a pan of one pixel per frame (v 0) or of -0.5, 0.25 (v 1)."""
    import mosaic
    pair = np.array([1.0, 0, 1.0, 0, 1.0, 0, 0, 0]) if v == 0 else np.array([1.0, 0, -0.5, 0, 1.0, 0.25, 0, 0])
    return mosaic.plan(np.tile(pair, (MOSAIC_FRAMES - 1, 1)), H, W)


# ---- host definitions -------------------------------------------------------------------------------------------------------------
_MEMO = {}


def _digest(parts):
    h = hashlib.sha1()
    for p in parts:
        if isinstance(p, np.ndarray):
            h.update(("%s%s" % (p.dtype, p.shape)).encode())
            h.update(np.ascontiguousarray(p).tobytes())
        else:
            h.update(repr(p).encode())
    return h.digest()


def _freeze(r):
    if isinstance(r, np.ndarray):
        r.setflags(write=False)
    elif isinstance(r, (tuple, list)):
        for a in r:
            _freeze(a)
    elif isinstance(r, dict):
        for a in r.values():
            _freeze(a)
    return r


def memo(fn):
    """Computed once per argument values (arrays by content): the tests share every host result and leave it unchanged."""
    @functools.wraps(fn)
    def wrapper(*args):
        key = _digest((fn.__module__, fn.__name__) + args)
        if key not in _MEMO:
            _MEMO[key] = _freeze(fn(*args))
        return _MEMO[key]
    return wrapper


def _sse(a, b):
    return c_oracle().sse(a, b)


def _pairs(frames, fd):
    return [(frames[k], frames[k + fd]) for k in range(len(frames) - fd)]


@memo
def host_bbme(frames, args):
    """The field of gme_seq_bbme: the C oracle, pair by pair -> int32[P, h, w, 2]."""
    fd, bs, sw, procedure, pnorm = args
    return np.stack([c_oracle().bbme(p, c, bs, sw, procedure, pnorm) for p, c in _pairs(frames, fd)])


@memo
def pyramids(frames):
    """[level 0, level 1, level 2] stacks of a frame stack (utils.get_pyramids through the C oracle)."""
    co = c_oracle()
    l1 = np.stack([co.pyrdown(f) for f in frames])
    l0 = np.stack([co.pyrdown(f) for f in l1])
    return [l0, l1, np.asarray(frames)]


@memo
def host_hier(frames, args):
    """hier.search -> ((field of level 1, of level 2), (cost of level 1, of level 2)), each stacked over the pairs."""
    import hier
    fd, bs, cw, radius, pnorm, levels = args
    pyr = pyramids(frames)
    res = [hier.search([l[k] for l in pyr], [l[k + fd] for l in pyr], bs, cw, radius, pnorm, levels) for k in range(len(frames) - fd)]
    return (tuple(np.stack([r[0][l] for r in res]) for l in HIER_LEVELS), tuple(np.stack([r[1][l] for r in res]) for l in HIER_LEVELS))


def prop_camera(v, pairs):
    return prop_cases.seq_camera(pairs, BS) if v == 0 else None


@memo
def host_prop(frames, prior, args, v):
    """propagate.search on the prior field, t = the prior field of the pair before -> (mf, cost, source)."""
    import propagate
    fd, bs, pnorm, rounds, steps, temporal = args
    g = prop_camera(v, len(frames) - fd)
    res = [propagate.search(p, c, prior[k], bs, pnorm, rounds, steps, prior[k - 1] if temporal and k else None, None if g is None else g[k])
           for k, (p, c) in enumerate(_pairs(frames, fd))]
    return tuple(np.stack([r[i] for r in res]) for i in range(3))


@memo
def host_subpel(frames, mv, args):
    """subpel.refine and subpel.compensate -> (qfield, cost, compensated planes, sse)."""
    import subpel
    fd, bs, pnorm, levels = args
    res = [subpel.refine(p, c, mv[k], bs, pnorm, levels) for k, (p, c) in enumerate(_pairs(frames, fd))]
    q, cost = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    planes = np.stack([subpel.compensate(p, q[k], bs) for k, (p, c) in enumerate(_pairs(frames, fd))])
    sse = np.array([_sse(c, planes[k]) for k, (p, c) in enumerate(_pairs(frames, fd))], np.int64)
    return q, cost, planes, sse


@memo
def host_vbs(frames, mv, args):
    """vbs.tree and the integer compensation at the leaf size -> (leaf, depth, cost, compensated planes, sse)."""
    import subpel
    import vbs
    fd, bs, depth, radius, pnorm, penalty = args
    res = [vbs.tree(p, c, mv[k], bs, depth, radius, pnorm, penalty) for k, (p, c) in enumerate(_pairs(frames, fd))]
    leaf, dmap, cost = (np.stack([r[i] for r in res]) for i in range(3))
    planes = np.stack([subpel.compensate_integer(p, leaf[k], bs >> depth) for k, (p, c) in enumerate(_pairs(frames, fd))])
    sse = np.array([_sse(c, planes[k]) for k, (p, c) in enumerate(_pairs(frames, fd))], np.int64)
    return leaf, dmap, cost, planes, sse


@memo
def host_bipred(frames, args):
    """Both searches (the C oracle, the target frame as the previous one), bipred.decide and bipred.predict ->
    (f0, f1, mode, v0, v1, cost, costs, predicted planes, sse) over the targets."""
    import bipred
    fd, bs, sw, procedure, pnorm, radius, rounds, penalty = args
    out = []
    for t in range(fd, len(frames) - fd):
        past, mid, nxt = frames[t - fd], frames[t], frames[t + fd]
        f0, f1 = c_oracle().bbme(mid, past, bs, sw, procedure, pnorm), c_oracle().bbme(mid, nxt, bs, sw, procedure, pnorm)
        mode, v0, v1, cost, costs = bipred.decide(past, mid, nxt, f0, f1, bs, radius, rounds, pnorm, penalty)
        pred = bipred.predict(past, nxt, mode, v0, v1, bs)
        out.append((f0, f1, mode, v0, v1, cost, costs, pred, np.int64(_sse(mid, pred))))
    return tuple(np.stack([r[i] for r in out]) for i in range(9))


@memo
def host_gmc(frames, args, v):
    """The search (the C oracle, the predicted frame as the previous one), gmc.decide and gmc.predict ->
    (f, mode, cost, costs, usable, predicted planes, sse) over the pairs."""
    import gmc
    fd, bs, sw, procedure, pnorm, penalty = args
    h = named_warps(GMC_WARPS[v], len(frames) - fd)
    out = []
    for k, (ref, cur) in enumerate(_pairs(frames, fd)):
        f = c_oracle().bbme(cur, ref, bs, sw, procedure, pnorm)
        mode, cost, costs = gmc.decide(ref, cur, h[k], f, bs, pnorm, penalty)
        pred = gmc.predict(ref, h[k], mode, f, bs)
        out.append((f, mode, cost, costs, np.uint8(gmc.usable(h[k], H, W)), pred, np.int64(_sse(cur, pred))))
    return tuple(np.stack([r[i] for r in out]) for i in range(7))


@memo
def host_staged(frames, args):
    """gme_seq_gme_begin_fit through the C oracle (helpers.oracle_gme's first stages) and the level-2 fit of fit_params ->
    dict of arrays stacked over the pairs."""
    fd, bs, frac, procedure, sw = args
    co, o = c_oracle(), np_oracle()
    pyr = pyramids(frames)
    fit = fit_params(len(frames) - fd)
    rows = []
    for k in range(len(frames) - fd):
        dense = co.bbme(pyr[0][k], pyr[0][k + fd], 2, 2, 3, 1)
        p0 = co.first_parameters(dense)
        gts = [co.bbme(pyr[lvl][k], pyr[lvl][k + fd], bs, sw, procedure, 1) for lvl in (1, 2)]
        st = [co.fit_level(gts[0], o.project_parameters(p0.copy()), frac, pyr[1][k].shape), co.fit_level(gts[1], fit[k], FIT_FRACTION, pyr[2][k].shape)]
        row = {"dense": dense, "p0": np.asarray(p0, np.float32)}
        for lvl, (s, gt) in enumerate(zip(st, gts), 1):
            row.update({"gt%d" % lvl: gt, "model%d" % lvl: s["model"], "mask%d" % lvl: s["mask"], "thr%d" % lvl: np.int64(s["thr"]),
                        "sums%d" % lvl: np.concatenate([s["F"].reshape(9), s["Sx"], s["Sy"]])})
        rows.append(row)
    return {name: np.stack([r[name] for r in rows]) for name in rows[0]}


def field2(params, h, w):
    """gme_hip.h: d = ((p0 + p2 j) + p1 i) + ((a3 (i i) + a4 (i j)) + a5 (j j)), round-half-even, int16 wrap."""
    p = np.asarray(params, np.float64)
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.empty((h, w, 2), np.int16)
    for c in range(2):
        q0, q1, q2, s0, s1, s2 = p[3 * c], p[3 * c + 1], p[3 * c + 2], p[6 + 3 * c], p[7 + 3 * c], p[8 + 3 * c]
        out[:, :, c] = np.rint(((q0 + q2 * j) + q1 * i) + ((s0 * (i * i) + s1 * (i * j)) + s2 * (j * j))).astype(np.int64).astype(np.int16)
    return out


@memo
def host_compensate(frames, order, v):
    """gme_seq_compensate (order 1) and gme_seq_compensate2 (order 2): the model field, the C oracle's compensation -> (planes, sse)."""
    co = c_oracle()
    pairs = len(frames) - FD
    params = comp_params(v, pairs) if order == 1 else comp2_params(v, pairs)
    planes = []
    for k, (p, c) in enumerate(_pairs(frames, FD)):
        field = co.affine_field(params[k], H // BS, W // BS) if order == 1 else field2(params[k], H // BS, W // BS)
        planes.append(co.compensate(p, field.astype(np.int32)))
    return np.stack(planes), np.array([_sse(c, planes[k]) for k, (p, c) in enumerate(_pairs(frames, FD))], np.int64)


@memo
def host_compensate_projective(frames, v):
    """direct.compensate -> (planes, sse)."""
    import direct
    h = named_warps(PROJ_WARPS[v], len(frames) - FD)
    res = [direct.compensate(p, c, h[k]) for k, (p, c) in enumerate(_pairs(frames, FD))]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int64)


@memo
def host_warp(frames, v):
    """stabilize.warp_frames of every frame -> (frames, valid)."""
    import stabilize
    border, fill = ARGS["warp_frames"][v]
    return stabilize.warp_frames(frames, frame_warps(v, len(frames)), ("constant", "replicate")[border], fill)


@memo
def host_mosaic(frames, v):
    """mosaic.build of frames [0, MOSAIC_FRAMES) -> (sprite, count)."""
    import mosaic
    return mosaic.build(frames[:MOSAIC_FRAMES], mosaic_plan(v), ARGS["mosaic"][v][0])


@memo
def host_masks(frames, sprite, count, plan_v, v):
    """mosaic.moving_masks of frames [0, MOSAIC_FRAMES) against a sprite built under mosaic_plan(plan_v) -> (masks, known, moving)."""
    import mosaic
    threshold, min_count = ARGS["moving_masks"][v]
    return mosaic.moving_masks(frames[:MOSAIC_FRAMES], mosaic_plan(plan_v), sprite, count, threshold, min_count)


# ---- readers, events, the table -----------------------------------------------------------------------------------------------------
REFUSES, UNCHANGED, FRESH = "refuses", "unchanged", "fresh"

# reader -> (family, the C calls it makes).  The readers that end in [..] are probes of one call.
READERS = {
    "read_frame": ("frames", ("gme_seq_read_frame",)),
    "read_mv": ("mv", ("gme_seq_read_mv",)),
    "read_qmv": ("qmv", ("gme_seq_read_qmv",)),
    "compensate_qpel": ("qmv", ("gme_seq_compensate_qpel",)),
    "read_hier[1]": ("hier", ("gme_seq_read_hier",)),
    "read_hier[2]": ("hier", ("gme_seq_read_hier",)),
    "read_vbs": ("vbs", ("gme_seq_read_vbs",)),
    "compensate_vbs": ("vbs", ("gme_seq_compensate_vbs",)),
    "read_bipred": ("bipred", ("gme_seq_read_bipred",)),
    "predict_bipred": ("bipred", ("gme_seq_predict_bipred",)),
    "read_gmc": ("gmc", ("gme_seq_read_gmc",)),
    "predict_gmc": ("gmc", ("gme_seq_predict_gmc",)),
    "read_prop": ("prop", ("gme_seq_read_prop",)),
    "read_stage": ("staged", ("gme_seq_gme_read_stage",)),
    "gme_fit": ("staged", ("gme_seq_gme_fit", "gme_seq_gme_read_stage")),
    "read_compensated[first]": ("comp", ("gme_seq_read_compensated",)),                # plane 0: every writer writes it
    "read_compensated[last]": ("comp_last", ("gme_seq_read_compensated",)),            # plane N - FD - 1: gme_seq_predict_bipred does not
    "read_compensated_range[written]": ("comp", ("gme_seq_read_compensated_range",)),  # the planes of the last writer
    "read_compensated_range[all]": ("comp_last", ("gme_seq_read_compensated_range",)),  # planes 0 .. N - FD - 1
    "compensate": ("frames", ("gme_seq_compensate",)),
    "compensate2": ("frames", ("gme_seq_compensate2",)),
    "compensate_projective": ("frames", ("gme_seq_compensate_projective",)),
    "read_warped_range": ("warped", ("gme_seq_read_warped_range",)),
    "read_mosaic": ("mosaic", ("gme_seq_read_mosaic",)),
    "read_masks_range": ("masks", ("gme_seq_read_masks_range",)),
}

# event -> the C call it makes
EVENTS = {
    "upload_all": "gme_seq_upload", "upload_one": "gme_seq_upload", "synth": "gme_seq_synth", "invalidate_pyramids": "gme_seq_invalidate",
    "set_frames_4": "gme_seq_set_frames", "set_frames_4_and_back": "gme_seq_set_frames", "bbme_streamed": "gme_seq_bbme_streamed",
    "bbme": "gme_seq_bbme", "hier": "gme_seq_hier", "prop": "gme_seq_prop", "subpel": "gme_seq_subpel", "vbs": "gme_seq_vbs",
    "bipred": "gme_seq_bipred", "gmc": "gme_seq_gmc", "gme_begin_fit": "gme_seq_gme_begin_fit",
    "compensate": "gme_seq_compensate", "compensate2": "gme_seq_compensate2", "compensate_projective": "gme_seq_compensate_projective",
    "compensate_qpel": "gme_seq_compensate_qpel", "compensate_vbs": "gme_seq_compensate_vbs", "predict_bipred": "gme_seq_predict_bipred",
    "predict_gmc": "gme_seq_predict_gmc",
    "warp_frames": "gme_seq_warp_frames", "mosaic": "gme_seq_mosaic", "moving_masks": "gme_seq_moving_masks",
}
# "New frame data" (gme_hip.h, Result lifetimes); the stack the sequence holds afterwards and how many of its frames are in use.
# invalidate_pyramids and set_frames_4_and_back leave the bytes of the frames as they were, and still end what new frame data ends.
FRAME_EVENTS = {
    "upload_all": ("B", N), "upload_one": ("A+B[slot]", N), "synth": ("synth", N), "invalidate_pyramids": ("A", N),
    "set_frames_4": ("A", N_SHORT), "set_frames_4_and_back": ("A", N), "bbme_streamed": ("B", N),
}
CHANGED_STACKS = ("B", "A+B[slot]", "synth")                     # the stacks of the events that change frame bytes
# the calls that write the compensated planes; readers too (they return a squared error).  gme_seq_predict_bipred writes
# N - 2 FD planes, one fewer than the others: it stands last so that the full state ends with an unwritten plane
COMP_WRITERS = ("compensate", "compensate2", "compensate_projective", "compensate_qpel", "compensate_vbs", "predict_gmc", "predict_bipred")

# The sentences of include/gme_hip.h the table is taken from (test_lifetimes_host.py checks that the header holds each, word for
# word).  Where no sentence names an event for a family, the family is UNCHANGED by it: "a call that a family's text does not
# name leaves that result readable and byte-identical".
Q_SILENT = "a call that a family's text does not name leaves that result readable and byte-identical"
Q_NEW_DATA = ("\"New frame data\" below is gme_seq_upload, gme_seq_synth, gme_seq_invalidate, a gme_seq_set_frames that changes the "
              "count, and the upload inside gme_seq_bbme_streamed.")
Q_MV = ("the motion field of gme_seq_read_mv survives new frame data: it is a prior (gme_seq_prop, gme_seq_vbs), replaced only by "
        "gme_seq_bbme, gme_seq_bbme_streamed, gme_seq_hier and gme_seq_prop;")
Q_QMV = ("the quarter-pel result ends with new frame data and with the next block-matching call (gme_seq_bbme, "
         "gme_seq_bbme_streamed, gme_seq_hier, gme_seq_prop), exactly where the hierarchical, variable-block-size and propagation "
         "results end;")
Q_QMV_READ = ("GME_ERR_STATE before any gme_seq_subpel, after new frame data or after the next block-matching call; "
              "gme_seq_compensate_qpel likewise.")
Q_HIER = "GME_ERR_STATE before any gme_seq_hier, after new frame data or after another block-matching call."
Q_HIER_MV = "The level-2 field becomes the sequence's motion field with this block size and frame distance, as after gme_seq_bbme:"
Q_VBS = "it is no longer valid after new frame data or the next block-matching call."
Q_VBS_MV = "does not replace the sequence's motion field;"
Q_BIPRED = "The result is kept in the sequence (allocated on first use) until new frame data."
Q_BIPRED_OTHERS = ("the sequence's motion field and the quarter-pel, hierarchical and variable-block-size results stay as they were.")
Q_GMC_OTHERS = ("the sequence's motion field and the quarter-pel, hierarchical, variable-block-size and bidirectional results stay as "
                "they were.")
Q_PROP = "GME_ERR_STATE before any gme_seq_prop, after new frame data or after another block-matching call."
Q_PROP_OTHERS = ("earlier quarter-pel, hierarchical and variable-block-size results are no longer valid, the bidirectional and "
                 "global-motion-compensation results stay.")
Q_STAGED = "ends a staged run: fit and the stage read-back then report GME_ERR_STATE until begin."
Q_SET_FRAMES = "Ends a staged GME run."
Q_COMP = ("each call writes planes 0 .. its own count - 1 and ends the planes of the call before it. They stay readable through new "
          "frame data.")
Q_COMP_READ = ("gme_seq_read_compensated(_range) of a range that holds a plane the last writer did not write, or before any writer, "
               "is GME_ERR_STATE.")
Q_KEPT = ("the warped frames, the mosaic and the masks are kept in the sequence through new frame data, until their own call writes "
          "them again.")
QUOTES = [v for k, v in sorted(globals().items()) if k.startswith("Q_")]

NEW_DATA = tuple(FRAME_EVENTS)
BLOCK_MATCHING = ("bbme", "bbme_streamed", "hier", "prop")


def _rule(refuses=(), fresh=()):
    out = {e: REFUSES for e in refuses}
    out.update({e: FRESH for e in fresh})
    return out


# family -> {event: outcome}; every event that is not named is UNCHANGED (Q_SILENT).
RULES = {
    # the frames: what gme_seq_read_frame and the three compensations with caller-given parameters see is always the frames the
    # sequence holds now (Q_NEW_DATA names the events that change them); these readers carry no state of their own
    "frames": _rule(fresh=tuple(EVENTS)),
    # Q_MV; Q_HIER_MV; gme_seq_prop: "The result becomes the sequence's motion field"
    "mv": _rule(fresh=BLOCK_MATCHING),
    # Q_QMV, Q_QMV_READ; gme_seq_subpel: "kept in the sequence"
    "qmv": _rule(refuses=NEW_DATA + BLOCK_MATCHING, fresh=("subpel",)),
    # Q_HIER; Q_BIPRED_OTHERS and Q_GMC_OTHERS keep it through gme_seq_bipred and gme_seq_gmc
    "hier": _rule(refuses=NEW_DATA + ("bbme", "prop"), fresh=("hier",)),
    # Q_VBS, Q_VBS_MV; Q_PROP_OTHERS
    "vbs": _rule(refuses=NEW_DATA + BLOCK_MATCHING, fresh=("vbs",)),
    # Q_BIPRED; Q_PROP_OTHERS and Q_GMC_OTHERS keep it through gme_seq_prop and gme_seq_gmc
    "bipred": _rule(refuses=NEW_DATA, fresh=("bipred",)),
    # gme_seq_gmc: "The result is kept in the sequence (allocated on first use) until new frame data." (Q_BIPRED's words); Q_PROP_OTHERS
    "gmc": _rule(refuses=NEW_DATA, fresh=("gmc",)),
    # Q_PROP
    "prop": _rule(refuses=NEW_DATA + ("bbme", "hier"), fresh=("prop",)),
    # Q_STAGED, Q_SET_FRAMES (and Q_NEW_DATA for the upload inside gme_seq_bbme_streamed)
    "staged": _rule(refuses=NEW_DATA, fresh=("gme_begin_fit",)),
    # Q_COMP: plane 0 and the planes of the last writer
    "comp": _rule(fresh=COMP_WRITERS),
    # Q_COMP, Q_COMP_READ: plane N - FD - 1, which gme_seq_predict_bipred (N - 2 FD planes) does not write
    "comp_last": _rule(refuses=("predict_bipred",), fresh=tuple(w for w in COMP_WRITERS if w != "predict_bipred")),
    # Q_KEPT
    "warped": _rule(fresh=("warp_frames",)),
    "mosaic": _rule(fresh=("mosaic",)),
    "masks": _rule(fresh=("moving_masks",)),
}


def outcome(event, reader):
    return RULES[READERS[reader][0]].get(event, UNCHANGED)


TABLE = {(e, r): outcome(e, r) for e in EVENTS for r in READERS}

# gme_seq_* declarations of the header that are neither a reader nor an event here, and why
EXCEPTIONS = {
    "gme_seq_create": "makes the sequence",
    "gme_seq_destroy": "frees the sequence",
    "gme_seq_set_split_phase": "a mode switch that holds no result; test_gpu_lifetimes.test_split_phase runs the frame events under it",
    "gme_seq_wait": "waits for the last split-phase call; holds no result",
    "gme_seq_poll": "asks whether gme_seq_wait would block; holds no result",
}


def header_text():
    """The header with comment decoration and line breaks collapsed into single spaces."""
    with open(HEADER) as f:
        text = f.read()
    return re.sub(r"\s+", " ", re.sub(r"\n\s*\*(?!/)", " ", text))


def header_declarations():
    """{name: (return type, [parameter text, ...])} of every gme_seq_* function include/gme_hip.h declares."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"GME_API\s+([\w\s]+?[\s\*]+)(gme_seq_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        out[m.group(2)] = (re.sub(r"\s+", " ", m.group(1)).strip(), [re.sub(r"\s+", " ", a).strip() for a in m.group(3).split(",")])
    return out


def has_output_pointer(params):
    """A parameter that is a pointer to something the call may write: not const, and not the sequence itself."""
    return any("*" in p and not p.startswith("const ") and not p.startswith("gme_seq ") for p in params)


# ---- the seed of stack B ------------------------------------------------------------------------------------------------------------
def family_results(frames):
    """name -> the host result of every family on a frame stack (argument set 0, the prior field that of gme_seq_bbme), as the
    tuple of arrays its readers return; what the discrimination check compares between stacks."""
    n = len(frames)
    mv = host_bbme(frames, ARGS["bbme"][0])
    hier_fields, hier_costs = host_hier(frames, ARGS["hier"][0])
    staged = host_staged(frames, ARGS["begin_fit"][0])
    sprite, count = host_mosaic(frames, 0)
    out = {
        "mv": (mv,),
        "qmv": host_subpel(frames, mv, ARGS["subpel"][0]),
        "hier[1]": (hier_fields[0], hier_costs[0]), "hier[2]": (hier_fields[1], hier_costs[1]),
        "vbs": host_vbs(frames, mv, ARGS["vbs"][0]),
        "bipred": host_bipred(frames, ARGS["bipred"][0]),
        "gmc": host_gmc(frames, ARGS["gmc"][0], 0),
        "prop": host_prop(frames, mv, ARGS["prop"][0], 0),
        "staged": tuple(staged[k] for k in sorted(staged)),
        "compensate": host_compensate(frames, 1, 0), "compensate2": host_compensate(frames, 2, 0),
        "compensate_projective": host_compensate_projective(frames, 0),
        "warped": (host_warp(frames, 0)[0][RANGE[0]:RANGE[0] + RANGE[1]],),
        "mosaic": (sprite, count),
        "masks": (host_masks(frames, sprite, count, 0, 0)[0][RANGE[0]:RANGE[0] + RANGE[1]],),
    }
    assert n == N
    return out


def same_arrays(a, b):
    return len(a) == len(b) and all(np.shape(x) == np.shape(y) and np.array_equal(x, y) for x, y in zip(a, b))


def writer_planes(frames):
    """writer -> the compensated planes it leaves on a stack in the full state (argument set 0)."""
    mv = host_bbme(frames, ARGS["bbme"][0])
    return {"compensate": host_compensate(frames, 1, 0)[0], "compensate2": host_compensate(frames, 2, 0)[0],
            "compensate_projective": host_compensate_projective(frames, 0)[0],
            "compensate_qpel": host_subpel(frames, mv, ARGS["subpel"][0])[2], "compensate_vbs": host_vbs(frames, mv, ARGS["vbs"][0])[3],
            "predict_bipred": host_bipred(frames, ARGS["bipred"][0])[7], "predict_gmc": host_gmc(frames, ARGS["gmc"][0], 0)[5]}


def discrimination_failures(seed_b=SEED_B):
    """What test_lifetimes_host.test_discrimination asserts to be empty: (stack, family) where the host result on a changed
    stack equals the one on stack A, and pairs of writers whose plane 0 or whose last common plane are equal on stack A."""
    base = family_results(stack("A"))
    bad = []
    for name in CHANGED_STACKS:
        other = family_results(stack(name, seed_b) if name != "synth" else stack(name))
        bad += [(name, fam) for fam in base if same_arrays(base[fam], other[fam])]
    planes = writer_planes(stack("A"))
    names = sorted(planes)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            last = min(len(planes[a]), len(planes[b])) - 1
            if np.array_equal(planes[a][0], planes[b][0]) or np.array_equal(planes[a][last], planes[b][last]):
                bad.append((a, b))
    return bad


def find_seed_b(start=49):
    """How SEED_B was chosen (CPU only, not run by the tests)."""
    seed = start
    while discrimination_failures(seed):
        seed += 1
    return seed
