"""One resident sequence asked for changing sizes: the frames, the demands, the steps and what every step returns by its
definition.  Shared by test_reuse_host.py (coverage of the header, rise and fall of every result's size, discrimination between
demands, the two oracles) and test_gpu_reuse.py (the library, one long-lived sequence per test, against these expectations).

A demand is (frames in use, frame distance, block size, search); a step is one producer with all its readers, run(seq, demand)
-> dict of arrays on a sequence and host(frames, demand) -> the same dict from the definitions: the C oracle for block
matching, subpel / hier / vbs / propagate / bipred / gmc / interp / obmc / denoise / stabilize / direct / mosaic for the passes,
the NumPy restatements of the fit stages (helpers.stage_np, helpers.field2_np).  Nothing here touches a device by itself: run()
only uses the sequence it is handed."""
import collections

import numpy as np

import gmc_cases
import lifetime_cases as lc
from helpers import c_oracle, clear_of_ties2, contract_violations2, field2_np, mv_summary_rows, np_oracle, stage_np
from lifetime_cases import memo

# ---- frames ---------------------------------------------------------------------------------------------------------------------
N, H, W = 7, 80, 112             # W is no multiple of 64 (uploads are staged); level 1 = 40 x 56, level 0 = 20 x 28
SEED_A = 48
# How SEED_B was chosen (find_seed_b below, on the CPU): the first seed from 49 on at which test_reuse_host.py's discrimination
# check holds -- every step's expectation differs between any two different entries of the schedule.
SEED_B = 49


def _pan_stack(seed, reverse):
    """prop_cases.seq_frames()'s recipe at 7 x 80 x 112: a pan of one pixel per frame over a noise canvas, fresh noise of +-6 on
    every frame."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H + 8, W + 8), dtype=np.uint8)
    cols = [N - 1 - k if reverse else k for k in range(N)]
    frames = np.stack([np.clip(base[4:-4, c:c + W].astype(np.int64) + rng.integers(-6, 7, size=(H, W)), 0, 255) for c in cols]).astype(np.uint8)
    frames = np.ascontiguousarray(frames)
    frames.setflags(write=False)
    return frames


_STACKS = {}


def stack(name, seed_b=SEED_B):
    """"A": the pan to the left; "B": another canvas under the opposite pan, the stack the uploads bring."""
    key = (name, seed_b if name == "B" else SEED_A)
    if key not in _STACKS:
        _STACKS[key] = _pan_stack(key[1], name == "B")
    return _STACKS[key]


# ---- demands --------------------------------------------------------------------------------------------------------------------
# v numbers the demand: the caller-given parameters of a step (warps, model parameters, penalties, ...) are taken from it, so
# that two demands of one shape still ask for different bytes
Demand = collections.namedtuple("Demand", "name n fd bs sw proc norm v")
EXHAUSTIVE, DIAMOND, MAE, MSE = 0, 3, 0, 1
S = Demand("S", 5, 2, 16, 8, EXHAUSTIVE, MSE, 0)       # 3 pairs of 5 x 7 blocks; the matrix-core kernel, signed box sums
L = Demand("L", 7, 1, 8, 3, EXHAUSTIVE, MAE, 1)        # 6 pairs of 10 x 14 blocks
M = Demand("M", 7, 1, 16, 32, EXHAUSTIVE, MSE, 2)      # 6 pairs of 5 x 7 blocks; the elimination kernel, plain box sums
MD = Demand("Md", 7, 1, 16, 32, DIAMOND, MSE, 3)       # M's shapes under the diamond search
S7 = S._replace(name="S7", n=7)                         # S on all seven frames: beside M, the other table kind at the same frame count
SCHEDULE = (S, L, S, M, MD)
STACKS = ("A", "A", "A", "B", "B")                     # the second stack is uploaded between the third and the fourth demand
EQUAL_SHAPES = (3, 4)                                  # the adjacent pair with equal shapes and different search kernels
# what gme_last_bbme_info names after gme_seq_bbme at each demand (the kernel the demand is named for)
PLAN = {"S": "k_exh_mfma16", "S7": "k_exh_mfma16", "L": "k_exh_generic", "M": "k_exh_sea16_mse", "Md": "k_walk16"}


def pairs(d):
    return d.n - d.fd


def search(d):
    return (d.fd, d.bs, d.sw, d.proc, d.norm)


def staged_search(d):
    """(procedure, window) of the staged estimate's level searches: the demand's, the window capped at 8 (level 1 is 40 x 56)."""
    return d.proc, min(d.sw, 8)


# ---- caller-given parameters ------------------------------------------------------------------------------------------------------
def _rows(seed, count, scale):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=(N, len(scale)))[:count] * np.asarray(scale)


AFFINE_SCALE = [2.0, 0.03, 0.03, 2.0, 0.03, 0.03]


def affine_rows(d, salt=0):
    return _rows(1000 + 10 * d.v + salt, pairs(d), AFFINE_SCALE)


def order2_rows(d, salt=0):
    return _rows(2000 + 10 * d.v + salt, pairs(d), AFFINE_SCALE + [2e-3] * 6)


WARP_NAMES = ("rotzoom", "fractional", "projective", "integer", "identity", "unusable")


def named_warps(d, count, salt=0):
    return np.stack([gmc_cases.warp_of(WARP_NAMES[(k + d.v + salt) % len(WARP_NAMES)], H, W) for k in range(count)])


def usable_warps(d, count):
    """Warps whose denominators stay positive (direct_eval, compensate_projective, refine_projective's start)."""
    names = ("fractional", "projective", "rotzoom", "integer")
    return np.stack([gmc_cases.warp_of(names[(k + d.v) % 4], H, W) for k in range(count)])


def frame_warps(d):
    w = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0]), (d.n, 1))
    w[:, 2] = 0.5 * np.arange(d.n) + 0.25 * (d.v + 1)
    w[:, 5] = -0.75 * np.arange(d.n) + d.v
    if d.v & 1:
        w[:, 0], w[:, 4], w[:, 6] = 0.99, 1.01, 1e-5
    return w


def fill_candidates(d):
    """(sources int32[n, 3], warps float64[n, 3, 8]): frame t shifted out of itself by a few pixels, then its two neighbours
    (the second one absent on every other frame)."""
    src = np.empty((d.n, 3), np.int32)
    w = np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0]), (d.n, 3, 1))
    for t in range(d.n):
        src[t] = (t, (t + 1) % d.n, -1 if t & 1 else (t + d.n - 1) % d.n)
        w[t, 0, [2, 5]] = (3.5 + d.v, -2.25 - t)
        w[t, 1, [2, 5]] = (2.5 + d.v, 6.0)
        w[t, 2, [2, 5]] = (-30.0, -1.25 - t)
    return src, w


def mosaic_plan(d):
    """mosaic.plan of the demand's frames under a pan that depends on the demand: the canvas changes size with it."""
    import mosaic
    v = min(d.v, 2)                                              # M and Md share a canvas: they differ in fill and thresholds
    pair = np.array([1.0, 0, 1.0 + 0.5 * v, 0, 1.0, 0.25 * v, 0, 0])
    return mosaic.plan(np.tile(pair, (d.n - 1, 1)), H, W)


def camera_field(d):
    g = np.zeros((pairs(d), H // d.bs, W // d.bs, 2), np.int32)
    for k in range(pairs(d)):
        g[k, :, :] = (-d.fd - (k & 1) + (d.v & 1), k & 1)
    return g


def hier_args(d):
    return (d.fd, d.bs, (8, 3, 8, 4)[d.v], 1 + (d.v & 1), d.norm, 3 if d.bs == 16 else 2)     # fd, bs, coarse window, radius, pnorm, levels


def vbs_args(d):
    return (d.fd, d.bs, 2 if d.bs == 16 else 1, 1 + (d.v & 1), d.norm, 300 + 200 * d.v)       # fd, bs, depth, radius, pnorm, penalty


def bipred_args(d):
    return search(d) + (1 + (d.v & 1), 1 + (d.v >> 1), 32 * d.v)                              # ..., radius, rounds, penalty


def gmc_args(d):
    return search(d) + (16 + 24 * d.v,)                                                        # ..., penalty


def prop_args(d):
    return (d.fd, d.bs, d.norm, 1 + (d.v & 1), 1 + (d.v >> 1), True)                            # fd, bs, pnorm, rounds, steps, temporal


def subpel_args(d):
    return (d.fd, d.bs, d.norm, 2 - (d.v & 1))                                                 # fd, bs, pnorm, levels


def interp_args(d):
    return (d.fd, d.bs, min(d.sw, 8), d.norm, 4 * d.v)                                         # fd, bs, window, pnorm, bias


DENOISE_MODES = {"denoise_r1": (1, 0), "denoise_r2": (2, 2)}                                   # (radius, levels)


def denoise_args(d, mode):
    """fd, bs, window, procedure, pnorm, radius, levels, strength.  Radius 2 needs 4 fd + 1 frames: it runs at frame distance 1."""
    radius, levels = DENOISE_MODES[mode]
    return (d.fd if radius == 1 else 1, d.bs, d.sw, d.proc, d.norm, radius, levels, 16 + 4 * d.v)


def fraction(d):
    return (0.3, 0.25)[d.v & 1]


# The second-order model of gme_seq_gme_device_solve2 per demand.  At block size 16 level 1 has 2 x 3 blocks: the quadratic model
# is singular there (S: the host raises, the device must flag every pair), the other two are not.
MODEL_OF = {"S": "quadratic", "S7": "quadratic", "L": "quadratic", "M": "bilinear", "Md": "pseudo_perspective"}


# ---- host definitions -------------------------------------------------------------------------------------------------------------
def _pairs_of(frames, fd):
    return [(frames[k], frames[k + fd]) for k in range(len(frames) - fd)]


def _sse(a, b):
    return c_oracle().sse(a, b)


def _stage(st, gt):
    return {"gt": gt, "model": st["model"], "mask": st["mask"], "thr": np.int64(st["thr"])}


def _sums15(st):
    return np.concatenate([st["F"].reshape(9), st["Sx"], st["Sy"]])


def _stack_rows(rows):
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


@memo
def host_bbme(frames, d):
    co = c_oracle()
    mv = lc.host_bbme(frames, search(d))
    p = affine_rows(d)
    st = [co.fit_level(mv[k], p[k], fraction(d), (H, W)) for k in range(len(mv))]
    out = {"mv": mv, "summary": mv_summary_rows(mv), "fit": np.stack([_sums15(s) for s in st])}
    out.update({"stage_" + k: v for k, v in _stage(st[-1], mv[-1]).items()})
    return out


@memo
def host_bbme_streamed(frames, d):
    mv = lc.host_bbme(frames, search(d))
    return {"out": mv, "mv": mv}


@memo
def host_subpel(frames, d):
    q, cost, planes, sse = lc.host_subpel(frames, lc.host_bbme(frames, search(d)), subpel_args(d))
    return {"qmv": q, "cost": cost, "sse": sse, "planes": planes}


@memo
def host_hier(frames, d):
    import hier
    fd, bs, cw, radius, pnorm, levels = hier_args(d)
    pyr = lc.pyramids(frames)
    res = [hier.search([l[k] for l in pyr], [l[k + fd] for l in pyr], bs, cw, radius, pnorm, levels) for k in range(len(frames) - fd)]
    out = {"mv": np.stack([r[0][2] for r in res])}
    for lvl in range(3 - levels, 3):
        out["field%d" % lvl] = np.stack([r[0][lvl] for r in res])
        out["cost%d" % lvl] = np.stack([r[1][lvl] for r in res])
    return out


@memo
def host_vbs(frames, d):
    leaf, dmap, cost, planes, sse = lc.host_vbs(frames, lc.host_bbme(frames, search(d)), vbs_args(d))
    return {"leaf": leaf, "depth": dmap, "cost": cost, "sse": sse, "planes": planes}


@memo
def host_prop(frames, d):
    import propagate
    fd, bs, pnorm, rounds, steps, temporal = prop_args(d)
    prior, g = lc.host_bbme(frames, search(d)), camera_field(d)
    res = [propagate.search(p, c, prior[k], bs, pnorm, rounds, steps, prior[k - 1] if temporal and k else None, g[k])
           for k, (p, c) in enumerate(_pairs_of(frames, fd))]
    mf, cost, source = (np.stack([r[i] for r in res]) for i in range(3))
    return {"mf": mf, "cost": cost, "source": source, "mv": mf}


@memo
def host_bipred(frames, d):
    r = lc.host_bipred(frames, bipred_args(d))
    out = dict(zip(("f0", "f1", "mode", "v0", "v1", "cost", "costs", "planes", "sse"), r))
    return out


@memo
def host_gmc(frames, d):
    import gmc
    fd, bs, sw, procedure, pnorm, penalty = gmc_args(d)
    h = named_warps(d, len(frames) - fd)
    rows = []
    for k, (ref, cur) in enumerate(_pairs_of(frames, fd)):
        f = c_oracle().bbme(cur, ref, bs, sw, procedure, pnorm)
        mode, cost, costs = gmc.decide(ref, cur, h[k], f, bs, pnorm, penalty)
        pred = gmc.predict(ref, h[k], mode, f, bs)
        rows.append({"f": f, "mode": mode, "cost": cost, "costs": costs, "usable": np.uint8(gmc.usable(h[k], H, W)), "planes": pred,
                     "sse": np.int64(_sse(cur, pred))})
    return _stack_rows(rows)


@memo
def host_interp(frames, d):
    import interp
    fd, bs, sw, pnorm, bias = interp_args(d)
    rows = []
    for k, (past, nxt) in enumerate(_pairs_of(frames, fd)):
        mv, cost, dist = interp.search(past, nxt, bs, sw, pnorm, bias)
        made = interp.interpolate(past, nxt, mv, bs)
        rows.append({"mv": mv, "cost": cost, "dist": dist, "frames": made,
                     "sse": np.int64(interp.sse(made, frames[k + fd // 2]) if fd % 2 == 0 else -1)})
    return _stack_rows(rows)


@memo
def host_obmc(frames, d):
    import obmc
    mv = lc.host_bbme(frames, search(d))
    q = lc.host_subpel(frames, mv, subpel_args(d))[0]
    out = {}
    for name, field, quarter in (("unit4", mv, False), ("unit1", q, True)):
        made = np.stack([obmc.compensate(p, field[k], d.bs, quarter) for k, (p, c) in enumerate(_pairs_of(frames, d.fd))])
        out[name + "_frames"] = made
        out[name + "_sse"] = np.array([obmc.sse(made[k], c) for k, (p, c) in enumerate(_pairs_of(frames, d.fd))], np.int64)
    return out


def _host_denoise(frames, d, mode):
    import denoise
    import subpel
    fd, bs, sw, procedure, pnorm, radius, levels, strength = denoise_args(d, mode)
    made = []
    for t in range(radius * fd, len(frames) - radius * fd):
        refs = denoise.references(t, len(frames), fd, radius)
        assert len(refs) == 2 * radius
        fields = []
        for k in refs:
            mf = c_oracle().bbme(frames[t], frames[k], bs, sw, procedure, pnorm)
            fields.append(subpel.refine(frames[t], frames[k], mf, bs, pnorm, levels)[0] if levels else mf)
        made.append(denoise.frame(frames[t], [frames[k] for k in refs], fields, bs, levels > 0, strength))
    made = np.stack(made)
    targets = frames[radius * fd:len(frames) - radius * fd]
    return {"frames": made, "change": np.array([denoise.sse(m, t) for m, t in zip(made, targets)], np.int64)}


@memo
def host_denoise_r1(frames, d):
    return _host_denoise(frames, d, "denoise_r1")


@memo
def host_denoise_r2(frames, d):
    return _host_denoise(frames, d, "denoise_r2")


@memo
def _level_fields(frames, d):
    """Per pair: the dense field, the first parameters and the level-1 and level-2 fields of the staged estimate."""
    co = c_oracle()
    pyr = lc.pyramids(frames)
    procedure, sw = staged_search(d)
    rows = []
    for k in range(len(frames) - d.fd):
        dense = co.bbme(pyr[0][k], pyr[0][k + d.fd], 2, 2, 3, 1)
        rows.append({"dense": dense, "p0": np.asarray(co.first_parameters(dense), np.float32),
                     "gt1": co.bbme(pyr[1][k], pyr[1][k + d.fd], d.bs, sw, procedure, 1),
                     "gt2": co.bbme(pyr[2][k], pyr[2][k + d.fd], d.bs, sw, procedure, 1)})
    return _stack_rows(rows)


LEVEL1 = ((H + 1) // 2, (W + 1) // 2)


@memo
def host_staged(frames, d):
    """gme_begin_fit, gme_fit(2), gme_begin_fit2 and gme_fit2(2) with every stage read-back."""
    co, o = c_oracle(), np_oracle()
    lf = _level_fields(frames, d)
    fit1, fit2, frac = affine_rows(d, 1), order2_rows(d, 2), fraction(d)
    rows = []
    for k in range(len(lf["dense"])):
        gt1, gt2 = lf["gt1"][k], lf["gt2"][k]
        s1 = co.fit_level(gt1, o.project_parameters(lf["p0"][k].copy()), frac, LEVEL1)
        s2 = co.fit_level(gt2, fit1[k], frac, (H, W))
        row = {"p0": lf["p0"][k], "dense": lf["dense"][k], "sums1": _sums15(s1), "sums2": _sums15(s2)}
        row.update({"l1_" + n: v for n, v in _stage(s1, gt1).items()})
        row.update({"l2_" + n: v for n, v in _stage(s2, gt2).items()})
        # order 2: level 1 is the projected translation's field, mask and threshold with the 27 sums; level 2 the order-2 field
        thr, mask, sums = stage_np(gt1, s1["model"], frac, LEVEL1)
        assert thr == s1["thr"] and np.array_equal(mask, s1["mask"])
        model = field2_np(fit2[k], *gt2.shape[:2])
        thr2, mask2, sums2 = stage_np(gt2, model, frac, (H, W))
        row.update({"o2_sums1": sums, "o2_sums2": sums2, "o2_l2_gt": gt2, "o2_l2_model": model, "o2_l2_mask": mask2, "o2_l2_thr": np.int64(thr2)})
        rows.append(row)
    return _stack_rows(rows)


def _solved(sums, model):
    import roadmap
    try:
        p = roadmap.solve_model(np.asarray(sums)[None], model)[0]
    except np.linalg.LinAlgError:
        return None
    return p if np.all(np.isfinite(p)) else None


def _host_solve(frames, d, model):
    """The staged path of the device solves (include/gme_hip.h): begin_fit -> solve -> project -> fit(2) -> solve -> compensate
    -> {"gt": the level-2 fields, which no solve touches, "pairs": per pair the path's results, or None for a pair whose system
    the host cannot solve (the device must flag it)}."""
    import roadmap
    co, o = c_oracle(), np_oracle()
    lf = _level_fields(frames, d)
    frac = fraction(d)
    h, w = H // d.bs, W // d.bs
    out = []
    for k in range(len(lf["dense"])):
        gt1, gt2 = lf["gt1"][k], lf["gt2"][k]
        s1 = co.fit_level(gt1, o.project_parameters(lf["p0"][k].copy()), frac, LEVEL1)
        sums1 = _sums15(s1) if model == "affine" else stage_np(gt1, s1["model"], frac, LEVEL1)[2]
        p1 = _solved(sums1, model)
        if p1 is None:
            out.append(None)
            continue
        p1 = roadmap.project(p1[None])[0]
        if model == "affine":
            s2 = co.fit_level(gt2, p1, frac, (H, W))
            model2, mask2, thr2, sums2 = s2["model"], s2["mask"], s2["thr"], _sums15(s2)
        else:
            model2 = field2_np(p1, *gt2.shape[:2])
            thr2, mask2, sums2 = stage_np(gt2, model2, frac, (H, W))
        p2 = _solved(sums2, model)
        if p2 is None:
            out.append(None)
            continue
        field = co.affine_field(p2, h, w) if model == "affine" else field2_np(p2, h, w)
        comp = co.compensate(frames[k], field.astype(np.int32))
        out.append({"params": p2, "p1": p1, "model": model2, "mask": mask2, "thr": np.int64(thr2), "comp": comp, "sse": np.int64(_sse(frames[k + d.fd], comp))})
    return {"gt": lf["gt2"], "pairs": out}


@memo
def host_solve(frames, d):
    return _host_solve(frames, d, "affine")


@memo
def host_solve2(frames, d):
    return _host_solve(frames, d, MODEL_OF[d.name])


@memo
def host_models(frames, d):
    """compensate and compensate2."""
    co = c_oracle()
    P, h, w = len(frames) - d.fd, H // d.bs, W // d.bs
    p6, p12 = affine_rows(d, 3), order2_rows(d, 4)
    out = {}
    for name, fields in (("c1", [co.affine_field(p6[k], h, w) for k in range(P)]), ("c2", [field2_np(p12[k], h, w) for k in range(P)])):
        planes = np.stack([co.compensate(p, fields[k].astype(np.int32)) for k, (p, c) in enumerate(_pairs_of(frames, d.fd))])
        out[name + "_planes"] = planes
        out[name + "_sse"] = np.array([_sse(c, planes[k]) for k, (p, c) in enumerate(_pairs_of(frames, d.fd))], np.int64)
    return out


@memo
def host_direct(frames, d):
    """compensate_projective, direct_eval and refine_projective."""
    import direct
    P = len(frames) - d.fd
    warps = usable_warps(d, P)
    out = {}
    res = [direct.compensate(p, c, warps[k]) for k, (p, c) in enumerate(_pairs_of(frames, d.fd))]
    out["cp_planes"], out["cp_sse"] = np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int64)
    pyr = lc.pyramids(frames)
    level = d.v % 3
    at_level = np.stack([direct.projective_to_level(wk, level) for wk in warps])
    out["eval"] = [direct.evaluate(pyr[level][k], pyr[level][k + d.fd], at_level[k], fraction(d)) for k in range(P)]
    out["refine"] = [direct.refine([l[k] for l in pyr], [l[k + d.fd] for l in pyr], warps[k], fraction(d), 3 + d.v) for k in range(P)]
    return out


@memo
def host_warp_frames(frames, d):
    import stabilize
    made, valid = stabilize.warp_frames(frames, frame_warps(d), ("constant", "replicate")[d.v & 1], 7 * d.v)
    def sse(f):
        return np.array([_sse(f[k + 1], f[k]) for k in range(len(f) - 1)], np.int64)
    return {"valid": valid, "warped": made, "sse_warped": sse(made), "sse_frames": sse(frames)}


@memo
def host_warp_fill(frames, d):
    import stabilize
    src, w = fill_candidates(d)
    made, who, valid, filled, sse = stabilize.warp_fill(frames, src, w, ("constant", "replicate")[d.v & 1], 11 * d.v)
    return {"frames": made, "source": who, "valid": valid, "filled": filled, "sse": np.asarray(sse, np.int64)}


@memo
def host_mosaic(frames, d):
    import mosaic
    pl = mosaic_plan(d)
    sprite, count = mosaic.build(frames, pl, 9 * d.v)
    masks, known, moving = mosaic.moving_masks(frames, pl, sprite, count, 16 - 2 * d.v, 2 + (d.v & 1))
    return {"sprite": sprite, "count": count, "known": known, "moving": moving, "masks": masks}


# ---- the steps on a sequence ------------------------------------------------------------------------------------------------------
def _nothing():
    pass


def _stage_dict(prefix, st):
    return {prefix + "gt": st["gt"], prefix + "model": st["model"], prefix + "mask": st["mask"], prefix + "thr": np.int64(st["thr"])}


def run_bbme(seq, d, wait=_nothing):
    seq.bbme(*search(d))
    out = {"mv": seq.read_mv(), "summary": seq.mv_summary()}
    fit = seq.gme_fit(-1, affine_rows(d), fraction(d))
    wait()
    out["fit"] = np.array(fit)
    out.update(_stage_dict("stage_", seq.gme_read_stage(-1, pairs(d) - 1)))
    return out


def run_bbme_streamed(seq, d, wait=_nothing, frames=None):
    out = np.array(seq.bbme_streamed(frames[:d.n], *search(d), chunk_frames=2))
    return {"out": out, "mv": seq.read_mv()}


def run_subpel(seq, d, wait=_nothing):
    seq.bbme(*search(d))
    seq.subpel(*subpel_args(d))
    q, cost = seq.read_qmv()
    sse = np.array(seq.compensate_qpel(d.fd, d.bs))
    return {"qmv": q, "cost": cost, "sse": sse, "planes": seq.read_compensated_range(0, pairs(d))}


def run_hier(seq, d, wait=_nothing):
    a = hier_args(d)
    seq.hier(*a)
    out = {"mv": seq.read_mv()}
    for lvl in range(3 - a[5], 3):
        out["field%d" % lvl], out["cost%d" % lvl] = seq.read_hier(lvl)
    return out


def run_vbs(seq, d, wait=_nothing):
    seq.bbme(*search(d))
    seq.vbs(*vbs_args(d))
    leaf, dmap, cost = seq.read_vbs()
    sse = np.array(seq.compensate_vbs(d.fd, d.bs))
    return {"leaf": leaf, "depth": dmap, "cost": cost, "sse": sse, "planes": seq.read_compensated_range(0, pairs(d))}


def run_prop(seq, d, wait=_nothing):
    seq.bbme(*search(d))
    seq.prop(*prop_args(d), camera_field(d))
    mf, cost, source = seq.read_prop()
    return {"mf": mf, "cost": cost, "source": source, "mv": seq.read_mv()}


def run_bipred(seq, d, wait=_nothing):
    seq.bipred(*bipred_args(d))
    out = dict(zip(("f0", "f1", "mode", "v0", "v1", "cost", "costs"), seq.read_bipred()))
    out["sse"] = np.array(seq.predict_bipred())
    out["planes"] = seq.read_compensated_range(0, d.n - 2 * d.fd)
    return out


def run_gmc(seq, d, wait=_nothing):
    a = gmc_args(d)
    seq.gmc(a[0], named_warps(d, pairs(d)), *a[1:])
    out = dict(zip(("f", "mode", "cost", "costs", "usable"), seq.read_gmc()))
    out["sse"] = np.array(seq.predict_gmc())
    out["planes"] = seq.read_compensated_range(0, pairs(d))
    return out


def run_interp(seq, d, wait=_nothing):
    return dict(zip(("mv", "cost", "dist", "frames", "sse"), seq.interp(*interp_args(d))))


def run_obmc(seq, d, wait=_nothing):
    seq.bbme(*search(d))
    seq.subpel(*subpel_args(d))
    out = {}
    for name, quarter in (("unit4", False), ("unit1", True)):
        out[name + "_frames"], out[name + "_sse"] = seq.obmc(d.fd, d.bs, quarter)
    return out


def _run_denoise(seq, d, mode):
    fd, bs, sw, procedure, pnorm, radius, levels, strength = denoise_args(d, mode)
    made, change = seq.denoise(fd, bs, sw, procedure, pnorm, radius, levels, strength)
    return {"frames": made, "change": change}


def run_denoise_r1(seq, d, wait=_nothing):
    return _run_denoise(seq, d, "denoise_r1")


def run_denoise_r2(seq, d, wait=_nothing):
    return _run_denoise(seq, d, "denoise_r2")


def _stages(seq, level, count, prefix):
    rows = [seq.gme_read_stage(level, p) for p in range(count)]
    return {prefix + k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def run_staged(seq, d, wait=_nothing):
    procedure, sw = staged_search(d)
    P = pairs(d)
    p0, sums1 = seq.gme_begin_fit(d.fd, d.bs, fraction(d), procedure, sw)
    wait()
    out = {"p0": np.array(p0), "sums1": np.array(sums1), "dense": _stages(seq, 0, P, "")["gt"]}
    out.update(_stages(seq, 1, P, "l1_"))
    sums2 = seq.gme_fit(2, affine_rows(d, 1), fraction(d))
    wait()
    out["sums2"] = np.array(sums2)
    out.update(_stages(seq, 2, P, "l2_"))
    q0, sums = seq.gme_begin_fit2(d.fd, d.bs, fraction(d), procedure, sw)
    wait()
    out["o2_p0"], out["o2_sums1"] = np.array(q0), np.array(sums)
    out.update(_stages(seq, 1, P, "o2_l1_"))
    sums = seq.gme_fit2(2, order2_rows(d, 2), fraction(d))
    wait()
    out["o2_sums2"] = np.array(sums)
    out.update(_stages(seq, 2, P, "o2_l2_"))
    return out


def _run_solve(seq, d, wait, model):
    procedure, sw = staged_search(d)
    if model == "affine":
        got = seq.gme_device_solve(d.fd, d.bs, fraction(d), procedure, sw)
    else:
        got = seq.gme_device_solve2(model, d.fd, d.bs, fraction(d), procedure, sw)
    wait()
    out = dict(zip(("params", "sse", "flags"), (np.array(a) for a in got)))
    out.update(_stages(seq, 2, pairs(d), ""))
    out["comp"] = seq.read_compensated_range(0, pairs(d))
    return out


def run_solve(seq, d, wait=_nothing):
    return _run_solve(seq, d, wait, "affine")


def run_solve2(seq, d, wait=_nothing):
    return _run_solve(seq, d, wait, MODEL_OF[d.name])


def run_models(seq, d, wait=_nothing):
    P = pairs(d)
    out = {}
    sse = seq.compensate(d.fd, d.bs, affine_rows(d, 3))
    wait()
    out["c1_sse"], out["c1_planes"] = np.array(sse), seq.read_compensated_range(0, P)
    sse = seq.compensate2(d.fd, d.bs, order2_rows(d, 4))
    wait()
    out["c2_sse"], out["c2_planes"] = np.array(sse), seq.read_compensated_range(0, P)
    return out


def run_direct(seq, d, wait=_nothing):
    import direct
    P = pairs(d)
    out = {}
    warps = usable_warps(d, P)
    out["cp_sse"] = np.array(seq.compensate_projective(d.fd, warps))
    out["cp_planes"] = np.stack([seq.read_compensated(k) for k in range(P)])
    level = d.v % 3
    out["eval"] = seq.direct_eval(d.fd, level, np.stack([direct.projective_to_level(w, level) for w in warps]), fraction(d))
    out["refine"] = seq.refine_projective(d.fd, warps, fraction(d), 3 + d.v)
    return out


def run_warp_frames(seq, d, wait=_nothing):
    valid = seq.warp_frames(0, frame_warps(d), d.v & 1, 7 * d.v)
    return {"valid": valid, "warped": seq.read_warped_range(0, d.n), "sse_warped": seq.frame_sse(1, 0, d.n - 1),
            "sse_frames": seq.frame_sse(0, 0, d.n - 1)}


def run_warp_fill(seq, d, wait=_nothing):
    src, w = fill_candidates(d)
    return dict(zip(("frames", "source", "valid", "filled", "sse"), seq.warp_fill(0, src, w, d.v & 1, 11 * d.v, want_source=True)))


def run_mosaic(seq, d, wait=_nothing):
    pl = mosaic_plan(d)
    usable = np.asarray(pl["flags"]) == 0
    seq.mosaic(0, pl["G"], usable, pl["ox"], pl["oy"], pl["Hc"], pl["Wc"], 9 * d.v, True)
    sprite, count = seq.read_mosaic()
    known, moving = seq.moving_masks(0, pl["A"], usable, pl["ox"], pl["oy"], 16 - 2 * d.v, 2 + (d.v & 1))
    return {"sprite": sprite, "count": count, "known": known, "moving": moving, "masks": seq.read_masks_range(0, d.n)}


# ---- comparisons: each step as its own suite compares it ---------------------------------------------------------------------------
def same_bytes(got, want, where):
    """test_gpu_regrow.py's comparison: shapes, types and bytes equal."""
    if isinstance(want, dict):
        assert sorted(got) == sorted(want), where
        for k in want:
            same_bytes(got[k], want[k], where + (k,))
    elif isinstance(want, (tuple, list)):
        assert len(got) == len(want), where
        for k, (g, w) in enumerate(zip(got, want)):
            same_bytes(g, w, where + (k,))
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape and g.dtype == w.dtype and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), where


def compare_staged(got, want, where, d):
    """Bytes; the order-2 run's first parameters and level-1 stage are the order-1 run's."""
    got = dict(got)
    same_bytes(got.pop("o2_p0"), want["p0"], where + ("o2_p0",))
    for k in ("gt", "model", "mask", "thr"):
        same_bytes(got.pop("o2_l1_" + k), want["l1_" + k], where + ("o2_l1_" + k,))
    same_bytes(got, want, where)


def _compare_solve(got, want, where, violations, clear, d):
    """The bit-equal-or-flagged contract of include/gme_hip.h: a pair the host cannot solve is flagged; a pair whose level-2 and
    final fields on the host keep 1e-8 max(1, S) away from every rounding tie (ten times the device's own margin, the bar of the
    solves' own suites) is not; an unflagged pair keeps the parameter bound against the staged host path and has that path's
    level-2 model, mask and threshold, compensated frame and squared error."""
    P = pairs(d)
    assert got["params"].shape[0] == P and got["flags"].shape == (P,) and got["sse"].shape == (P,) and got["comp"].shape == (P, H, W), where
    same_bytes(got["gt"], want["gt"], where + ("gt",))
    want = want["pairs"]
    for p in range(P):
        at = where + (p,)
        if want[p] is None:
            assert got["flags"][p] != 0, at
        elif clear(want[p], d):
            assert got["flags"][p] == 0, at + ("clear of ties, flagged", int(got["flags"][p]))
        if got["flags"][p] != 0:
            continue
        assert want[p] is not None, at
        assert violations(got["params"][p], want[p]["params"], H // d.bs, W // d.bs) == [], at
        for k in ("model", "mask", "thr"):
            same_bytes(got[k][p], want[p][k], at + (k,))
        same_bytes(got["comp"][p], want[p]["comp"], at + ("comp",))
        assert got["sse"][p] == want[p]["sse"], at


def clear_solve(row, d):
    """An affine pair of host_solve whose level-2 field (of the projected level-1 solution) and final field are clear of ties."""
    import solve_cases
    h, w = H // d.bs, W // d.bs
    return solve_cases.clear_of_ties(row["p1"], h, w, 1e-8) and solve_cases.clear_of_ties(row["params"], h, w, 1e-8)


def clear_solve2(row, d):
    h, w = H // d.bs, W // d.bs
    return bool(clear_of_ties2(row["p1"], h, w)[0] and clear_of_ties2(row["params"], h, w)[0])


def compare_solve(got, want, where, d):
    import solve_cases
    _compare_solve(got, want, where, solve_cases.contract_violations, clear_solve, d)


def compare_solve2(got, want, where, d):
    _compare_solve(got, want, where, contract_violations2, clear_solve2, d)


def compare_direct(got, want, where, d):
    """The compensation byte for byte; direct_eval and refine_projective as test_gpu_direct.py compares them."""
    from helpers import check_eval, check_refine
    got, want = dict(got), dict(want)
    ev, ref, want_ev, want_ref = got.pop("eval"), got.pop("refine"), want.pop("eval"), want.pop("refine")
    same_bytes(got, want, where)
    P = pairs(d)
    assert all(len(ev[k]) == P for k in ("threshold", "counts", "cost", "sums")) and len(ref[0]) == P and len(ref[1]) == P, where
    warps = usable_warps(d, P)
    for p in range(P):
        check_eval(ev, p, want_ev[p], where + ("eval", p))
        check_refine(ref[0][p], ref[1][p], want_ref[p][0], want_ref[p][1], warps[p], H, W, where + ("refine", p))


# ---- the registry -----------------------------------------------------------------------------------------------------------------
# events: the lifetime events (lifetime_cases.EVENTS) the step's calls are, in order; calls: the gme_seq_* entry points it drives
# planes: how many compensated planes the step's last writer leaves at a demand (None: it writes none)
Step = collections.namedtuple("Step", "name run host compare events calls planes")


def compare_bytes(got, want, where, d):
    same_bytes(got, want, where)


def _step(name, events, calls, compare=compare_bytes, planes=None):
    g = globals()
    return Step(name, g["run_" + name], g["host_" + name], compare, events, tuple("gme_seq_" + c for c in calls), planes)


def targets(d):
    return d.n - 2 * d.fd


STEPS = collections.OrderedDict((s.name, s) for s in (
    _step("bbme", ("bbme",), ("bbme", "read_mv", "mv_summary", "gme_fit", "gme_read_stage")),
    _step("bbme_streamed", ("bbme_streamed",), ("bbme_streamed", "read_mv")),
    _step("subpel", ("bbme", "subpel", "compensate_qpel"), ("bbme", "subpel", "read_qmv", "compensate_qpel", "read_compensated_range"),
          planes=pairs),
    _step("hier", ("hier",), ("hier", "read_hier", "read_mv")),
    _step("vbs", ("bbme", "vbs", "compensate_vbs"), ("bbme", "vbs", "read_vbs", "compensate_vbs", "read_compensated_range"), planes=pairs),
    _step("prop", ("bbme", "prop"), ("bbme", "prop", "read_prop", "read_mv")),
    _step("bipred", ("bipred", "predict_bipred"), ("bipred", "read_bipred", "predict_bipred", "read_compensated_range"), planes=targets),
    _step("gmc", ("gmc", "predict_gmc"), ("gmc", "read_gmc", "predict_gmc", "read_compensated_range"), planes=pairs),
    _step("interp", (), ("interp",)),
    _step("obmc", ("bbme", "subpel"), ("bbme", "subpel", "obmc")),
    _step("denoise_r1", (), ("denoise",)),
    _step("denoise_r2", (), ("denoise",)),
    _step("staged", ("gme_begin_fit",), ("gme_begin_fit", "gme_fit", "gme_begin_fit2", "gme_fit2", "gme_read_stage"), compare_staged),
    _step("solve", ("gme_begin_fit", "compensate"), ("gme_device_solve", "gme_read_stage", "read_compensated_range"), compare_solve, pairs),
    _step("solve2", ("gme_begin_fit", "compensate2"), ("gme_device_solve2", "gme_read_stage", "read_compensated_range"), compare_solve2, pairs),
    _step("models", ("compensate", "compensate2"), ("compensate", "compensate2", "read_compensated_range"), planes=pairs),
    _step("direct", ("compensate_projective",), ("compensate_projective", "read_compensated", "direct_eval", "refine_projective"),
          compare_direct, pairs),
    _step("warp_frames", ("warp_frames",), ("warp_frames", "read_warped_range", "frame_sse")),
    _step("warp_fill", (), ("warp_fill",)),
    _step("mosaic", ("mosaic", "moving_masks"), ("mosaic", "read_mosaic", "moving_masks", "read_masks_range")),
))

# The groups test_gpu_reuse.py is parametrised by.  A group mixes families that share buffers: the motion field; the compensated
# planes, their squared errors and parameters; the box-sum tables and the context's search scratch; the staged estimate's levels.
GROUPS = collections.OrderedDict((
    ("field", ("bbme", "hier", "prop", "bbme_streamed", "vbs")),
    ("planes", ("subpel", "models", "bipred", "gmc", "solve")),
    ("projective", ("direct", "bipred", "models", "vbs")),
    ("boxsum", ("bbme", "denoise_r1", "bipred", "denoise_r2", "gmc")),
    ("staged", ("staged", "obmc", "solve2", "interp", "solve")),
    ("frames", ("warp_frames", "mosaic", "warp_fill", "direct")),
    ("queued", ("bbme", "staged", "models", "solve", "warp_fill", "interp", "solve2", "denoise_r1", "bbme_streamed")),
))

# The split-phase runs.  SPLIT_LIBRARY: groups run with the library's switch alone (ordinary result buffers); every call of them
# is split-phase (gme_seq_gme_begin_fit(2), gme_seq_gme_fit(2), gme_seq_compensate(2), the device solves, gme_seq_upload) or
# "blocking, also in split-phase mode" by the header, which is why the projective calls, gme_seq_warp_frames and the mosaic are
# in none of them.  SPLIT_WRAPPER: the group run through Sequence.set_split_phase(True), whose results arrive in the wrapper's
# page-locked buffers; it holds only steps the wrapper lets through in that mode.
SPLIT_LIBRARY = ("field", "planes", "boxsum", "staged")
SPLIT_WRAPPER = ("queued",)
NO_SPLIT = ("direct", "warp_frames", "mosaic")                  # steps whose calls the header does not allow in split-phase mode

# gme_seq_* declarations of the header that no step drives, and why
EXEMPT = {
    "gme_seq_create": "makes the sequence every test runs on",
    "gme_seq_destroy": "frees it",
    "gme_seq_upload": "the event between two demands (test_gpu_reuse.py uploads the second stack once per order), not a step",
    "gme_seq_set_frames": "how a demand sets the frames in use, before every step",
    "gme_seq_synth": "an upload by another route; holds no result of its own (test_gpu_lifetimes.py has it as an event)",
    "gme_seq_invalidate": "marks the pyramids stale and sizes nothing (test_gpu_lifetimes.py has it as an event)",
    "gme_seq_read_frame": "reads the frames, whose buffers gme_seq_create sizes once",
    "gme_seq_gme_begin": "gme_seq_gme_begin_fit without the level-1 fit; the steps drive the fused call the drivers use",
    "gme_seq_set_split_phase": "the split-phase switch: the round-robin order runs again under it",
    "gme_seq_wait": "waits for the last split-phase call; holds no result",
    "gme_seq_poll": "asks whether gme_seq_wait would block; holds no result",
    "gme_seq_mv_summary_gather": "a communicator call: needs the RCCL communicator of a multi-GPU run",
}


def expected_for(step, d, stack_name, seed_b=SEED_B):
    """What step ``step`` returns at demand ``d`` on a stack (cached per step, demand and stack)."""
    return STEPS[step].host(stack(stack_name, seed_b)[:d.n], d)


def expected(step, index, seed_b=SEED_B):
    """... at entry ``index`` of the schedule."""
    return expected_for(step, SCHEDULE[index], STACKS[index], seed_b)


def compare(step, got, want, where, d):
    STEPS[step].compare(got, want, where, d)


# ---- what the host test measures -----------------------------------------------------------------------------------------------------
def arrays_of(result):
    """The arrays of an expectation, flattened: [(name, array)]."""
    out = []

    def walk(name, r):
        if r is None:
            return
        if isinstance(r, dict):
            for k in sorted(r):
                walk(name + (k,), r[k])
        elif isinstance(r, (tuple, list)):
            for k, v in enumerate(r):
                walk(name + (k,), v)
        else:
            out.append((name, np.asarray(r)))
    walk((), result)
    return out


def elements(result):
    return sum(a.size for _, a in arrays_of(result))


def same_result(a, b):
    a, b = arrays_of(a), arrays_of(b)
    return len(a) == len(b) and all(na == nb and x.shape == y.shape and np.array_equal(x, y) for (na, x), (nb, y) in zip(a, b))


def same_shapes(a, b):
    a, b = arrays_of(a), arrays_of(b)
    return len(a) == len(b) and all(na == nb and x.shape == y.shape for (na, x), (nb, y) in zip(a, b))


def discrimination_failures(seed_b=SEED_B):
    """(step, i, j) where the expectations at two different entries of the schedule are the same arrays."""
    distinct = sorted({(SCHEDULE[i].name, STACKS[i]): i for i in range(len(SCHEDULE))}.values())
    bad = []
    for step in STEPS:
        for x, i in enumerate(distinct):
            for j in distinct[x + 1:]:
                if same_result(expected(step, i, seed_b), expected(step, j, seed_b)):
                    bad.append((step, i, j))
    return bad


def find_seed_b(start=49):
    """How SEED_B was chosen (CPU only, not run by the tests)."""
    seed = start
    while discrimination_failures(seed):
        seed += 1
    return seed
