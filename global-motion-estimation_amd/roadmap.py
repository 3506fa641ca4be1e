"""The authors' roadmap (``recap_future_updates.md:9-14``), built on the same device pipeline.

EXTENSIONS -- nothing here has a reference implementation to be bit-compared with (SURVEY.md §8(f)4:
"other motion models, auto-selection of bs / sw / outlier fraction ... change results").  The default
path (``motion.global_motion_estimation``, affine model, fixed constants) is untouched; these helpers
are opt-in and tested for self-consistency (``tests/test_gpu_round2.py``).

1. **Other motion models.**  The device fit stage (``k_fit_level``, motion.py:232-279) leaves the
   weighted normal-equation sums ``F = sum [1 x y]^T [1 x y]``, ``Sx = sum [1 x y] dx``,
   ``Sy = sum [1 x y] dy`` over the inlier blocks.  Those sums also determine the least-squares fit of
   every model that is linear in ``[1, x, y]``; only the small host solve differs:

   * ``affine``       6 parameters -- the reference (two 3x3 systems, motion.py:262-282)
   * ``translation``  2 parameters -- ``dx = a0, dy = b0``
   * ``similarity``   4 parameters -- zoom ``s`` + rotation ``r`` + shift.  In the reference's convention ``x`` is the
     ROW coordinate and ``dx`` the COLUMN displacement (motion.py:254-259, bbme.py:176-177), so the model reads
     ``dx = a0 - r x + s y``, ``dy = b0 + s x + r y``

   Every model is returned in the affine layout ``[a0, a1, a2, b0, b1, b2]`` so the model field, the
   outlier mask of the next level and the compensation run unchanged -- including the reference's own
   coordinate mismatch: the fit sees ``x = 4 i, y = 4 j`` (motion.py:254-255) while the model field is
   evaluated at the raw block indices (motion.py:139-157), so the linear terms of ANY model act with a
   quarter of their fitted strength downstream, exactly as in the reference's affine path.

   **Second-order models.**  The paper the reference follows has second-order terms (motion.py:191-207 quotes its
   projection rule); the 15 sums above cannot determine them, so these models have their own device fit
   (``k_fit_level2``, gme_kernels.hip) leaving 27 sums: the 15 weighted moments ``sum w x^p y^q`` (p + q <= 4, in the
   order ``1 x y x2 xy y2 x3 x2y xy2 y3 x4 x3y x2y2 xy3 y4``), then ``Sx = sum w phi dx`` and ``Sy = sum w phi dy`` over the
   basis ``phi = [1, x, y, x^2, xy, y^2]``.  Parameters are float64[12] = ``[a0 a1 a2 b0 b1 b2 | a3 a4 a5 b3 b4 b5]``,
   ``dx = a0 + a1 x + a2 y + a3 x^2 + a4 xy + a5 y^2``, ``dy`` likewise -- the first six are the affine layout:

   * ``bilinear``            only ``xy`` among the second-order terms (two 4x4 systems)
   * ``pseudo_perspective``  ``dx = a0 + a1 x + a2 y + c1 y^2 + c2 xy``, ``dy = b0 + b1 x + b2 y + c1 xy + c2 x^2`` in the
     reference's axes, i.e. ``a4 = b3 = c2``, ``a5 = b4 = c1``, ``a3 = b5 = 0`` (one coupled 8x8 system)
   * ``quadratic``           all twelve (two 6x6 systems)

   The same coordinate quirk holds: downstream, linear terms act at 1/4 of their fitted strength and second-order terms
   at 1/16 (``model_field`` evaluates at the raw block indices ``(i, j)``).  Projection between the levels doubles the
   constants, keeps the linear terms and halves the second-order ones (``project``: x, y double per level).  The normal
   matrices are Jacobi-equilibrated before the solve (raw condition number ~6e9 at 720p, ~3e11 at 1080p for the 6x6
   quadratic system; ~6e2 scaled).  The projective model is nonlinear and is not one of these indirect models: it has its
   own direct estimator below.

   **Projective (direct).**  ``refine_projective`` / ``refine_sequence`` start from the indirect affine estimate
   (``affine_to_projective``) and refine an 8-parameter perspective warp on the pixels of the pyramids, coarse to fine, by
   Gauss-Newton under a truncated quadratic (k_direct_sums / k_direct_state, csrc/gme_direct.hip; host definition
   direct.py), with dense sub-pixel compensation under it.  It is a separate estimator, not an entry of ``MODELS``.
   **Stabilization.**  ``stabilize.stabilize`` chains the pair warps of either estimator into a camera path, smooths it and
   warps every frame on the device (k_warp_frames, csrc/gme_stab.hip).  With ``neighbours=K`` the border of
   frame t is filled from frames t-1, t+1, .. t-K, t+K instead of being cropped away (k_warp_fill, csrc/gme_stab_fill.hip;
   host definition stabilize.warp_fill / fill_candidates).
   **Quarter-pel block matching.**  ``subpel.motion_field`` refines the integer field of any search to half and quarter
   pixels and ``Sequence.compensate_qpel`` compensates with it (k_subpel_refine / k_compensate_qpel, csrc/bbme_subpel.hip;
   host definition subpel.py).  The fits above still take integer vectors.
   **Hierarchical block matching.**  ``hier.motion_field`` searches coarse to fine over the pyramid, every level of a block
   in one wave of one kernel (k_hier, csrc/bbme_hier.hip; host definition hier.py); its field is refined to
   quarter pixels like that of any other search.
   **Variable block size.**  ``vbs.motion_field`` splits the blocks of any search's field in four, refines each quarter
   around its parent's vector and keeps a split only where it lowers the cost by more than a penalty, the whole tree of a
   block in one wave of one kernel (k_vbs, csrc/bbme_vbs.hip; host definition vbs.py);
   ``Sequence.compensate_vbs`` compensates with the leaf field.
   **Bidirectional prediction.**  ``bipred.motion_field`` predicts a frame from the frames on both sides of it: per block the
   past reference, the next one or the rounded average of both, the averaged pair refined in alternating passes, a block's
   whole decision in one wave of one kernel (k_bipred, csrc/bbme_bipred.hip; host definition bipred.py);
   ``Sequence.predict_bipred`` writes the predicted frames.
   **Global motion compensation.**  ``gmc.motion_field`` lets every block choose between the pair's camera warp, applied pixel
   by pixel (the direct projective estimate above, or any float64[8] warp), and its own integer vector, which must beat the warp
   by a penalty; the mode map is a block-level foreground map of one pair.  A block's whole decision runs in one wave of one
   kernel (k_gmc, csrc/bbme_gmc.hip; host definition gmc.py); ``Sequence.predict_gmc`` writes the predicted
   frames.
   **Vector propagation search.**  ``propagate.motion_field`` repairs the field of a fast search with the vectors a block
   inherits: its own, its neighbours', the previous pair's, the camera's (``propagate.camera_field`` of the projective estimate
   above, or of any float64[8] warp) and zero, the cheapest refined by one pixel per pass, in rounds that each read only the field
   of the round before.  A block's whole decision runs in one wave of one kernel (k_prop, csrc/bbme_prop.hip; host definition
   propagate.py); ``Sequence.prop`` leaves the result as the sequence's motion field.
   **Frame interpolation.**  ``interp.frame`` makes the frame halfway between two frames, where there is no target block to match
   against: a block takes the vector v for which the past frame at origin - v and the next frame at origin + v differ least
   (a bilateral search within +-8 with a bias on |v|, the border replicated) and is their rounded average;
   ``interp.upconvert`` doubles the frame rate of a clip.  A block's whole search runs in one wave of one kernel (k_interp,
   csrc/bbme_interp.hip; host definition interp.py); ``Sequence.interp`` computes and returns in one call and
   keeps nothing.
   **Frame retiming.**  ``retime.frame`` makes the frame at any phase n / d (d <= 64) between two frames: a candidate V within
   +-16 whole pixels is how far content moves between them, the past frame is read -n V / d and the next one (d - n) V / d away,
   rounded to quarter pixels with one shared fraction and sampled with the four clamped taps of the quarter-pel section, and
   the pixel is the weighted blend; ``retime.convert`` changes the frame rate of a clip (24 -> 60 fps is the step 2/5) and
   ``retime.slow_motion`` slows it down, both over ``retime.schedule``.  A block's whole search runs in one wave of one kernel
   that stages the interpolated windows once per fraction (k_retime, csrc/bbme_retime.hip; host definition retime.py; DESIGN.md
   §7r); ``Context.retime_clip`` takes a host clip, computes and returns in one call and keeps nothing.
   **Overlapped block motion compensation.**  ``obmc.frame`` compensates a frame by a block field, whole or quarter pixels,
   without the jump at block edges where two neighbours disagree: every pixel is blended from the prediction of its own block and
   of the nearest vertical, horizontal and diagonal neighbour under a linear ramp, the border replicated per pixel so that no
   vector is unavailable.  One wave per row of one kernel (k_obmc, csrc/bbme_obmc.hip; host definition obmc.py);
   ``Sequence.obmc`` takes the sequence's motion field or its quarter-pel field, computes and returns in one call and keeps
   nothing.
   **Motion-compensated temporal denoising.**  ``denoise.clip`` cleans a noisy clip: every frame is averaged with the overlapped
   predictions of it from its neighbour frames (``radius`` 1 or 2 on each side), each pixel gated by the prediction error over
   its 3 x 3 window, so the filter follows local motion and leaves the frame alone where the prediction fails; the fields are
   searched from the frame being filtered and applied negated.  ``denoise.blend`` and ``denoise.frame`` are the host definition;
   one wave per row of one kernel (k_denoise, csrc/bbme_denoise.hip); ``Sequence.denoise`` searches, predicts and
   filters in one call and keeps nothing.  The default strength 24 is a convention of the tool, not a tuned value.
2. **Parameter heuristics** (``suggest_parameters``): block size from the frame height (the authors'
   slide settings, docs/presentation/main.tex:382-558, follow ``H / 20`` in 4 of 5 cases), search window
   from the dense coarse field, outlier fraction from the spread of the block vectors.
3. **One CLI** for all scripts: ``gme_cli.py``.
"""
import numpy as np

import motion

MODELS = ("affine", "translation", "similarity", "bilinear", "pseudo_perspective", "quadratic")
SECOND_ORDER = ("bilinear", "pseudo_perspective", "quadratic")

# moment index of x^p y^q in the 27 sums (M order: 1 x y x2 xy y2 x3 x2y xy2 y3 x4 x3y x2y2 xy3 y4)
_MOMENT = {(0, 0): 0, (1, 0): 1, (0, 1): 2, (2, 0): 3, (1, 1): 4, (0, 2): 5, (3, 0): 6, (2, 1): 7, (1, 2): 8, (0, 3): 9,
           (4, 0): 10, (3, 1): 11, (2, 2): 12, (1, 3): 13, (0, 4): 14}
_PHI = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))          # exponents of phi = [1, x, y, x^2, xy, y^2]


def affine_sums(sums27):
    """float64[P, 27] order-2 sums -> the exact float64[P, 15] affine sums F (3x3) | Sx[0:3] | Sy[0:3] (the same values the
    order-1 fit leaves: every term of both is one rounding of (integer) * w)."""
    s = np.asarray(sums27, dtype=np.float64).reshape(-1, 27)
    M = s[:, :15]
    F = M[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]
    return np.concatenate([F, s[:, 15:18], s[:, 21:24]], axis=1)


def project(params):
    """motion.parameter_projection (motion.py:191-207) generalised to float64[..., 6 or 12]: constants doubled, linear
    terms kept, second-order terms halved (x, y double per level).  Exact in float64.  Returns a new array."""
    p = np.array(params, dtype=np.float64)
    p[..., 0] = p[..., 0] * 2
    p[..., 3] = p[..., 3] * 2
    if p.shape[-1] == 12:
        p[..., 6:12] = p[..., 6:12] * 0.5
    return p


def _jacobi_solve(N, rhs):
    """Solve the stacked symmetric systems N x = rhs after Jacobi scaling (D N D) z = D rhs, x = D z.  Every step is an
    elementwise operation or np.linalg.solve's per-matrix LAPACK call, so a stacked batch equals per-pair solves bit for bit."""
    d = np.diagonal(N, axis1=1, axis2=2)
    if np.any(~(d > 0)):
        raise np.linalg.LinAlgError("Singular matrix")
    D = 1.0 / np.sqrt(d)
    A = N * D[:, :, None] * D[:, None, :]
    z = np.linalg.solve(A, (rhs * D)[:, :, None])[:, :, 0]        # LinAlgError on a singular system
    return z * D


def _solve_second_order(sums, model):
    s = np.asarray(sums, dtype=np.float64)
    if s.ndim == 1:
        s = s[None, :]
    if s.shape[-1] != 27:
        raise ValueError("model %r needs the 27 order-2 sums (gme_fit2), got %d per pair" % (model, s.shape[-1]))
    P = len(s)
    M, sx, sy = s[:, :15], s[:, 15:21], s[:, 21:27]
    out = np.zeros((P, 12))
    if P == 0:
        return out
    if model in ("quadratic", "bilinear"):
        basis = (0, 1, 2, 3, 4, 5) if model == "quadratic" else (0, 1, 2, 4)
        idx = [[_MOMENT[(_PHI[a][0] + _PHI[b][0], _PHI[a][1] + _PHI[b][1])] for b in basis] for a in basis]
        N = M[:, np.array(idx)]
        # both displacements share N: one stacked solve of 2P systems
        th = _jacobi_solve(np.concatenate([N, N]), np.concatenate([sx[:, basis], sy[:, basis]]))
        tx, ty = th[:P], th[P:]
        slots = [0, 1, 2, 6, 7, 8]                                    # phi_k -> parameter slot of dx (dy: + 3)
        for c, k in enumerate(basis):
            out[:, slots[k]] = tx[:, c]
            out[:, slots[k] + 3] = ty[:, c]
        return out
    if model == "pseudo_perspective":
        # unknowns (a0 a1 a2 b0 b1 b2 c1 c2); rows r_x = [1 x y 0 0 0 y^2 xy] for dx, r_y = [0 0 0 1 x y xy x^2] for dy
        rx = [(0, 0), (1, 0), (0, 1), None, None, None, (0, 2), (1, 1)]
        ry = [None, None, None, (0, 0), (1, 0), (0, 1), (1, 1), (2, 0)]
        N = np.zeros((P, 8, 8))
        for a in range(8):
            for b in range(8):
                acc = None
                for r in (rx, ry):
                    if r[a] is not None and r[b] is not None:
                        v = M[:, _MOMENT[(r[a][0] + r[b][0], r[a][1] + r[b][1])]]
                        acc = v if acc is None else acc + v
                if acc is not None:
                    N[:, a, b] = acc
        rhs = np.stack([sx[:, 0], sx[:, 1], sx[:, 2], sy[:, 0], sy[:, 1], sy[:, 2], sx[:, 5] + sy[:, 4], sx[:, 4] + sy[:, 3]], axis=1)
        th = _jacobi_solve(N, rhs)
        out[:, 0:6] = th[:, 0:6]
        c1, c2 = th[:, 6], th[:, 7]
        out[:, 7], out[:, 9] = c2, c2                                 # a4 = b3 = c2
        out[:, 8], out[:, 10] = c1, c1                                # a5 = b4 = c1
        return out
    raise ValueError("unknown motion model %r (choose from %r)" % (model, MODELS))


def solve_model(sums, model="affine"):
    """Normal-equation sums -> parameters.  First-order models: float64[P, 15] (F | Sx | Sy; or the 27 order-2 sums,
    reduced by affine_sums) -> float64[P, 6] in affine layout.  Second-order models (SECOND_ORDER): float64[P, 27] ->
    float64[P, 12]; 15-wide sums raise ValueError."""
    if model in SECOND_ORDER:
        return _solve_second_order(sums, model)
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim >= 1 and sums.shape[-1] == 27:
        sums = affine_sums(sums)
    sums = sums.reshape(-1, 15)
    if model == "affine":
        return motion._solve_batch(sums)
    F = sums[:, :9].reshape(-1, 3, 3)
    sx, sy = sums[:, 9:12], sums[:, 12:15]
    out = np.zeros((len(sums), 6))
    if model == "translation":
        n = F[:, 0, 0]
        if np.any(n == 0):
            raise np.linalg.LinAlgError("Singular matrix")
        out[:, 0] = sx[:, 0] / n
        out[:, 3] = sy[:, 0] / n
        return out
    if model == "similarity":
        n, mx, my = F[:, 0, 0], F[:, 0, 1], F[:, 0, 2]
        q = F[:, 1, 1] + F[:, 2, 2]
        # unknowns (a0, b0, s, r); rows [1, 0, y, -x] for dx and [0, 1, x, y] for dy
        N = np.zeros((len(sums), 4, 4))
        N[:, 0, 0] = n; N[:, 0, 2] = my; N[:, 0, 3] = -mx
        N[:, 1, 1] = n; N[:, 1, 2] = mx; N[:, 1, 3] = my
        N[:, 2, 0] = my; N[:, 2, 1] = mx; N[:, 2, 2] = q
        N[:, 3, 0] = -mx; N[:, 3, 1] = my; N[:, 3, 3] = q
        rhs = np.stack([sx[:, 0], sy[:, 0], sx[:, 2] + sy[:, 1], sy[:, 2] - sx[:, 1]], axis=1)
        th = np.linalg.solve(N, rhs[:, :, None])[:, :, 0]            # LinAlgError on a singular system
        a0, b0, zoom, rot = th[:, 0], th[:, 1], th[:, 2], th[:, 3]
        out[:, 0], out[:, 1], out[:, 2] = a0, -rot, zoom
        out[:, 3], out[:, 4], out[:, 5] = b0, zoom, rot
        return out
    raise ValueError("unknown motion model %r (choose from %r)" % (model, MODELS))


def model_field(shape, params):
    """motion.get_motion_field_affine (motion.py:139-157) for any model: float64[6] -> the affine field, float64[12] -> the
    second-order field ``((p0 + p2 j) + p1 i) + ((a3 (i i) + a4 (i j)) + a5 (j j))`` -> int16[shape[0], shape[1], 2]."""
    p = np.asarray(params, dtype=np.float64).reshape(-1)
    if p.size == 6:
        return motion.get_motion_field_affine(shape, p)
    if p.size != 12:
        raise ValueError("parameters of %d entries (6 or 12)" % p.size)
    import _gme_native
    return _gme_native.default_context().model2_field(p, int(shape[0]), int(shape[1]))


def normalize_model(model):
    """A motion model name -> (name, order, parameters per pair): None and "affine" give ("affine", 1, 6), the other
    first-order models order 1 and 6 parameters, SECOND_ORDER order 2 and 12; ValueError for a name not in MODELS."""
    if model is None:
        model = "affine"
    if model not in MODELS:
        raise ValueError("unknown motion model %r (choose from %r)" % (model, MODELS))
    return (model, 2, 12) if model in SECOND_ORDER else (model, 1, 6)


def stages(seq, frame_distance, model="affine", procedure=3, search_window=2, compensate=False):
    """The staged estimate of every pair of ``seq`` (motion.py:123-136), as a generator that queues each device call and
    yields when the next step needs its result: begin-fit (dense field, first parameters, projection, level-1 fit) ->
    host solve -> ``project`` -> level-2 fit -> host solve, then optionally compensation.  Returns (params, sse int64[P] or
    None).  A blocking sequence has the result at the yield already; a split-phase one once wait() returns.  Block size and
    outlier fraction are read from ``motion`` here, at call time."""
    model, order, _ = normalize_model(model)
    frac = float(motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE)
    bs = int(motion.BBME_BLOCK_SIZE)
    _, sums = seq._begin_fit(order, frame_distance, bs, frac, procedure, search_window)
    yield
    sums = seq._fit(order, 2, project(solve_model(sums, model)), frac)      # projected in float64, the solution's dtype
    yield
    params = solve_model(sums, model)
    if not compensate:
        return params, None
    sse = seq._compensate(order, frame_distance, bs, params)
    yield
    return params, np.array(sse)                 # a split-phase call's buffer is reused by the next call of its kind


def device_stages(seq, frame_distance, model="affine", procedure=3, search_window=2):
    """The whole estimate + compensation with the solves on the device (gme_device_solve, or gme_device_solve2 for a
    second-order model) as a one-step chain like ``stages`` -> (params, sse, flags).  Pairs with a non-zero flag must be
    redone by ``stages``."""
    model, order, _ = normalize_model(model)
    frac = float(motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE)
    bs = int(motion.BBME_BLOCK_SIZE)
    if model == "affine":
        params, sse, flags = seq.gme_device_solve(frame_distance, bs, frac, procedure, search_window)
    else:
        params, sse, flags = seq.gme_device_solve2(model, frame_distance, bs, frac, procedure, search_window)
    yield
    return np.array(params), np.array(sse), np.array(flags)


def estimate_blocking(seq, frame_distance, model="affine", procedure=3, search_window=2, compensate=False):
    """``stages`` run to its end with blocking calls -> (params, sse or None)."""
    if getattr(seq, "_split", False):
        raise RuntimeError("estimate_sequence needs blocking calls: the sequence is in split-phase mode (set_split_phase(False) "
                           "first, or drive roadmap.stages with wait() like sequence.ShardedSequence._round_robin)")
    chain = stages(seq, frame_distance, model, procedure, search_window, compensate)
    while True:
        try:
            next(chain)
        except StopIteration as done:
            return done.value


def estimate_sequence(seq, frame_distance=1, model="affine", procedure=3, search_window=2):
    """motion.estimate_sequence with a selectable motion model -> float64[P, 6] (affine layout), or float64[P, 12] for the
    second-order models (order-2 device fits, gme_seq_gme_begin_fit2 / gme_seq_gme_fit2)."""
    return estimate_blocking(seq, frame_distance, model, procedure, search_window)[0]


def global_motion_estimation(previous, current, model="affine"):
    """motion.global_motion_estimation (motion.py:109-136) with a selectable model."""
    return estimate_sequence(motion._pair_sequence(previous, current), 1, model)[0]      # the cached two-frame sequence of motion.py


def affine_to_projective(params, block_size=16):
    """The indirect affine estimate float64[..., 6] (or a second-order model's 12, of which the first six are used) ->
    the projective start float64[..., 8] of the same displacement field (direct.affine_to_projective)."""
    import direct
    return direct.affine_to_projective(params, block_size)


def projective_to_level(h, level):
    """Full-resolution projective parameters -> those of pyramid level ``level`` (0 coarsest, 2 full resolution): h2, h5
    scaled by 2^-(2-level), h6, h7 by its inverse.  Exact in float64."""
    import direct
    return direct.projective_to_level(h, level)


def refine_sequence(seq, frame_distance=1, init=None, outlier_fraction=0.1, max_iters=10, procedure=3, search_window=2):
    """Direct projective refinement of every pair of a device-resident sequence (gme_seq_refine_projective) ->
    (h float64[P, 8], flags int32[P]).  ``init`` float64[P, 8] defaults to the indirect affine estimate
    (motion.estimate_sequence, affine_to_projective at motion.BBME_BLOCK_SIZE)."""
    if init is None:
        init = affine_to_projective(motion.estimate_sequence(seq, frame_distance, procedure, search_window),
                                    int(motion.BBME_BLOCK_SIZE))
    return seq.refine_projective(frame_distance, init, outlier_fraction, max_iters)


def refine_projective(previous, current, init=None, outlier_fraction=0.1, max_iters=10):
    """One pair: the projective warp from ``current`` back into ``previous`` -> (h float64[8], flags).  ``init`` float64[8]
    defaults to the indirect affine estimate."""
    seq = motion._pair_sequence(previous, current)
    h, flags = refine_sequence(seq, 1, None if init is None else np.asarray(init, dtype=np.float64).reshape(1, 8),
                               outlier_fraction, max_iters)
    return h[0], int(flags[0])


def suggest_parameters(previous, current):
    """Heuristics for the constants the authors tuned by hand per video (recap_future_updates.md:4-8):

    * ``block_size``     frame height / 20, to a multiple of 4 in [8, 32]
    * ``search_window``  covers the 95th percentile of the dense coarse field (pyramid level 0,
                         motion.py:13-30) scaled to full resolution, multiple of 4 in [4, 32]
    * ``outlier_fraction``  share of level-2 block vectors further than 2 px (L1) from the translational
                         fit of the rest, plus a margin, in [0.1, 0.5] (motion.py:10 uses a fixed 0.3)
    """
    import bbme
    import utils
    H, W = previous.shape
    bs = int(min(32, max(8, 4 * round(H / 20.0 / 4.0))))
    pyr_p, pyr_c = utils.get_pyramids(previous), utils.get_pyramids(current)
    dense = motion.dense_motion_estimation(pyr_p[0], pyr_c[0]).reshape(-1, 2)
    reach = 4.0 * np.percentile(np.abs(dense).max(axis=1), 95) if len(dense) else 0.0
    sw = int(min(32, max(4, 4 * int(np.ceil((reach + 2.0) / 4.0)))))
    field = bbme.get_motion_field(previous, current, block_size=bs, searching_procedure=3).reshape(-1, 2)
    frac = 0.3
    if len(field):
        med = np.median(field, axis=0)
        far = np.abs(field - med).sum(axis=1) > 2
        frac = float(min(0.5, max(0.1, far.mean() + 0.05)))
    return {"block_size": bs, "search_window": sw, "outlier_fraction": round(frac, 3)}
