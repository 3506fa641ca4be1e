/*
 * gme_hip.h -- C ABI of libgme_hip.so, the MI355X (gfx950) implementation of the
 * per-frame-pair hot path of Samaretas/global-motion-estimation.
 *
 * The reference is pure Python and has no FFI; its boundary is the module surface
 * of global_motion_estimation/{bbme,motion,utils}.py.  Each entry point below names
 * the reference function(s) it replaces (paths relative to
 * /root/reference/global_motion_estimation/).  The Python mirror of that surface
 * (global-motion-estimation_amd/{bbme,motion,utils}.py) binds these symbols with
 * ctypes; INTEGRATION.md shows the stub a maintainer would add upstream.
 *
 * Conventions
 *   - plain C types only; every function returns 0 (GME_OK) or a negative GME_ERR_*;
 *     gme_last_error() gives the text for the calling thread's last failure.
 *   - host images are uint8, row-major, `stride` bytes between rows; motion fields
 *     are int32[h][w][2] with [..][0] = column (x) and [..][1] = row (y)
 *     displacement, position in `cur` minus position in `prev` (bbme.py:176-177).
 *   - the caller allocates every output; the library owns device memory inside the
 *     opaque gme_ctx / gme_seq objects; one HIP stream per context.  Every entry point locks
 *     its context for the whole call, so threads may share a context (their calls serialise;
 *     the reference is single-threaded); use one context per thread for
 *     concurrency.
 *   - integer results (motion vectors, masks, model fields, compensated frames,
 *     squared-error sums) are bit-exact with the reference; the normal-equation
 *     sums are bit-exact float64; the 3x3 solve stays on the host (NumPy) because
 *     LAPACK builds differ in the last bits.
 */
#ifndef GME_HIP_H
#define GME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define GME_API __attribute__((visibility("default")))
#else
#define GME_API
#endif

typedef struct gme_ctx gme_ctx;   /* one device + one stream + scratch */
typedef struct gme_seq gme_seq;   /* a frame sequence resident in HBM + per-pair results */

enum {
    GME_OK = 0,
    GME_ERR_ARG = -1,        /* bad pointer / size / index (reference: IndexError, bbme.py:27,60) */
    /* -2 is unused (rounds 1-3 reserved it for "inexact": outside float32's exact-integer range, bbme.py:61-64, the kernels
     * sum in NumPy's float32 order instead of refusing) */
    GME_ERR_GEOMETRY = -3,   /* frame smaller than the search needs (reference: AssertionError, bbme.py:59) */
    GME_ERR_HIP = -4,        /* HIP runtime failure */
    GME_ERR_STATE = -5,      /* call order violated (e.g. fit before begin) */
    GME_ERR_NOMEM = -6
};

/* bbme.py:609-614 searching_procedures, bbme.py:608 pnorm_distances */
enum { GME_SEARCH_EXHAUSTIVE = 0, GME_SEARCH_THREESTEP = 1, GME_SEARCH_TWODLOG = 2, GME_SEARCH_DIAMOND = 3 };
enum { GME_NORM_MAE = 0, GME_NORM_MSE = 1 };

GME_API const char *gme_last_error(void);
GME_API int gme_device_count(void);
GME_API gme_ctx *gme_create(int device_id);
GME_API void gme_destroy(gme_ctx *ctx);
GME_API int gme_sync(gme_ctx *ctx);
GME_API int gme_device_info(gme_ctx *ctx, char *name, int name_len, int *cu_count, int *clock_khz);
/* PCI bus id of the context's device ("0000:05:00.0"); makes that device current and checks that it answers.  The
 * all-ranks-agree bring-up of the RCCL communicator (sequence.comm_init) publishes it in its first phase, so that a
 * lost device or two ranks on one device end in a clean refusal on every rank instead of inside ncclCommInitRank.
 * No reference counterpart (the reference is single-process, results.py:41-50). */
GME_API int gme_device_bus_id(gme_ctx *ctx, char *out, int out_len);
/* opaque handle of the context's HIP stream (hipStream_t), for callers that
 * want to order their own work or events after the library's */
GME_API void *gme_stream(gme_ctx *ctx);

/* Diagnostics of the context's last block-matching call (gme_bbme_u8, gme_seq_bbme, or the last
 * level search of a staged GME run): the kernel / tile shape / schedule the launch plan chose, e.g.
 * "k_exh_sea16p<3,6> tiles 2x4 persistent-dynamic grid 2048 lds 34864", and for the successive-
 * elimination kernels how many candidate patches the bound was applied to and how many it left
 * for exact evaluation (both 0 for kernels that evaluate every candidate, bbme.py:146-174), and how many
 * tiles it handed to the brute-force redo kernel because the bound pruned too little there.
 * No reference counterpart; tests use it to assert which kernel instance they exercised.
 * Any pointer may be NULL.  Synchronises. */
GME_API int gme_last_bbme_info(gme_ctx *ctx, char *plan, int plan_len, int64_t *patches, int64_t *surviving,
                       int64_t *redo_tiles);
/* Same call, one more figure: the patches the FIRST upper bound of each block left (what a single evaluation round
 * would have scored); gme_last_bbme_info's `surviving` is what the ordered two-round evaluation really scored
 * (the exactness argument of bbme.py:171 -- only a smaller key replaces the best one -- holds for any upper bound that
 * is a real candidate's cost, so tightening it between the rounds changes the work, never the result).  Synchronises. */
GME_API int gme_last_bbme_listed(gme_ctx *ctx, int64_t *listed);

/* HIP-event stopwatch on the context's stream (bench.py: kernel time of the timed region) */
GME_API int gme_timer_start(gme_ctx *ctx);
GME_API int gme_timer_stop(gme_ctx *ctx, float *elapsed_ms);   /* synchronises */

/* ---------------------------------------------------------------------------
 * Single-pair calls on host buffers (H2D, kernel, D2H inside the call).
 * ------------------------------------------------------------------------- */

/* bbme.get_motion_field (bbme.py:12-38) with the four searches (bbme.py:105-534).
 * mf_out: int32[H/bs][W/bs][2]. */
GME_API int gme_bbme_u8(gme_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int H, int W, int stride,
                int block_size, int search_window, int procedure, int pnorm, int32_t *mf_out);

/* cv2.pyrDown as called by utils.get_pyramids (utils.py:34-51); dst is ((H+1)/2) x ((W+1)/2), tight. */
GME_API int gme_pyrdown_u8(gme_ctx *ctx, const uint8_t *src, int H, int W, int stride, uint8_t *dst);

/* motion.get_motion_field_affine (motion.py:139-157): int16[h][w][2], round-half-even. */
GME_API int gme_affine_field(gme_ctx *ctx, const double params[6], int h, int w, int16_t *mf_out);

/* motion.compensate_frame (motion.py:289-321); mf is int32[h][w][2]; out is H x W, tight. */
GME_API int gme_compensate_u8(gme_ctx *ctx, const uint8_t *frame, int H, int W, int stride,
                      const int32_t *mf, int h, int w, uint8_t *out);

/* integer core of utils.PSNR (utils.py:100-116): sum over pixels of (a-b)^2. */
GME_API int gme_sse_u8(gme_ctx *ctx, const uint8_t *a, const uint8_t *b, int H, int W, int stride_a,
               int stride_b, int64_t *sse_out);

/* ---------------------------------------------------------------------------
 * Sequence API: N frames resident in HBM; pair p = (frame p, frame p + fd) as in
 * results.py:41-48.  This is the batch form of the hot path and what bench.py times.
 * ------------------------------------------------------------------------- */
GME_API gme_seq *gme_seq_create(gme_ctx *ctx, int n_frames, int H, int W);
GME_API void gme_seq_destroy(gme_seq *seq);
GME_API int gme_seq_upload(gme_seq *seq, int first, int count, const uint8_t *frames, int row_stride,
                   int64_t frame_stride);
/* Use only the first n_frames frames (1 <= n_frames <= the count given to gme_seq_create) from now on: every stage call covers
 * the pairs of frames [0, n_frames) -- results.py:41-48 over a shorter list -- while the buffers stay sized for the full count.
 * How one sequence serves chunks of different lengths of a longer video (sequence.StreamEstimator).  Ends a staged GME run.
 * A change of the count is new frame data to every result the sequence keeps (see "Result lifetimes" below). */
GME_API int gme_seq_set_frames(gme_seq *seq, int n_frames);
/* deterministic synthetic frames t0 .. t0+N-1 generated on the device */
GME_API int gme_seq_synth(gme_seq *seq, uint64_t seed, int t0);
/* mark the pyramid levels stale (upload and synth do so themselves); new frame data to every result the sequence keeps */
GME_API int gme_seq_invalidate(gme_seq *seq);
/* level 2 = full resolution, 1 and 0 = pyramid levels (valid after gme_seq_gme_begin) */
GME_API int gme_seq_read_frame(gme_seq *seq, int level, int index, uint8_t *out);

/* Result lifetimes.  "New frame data" below is gme_seq_upload, gme_seq_synth, gme_seq_invalidate, a gme_seq_set_frames that
 * changes the count, and the upload inside gme_seq_bbme_streamed.  Each result family states where it ends; a call that a
 * family's text does not name leaves that result readable and byte-identical (tests/lifetime_cases.py holds the whole table,
 * tests/test_gpu_lifetimes.py enforces it).  Three rules the families share:
 *   - the motion field of gme_seq_read_mv survives new frame data: it is a prior (gme_seq_prop, gme_seq_vbs), replaced only by
 *     gme_seq_bbme, gme_seq_bbme_streamed, gme_seq_hier and gme_seq_prop;
 *   - the quarter-pel result ends with new frame data and with the next block-matching call (gme_seq_bbme,
 *     gme_seq_bbme_streamed, gme_seq_hier, gme_seq_prop), exactly where the hierarchical, variable-block-size and propagation
 *     results end;
 *   - the warped frames, the mosaic and the masks are kept in the sequence through new frame data, until their own call
 *     writes them again. */

/* bbme.get_motion_field over every pair of the sequence; results stay on the device */
GME_API int gme_seq_bbme(gme_seq *seq, int frame_distance, int block_size, int search_window,
                 int procedure, int pnorm);
GME_API int gme_seq_read_mv(gme_seq *seq, int first_pair, int count, int32_t *mf_out);

/* The same search for frames that still live in host memory (results.py:41-50 hands the path a list of
 * host arrays, utils.py:9-31): frames [0, count) are uploaded in chunks of `chunk_frames` on a copy
 * stream while the search of the previous chunk runs, and each chunk's fields are read back into
 * mf_out[count - fd][H/bs][W/bs][2] behind its kernel.  The frames stay resident in `seq` afterwards.
 * Page-locked `frames` (gme_host_alloc) cross at link speed; pageable memory works but is staged by
 * the HIP runtime.  Returns when mf_out is complete. */
GME_API int gme_seq_bbme_streamed(gme_seq *seq, const uint8_t *frames, int row_stride, int64_t frame_stride,
                          int count, int frame_distance, int block_size, int search_window, int procedure,
                          int pnorm, int chunk_frames, int32_t *mf_out);
/* page-locked host memory for frame loaders (hipHostMalloc); NULL on failure */
GME_API void *gme_host_alloc(size_t bytes);
GME_API void gme_host_free(void *p);

/* motion.global_motion_estimation (motion.py:109-136), staged so that the host does
 * the 3x3 solves (motion.py:262-264,280-282) between levels:
 *   begin : pyramids (utils.py:34-51) of all frames, diamond BBME at the three levels
 *           (motion.py:27-29,224-229), first parameters (motion.py:176-188) -> float32[P][6]
 *   fit   : for level 1 or 2 and parameters already projected by the caller
 *           (motion.py:191-207): model field, L1 difference, threshold, outlier mask,
 *           sequential float64 normal-equation sums (motion.py:232-279)
 *           -> sums_out[P][15] = F (9, row-major) | Sx (3) | Sy (3)
 * `procedure` / `search_window` select the BBME used at levels 1 and 2 (the reference
 * hard-codes diamond, GME_SEARCH_DIAMOND; exhaustive serves BASELINE config 4).
 * The level searches are launched so that the caller's work between the stages overlaps them:
 * begin returns once the first parameters are on the host with the level-1 search already
 * running; fit(level 1) returns its sums with the level-2 search running.  New frame data
 * (upload / synth / invalidate) ends a staged run: fit and the stage read-back then report GME_ERR_STATE until begin. */
GME_API int gme_seq_gme_begin(gme_seq *seq, int frame_distance, int bbme_block_size, int procedure,
                      int search_window, float *params0_out);
GME_API int gme_seq_gme_fit(gme_seq *seq, int level, const double *params_in, double outlier_fraction,
                    double *sums_out);
/* begin + projection of the first parameters (motion.py:191-207: two exact doublings of the float32 vector) + fit(level 1) in
 * one call: the first parameters go from the dense field to the level-1 fit on the device, so a staged run needs three
 * dependent host round trips instead of four (level-1 sums, level-2 sums, squared errors).  Returns the level-1 sums
 * (split-phase: once gme_seq_wait has returned) with the level-2 search already queued.  params0_out may be NULL. */
GME_API int gme_seq_gme_begin_fit(gme_seq *seq, int frame_distance, int bbme_block_size, int procedure, int search_window,
                          double outlier_fraction, float *params0_out, double *sums1_out);
/* stage read-back for parity tests; any pointer may be NULL.
 * level 0: gt = dense field (bs 2); levels 1, 2: gt, model (int16), mask, threshold */
GME_API int gme_seq_gme_read_stage(gme_seq *seq, int level, int pair, int32_t *gt, int16_t *model,
                           uint8_t *mask, int64_t *threshold);

/* motion.get_motion_field_affine((H/bs, W/bs), params) + motion.compensate_frame(prev, field)
 * + sum of squared error against `cur` for every pair (results.py:52-59,109).
 * Compensated frames stay on the device; sse_out[P] may be NULL.
 * The compensated frames are one stack of planes that every compensating or predicting call of the sequence writes
 * (gme_seq_compensate, gme_seq_compensate2, gme_seq_compensate_projective, gme_seq_compensate_qpel, gme_seq_compensate_vbs,
 * gme_seq_predict_bipred, gme_seq_predict_gmc and the device solves): each call writes planes 0 .. its own count - 1 and ends
 * the planes of the call before it.  They stay readable through new frame data.  gme_seq_read_compensated(_range) of a
 * range that holds a plane the last writer did not write, or before any writer, is GME_ERR_STATE. */
GME_API int gme_seq_compensate(gme_seq *seq, int frame_distance, int block_size, const double *params,
                       int64_t *sse_out);
GME_API int gme_seq_read_compensated(gme_seq *seq, int pair, uint8_t *out);
/* the compensated frames of pairs first .. first+count-1 into out[count][H][W] (tight), one wait for all of them: a finished
 * chunk of a streamed video for results.py's writers (results.py:59-76) */
GME_API int gme_seq_read_compensated_range(gme_seq *seq, int first, int count, uint8_t *out);

/* Second-order motion models (EXTENSION: roadmap.py bilinear / pseudo_perspective / quadratic; the reference fits the affine
 * part of the paper's model only, motion.py:191-207).  params[12] = [a0 a1 a2 b0 b1 b2 | a3 a4 a5 b3 b4 b5] with
 * dx = a0 + a1 x + a2 y + a3 x^2 + a4 xy + a5 y^2 and dy likewise: the first six are the affine layout.  The fit sees
 * x = 4 i, y = 4 j (motion.py:254-255); the field is evaluated at the raw block indices (motion.py:139-157) as
 * d = ((p0 + p2 j) + p1 i) + ((a3 (i i) + a4 (i j)) + a5 (j j)), each product and sum rounded separately, round-half-even,
 * int16 wrap -- with zero second-order terms the affine field bit for bit.
 * sums[27] = the 15 weighted moments sum w x^p y^q, p + q <= 4, in the order 1 x y x2 xy y2 x3 x2y xy2 y3 x4 x3y x2y2 xy3 y4,
 * then Sx[6] = sum w phi_k dx, Sy[6] = sum w phi_k dy with phi = [1 x y x2 xy y2]; each a sequential float64 sum over the
 * inliers in row-major order (motion.py:248-261,266-279), so the entries M[0..5], Sx[0..2], Sy[0..2] equal the 15 sums of the
 * order-1 calls bit for bit.  Staging, split-phase behaviour and state errors are those of the order-1 counterparts; the
 * stage and compensated-frame read-backs work after them. */
/* motion.get_motion_field_affine (motion.py:139-157) for params[12]: int16[h][w][2] */
GME_API int gme_model2_field(gme_ctx *ctx, const double params[12], int h, int w, int16_t *mf_out);
/* gme_seq_gme_begin_fit with sums1_out[P][27] (the level-1 field is the projected translation's: same field, mask and
 * threshold as gme_seq_gme_begin_fit) */
GME_API int gme_seq_gme_begin_fit2(gme_seq *seq, int frame_distance, int bbme_block_size, int procedure, int search_window,
                                   double outlier_fraction, float *params0_out, double *sums1_out);
/* gme_seq_gme_fit (motion.py:210-279) with params_in[P][12] and sums_out[P][27]; levels 1, 2 and -1 (the field of the last
 * gme_seq_bbme, negative outlier_fraction: the unmasked fit of motion.py:33-88) */
GME_API int gme_seq_gme_fit2(gme_seq *seq, int level, const double *params_in, double outlier_fraction, double *sums_out);
/* gme_seq_compensate (motion.py:289-321, results.py:52-59,109) with the order-2 field of params[P][12] */
GME_API int gme_seq_compensate2(gme_seq *seq, int frame_distance, int block_size, const double *params, int64_t *sse_out);
/* Second-order model ids of gme_solve_model2_sums / gme_seq_gme_device_solve2: the indices of roadmap.MODELS.  Any other id
 * is GME_ERR_ARG. */
enum { GME_MODEL_BILINEAR = 3, GME_MODEL_PSEUDO_PERSPECTIVE = 4, GME_MODEL_QUADRATIC = 5 };
/* Opt-in device solve of the second-order normal equations (the order-2 counterpart of gme_solve_fit_sums, below):
 * sums[P][27] -> params_out[P][12] in the layout above (pseudo-perspective: a4 = b3 = c2, a5 = b4 = c1; if `project`,
 * roadmap.project: constants x2, second-order terms x1/2) and flags_out[P].  The system is roadmap._solve_second_order's,
 * Jacobi-equilibrated and solved by Gaussian elimination with partial pivoting.  LAPACK's last bits are not reproduced; with
 * m_k = max |phi_k(i, j)| over the h x w field (1, h-1, w-1, (h-1)^2, (h-1)(w-1), (w-1)^2) and S = sum_k |p_k| m_k over the six
 * terms of one displacement, every parameter of an unflagged pair satisfies |p_dev - p_host| m_k <= 1e-10 max(1, S).
 * flags_out: bit 1 -- a displacement of the h x w order-2 field of the output within 1e-9 max(1, S) of k + 0.5 (or
 * |d| >= 30000, or NaN); bit 4 -- singular (a non-positive diagonal entry: LinAlgError in roadmap; or a zero pivot); bit 8 --
 * ill-conditioned (min / max |pivot| of the equilibrated system below 3e-5: the inliers leave a direction of the model almost
 * undetermined and the bound above is not assured; DESIGN.md gives the measurement).  Host pointers. */
GME_API int gme_solve_model2_sums(gme_ctx *ctx, int model, const double *sums, int pairs, int project, int h, int w,
                                  double *params_out, int32_t *flags_out);
/* gme_seq_gme_device_solve for a second-order model: begin_fit2 -> device solve + projection -> fit2(2) -> device solve ->
 * compensate2 in one call with one host round trip.  params_out[P][12] meets the parameter bound of gme_solve_model2_sums
 * against the staged path (gme_seq_gme_begin_fit2 -> roadmap.solve_model -> roadmap.project -> gme_seq_gme_fit2(2) ->
 * roadmap.solve_model -> gme_seq_compensate2) over the final H/bs x W/bs field; for every pair whose flags_out[p] is 0 the
 * level-2 model field, mask and threshold, the compensated frame and sse_out[p] (may be NULL) are bit-equal to that path's.
 * flags_out[p]: bit 1 / 2 -- a displacement near a rounding tie in the level-2 field / the final field; bit 4 singular,
 * bit 8 ill-conditioned, as above: redo that pair through the staged calls.  Split-phase like gme_seq_gme_device_solve. */
GME_API int gme_seq_gme_device_solve2(gme_seq *seq, int model, int frame_distance, int bbme_block_size, int procedure,
                                      int search_window, double outlier_fraction, double *params_out, int64_t *sse_out,
                                      int32_t *flags_out);
/* ---------------------------------------------------------------------------------------------------------------------
 * Direct projective refinement (host definition: direct.py).  An opt-in estimator beside the
 * indirect models, working on the pixels of the resident pyramids.  Parameters are float64[8] h, H = [[h0 h1 h2] [h3 h4 h5]
 * [h6 h7 1]]: the pixel (u = column, v = row) of the CURRENT frame samples the PREVIOUS frame at u' = (h0 u + h1 v + h2) / d,
 * v' = (h3 u + h4 v + h5) / d, d = h6 u + h7 v + 1 (OpenCV's warpPerspective with WARP_INVERSE_MAP) -- image axes, not the
 * reference's "x = row".  Identity [1 0 0 0 1 0 0 0].  At pyramid level L, h2 and h5 are scaled by s = 2^-(2-L) and h6, h7
 * by 1/s.  Prediction: prev sampled bilinearly at (u', v') where 0 <= u' <= W_L-1 and 0 <= v' <= H_L-1 (valid pixels), the
 * far tap clamped on the last row / column; warp, weights and residual e = cur - prediction in float64, one rounding per
 * operation, bit-identical to direct.py.  Objective of a level: a truncated quadratic with threshold t fixed at the level's
 * start (the upper edge of the first 1/16-wide bin of the |e| histogram at which the count reaches
 * ceil((1 - outlier_fraction) n_valid)); cost = (sum over |e| < t of e^2 + (n_valid - n_in) t^2) / n_valid.  These calls
 * build the pyramids if they are stale and cover the pairs (p, p + frame_distance) of the frames in use.  Host pointers.
 * ------------------------------------------------------------------------------------------------------------------- */
/* One evaluation per pair at params_in[P][8] in level-`level` coordinates (0 coarsest .. 2 full resolution) with a fresh
 * threshold: threshold_out[P], counts_out[P][2] = n_valid, n_in, cost_out[P], sums_out[P][44] = the upper triangle of JtJ
 * row by row (36) then Jte (8) over the inliers, J the derivative of the prediction.  threshold and
 * counts are exact; cost and sums are float64 sums in another order than direct.py's (relative 1e-9 of the sums of absolute
 * terms).  Any output pointer may be NULL. */
GME_API int gme_seq_direct_eval(gme_seq *seq, int frame_distance, int level, const double *params_in, double outlier_fraction,
                                double *threshold_out, int64_t *counts_out, double *cost_out, double *sums_out);
/* Gauss-Newton with step halving (at most 4 halvings, at most max_iters steps per level, a level ends when a step moves no
 * corner by more than 1e-3 level pixels) over levels 0 -> 1 -> 2 from init[P][8] (full resolution), every launch queued in
 * this call, one wait -> params_out[P][8], flags_out[P]: 1 singular / ill-conditioned system, 2 fewer than a quarter of a
 * level's pixels valid, 4 d <= 0 at a frame corner, 8 no improvement over init at full resolution, 16 max_iters reached at
 * level 2 (informational).  Under 1, 2, 4 or 8 params_out is init.  Deterministic; a pair's result does not depend on the
 * other pairs of the call.  0 <= outlier_fraction < 1, 1 <= max_iters <= 1000. */
GME_API int gme_seq_refine_projective(gme_seq *seq, int frame_distance, const double *init, double outlier_fraction,
                                      int max_iters, double *params_out, int32_t *flags_out);
/* Dense compensation under params[P][8]: comp[v][u] = floor(bilinear(prev)(u', v') + 0.5) at valid pixels, prev[v][u]
 * elsewhere (the reference keeps the previous frame's pixel, motion.py:289-321); the frames are read back with
 * gme_seq_read_compensated(_range); sse_out[P] = sum (cur - comp)^2 (may be NULL). */
GME_API int gme_seq_compensate_projective(gme_seq *seq, int frame_distance, const double *params, int64_t *sse_out);
/* Opt-in one-call form of begin_fit -> solve -> fit(2) -> solve -> compensate with the two 3x3 solves of
 * motion.py:262-264,280-282 on the device: one host round trip per estimate instead of three.  LAPACK's last bits are not
 * reproduced.  With m_k = (1, h-1, w-1) over the H/bs x W/bs field and S = |p0| + |p1| (h-1) + |p2| (w-1) over the three terms
 * of one displacement, every parameter of a pair whose flags_out[p] is 0 satisfies |p_dev - p_host| m_k <= 1e-10 max(1, S)
 * against the staged path's (motion.py:109-136), and its model fields, masks, compensated frame (results.py:52-59) and
 * sse_out[p] (may be NULL) are bit-equal to that path's.  A non-zero flag -- bit 1 / 2: a model displacement within
 * 1e-9 max(1, S) of a rounding tie at level 2 / in the final field; bit 4: a singular system (numpy.linalg.LinAlgError
 * upstream, motion.py:262); bit 8: an ill-conditioned one (below) -- tells the caller to redo that pair through the staged
 * calls.  Split-phase like them (gme_seq_set_split_phase). */
/* The device solve by itself: sums[P][15] = F (9, row-major) | Sx | Sy -> params_out[P][6] (motion.py:262-286; first
 * components doubled if `project`, motion.py:191-207) and flags_out[P].  Both systems are Jacobi-equilibrated and solved by
 * Gaussian elimination with partial pivoting.  bit 1: a displacement of the h x w model field of those parameters
 * (motion.py:139-157) within 1e-9 max(1, S) of k + 0.5, or |d| >= 30000, or NaN; bit 4: singular (a non-positive diagonal
 * entry or a zero pivot); bit 8: ill-conditioned (min / max |pivot| of the equilibrated system below 3e-5, as in
 * gme_solve_model2_sums).  The parameters of an unflagged pair meet the bound above.  Host pointers. */
GME_API int gme_solve_fit_sums(gme_ctx *ctx, const double *sums, int pairs, int project, int h, int w, double *params_out,
                       int32_t *flags_out);
GME_API int gme_seq_gme_device_solve(gme_seq *seq, int frame_distance, int bbme_block_size, int procedure, int search_window,
                             double outlier_fraction, double *params_out, int64_t *sse_out, int32_t *flags_out);


/* Split-phase form of the three calls above (no counterpart in the reference, whose stages are plain function calls,
 * motion.py:109-136; this is how ONE host thread keeps several streams busy).  With the switch on,
 * gme_seq_gme_begin / gme_seq_gme_fit / gme_seq_compensate return as soon as their work is queued; their output
 * buffer (page-locked: gme_host_alloc) is valid after gme_seq_wait, which waits for the result of the last such call
 * only -- the level search queued behind it keeps running.  gme_sync still drains the stream and reports walk
 * overruns.  gme_seq_upload is split-phase too: it returns with its copies queued on the context's stream, and the
 * host frames must stay untouched until a later gme_seq_wait / gme_sync returns -- how sequence.estimate_stream keeps the
 * link busy with chunk k + 1 of a video in host memory (results.py:41-50, utils.py:9-31) while chunk k is estimated. */
GME_API int gme_seq_set_split_phase(gme_seq *seq, int on);
GME_API int gme_seq_wait(gme_seq *seq);
/* 1: the result of the last split-phase call has arrived (gme_seq_wait would not block), 0: not yet, < 0: error */
GME_API int gme_seq_poll(gme_seq *seq);

/* Video stabilization (host definition stabilize.py).  Blocking calls on the resident frames.
 * Out frame first+k = frames[first+k] warped by params[k][8]: output pixel (u, v) samples the frame at direct.warp(params[k],
 * u, v) bilinearly, rounded to nearest, where that point lies in the frame; elsewhere border 0 (constant) writes `fill`,
 * border 1 (replicate) clamps the point into the frame first.  valid_out[count] (may be NULL): the in-frame samples per
 * frame.  Output kept in the sequence (allocated on first use, N_cap frames).  A range outside [0, N), a bad border or
 * fill, or a read of warped frames that were never written is GME_ERR_ARG. */
GME_API int gme_seq_warp_frames(gme_seq *seq, int first, int count, const double *params, int border, int fill,
                                int64_t *valid_out);
GME_API int gme_seq_read_warped_range(gme_seq *seq, int first, int count, uint8_t *out);
/* sse_out[k] = sum (f[first+k+1] - f[first+k])^2, k < count; warped 0: the resident frames, 1: the warped ones */
GME_API int gme_seq_frame_sse(gme_seq *seq, int warped, int first, int count, int64_t *sse_out);

/* Full-frame stabilization (host definition stabilize.warp_fill): the border of a stabilized frame filled
 * from what neighbouring frames saw.  Output pixel (u, v) of frame first+k walks its n_cand candidates in order: candidate j is
 * frame sources[k][j] (an absolute index of the resident frames, or -1: skipped) sampled at direct.warp(warps[k][j], u, v).  The
 * first candidate whose point lies in its frame (gme_seq_warp_frames' test) gives the pixel, bilinear and rounded to nearest.
 * Where none does, the pixel follows `border` / `fill` as gme_seq_warp_frames does for candidate 0, which must be a frame.
 * frames_out[count][H][W]; source_out[count][H][W] the winning j per pixel, 255 where there is none; valid_out[count] the pixels
 * won by candidate 0, filled_out[count] those won by a later one; sse_out[count - 1] the squared errors of consecutive output
 * frames.  Every output pointer may be NULL.
 * One blocking call, also in split-phase mode, that computes and returns: it works in buffers of its own and keeps nothing, so
 * the warped frames of gme_seq_warp_frames and every other kept result stay as they were.  A range outside [0, N), n_cand
 * outside 1 .. 17, a source outside -1 .. N-1, sources[k][0] < 0, or a bad border or fill is GME_ERR_ARG. */
GME_API int gme_seq_warp_fill(gme_seq *seq, int first, int count, int n_cand, const int32_t *sources, const double *warps,
                              int border, int fill, uint8_t *frames_out, uint8_t *source_out, int64_t *valid_out,
                              int64_t *filled_out, int64_t *sse_out);

/* Background mosaic and moving-object masks (host definition mosaic.py).  Blocking calls on the
 * resident frames; sprite, counts and masks are kept in the sequence (allocated on first use).
 * gme_seq_mosaic: canvas pixel (x, y) of the Hc x Wc canvas with origin (ox, oy) samples frame first+k at direct.warp(
 *   inv_warps[k], x + ox, y + oy) where that point lies in the frame (usable[k] != 0; NULL: every frame); the sample is the
 *   bilinear value rounded to nearest.  count[y][x] = number of samples, sprite[y][x] = their lower median (rank
 *   (count - 1) / 2 in ascending order), `fill` where there is none.  cull 1 skips, per 64-pixel row segment, the frames
 *   whose footprint provably misses it (the result is the same bytes); 0 samples every frame everywhere.
 * gme_seq_moving_masks: frame pixel (u, v) of frame first+k is compared with the sprite sampled at direct.warp(warps[k], u,
 *   v) - (ox, oy), known where that point lies in the canvas and its four taps have count >= min_count; mask = 1 where the
 *   pixel is known and the residuals |frame - background| of the known pixels of its 3x3 neighbourhood sum to more than
 *   threshold times their number.  One byte per pixel (0 / 1); known_out / moving_out [count] (may be NULL) count the
 *   known and the mask pixels per frame.  A frame with usable[k] == 0 gets an all-zero mask and zero counts.
 * A range outside [0, N), more than 65535 frames, a canvas of more than 2^31 - 1 pixels, a fill or threshold outside
 * 0 .. 255, min_count < 1, masks before a mosaic, or a read of what was never written is GME_ERR_ARG. */
GME_API int gme_seq_mosaic(gme_seq *seq, int first, int count, const double *inv_warps, const uint8_t *usable, int ox, int oy,
                           int Hc, int Wc, int fill, int cull);
GME_API int gme_seq_read_mosaic(gme_seq *seq, uint8_t *sprite, uint16_t *count);
GME_API int gme_seq_moving_masks(gme_seq *seq, int first, int count, const double *warps, const uint8_t *usable, int ox, int oy,
                                 int threshold, int min_count, int64_t *known_out, int64_t *moving_out);
GME_API int gme_seq_read_masks_range(gme_seq *seq, int first, int count, uint8_t *out);

/* Quarter-pel block matching (host definition subpel.py).  A quarter-pel field is int32[h][w][2] in
 * units of 1/4 pixel (4 * mf is the integer field mf); everything is integer and equals the host definition bit for bit.
 * The block of an image at origin (X, Y) in quarter units: x0 = X >> 2, fx = X & 3 (floor), the same for y; inside iff x0 >= 0,
 * y0 >= 0, x0 + bs - 1 + (fx != 0) <= W - 1 and y0 + bs - 1 + (fy != 0) <= H - 1; pixel = ((4-fx)(4-fy) p00 + fx(4-fy) p01 +
 * (4-fx) fy p10 + fx fy p11 + 8) >> 4.
 * gme_subpel_u8: one pair on host buffers.  From 4 * mf_in[i][j] and its cost against the anchor block of `prev` (sum |d|
 *   for pnorm 0, sum d^2 for 1), levels >= 1 tries the eight candidates at +-2 quarter units (column offset in the outer loop),
 *   levels == 2 then the eight at +-1 around the half-pel winner; candidates that are not inside are skipped, only a strictly
 *   smaller cost replaces the best.  A block whose integer match is not inside keeps 4 * mf_in and gets cost -1.
 *   qmf_out int32[H/bs][W/bs][2], cost_out int64[H/bs][W/bs].
 * gme_seq_subpel: the same for every pair of the field the last gme_seq_bbme left, kept in the sequence (allocated on first
 *   use); GME_ERR_STATE if there is no such field or it was made with another frame distance or block size.
 * gme_seq_read_qmv: pairs first_pair .. first_pair + count - 1 of it; either output may be NULL.  GME_ERR_STATE before any
 *   gme_seq_subpel, after new frame data or after the next block-matching call; gme_seq_compensate_qpel likewise.
 * gme_seq_compensate_qpel: with the refined field, block (i, j) of compensated frame k becomes the interpolated block of
 *   frame k at (4 j bs - q0, 4 i bs - q1) where that block is inside, elsewhere (and beyond the last whole block) the copy of
 *   frame k; written into the sequence's compensated frames (gme_seq_read_compensated_range reads them); sse_out[pairs] (may be
 *   NULL) = exact squared error against frame k + frame_distance.
 * Blocking calls.  levels outside 0 .. 2, a bad norm or block size, or a pair range outside the field is GME_ERR_ARG. */
GME_API int gme_subpel_u8(gme_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int H, int W, int stride, int block_size,
                          int pnorm, int levels, const int32_t *mf_in, int32_t *qmf_out, int64_t *cost_out);
GME_API int gme_seq_subpel(gme_seq *seq, int frame_distance, int block_size, int pnorm, int levels);
GME_API int gme_seq_read_qmv(gme_seq *seq, int first_pair, int count, int32_t *qmf_out, int64_t *cost_out);
GME_API int gme_seq_compensate_qpel(gme_seq *seq, int frame_distance, int block_size, int64_t *sse_out);

/* Hierarchical block matching (host definition hier.py): a coarse-to-fine search over the pyramid, one
 * kernel for all levels; integer throughout and equal to hier.search bit for bit.  levels in 1 .. 3: the search starts at
 * pyramid level s = 3 - levels and ends at level 2, the frame.  The block of level l has side b_l = block_size >> (2 - l);
 * block (i, j), i < H / block_size, j < W / block_size, has its origin at (i b_l, j b_l) of level l.  Its centre is (0, 0) at
 * level s and twice its own vector of level l - 1 below, clamped per component so that the displaced block lies inside the
 * level.  The centre is scored first; then the offsets in [-R, R]^2 around it (R = coarse_window at level s, radius below;
 * column offset in the outer loop, ascending), skipping blocks that are not inside the level; only a strictly smaller cost
 * (sum |d| for pnorm 0, sum d^2 for 1) replaces the best.  Vectors reach coarse_window * 2^(levels-1) + radius * (2^(levels-1) - 1).
 * gme_hier_u8: one pair on host buffers, the pyramids built on the device; mf_out int32[H/bs][W/bs][2] is the level-2 field,
 *   cost_out int64[H/bs][W/bs] its costs (may be NULL).
 * gme_seq_hier: every pair of the resident sequence (the pyramids are built if they are stale).  The level-2 field becomes the
 *   sequence's motion field with this block size and frame distance, as after gme_seq_bbme: gme_seq_read_mv, gme_seq_subpel,
 *   gme_seq_read_qmv and gme_seq_compensate_qpel work on it, and an earlier quarter-pel result is no longer valid.
 * gme_seq_read_hier: field and costs of pairs first_pair .. first_pair + count - 1 at any level the last gme_seq_hier used (either
 *   output may be NULL); another level is GME_ERR_ARG; GME_ERR_STATE before any gme_seq_hier, after new frame data or after
 *   another block-matching call.
 * Blocking calls, also in split-phase mode (as gme_seq_subpel).  GME_ERR_ARG unless block_size % 2^(levels-1) == 0,
 * block_size >> (levels - 1) >= 4, block_size <= 64, 0 <= coarse_window <= 8 and 0 <= radius <= 3.  gme_last_bbme_info names the
 * kernel instance: k_hier<16,3>, k_hier<32,3>, k_hier<64,3>, or k_hier<0,0> (block size and levels at run time). */
GME_API int gme_hier_u8(gme_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int H, int W, int stride, int block_size,
                        int coarse_window, int radius, int pnorm, int levels, int32_t *mf_out, int64_t *cost_out);
GME_API int gme_seq_hier(gme_seq *seq, int frame_distance, int block_size, int coarse_window, int radius, int pnorm, int levels);
GME_API int gme_seq_read_hier(gme_seq *seq, int level, int first_pair, int count, int32_t *mf_out, int64_t *cost_out);

/* Variable-block-size motion (host definition vbs.py): a quadtree over the blocks of an integer motion
 * field, one kernel for the whole tree; integer throughout and equal to vbs.tree byte for byte.  block_size B is the side of
 * the root blocks (the block size of the input field), depth D in 0 .. 2, radius r in 0 .. 3, pnorm 0 (sum |d|) or 1 (sum d^2),
 * penalty in 0 .. 2^30.  Root (i, j), i < H / B, j < W / B, has its origin at (j B, i B) and the vector v = mf[i][j].  If its
 * displaced block does not lie entirely in the frame it is a leaf of depth 0 with cost -1 whose cells carry v (the rule of
 * gme_subpel_u8); otherwise its own cost c is the cost at v.  A node of depth d < D has four children of half its side, child k
 * at row k >> 1 and column k & 1.  A child is searched around its parent's vector: the centre is scored first; then the offsets
 * in [-r, r]^2 without it (column offset in the outer loop, ascending), skipping blocks that are not inside the frame; only a
 * strictly smaller cost replaces the best.  Each child is a node of depth d + 1 with its winning vector and cost, resolved
 * first.  With S = penalty + sum of the children's F the node splits iff S < c (a tie does not split), and F = min(c, S); a
 * node of depth D is a leaf with F = c.  Every sum of a decision stays below 2^31.
 * Result per pair, g = B >> D: leaf int32[(H/B) 2^D][(W/B) 2^D][2], every g x g cell carries the vector of the leaf that covers
 * it; depth uint8 of the same grid, the depth of that leaf; cost int64[H/B][W/B], F of the root (penalties included) or -1.
 * gme_vbs_u8: one pair on host buffers, mf_in int32[H/B][W/B][2]; depth_out and cost_out may be NULL.
 * gme_seq_vbs: every pair of the field the last gme_seq_bbme or gme_seq_hier left; GME_ERR_STATE if there is no such field or it
 *   was made with another frame distance or block size.  The result is kept in the sequence (allocated on first use) and does
 *   not replace the sequence's motion field; it is no longer valid after new frame data or the next block-matching call.
 * gme_seq_read_vbs: pairs first_pair .. first_pair + count - 1 of it; any output may be NULL; a range outside the field is
 *   GME_ERR_ARG, GME_ERR_STATE where there is no valid result.
 * gme_seq_compensate_vbs: the per-pixel rule of the integer fields at the leaf size g: pixel (a, b) of every whole cell of
 *   compensated frame k becomes pixel (a - d1, b - d0) of frame k where that lies in the frame, elsewhere (and beyond the last
 *   whole cell) the pixel is kept; written into the sequence's compensated frames (gme_seq_read_compensated_range reads them);
 *   sse_out[pairs] (may be NULL) = exact squared error against frame k + frame_distance.
 * Blocking calls, also in split-phase mode.  GME_ERR_ARG unless B % 2^D == 0, B >> D >= 4, B <= 64 and depth, radius, pnorm and
 * penalty lie in their ranges.  gme_last_bbme_info names the kernel instance: k_vbs<16,2>, k_vbs<32,2>, or k_vbs<0,0> (block
 * size and depth at run time). */
GME_API int gme_vbs_u8(gme_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int H, int W, int stride, int block_size, int depth,
                       int radius, int pnorm, int penalty, const int32_t *mf_in, int32_t *leaf_out, uint8_t *depth_out,
                       int64_t *cost_out);
GME_API int gme_seq_vbs(gme_seq *seq, int frame_distance, int block_size, int depth, int radius, int pnorm, int penalty);
GME_API int gme_seq_read_vbs(gme_seq *seq, int first_pair, int count, int32_t *leaf_out, uint8_t *depth_out, int64_t *cost_out);
GME_API int gme_seq_compensate_vbs(gme_seq *seq, int frame_distance, int block_size, int64_t *sse_out);

/* Bidirectional block prediction (host definition bipred.py): a block of the frame `mid` is predicted from
 * the frame before it, from the frame after it, or from the rounded average of both; integer throughout and equal to
 * bipred.decide and bipred.predict byte for byte.  block_size B in 4 .. 64, radius r in 0 .. 2, rounds in 0 .. 2, pnorm 0
 * (sum |d|) or 1 (sum d^2), penalty in 0 .. 2^30.  Block (i, j), i < H / B, j < W / B, has its origin at (j B, i B); f0[i][j]
 * (column, row) says where it is found in `past`, f1[i][j] where in `next` (the fields of a search with `mid` as the previous
 * and `past`, or `next`, as the current frame).  c0 is the cost against `past` at f0, c1 against `next` at f1, each unavailable
 * (-1) if the displaced block does not lie entirely in the frame.  cb exists only when both do: the cost of the predictor
 * (p + n + 1) >> 1 at (f0, f1), then refined by `rounds` rounds of two passes.  Pass 1 holds the `next` vector and tries the
 * `past` vector at its value at the start of the pass plus the offsets in [-r, r]^2 without the centre (column offset in the
 * outer loop, ascending), skipping blocks that are not inside the frame; only a strictly smaller cost replaces the best.  Pass
 * 2 holds the new `past` vector and does the same for the `next` vector.  Decision: (mode 0, c0), (mode 1, c1), (mode 2,
 * cb + penalty) in that order, unavailable ones left out, only a strictly smaller value replaces the best; with none
 * available, mode 3 and cost -1.  Every sum of a decision stays below 2^31.
 * Result per target: mode uint8[H/B][W/B]; v0, v1 int32[H/B][W/B][2], the refined pair where mode is 2 and the inputs
 * elsewhere; cost int64[H/B][W/B], the chosen value (penalty included) or -1; costs int64[H/B][W/B][3] = c0, c1, cb (without
 * the penalty), -1 where unavailable.
 * Prediction: a block of mode 0 is the `past` block at v0, of mode 1 the `next` block at v1, of mode 2 their rounded average;
 * a block of mode 3 and every pixel beyond the last whole block is the co-located pixel of `past`.
 * gme_bipred_u8: one triple on host buffers with the fields f0, f1 int32[H/B][W/B][2]; every output but mode_out may be NULL;
 *   pred_out uint8[H][W] (tight) is the predicted frame and *sse_out its exact squared error against `mid`.
 * gme_seq_bipred: the targets t = frame_distance .. N - 1 - frame_distance of the sequence, T = N - 2 frame_distance of them
 *   (GME_ERR_ARG unless N >= 2 frame_distance + 1), target k predicted from the frames t - frame_distance and
 *   t + frame_distance.  It runs both searches itself (the arguments and rules of gme_seq_bbme) into fields of its own and
 *   then the decision; the sequence's motion field and the quarter-pel, hierarchical and variable-block-size results stay as
 *   they were.  The result is kept in the sequence (allocated on first use) until new frame data.
 * gme_seq_read_bipred: targets first .. first + count - 1 of it; any output may be NULL; a range outside [0, T) is GME_ERR_ARG,
 *   GME_ERR_STATE where there is no valid result.
 * gme_seq_predict_bipred: the T predicted frames into the sequence's compensated frames (gme_seq_read_compensated_range reads
 *   them), sse_out[T] (may be NULL) = exact squared error of each against its target frame.
 * Blocking calls, also in split-phase mode.  gme_last_bbme_info names the kernel instance: k_bipred<16>, k_bipred<32>, or
 * k_bipred<0> (block size at run time). */
GME_API int gme_bipred_u8(gme_ctx *ctx, const uint8_t *past, const uint8_t *mid, const uint8_t *next, int H, int W, int stride,
                          int block_size, int radius, int rounds, int pnorm, int penalty, const int32_t *f0, const int32_t *f1,
                          uint8_t *mode_out, int32_t *v0_out, int32_t *v1_out, int64_t *cost_out, int64_t *costs_out,
                          uint8_t *pred_out, int64_t *sse_out);
GME_API int gme_seq_bipred(gme_seq *seq, int frame_distance, int block_size, int search_window, int procedure, int pnorm, int radius,
                           int rounds, int penalty);
GME_API int gme_seq_read_bipred(gme_seq *seq, int first, int count, int32_t *f0_out, int32_t *f1_out, uint8_t *mode_out,
                                int32_t *v0_out, int32_t *v1_out, int64_t *cost_out, int64_t *costs_out);
GME_API int gme_seq_predict_bipred(gme_seq *seq, int64_t *sse_out);

/* Global motion compensation (host definition gmc.py): a block of the frame `cur` is predicted from the
 * frame `ref` either by the pair's camera warp, pixel by pixel, or by the block its own integer vector points at; equal to
 * gmc.decide and gmc.predict byte for byte.  block_size B in 4 .. 64, pnorm 0 (sum |d|) or 1 (sum d^2), penalty in 0 .. 2^30.
 * h[8] is a warp in the convention of gme_seq_refine_projective: pixel (u, v) of `cur` samples `ref` at
 * u' = (h0 u + h1 v + h2) / d, v' = (h3 u + h4 v + h5) / d, d = h6 u + h7 v + 1.  It is usable when it is finite and d > 0 at
 * the four corners of the frame; an unusable warp is no error, only no block of that pair has a global candidate.  Block
 * (i, j), i < H / B, j < W / B, has its origin at (j B, i B); f[i][j] (column, row) says where it is found in `ref` (the field
 * of a search with `cur` as the previous and `ref` as the current frame).
 * The global predictor pixel is floor(bilinear(ref)(u', v') + 0.5), gme_seq_compensate_projective's pixel; it exists where
 * 0 <= u' <= W - 1 and 0 <= v' <= H - 1.  cg is the cost of the block's global pixels against the `cur` block, unavailable (-1)
 * unless the warp is usable and all B^2 pixels exist; cl the cost of the `ref` block at f, unavailable unless the displaced
 * block lies entirely in the frame.  Decision: (mode 0 GLOBAL, cg), (mode 1 LOCAL, cl + penalty) in that order, unavailable
 * ones left out, only a strictly smaller value replaces the best (GLOBAL wins ties); with none available, mode 2 and cost -1.
 * Every sum of a decision stays below 2^31.
 * Result per pair: mode uint8[H/B][W/B]; cost int64[H/B][W/B], the chosen value (penalty included) or -1; costs
 * int64[H/B][W/B][2] = cg, cl (without the penalty), -1 where unavailable.
 * Prediction: a block of mode 0 is its global pixels, of mode 1 the `ref` block at f; a block of mode 2 and every pixel beyond
 * the last whole block is the co-located pixel of `ref`.
 * gme_gmc_u8: one pair on host buffers with the warp h and the field f int32[H/B][W/B][2]; every output but mode_out may be
 *   NULL; pred_out uint8[H][W] (tight) is the predicted frame and *sse_out its exact squared error against `cur`.
 * gme_seq_gmc: the P = N - frame_distance pairs of the sequence, pair k predicting frame k + frame_distance from frame k under
 *   h[k] (h is double[P][8], the pair convention of gme_seq_refine_projective).  It runs the search itself (frame
 *   k + frame_distance looked for in frame k; the arguments and rules of gme_seq_bbme) into a field of its own and then the
 *   decision; the sequence's motion field and the quarter-pel, hierarchical, variable-block-size and bidirectional results
 *   stay as they were.  The result is kept in the sequence (allocated on first use) until new frame data.
 * gme_seq_read_gmc: pairs first .. first + count - 1 of it; any output may be NULL; usable_out uint8[count] says which warps
 *   were usable; a range outside [0, P) is GME_ERR_ARG, GME_ERR_STATE where there is no valid result.
 * gme_seq_predict_gmc: the P predicted frames into the sequence's compensated frames (gme_seq_read_compensated_range reads
 *   them), sse_out[P] (may be NULL) = exact squared error of each against the frame it predicts.
 * Blocking calls, also in split-phase mode.  gme_last_bbme_info names the kernel instance: k_gmc<16>, k_gmc<32>, or k_gmc<0>
 * (block size at run time). */
GME_API int gme_gmc_u8(gme_ctx *ctx, const uint8_t *ref, const uint8_t *cur, int H, int W, int stride, int block_size, int pnorm,
                       int penalty, const double *h, const int32_t *f, uint8_t *mode_out, int64_t *cost_out, int64_t *costs_out,
                       uint8_t *pred_out, int64_t *sse_out);
GME_API int gme_seq_gmc(gme_seq *seq, int frame_distance, int block_size, int search_window, int procedure, int pnorm, int penalty,
                        const double *h /* [P][8] */);
GME_API int gme_seq_read_gmc(gme_seq *seq, int first, int count, int32_t *f_out, uint8_t *mode_out, int64_t *cost_out,
                             int64_t *costs_out, uint8_t *usable_out);
GME_API int gme_seq_predict_gmc(gme_seq *seq, int64_t *sse_out);

/* ---------------------------------------------------------------------------
 * Vector propagation search (csrc/bbme_prop.hip; host definition: propagate.py): a block scores the
 * vectors it inherits -- its own, its eight neighbours', the previous pair's, the camera's and zero -- keeps the cheapest and
 * refines it by one pixel per pass, for `rounds` rounds that each read only the field of the round before.  All integer,
 * byte-equal to propagate.search.  block_size 4 .. 64, pnorm 0 (sum |d|) or 1 (sum d^2), rounds 1 .. 4, steps 0 .. 4; anything
 * else is GME_ERR_ARG.
 * gme_prop_u8: one pair on the prior field f int32[H / bs][W / bs][2], the previous pair's field t and the camera field g (same
 *   shape, either may be NULL) -> mf_out of that shape, cost_out int64[H / bs][W / bs] and source_out uint8[H / bs][W / bs] (may
 *   be NULL): class of the winning candidate (0 own, 1 spatial, 2 temporal, 3 camera, 4 zero), plus 8 where a pass moved it.
 * gme_seq_prop: every pair of the sequence.  The prior is the field the last gme_seq_bbme, gme_seq_hier or gme_seq_prop left;
 *   GME_ERR_STATE if there is none or it was made with another frame distance or block size.  With temporal != 0, pair k >= 1
 *   gets the PRIOR field of pair k - 1 as t (not the propagated one: the pairs stay independent and share one launch per
 *   round); pair 0 has none.  g int32[P][H / bs][W / bs][2] or NULL.  The result becomes the sequence's motion field
 *   (gme_seq_read_mv, gme_seq_subpel, gme_seq_vbs and a further gme_seq_prop work on it); earlier quarter-pel, hierarchical
 *   and variable-block-size results are no longer valid, the bidirectional and global-motion-compensation results stay.
 * gme_seq_read_prop: pairs first_pair .. first_pair + count - 1 of it; any output may be NULL; a range outside [0, P) is
 *   GME_ERR_ARG; GME_ERR_STATE before any gme_seq_prop, after new frame data or after another block-matching call.
 * Blocking calls, also in split-phase mode.  gme_last_bbme_info names the kernel instance: k_prop<16>, k_prop<32>, or k_prop<0>
 * (block size at run time). */
GME_API int gme_prop_u8(gme_ctx *ctx, const uint8_t *prev, const uint8_t *cur, int H, int W, int stride, int block_size, int pnorm,
                        int rounds, int steps, const int32_t *f, const int32_t *t /* may be NULL */, const int32_t *g /* may be NULL */,
                        int32_t *mf_out, int64_t *cost_out /* may be NULL */, uint8_t *source_out /* may be NULL */);
GME_API int gme_seq_prop(gme_seq *seq, int frame_distance, int block_size, int pnorm, int rounds, int steps, int temporal,
                         const int32_t *g /* [P][H/B][W/B][2] or NULL */);
GME_API int gme_seq_read_prop(gme_seq *seq, int first_pair, int count, int32_t *mf_out, int64_t *cost_out, uint8_t *source_out);

/* ---------------------------------------------------------------------------
 * Motion-compensated frame interpolation (csrc/bbme_interp.hip; host definition: interp.py): the frame
 * halfway between `past` and `next`.  Block (i, j) of the new frame takes the vector v = (vx, vy) within +-search_window that
 * minimises J(v) = D(v) + bias (|vx| + |vy|), D the sum of |d| (pnorm 0) or d^2 (pnorm 1) between `past` at origin - v and
 * `next` at origin + v, coordinates clamped to the frame (border replication); the centre first, then column offset outer, both
 * ascending, only a strictly smaller J replaces the incumbent.  A pixel of the new frame is the rounded average of the two
 * displaced pixels; beyond the last whole block v = 0.  All integer, byte-equal to interp.search and interp.interpolate.
 * block_size 4 .. 64 (H >= block_size and W >= block_size), search_window 0 .. 8, pnorm 0 or 1, bias 0 .. 2^16; anything else is
 * GME_ERR_ARG.
 * gme_interp_u8: one pair on host buffers -> mv_out int32[H/B][W/B][2], cost_out (J) and dist_out (D of the winner)
 *   int64[H/B][W/B], frame_out uint8[H][W] (tight), *sse_out = exact squared error of the interpolated frame against `truth`,
 *   the true middle frame, or -1 where truth is NULL.  Any output may be NULL.
 * gme_seq_interp: the pairs (k, k + frame_distance), k = first_pair .. first_pair + count - 1, of the P = N - frame_distance
 *   pairs of the sequence (GME_ERR_ARG unless 1 <= frame_distance < N and the range lies in [0, P)) -> mv_out
 *   int32[count][H/B][W/B][2], cost_out and dist_out int64[count][H/B][W/B], frames_out uint8[count][H][W] (tight), sse_out[count]
 *   = exact squared error of each interpolated frame against frame k + frame_distance / 2 for an even frame_distance, -1 for an
 *   odd one.  Any output may be NULL.  It computes and returns in one call, in buffers of its own that live as long as the
 *   call: it keeps no result and leaves everything the sequence holds as it was (the motion field and what was derived from it,
 *   the bidirectional and global-motion-compensation results, the compensated planes), so it is no part of the result lifetimes
 *   above.
 * Blocking calls, also in split-phase mode.  gme_last_bbme_info names the kernel instance: k_interp<16>, k_interp<32>, or
 * k_interp<0> (block size at run time). */
GME_API int gme_interp_u8(gme_ctx *ctx, const uint8_t *past, const uint8_t *next, const uint8_t *truth /* may be NULL */, int H, int W,
                          int stride, int block_size, int search_window, int pnorm, int bias, int32_t *mv_out, int64_t *cost_out,
                          int64_t *dist_out, uint8_t *frame_out, int64_t *sse_out);
GME_API int gme_seq_interp(gme_seq *seq, int frame_distance, int block_size, int search_window, int pnorm, int bias, int first_pair,
                           int count, int32_t *mv_out, int64_t *cost_out, int64_t *dist_out, uint8_t *frames_out, int64_t *sse_out);

/* ---------------------------------------------------------------------------
 * Frame interpolation at any phase, for rate conversion and slow motion (csrc/bbme_retime.hip; host
 * definition: retime.py): the frame at phase n / d between `past` (phase 0) and `next` (phase 1), 1 <= n < d <= 64 after n / d
 * has been reduced.  A vector V = (Vx, Vy) within +-search_window, in whole pixels, is how far content moves from `past` to
 * `next`.  Per component and in quarter pixels `past` is read at a(V) = -floor((8 n V + d) / (2 d)) and `next` at b(V) = a(V) +
 * 4 V, through the four-tap sampler of the quarter-pel section with every tap clamped to the frame.  Block (i, j) takes the V
 * that minimises J(V) = D(V) + bias (|Vx| + |Vy|), D the sum of |P - N| (pnorm 0) or (P - N)^2 (pnorm 1); the centre first, then
 * column offset outer, both ascending, only a strictly smaller J replaces the incumbent.  A pixel of the new frame is
 * ((d - n) P + n N + d / 2) / d, rounded down; beyond the last whole block V = 0.  All integer, byte-equal to retime.search and
 * retime.interpolate.  block_size 4 .. 64 (H >= block_size and W >= block_size), search_window 0 .. 16, pnorm 0 or 1, bias
 * 0 .. 2^16; anything else is GME_ERR_ARG.
 * gme_retime_u8: one pair at one phase on host buffers -> mv_out int32[H/B][W/B][2], cost_out (J) and dist_out (D of the
 *   winner) int64[H/B][W/B], frame_out uint8[H][W] (tight), *sse_out = exact squared error of the made frame against `truth`,
 *   the true frame at that time, or -1 where truth is NULL.  Any output may be NULL.
 * gme_retime_clip_u8: a host clip frames uint8[n_frames][H][stride] at a step of step_num / step_den input frames per output
 *   (input rate over output rate; both >= 1).  Output m of M = ((n_frames - 1) step_den) / step_num + 1 lies at k = (m step_num)
 *   / step_den, r = (m step_num) % step_den: frame k itself for r = 0, else the pair (k, k + 1) at phase r / step_den, reduced
 *   (a denominator above 64 anywhere in the schedule is GME_ERR_ARG).  The outputs first_out .. first_out + count - 1 (a range
 *   outside [0, M) is GME_ERR_ARG) -> frames_out uint8[count][H][W] (tight), mv_out int32[count][H/B][W/B][2], cost_out and
 *   dist_out int64[count][H/B][W/B]; a copy comes out as the frame itself with zero vectors and costs.  Any output may be NULL.
 *   Every input frame an output needs is uploaded once; the launches carry at most the per-launch limit of outputs
 *   (GME_MAX_GRID_PAIRS lowers it); the call works in buffers of its own and keeps nothing.
 * Blocking calls.  gme_last_bbme_info names the kernel instance: k_retime<16>, k_retime<32>, or k_retime<0> (block size at run
 * time). */
GME_API int gme_retime_u8(gme_ctx *ctx, const uint8_t *past, const uint8_t *next, const uint8_t *truth /* may be NULL */, int H, int W,
                          int stride, int block_size, int search_window, int pnorm, int bias, int n, int d, int32_t *mv_out,
                          int64_t *cost_out, int64_t *dist_out, uint8_t *frame_out, int64_t *sse_out);
GME_API int gme_retime_clip_u8(gme_ctx *ctx, const uint8_t *frames, int n_frames, int H, int W, int stride, int block_size,
                               int search_window, int pnorm, int bias, int step_num, int step_den, int first_out, int count,
                               uint8_t *frames_out, int32_t *mv_out, int64_t *cost_out, int64_t *dist_out);

/* ---------------------------------------------------------------------------
 * Overlapped block motion compensation (csrc/bbme_obmc.hip; host definition: obmc.py): `prev` compensated
 * by a block field, every pixel blended from the predictions of its own block and of the nearest vertical, horizontal and
 * diagonal neighbour blocks under a linear ramp, so the prediction does not jump where two neighbours disagree.  field is
 * int32[H/B][W/B][2] (column, row; sign and axes of the quarter-pel section); unit 4: whole pixels, unit 1: quarter pixels (the
 * product is formed in 64 bits).  A prediction of pixel (u, v) under the vector q is the four-tap blend of the quarter-pel
 * section at (4 u - q0, 4 v - q1) with every tap's coordinates clamped to the frame (border replication): no vector is
 * unavailable, INT32_MIN and INT32_MAX included.  With ty = 2 (v mod B) + 1 - B the vertical neighbour is the block row above
 * (ty < 0) or below, clamped to the grid, and the two rows weigh 2B - |ty| and |ty|; the same for the columns; the pixel is
 * (sum of the four weighted 8-bit predictions + 2 B^2) / (4 B^2), rounded down.  Beyond the last whole block the pixel is the
 * copy of `prev`.  All integer, byte-equal to obmc.compensate.  block_size 4 .. 64 (H >= block_size and W >= block_size), unit 1
 * or 4; anything else is GME_ERR_ARG.
 * gme_obmc_u8: one pair on host buffers -> frame_out uint8[H][W] (tight), *sse_out = exact squared error against `cur`, or -1
 *   where cur is NULL.  Either output may be NULL.
 * gme_seq_obmc: the pairs (k, k + frame_distance), k = first_pair .. first_pair + count - 1 (a range outside the field's pairs is
 *   GME_ERR_ARG) -> frames_out uint8[count][H][W] (tight), sse_out[count] = exact squared error against frame k + frame_distance.
 *   Either output may be NULL.  unit 4 takes the sequence's motion field as gme_seq_vbs takes it (the field survives new frame
 *   data; GME_ERR_STATE without a field, or for another frame distance or block size than the field's); unit 1 takes the
 *   quarter-pel field and is GME_ERR_STATE wherever gme_seq_compensate_qpel is.  It computes and returns in one call, in buffers
 *   of its own that live as long as the call: it keeps nothing, writes neither the compensated planes nor any field, and leaves
 *   every kept result readable and byte-identical, so it is no part of the result lifetimes above.
 * Blocking calls, also in split-phase mode.  gme_last_bbme_info names the kernel: k_obmc. */
GME_API int gme_obmc_u8(gme_ctx *ctx, const uint8_t *prev, const uint8_t *cur /* may be NULL */, int H, int W, int stride,
                        int block_size, const int32_t *field, int unit /* 4: whole pixels, 1: quarter pixels */,
                        uint8_t *frame_out, int64_t *sse_out);
GME_API int gme_seq_obmc(gme_seq *seq, int frame_distance, int block_size, int unit, int first_pair, int count,
                         uint8_t *frames_out, int64_t *sse_out);

/* ---------------------------------------------------------------------------
 * Motion-compensated temporal denoising (csrc/bbme_denoise.hip; host definition: denoise.py): a frame
 * averaged with R = 1 .. 4 overlapped predictions of it from neighbour frames, every pixel gated by how well its neighbourhood
 * was predicted.  With S = 9 strength (strength 1 .. 64 grey levels) and D_r the sum of |prediction_r - cur| over the pixel's
 * 3 x 3 window (both coordinates clamped to the frame), prediction r weighs w_r = max(0, S - D_r) and the pixel itself S:
 * out = (S cur + sum w_r p_r + tot / 2) / tot, tot = S + sum w_r, rounded down.  All integer, byte-equal to denoise.blend.
 * A prediction is the overlapped compensation of the section above by the NEGATED field: field r is int32[H/B][W/B][2] (column,
 * row) on the block grid of the frame being filtered and says where that frame's block is found in reference r (what
 * gme_bbme_u8 returns with the frame as `prev` and the reference as `cur`; f0 and f1 of the bidirectional section), so pixel
 * (u, v) reads the reference at (4 u + q0, 4 v + q1) quarter pixels, every tap clamped; any int32 vector is valid.  unit 4: whole
 * pixels, unit 1: quarter pixels.  R outside 1 .. 4, strength outside 1 .. 64, unit not 1 or 4, block_size outside 4 .. 64 or
 * above H or W: GME_ERR_ARG.
 * gme_denoise_u8: one frame on host buffers (refs and fields: R pointers each, all images with the row stride `stride`) ->
 *   frame_out uint8[H][W] (tight), *sse_out = exact squared error of the filtered frame against `truth`, or -1 where truth is
 *   NULL.  Either output may be NULL.
 * gme_seq_denoise: the interior targets t = radius * frame_distance + first_target + k, k < count, of a resident sequence, each
 *   with the 2 radius references t -+ d frame_distance, d = 1 .. radius (radius 1 .. 2; fewer than 2 radius frame_distance + 1
 *   frames, or a target range outside [0, N - 2 radius frame_distance), is GME_ERR_ARG; the rules of gme_seq_bbme apply to the
 *   search arguments).  Per reference it runs the named search from the target into a field of its own, with levels 1 or 2 the
 *   sub-pel refinement of the quarter-pel section, and the overlapped prediction; then the filter -> frames_out
 *   uint8[count][H][W] (tight), change_out[count] = sum (out - target)^2, the energy the filter removed.  Either output may be
 *   NULL.  It computes and returns in one call, in buffers of its own that live as long as the call: it keeps nothing, writes
 *   neither a field nor the compensated planes, and leaves every kept result readable and byte-identical, so it is no part of the
 *   result lifetimes above.
 * Blocking calls, also in split-phase mode.  gme_last_bbme_info names the kernel: k_denoise. */
GME_API int gme_denoise_u8(gme_ctx *ctx, const uint8_t *cur, const uint8_t *const *refs, const int32_t *const *fields, int R,
                           int H, int W, int stride, int block_size, int unit /* 4: whole pixels, 1: quarter pixels */,
                           int strength, const uint8_t *truth /* may be NULL */, uint8_t *frame_out, int64_t *sse_out);
GME_API int gme_seq_denoise(gme_seq *seq, int frame_distance, int block_size, int search_window, int procedure, int pnorm,
                            int radius, int levels, int strength, int first_target, int count, uint8_t *frames_out,
                            int64_t *change_out);

/* ---------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, contiguous pair ranges per rank (results.py:41-50 carries no state
 * between pairs), and ONE exchange: the all-gather of the per-pair parameter rows over RCCL / xGMI on
 * the context's stream.  The reference has no distributed code; SURVEY.md §8(e) defines this split.
 *   gme_comm_unique_id   rank 0 makes the 128-byte RCCL id; the launcher hands it to the other ranks
 *                        (file / env / socket -- before or after their contexts exist)
 *   gme_comm_init        collective over all ranks (ncclCommInitRank)
 *   gme_shard_gather     rows[n_local][k] of every rank -> out[world][n_max][k], blocks zero-padded to
 *                        n_max rows (n_max = the largest shard, the same on every rank); synchronises
 *   gme_comm_allreduce_max   element-wise max of v[n] over the ranks, in place (barrier; max-over-ranks time)
 *   gme_comm_probe       loads librccl.so and nothing else: a launcher lets every rank probe and agree BEFORE any rank
 *                        enters the collective gme_comm_init (which cannot time out), sequence.comm_init does
 *   gme_comm_info        rank and rank count as RCCL reports them (ncclCommUserRank / ncclCommCount)
 *   gme_seq_mv_summary   per-pair summary rows of the last gme_seq_bbme field, float64[P][6] = modal vector x, y (over the
 *                        vectors inside [-64, 64)^2, ties to the smaller (x+64)*128 + (y+64)), its block count, sum of
 *                        x, sum of y, checksum sum_i ((i mod 251) + 1)(3 x_i + 5 y_i) over the blocks in row-major
 *                        order -- what a sharded bbme.get_motion_field run (bbme.py:12-38 per pair, results.py:41-50 over
 *                        pairs) exchanges instead of its 10.8 kB fields; synchronises
 *   gme_seq_mv_summary_gather   the same rows all-gathered device to device: out[world][n_max][6], blocks zero-padded
 *                        to n_max >= this rank's pairs (the same on every rank); split-phase aware (gme_seq_wait)
 * ------------------------------------------------------------------------- */
GME_API int gme_comm_probe(void);
GME_API int gme_comm_info(gme_ctx *ctx, int *rank_out, int *world_out);
GME_API int gme_seq_mv_summary(gme_seq *seq, double *rows_out);
GME_API int gme_seq_mv_summary_gather(gme_seq *seq, int n_max, double *out);
GME_API int gme_comm_unique_id(char id_out[128]);
GME_API int gme_comm_init(gme_ctx *ctx, const char id[128], int rank, int world);
GME_API int gme_comm_destroy(gme_ctx *ctx);
GME_API int gme_shard_gather(gme_ctx *ctx, const double *rows, int n_local, int k, int n_max, double *out);
GME_API int gme_comm_allreduce_max(gme_ctx *ctx, double *v, int n);

#ifdef __cplusplus
}
#endif
#endif /* GME_HIP_H */
