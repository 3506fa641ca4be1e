// Internal declarations of the passes built on the core of gme_internal.h: direct projective refinement, stabilization and
// border fill, mosaic and masks, and the block-field passes.  Their launchers and argument rules, what a resident sequence
// keeps for them, and what their entry points (gme_api_passes.hip, gme_api_frames.hip) share.  No translation unit of the
// benchmarked core includes this file, so a new pass or a change to one leaves the identity of every benchmarked kernel alone
// (bench.py: COMMON_SOURCES, CONFIG_SOURCES; tests/test_host.py holds the separation).
#pragma once
#include "gme_internal.h"

// What a resident sequence keeps for the passes between calls: gme_seq::passes, made and freed with the sequence
// (passes_create, passes_destroy; gme_api_passes.hip).
struct SeqPasses {
    DevBuf<uint8_t> direct;       // gme_direct.hip: per-pair refinement state, histograms, slabs and parameters
    // stabilization (gme_stab.hip): the warped frames (N_cap, allocated by the first gme_seq_warp_frames), which of them a
    // warp has written, and N_cap rows of parameters and counts
    PlaneBuf warped;
    WrittenFrames warped_written;
    DevBuf<double> warp_params;          // [N_cap][8]
    DevBuf<unsigned long long> warp_counts;      // [N_cap] valid samples, or squared errors of gme_seq_frame_sse
    // background mosaic (gme_mosaic.hip): sprite and sample counts [Hc][pitch] of the last gme_seq_mosaic, the masks of
    // gme_seq_moving_masks (N_cap planes, allocated by its first call) with which of them were written, and N_cap rows of
    // parameters, usable flags and known / moving counts
    DevBuf<uint8_t> mosaic_sprite;       // both hold the same number of pixels
    DevBuf<uint16_t> mosaic_count;
    int mosaic_Hc = 0, mosaic_Wc = 0, mosaic_pitch = 0;
    bool mosaic_valid = false;
    PlaneBuf masks;
    WrittenFrames masks_written;
    DevBuf<double> mosaic_params;        // [N_cap][8]
    DevBuf<uint8_t> mosaic_usable;       // [N_cap]
    DevBuf<unsigned long long> mosaic_counts;    // [2][N_cap] known, moving
    // Result lifetimes of the block-field passes below, in one place: seq_field_replaced (gme_api.hip) ends what was derived from
    // `mv` through passes_field_replaced, and every writer of `mv` calls it; seq_frames_changed (new frame data, another frame
    // count) does the same through passes_frames_changed, which then ends the results that keep fields of their own.
    // quarter-pel refinement (bbme_subpel.hip): the refined field and its costs of the last gme_seq_subpel, allocated by
    // its first call; valid until seq_field_replaced
    DevBuf<int32_t> qmv;                 // [P][h][w][2], quarter units
    DevBuf<long long> qcost;             // [P][h][w]
    bool qmv_valid = false;
    // hierarchical search (bbme_hier.hip): fields of the levels above the frame and the costs of every level of the last
    // gme_seq_hier (its level-2 field is `mv`), allocated by its first call; valid until seq_field_replaced
    DevBuf<int32_t> hier_mv[2];          // [P][h][w][2] of levels 0 and 1
    DevBuf<long long> hier_cost[3];      // [P][h][w]
    int hier_levels = 0;                 // levels the last gme_seq_hier used
    bool hier_valid = false;
    // variable-block-size tree (bbme_vbs.hip): leaf field, depth map and root costs of the last gme_seq_vbs on `mv`, allocated
    // by its first call; valid until seq_field_replaced
    DevBuf<int32_t> vbs_leaf;            // [P][h << D][w << D][2]
    DevBuf<uint8_t> vbs_dmap;            // [P][h << D][w << D]
    DevBuf<long long> vbs_cost;          // [P][h][w]
    int vbs_depth = 0;                   // D of the last gme_seq_vbs
    bool vbs_valid = false;
    // bidirectional prediction (bbme_bipred.hip): both fields of gme_seq_bipred's own searches, the modes, the vector pairs and
    // the costs of its T = N - 2 fd targets, allocated by its first call; valid until seq_frames_changed.  No other call reads or
    // writes them, and gme_seq_bipred writes nothing else of the sequence.
    DevBuf<int32_t> bp_f0, bp_f1;        // [T][h][w][2]
    DevBuf<uint8_t> bp_mode;             // [T][h][w]
    DevBuf<int32_t> bp_v0, bp_v1;        // [T][h][w][2]
    DevBuf<long long> bp_cost;           // [T][h][w]
    DevBuf<long long> bp_costs;          // [T][h][w][3]
    int bp_targets = 0, bp_h = 0, bp_w = 0, bp_fd = 0, bp_bs = 0;
    bool bp_valid = false;
    // global motion compensation (bbme_gmc.hip): the field of gme_seq_gmc's own search, the warps it was given with their usable
    // flags, the modes and the costs of its P = N - fd pairs, allocated by its first call; valid until seq_frames_changed.  No other
    // call reads or writes them, and gme_seq_gmc writes nothing else of the sequence.
    DevBuf<int32_t> gm_f;                // [P][h][w][2]
    DevBuf<double> gm_h;                 // [P][8]
    DevBuf<uint8_t> gm_usable;           // [P]
    DevBuf<uint8_t> gm_mode;             // [P][h][w]
    DevBuf<long long> gm_cost;           // [P][h][w]
    DevBuf<long long> gm_costs;          // [P][h][w][2]
    int gm_pairs = 0, gm_h_blocks = 0, gm_w_blocks = 0, gm_fd = 0, gm_bs = 0;
    bool gm_valid = false;
    // vector propagation (bbme_prop.hip): the two fields the rounds of gme_seq_prop alternate between (the last one is copied
    // into `mv`), the camera field it was given, and the costs and sources of the last round, allocated by its first call;
    // valid until seq_field_replaced
    DevBuf<int32_t> prop_work[2];        // [P][h][w][2]
    DevBuf<int32_t> prop_g;              // [P][h][w][2]
    DevBuf<long long> prop_cost;         // [P][h][w]
    DevBuf<uint8_t> prop_source;         // [P][h][w]
    bool prop_valid = false;
};

// ---- gme_direct.hip: direct projective refinement ---------------------------------------------
// device blocks of the sequence's workspace for `pairs` pairs: in[P][8] (parameters the calls below read), out[P][8],
// flags[P] (refinement results), eval[P][48] = threshold, n_valid, n_in, cost, sums[44] (gme_seq_direct_eval)
struct DirectIo {
    double *in = nullptr, *out = nullptr, *eval = nullptr;
    int32_t* flags = nullptr;
};
int direct_io(gme_seq* s, int pairs, DirectIo* io);
// the whole refinement of in[] (full-resolution start) into out[] / flags[], every launch queued, no wait
int launch_direct_refine(gme_seq* s, int fd, int pairs, double outlier_fraction, int max_iters);
// one evaluation of in[] (level-`level` coordinates) with a fresh threshold into eval[]
int launch_direct_eval(gme_seq* s, int fd, int level, int pairs, double outlier_fraction);
// compensation of every pair under params[P][8] (device) into s->comp, squared errors into s->sse
int launch_compensate_proj(gme_seq* s, int fd, int pairs, const double* params);

// ---- gme_stab.hip: video stabilization -------------------------------------------------------
// frames first .. first + count - 1 of src warped by params[count][8] (device; border 0 constant fill, 1 replicate) into the
// same frames of dst, in-frame samples per frame into valid[count] (device)
int launch_warp_frames(gme_ctx* ctx, const Plane& src, const Plane& dst, int first, int count, const double* params, int border,
                       int fill, unsigned long long* valid);
// sse[k] = sum (p[first + k + 1] - p[first + k])^2, k < count (device)
int launch_frame_sse(gme_ctx* ctx, const Plane& p, int first, int count, unsigned long long* sse);

// ---- gme_stab_fill.hip: full-frame stabilization ----------------------------------------------
// output frames 0 .. count - 1 of dst, each pixel from the first of its frame's n_cand candidates (sources[count][n_cand]
// absolute frames of src or -1, params[count][n_cand][8]; device) whose sample point lies in its frame, the border rule on
// candidate 0 elsewhere; who (same geometry as dst; no memory: not wanted) the winning candidate or 255 per pixel;
// valid / filled [count] (device) the pixels won by candidate 0 / by a later one.  The caller has checked the indices.
int launch_warp_fill(gme_ctx* ctx, const Plane& src, const Plane& dst, const Plane& who, int count, int n_cand, const int* sources,
                     const double* params, int border, int fill, unsigned long long* valid, unsigned long long* filled);

// ---- gme_mosaic.hip: background mosaic and moving-object masks --------------------------------
// sprite / cnt [Hc][out_pitch] = lower median / number of the in-frame samples of frames first .. first + count - 1 of src at
// every canvas pixel (fill where there is none); G[count][8] and usable[count] on the device; cull 0 samples every frame
// at every pixel
int launch_mosaic_median(gme_ctx* ctx, const Plane& src, int first, int count, const double* G, const uint8_t* usable, int ox,
                         int oy, int Hc, int Wc, int fill, int cull, uint8_t* sprite, uint16_t* cnt, int out_pitch);
// masks of frames first .. first + count - 1 into dst, their known and moving pixels into known[count] and moving[count]
// (device, zeroed by the caller); A[count][8] and usable[count] on the device
int launch_moving_masks(gme_ctx* ctx, const Plane& src, const Plane& dst, int first, int count, const double* A,
                        const uint8_t* usable, const uint8_t* sprite, const uint16_t* cnt, int sp_pitch, int Hc, int Wc, int ox,
                        int oy, int threshold, int min_count, unsigned long long* known, unsigned long long* moving);

// ---- bbme_subpel.hip: quarter-pel refinement and compensation ------------------------------------
// qmf[pairs][H / bs][W / bs][2] (quarter units) and cost[pairs][H / bs][W / bs] = subpel.refine of the integer field mf of the
// same shape; pair k reads the planes prev + k * plane_stride and cur + k * plane_stride (device)
int launch_subpel_refine(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                         int pitch, int bs, int pnorm, int levels, const int32_t* mf, int32_t* qmf, long long* cost);
// out planes = subpel.compensate of the prev planes by qmf, sse[pairs] (device) = squared error of each against its cur plane
int launch_compensate_qpel(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                           int pitch, int bs, const int32_t* qmf, uint8_t* out, long long out_stride, int out_pitch,
                           unsigned long long* sse);

// ---- bbme_hier.hip: hierarchical block matching ----------------------------------------------------
// the argument rules of hier.py (GME_ERR_ARG)
int hier_check_args(const char* who, int bs, int cw, int radius, int pnorm, int levels);
// hier.search of `pairs` pairs: level[l] holds the planes of pyramid level l ([2] = the frames), pair k = planes first_prev + k
// and first_cur + k of each stack; mf[l] [pairs][hb][wb][2] and cost[l] [pairs][hb][wb] (device) for the levels
// l >= 3 - levels, hb = H / bs and wb = W / bs of level 2.  Names the kernel instance in the context's plan.
int launch_hier(gme_ctx* ctx, const Plane (&level)[3], int first_prev, int first_cur, int pairs, int bs, int cw, int radius,
                int pnorm, int levels, int32_t* const (&mf)[3], long long* const (&cost)[3]);

// ---- bbme_vbs.hip: variable-block-size motion -------------------------------------------------------
// the argument rules of vbs.py (GME_ERR_ARG)
int vbs_check_args(const char* who, int bs, int depth, int radius, int pnorm, int penalty);
// vbs.tree of `pairs` pairs on the field mf[pairs][H / bs][W / bs][2]: pair k reads the planes prev + k * plane_stride and
// cur + k * plane_stride; leaf [pairs][hb << depth][wb << depth][2], dmap of the same grid, cost [pairs][hb][wb] (device).
// Names the kernel instance in the context's plan.
int launch_vbs(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch,
               int bs, int depth, int radius, int pnorm, int penalty, const int32_t* mf, int32_t* leaf, uint8_t* dmap,
               long long* cost);
// out planes = subpel.compensate_integer of the prev planes by leaf[pairs][hg][wg][2] at cell size g, sse[pairs] (device) =
// squared error of each against its cur plane
int launch_compensate_vbs(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                          int pitch, int g, int hg, int wg, const int32_t* leaf, uint8_t* out, long long out_stride, int out_pitch,
                          unsigned long long* sse);

// ---- bbme_bipred.hip: bidirectional block prediction ------------------------------------------------
// the argument rules of bipred.py (GME_ERR_ARG)
int bipred_check_args(const char* who, int bs, int radius, int rounds, int pnorm, int penalty);
// bipred.decide of `targets` triples on the fields f0, f1 [targets][H / bs][W / bs][2]: target k reads the planes
// past + k * plane_stride, mid + k * plane_stride and next + k * plane_stride; mode [targets][hb][wb], v0 and v1
// [targets][hb][wb][2], cost [targets][hb][wb], costs [targets][hb][wb][3] (device).  Names the kernel instance in the
// context's plan.
int launch_bipred(gme_ctx* ctx, const uint8_t* past, const uint8_t* mid, const uint8_t* next, long long plane_stride, int targets,
                  int H, int W, int pitch, int bs, int radius, int rounds, int pnorm, int penalty, const int32_t* f0, const int32_t* f1,
                  uint8_t* mode, int32_t* v0, int32_t* v1, long long* cost, long long* costs);
// out planes = bipred.predict of the past and next planes, sse[targets] (device) = squared error of each against its mid plane
int launch_predict_bipred(gme_ctx* ctx, const uint8_t* past, const uint8_t* mid, const uint8_t* next, long long plane_stride,
                          int targets, int H, int W, int pitch, int bs, const uint8_t* mode, const int32_t* v0, const int32_t* v1,
                          uint8_t* out, long long out_stride, int out_pitch, unsigned long long* sse);

// ---- bbme_gmc.hip: global motion compensation -------------------------------------------------------
// the argument rules of gmc.py (GME_ERR_ARG)
int gmc_check_args(const char* who, int bs, int pnorm, int penalty);
// gmc.usable of one warp of an H x W frame (host): the per-pair flag the two launchers take
bool gmc_usable(const double* h, int H, int W);
// gmc.decide of `pairs` pairs on the fields f [pairs][H / bs][W / bs][2] under the warps h [pairs][8] with their flags usable
// [pairs]: pair k reads the planes ref + k * plane_stride and cur + k * plane_stride; mode [pairs][hb][wb], cost [pairs][hb][wb],
// costs [pairs][hb][wb][2] (all device).  Names the kernel instance in the context's plan.
int launch_gmc(gme_ctx* ctx, const uint8_t* ref, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
               int pnorm, int penalty, const double* h, const uint8_t* usable, const int32_t* f, uint8_t* mode, long long* cost,
               long long* costs);
// out planes = gmc.predict of the ref planes, sse[pairs] (device) = squared error of each against its cur plane
int launch_predict_gmc(gme_ctx* ctx, const uint8_t* ref, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch,
                       int bs, const double* h, const uint8_t* usable, const uint8_t* mode, const int32_t* f, uint8_t* out,
                       long long out_stride, int out_pitch, unsigned long long* sse);

// ---- bbme_prop.hip: vector propagation search --------------------------------------------------------
// the argument rules of propagate.py (GME_ERR_ARG)
int prop_check_args(const char* who, int bs, int pnorm, int rounds, int steps);
// propagate.search of `pairs` pairs on the prior fields f [pairs][H / bs][W / bs][2]: pair k reads the planes
// prev + k * plane_stride and cur + k * plane_stride, the temporal field t[k + t_shift] (t null: none; neither where
// k + t_shift < 0) and the camera field g[k] (null: none).  The rounds alternate between work[0] and work[1] (each
// [pairs][hb][wb][2]) and only read f, so t may lie in it; *result is the one the last round wrote, cost [pairs][hb][wb] and
// source [pairs][hb][wb] are that round's (all device).  Names the kernel instance in the context's plan.
int launch_prop(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
                int pnorm, int rounds, int steps, const int32_t* f, const int32_t* t, int t_shift, const int32_t* g, int32_t* const work[2],
                long long* cost, uint8_t* source, int32_t** result);

// ---- bbme_interp.hip: motion-compensated frame interpolation -----------------------------------------
// the argument rules of interp.py for H x W frames (GME_ERR_ARG)
int interp_check_args(const char* who, int H, int W, int bs, int sw, int pnorm, int bias);
// interp.search of `pairs` pairs: pair k reads the planes past + k * plane_stride and next + k * plane_stride; mv
// [pairs][H / bs][W / bs][2], cost (J) and dist (D) [pairs][H / bs][W / bs] (device).  Names the kernel instance in the context's
// plan.
int launch_interp(gme_ctx* ctx, const uint8_t* past, const uint8_t* next, long long plane_stride, int pairs, int H, int W, int pitch,
                  int bs, int sw, int pnorm, int bias, int32_t* mv, long long* cost, long long* dist);
// out planes = interp.interpolate of the past and next planes by mv, sse[pairs] (device) = squared error of each against its cur
// plane (the true middle frame; any plane of the stack where there is none)
int launch_interp_frame(gme_ctx* ctx, const uint8_t* past, const uint8_t* next, const uint8_t* cur, long long plane_stride, int pairs,
                        int H, int W, int pitch, int bs, const int32_t* mv, uint8_t* out, long long out_stride, int out_pitch,
                        unsigned long long* sse);

// ---- bbme_retime.hip: frame interpolation at any phase ------------------------------------------------
// the argument rules of retime.py for H x W frames (GME_ERR_ARG), and retime.check_phase: n / d reduced in place
int retime_check_args(const char* who, int H, int W, int bs, int sw, int pnorm, int bias);
int retime_check_phase(const char* who, int* n, int* d);
// The phase table: one row of retime_row_ints() int32 per output, written on the host by retime_row for the output whose `past`
// is plane `plane` of the stack (`next` the plane behind it) at the reduced phase n / d -> the LDS a wave of that output needs
int retime_row_ints();
int retime_row(int32_t* row, int plane, int n, int d, int bs, int sw);
// retime.search of `outputs` outputs under their table rows (device; wave_lds: the largest retime_row of them); mv
// [outputs][H / bs][W / bs][2], cost (J) and dist (D) [outputs][H / bs][W / bs] (device).  Names the kernel instance in the
// context's plan.
int launch_retime(gme_ctx* ctx, const uint8_t* frames, long long plane_stride, int outputs, int H, int W, int pitch, int bs, int sw,
                  int pnorm, int bias, const int32_t* table, int wave_lds, int32_t* mv, long long* cost, long long* dist);
// out planes = retime.interpolate of each output's planes by mv, sse[outputs] (device) = squared error of each against its cur
// plane (cur + k * cur_stride: the true frame; any plane where there is none)
int launch_retime_frame(gme_ctx* ctx, const uint8_t* frames, long long plane_stride, int outputs, int H, int W, int pitch, int bs,
                        const int32_t* table, const int32_t* mv, const uint8_t* cur, long long cur_stride, uint8_t* out,
                        long long out_stride, int out_pitch, unsigned long long* sse);

// ---- bbme_obmc.hip: overlapped block motion compensation ---------------------------------------------
// the argument rules of obmc.py for H x W frames (GME_ERR_ARG)
int obmc_check_args(const char* who, int H, int W, int bs, int unit);
// out planes = obmc.compensate of the prev planes by field [pairs][H / bs][W / bs][2] in units of unit / 4 pixels (4: whole
// pixels, 1: quarter pixels), sse[pairs] (device) = squared error of each against its cur plane.  Names the kernel in the context's
// plan.  negate: by the negated field, for a field anchored at the predicted frame (denoise.predict).
int launch_obmc(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
                const int32_t* field, int unit, uint8_t* out, long long out_stride, int out_pitch, unsigned long long* sse,
                bool negate = false);

// ---- bbme_denoise.hip: motion-compensated temporal denoising -----------------------------------------
// the argument rules of denoise.py (GME_ERR_ARG)
int denoise_check_args(const char* who, int R, int strength);
// out planes = denoise.blend of the cur planes (cur_stride apart) with R prediction planes each: target k reads prediction r at
// preds + k * plane_stride + r * pred_stride; sse[targets] (device) = squared difference of each output against its truth plane
// (truth_stride apart).  Every input plane has the row pitch `pitch`.  Names the kernel in the context's plan; GME_OK for zero
// targets.
int launch_denoise(gme_ctx* ctx, const uint8_t* cur, long long cur_stride, const uint8_t* preds, long long pred_stride, long long plane_stride,
                   int targets, int R, int H, int W, int pitch, int strength, const uint8_t* truth, long long truth_stride, uint8_t* out,
                   long long out_stride, int out_pitch, unsigned long long* sse);

// ---- what the entry points of the passes share (gme_api_passes.hip, gme_api_frames.hip) -------------------------------------
// The ending of a single-pair call that can predict (gme_bipred_u8, gme_gmc_u8): where the caller wants the predicted frame or
// its squared error, predict() launches it into plane `pred` of the stack with the error in *d_sse (device); then the wait.
template <class Predict>
int oneshot_predict(gme_ctx* ctx, const Plane& st, int pred, const unsigned long long* d_sse, uint8_t* pred_out, int64_t* sse_out,
                    Predict predict)
{
    unsigned long long sse = 0;
    int rc = GME_OK;
    if (pred_out || sse_out) {
        rc = predict();
        if (rc) return rc;
        if (pred_out) {
            rc = read_planes(ctx, st, pred, 1, pred_out);
            if (rc) return rc;
        }
        GME_HIP_TRY(hipMemcpyAsync(&sse, d_sse, sizeof(sse), hipMemcpyDeviceToHost, ctx->stream));
    }
    rc = ctx_finish(ctx);
    if (sse_out) *sse_out = (int64_t)sse;
    return rc;
}

// What the predicting entries of the block-field passes share behind their own state checks: the compensated planes for
// `planes` pairs or targets, predict() (the pass's launch into s->comp and s->sse), the squared errors into sse_out where the
// caller wants them, and the wait.
template <class Predict>
int seq_predict(gme_seq* s, int fd, int planes, int64_t* sse_out, Predict predict)
{
    gme_ctx* ctx = s->ctx;
    int rc = ensure_comp(s, fd, planes);
    if (rc) return rc;
    rc = predict();
    if (rc) return rc;
    comp_wrote(s, planes);
    if (sse_out && planes)
        GME_HIP_TRY(hipMemcpyAsync(sse_out, s->sse, (size_t)planes * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

// One optional output of a reader: `bytes` per item (pair or target) from the device array `src`, whose first item is item 0.
struct ReadPart {
    void* out;
    const void* src;
    size_t bytes;
};

// The reader `who` of a result that `made_by` makes: refused unless the result stands (`valid`) and the items
// [first, first + count) lie within its `limit` items (`noun`: what an item is); then every part the caller gave a buffer for,
// and the wait.  Nothing is copied where there is nothing to copy.
inline int seq_read(gme_seq* s, const char* who, bool valid, const char* made_by, const char* noun, int first, int count, int limit,
                    std::initializer_list<ReadPart> parts)
{
    GME_REQUIRE(valid, GME_ERR_STATE, "%s before %s", who, made_by);
    GME_REQUIRE(first >= 0 && count >= 0 && first + count <= limit, GME_ERR_ARG, "%s: %s [%d, %d) outside [0, %d)", who, noun, first,
                first + count, limit);
    for (const ReadPart& part : parts)
        if (part.out && part.bytes * count)
            GME_HIP_TRY(hipMemcpyAsync(part.out, (const uint8_t*)part.src + part.bytes * first, part.bytes * count, hipMemcpyDeviceToHost,
                                       s->ctx->stream));
    return ctx_finish(s->ctx);
}
