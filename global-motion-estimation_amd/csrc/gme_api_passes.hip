// C ABI of libgme_hip.so (include/gme_hip.h), the block-field passes built on the core of gme_api.hip: quarter-pel refinement,
// hierarchical and variable-block-size search, bidirectional prediction, global motion compensation, vector propagation,
// frame interpolation and retiming, overlapped compensation and temporal denoising (the bbme_*.hip from bbme_subpel.hip to
// bbme_denoise.hip).  First the single-pair calls on host buffers, then the calls on a resident sequence.  Also the owner of
// what a sequence keeps for every pass (SeqPasses, gme_passes.h): its creation, its end and its result lifetimes.
#include <new>
#include <vector>

#include "gme_passes.h"

SeqPasses* passes_create() { return new (std::nothrow) SeqPasses(); }

void passes_destroy(SeqPasses* p) { delete p; }            // frees the device buffers of the passes

// Replacing the motion field ends what was derived from it: the quarter-pel, hierarchical, variable-block-size and propagation
// results.  A result type that reads the field joins this list.
void passes_field_replaced(SeqPasses* p)
{
    p->qmv_valid = false;
    p->hier_valid = false;
    p->vbs_valid = false;
    p->prop_valid = false;
}

// New frame data or another frame count ends those, and every result that was measured on the old frames with a field of its
// own (the warped frames, mosaic and masks stay).
void passes_frames_changed(SeqPasses* p)
{
    passes_field_replaced(p);
    p->bp_valid = false;
    p->gm_valid = false;
}

// ---------------------------------------------------------------------------
// single-pair calls on host buffers
// ---------------------------------------------------------------------------
static int subpel_check(const char* who, int H, int W, int bs, int pnorm, int levels)
{
    GME_REQUIRE(bs >= 1 && bs <= 4096, GME_ERR_ARG, "%s: block_size %d (1 .. 4096)", who, bs);
    GME_REQUIRE(pnorm == 0 || pnorm == 1, GME_ERR_ARG, "%s: pnorm_distance %d out of range (bbme.py:60)", who, pnorm);
    GME_REQUIRE(levels >= 0 && levels <= 2, GME_ERR_ARG, "%s: levels %d (0 integer, 1 half-pel, 2 quarter-pel)", who, levels);
    GME_REQUIRE(H <= 0x7FFFFFFF / 4 - 4 && W <= 0x7FFFFFFF / 4 - 4, GME_ERR_ARG, "%s: a %d x %d frame in quarter units", who, H, W);
    return GME_OK;
}

extern "C" int gme_subpel_u8(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int H, int W, int stride, int block_size,
                             int pnorm, int levels, const int32_t* mf_in, int32_t* qmf_out, int64_t* cost_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_subpel_u8", prev && cur && mf_in && qmf_out && cost_out, H, W, stride);
    if (rc) return rc;
    rc = subpel_check("gme_subpel_u8", H, W, block_size, pnorm, levels);
    if (rc) return rc;
    const int h = H / block_size, w = W / block_size;
    if (h == 0 || w == 0) return GME_OK;
    const size_t n = (size_t)h * w;
    Plane pp = plane_shape(H, W, 1), pc = pp;
    int32_t *d_mf = nullptr, *d_q = nullptr;
    long long* d_cost = nullptr;
    Carver c;
    c.take(&pp, true); c.take(&pc, true);
    c.take(&d_mf, n * 2); c.take(&d_q, n * 2); c.take(&d_cost, n);
    rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(hipMemsetAsync(pp.ptr, 0, (uint8_t*)d_mf - pp.ptr, ctx->stream));
    GME_HIP_TRY(put_plane(ctx, pp, prev, stride));
    GME_HIP_TRY(put_plane(ctx, pc, cur, stride));
    GME_HIP_TRY(hipMemcpyAsync(d_mf, mf_in, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_subpel_refine(ctx, pp.ptr, pc.ptr, 0, 1, H, W, pp.pitch, block_size, pnorm, levels, d_mf, d_q, d_cost);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(qmf_out, d_q, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    GME_HIP_TRY(hipMemcpyAsync(cost_out, d_cost, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

// Hierarchical block matching of one pair (bbme_hier.hip): both frames and their two pyramid levels in
// the scratch, each level a stack of two planes (previous, current).
extern "C" int gme_hier_u8(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int H, int W, int stride, int block_size,
                           int coarse_window, int radius, int pnorm, int levels, int32_t* mf_out, int64_t* cost_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_hier_u8", prev && cur && mf_out, H, W, stride);
    if (rc) return rc;
    rc = hier_check_args("gme_hier_u8", block_size, coarse_window, radius, pnorm, levels);
    if (rc) return rc;
    const int h = H / block_size, w = W / block_size;
    if (h == 0 || w == 0) return GME_OK;
    const size_t n = (size_t)h * w;
    Plane lv[3];
    lv[2] = plane_shape(H, W, 2);
    lv[1] = plane_shape((H + 1) / 2, (W + 1) / 2, 2);
    lv[0] = plane_shape((lv[1].H + 1) / 2, (lv[1].W + 1) / 2, 2);
    int32_t* d_mf[3] = { nullptr, nullptr, nullptr };
    long long* d_cost[3] = { nullptr, nullptr, nullptr };
    Carver c;
    for (int l = 2; l >= 0; --l) c.take(&lv[l], true);
    c.take(&d_mf[0], n * 2 * 3);
    c.take(&d_cost[0], n * 3);
    rc = c.commit(ctx);
    if (rc) return rc;
    for (int l = 1; l < 3; ++l) { d_mf[l] = d_mf[0] + n * 2 * l; d_cost[l] = d_cost[0] + n * l; }
    GME_HIP_TRY(hipMemsetAsync(lv[2].ptr, 0, (uint8_t*)d_mf[0] - lv[2].ptr, ctx->stream));
    rc = put_planes(ctx, lv[2], { prev, cur }, stride);
    if (rc) return rc;
    for (int l = 1; l >= 3 - levels; --l) {
        rc = launch_pyrdown(ctx, lv[l + 1], lv[l]);
        if (rc) return rc;
    }
    rc = launch_hier(ctx, lv, 0, 1, 1, block_size, coarse_window, radius, pnorm, levels, d_mf, d_cost);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(mf_out, d_mf[2], n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out, d_cost[2], n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

// The variable-block-size tree of one pair on a given field (bbme_vbs.hip).
extern "C" int gme_vbs_u8(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int H, int W, int stride, int block_size, int depth,
                          int radius, int pnorm, int penalty, const int32_t* mf_in, int32_t* leaf_out, uint8_t* depth_out,
                          int64_t* cost_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_vbs_u8", prev && cur && mf_in && leaf_out, H, W, stride);
    if (rc) return rc;
    rc = vbs_check_args("gme_vbs_u8", block_size, depth, radius, pnorm, penalty);
    if (rc) return rc;
    const int h = H / block_size, w = W / block_size;
    if (h == 0 || w == 0) return GME_OK;
    const size_t n = (size_t)h * w, cells = n << (2 * depth);
    Plane pp = plane_shape(H, W, 1), pc = pp;
    int32_t *d_mf = nullptr, *d_leaf = nullptr;
    long long* d_cost = nullptr;
    uint8_t* d_dmap = nullptr;
    Carver c;
    c.take(&pp, true); c.take(&pc, true);
    c.take(&d_mf, n * 2); c.take(&d_leaf, cells * 2); c.take(&d_cost, n); c.take(&d_dmap, cells);
    rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(hipMemsetAsync(pp.ptr, 0, (uint8_t*)d_mf - pp.ptr, ctx->stream));
    GME_HIP_TRY(put_plane(ctx, pp, prev, stride));
    GME_HIP_TRY(put_plane(ctx, pc, cur, stride));
    GME_HIP_TRY(hipMemcpyAsync(d_mf, mf_in, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_vbs(ctx, pp.ptr, pc.ptr, 0, 1, H, W, pp.pitch, block_size, depth, radius, pnorm, penalty, d_mf, d_leaf, d_dmap, d_cost);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(leaf_out, d_leaf, cells * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (depth_out) GME_HIP_TRY(hipMemcpyAsync(depth_out, d_dmap, cells, hipMemcpyDeviceToHost, ctx->stream));
    if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out, d_cost, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

// Bidirectional prediction of one triple on given fields (bbme_bipred.hip): the three frames and the
// predicted one as one stack of four planes in the scratch.
extern "C" int gme_bipred_u8(gme_ctx* ctx, const uint8_t* past, const uint8_t* mid, const uint8_t* next, int H, int W, int stride,
                             int block_size, int radius, int rounds, int pnorm, int penalty, const int32_t* f0, const int32_t* f1,
                             uint8_t* mode_out, int32_t* v0_out, int32_t* v1_out, int64_t* cost_out, int64_t* costs_out,
                             uint8_t* pred_out, int64_t* sse_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_bipred_u8", past && mid && next && f0 && f1 && mode_out, H, W, stride);
    if (rc) return rc;
    rc = bipred_check_args("gme_bipred_u8", block_size, radius, rounds, pnorm, penalty);
    if (rc) return rc;
    const int h = H / block_size, w = W / block_size;
    const size_t n = (size_t)h * w;
    Plane st = plane_shape(H, W, 4);                           // past, mid, next, predicted
    int32_t* d_vec = nullptr;                                  // f0, f1, v0, v1
    long long* d_cost = nullptr;                               // cost, costs, then the squared error
    uint8_t* d_mode = nullptr;
    Carver c;
    c.take(&st, true); c.take(&d_vec, n * 8); c.take(&d_cost, n * 4 + 1); c.take(&d_mode, n + 1);
    rc = c.commit(ctx);
    if (rc) return rc;
    int32_t *d_f0 = d_vec, *d_f1 = d_vec + n * 2, *d_v0 = d_vec + n * 4, *d_v1 = d_vec + n * 6;
    long long* d_costs = d_cost + n;
    unsigned long long* d_sse = (unsigned long long*)(d_cost + n * 4);
    GME_HIP_TRY(hipMemsetAsync(st.ptr, 0, (uint8_t*)d_vec - st.ptr, ctx->stream));
    rc = put_planes(ctx, st, { past, mid, next }, stride);
    if (rc) return rc;
    if (n) {
        GME_HIP_TRY(hipMemcpyAsync(d_f0, f0, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        GME_HIP_TRY(hipMemcpyAsync(d_f1, f1, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    rc = launch_bipred(ctx, st.at(0), st.at(1), st.at(2), 0, 1, H, W, st.pitch, block_size, radius, rounds, pnorm, penalty, d_f0, d_f1,
                       d_mode, d_v0, d_v1, d_cost, d_costs);
    if (rc) return rc;
    if (n) {
        GME_HIP_TRY(hipMemcpyAsync(mode_out, d_mode, n, hipMemcpyDeviceToHost, ctx->stream));
        if (v0_out) GME_HIP_TRY(hipMemcpyAsync(v0_out, d_v0, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (v1_out) GME_HIP_TRY(hipMemcpyAsync(v1_out, d_v1, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out, d_cost, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        if (costs_out) GME_HIP_TRY(hipMemcpyAsync(costs_out, d_costs, n * 3 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    }
    return oneshot_predict(ctx, st, 3, d_sse, pred_out, sse_out, [&] {
        return launch_predict_bipred(ctx, st.at(0), st.at(1), st.at(2), 0, 1, H, W, st.pitch, block_size, d_mode, d_v0, d_v1, st.at(3), 0,
                                     st.pitch, d_sse);
    });
}

// Global motion compensation of one pair on a given warp and field (bbme_gmc.hip): the two frames and the
// predicted one as one stack of three planes in the scratch.
extern "C" int gme_gmc_u8(gme_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int H, int W, int stride, int block_size, int pnorm,
                          int penalty, const double* h, const int32_t* f, uint8_t* mode_out, int64_t* cost_out, int64_t* costs_out,
                          uint8_t* pred_out, int64_t* sse_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_gmc_u8", ref && cur && h && f && mode_out, H, W, stride);
    if (rc) return rc;
    rc = gmc_check_args("gme_gmc_u8", block_size, pnorm, penalty);
    if (rc) return rc;
    const int hb = H / block_size, wb = W / block_size;
    const size_t n = (size_t)hb * wb;
    Plane st = plane_shape(H, W, 3);                           // ref, cur, predicted
    int32_t* d_f = nullptr;
    long long* d_cost = nullptr;                               // cost, costs, then the squared error
    double* d_h = nullptr;
    uint8_t* d_mode = nullptr;                                 // the modes, then the usable flag
    Carver c;
    c.take(&st, true); c.take(&d_f, n * 2 + 1); c.take(&d_cost, n * 3 + 1); c.take(&d_h, 8); c.take(&d_mode, n + 1);
    rc = c.commit(ctx);
    if (rc) return rc;
    long long* d_costs = d_cost + n;
    unsigned long long* d_sse = (unsigned long long*)(d_cost + n * 3);
    uint8_t* d_usable = d_mode + n;
    GME_HIP_TRY(hipMemsetAsync(st.ptr, 0, (uint8_t*)d_f - st.ptr, ctx->stream));
    rc = put_planes(ctx, st, { ref, cur }, stride);
    if (rc) return rc;
    const uint8_t usable = gmc_usable(h, H, W) ? 1 : 0;        // read by the copy below before this call returns (ctx_finish)
    GME_HIP_TRY(hipMemcpyAsync(d_h, h, 8 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    GME_HIP_TRY(hipMemcpyAsync(d_usable, &usable, 1, hipMemcpyHostToDevice, ctx->stream));
    if (n) GME_HIP_TRY(hipMemcpyAsync(d_f, f, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_gmc(ctx, st.at(0), st.at(1), 0, 1, H, W, st.pitch, block_size, pnorm, penalty, d_h, d_usable, d_f, d_mode, d_cost, d_costs);
    if (rc) return rc;
    if (n) {
        GME_HIP_TRY(hipMemcpyAsync(mode_out, d_mode, n, hipMemcpyDeviceToHost, ctx->stream));
        if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out, d_cost, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        if (costs_out) GME_HIP_TRY(hipMemcpyAsync(costs_out, d_costs, n * 2 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    }
    return oneshot_predict(ctx, st, 2, d_sse, pred_out, sse_out, [&] {
        return launch_predict_gmc(ctx, st.at(0), st.at(1), 0, 1, H, W, st.pitch, block_size, d_h, d_usable, d_mode, d_f, st.at(2), 0, st.pitch,
                                  d_sse);
    });
}

// Vector propagation of one pair on given fields (bbme_prop.hip): the two frames as one stack of two planes
// in the scratch, behind them the prior, temporal and camera fields and the two fields the rounds alternate between.
extern "C" int gme_prop_u8(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int H, int W, int stride, int block_size, int pnorm,
                           int rounds, int steps, const int32_t* f, const int32_t* t, const int32_t* g, int32_t* mf_out, int64_t* cost_out,
                           uint8_t* source_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_prop_u8", prev && cur && f && mf_out, H, W, stride);
    if (rc) return rc;
    rc = prop_check_args("gme_prop_u8", block_size, pnorm, rounds, steps);
    if (rc) return rc;
    const int hb = H / block_size, wb = W / block_size;
    const size_t n = (size_t)hb * wb;
    if (n == 0) return GME_OK;
    Plane st = plane_shape(H, W, 2);                           // previous, current
    int32_t* d_vec = nullptr;                                  // f, t, g, then the two working fields
    long long* d_cost = nullptr;
    uint8_t* d_source = nullptr;
    Carver c;
    c.take(&st, true); c.take(&d_vec, n * 10); c.take(&d_cost, n); c.take(&d_source, n);
    rc = c.commit(ctx);
    if (rc) return rc;
    int32_t *d_f = d_vec, *d_t = d_vec + n * 2, *d_g = d_vec + n * 4;
    int32_t* const work[2] = { d_vec + n * 6, d_vec + n * 8 };
    GME_HIP_TRY(hipMemsetAsync(st.ptr, 0, (uint8_t*)d_vec - st.ptr, ctx->stream));
    rc = put_planes(ctx, st, { prev, cur }, stride);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(d_f, f, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (t) GME_HIP_TRY(hipMemcpyAsync(d_t, t, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (g) GME_HIP_TRY(hipMemcpyAsync(d_g, g, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    int32_t* d_mf = nullptr;
    rc = launch_prop(ctx, st.at(0), st.at(1), 0, 1, H, W, st.pitch, block_size, pnorm, rounds, steps, d_f, t ? d_t : nullptr, 0,
                     g ? d_g : nullptr, work, d_cost, d_source, &d_mf);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(mf_out, d_mf, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out, d_cost, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    if (source_out) GME_HIP_TRY(hipMemcpyAsync(source_out, d_source, n, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

// Frame interpolation of one pair (bbme_interp.hip): the two frames, the true middle frame where the caller
// has one and the interpolated frame as one stack of four planes in the scratch.
extern "C" int gme_interp_u8(gme_ctx* ctx, const uint8_t* past, const uint8_t* next, const uint8_t* truth, int H, int W, int stride,
                             int block_size, int search_window, int pnorm, int bias, int32_t* mv_out, int64_t* cost_out, int64_t* dist_out,
                             uint8_t* frame_out, int64_t* sse_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_interp_u8", past && next, H, W, stride);
    if (rc) return rc;
    rc = interp_check_args("gme_interp_u8", H, W, block_size, search_window, pnorm, bias);
    if (rc) return rc;
    const size_t n = (size_t)(H / block_size) * (W / block_size);
    Plane st = plane_shape(H, W, 4);                           // past, next, truth, interpolated
    int32_t* d_mv = nullptr;
    long long* d_cost = nullptr;                               // J, D, then the squared error
    Carver c;
    c.take(&st, true); c.take(&d_mv, n * 2); c.take(&d_cost, n * 2 + 1);
    rc = c.commit(ctx);
    if (rc) return rc;
    long long* d_dist = d_cost + n;
    unsigned long long* d_sse = (unsigned long long*)(d_cost + n * 2);
    GME_HIP_TRY(hipMemsetAsync(st.ptr, 0, (uint8_t*)d_mv - st.ptr, ctx->stream));
    rc = put_planes(ctx, st, { past, next, truth ? truth : past }, stride);
    if (rc) return rc;
    rc = launch_interp(ctx, st.at(0), st.at(1), 0, 1, H, W, st.pitch, block_size, search_window, pnorm, bias, d_mv, d_cost, d_dist);
    if (rc) return rc;
    if (mv_out) GME_HIP_TRY(hipMemcpyAsync(mv_out, d_mv, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out, d_cost, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    if (dist_out) GME_HIP_TRY(hipMemcpyAsync(dist_out, d_dist, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    int64_t sse = -1;                                          // without a true middle frame there is no error to report
    rc = oneshot_predict(ctx, st, 3, d_sse, frame_out, truth && sse_out ? &sse : nullptr, [&] {
        return launch_interp_frame(ctx, st.at(0), st.at(1), st.at(2), 0, 1, H, W, st.pitch, block_size, d_mv, st.at(3), 0, st.pitch, d_sse);
    });
    if (sse_out) *sse_out = sse;
    return rc;
}

// Frame interpolation at any phase of one pair (bbme_retime.hip): the two frames, the true frame at that time
// where the caller has one and the made frame as one stack of four planes in the scratch, behind them the one row of the phase
// table.
extern "C" int gme_retime_u8(gme_ctx* ctx, const uint8_t* past, const uint8_t* next, const uint8_t* truth, int H, int W, int stride,
                             int block_size, int search_window, int pnorm, int bias, int n, int d, int32_t* mv_out, int64_t* cost_out,
                             int64_t* dist_out, uint8_t* frame_out, int64_t* sse_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_retime_u8", past && next, H, W, stride);
    if (rc) return rc;
    rc = retime_check_args("gme_retime_u8", H, W, block_size, search_window, pnorm, bias);
    if (rc) return rc;
    rc = retime_check_phase("gme_retime_u8", &n, &d);
    if (rc) return rc;
    const size_t blocks = (size_t)(H / block_size) * (W / block_size);
    Plane st = plane_shape(H, W, 4);                           // past, next, truth, made
    int32_t* d_mv = nullptr;
    int32_t* d_table = nullptr;
    long long* d_cost = nullptr;                               // J, D, then the squared error
    Carver c;
    c.take(&st, true); c.take(&d_mv, blocks * 2); c.take(&d_cost, blocks * 2 + 1); c.take(&d_table, (size_t)retime_row_ints());
    rc = c.commit(ctx);
    if (rc) return rc;
    long long* d_dist = d_cost + blocks;
    unsigned long long* d_sse = (unsigned long long*)(d_cost + blocks * 2);
    std::vector<int32_t> row((size_t)retime_row_ints());       // read by the copy below before this call returns (ctx_finish)
    const int wave_lds = retime_row(row.data(), 0, n, d, block_size, search_window);
    GME_HIP_TRY(hipMemsetAsync(st.ptr, 0, (uint8_t*)d_mv - st.ptr, ctx->stream));
    rc = put_planes(ctx, st, { past, next, truth ? truth : past }, stride);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(d_table, row.data(), row.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_retime(ctx, st.ptr, st.stride, 1, H, W, st.pitch, block_size, search_window, pnorm, bias, d_table, wave_lds, d_mv, d_cost,
                       d_dist);
    if (rc) return rc;
    if (mv_out) GME_HIP_TRY(hipMemcpyAsync(mv_out, d_mv, blocks * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out, d_cost, blocks * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    if (dist_out) GME_HIP_TRY(hipMemcpyAsync(dist_out, d_dist, blocks * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    int64_t sse = -1;                                          // without a true frame there is no error to report
    rc = oneshot_predict(ctx, st, 3, d_sse, frame_out, truth && sse_out ? &sse : nullptr, [&] {
        return launch_retime_frame(ctx, st.ptr, st.stride, 1, H, W, st.pitch, block_size, d_table, d_mv, st.at(2), 0, st.at(3), 0, st.pitch,
                                   d_sse);
    });
    if (sse_out) *sse_out = sse;
    return rc;
}

// Rate conversion of a host clip (bbme_retime.hip): the outputs first_out .. first_out + count - 1 of
// retime.schedule.  Copies are made on the host; the frames the other outputs need are uploaded once into one stack, and the
// outputs run in chunks of at most one launch's planes, each with its rows of the phase table.  Every buffer lives as long as
// the call.
extern "C" int gme_retime_clip_u8(gme_ctx* ctx, const uint8_t* frames, int n_frames, int H, int W, int stride, int block_size,
                                  int search_window, int pnorm, int bias, int step_num, int step_den, int first_out, int count,
                                  uint8_t* frames_out, int32_t* mv_out, int64_t* cost_out, int64_t* dist_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_retime_clip_u8", frames != nullptr, H, W, stride);
    if (rc) return rc;
    GME_REQUIRE(n_frames >= 1, GME_ERR_ARG, "gme_retime_clip_u8: %d frames", n_frames);
    rc = retime_check_args("gme_retime_clip_u8", H, W, block_size, search_window, pnorm, bias);
    if (rc) return rc;
    GME_REQUIRE(step_num >= 1 && step_den >= 1, GME_ERR_ARG, "gme_retime_clip_u8: step %d/%d", step_num, step_den);
    const long long M = ((long long)(n_frames - 1) * step_den) / step_num + 1;
    GME_REQUIRE(M <= 0x7FFFFFFF, GME_ERR_ARG, "gme_retime_clip_u8: %lld outputs", M);
    // the phases of the whole schedule, as retime.schedule checks them: r takes the multiples of gcd(step_num, step_den) that
    // the M outputs reach
    for (long long m = 0; m < M && m < step_den; ++m) {
        int n = (int)((m * step_num) % step_den), d = step_den;
        if (n == 0) continue;
        rc = retime_check_phase("gme_retime_clip_u8", &n, &d);
        if (rc) return rc;
    }
    GME_REQUIRE(first_out >= 0 && count >= 0 && (long long)first_out + count <= M, GME_ERR_ARG,
                "gme_retime_clip_u8: outputs [%d, %lld) outside [0, %lld)", first_out, (long long)first_out + count, M);
    const size_t per = (size_t)(H / block_size) * (W / block_size), image = (size_t)H * W, frame_bytes = (size_t)H * stride;
    struct Made { int out, k, n, d; };                         // an output that is not a copy: its index in the range, pair and phase
    std::vector<Made> made;
    int k_lo = n_frames, k_hi = -1;
    for (int i = 0; i < count; ++i) {
        const long long t = (long long)(first_out + i) * step_num;
        const int k = (int)(t / step_den);
        int n = (int)(t % step_den), d = step_den;
        if (n == 0) {                                          // the frame itself, zero vectors and costs
            if (frames_out)
                for (int y = 0; y < H; ++y) memcpy(frames_out + image * i + (size_t)y * W, frames + frame_bytes * k + (size_t)y * stride, (size_t)W);
            if (mv_out) memset(mv_out + per * 2 * i, 0, per * 2 * sizeof(int32_t));
            if (cost_out) memset(cost_out + per * i, 0, per * sizeof(int64_t));
            if (dist_out) memset(dist_out + per * i, 0, per * sizeof(int64_t));
            continue;
        }
        rc = retime_check_phase("gme_retime_clip_u8", &n, &d);
        if (rc) return rc;
        made.push_back({ i, k, n, d });
        if (k < k_lo) k_lo = k;
        if (k + 1 > k_hi) k_hi = k + 1;
    }
    ctx->plan[0] = 0; ctx->plan_patches = 0;
    if (made.empty()) return GME_OK;
    // the input frames an output needs, each uploaded once into its plane of one stack (plane = frame - k_lo)
    PlaneBuf in;
    rc = plane_alloc(ctx, &in, k_hi - k_lo + 1, H, W);
    if (rc) return rc;
    std::vector<uint8_t> needed((size_t)(k_hi - k_lo + 1), 0);
    for (const Made& o : made) needed[(size_t)(o.k - k_lo)] = needed[(size_t)(o.k + 1 - k_lo)] = 1;
    for (int k = k_lo; k <= k_hi; ++k)
        if (needed[(size_t)(k - k_lo)])
            GME_HIP_TRY(hipMemcpy2DAsync(in.at(k - k_lo), in.pitch, frames + frame_bytes * k, stride, W, H, hipMemcpyHostToDevice, ctx->stream));
    const int total = (int)made.size(), step = max_grid_planes(), most = total < step ? total : step, ints = retime_row_ints();
    DevBuf<int32_t> mv, table;
    DevBuf<long long> cost;                                    // per chunk: J of every block, then D of every block
    DevBuf<unsigned long long> sse;
    PlaneBuf out;
    rc = mv.ensure(per * 2 * most, "retiming vectors");
    if (rc) return rc;
    rc = cost.ensure(per * 2 * most, "retiming costs");
    if (rc) return rc;
    rc = table.ensure((size_t)ints * most, "retiming phase table");
    if (rc) return rc;
    if (frames_out) {
        rc = sse.ensure((size_t)most, "retiming errors");
        if (rc) return rc;
        rc = plane_alloc(ctx, &out, most, H, W);
        if (rc) return rc;
    }
    std::vector<int32_t> rows((size_t)ints * most);            // read by the copy of a chunk before its ctx_finish
    for (int at = 0; at < total; at += step) {
        const int n = total - at < step ? total - at : step;
        int wave_lds = 0;
        for (int i = 0; i < n; ++i) {
            const Made& o = made[(size_t)(at + i)];
            const int lds = retime_row(rows.data() + (size_t)ints * i, o.k - k_lo, o.n, o.d, block_size, search_window);
            if (lds > wave_lds) wave_lds = lds;
        }
        GME_HIP_TRY(hipMemcpyAsync(table.get(), rows.data(), (size_t)ints * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        long long* dist = cost.get() + per * n;
        rc = launch_retime(ctx, in.ptr, in.stride, n, H, W, in.pitch, block_size, search_window, pnorm, bias, table, wave_lds, mv, cost, dist);
        if (rc) return rc;
        if (frames_out) {                                      // no true frames: the errors against `past` are not used
            rc = launch_retime_frame(ctx, in.ptr, in.stride, n, H, W, in.pitch, block_size, table, mv, in.ptr, 0, out.ptr, out.stride,
                                     out.pitch, sse);
            if (rc) return rc;
        }
        for (int i = 0; i < n; ++i) {
            const size_t o = (size_t)made[(size_t)(at + i)].out;
            if (mv_out) GME_HIP_TRY(hipMemcpyAsync(mv_out + per * 2 * o, mv.get() + per * 2 * i, per * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out + per * o, cost.get() + per * i, per * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
            if (dist_out) GME_HIP_TRY(hipMemcpyAsync(dist_out + per * o, dist + per * i, per * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
            if (frames_out) {
                rc = read_planes(ctx, out, i, 1, frames_out + image * o);
                if (rc) return rc;
            }
        }
        rc = ctx_finish(ctx);                                  // the next chunk writes the same buffers
        if (rc) return rc;
    }
    return GME_OK;
}

// Overlapped block motion compensation of one pair (bbme_obmc.hip): `prev`, `cur` where the caller has one
// and the compensated frame as one stack of three planes in the scratch.
extern "C" int gme_obmc_u8(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int H, int W, int stride, int block_size,
                           const int32_t* field, int unit, uint8_t* frame_out, int64_t* sse_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_obmc_u8", prev && field, H, W, stride);
    if (rc) return rc;
    rc = obmc_check_args("gme_obmc_u8", H, W, block_size, unit);
    if (rc) return rc;
    const size_t n = (size_t)(H / block_size) * (W / block_size);
    Plane st = plane_shape(H, W, 3);                           // prev, cur, compensated
    int32_t* d_field = nullptr;
    unsigned long long* d_sse = nullptr;
    Carver c;
    c.take(&st, true); c.take(&d_field, n * 2); c.take(&d_sse, 1);
    rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(hipMemsetAsync(st.ptr, 0, (uint8_t*)d_field - st.ptr, ctx->stream));
    rc = put_planes(ctx, st, { prev, cur ? cur : prev }, stride);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(d_field, field, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    int64_t sse = -1;                                          // without `cur` there is no error to report
    rc = oneshot_predict(ctx, st, 2, d_sse, frame_out, cur && sse_out ? &sse : nullptr, [&] {
        return launch_obmc(ctx, st.at(0), st.at(1), 0, 1, H, W, st.pitch, block_size, d_field, unit, st.at(2), 0, st.pitch, d_sse);
    });
    if (sse_out) *sse_out = sse;
    return rc;
}

// Motion-compensated temporal denoising of one frame (bbme_denoise.hip): `cur`, the comparison plane, the R
// references, their R overlapped predictions and the filtered frame as one stack of 2 R + 3 planes in the scratch.
extern "C" int gme_denoise_u8(gme_ctx* ctx, const uint8_t* cur, const uint8_t* const* refs, const int32_t* const* fields, int R, int H, int W,
                              int stride, int block_size, int unit, int strength, const uint8_t* truth, uint8_t* frame_out, int64_t* sse_out)
{
    GME_ENTER(ctx);
    int rc = oneshot_check("gme_denoise_u8", cur && refs && fields, H, W, stride);
    if (rc) return rc;
    rc = denoise_check_args("gme_denoise_u8", R, strength);
    if (rc) return rc;
    for (int r = 0; r < R; ++r) GME_REQUIRE(refs[r] && fields[r], GME_ERR_ARG, "gme_denoise_u8: null reference or field %d", r);
    rc = obmc_check_args("gme_denoise_u8", H, W, block_size, unit);
    if (rc) return rc;
    const size_t n = (size_t)(H / block_size) * (W / block_size);
    Plane st = plane_shape(H, W, 2 * R + 3);                   // cur, truth, R references, R predictions, filtered
    int32_t* d_field = nullptr;
    unsigned long long* d_sse = nullptr;                       // [0] of the filter, [1 + r] of prediction r (not reported)
    Carver c;
    c.take(&st, true); c.take(&d_field, n * 2 * R); c.take(&d_sse, 1 + (size_t)R);
    rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(hipMemsetAsync(st.ptr, 0, (uint8_t*)d_field - st.ptr, ctx->stream));
    rc = put_planes(ctx, st, { cur, truth ? truth : cur }, stride);
    if (rc) return rc;
    for (int r = 0; r < R; ++r) {
        Plane one = st;
        one.ptr = st.at(2 + r);
        GME_HIP_TRY(put_plane(ctx, one, refs[r], stride));
        GME_HIP_TRY(hipMemcpyAsync(d_field + n * 2 * r, fields[r], n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    int64_t sse = -1;                                          // without `truth` there is no error to report
    rc = oneshot_predict(ctx, st, 2 * R + 2, d_sse, frame_out, truth && sse_out ? &sse : nullptr, [&] {
        for (int r = 0; r < R; ++r) {
            const int e = launch_obmc(ctx, st.at(2 + r), st.at(0), 0, 1, H, W, st.pitch, block_size, d_field + n * 2 * r, unit, st.at(2 + R + r), 0,
                                      st.pitch, d_sse + 1 + r, true);
            if (e) return e;
        }
        return launch_denoise(ctx, st.at(0), 0, st.at(2 + R), st.stride, 0, 1, R, H, W, st.pitch, strength, st.at(1), 0, st.at(2 * R + 2), 0,
                              st.pitch, d_sse);
    });
    if (sse_out) *sse_out = sse;
    return rc;
}

// ---------------------------------------------------------------------------
// Quarter-pel block matching (bbme_subpel.hip): blocking calls on the field of the last gme_seq_bbme.
// ---------------------------------------------------------------------------
static int subpel_field(gme_seq* s, const char* who, int fd, int bs)
{
    GME_REQUIRE(s->mv != nullptr && s->mv_pairs > 0, GME_ERR_STATE, "%s before gme_seq_bbme", who);
    GME_REQUIRE(s->mv_fd == fd && s->mv_bs == bs, GME_ERR_STATE,
                "%s: frame distance %d, block size %d, but the field of the last gme_seq_bbme has %d and %d", who, fd, bs, s->mv_fd,
                s->mv_bs);
    GME_REQUIRE(s->mv_pairs <= s->N - fd, GME_ERR_STATE, "%s: the field has %d pairs, the sequence %d", who, s->mv_pairs, s->N - fd);
    return GME_OK;
}

extern "C" int gme_seq_subpel(gme_seq* s, int fd, int bs, int pnorm, int levels)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_subpel: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = subpel_check("gme_seq_subpel", s->H, s->W, bs, pnorm, levels);
    if (rc) return rc;
    rc = subpel_field(s, "gme_seq_subpel", fd, bs);
    if (rc) return rc;
    const size_t n = (size_t)s->mv_pairs * s->mv_h * s->mv_w;
    s->passes->qmv_valid = false;
    rc = s->passes->qmv.ensure(n * 2, "quarter-pel field");
    if (rc) return rc;
    rc = s->passes->qcost.ensure(n, "quarter-pel costs");
    if (rc) return rc;
    const Plane& p = s->level[2];
    rc = launch_subpel_refine(ctx, p.at(0), p.at(fd), p.stride, s->mv_pairs, s->H, s->W, p.pitch, bs, pnorm, levels, s->mv, s->passes->qmv,
                              s->passes->qcost);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->passes->qmv_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_qmv(gme_seq* s, int first_pair, int count, int32_t* qmf_out, int64_t* cost_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_qmv: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->mv_h * s->mv_w;
    return seq_read(s, "gme_seq_read_qmv", s->passes->qmv_valid, "gme_seq_subpel", "pairs", first_pair, count, s->mv_pairs,
                    { { qmf_out, s->passes->qmv.get(), per * 2 * sizeof(int32_t) }, { cost_out, s->passes->qcost.get(), per * sizeof(long long) } });
}

extern "C" int gme_seq_compensate_qpel(gme_seq* s, int fd, int bs, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_compensate_qpel: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    GME_REQUIRE(s->passes->qmv_valid, GME_ERR_STATE, "gme_seq_compensate_qpel before gme_seq_subpel");
    int rc = subpel_field(s, "gme_seq_compensate_qpel", fd, bs);
    if (rc) return rc;
    const int pairs = s->mv_pairs;
    const Plane& p = s->level[2];
    return seq_predict(s, fd, pairs, sse_out, [&] {
        return launch_compensate_qpel(ctx, p.at(0), p.at(fd), p.stride, pairs, s->H, s->W, p.pitch, bs, s->passes->qmv, s->comp.ptr, s->comp.stride,
                                      s->comp.pitch, s->sse);
    });
}

// ---------------------------------------------------------------------------
// Hierarchical block matching (bbme_hier.hip): blocking calls.  The level-2 field of gme_seq_hier is the
// sequence's motion field (gme_seq_read_mv, gme_seq_subpel, ... take it as they take the field of gme_seq_bbme).
// ---------------------------------------------------------------------------
extern "C" int gme_seq_hier(gme_seq* s, int fd, int bs, int cw, int radius, int pnorm, int levels)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_hier: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    int rc = hier_check_args("gme_seq_hier", bs, cw, radius, pnorm, levels);
    if (rc) return rc;
    const int pairs = s->N - fd, h = s->H / bs, w = s->W / bs;
    const size_t n = (size_t)pairs * h * w;
    seq_field_replaced(s);
    rc = seq_levels(s);
    if (rc) return rc;
    rc = seq_pyramids(s);
    if (rc) return rc;
    rc = s->mv.ensure(n * 2, "motion field");
    if (rc) return rc;
    s->mv_h = h; s->mv_w = w; s->mv_pairs = pairs;
    s->mv_fd = fd; s->mv_bs = bs;
    for (int l = 3 - levels; l < 3; ++l) {
        if (l < 2) {
            rc = s->passes->hier_mv[l].ensure(n * 2, "hierarchical fields");
            if (rc) return rc;
        }
        rc = s->passes->hier_cost[l].ensure(n, "hierarchical costs");
        if (rc) return rc;
    }
    const Plane lv[3] = { s->level[0], s->level[1], s->level[2] };
    int32_t* const mf[3] = { s->passes->hier_mv[0].get(), s->passes->hier_mv[1].get(), s->mv.get() };
    long long* const cost[3] = { s->passes->hier_cost[0].get(), s->passes->hier_cost[1].get(), s->passes->hier_cost[2].get() };
    rc = launch_hier(ctx, lv, 0, fd, pairs, bs, cw, radius, pnorm, levels, mf, cost);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->passes->hier_levels = levels;
    s->passes->hier_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_hier(gme_seq* s, int level, int first_pair, int count, int32_t* mf_out, int64_t* cost_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_hier: null sequence");
    GME_ENTER(s->ctx);
    // the level indexes the table below, and which levels there are is part of the result: both checks come before it
    GME_REQUIRE(s->passes->hier_valid, GME_ERR_STATE, "gme_seq_read_hier before gme_seq_hier");
    GME_REQUIRE(level >= 3 - s->passes->hier_levels && level <= 2, GME_ERR_ARG, "gme_seq_read_hier: level %d, the last gme_seq_hier used %d .. 2",
                level, 3 - s->passes->hier_levels);
    const size_t per = (size_t)s->mv_h * s->mv_w;
    return seq_read(s, "gme_seq_read_hier", s->passes->hier_valid, "gme_seq_hier", "pairs", first_pair, count, s->mv_pairs,
                    { { mf_out, level == 2 ? s->mv.get() : s->passes->hier_mv[level].get(), per * 2 * sizeof(int32_t) },
                      { cost_out, s->passes->hier_cost[level].get(), per * sizeof(long long) } });
}

// ---------------------------------------------------------------------------
// Variable-block-size motion (bbme_vbs.hip): blocking calls on the field of the last gme_seq_bbme or
// gme_seq_hier, which stays the sequence's motion field.
// ---------------------------------------------------------------------------
extern "C" int gme_seq_vbs(gme_seq* s, int fd, int bs, int depth, int radius, int pnorm, int penalty)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_vbs: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = vbs_check_args("gme_seq_vbs", bs, depth, radius, pnorm, penalty);
    if (rc) return rc;
    rc = subpel_field(s, "gme_seq_vbs", fd, bs);
    if (rc) return rc;
    const size_t n = (size_t)s->mv_pairs * s->mv_h * s->mv_w, cells = n << (2 * depth);
    s->passes->vbs_valid = false;
    rc = s->passes->vbs_leaf.ensure(cells * 2, "variable-block-size field");
    if (rc) return rc;
    rc = s->passes->vbs_dmap.ensure(cells, "variable-block-size depths");
    if (rc) return rc;
    rc = s->passes->vbs_cost.ensure(n, "variable-block-size costs");
    if (rc) return rc;
    const Plane& p = s->level[2];
    rc = launch_vbs(ctx, p.at(0), p.at(fd), p.stride, s->mv_pairs, s->H, s->W, p.pitch, bs, depth, radius, pnorm, penalty, s->mv,
                    s->passes->vbs_leaf, s->passes->vbs_dmap, s->passes->vbs_cost);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->passes->vbs_depth = depth;
    s->passes->vbs_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_vbs(gme_seq* s, int first_pair, int count, int32_t* leaf_out, uint8_t* depth_out, int64_t* cost_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_vbs: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->mv_h * s->mv_w, cells = per << (2 * s->passes->vbs_depth);
    return seq_read(s, "gme_seq_read_vbs", s->passes->vbs_valid, "gme_seq_vbs", "pairs", first_pair, count, s->mv_pairs,
                    { { leaf_out, s->passes->vbs_leaf.get(), cells * 2 * sizeof(int32_t) }, { depth_out, s->passes->vbs_dmap.get(), cells },
                      { cost_out, s->passes->vbs_cost.get(), per * sizeof(long long) } });
}

extern "C" int gme_seq_compensate_vbs(gme_seq* s, int fd, int bs, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_compensate_vbs: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    GME_REQUIRE(s->passes->vbs_valid, GME_ERR_STATE, "gme_seq_compensate_vbs before gme_seq_vbs");
    int rc = subpel_field(s, "gme_seq_compensate_vbs", fd, bs);
    if (rc) return rc;
    const int pairs = s->mv_pairs;
    const Plane& p = s->level[2];
    return seq_predict(s, fd, pairs, sse_out, [&] {
        return launch_compensate_vbs(ctx, p.at(0), p.at(fd), p.stride, pairs, s->H, s->W, p.pitch, bs >> s->passes->vbs_depth, s->mv_h << s->passes->vbs_depth,
                                     s->mv_w << s->passes->vbs_depth, s->passes->vbs_leaf, s->comp.ptr, s->comp.stride, s->comp.pitch, s->sse);
    });
}

// ---------------------------------------------------------------------------
// Bidirectional block prediction (bbme_bipred.hip): blocking calls.  gme_seq_bipred runs both searches
// from every target frame itself, into fields of its own, and leaves the sequence's motion field and what was derived from it
// (quarter-pel, hierarchical, variable-block-size results) as they were.
// ---------------------------------------------------------------------------
extern "C" int gme_seq_bipred(gme_seq* s, int fd, int bs, int sw, int procedure, int pnorm, int radius, int rounds, int penalty)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_bipred: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && s->N - fd >= fd + 1, GME_ERR_ARG, "gme_seq_bipred: frame_distance %d needs at least %d frames", fd, 2 * fd + 1);
    int rc = bipred_check_args("gme_seq_bipred", bs, radius, rounds, pnorm, penalty);
    if (rc) return rc;
    rc = bbme_check_args(s->H, s->W, bs, sw, procedure, pnorm);
    if (rc) return rc;
    const int T = s->N - 2 * fd, h = s->H / bs, w = s->W / bs;
    const size_t n = (size_t)T * h * w;
    s->passes->bp_valid = false;
    rc = dev_ensure_all("bidirectional prediction", { { s->passes->bp_f0, n * 2 }, { s->passes->bp_f1, n * 2 }, { s->passes->bp_v0, n * 2 }, { s->passes->bp_v1, n * 2 } });
    if (rc) return rc;
    rc = s->passes->bp_mode.ensure(n, "bidirectional modes");
    if (rc) return rc;
    rc = dev_ensure_all("bidirectional costs", { { s->passes->bp_cost, n }, { s->passes->bp_costs, n * 3 } });
    if (rc) return rc;
    const Plane& p = s->level[2];
    // the anchor of both searches is the target frame t = fd + k; it is looked for in frame t - fd = k and in frame t + fd
    BbmeJob job = bbme_job(p, fd, 0, T, bs, sw, procedure, pnorm, s->passes->bp_f0);
    job.cur = p.at(0);
    rc = seq_launch_bbme_from(s, 2, 0, job);
    if (rc) return rc;
    rc = seq_launch_bbme_from(s, 2, 2 * fd, bbme_job(p, fd, fd, T, bs, sw, procedure, pnorm, s->passes->bp_f1));
    if (rc) return rc;
    rc = launch_bipred(ctx, p.at(0), p.at(fd), p.at(2 * fd), p.stride, T, s->H, s->W, p.pitch, bs, radius, rounds, pnorm, penalty, s->passes->bp_f0,
                       s->passes->bp_f1, s->passes->bp_mode, s->passes->bp_v0, s->passes->bp_v1, s->passes->bp_cost, s->passes->bp_costs);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->passes->bp_targets = T; s->passes->bp_h = h; s->passes->bp_w = w; s->passes->bp_fd = fd; s->passes->bp_bs = bs;
    s->passes->bp_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_bipred(gme_seq* s, int first, int count, int32_t* f0_out, int32_t* f1_out, uint8_t* mode_out, int32_t* v0_out,
                                   int32_t* v1_out, int64_t* cost_out, int64_t* costs_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_bipred: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->passes->bp_h * s->passes->bp_w, vec = per * 2 * sizeof(int32_t);
    return seq_read(s, "gme_seq_read_bipred", s->passes->bp_valid, "gme_seq_bipred", "targets", first, count, s->passes->bp_targets,
                    { { f0_out, s->passes->bp_f0.get(), vec }, { f1_out, s->passes->bp_f1.get(), vec }, { mode_out, s->passes->bp_mode.get(), per },
                      { v0_out, s->passes->bp_v0.get(), vec }, { v1_out, s->passes->bp_v1.get(), vec },
                      { cost_out, s->passes->bp_cost.get(), per * sizeof(long long) }, { costs_out, s->passes->bp_costs.get(), per * 3 * sizeof(long long) } });
}

extern "C" int gme_seq_predict_bipred(gme_seq* s, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_predict_bipred: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(s->passes->bp_valid, GME_ERR_STATE, "gme_seq_predict_bipred before gme_seq_bipred");
    const int T = s->passes->bp_targets, fd = s->passes->bp_fd;
    GME_REQUIRE(T <= s->N - 2 * fd, GME_ERR_STATE, "gme_seq_predict_bipred: %d targets, the sequence has %d", T, s->N - 2 * fd);
    const Plane& p = s->level[2];
    return seq_predict(s, fd, T, sse_out, [&] {
        return launch_predict_bipred(ctx, p.at(0), p.at(fd), p.at(2 * fd), p.stride, T, s->H, s->W, p.pitch, s->passes->bp_bs, s->passes->bp_mode, s->passes->bp_v0,
                                     s->passes->bp_v1, s->comp.ptr, s->comp.stride, s->comp.pitch, s->sse);
    });
}

// ---------------------------------------------------------------------------
// Global motion compensation (bbme_gmc.hip): blocking calls.  gme_seq_gmc runs the search from every
// predicted frame itself, into a field of its own, and leaves the sequence's motion field and what was derived from it
// (quarter-pel, hierarchical, variable-block-size and bidirectional results) as they were.
// ---------------------------------------------------------------------------
extern "C" int gme_seq_gmc(gme_seq* s, int fd, int bs, int sw, int procedure, int pnorm, int penalty, const double* h)
{
    GME_REQUIRE(s != nullptr && h != nullptr, GME_ERR_ARG, "gme_seq_gmc: null pointer");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "gme_seq_gmc: frame_distance %d needs at least %d frames", fd, fd + 1);
    int rc = gmc_check_args("gme_seq_gmc", bs, pnorm, penalty);
    if (rc) return rc;
    rc = bbme_check_args(s->H, s->W, bs, sw, procedure, pnorm);
    if (rc) return rc;
    const int P = s->N - fd, hb = s->H / bs, wb = s->W / bs;
    const size_t n = (size_t)P * hb * wb;
    s->passes->gm_valid = false;
    rc = s->passes->gm_f.ensure(n * 2, "global motion compensation field");
    if (rc) return rc;
    rc = s->passes->gm_h.ensure((size_t)P * 8, "global motion compensation warps");
    if (rc) return rc;
    rc = dev_ensure_all("global motion compensation modes", { { s->passes->gm_usable, (size_t)P }, { s->passes->gm_mode, n } });
    if (rc) return rc;
    rc = dev_ensure_all("global motion compensation costs", { { s->passes->gm_cost, n }, { s->passes->gm_costs, n * 2 } });
    if (rc) return rc;
    // unusable warps are found here, before the launch: the kernels take a flag per pair
    std::vector<uint8_t> usable((size_t)P);
    for (int k = 0; k < P; ++k) usable[(size_t)k] = gmc_usable(h + (size_t)k * 8, s->H, s->W) ? 1 : 0;
    GME_HIP_TRY(hipMemcpyAsync(s->passes->gm_h, h, (size_t)P * 8 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    GME_HIP_TRY(hipMemcpyAsync(s->passes->gm_usable, usable.data(), (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    const Plane& p = s->level[2];
    // the anchor of the search is the predicted frame k + fd; it is looked for in frame k
    BbmeJob job = bbme_job(p, fd, 0, P, bs, sw, procedure, pnorm, s->passes->gm_f);
    job.cur = p.at(0);
    rc = seq_launch_bbme_from(s, 2, 0, job);
    if (rc) return rc;
    rc = launch_gmc(ctx, p.at(0), p.at(fd), p.stride, P, s->H, s->W, p.pitch, bs, pnorm, penalty, s->passes->gm_h, s->passes->gm_usable, s->passes->gm_f, s->passes->gm_mode,
                    s->passes->gm_cost, s->passes->gm_costs);
    if (rc) return rc;
    rc = ctx_finish(ctx);                                      // `usable` is read by its copy until here
    if (rc) return rc;
    s->passes->gm_pairs = P; s->passes->gm_h_blocks = hb; s->passes->gm_w_blocks = wb; s->passes->gm_fd = fd; s->passes->gm_bs = bs;
    s->passes->gm_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_gmc(gme_seq* s, int first, int count, int32_t* f_out, uint8_t* mode_out, int64_t* cost_out, int64_t* costs_out,
                                uint8_t* usable_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_gmc: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->passes->gm_h_blocks * s->passes->gm_w_blocks;
    return seq_read(s, "gme_seq_read_gmc", s->passes->gm_valid, "gme_seq_gmc", "pairs", first, count, s->passes->gm_pairs,
                    { { f_out, s->passes->gm_f.get(), per * 2 * sizeof(int32_t) }, { mode_out, s->passes->gm_mode.get(), per },
                      { cost_out, s->passes->gm_cost.get(), per * sizeof(long long) }, { costs_out, s->passes->gm_costs.get(), per * 2 * sizeof(long long) },
                      { usable_out, s->passes->gm_usable.get(), 1 } });                  // one flag per pair, whatever the block grid
}

extern "C" int gme_seq_predict_gmc(gme_seq* s, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_predict_gmc: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(s->passes->gm_valid, GME_ERR_STATE, "gme_seq_predict_gmc before gme_seq_gmc");
    const int P = s->passes->gm_pairs, fd = s->passes->gm_fd;
    GME_REQUIRE(P <= s->N - fd, GME_ERR_STATE, "gme_seq_predict_gmc: %d pairs, the sequence has %d", P, s->N - fd);
    const Plane& p = s->level[2];
    return seq_predict(s, fd, P, sse_out, [&] {
        return launch_predict_gmc(ctx, p.at(0), p.at(fd), p.stride, P, s->H, s->W, p.pitch, s->passes->gm_bs, s->passes->gm_h, s->passes->gm_usable, s->passes->gm_mode, s->passes->gm_f,
                                  s->comp.ptr, s->comp.stride, s->comp.pitch, s->sse);
    });
}

// ---------------------------------------------------------------------------
// Vector propagation search (bbme_prop.hip): blocking calls.  gme_seq_prop takes the field of the last
// gme_seq_bbme, gme_seq_hier or gme_seq_prop as the prior F_0 and leaves its result as the sequence's motion field; with
// `temporal`, pair k >= 1 also scores F_0 of pair k - 1 (the prior field, not the propagated one: the pairs stay independent
// and go into one launch per round).  The rounds write fields of their own and the last one is copied over F_0 behind them, so
// F_0 is whole while any round reads it.  Quarter-pel, hierarchical and variable-block-size results of the old field end here;
// the bidirectional and global-motion-compensation results stay.
// ---------------------------------------------------------------------------
extern "C" int gme_seq_prop(gme_seq* s, int fd, int bs, int pnorm, int rounds, int steps, int temporal, const int32_t* g)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_prop: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = prop_check_args("gme_seq_prop", bs, pnorm, rounds, steps);
    if (rc) return rc;
    rc = subpel_field(s, "gme_seq_prop", fd, bs);
    if (rc) return rc;
    const int P = s->mv_pairs;
    const size_t n = (size_t)P * s->mv_h * s->mv_w;
    s->passes->prop_valid = false;
    rc = dev_ensure_all("vector propagation fields", { { s->passes->prop_work[0], n * 2 }, { s->passes->prop_work[1], n * 2 } });
    if (rc) return rc;
    if (g) {
        rc = s->passes->prop_g.ensure(n * 2, "camera field");
        if (rc) return rc;
    }
    rc = s->passes->prop_cost.ensure(n, "vector propagation costs");
    if (rc) return rc;
    rc = s->passes->prop_source.ensure(n, "vector propagation sources");
    if (rc) return rc;
    if (n == 0) {
        s->passes->prop_valid = true;
        return GME_OK;
    }
    seq_field_replaced(s);
    if (g) GME_HIP_TRY(hipMemcpyAsync(s->passes->prop_g, g, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const Plane& p = s->level[2];
    int32_t* const work[2] = { s->passes->prop_work[0].get(), s->passes->prop_work[1].get() };
    int32_t* result = nullptr;
    rc = launch_prop(ctx, p.at(0), p.at(fd), p.stride, P, s->H, s->W, p.pitch, bs, pnorm, rounds, steps, s->mv, temporal ? s->mv.get() : nullptr,
                     -1, g ? s->passes->prop_g.get() : nullptr, work, s->passes->prop_cost, s->passes->prop_source, &result);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(s->mv, result, n * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    rc = ctx_finish(ctx);                                      // `g` is read by its copy until here
    if (rc) return rc;
    s->passes->prop_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_prop(gme_seq* s, int first_pair, int count, int32_t* mf_out, int64_t* cost_out, uint8_t* source_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_prop: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->mv_h * s->mv_w;
    return seq_read(s, "gme_seq_read_prop", s->passes->prop_valid, "gme_seq_prop", "pairs", first_pair, count, s->mv_pairs,
                    { { mf_out, s->mv.get(), per * 2 * sizeof(int32_t) }, { cost_out, s->passes->prop_cost.get(), per * sizeof(long long) },
                      { source_out, s->passes->prop_source.get(), per } });
}

// ---------------------------------------------------------------------------
// Motion-compensated frame interpolation (bbme_interp.hip): one blocking call that computes and returns.
// It works in buffers of its own that live as long as the call, keeps no result and touches nothing the sequence holds (not the
// motion field, not the compensated planes): there is nothing of it that a later call could read stale.
// ---------------------------------------------------------------------------
extern "C" int gme_seq_interp(gme_seq* s, int fd, int bs, int sw, int pnorm, int bias, int first_pair, int count, int32_t* mv_out,
                              int64_t* cost_out, int64_t* dist_out, uint8_t* frames_out, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_interp: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "gme_seq_interp: frame_distance %d needs at least %d frames", fd, fd + 1);
    int rc = interp_check_args("gme_seq_interp", s->H, s->W, bs, sw, pnorm, bias);
    if (rc) return rc;
    const int P = s->N - fd;
    GME_REQUIRE(first_pair >= 0 && count >= 0 && first_pair + count <= P, GME_ERR_ARG, "gme_seq_interp: pairs [%d, %d) outside [0, %d)",
                first_pair, first_pair + count, P);
    const size_t per = (size_t)(s->H / bs) * (s->W / bs), image = (size_t)s->H * s->W;
    const bool truth = fd % 2 == 0, frames = frames_out || (sse_out && truth);
    if (sse_out && !truth)
        for (int k = 0; k < count; ++k) sse_out[k] = -1;
    const int step = max_grid_planes(), most = count < step ? count : step;
    DevBuf<int32_t> mv;
    DevBuf<long long> cost;                                    // per chunk: J of every block, then D of every block
    DevBuf<unsigned long long> sse;
    PlaneBuf made;
    rc = mv.ensure(per * 2 * most, "interpolation vectors");
    if (rc) return rc;
    rc = cost.ensure(per * 2 * most, "interpolation costs");
    if (rc) return rc;
    if (frames) {
        rc = sse.ensure((size_t)most, "interpolation errors");
        if (rc) return rc;
        rc = plane_alloc(ctx, &made, most, s->H, s->W);
        if (rc) return rc;
    }
    const Plane& p = s->level[2];
    for (int k = 0; k < count; k += step) {
        const int n = count - k < step ? count - k : step, at = first_pair + k;
        long long* dist = cost.get() + per * n;
        rc = launch_interp(ctx, p.at(at), p.at(at + fd), p.stride, n, s->H, s->W, p.pitch, bs, sw, pnorm, bias, mv, cost, dist);
        if (rc) return rc;
        if (mv_out) GME_HIP_TRY(hipMemcpyAsync(mv_out + per * 2 * k, mv.get(), per * 2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (cost_out) GME_HIP_TRY(hipMemcpyAsync(cost_out + per * k, cost.get(), per * n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        if (dist_out) GME_HIP_TRY(hipMemcpyAsync(dist_out + per * k, dist, per * n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        if (frames) {
            rc = launch_interp_frame(ctx, p.at(at), p.at(at + fd), p.at(truth ? at + fd / 2 : at), p.stride, n, s->H, s->W, p.pitch, bs, mv,
                                     made.ptr, made.stride, made.pitch, sse);
            if (rc) return rc;
            if (frames_out) {
                rc = read_planes(ctx, made, 0, n, frames_out + image * k);
                if (rc) return rc;
            }
            if (sse_out && truth)
                GME_HIP_TRY(hipMemcpyAsync(sse_out + k, sse.get(), (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        }
        rc = ctx_finish(ctx);                                  // the next chunk writes the same buffers
        if (rc) return rc;
    }
    return GME_OK;
}

// ---------------------------------------------------------------------------
// Overlapped block motion compensation (bbme_obmc.hip): one blocking call that computes and returns, in the
// form of gme_seq_interp.  It reads the sequence's motion field (unit 4) or its quarter-pel field (unit 1), works in buffers of its
// own that live as long as the call and keeps nothing: it writes neither the compensated planes nor any field, so there is
// nothing of it that a later call could read stale.
// ---------------------------------------------------------------------------
extern "C" int gme_seq_obmc(gme_seq* s, int fd, int bs, int unit, int first_pair, int count, uint8_t* frames_out, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_obmc: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "gme_seq_obmc: frame_distance %d needs at least %d frames", fd, fd + 1);
    int rc = obmc_check_args("gme_seq_obmc", s->H, s->W, bs, unit);
    if (rc) return rc;
    GME_REQUIRE(unit == 4 || s->passes->qmv_valid, GME_ERR_STATE, "gme_seq_obmc with the quarter-pel field before gme_seq_subpel");
    rc = subpel_field(s, "gme_seq_obmc", fd, bs);
    if (rc) return rc;
    GME_REQUIRE(first_pair >= 0 && count >= 0 && first_pair + count <= s->mv_pairs, GME_ERR_ARG, "gme_seq_obmc: pairs [%d, %d) outside [0, %d)",
                first_pair, first_pair + count, s->mv_pairs);
    const size_t per = (size_t)s->mv_h * s->mv_w, image = (size_t)s->H * s->W;
    const int32_t* field = unit == 4 ? s->mv.get() : s->passes->qmv.get();
    const int step = max_grid_planes(), most = count < step ? count : step;
    DevBuf<unsigned long long> sse;
    PlaneBuf made;
    rc = sse.ensure((size_t)most, "overlapped compensation errors");
    if (rc) return rc;
    rc = plane_alloc(ctx, &made, most, s->H, s->W);
    if (rc) return rc;
    const Plane& p = s->level[2];
    for (int k = 0; k < count; k += step) {
        const int n = count - k < step ? count - k : step, at = first_pair + k;
        rc = launch_obmc(ctx, p.at(at), p.at(at + fd), p.stride, n, s->H, s->W, p.pitch, bs, field + per * 2 * at, unit, made.ptr, made.stride,
                         made.pitch, sse);
        if (rc) return rc;
        if (frames_out) {
            rc = read_planes(ctx, made, 0, n, frames_out + image * k);
            if (rc) return rc;
        }
        if (sse_out) GME_HIP_TRY(hipMemcpyAsync(sse_out + k, sse.get(), (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        rc = ctx_finish(ctx);                                  // the next chunk writes the same buffers
        if (rc) return rc;
    }
    return GME_OK;
}

// ---------------------------------------------------------------------------
// Motion-compensated temporal denoising (bbme_denoise.hip): one blocking call that computes and returns, in
// the form of gme_seq_obmc.  For every chunk of targets and each of the 2 radius references it runs the search from the target
// into a field of its own (as gme_seq_bipred and gme_seq_gmc do), the sub-pel refinement where asked for, and the overlapped
// prediction; then the filter.  All its buffers live as long as the call and it keeps nothing: it writes neither the motion
// field, the quarter-pel field, the compensated planes nor any other kept result, so there is nothing of it that a later call
// could read stale.
// ---------------------------------------------------------------------------
extern "C" int gme_seq_denoise(gme_seq* s, int fd, int bs, int sw, int procedure, int pnorm, int radius, int levels, int strength,
                               int first_target, int count, uint8_t* frames_out, int64_t* change_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_denoise: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(radius >= 1 && radius <= 2, GME_ERR_ARG, "gme_seq_denoise: radius %d (1 .. 2)", radius);
    GME_REQUIRE(fd >= 1 && fd <= (s->N - 1) / (2 * radius), GME_ERR_ARG, "gme_seq_denoise: frame_distance %d at radius %d needs at least %lld frames",
                fd, radius, 2ll * radius * fd + 1);
    const int R = 2 * radius;
    int rc = denoise_check_args("gme_seq_denoise", R, strength);
    if (rc) return rc;
    rc = obmc_check_args("gme_seq_denoise", s->H, s->W, bs, 4);
    if (rc) return rc;
    rc = bbme_check_args(s->H, s->W, bs, sw, procedure, pnorm);
    if (rc) return rc;
    rc = subpel_check("gme_seq_denoise", s->H, s->W, bs, pnorm, levels);
    if (rc) return rc;
    const int reach = radius * fd, T = s->N - 2 * reach;
    GME_REQUIRE(first_target >= 0 && count >= 0 && first_target <= T - count, GME_ERR_ARG, "gme_seq_denoise: targets [%d, %lld) outside [0, %d)",
                first_target, (long long)first_target + count, T);
    if (count == 0) return GME_OK;
    const size_t per = (size_t)(s->H / bs) * (s->W / bs), image = (size_t)s->H * s->W;
    const int step = max_grid_planes(), most = count < step ? count : step;
    DevBuf<int32_t> mf, qmf;
    DevBuf<long long> qcost;
    DevBuf<unsigned long long> sse;                            // [most] of the filter, then [most] of a prediction (not reported)
    PlaneBuf preds, made;                                      // preds: reference r's planes at r * most
    rc = mf.ensure(per * 2 * most, "denoising field");
    if (rc) return rc;
    if (levels > 0) {
        rc = qmf.ensure(per * 2 * most, "denoising quarter-pel field");
        if (rc) return rc;
        rc = qcost.ensure(per * most, "denoising quarter-pel costs");
        if (rc) return rc;
    }
    rc = sse.ensure((size_t)most * 2, "denoising errors");
    if (rc) return rc;
    rc = plane_alloc(ctx, &preds, most * R, s->H, s->W);
    if (rc) return rc;
    rc = plane_alloc(ctx, &made, most, s->H, s->W);
    if (rc) return rc;
    const Plane& p = s->level[2];
    for (int k = 0; k < count; k += step) {
        const int n = count - k < step ? count - k : step, t0 = reach + first_target + k;
        for (int r = 0; r < R; ++r) {
            // reference r of target t: t - fd, t + fd, t - 2 fd, t + 2 fd.  The anchor of the search is the target.
            const int d = (r / 2 + 1) * fd, ref0 = r % 2 == 0 ? t0 - d : t0 + d;
            BbmeJob job = bbme_job(p, t0, 0, n, bs, sw, procedure, pnorm, mf);
            job.cur = p.at(ref0);
            rc = seq_launch_bbme_from(s, 2, ref0, job);
            if (rc) return rc;
            if (levels > 0) {
                rc = launch_subpel_refine(ctx, p.at(t0), p.at(ref0), p.stride, n, s->H, s->W, p.pitch, bs, pnorm, levels, mf, qmf, qcost);
                if (rc) return rc;
            }
            rc = launch_obmc(ctx, p.at(ref0), p.at(t0), p.stride, n, s->H, s->W, p.pitch, bs, levels > 0 ? qmf.get() : mf.get(), levels > 0 ? 1 : 4,
                             preds.at(r * most), preds.stride, preds.pitch, sse.get() + most, true);
            if (rc) return rc;
        }
        rc = launch_denoise(ctx, p.at(t0), p.stride, preds.ptr, (long long)most * preds.stride, preds.stride, n, R, s->H, s->W, p.pitch, strength,
                            p.at(t0), p.stride, made.ptr, made.stride, made.pitch, sse);
        if (rc) return rc;
        if (frames_out) {
            rc = read_planes(ctx, made, 0, n, frames_out + image * k);
            if (rc) return rc;
        }
        if (change_out)
            GME_HIP_TRY(hipMemcpyAsync(change_out + k, sse.get(), (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        rc = ctx_finish(ctx);                                  // the next chunk writes the same buffers
        if (rc) return rc;
    }
    return GME_OK;
}
