// C ABI of libgme_hip.so (include/gme_hip.h), the whole-frame passes built on the core of gme_api.hip, all on a resident
// sequence: direct projective refinement (gme_direct.hip), stabilization and border fill (gme_stab.hip, gme_stab_fill.hip),
// background mosaic and moving-object masks (gme_mosaic.hip).  What they keep lives in SeqPasses (gme_passes.h).
#include <vector>

#include "gme_passes.h"

// ---------------------------------------------------------------------------
// Direct projective refinement (gme_direct.hip): pyramids if stale, parameters up, every launch
// queued, results down, one wait.
// ---------------------------------------------------------------------------
static int direct_begin(gme_seq* s, const char* who, int fd, const double* params, DirectIo* io)
{
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "%s: frame_distance %d needs at least %d frames", who, fd, fd + 1);
    int rc = seq_levels(s);
    if (rc) return rc;
    rc = seq_pyramids(s);
    if (rc) return rc;
    const int pairs = s->N - fd;
    rc = direct_io(s, pairs, io);
    if (rc) return rc;
    if (pairs > 0) GME_HIP_TRY(hipMemcpyAsync(io->in, params, (size_t)pairs * 8 * sizeof(double), hipMemcpyHostToDevice, s->ctx->stream));
    return GME_OK;
}

extern "C" int gme_seq_direct_eval(gme_seq* s, int fd, int level, const double* params_in, double outlier_fraction,
                                   double* threshold_out, int64_t* counts_out, double* cost_out, double* sums_out)
{
    GME_REQUIRE(s != nullptr && params_in != nullptr, GME_ERR_ARG, "gme_seq_direct_eval: null pointer");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(level >= 0 && level <= 2, GME_ERR_ARG, "gme_seq_direct_eval: level %d (0 .. 2)", level);
    GME_REQUIRE(outlier_fraction >= 0.0 && outlier_fraction < 1.0, GME_ERR_ARG, "gme_seq_direct_eval: outlier_fraction %g", outlier_fraction);
    DirectIo io;
    int rc = direct_begin(s, "gme_seq_direct_eval", fd, params_in, &io);
    if (rc) return rc;
    const int pairs = s->N - fd;
    if (pairs == 0) return GME_OK;
    rc = launch_direct_eval(s, fd, level, pairs, outlier_fraction);
    if (rc) return rc;
    std::vector<double> rows((size_t)pairs * 48);
    GME_HIP_TRY(hipMemcpyAsync(rows.data(), io.eval, rows.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    rc = ctx_finish(ctx);
    if (rc) return rc;
    for (int p = 0; p < pairs; ++p) {
        const double* r = rows.data() + (size_t)p * 48;
        if (threshold_out) threshold_out[p] = r[0];
        if (counts_out) { counts_out[2 * p] = (int64_t)r[1]; counts_out[2 * p + 1] = (int64_t)r[2]; }
        if (cost_out) cost_out[p] = r[3];
        if (sums_out) memcpy(sums_out + (size_t)p * 44, r + 4, 44 * sizeof(double));
    }
    return GME_OK;
}

extern "C" int gme_seq_refine_projective(gme_seq* s, int fd, const double* init, double outlier_fraction, int max_iters,
                                         double* params_out, int32_t* flags_out)
{
    GME_REQUIRE(s != nullptr && init != nullptr && params_out != nullptr && flags_out != nullptr, GME_ERR_ARG,
                "gme_seq_refine_projective: null pointer");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(outlier_fraction >= 0.0 && outlier_fraction < 1.0, GME_ERR_ARG, "gme_seq_refine_projective: outlier_fraction %g",
                outlier_fraction);
    GME_REQUIRE(max_iters >= 1 && max_iters <= 1000, GME_ERR_ARG, "gme_seq_refine_projective: max_iters %d (1 .. 1000)", max_iters);
    DirectIo io;
    int rc = direct_begin(s, "gme_seq_refine_projective", fd, init, &io);
    if (rc) return rc;
    const int pairs = s->N - fd;
    if (pairs == 0) return GME_OK;
    rc = launch_direct_refine(s, fd, pairs, outlier_fraction, max_iters);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(params_out, io.out, (size_t)pairs * 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GME_HIP_TRY(hipMemcpyAsync(flags_out, io.flags, (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

extern "C" int gme_seq_compensate_projective(gme_seq* s, int fd, const double* params, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr && params != nullptr, GME_ERR_ARG, "gme_seq_compensate_projective: null pointer");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    DirectIo io;
    int rc = direct_begin(s, "gme_seq_compensate_projective", fd, params, &io);
    if (rc) return rc;
    const int pairs = s->N - fd;
    rc = ensure_comp(s, fd, pairs);
    if (rc) return rc;
    if (pairs == 0) return GME_OK;
    rc = launch_compensate_proj(s, fd, pairs, io.in);
    if (rc) return rc;
    comp_wrote(s, pairs);
    if (sse_out) GME_HIP_TRY(hipMemcpyAsync(sse_out, s->sse, (size_t)pairs * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

// ---------------------------------------------------------------------------
// Video stabilization (gme_stab.hip): blocking calls on the resident frames.
// ---------------------------------------------------------------------------
static int stab_buffers(gme_seq* s)
{
    if (s->passes->warped.ptr) return GME_OK;
    int rc = plane_alloc(s->ctx, &s->passes->warped, s->N_cap, s->H, s->W);
    if (rc == GME_OK)
        rc = dev_ensure_all("stabilization buffers", { { s->passes->warp_params, (size_t)s->N_cap * 8 }, { s->passes->warp_counts, (size_t)s->N_cap } });
    if (rc) { s->passes->warped = PlaneBuf(); s->passes->warped_written.flag.clear(); return rc; }
    s->passes->warped_written.flag.assign((size_t)s->N_cap, 0);
    return GME_OK;
}

extern "C" int gme_seq_warp_frames(gme_seq* s, int first, int count, const double* params, int border, int fill,
                                   int64_t* valid_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_warp_frames: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(first >= 0 && count >= 0 && first + count <= s->N, GME_ERR_ARG, "gme_seq_warp_frames: frames [%d, %d) outside [0, %d)",
                first, first + count, s->N);
    GME_REQUIRE(params != nullptr || count == 0, GME_ERR_ARG, "gme_seq_warp_frames: null parameters");
    GME_REQUIRE(border == 0 || border == 1, GME_ERR_ARG, "gme_seq_warp_frames: border %d (0 constant, 1 replicate)", border);
    GME_REQUIRE(fill >= 0 && fill <= 255, GME_ERR_ARG, "gme_seq_warp_frames: fill %d (0 .. 255)", fill);
    if (count == 0) return GME_OK;
    int rc = stab_buffers(s);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(s->passes->warp_params, params, (size_t)count * 8 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_warp_frames(ctx, s->level[2], s->passes->warped, first, count, s->passes->warp_params, border, fill, s->passes->warp_counts);
    if (rc) return rc;
    if (valid_out)
        GME_HIP_TRY(hipMemcpyAsync(valid_out, s->passes->warp_counts, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   ctx->stream));
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->passes->warped_written.mark(first, count);
    return GME_OK;
}

extern "C" int gme_seq_read_warped_range(gme_seq* s, int first, int count, uint8_t* out)
{
    GME_REQUIRE(s != nullptr && out != nullptr, GME_ERR_ARG, "gme_seq_read_warped_range: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(first >= 0 && count >= 0 && first + count <= s->N, GME_ERR_ARG,
                "gme_seq_read_warped_range: frames [%d, %d) outside [0, %d)", first, first + count, s->N);
    GME_REQUIRE(s->passes->warped_written.all(first, count), GME_ERR_ARG, "gme_seq_read_warped_range: frames [%d, %d) were never warped",
                first, first + count);
    const int rc = read_planes(s->ctx, s->passes->warped, first, count, out);
    return rc ? rc : ctx_finish(s->ctx);
}

extern "C" int gme_seq_frame_sse(gme_seq* s, int warped, int first, int count, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr && sse_out != nullptr, GME_ERR_ARG, "gme_seq_frame_sse: null pointer");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(warped == 0 || warped == 1, GME_ERR_ARG, "gme_seq_frame_sse: warped %d (0 resident, 1 warped frames)", warped);
    GME_REQUIRE(first >= 0 && count >= 0 && first + count + 1 <= s->N, GME_ERR_ARG,
                "gme_seq_frame_sse: frames [%d, %d] outside [0, %d)", first, first + count, s->N);
    if (count == 0) return GME_OK;
    GME_REQUIRE(!warped || s->passes->warped_written.all(first, count + 1), GME_ERR_ARG, "gme_seq_frame_sse: frames [%d, %d] were never warped",
                first, first + count);
    int rc = stab_buffers(s);
    if (rc) return rc;
    rc = launch_frame_sse(ctx, warped ? s->passes->warped : s->level[2], first, count, s->passes->warp_counts);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(sse_out, s->passes->warp_counts, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

// ---------------------------------------------------------------------------
// Full-frame stabilization (gme_stab_fill.hip): one blocking call that computes and returns, in the form
// of gme_seq_obmc.  The output frames, the winning candidates, the counts and the candidate rows live in buffers of the
// call's own; it touches neither the sequence's warped planes and their written flags nor any other kept result, so there
// is nothing of it that a later call could read stale.  The source frames are absolute resident indices, so the whole
// range is warped into one buffer (chunked over output frames by the launcher) and the squared errors are taken there.
// ---------------------------------------------------------------------------
extern "C" int gme_seq_warp_fill(gme_seq* s, int first, int count, int n_cand, const int32_t* sources, const double* warps, int border,
                                 int fill, uint8_t* frames_out, uint8_t* source_out, int64_t* valid_out, int64_t* filled_out,
                                 int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_warp_fill: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(first >= 0 && count >= 0 && first <= s->N - count, GME_ERR_ARG, "gme_seq_warp_fill: frames [%d, %lld) outside [0, %d)",
                first, (long long)first + count, s->N);
    GME_REQUIRE(n_cand >= 1 && n_cand <= 17, GME_ERR_ARG, "gme_seq_warp_fill: %d candidates (1 .. 17)", n_cand);
    GME_REQUIRE((sources != nullptr && warps != nullptr) || count == 0, GME_ERR_ARG, "gme_seq_warp_fill: null sources or warps");
    GME_REQUIRE(border == 0 || border == 1, GME_ERR_ARG, "gme_seq_warp_fill: border %d (0 constant, 1 replicate)", border);
    GME_REQUIRE(fill >= 0 && fill <= 255, GME_ERR_ARG, "gme_seq_warp_fill: fill %d (0 .. 255)", fill);
    const size_t rows = (size_t)count * n_cand;
    for (size_t i = 0; i < rows; ++i) {
        GME_REQUIRE(sources[i] >= -1 && sources[i] < s->N, GME_ERR_ARG, "gme_seq_warp_fill: source %d of frame %d outside -1 .. %d",
                    sources[i], first + (int)(i / n_cand), s->N - 1);
        GME_REQUIRE(i % n_cand != 0 || sources[i] >= 0, GME_ERR_ARG, "gme_seq_warp_fill: candidate 0 of frame %d is not a frame",
                    first + (int)(i / n_cand));
    }
    if (count == 0) return GME_OK;
    DevBuf<int32_t> cand;
    DevBuf<double> par;
    DevBuf<unsigned long long> counts;                         // valid [count] | filled [count] | sse [count - 1]
    PlaneBuf made, who;
    int rc = dev_ensure_all("fill candidates", { { cand, rows }, { par, rows * 8 }, { counts, (size_t)count * 3 } });
    if (rc) return rc;
    rc = plane_alloc(ctx, &made, count, s->H, s->W);
    if (rc) return rc;
    if (source_out) {
        rc = plane_alloc(ctx, &who, count, s->H, s->W);
        if (rc) return rc;
    }
    GME_HIP_TRY(hipMemcpyAsync(cand.get(), sources, rows * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    GME_HIP_TRY(hipMemcpyAsync(par.get(), warps, rows * 8 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    unsigned long long *valid = counts.get(), *filled = valid + count, *sse = filled + count;
    rc = launch_warp_fill(ctx, s->level[2], made, who, count, n_cand, cand, par, border, fill, valid, filled);
    if (rc) return rc;
    if (sse_out) {
        rc = launch_frame_sse(ctx, made, 0, count - 1, sse);
        if (rc) return rc;
    }
    const hipStream_t st = ctx->stream;
    if (frames_out) {
        rc = read_planes(ctx, made, 0, count, frames_out);
        if (rc) return rc;
    }
    if (source_out) {
        rc = read_planes(ctx, who, 0, count, source_out);
        if (rc) return rc;
    }
    if (valid_out) GME_HIP_TRY(hipMemcpyAsync(valid_out, valid, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (filled_out) GME_HIP_TRY(hipMemcpyAsync(filled_out, filled, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (sse_out && count > 1)
        GME_HIP_TRY(hipMemcpyAsync(sse_out, sse, (size_t)(count - 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    return ctx_finish(ctx);                                    // the buffers are freed behind a drained stream
}

// ---------------------------------------------------------------------------
// Background mosaic and moving-object masks (gme_mosaic.hip): blocking calls on the resident frames.
// ---------------------------------------------------------------------------
static int mosaic_rows(gme_seq* s)
{
    if (s->passes->mosaic_params) return GME_OK;
    return dev_ensure_all("mosaic parameters", { { s->passes->mosaic_params, (size_t)s->N_cap * 8 }, { s->passes->mosaic_usable, (size_t)s->N_cap },
                                                 { s->passes->mosaic_counts, (size_t)s->N_cap * 2 } });
}

// the per-frame rows of a call: parameters and usable flags (all ones for NULL) to the device
static int mosaic_put_rows(gme_seq* s, int count, const double* params, const uint8_t* usable)
{
    hipStream_t st = s->ctx->stream;
    GME_HIP_TRY(hipMemcpyAsync(s->passes->mosaic_params, params, (size_t)count * 8 * sizeof(double), hipMemcpyHostToDevice, st));
    if (usable) GME_HIP_TRY(hipMemcpyAsync(s->passes->mosaic_usable, usable, (size_t)count, hipMemcpyHostToDevice, st));
    else GME_HIP_TRY(hipMemsetAsync(s->passes->mosaic_usable, 1, (size_t)count, st));
    return GME_OK;
}

extern "C" int gme_seq_mosaic(gme_seq* s, int first, int count, const double* inv_warps, const uint8_t* usable, int ox, int oy,
                              int Hc, int Wc, int fill, int cull)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_mosaic: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(first >= 0 && count >= 1 && first + count <= s->N, GME_ERR_ARG, "gme_seq_mosaic: frames [%d, %d) outside [0, %d)",
                first, first + count, s->N);
    GME_REQUIRE(count <= 65535, GME_ERR_ARG, "gme_seq_mosaic: %d frames (the sample counts are 16 bits: at most 65535)", count);
    GME_REQUIRE(inv_warps != nullptr, GME_ERR_ARG, "gme_seq_mosaic: null parameters");
    GME_REQUIRE(Hc >= 1 && Wc >= 1 && (long long)Hc * round_up(Wc, 64) <= 0x7FFFFFFFLL && Wc <= 0x7FFFFFFF - 64, GME_ERR_ARG,
                "gme_seq_mosaic: canvas %d x %d (1 x 1 .. 2^31 - 1 pixels, rows padded to 64)", Hc, Wc);
    GME_REQUIRE(fill >= 0 && fill <= 255, GME_ERR_ARG, "gme_seq_mosaic: fill %d (0 .. 255)", fill);
    GME_REQUIRE(cull == 0 || cull == 1, GME_ERR_ARG, "gme_seq_mosaic: cull %d (0 off, 1 on)", cull);
    int rc = mosaic_rows(s);
    if (rc) return rc;
    const int pitch = round_up(Wc, 64);
    const size_t pixels = (size_t)Hc * (size_t)pitch;
    s->passes->mosaic_valid = false;
    if (pixels > s->passes->mosaic_sprite.cap) {
        s->passes->mosaic_sprite.reset(); s->passes->mosaic_count.reset();     // both go before either comes back: no more memory at the peak
        rc = dev_ensure_all("mosaic", { { s->passes->mosaic_sprite, pixels }, { s->passes->mosaic_count, pixels } });
        if (rc) return rc;
    }
    GME_HIP_TRY(hipMemsetAsync(s->passes->mosaic_sprite, 0, pixels, ctx->stream));
    GME_HIP_TRY(hipMemsetAsync(s->passes->mosaic_count, 0, pixels * sizeof(uint16_t), ctx->stream));
    rc = mosaic_put_rows(s, count, inv_warps, usable);
    if (rc) return rc;
    rc = launch_mosaic_median(ctx, s->level[2], first, count, s->passes->mosaic_params, s->passes->mosaic_usable, ox, oy, Hc, Wc, fill, cull,
                              s->passes->mosaic_sprite, s->passes->mosaic_count, pitch);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->passes->mosaic_Hc = Hc; s->passes->mosaic_Wc = Wc; s->passes->mosaic_pitch = pitch;
    s->passes->mosaic_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_mosaic(gme_seq* s, uint8_t* sprite, uint16_t* count)
{
    GME_REQUIRE(s != nullptr && sprite != nullptr, GME_ERR_ARG, "gme_seq_read_mosaic: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(s->passes->mosaic_valid, GME_ERR_ARG, "gme_seq_read_mosaic: no mosaic was built (gme_seq_mosaic first)");
    const int Hc = s->passes->mosaic_Hc, Wc = s->passes->mosaic_Wc, pitch = s->passes->mosaic_pitch;
    GME_HIP_TRY(hipMemcpy2DAsync(sprite, Wc, s->passes->mosaic_sprite, pitch, Wc, Hc, hipMemcpyDeviceToHost, s->ctx->stream));
    if (count)
        GME_HIP_TRY(hipMemcpy2DAsync(count, (size_t)Wc * sizeof(uint16_t), s->passes->mosaic_count, (size_t)pitch * sizeof(uint16_t),
                                     (size_t)Wc * sizeof(uint16_t), Hc, hipMemcpyDeviceToHost, s->ctx->stream));
    return ctx_finish(s->ctx);
}

extern "C" int gme_seq_moving_masks(gme_seq* s, int first, int count, const double* warps, const uint8_t* usable, int ox, int oy,
                                    int threshold, int min_count, int64_t* known_out, int64_t* moving_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_moving_masks: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(first >= 0 && count >= 0 && first + count <= s->N, GME_ERR_ARG,
                "gme_seq_moving_masks: frames [%d, %d) outside [0, %d)", first, first + count, s->N);
    GME_REQUIRE(warps != nullptr || count == 0, GME_ERR_ARG, "gme_seq_moving_masks: null parameters");
    GME_REQUIRE(threshold >= 0 && threshold <= 255, GME_ERR_ARG, "gme_seq_moving_masks: threshold %d (0 .. 255)", threshold);
    GME_REQUIRE(min_count >= 1, GME_ERR_ARG, "gme_seq_moving_masks: min_count %d (at least 1)", min_count);
    GME_REQUIRE(s->passes->mosaic_valid, GME_ERR_ARG, "gme_seq_moving_masks: no mosaic was built (gme_seq_mosaic first)");
    if (count == 0) return GME_OK;
    int rc = mosaic_rows(s);
    if (rc) return rc;
    if (!s->passes->masks.ptr) {
        rc = plane_alloc(ctx, &s->passes->masks, s->N_cap, s->H, s->W);
        if (rc) { s->passes->masks_written.flag.clear(); return rc; }
        s->passes->masks_written.flag.assign((size_t)s->N_cap, 0);
    }
    rc = mosaic_put_rows(s, count, warps, usable);
    if (rc) return rc;
    unsigned long long* known = s->passes->mosaic_counts;
    unsigned long long* moving = s->passes->mosaic_counts + s->N_cap;
    GME_HIP_TRY(hipMemsetAsync(s->passes->mosaic_counts, 0, (size_t)s->N_cap * 2 * sizeof(unsigned long long), ctx->stream));
    rc = launch_moving_masks(ctx, s->level[2], s->passes->masks, first, count, s->passes->mosaic_params, s->passes->mosaic_usable, s->passes->mosaic_sprite,
                             s->passes->mosaic_count, s->passes->mosaic_pitch, s->passes->mosaic_Hc, s->passes->mosaic_Wc, ox, oy, threshold, min_count, known,
                             moving);
    if (rc) return rc;
    if (known_out)
        GME_HIP_TRY(hipMemcpyAsync(known_out, known, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (moving_out)
        GME_HIP_TRY(hipMemcpyAsync(moving_out, moving, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->passes->masks_written.mark(first, count);
    return GME_OK;
}

extern "C" int gme_seq_read_masks_range(gme_seq* s, int first, int count, uint8_t* out)
{
    GME_REQUIRE(s != nullptr && out != nullptr, GME_ERR_ARG, "gme_seq_read_masks_range: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(first >= 0 && count >= 0 && first + count <= s->N, GME_ERR_ARG,
                "gme_seq_read_masks_range: frames [%d, %d) outside [0, %d)", first, first + count, s->N);
    GME_REQUIRE(s->passes->masks_written.all(first, count), GME_ERR_ARG, "gme_seq_read_masks_range: the masks of frames [%d, %d) were never computed", first,
                first + count);
    const int rc = read_planes(s->ctx, s->passes->masks, first, count, out);
    return rc ? rc : ctx_finish(s->ctx);
}
