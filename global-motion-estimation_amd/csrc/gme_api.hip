// C ABI of libgme_hip.so (include/gme_hip.h), the core: contexts, the resident sequence with its block search, the staged
// global-motion estimate and the compensation, host<->device plumbing around the kernels in bbme_kernels.hip and its search
// kernels, gme_kernels.hip and synth_kernels.hip.  The passes built on this core have their entry points in
// gme_api_passes.hip and gme_api_frames.hip and their declarations and state in gme_passes.h: a new pass goes there.
#include <stdarg.h>
#include <string.h>

#include <mutex>
#include <new>
#include <vector>

#include "gme_internal.h"

static thread_local char g_err[512] = "";

void gme_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* gme_last_error(void) { return g_err; }

// first chunk of a block-matching call names the plan, later chunks only add their patches
void plan_note(gme_ctx* ctx, long long patches, const char* fmt, ...)
{
    ctx->plan_patches += patches;
    if (ctx->plan[0]) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->plan, sizeof(ctx->plan), fmt, ap);
    va_end(ap);
}

extern "C" int gme_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { gme_set_error("hipGetDeviceCount failed (no HIP device?)"); return 0; }
    return n;
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" gme_ctx* gme_create(int device_id)
{
    int n = gme_device_count();
    if (device_id < 0 || device_id >= n) {
        gme_set_error("gme_create: device %d not available (%d HIP devices visible)", device_id, n);
        return nullptr;
    }
    gme_ctx* ctx = new (std::nothrow) gme_ctx();
    if (!ctx) return nullptr;
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&ctx->prop, device_id) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        ctx->status.ensure(GME_STATUS_WORDS, "status words") != GME_OK ||
        hipMemsetAsync(ctx->status, 0, GME_STATUS_WORDS * sizeof(int), ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        gme_set_error("gme_create: HIP initialisation failed on device %d: %s", device_id,
                      hipGetErrorString(hipGetLastError()));
    else if (strncmp(ctx->prop.gcnArchName, "gfx950", 6) != 0)
        gme_set_error("gme_create: device %d is %s; this library carries gfx950 code only", device_id,
                      ctx->prop.gcnArchName);
    else
        return ctx;
    if (ctx->ev0) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) hipEventDestroy(ctx->ev1);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return nullptr;
}

extern "C" void gme_destroy(gme_ctx* ctx)
{
    if (!ctx) return;
    { std::lock_guard<std::mutex> lock(ctx->mu); }        // let a call in flight on another thread finish
    gme_comm_destroy(ctx);
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
    if (ctx->back_stream) hipStreamDestroy(ctx->back_stream);
    hipEventDestroy(ctx->ev0);
    hipEventDestroy(ctx->ev1);
    hipStreamDestroy(ctx->stream);
    delete ctx;                                            // frees the context's device buffers
}

// wait for the stream and report a tripped in-kernel guard
int ctx_finish(gme_ctx* ctx)
{
    int st = 0;
    GME_HIP_TRY(hipMemcpyAsync(&st, ctx->status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GME_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (st != 0) {
        hipMemsetAsync(ctx->status, 0, sizeof(int), ctx->stream);
        gme_set_error("a search walk exceeded its iteration guard (internal error)");
        return GME_ERR_STATE;
    }
    return GME_OK;
}

// Small results and arguments of the split-phase calls (parameters, sums, squared errors: a few dozen KB) do not go
// through hipMemcpyAsync when the caller's buffer is page-locked: the copy engines serve copies in order, and a 60 KB result
// queued behind another context's 177 MB upload arrived 3.4 ms late -- every stage of a streamed estimate waited for
// whatever chunk was crossing the link (round 3 timeline).  Page-locked memory (gme_host_alloc /
// hipHostMalloc) is mapped into the device's address space, so a kernel on the context's own stream moves the words
// itself.  Ordinary memory falls back to hipMemcpyAsync.
__global__ void __launch_bounds__(256) k_copy_words(const uint32_t* src, uint32_t* dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

static bool mapped_host_view(const void* host, void** dev)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return false; }      // ordinary memory: not an error
    if (at.type != hipMemoryTypeHost || at.devicePointer == nullptr) return false;
    *dev = at.devicePointer;
    return true;
}

// dst <- src of `bytes` (a multiple of 4) on the context's stream; exactly one of the two is host memory
static int copy_small(gme_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, bool prefer_kernel)
{
    if (bytes == 0) return GME_OK;
    void* view = nullptr;
    if (prefer_kernel && bytes % 4 == 0 && bytes <= ((size_t)16 << 20) && mapped_host_view(kind == hipMemcpyDeviceToHost ? dst : src, &view)) {
        const uint32_t* s4 = (const uint32_t*)(kind == hipMemcpyDeviceToHost ? src : view);
        uint32_t* d4 = (uint32_t*)(kind == hipMemcpyDeviceToHost ? view : dst);
        const size_t n = bytes / 4;
        const unsigned grid = (unsigned)((n + 255) / 256 < 256 ? (n + 255) / 256 : 256);
        hipLaunchKernelGGL(k_copy_words, dim3(grid), dim3(256), 0, ctx->stream, s4, d4, n);
        GME_HIP_TRY(hipGetLastError());
        return GME_OK;
    }
    GME_HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
    return GME_OK;
}

extern "C" int gme_sync(gme_ctx* ctx)
{
    GME_ENTER(ctx);
    return ctx_finish(ctx);
}

// statistics of the last block-matching call, summed over the XCDs: surviving patches, tiles redone, patches listed
static int read_bbme_stats(gme_ctx* ctx, int64_t (&sum)[3])
{
    uint32_t st[8 * 16];
    GME_HIP_TRY(hipMemcpyAsync(st, ctx->status + GME_STATUS_STATS, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    GME_HIP_TRY(hipStreamSynchronize(ctx->stream));
    sum[0] = sum[1] = sum[2] = 0;
    for (int x = 0; x < 8; ++x)
        for (int k = 0; k < 3; ++k) sum[k] += st[16 * x + k];
    return GME_OK;
}

extern "C" int gme_last_bbme_info(gme_ctx* ctx, char* plan, int plan_len, int64_t* patches, int64_t* surviving,
                                  int64_t* redo_tiles)
{
    GME_ENTER(ctx);
    if (plan && plan_len > 0) snprintf(plan, plan_len, "%s", ctx->plan);
    if (patches) *patches = ctx->plan_patches;
    if (surviving || redo_tiles) {
        int64_t sum[3];
        const int rc = read_bbme_stats(ctx, sum);
        if (rc) return rc;
        if (surviving) *surviving = sum[0];
        if (redo_tiles) *redo_tiles = sum[1];
    }
    return GME_OK;
}

extern "C" int gme_last_bbme_listed(gme_ctx* ctx, int64_t* listed)
{
    GME_ENTER(ctx);
    int64_t sum[3];
    const int rc = read_bbme_stats(ctx, sum);
    if (rc == GME_OK && listed) *listed = sum[2];
    return rc;
}

extern "C" void* gme_stream(gme_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" int gme_device_info(gme_ctx* ctx, char* name, int name_len, int* cu_count, int* clock_khz)
{
    GME_REQUIRE(ctx != nullptr, GME_ERR_ARG, "null context");
    if (name && name_len > 0) snprintf(name, name_len, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
    if (cu_count) *cu_count = ctx->prop.multiProcessorCount;
    if (clock_khz) *clock_khz = ctx->prop.clockRate;
    return GME_OK;
}

extern "C" int gme_device_bus_id(gme_ctx* ctx, char* out, int out_len)
{
    GME_ENTER(ctx);
    GME_REQUIRE(out != nullptr && out_len >= 16, GME_ERR_ARG, "gme_device_bus_id: buffer of at least 16 bytes");
    GME_HIP_TRY(hipDeviceGetPCIBusId(out, out_len, ctx->device));
    const hipError_t q = hipStreamQuery(ctx->stream);                  // the device still answers (work in flight is fine)
    GME_REQUIRE(q == hipSuccess || q == hipErrorNotReady, GME_ERR_HIP, "gme_device_bus_id: %s", hipGetErrorString(q));
    return GME_OK;
}

extern "C" int gme_timer_start(gme_ctx* ctx)
{
    GME_ENTER(ctx);
    GME_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    return GME_OK;
}

extern "C" int gme_timer_stop(gme_ctx* ctx, float* elapsed_ms)
{
    GME_ENTER(ctx);
    GME_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    GME_HIP_TRY(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    GME_HIP_TRY(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (elapsed_ms) *elapsed_ms = ms;
    return GME_OK;
}

int ctx_scratch(gme_ctx* ctx, size_t bytes, void** out)
{
    if (bytes > ctx->scratch.cap) {
        GME_HIP_TRY(hipStreamSynchronize(ctx->stream));        // work in flight may still read the old block
        const int rc = ctx->scratch.ensure((bytes + (1u << 20)) & ~((size_t)(1u << 20) - 1), "scratch");
        if (rc) return rc;
    }
    *out = ctx->scratch.get();
    return GME_OK;
}

int ctx_redo_list(gme_ctx* ctx, size_t entries, uint32_t** out)
{
    if (entries > ctx->redo_list.cap) {
        GME_HIP_TRY(hipStreamSynchronize(ctx->stream));
        const int rc = ctx->redo_list.ensure((entries + 4095) & ~(size_t)4095, "redo entries");
        if (rc) return rc;
    }
    *out = ctx->redo_list.get();
    return GME_OK;
}

int plane_alloc(gme_ctx* ctx, PlaneBuf* p, int count, int H, int W)
{
    *p = PlaneBuf();
    Plane v = plane_shape(H, W, count);
    if (count != 0 && H != 0 && W != 0) {
        // one guard row behind the stack: dword loads near the last row never leave the allocation
        const int rc = p->mem.ensure(v.bytes() + v.pitch, "frames");
        if (rc) return rc;
        v.ptr = p->mem.get();
        // on the context's stream: a null-stream memset would not be ordered against the
        // kernels this (non-blocking) stream runs next and could land on top of their output
        const hipError_t e = hipMemsetAsync(v.ptr, 0, v.bytes() + v.pitch, ctx->stream);
        if (e != hipSuccess) {
            p->mem.reset();
            gme_set_error("hipMemsetAsync of %zu bytes of frames failed: %s", v.bytes() + v.pitch, hipGetErrorString(e));
            return GME_ERR_HIP;
        }
    }
    static_cast<Plane&>(*p) = v;
    return GME_OK;
}

// The search of the pairs (first + k, first + k + fd), k < pairs, of a plane stack into mf.
BbmeJob bbme_job(const Plane& p, int first, int fd, int pairs, int bs, int sw, int procedure, int pnorm, int32_t* mf)
{
    BbmeJob job;
    job.prev = p.at(first); job.cur = p.at(first + fd); job.plane_stride = p.stride; job.pairs = pairs;
    job.H = p.H; job.W = p.W; job.pitch = p.pitch;
    job.bs = bs; job.sw = sw; job.procedure = procedure; job.pnorm = pnorm;
    job.mf = mf;
    return job;
}

// ---------------------------------------------------------------------------
// single-pair calls on host buffers
// ---------------------------------------------------------------------------
extern "C" int gme_bbme_u8(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int H, int W, int stride,
                           int block_size, int search_window, int procedure, int pnorm, int32_t* mf_out)
{
    GME_ENTER(ctx);
    GME_REQUIRE(prev && cur && mf_out, GME_ERR_ARG, "gme_bbme_u8: null pointer");
    GME_REQUIRE(H > 0 && W > 0 && stride >= W, GME_ERR_ARG, "gme_bbme_u8: bad shape H=%d W=%d stride=%d", H, W, stride);
    GME_REQUIRE(block_size >= 1, GME_ERR_ARG, "gme_bbme_u8: block_size %d", block_size);
    int rc = bbme_check_args(H, W, block_size, search_window, procedure, pnorm);
    if (rc) return rc;
    const int h = H / block_size, w = W / block_size;
    if (h == 0 || w == 0) return GME_OK;
    Plane pp = plane_shape(H, W, 1), pc = pp;
    int32_t* mf = nullptr;
    uint32_t* sq = nullptr;
    const int aux = bbme_aux_kind(H, W, pp.pitch, 1, block_size, search_window, procedure, pnorm);
    Carver c;
    c.take(&pp, true); c.take(&pc, true);
    c.take(&mf, (size_t)h * w * 2);
    c.take(&sq, aux != 0 ? (size_t)pp.stride : 0);
    rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(hipMemsetAsync(pp.ptr, 0, (uint8_t*)mf - pp.ptr, ctx->stream));
    GME_HIP_TRY(put_plane(ctx, pp, prev, stride));
    GME_HIP_TRY(put_plane(ctx, pc, cur, stride));
    Plane both = pp;                                           // the two carved planes as a stack
    both.stride = pc.ptr - pp.ptr; both.count = 2;
    auto job = bbme_job(both, 0, 1, 1, block_size, search_window, procedure, pnorm, mf);
    if (aux != 0) {
        rc = launch_aux_table(ctx, aux, pc.ptr, 0, 1, H, W, pc.pitch, sq, 0);
        if (rc) return rc;
        job.sqbox_cur = sq;
        job.sqbox_kind = aux;
    }
    rc = launch_bbme(ctx, job);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(mf_out, mf, (size_t)h * w * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

extern "C" int gme_pyrdown_u8(gme_ctx* ctx, const uint8_t* src, int H, int W, int stride, uint8_t* dst)
{
    GME_ENTER(ctx);
    GME_REQUIRE(src && dst && H > 0 && W > 0 && stride >= W, GME_ERR_ARG, "gme_pyrdown_u8: bad arguments");
    Plane s = plane_shape(H, W, 1), d = plane_shape((H + 1) / 2, (W + 1) / 2, 1);
    Carver c;
    c.take(&s, false); c.take(&d, false);
    int rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(put_plane(ctx, s, src, stride));
    rc = launch_pyrdown(ctx, s, d);
    if (rc) return rc;
    rc = read_planes(ctx, d, 0, 1, dst);
    return rc ? rc : ctx_finish(ctx);
}

// Model orders: 1 = affine (params [P][6], sums [P][15] = F (9) | Sx (3) | Sy (3)); 2 = the second-order models
// (params [P][12], sums [P][27], see the section at the end of this file).
static int order_params(int order) { return order == 1 ? 6 : 12; }
static int order_sums(int order) { return order == 1 ? 15 : 27; }

// the h x w field of one parameter vector of `order` through the scratch
static int model_field(gme_ctx* ctx, int order, const char* who, const double* params, int h, int w, int16_t* mf_out)
{
    GME_ENTER(ctx);
    GME_REQUIRE(params && mf_out && h >= 0 && w >= 0, GME_ERR_ARG, "%s: bad arguments", who);
    if (h == 0 || w == 0) return GME_OK;
    double* d_params = nullptr;
    int16_t* d_field = nullptr;
    const size_t np = (size_t)order_params(order), nf = (size_t)h * w * 2;
    Carver c;
    c.take(&d_params, np); c.take(&d_field, nf);
    int rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(d_params, params, np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = order == 1 ? launch_affine_field(ctx, d_params, 1, h, w, d_field) : launch_model2_field(ctx, d_params, 1, h, w, d_field, nullptr);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(mf_out, d_field, nf * sizeof(int16_t), hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

extern "C" int gme_affine_field(gme_ctx* ctx, const double params[6], int h, int w, int16_t* mf_out)
{
    return model_field(ctx, 1, "gme_affine_field", params, h, w, mf_out);
}

extern "C" int gme_compensate_u8(gme_ctx* ctx, const uint8_t* frame, int H, int W, int stride, const int32_t* mf,
                                 int h, int w, uint8_t* out)
{
    GME_ENTER(ctx);
    GME_REQUIRE(frame && mf && out && H > 0 && W > 0 && stride >= W, GME_ERR_ARG, "gme_compensate_u8: bad arguments");
    GME_REQUIRE(h > 0 && w > 0 && h <= H, GME_ERR_ARG,
                "gme_compensate_u8: field of %d x %d blocks on a %d-row frame (motion.py:303 divides H by it)", h, w, H);
    Plane pf = plane_shape(H, W, 1), po = pf;
    int32_t* d_mf = nullptr;
    Carver c;
    c.take(&pf, false); c.take(&po, false); c.take(&d_mf, (size_t)h * w * 2);
    int rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(put_plane(ctx, pf, frame, stride));
    GME_HIP_TRY(hipMemcpyAsync(d_mf, mf, (size_t)h * w * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_compensate(ctx, pf.ptr, 0, 1, H, W, pf.pitch, d_mf, nullptr, h, w, po.ptr, 0, po.pitch, nullptr, 0, nullptr);
    if (rc) return rc;
    rc = read_planes(ctx, po, 0, 1, out);
    return rc ? rc : ctx_finish(ctx);
}

extern "C" int gme_sse_u8(gme_ctx* ctx, const uint8_t* a, const uint8_t* b_, int H, int W, int stride_a, int stride_b,
                          int64_t* sse_out)
{
    GME_ENTER(ctx);
    GME_REQUIRE(a && b_ && sse_out && H > 0 && W > 0 && stride_a >= W && stride_b >= W, GME_ERR_ARG,
                "gme_sse_u8: bad arguments");
    Plane pa = plane_shape(H, W, 1), pb = pa;
    unsigned long long* d_sse = nullptr;
    Carver c;
    c.take(&pa, false); c.take(&pb, false); c.take(&d_sse, 1);
    int rc = c.commit(ctx);
    if (rc) return rc;
    GME_HIP_TRY(put_plane(ctx, pa, a, stride_a));
    GME_HIP_TRY(put_plane(ctx, pb, b_, stride_b));
    rc = launch_sse(ctx, pa.ptr, 0, pa.pitch, pb.ptr, 0, pb.pitch, 1, H, W, d_sse);
    if (rc) return rc;
    unsigned long long v = 0;
    GME_HIP_TRY(hipMemcpyAsync(&v, d_sse, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
    rc = ctx_finish(ctx);
    *sse_out = (int64_t)v;
    return rc;
}

// ---------------------------------------------------------------------------
// sequences
// ---------------------------------------------------------------------------
extern "C" gme_seq* gme_seq_create(gme_ctx* ctx, int n_frames, int H, int W)
{
    if (!ctx) { gme_set_error("null context"); return nullptr; }
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) { gme_set_error("hipSetDevice(%d) failed", ctx->device); return nullptr; }
    if (n_frames < 1 || H < 1 || W < 1) { gme_set_error("gme_seq_create: bad shape"); return nullptr; }
    gme_seq* s = new (std::nothrow) gme_seq();
    if (!s) return nullptr;
    s->ctx = ctx; s->N = s->N_cap = n_frames; s->H = H; s->W = W;
    if (plane_alloc(ctx, &s->level[2], n_frames, H, W) != GME_OK || !(s->passes = passes_create())) { delete s; return nullptr; }
    return s;
}

extern "C" void gme_seq_destroy(gme_seq* s)
{
    if (!s) return;
    std::lock_guard<std::mutex> lock(s->ctx->mu);
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    if (s->ready) hipEventDestroy(s->ready);
    if (s->upload_gate) hipEventDestroy(s->upload_gate);
    if (s->uploaded) hipEventDestroy(s->uploaded);
    passes_destroy(s->passes);                             // frees the device buffers of the passes ...
    delete s;                                              // ... and the sequence's own
}

// Split-phase calls: with the switch on, gme_seq_gme_begin / gme_seq_gme_fit / gme_seq_compensate queue their work
// (including the copy of their result into the caller's buffer, which should be page-locked: gme_host_alloc) and
// return; gme_seq_wait blocks until the result of the LAST such call has arrived -- not until the stream is idle, so
// the searches queued behind the copy keep running, and one host thread can drive several sequences on several
// streams, solving one's 3x3 systems while the others' kernels run.
extern "C" int gme_seq_set_split_phase(gme_seq* s, int on)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    GME_ENTER(s->ctx);
    // release-to-system: the results behind this event are written by a kernel into host memory the CALLER chose; whatever
    // its coherence (hipHostMallocNonCoherent, hipHostRegister'ed, HIP_HOST_COHERENT=0), they are visible once it fires
    if (on && !s->ready) GME_HIP_TRY(hipEventCreateWithFlags(&s->ready, hipEventDisableTiming | hipEventReleaseToSystem));
    s->split_phase = on != 0;
    return GME_OK;
}

extern "C" int gme_seq_wait(gme_seq* s)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    GME_ENTER(s->ctx);
    GME_REQUIRE(s->ready != nullptr, GME_ERR_STATE, "gme_seq_wait without gme_seq_set_split_phase");
    GME_HIP_TRY(hipEventSynchronize(s->ready));
    return GME_OK;
}

// 1 when the result of the last split-phase call has arrived (gme_seq_wait would return at once), 0 when it is still
// on its way: lets one host thread serve whichever of several sequences is ready first instead of blocking on one.
extern "C" int gme_seq_poll(gme_seq* s)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    GME_ENTER(s->ctx);
    GME_REQUIRE(s->ready != nullptr, GME_ERR_STATE, "gme_seq_poll without gme_seq_set_split_phase");
    const hipError_t e = hipEventQuery(s->ready);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
    gme_set_error("hipEventQuery failed: %s", hipGetErrorString(e));
    return GME_ERR_HIP;
}

// the ending of a call that hands results to the caller: split-phase records s->ready behind their copies, otherwise it waits
static int seq_deliver(gme_seq* s)
{
    if (!s->split_phase) return ctx_finish(s->ctx);
    GME_HIP_TRY(hipEventRecord(s->ready, s->ctx->stream));
    return GME_OK;
}

// new frame data ends a staged GME run: searches gme_seq_gme_begin deferred must not see other frames
// than the stages already done, so the run is dropped (gme_seq_gme_fit then asks for a new begin)
static void gme_drop_run(gme_seq* s)
{
    s->bbme_pending[0] = s->bbme_pending[1] = s->bbme_pending[2] = false;
    s->gme_pairs = 0;
}

// Replacing the motion field ends what was derived from it.  Every writer of s->mv comes through here, and so do new frames;
// the core keeps no such result, the passes' are ended by passes_field_replaced (gme_api_passes.hip names them).
void seq_field_replaced(gme_seq* s)
{
    passes_field_replaced(s->passes);
}

// the frames changed: pyramids and auxiliary tables are stale, a staged run ends, and so does every result that was measured
// on the old frames (the motion field stays: it is a prior; the compensated and warped frames, mosaic and masks stay too)
static void seq_frames_changed(gme_seq* s)
{
    s->pyramids_valid = false;
    s->sqbox_valid[0] = s->sqbox_valid[1] = s->sqbox_valid[2] = false;
    gme_drop_run(s);
    passes_frames_changed(s->passes);                      // ... which ends what seq_field_replaced ends, too
}

// The sequence acts as one of `n_frames` frames (1 <= n_frames <= the count it was created with) from now on: every
// stage call covers the pairs of frames [0, n_frames) only.  Buffers stay sized for the full count, so a caller that
// streams chunks of different lengths through one sequence (sequence.StreamEstimator) pays for the pairs it has, not for
// the capacity, and nothing is reallocated.  Ends a staged GME run like new frame data does.
extern "C" int gme_seq_set_frames(gme_seq* s, int n_frames)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    GME_ENTER(s->ctx);
    GME_REQUIRE(n_frames >= 1 && n_frames <= s->N_cap, GME_ERR_ARG, "gme_seq_set_frames: %d frames in a sequence created for %d", n_frames, s->N_cap);
    if (n_frames != s->N) {
        s->N = n_frames;
        seq_frames_changed(s);
    }
    return GME_OK;
}

// One upload lane per device for the split-phase uploads of ALL contexts: host-to-device copies issued from several
// streams at once share the link badly (two concurrent copy streams moved 22-25 GB/s where one moves 38-54, DESIGN.md
// section 5; three lanes uploading on their own streams reached 62 % of the copy-alone rate, one shared lane does the
// rest), so they queue on ONE stream in call order; events tie each copy to its sequence's own stream.
namespace {
struct Uploader {
    std::mutex mu;
    hipStream_t stream = nullptr;
    // Device staging of tight host frames, repacked into the pitched planes.  The one device block no DevBuf owns: the
    // array below lives as long as the process, and a destructor there would call hipFree after the HIP runtime has
    // shut down.  So the pointer is raw, and the last block is never freed.
    uint8_t* stage = nullptr;
    size_t stage_bytes = 0;
};
Uploader g_uploader[16];
}  // namespace

// tight host frames (the usual NumPy stack) whose rows are narrower than the plane pitch: linear copy + repack
static bool host_frames_tight(const gme_seq* s, int row_stride, int64_t frame_stride)
{
    return row_stride == s->W && frame_stride == (int64_t)s->W * s->H && s->level[2].pitch != s->W;
}

// Frames per linear copy when gme_seq_upload goes through a staging buffer (0: it does not).  Tight frames: linear copies
// (what the DMA engines move at link speed; 2-D copies of 720-byte rows reach ~37 GB/s) through a device staging buffer,
// spread into the pitched planes by k_repack.
static size_t upload_stage_frames(const gme_seq* s, int count, int row_stride, int64_t frame_stride)
{
    if (!host_frames_tight(s, row_stride, frame_stride) || count <= 0) return 0;
    size_t per = ((size_t)64 << 20) / ((size_t)s->H * s->W);
    if (per < 1) per = 1;
    return per > (size_t)count ? (size_t)count : per;
}

// The copies of host frames into planes first .. first + count - 1 on `stream`, the one place that knows the three host
// layouts; `stage` holds `per` frames (0: the frames are not tight) and belongs to that stream.
static int upload_copies(gme_seq* s, hipStream_t stream, uint8_t* stage, size_t per, int first, int count,
                         const uint8_t* frames, int row_stride, int64_t frame_stride)
{
    const Plane& p = s->level[2];
    gme_ctx* ctx = s->ctx;
    if (per > 0) {
        // one linear copy (link speed), then spread into the pitched planes on the same stream: the next copy into the
        // staging buffer is ordered behind this repack.  Measured against the two alternatives: the repack kernel
        // reading page-locked frames across the link itself (34 against 40 GB/s) and the frames split over two copy
        // engines (22-25 against 38-39 GB/s) were both slower.
        const size_t frame_bytes = (size_t)s->H * s->W;
        for (int f0 = 0; f0 < count; f0 += (int)per) {
            const int n = count - f0 < (int)per ? count - f0 : (int)per;
            GME_HIP_TRY(hipMemcpyAsync(stage, frames + (int64_t)f0 * frame_stride, (size_t)n * frame_bytes, hipMemcpyHostToDevice, stream));
            int rc2 = launch_repack(ctx, stream, stage, n, s->H, s->W, p.at(first + f0), p.pitch, p.stride);
            if (rc2) return rc2;
        }
    } else if (p.stride == (int64_t)p.pitch * s->H && frame_stride == (int64_t)row_stride * s->H) {
        // planes and host frames are both back to back: one 2-D copy of count*H rows
        GME_HIP_TRY(hipMemcpy2DAsync(p.at(first), p.pitch, frames, row_stride, s->W, (size_t)s->H * count,
                                     hipMemcpyHostToDevice, stream));
    } else {
        for (int i = 0; i < count; ++i)
            GME_HIP_TRY(hipMemcpy2DAsync(p.at(first + i), p.pitch, frames + (int64_t)i * frame_stride, row_stride, s->W,
                                         s->H, hipMemcpyHostToDevice, stream));
    }
    return GME_OK;
}

extern "C" int gme_seq_upload(gme_seq* s, int first, int count, const uint8_t* frames, int row_stride,
                              int64_t frame_stride)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    GME_ENTER(s->ctx);
    GME_REQUIRE(frames && first >= 0 && count >= 0 && first + count <= s->N_cap && row_stride >= s->W, GME_ERR_ARG,
                "gme_seq_upload: frames [%d, %d) outside the sequence of %d", first, first + count, s->N_cap);
    gme_ctx* ctx = s->ctx;
    seq_frames_changed(s);
    const size_t per = upload_stage_frames(s, count, row_stride, frame_stride), stage_bytes = per * s->H * s->W;
    if (s->split_phase && ctx->device >= 0 && ctx->device < 16) {
        // split-phase: the copies are queued and the call returns; `frames` must stay untouched until a later
        // gme_seq_wait / gme_sync on this sequence has returned.  They run on the device's shared upload stream, behind
        // whatever of this context still reads the planes (gate) and in front of whatever it queues next (s->uploaded);
        // with page-locked frames (gme_host_alloc) the host thread is free at once and every context's kernels run beside the copy.
        Uploader& u = g_uploader[ctx->device];
        std::lock_guard<std::mutex> ulock(u.mu);
        if (!u.stream) GME_HIP_TRY(hipStreamCreateWithFlags(&u.stream, hipStreamNonBlocking));
        if (!s->upload_gate) {
            GME_HIP_TRY(hipEventCreateWithFlags(&s->upload_gate, hipEventDisableTiming));
            GME_HIP_TRY(hipEventCreateWithFlags(&s->uploaded, hipEventDisableTiming));
        }
        GME_HIP_TRY(hipEventRecord(s->upload_gate, ctx->stream));
        GME_HIP_TRY(hipStreamWaitEvent(u.stream, s->upload_gate, 0));
        if (stage_bytes > u.stage_bytes) {
            GME_HIP_TRY(hipStreamSynchronize(u.stream));
            if (u.stage) (void)hipFree(u.stage);               // see Uploader::stage
            u.stage = nullptr; u.stage_bytes = 0;
            if (hipMalloc((void**)&u.stage, stage_bytes) != hipSuccess) { gme_set_error("out of device memory (staging)"); return GME_ERR_NOMEM; }
            u.stage_bytes = stage_bytes;
        }
        int rc = upload_copies(s, u.stream, u.stage, per, first, count, frames, row_stride, frame_stride);
        if (rc) return rc;
        GME_HIP_TRY(hipEventRecord(s->uploaded, u.stream));
        GME_HIP_TRY(hipStreamWaitEvent(ctx->stream, s->uploaded, 0));
        GME_HIP_TRY(hipEventRecord(s->ready, ctx->stream));
        return GME_OK;
    }
    if (stage_bytes > ctx->stage.cap) {
        GME_HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->copy_stream) GME_HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
        const int rc = ctx->stage.ensure(stage_bytes, "staging");
        if (rc) return rc;
    }
    int rc = upload_copies(s, ctx->stream, ctx->stage, per, first, count, frames, row_stride, frame_stride);
    if (rc) return rc;
    GME_HIP_TRY(hipStreamSynchronize(ctx->stream));      // the host buffer may be reused on return
    return GME_OK;
}

extern "C" int gme_seq_synth(gme_seq* s, uint64_t seed, int t0)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    GME_ENTER(s->ctx);
    int rc = GME_OK;
    if (!s->synth_canvas) {
        rc = s->synth_canvas.ensure((size_t)2048 * 4096, "synthetic canvas");
        if (rc) return rc;
        s->synth_valid = false;
    }
    if (!s->synth_valid || s->synth_seed != seed) {
        rc = launch_synth_canvas(s->ctx, seed, s->synth_canvas);
        if (rc) return rc;
        s->synth_seed = seed; s->synth_valid = true;
    }
    seq_frames_changed(s);
    return launch_synth_frames(s->ctx, seed, t0, s->synth_canvas, s->level[2]);
}

extern "C" int gme_seq_invalidate(gme_seq* s)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    seq_frames_changed(s);
    return GME_OK;
}

extern "C" int gme_seq_read_frame(gme_seq* s, int level, int index, uint8_t* out)
{
    GME_REQUIRE(s != nullptr && out != nullptr, GME_ERR_ARG, "gme_seq_read_frame: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(level >= 0 && level <= 2 && index >= 0 && index < s->N_cap, GME_ERR_ARG, "gme_seq_read_frame: bad index");
    GME_REQUIRE(level == 2 || s->pyramids_valid, GME_ERR_STATE, "pyramid levels exist only after gme_seq_gme_begin");
    const int rc = read_planes(s->ctx, s->level[level], index, 1, out);
    return rc ? rc : ctx_finish(s->ctx);
}

// auxiliary table (bbme_aux_kind) for every frame of one pyramid level
static int seq_sqbox(gme_seq* s, int level, int kind)
{
    const Plane& p = s->level[level];
    int rc = s->sqbox[level].ensure((size_t)p.stride * p.count, "box sums");
    if (rc) return rc;
    if (!s->sqbox_valid[level] || s->sqbox_kind[level] != kind) {
        rc = launch_aux_table(s->ctx, kind, p.ptr, p.stride, s->N, p.H, p.W, p.pitch, s->sqbox[level], p.stride);
        if (rc) return rc;
        s->sqbox_valid[level] = true;
        s->sqbox_kind[level] = kind;
    }
    return GME_OK;
}

// launch_bbme of a job over the resident frames of one level whose first "current" plane is frame first_cur of the level,
// with the auxiliary table its kernel wants (one table per frame, so the job's tables start at that frame's)
int seq_launch_bbme_from(gme_seq* s, int level, int first_cur, BbmeJob job)
{
    if (const int aux = bbme_aux_kind(job.H, job.W, job.pitch, job.pairs, job.bs, job.sw, job.procedure, job.pnorm)) {      // BASELINE config 4
        const int rc = seq_sqbox(s, level, aux);
        if (rc) return rc;
        const Plane& p = s->level[level];
        job.sqbox_cur = s->sqbox[level] + (size_t)first_cur * p.stride; job.sqbox_stride = p.stride; job.sqbox_kind = aux;
    }
    return launch_bbme(s->ctx, job);
}

// ... of the pairs (k, k + fd): the first pair is pair 0
static int seq_launch_bbme(gme_seq* s, int level, int fd, BbmeJob job)
{
    return seq_launch_bbme_from(s, level, fd, job);
}

extern "C" int gme_seq_bbme(gme_seq* s, int fd, int bs, int sw, int procedure, int pnorm)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    GME_ENTER(s->ctx);
    int rc = GME_OK;
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    rc = bbme_check_args(s->H, s->W, bs, sw, procedure, pnorm);
    if (rc) return rc;
    const int pairs = s->N - fd, h = s->H / bs, w = s->W / bs;
    rc = s->mv.ensure((size_t)pairs * h * w * 2, "motion field");
    if (rc) return rc;
    s->mv_h = h; s->mv_w = w; s->mv_pairs = pairs;
    s->mv_fd = fd; s->mv_bs = bs;
    seq_field_replaced(s);
    return seq_launch_bbme(s, 2, fd, bbme_job(s->level[2], 0, fd, pairs, bs, sw, procedure, pnorm, s->mv));
}

// ---------------------------------------------------------------------------
// host frames -> fields with the upload overlapped (results.py:41-50 hands over host arrays)
// ---------------------------------------------------------------------------
extern "C" void* gme_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        gme_set_error("gme_host_alloc: cannot pin %zu bytes", bytes);
        return nullptr;
    }
    return p;
}

extern "C" void gme_host_free(void* p)
{
    if (p) hipHostFree(p);
}

// The events of one call, owned as DevBuf owns memory: add() creates them when the call asks, the destructor destroys them.
struct EventSet {
    std::vector<hipEvent_t> ev;
    EventSet() = default;
    EventSet(const EventSet&) = delete;
    EventSet& operator=(const EventSet&) = delete;
    ~EventSet() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    int add(size_t n)
    {
        for (; n > 0; --n) {
            hipEvent_t e = nullptr;
            GME_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ev.push_back(e);
        }
        return GME_OK;
    }
};

extern "C" int gme_seq_bbme_streamed(gme_seq* s, const uint8_t* frames, int row_stride, int64_t frame_stride, int count,
                                     int fd, int bs, int sw, int procedure, int pnorm, int chunk_frames, int32_t* mf_out)
{
    GME_REQUIRE(s != nullptr && frames != nullptr && mf_out != nullptr, GME_ERR_ARG, "gme_seq_bbme_streamed: null pointer");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(count >= 1 && count <= s->N && row_stride >= s->W, GME_ERR_ARG,
                "gme_seq_bbme_streamed: %d frames into a sequence of %d", count, s->N);
    GME_REQUIRE(fd >= 1 && fd < count, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    GME_REQUIRE(bs >= 1 && chunk_frames >= 1, GME_ERR_ARG, "block_size %d, chunk of %d frames", bs, chunk_frames);
    int rc = bbme_check_args(s->H, s->W, bs, sw, procedure, pnorm);
    if (rc) return rc;
    const int pairs = count - fd, h = s->H / bs, w = s->W / bs;
    const size_t per = (size_t)h * w * 2;
    rc = s->mv.ensure((size_t)(s->N - fd) * per, "motion field");
    if (rc) return rc;
    s->mv_h = h; s->mv_w = w; s->mv_pairs = pairs;
    s->mv_fd = fd; s->mv_bs = bs;
    seq_field_replaced(s);
    const Plane& p = s->level[2];
    // one table kind for the whole call: every chunk's launches carry at most `pairs` pairs, so one that the matrix-core
    // kernel would take at the largest also takes it at every chunk, and a smaller chunk of a declined call keeps kind 1
    const int aux = bbme_aux_kind(s->H, s->W, p.pitch, pairs, bs, sw, procedure, pnorm);
    if (aux) {
        rc = s->sqbox[2].ensure((size_t)p.stride * p.count, "box sums");
        if (rc) return rc;
    }
    if (!ctx->copy_stream) {
        GME_HIP_TRY(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        GME_HIP_TRY(hipStreamCreateWithFlags(&ctx->back_stream, hipStreamNonBlocking));
    }
    seq_frames_changed(s);
    // tight frames go through the staging buffer a chunk at a time: a chunk is one linear copy plus one repack
    const size_t stage_frames = host_frames_tight(s, row_stride, frame_stride) ? (size_t)(chunk_frames < count ? chunk_frames : count) : 0;
    if (stage_frames * s->H * s->W > ctx->stage.cap) {
        GME_HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
        rc = ctx->stage.ensure(stage_frames * s->H * s->W, "staging");
        if (rc) return rc;
    }
    const int nchunks = (count + chunk_frames - 1) / chunk_frames;
    EventSet events;                                           // per chunk: uploaded, searched; and the gate
    rc = events.add(2 * (size_t)nchunks + 1);
    if (rc) return rc;
    const hipEvent_t *up = events.ev.data(), *done = up + nchunks, gate = up[2 * nchunks];
    int tab_done = 0;                                          // frames whose auxiliary table rows exist (always from frame 0:
                                                               // a later call with a smaller frame distance reads them as `cur`)
    // everything the call queues; a failure leaves through the one error exit below
    auto queue_all = [&]() -> int {
        // earlier work of this context may still read or write the planes / the field buffer
        GME_HIP_TRY(hipEventRecord(gate, ctx->stream));
        GME_HIP_TRY(hipStreamWaitEvent(ctx->copy_stream, gate, 0));
        GME_HIP_TRY(hipStreamWaitEvent(ctx->back_stream, gate, 0));
        // upload of chunk c on the copy stream + the event behind it: it runs while the compute stream still searches chunk c - 1
        auto upload_chunk = [&](int c) -> int {
            const int f0 = c * chunk_frames, f1 = f0 + chunk_frames < count ? f0 + chunk_frames : count;
            const int r = upload_copies(s, ctx->copy_stream, ctx->stage, stage_frames, f0, f1 - f0, frames + (int64_t)f0 * frame_stride,
                                        row_stride, frame_stride);
            if (r) return r;
            GME_HIP_TRY(hipEventRecord(up[c], ctx->copy_stream));
            return GME_OK;
        };
        int p_done = 0;                                        // pairs searched so far
        int back_first = 0, back_count = 0, back_chunk = -1;   // fields of the previous chunk, still to be read back
        auto read_back = [&]() -> int {
            if (back_count == 0) return GME_OK;
            GME_HIP_TRY(hipStreamWaitEvent(ctx->back_stream, done[back_chunk], 0));
            const int first = back_first, n = back_count;
            back_count = 0;
            GME_HIP_TRY(hipMemcpyAsync(mf_out + per * first, s->mv + per * first, per * n * sizeof(int32_t), hipMemcpyDeviceToHost,
                                       ctx->back_stream));
            return GME_OK;
        };
        rc = upload_chunk(0);
        if (rc) return rc;
        for (int c = 0; c < nchunks; ++c) {
            const int f1 = (c + 1) * chunk_frames < count ? (c + 1) * chunk_frames : count;
            // The NEXT chunk's upload is queued before this chunk's search is launched: a kernel launch behind a cross-stream
            // wait on a copy holds the calling thread until that copy is done, and with the upload queued only afterwards the
            // link idled for the host's latency between chunks (94 % of the copy-alone rate; round 3).
            if (c + 1 < nchunks) {
                rc = upload_chunk(c + 1);
                if (rc) return rc;
            }
            // read-back of the previous chunk's fields only now, behind the next chunk's upload in program order: a copy
            // into pageable memory may hold the calling thread until that chunk's kernel is done, and the upload
            // queued above keeps the link busy meanwhile
            rc = read_back();
            if (rc) return rc;
            GME_HIP_TRY(hipStreamWaitEvent(ctx->stream, up[c], 0));
            const int p1 = f1 - fd;                            // pairs [p_done, p1) have both frames on the device now
            if (p1 > p_done) {
                auto job = bbme_job(p, p_done, fd, p1 - p_done, bs, sw, procedure, pnorm, s->mv + per * p_done);
                job.chained = p_done > 0;
                if (aux) {
                    // box sums of squares of every frame uploaded since the last table launch
                    const int t0 = tab_done;
                    tab_done = f1;
                    rc = launch_aux_table(ctx, aux, p.at(t0), p.stride, f1 - t0, p.H, p.W, p.pitch, s->sqbox[2] + (size_t)t0 * p.stride, p.stride);
                    if (rc) return rc;
                    job.sqbox_cur = s->sqbox[2] + (size_t)(p_done + fd) * p.stride; job.sqbox_stride = p.stride; job.sqbox_kind = aux;
                }
                rc = launch_bbme(ctx, job);
                if (rc) return rc;
                GME_HIP_TRY(hipEventRecord(done[c], ctx->stream));
                back_first = p_done; back_count = p1 - p_done; back_chunk = c;
                p_done = p1;
            }
        }
        return read_back();
    };
    rc = queue_all();
    const hipError_t e1 = hipStreamSynchronize(ctx->copy_stream), e2 = hipStreamSynchronize(ctx->back_stream);
    if (rc) {                                                  // the error exit: nothing of the call still runs when its events go
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    rc = ctx_finish(ctx);
    if (aux) { s->sqbox_valid[2] = (count == s->N && tab_done == count); s->sqbox_kind[2] = aux; }
    if (e1 != hipSuccess || e2 != hipSuccess) { gme_set_error("gme_seq_bbme_streamed: copy stream failed"); return GME_ERR_HIP; }
    return rc;
}

extern "C" int gme_seq_read_mv(gme_seq* s, int first_pair, int count, int32_t* mf_out)
{
    GME_REQUIRE(s != nullptr && mf_out != nullptr, GME_ERR_ARG, "gme_seq_read_mv: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(s->mv != nullptr, GME_ERR_STATE, "gme_seq_read_mv before gme_seq_bbme");
    GME_REQUIRE(first_pair >= 0 && count >= 0 && first_pair + count <= s->mv_pairs, GME_ERR_ARG,
                "gme_seq_read_mv: pairs [%d, %d) outside [0, %d)", first_pair, first_pair + count, s->mv_pairs);
    const size_t per = (size_t)s->mv_h * s->mv_w * 2;
    GME_HIP_TRY(hipMemcpyAsync(mf_out, s->mv + per * first_pair, per * count * sizeof(int32_t), hipMemcpyDeviceToHost,
                               s->ctx->stream));
    return ctx_finish(s->ctx);
}

// Buffers of one level for `pairs` fields of h x w, all or none.  gt: the level's own field, or (borrowed_gt) one the fit
// only reads, which is then never allocated or freed here.  full: also the stage buffers of the fit (model field, mask,
// sums, ...); the dense level needs gt only.
static int alloc_fit(FitLevelBuf& f, int pairs, int h, int w, bool full, int32_t* borrowed_gt = nullptr)
{
    f = FitLevelBuf();                                     // sized for this shape, not for the largest so far
    const size_t n = (size_t)pairs * h * w, nf = full ? n : 0, pf = nf ? (size_t)pairs : 0;
    const int rc = dev_ensure_all("GME level buffers",
                                  { { f.gt_own, borrowed_gt ? 0 : n * 2 }, { f.model, nf * 2 }, { f.mask, nf }, { f.diff, nf },
                                    { f.list, (size_t)h * w * 16 > FIT_LIST_LDS_BYTES ? nf : 0 }, { f.thr, pf }, { f.sums, pf * 15 },
                                    { f.sums2, pf * 27 } });
    if (rc) return rc;
    f.h = h; f.w = w;
    f.gt = borrowed_gt ? borrowed_gt : f.gt_own.get();
    return GME_OK;
}

// BBME of one pyramid level for the pairs of the current GME run (gme_seq_gme_begin's arguments):
// level 0 = dense field (bs 2, diamond, MSE: motion.py:27-29; bbme.py:18 default norm).
static int gme_level_bbme(gme_seq* s, int l)
{
    if (!s->bbme_pending[l]) return GME_OK;
    s->bbme_pending[l] = false;
    const Plane& p = s->level[l];
    if (s->fit[l].h == 0 || s->fit[l].w == 0) return GME_OK;
    const int fd = s->gme_fd, pairs = s->gme_pairs;
    if (l == 0) return seq_launch_bbme(s, l, fd, bbme_job(p, 0, fd, pairs, 2, 2, GME_SEARCH_DIAMOND, GME_NORM_MSE, s->fit[l].gt));
    return seq_launch_bbme(s, l, fd, bbme_job(p, 0, fd, pairs, s->gme_bs, s->gme_sw, s->gme_procedure, GME_NORM_MSE, s->fit[l].gt));
}

// launch whatever gme_seq_gme_begin deferred, up to and including `level`
static int gme_flush_bbme(gme_seq* s, int level)
{
    for (int l = 0; l <= level && l <= 2; ++l) {
        const int rc = gme_level_bbme(s, l);
        if (rc) return rc;
    }
    return GME_OK;
}

// pyramid planes (utils.py:34-51): level 1 = pyrDown(level 2), level 0 = pyrDown(level 1), sized for the sequence
int seq_levels(gme_seq* s)
{
    for (int l = 1; l >= 0; --l) {
        const Plane& src = s->level[l + 1];
        if (!s->level[l].ptr) {
            const int rc = plane_alloc(s->ctx, &s->level[l], s->N_cap, (src.H + 1) / 2, (src.W + 1) / 2);
            if (rc) return rc;
        }
    }
    return GME_OK;
}

// ... and their contents, unless they are current
int seq_pyramids(gme_seq* s)
{
    if (!s->pyramids_valid) {
        for (int l = 1; l >= 0; --l) {
            Plane src = s->level[l + 1], dst = s->level[l];       // views over the frames in use (gme_seq_set_frames)
            src.count = dst.count = s->N;
            const int rc = launch_pyrdown(s->ctx, src, dst);
            if (rc) return rc;
        }
        s->pyramids_valid = true;
        s->sqbox_valid[0] = s->sqbox_valid[1] = false;
    }
    return GME_OK;
}

// pyramids, buffers, dense field and first parameters (motion.py:123-128,160-188) of a staged run; the context is locked
static int gme_begin_common(gme_seq* s, int fd, int bbme_bs, int procedure, int sw)
{
    gme_ctx* ctx = s->ctx;
    int rc = GME_OK;
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    GME_REQUIRE(bbme_bs >= 1, GME_ERR_ARG, "block_size %d", bbme_bs);
    const int pairs = s->N - fd;
    rc = seq_levels(s);
    if (rc) return rc;
    // argument checks for the three BBME runs before anything is launched
    rc = bbme_check_args(s->level[0].H, s->level[0].W, 2, 2, GME_SEARCH_DIAMOND, GME_NORM_MSE);
    if (rc) return rc;
    for (int l = 1; l <= 2; ++l) {
        rc = bbme_check_args(s->level[l].H, s->level[l].W, bbme_bs, sw, procedure, GME_NORM_MSE);
        if (rc) return rc;
    }
    rc = seq_pyramids(s);
    if (rc) return rc;
    const int cap_pairs = s->N_cap - fd;                   // buffers hold the sequence's full count: gme_seq_set_frames never reallocates
    if (s->params0.cap < (size_t)cap_pairs * 6 || s->gme_bs != bbme_bs) {
        // one group: whatever fails, no level and no parameter block is left that a later call could take for allocated
        s->params0.reset(); s->params_in.reset(); s->solve_flags.reset();
        rc = alloc_fit(s->fit[0], cap_pairs, s->level[0].H / 2, s->level[0].W / 2, false);
        for (int l = 1; l <= 2 && rc == GME_OK; ++l)
            rc = alloc_fit(s->fit[l], cap_pairs, s->level[l].H / bbme_bs, s->level[l].W / bbme_bs, true);
        if (rc == GME_OK)
            rc = dev_ensure_all("parameters", { { s->params0, (size_t)cap_pairs * 6 }, { s->solve_flags, (size_t)cap_pairs },
                                                { s->params_in, (size_t)cap_pairs * 12 } });      // 12: gme_seq_gme_fit2
        if (rc) {
            for (int l = 0; l <= 2; ++l) s->fit[l] = FitLevelBuf();
            s->gme_bs = 0;
            gme_drop_run(s);
            return rc;
        }
    }
    s->gme_fd = fd; s->gme_bs = bbme_bs; s->gme_pairs = pairs;
    s->gme_procedure = procedure; s->gme_sw = sw;
    s->bbme_pending[0] = s->bbme_pending[1] = s->bbme_pending[2] = true;
    // Launch order: dense field + first parameters, hand those to the host, and only then the level-1
    // search; the level-2 search (the longest kernel) is launched by gme_seq_gme_fit(level 1) after
    // it has the level-1 sums.  The host's projection / 3x3 solves between the stages then run
    // while the GPU searches the next level instead of leaving it idle (motion.py:123-136 is a
    // strict chain only through the small fits, not through the searches).
    rc = gme_level_bbme(s, 0);
    if (rc) return rc;
    GME_REQUIRE(s->fit[0].h > 0 && s->fit[0].w > 0, GME_ERR_GEOMETRY, "frames too small for a dense field");
    return launch_first_params(ctx, s->fit[0].gt, pairs, s->fit[0].h * s->fit[0].w, s->params0);
}

extern "C" int gme_seq_gme_begin(gme_seq* s, int fd, int bbme_bs, int procedure, int sw, float* params0_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = gme_begin_common(s, fd, bbme_bs, procedure, sw);
    if (rc) return rc;
    if (params0_out) {
        rc = copy_small(ctx, params0_out, s->params0, (size_t)s->gme_pairs * 6 * sizeof(float), hipMemcpyDeviceToHost, s->split_phase);
        if (rc) return rc;
        rc = seq_deliver(s);
        if (rc) return rc;
        return gme_level_bbme(s, 1);                       // runs while the caller projects the parameters
    }
    return gme_flush_bbme(s, 2);
}

// model field, mask and sums of level -1 (fit_mv), 1 or 2 from parameters already on the device (pstride doubles per
// pair); result copy + event / wait.  The context is locked.
static int fit_launch(gme_seq* s, int order, int level, const double* dparams, int pstride, double outlier_fraction, double* sums_out)
{
    gme_ctx* ctx = s->ctx;
    const bool mv = level < 0;
    const FitLevelBuf& f = mv ? s->fit_mv : s->fit[level];
    const int pairs = mv ? s->mv_pairs : s->gme_pairs, n = f.h * f.w;
    GME_REQUIRE(n > 0, GME_ERR_GEOMETRY, "level %d holds no block (motion.py:243 would index an empty list)", level);
    // int(0.3 * len), motion.py:242; a negative fraction selects the unmasked fit (motion.py:33-88)
    const int drop = outlier_fraction < 0 ? -1 : (int)(outlier_fraction * (double)n);
    GME_REQUIRE(drop <= n, GME_ERR_ARG, "outlier fraction %g out of range", outlier_fraction);
    const int level_H = mv ? s->H : s->level[level].H, level_W = mv ? s->W : s->level[level].W;
    int rc = launch_fit_level(ctx, f, order, pairs, dparams, pstride, drop, level_H, level_W);
    if (rc) return rc;
    if (!sums_out) return GME_OK;                          // gme_seq_gme_device_solve: the sums stay on the device
    rc = copy_small(ctx, sums_out, order == 1 ? f.sums : f.sums2, (size_t)pairs * order_sums(order) * sizeof(double),
                    hipMemcpyDeviceToHost, s->split_phase);
    return rc ? rc : seq_deliver(s);
}

// gme_seq_gme_begin + the projection of the first parameters (motion.py:191-207 on the float32 vector: two exact doublings)
// + gme_seq_gme_fit(level 1) without the trip to the host in between: the first parameters never leave the device on the
// way to the level-1 fit, so a staged run has three dependent host round trips instead of four.  params0_out may be NULL.
// At order 2 the level-1 field is that of the projected first parameters (a translation, six doubles per pair), so mask
// and threshold are those of order 1.
static int seq_begin_fit(gme_seq* s, int order, const char* who, int fd, int bbme_bs, int procedure, int sw,
                         double outlier_fraction, float* params0_out, double* sums1_out)
{
    GME_REQUIRE(s != nullptr && sums1_out != nullptr, GME_ERR_ARG, "%s: null pointer", who);
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = gme_begin_common(s, fd, bbme_bs, procedure, sw);
    if (rc) return rc;
    rc = launch_project_first(ctx, s->params0, s->gme_pairs, s->params_in);
    if (rc) return rc;
    if (params0_out)
        { rc = copy_small(ctx, params0_out, s->params0, (size_t)s->gme_pairs * 6 * sizeof(float), hipMemcpyDeviceToHost, s->split_phase); if (rc) return rc; }
    rc = gme_level_bbme(s, 1);
    if (rc) return rc;
    rc = fit_launch(s, order, 1, s->params_in, 6, outlier_fraction, sums1_out);
    if (rc) return rc;
    return gme_level_bbme(s, 2);                           // searched while the caller solves level 1
}

extern "C" int gme_seq_gme_begin_fit(gme_seq* s, int fd, int bbme_bs, int procedure, int sw, double outlier_fraction,
                                     float* params0_out, double* sums1_out)
{
    return seq_begin_fit(s, 1, "gme_seq_gme_begin_fit", fd, bbme_bs, procedure, sw, outlier_fraction, params0_out, sums1_out);
}

// stage buffers for fitting `mv` (gme_seq_bbme's field) at level -1; its gt is s->mv, borrowed
static int ensure_fit_mv(gme_seq* s)
{
    FitLevelBuf& f = s->fit_mv;
    if (!(f.h == s->mv_h && f.w == s->mv_w && s->fit_mv_pairs == s->mv_pairs && f.model)) {
        s->fit_mv_pairs = 0;
        const int rc = alloc_fit(f, s->mv_pairs, s->mv_h, s->mv_w, true, s->mv);
        if (rc) return rc;
        s->fit_mv_pairs = s->mv_pairs;
    }
    f.gt = s->mv;                             // gme_seq_bbme may have moved it since
    return GME_OK;
}

static int seq_fit(gme_seq* s, int order, const char* who, int level, const double* params_in, double outlier_fraction,
                   double* sums_out)
{
    GME_REQUIRE(s != nullptr && params_in != nullptr && sums_out != nullptr, GME_ERR_ARG, "%s: null pointer", who);
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = GME_OK;
    GME_REQUIRE(level == 1 || level == 2 || level == -1, GME_ERR_ARG, "%s: level %d (1, 2 or -1)", who, level);
    const int width = order_params(order);
    int pairs;
    double* dparams;
    if (level == -1) {
        GME_REQUIRE(s->mv != nullptr && s->mv_pairs > 0, GME_ERR_STATE, "%s(level -1) before gme_seq_bbme", who);
        rc = ensure_fit_mv(s);
        if (rc) return rc;
        pairs = s->mv_pairs;
        rc = s->mv_params.ensure((size_t)pairs * width, "fit parameters");
        if (rc) return rc;
        dparams = s->mv_params;
    } else {
        GME_REQUIRE(s->gme_pairs > 0 && s->params_in, GME_ERR_STATE, "%s before gme_seq_gme_begin", who);
        rc = gme_flush_bbme(s, level);
        if (rc) return rc;
        pairs = s->gme_pairs;
        dparams = s->params_in;
    }
    rc = copy_small(ctx, dparams, params_in, (size_t)pairs * width * sizeof(double), hipMemcpyHostToDevice, s->split_phase);
    if (rc) return rc;
    rc = fit_launch(s, order, level, dparams, width, outlier_fraction, sums_out);
    if (rc) return rc;
    if (level == 1) return gme_level_bbme(s, 2);           // searched while the caller solves level 1
    return GME_OK;
}

extern "C" int gme_seq_gme_fit(gme_seq* s, int level, const double* params_in, double outlier_fraction,
                               double* sums_out)
{
    return seq_fit(s, 1, "gme_seq_gme_fit", level, params_in, outlier_fraction, sums_out);
}

extern "C" int gme_seq_gme_read_stage(gme_seq* s, int level, int pair, int32_t* gt, int16_t* model, uint8_t* mask,
                                      int64_t* threshold)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = GME_OK;
    GME_REQUIRE(level >= -1 && level <= 2 && pair >= 0, GME_ERR_ARG, "gme_seq_gme_read_stage: bad index");
    GME_REQUIRE(level < 0 || s->gme_pairs > 0, GME_ERR_STATE, "gme_seq_gme_read_stage before gme_seq_gme_begin");
    GME_REQUIRE(pair < (level < 0 ? s->fit_mv_pairs : s->gme_pairs), GME_ERR_ARG, "gme_seq_gme_read_stage: bad index");
    if (level >= 0) {
        rc = gme_flush_bbme(s, level);
        if (rc) return rc;
    }
    const FitLevelBuf& f = level < 0 ? s->fit_mv : s->fit[level];
    const size_t n = (size_t)f.h * f.w;
    int32_t thr = 0;
    if (gt && n) GME_HIP_TRY(hipMemcpyAsync(gt, f.gt + n * 2 * pair, n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (level != 0) {
        if (model && n) GME_HIP_TRY(hipMemcpyAsync(model, f.model + n * 2 * pair, n * 2 * sizeof(int16_t), hipMemcpyDeviceToHost, ctx->stream));
        if (mask && n) GME_HIP_TRY(hipMemcpyAsync(mask, f.mask + n * pair, n, hipMemcpyDeviceToHost, ctx->stream));
        if (threshold) GME_HIP_TRY(hipMemcpyAsync(&thr, f.thr + pair, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    rc = ctx_finish(ctx);
    if (threshold) *threshold = thr;
    return rc;
}

// The compensated planes for a writer of `pairs` planes.  Every writer comes through here before it launches, so this is
// where the planes of the writer before it end (a reallocation included); the writer marks planes 0 .. pairs - 1 with
// comp_wrote once its launch is queued.
int ensure_comp(gme_seq* s, int fd, int pairs)
{
    gme_ctx* ctx = s->ctx;
    s->comp_written.flag.clear();
    if (!s->comp.ptr || s->comp.count < pairs) {
        const int cap_pairs = s->N_cap - fd > pairs ? s->N_cap - fd : pairs;
        s->sse.reset(); s->comp_params.reset();
        int rc = plane_alloc(ctx, &s->comp, cap_pairs, s->H, s->W);
        if (rc == GME_OK)
            rc = dev_ensure_all("compensation", { { s->sse, (size_t)cap_pairs }, { s->comp_params, (size_t)cap_pairs * 12 } });      // 12: gme_seq_compensate2
        if (rc) { s->comp = PlaneBuf(); return rc; }       // all or nothing: comp.ptr and comp.count say what the three hold
    }
    s->comp_written.flag.assign((size_t)s->comp.count, 0);
    return GME_OK;
}

void comp_wrote(gme_seq* s, int pairs) { s->comp_written.mark(0, pairs); }

// Order 1 evaluates the affine field per block inside k_compensate16 / k_compensate; order 2 first writes the int32 field
// of every pair with k_model2_field, then takes their mf32 path.  Both sum the squared error (results.py:52-59,109).
// compensate_launch takes the parameters from s->comp_params (and, order 2, s->comp_mf sized for the h x w fields).
static int compensate_launch(gme_seq* s, int order, int fd, int pairs, int h, int w)
{
    if (order == 2) {
        const int rc = launch_model2_field(s->ctx, s->comp_params, pairs, h, w, nullptr, s->comp_mf);
        if (rc) return rc;
    }
    const Plane& p = s->level[2];
    return launch_compensate(s->ctx, p.at(0), p.stride, pairs, s->H, s->W, p.pitch, order == 2 ? s->comp_mf : nullptr,
                             order == 2 ? nullptr : s->comp_params, h, w, s->comp.ptr, s->comp.stride, s->comp.pitch, p.at(fd),
                             p.stride, s->sse);
}

static int seq_compensate(gme_seq* s, int order, const char* who, int fd, int bs, const double* params, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr && params != nullptr, GME_ERR_ARG, "%s: null pointer", who);
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = GME_OK;
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    const int pairs = s->N - fd;
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    const int h = s->H / bs, w = s->W / bs;
    GME_REQUIRE(h > 0 && w > 0, GME_ERR_GEOMETRY, "block_size %d does not fit a %d x %d frame", bs, s->H, s->W);
    rc = ensure_comp(s, fd, pairs);
    if (rc) return rc;
    if (order == 2) {
        rc = s->comp_mf.ensure((size_t)pairs * h * w * 2, "order-2 field");
        if (rc) return rc;
    }
    rc = copy_small(ctx, s->comp_params, params, (size_t)pairs * order_params(order) * sizeof(double), hipMemcpyHostToDevice,
                    s->split_phase);
    if (rc) return rc;
    rc = compensate_launch(s, order, fd, pairs, h, w);
    if (rc) return rc;
    comp_wrote(s, pairs);
    if (sse_out) {
        rc = copy_small(ctx, sse_out, s->sse, (size_t)pairs * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->split_phase);
        return rc ? rc : seq_deliver(s);
    }
    return GME_OK;
}

extern "C" int gme_seq_compensate(gme_seq* s, int fd, int bs, const double* params, int64_t* sse_out)
{
    return seq_compensate(s, 1, "gme_seq_compensate", fd, bs, params, sse_out);
}

// `count` compensated frames starting at pair `first` into out[count][H][W] (tight) with ONE wait: what results.py's
// per-pair imwrite loop (results.py:59-76) needs of a finished chunk (a blocking read per pair stalled the one host
// thread that drives all lanes of sequence.StreamEstimator).
extern "C" int gme_seq_read_compensated_range(gme_seq* s, int first, int count, uint8_t* out)
{
    GME_REQUIRE(s != nullptr && out != nullptr, GME_ERR_ARG, "gme_seq_read_compensated_range: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(s->comp.ptr && first >= 0 && count >= 0 && first + count <= s->comp.count, GME_ERR_STATE,
                "gme_seq_read_compensated_range: pairs %d .. %d of %d", first, first + count, s->comp.ptr ? s->comp.count : 0);
    GME_REQUIRE(s->comp_written.all(first, count), GME_ERR_STATE,
                "gme_seq_read_compensated_range: the last compensating call did not write all of pairs %d .. %d", first, first + count);
    const int rc = read_planes(s->ctx, s->comp, first, count, out);
    if (rc) return rc;
    GME_HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return GME_OK;
}

static bool model2_known(int model)
{
    return model == GME_MODEL_BILINEAR || model == GME_MODEL_PSEUDO_PERSPECTIVE || model == GME_MODEL_QUADRATIC;
}

// the device solve between two stages: order 1 the two 3x3 systems (k_solve3), order 2 the model's system (k_solve_model2)
static int solve_launch(gme_ctx* ctx, int order, int model, const double* sums, int pairs, int project, int h, int w,
                        double* params_out, int32_t* flags, int flag_bit)
{
    if (order == 1) return launch_solve3(ctx, sums, pairs, project, h, w, params_out, flags, flag_bit);
    return launch_solve_model2(ctx, sums, model, pairs, project, h, w, params_out, flags, flag_bit);
}

static int solve_sums(gme_ctx* ctx, int order, int model, const char* who, const double* sums, int pairs, int project, int h, int w,
                      double* params_out, int32_t* flags_out)
{
    GME_ENTER(ctx);
    GME_REQUIRE(sums != nullptr && params_out != nullptr && flags_out != nullptr && pairs >= 0 && h >= 0 && w >= 0, GME_ERR_ARG,
                "%s: bad arguments", who);
    GME_REQUIRE(order == 1 || model2_known(model), GME_ERR_ARG, "%s: model %d is not a second-order model (%d, %d or %d)", who,
                model, GME_MODEL_BILINEAR, GME_MODEL_PSEUDO_PERSPECTIVE, GME_MODEL_QUADRATIC);
    if (pairs == 0) return GME_OK;
    void* buf = nullptr;
    const size_t b_sums = (size_t)pairs * order_sums(order) * sizeof(double), b_par = (size_t)pairs * order_params(order) * sizeof(double);
    const size_t b_fl = (size_t)pairs * sizeof(int32_t);
    int rc = ctx_scratch(ctx, b_sums + b_par + b_fl, &buf);
    if (rc) return rc;
    double* d_sums = (double*)buf;
    double* d_par = (double*)((char*)buf + b_sums);
    int32_t* d_fl = (int32_t*)((char*)buf + b_sums + b_par);
    GME_HIP_TRY(hipMemcpyAsync(d_sums, sums, b_sums, hipMemcpyHostToDevice, ctx->stream));
    GME_HIP_TRY(hipMemsetAsync(d_fl, 0, b_fl, ctx->stream));
    rc = solve_launch(ctx, order, model, d_sums, pairs, project, h, w, d_par, d_fl, 1);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(params_out, d_par, b_par, hipMemcpyDeviceToHost, ctx->stream));
    GME_HIP_TRY(hipMemcpyAsync(flags_out, d_fl, b_fl, hipMemcpyDeviceToHost, ctx->stream));
    return ctx_finish(ctx);
}

// The device solve on its own (what gme_seq_gme_device_solve runs between its stages), for callers and tests that hold
// normal-equation sums: sums[P][15] = F | Sx | Sy -> params_out[P][6] (first components doubled if `project`,
// motion.py:191-207) and flags_out[P]: bit 1 where a displacement of the h x w model field of those parameters lies within
// 1e-9 max(1, S) of a rounding tie (S = |p0| + |p1| (h - 1) + |p2| (w - 1)), bit 4 for a singular system, bit 8 for an
// ill-conditioned one (k_solve3, gme_kernels.hip).
extern "C" int gme_solve_fit_sums(gme_ctx* ctx, const double* sums, int pairs, int project, int h, int w, double* params_out,
                                  int32_t* flags_out)
{
    return solve_sums(ctx, 1, 0, "gme_solve_fit_sums", sums, pairs, project, h, w, params_out, flags_out);
}

// begin + level-1 fit, solve + projection, level-2 fit, solve, field + compensation, all queued on the stream; the solves of
// `order` write their flags into s->solve_flags.  The context is locked by the entry points below.
static int seq_device_solve(gme_seq* s, int order, int model, const char* who, int fd, int bbme_bs, int procedure, int sw,
                            double outlier_fraction, double* params_out, int64_t* sse_out, int32_t* flags_out)
{
    GME_REQUIRE(s != nullptr && params_out != nullptr && flags_out != nullptr, GME_ERR_ARG, "%s: null pointer", who);
    GME_REQUIRE(order == 1 || model2_known(model), GME_ERR_ARG, "%s: model %d is not a second-order model (%d, %d or %d)", who,
                model, GME_MODEL_BILINEAR, GME_MODEL_PSEUDO_PERSPECTIVE, GME_MODEL_QUADRATIC);
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    int rc = gme_begin_common(s, fd, bbme_bs, procedure, sw);
    if (rc) return rc;
    const int pairs = s->gme_pairs;
    const int h = s->H / bbme_bs, w = s->W / bbme_bs;
    GME_REQUIRE(h > 0 && w > 0, GME_ERR_GEOMETRY, "block_size %d does not fit a %d x %d frame", bbme_bs, s->H, s->W);
    rc = ensure_comp(s, fd, pairs);
    if (rc) return rc;
    if (order == 2) {
        rc = s->comp_mf.ensure((size_t)pairs * h * w * 2, "order-2 field");
        if (rc) return rc;
    }
    GME_HIP_TRY(hipMemsetAsync(s->solve_flags, 0, (size_t)(pairs > 0 ? pairs : 1) * sizeof(int32_t), ctx->stream));
    rc = launch_project_first(ctx, s->params0, pairs, s->params_in);
    if (rc) return rc;
    rc = gme_level_bbme(s, 1);
    if (rc) return rc;
    rc = gme_level_bbme(s, 2);                             // independent of the parameters: queued ahead of the level-1 fit
    if (rc) return rc;
    rc = fit_launch(s, order, 1, s->params_in, 6, outlier_fraction, nullptr);
    if (rc) return rc;
    // level-1 solution, projected (motion.py:191-207), used for the level-2 model field: flag bit 1 where that rounds near a tie
    rc = solve_launch(ctx, order, model, order == 1 ? s->fit[1].sums : s->fit[1].sums2, pairs, 1, s->fit[2].h, s->fit[2].w,
                      s->params_in, s->solve_flags, 1);
    if (rc) return rc;
    rc = fit_launch(s, order, 2, s->params_in, order_params(order), outlier_fraction, nullptr);
    if (rc) return rc;
    rc = solve_launch(ctx, order, model, order == 1 ? s->fit[2].sums : s->fit[2].sums2, pairs, 0, h, w, s->comp_params,
                      s->solve_flags, 2);
    if (rc) return rc;
    rc = compensate_launch(s, order, fd, pairs, h, w);
    if (rc) return rc;
    comp_wrote(s, pairs);
    rc = copy_small(ctx, params_out, s->comp_params, (size_t)pairs * order_params(order) * sizeof(double), hipMemcpyDeviceToHost,
                    s->split_phase);
    if (rc) return rc;
    if (sse_out) { rc = copy_small(ctx, sse_out, s->sse, (size_t)pairs * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->split_phase); if (rc) return rc; }
    rc = copy_small(ctx, flags_out, s->solve_flags, (size_t)pairs * sizeof(int32_t), hipMemcpyDeviceToHost, s->split_phase);
    return rc ? rc : seq_deliver(s);
}

// motion.global_motion_estimation + get_motion_field_affine + compensate_frame + the squared error of results.py:50-59,109
// for every pair in ONE call with ONE host round trip: the 3x3 solves of motion.py:262-264,280-282 run on the device
// (k_solve3, gme_kernels.hip).  Opt-in (the package uses it under GME_DEVICE_SOLVE=1): LAPACK's last bits are not
// reproduced, parameters are within 1e-10 max(1, S) of the host path's per term (the header has the bound); flags_out[p] != 0
// names the pairs the caller must redo through the host path (a model displacement within 1e-9 max(1, S) of a rounding tie:
// bit 1 at level 2, bit 2 in the final field; bit 4: a singular system, numpy.linalg.LinAlgError upstream; bit 8: an
// ill-conditioned one) -- for all other pairs model fields, masks, compensated frames and squared errors are bit-equal to
// the staged calls'.  Split-phase like them.
extern "C" int gme_seq_gme_device_solve(gme_seq* s, int fd, int bbme_bs, int procedure, int sw, double outlier_fraction,
                                        double* params_out, int64_t* sse_out, int32_t* flags_out)
{
    return seq_device_solve(s, 1, 0, "gme_seq_gme_device_solve", fd, bbme_bs, procedure, sw, outlier_fraction, params_out,
                            sse_out, flags_out);
}

extern "C" int gme_seq_read_compensated(gme_seq* s, int pair, uint8_t* out)
{
    GME_REQUIRE(s != nullptr && out != nullptr, GME_ERR_ARG, "gme_seq_read_compensated: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(s->comp.ptr && pair >= 0 && pair < s->comp.count, GME_ERR_STATE, "gme_seq_read_compensated: no such pair");
    GME_REQUIRE(s->comp_written.all(pair, 1), GME_ERR_STATE, "gme_seq_read_compensated: the last compensating call did not write pair %d", pair);
    const int rc = read_planes(s->ctx, s->comp, pair, 1, out);
    return rc ? rc : ctx_finish(s->ctx);
}

// ---------------------------------------------------------------------------
// Second-order motion models (roadmap.py: bilinear, pseudo-perspective, quadratic; kernels in gme_kernels.hip).  The calls
// below are the order-1 calls above with params [P][12] = [a0 a1 a2 b0 b1 b2 | a3 a4 a5 b3 b4 b5] and sums [P][27]; same
// staging, split-phase behaviour and state errors.  The stage buffers (model field, mask, threshold, compensated frames)
// are shared with the order-1 calls, so gme_seq_gme_read_stage / gme_seq_read_compensated[_range] read whichever ran last.
// ---------------------------------------------------------------------------
extern "C" int gme_model2_field(gme_ctx* ctx, const double params[12], int h, int w, int16_t* mf_out)
{
    return model_field(ctx, 2, "gme_model2_field", params, h, w, mf_out);
}

extern "C" int gme_seq_gme_begin_fit2(gme_seq* s, int fd, int bbme_bs, int procedure, int sw, double outlier_fraction,
                                      float* params0_out, double* sums1_out)
{
    return seq_begin_fit(s, 2, "gme_seq_gme_begin_fit2", fd, bbme_bs, procedure, sw, outlier_fraction, params0_out, sums1_out);
}

extern "C" int gme_seq_gme_fit2(gme_seq* s, int level, const double* params_in, double outlier_fraction, double* sums_out)
{
    return seq_fit(s, 2, "gme_seq_gme_fit2", level, params_in, outlier_fraction, sums_out);
}

extern "C" int gme_seq_compensate2(gme_seq* s, int fd, int bs, const double* params, int64_t* sse_out)
{
    return seq_compensate(s, 2, "gme_seq_compensate2", fd, bs, params, sse_out);
}

// The order-2 device solves (k_solve_model2): the contract is the header's.
extern "C" int gme_solve_model2_sums(gme_ctx* ctx, int model, const double* sums, int pairs, int project, int h, int w,
                                     double* params_out, int32_t* flags_out)
{
    return solve_sums(ctx, 2, model, "gme_solve_model2_sums", sums, pairs, project, h, w, params_out, flags_out);
}

extern "C" int gme_seq_gme_device_solve2(gme_seq* s, int model, int fd, int bbme_bs, int procedure, int sw,
                                         double outlier_fraction, double* params_out, int64_t* sse_out, int32_t* flags_out)
{
    return seq_device_solve(s, 2, model, "gme_seq_gme_device_solve2", fd, bbme_bs, procedure, sw, outlier_fraction, params_out,
                            sse_out, flags_out);
}
