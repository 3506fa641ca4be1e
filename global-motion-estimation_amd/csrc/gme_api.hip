// C ABI of libgme_hip.so (include/gme_hip.h): contexts, sequences, host<->device
// plumbing around the kernels in bbme_*.hip, gme_kernels.hip and synth_kernels.hip.
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

// Every entry point that touches a context holds its mutex for the whole call: the context owns ONE
// stream and ONE growable scratch buffer, and ctypes releases the GIL, so two Python threads inside
// the module-level bbme/motion/utils functions (one shared default context) would otherwise carve
// the same scratch offsets or free the buffer under each other's kernels.  Calls on one context
// serialise; use one context per thread (sequence.ShardedSequence does) for concurrency.
#define GME_ENTER(c)                                                  \
    GME_REQUIRE((c) != nullptr, GME_ERR_ARG, "null context");         \
    std::lock_guard<std::mutex> gme_lock__((c)->mu);                  \
    GME_HIP_TRY(hipSetDevice((c)->device))

// wait for the stream and report a tripped in-kernel guard
static int ctx_finish(gme_ctx* ctx)
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

// The scratch of a single-pair call: take() sub-buffers (256-byte aligned, in order), then commit() gets the block from the
// context and sets every pointer handed to take().
struct Carver {
    void* var[8];
    size_t at[8], off = 0;
    int n = 0;
    template <class T> void take(T** v, size_t count)
    {
        var[n] = v; at[n++] = off;
        off = (off + count * sizeof(T) + 255) & ~(size_t)255;
    }
    // a plane of plane_shape(); guard: with the guard row behind it
    void take(Plane* v, bool guard) { take(&v->ptr, v->bytes() + (guard ? v->pitch : 0)); }
    int commit(gme_ctx* ctx)
    {
        void* base = nullptr;
        const int rc = ctx_scratch(ctx, off, &base);
        if (rc) return rc;
        for (int i = 0; i < n; ++i) {
            void* ptr = (uint8_t*)base + at[i];
            memcpy(var[i], &ptr, sizeof(ptr));                 // whatever T, *var[i] is an object pointer
        }
        return GME_OK;
    }
};

// a host image with rows `stride` bytes apart into plane 0 of v, queued on the context's stream
static hipError_t put_plane(gme_ctx* ctx, const Plane& v, const uint8_t* host, int stride)
{
    return hipMemcpy2DAsync(v.ptr, v.pitch, host, stride, v.W, v.H, hipMemcpyHostToDevice, ctx->stream);
}

// host images with rows `stride` bytes apart into planes 0, 1, ... of a stack, queued on the context's stream
static int put_planes(gme_ctx* ctx, const Plane& st, std::initializer_list<const uint8_t*> host, int stride)
{
    int k = 0;
    for (const uint8_t* image : host) {
        Plane one = st;
        one.ptr = st.at(k++);
        GME_HIP_TRY(put_plane(ctx, one, image, stride));
    }
    return GME_OK;
}

// planes first .. first + count - 1 of a stack into out[count][H][W] (tight), queued on the context's stream
static int read_planes(gme_ctx* ctx, const Plane& p, int first, int count, uint8_t* out)
{
    for (int k = 0; k < count; ++k)
        GME_HIP_TRY(hipMemcpy2DAsync(out + (size_t)k * p.H * p.W, p.W, p.at(first + k), p.pitch, p.W, p.H, hipMemcpyDeviceToHost,
                                     ctx->stream));
    return GME_OK;
}

// the pointer and shape rules of a single-pair call `who` on host images; `pointers`: none of those it needs is null
static int oneshot_check(const char* who, bool pointers, int H, int W, int stride)
{
    GME_REQUIRE(pointers, GME_ERR_ARG, "%s: null pointer", who);
    GME_REQUIRE(H > 0 && W > 0 && stride >= W, GME_ERR_ARG, "%s: bad shape H=%d W=%d stride=%d", who, H, W, stride);
    return GME_OK;
}

// The ending of a single-pair call that can predict (gme_bipred_u8, gme_gmc_u8): where the caller wants the predicted frame or
// its squared error, predict() launches it into plane `pred` of the stack with the error in *d_sse (device); then the wait.
template <class Predict>
static int oneshot_predict(gme_ctx* ctx, const Plane& st, int pred, const unsigned long long* d_sse, uint8_t* pred_out, int64_t* sse_out,
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

// The search of the pairs (first + k, first + k + fd), k < pairs, of a plane stack into mf.
static BbmeJob bbme_job(const Plane& p, int first, int fd, int pairs, int bs, int sw, int procedure, int pnorm, int32_t* mf)
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
    if (plane_alloc(ctx, &s->level[2], n_frames, H, W) != GME_OK) { delete s; return nullptr; }
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
    delete s;                                              // frees the sequence's device buffers
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

// Replacing the motion field ends what was derived from it: the quarter-pel, hierarchical, variable-block-size and propagation
// results.  Every writer of s->mv comes through here, and so do new frames; a result type that reads the field joins this list.
static void seq_field_replaced(gme_seq* s)
{
    s->qmv_valid = false;
    s->hier_valid = false;
    s->vbs_valid = false;
    s->prop_valid = false;
}

// the frames changed: pyramids and auxiliary tables are stale, a staged run ends, and so does every result that was measured
// on the old frames (the motion field stays: it is a prior; the compensated and warped frames, mosaic and masks stay too)
static void seq_frames_changed(gme_seq* s)
{
    s->pyramids_valid = false;
    s->sqbox_valid[0] = s->sqbox_valid[1] = s->sqbox_valid[2] = false;
    seq_field_replaced(s);
    s->bp_valid = false;
    s->gm_valid = false;
    gme_drop_run(s);
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
static int seq_launch_bbme_from(gme_seq* s, int level, int first_cur, BbmeJob job)
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
static int seq_levels(gme_seq* s)
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
static int seq_pyramids(gme_seq* s)
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
static int ensure_comp(gme_seq* s, int fd, int pairs)
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

static void comp_wrote(gme_seq* s, int pairs) { s->comp_written.mark(0, pairs); }

// What the predicting entries of the block-field passes share behind their own state checks: the compensated planes for
// `planes` pairs or targets, predict() (the pass's launch into s->comp and s->sse), the squared errors into sse_out where the
// caller wants them, and the wait.
template <class Predict>
static int seq_predict(gme_seq* s, int fd, int planes, int64_t* sse_out, Predict predict)
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
static int seq_read(gme_seq* s, const char* who, bool valid, const char* made_by, const char* noun, int first, int count, int limit,
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
    if (s->warped.ptr) return GME_OK;
    int rc = plane_alloc(s->ctx, &s->warped, s->N_cap, s->H, s->W);
    if (rc == GME_OK)
        rc = dev_ensure_all("stabilization buffers", { { s->warp_params, (size_t)s->N_cap * 8 }, { s->warp_counts, (size_t)s->N_cap } });
    if (rc) { s->warped = PlaneBuf(); s->warped_written.flag.clear(); return rc; }
    s->warped_written.flag.assign((size_t)s->N_cap, 0);
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
    GME_HIP_TRY(hipMemcpyAsync(s->warp_params, params, (size_t)count * 8 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_warp_frames(ctx, s->level[2], s->warped, first, count, s->warp_params, border, fill, s->warp_counts);
    if (rc) return rc;
    if (valid_out)
        GME_HIP_TRY(hipMemcpyAsync(valid_out, s->warp_counts, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                   ctx->stream));
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->warped_written.mark(first, count);
    return GME_OK;
}

extern "C" int gme_seq_read_warped_range(gme_seq* s, int first, int count, uint8_t* out)
{
    GME_REQUIRE(s != nullptr && out != nullptr, GME_ERR_ARG, "gme_seq_read_warped_range: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(first >= 0 && count >= 0 && first + count <= s->N, GME_ERR_ARG,
                "gme_seq_read_warped_range: frames [%d, %d) outside [0, %d)", first, first + count, s->N);
    GME_REQUIRE(s->warped_written.all(first, count), GME_ERR_ARG, "gme_seq_read_warped_range: frames [%d, %d) were never warped",
                first, first + count);
    const int rc = read_planes(s->ctx, s->warped, first, count, out);
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
    GME_REQUIRE(!warped || s->warped_written.all(first, count + 1), GME_ERR_ARG, "gme_seq_frame_sse: frames [%d, %d] were never warped",
                first, first + count);
    int rc = stab_buffers(s);
    if (rc) return rc;
    rc = launch_frame_sse(ctx, warped ? s->warped : s->level[2], first, count, s->warp_counts);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(sse_out, s->warp_counts, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
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
    if (s->mosaic_params) return GME_OK;
    return dev_ensure_all("mosaic parameters", { { s->mosaic_params, (size_t)s->N_cap * 8 }, { s->mosaic_usable, (size_t)s->N_cap },
                                                 { s->mosaic_counts, (size_t)s->N_cap * 2 } });
}

// the per-frame rows of a call: parameters and usable flags (all ones for NULL) to the device
static int mosaic_put_rows(gme_seq* s, int count, const double* params, const uint8_t* usable)
{
    hipStream_t st = s->ctx->stream;
    GME_HIP_TRY(hipMemcpyAsync(s->mosaic_params, params, (size_t)count * 8 * sizeof(double), hipMemcpyHostToDevice, st));
    if (usable) GME_HIP_TRY(hipMemcpyAsync(s->mosaic_usable, usable, (size_t)count, hipMemcpyHostToDevice, st));
    else GME_HIP_TRY(hipMemsetAsync(s->mosaic_usable, 1, (size_t)count, st));
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
    s->mosaic_valid = false;
    if (pixels > s->mosaic_sprite.cap) {
        s->mosaic_sprite.reset(); s->mosaic_count.reset();     // both go before either comes back: no more memory at the peak
        rc = dev_ensure_all("mosaic", { { s->mosaic_sprite, pixels }, { s->mosaic_count, pixels } });
        if (rc) return rc;
    }
    GME_HIP_TRY(hipMemsetAsync(s->mosaic_sprite, 0, pixels, ctx->stream));
    GME_HIP_TRY(hipMemsetAsync(s->mosaic_count, 0, pixels * sizeof(uint16_t), ctx->stream));
    rc = mosaic_put_rows(s, count, inv_warps, usable);
    if (rc) return rc;
    rc = launch_mosaic_median(ctx, s->level[2], first, count, s->mosaic_params, s->mosaic_usable, ox, oy, Hc, Wc, fill, cull,
                              s->mosaic_sprite, s->mosaic_count, pitch);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->mosaic_Hc = Hc; s->mosaic_Wc = Wc; s->mosaic_pitch = pitch;
    s->mosaic_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_mosaic(gme_seq* s, uint8_t* sprite, uint16_t* count)
{
    GME_REQUIRE(s != nullptr && sprite != nullptr, GME_ERR_ARG, "gme_seq_read_mosaic: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(s->mosaic_valid, GME_ERR_ARG, "gme_seq_read_mosaic: no mosaic was built (gme_seq_mosaic first)");
    const int Hc = s->mosaic_Hc, Wc = s->mosaic_Wc, pitch = s->mosaic_pitch;
    GME_HIP_TRY(hipMemcpy2DAsync(sprite, Wc, s->mosaic_sprite, pitch, Wc, Hc, hipMemcpyDeviceToHost, s->ctx->stream));
    if (count)
        GME_HIP_TRY(hipMemcpy2DAsync(count, (size_t)Wc * sizeof(uint16_t), s->mosaic_count, (size_t)pitch * sizeof(uint16_t),
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
    GME_REQUIRE(s->mosaic_valid, GME_ERR_ARG, "gme_seq_moving_masks: no mosaic was built (gme_seq_mosaic first)");
    if (count == 0) return GME_OK;
    int rc = mosaic_rows(s);
    if (rc) return rc;
    if (!s->masks.ptr) {
        rc = plane_alloc(ctx, &s->masks, s->N_cap, s->H, s->W);
        if (rc) { s->masks_written.flag.clear(); return rc; }
        s->masks_written.flag.assign((size_t)s->N_cap, 0);
    }
    rc = mosaic_put_rows(s, count, warps, usable);
    if (rc) return rc;
    unsigned long long* known = s->mosaic_counts;
    unsigned long long* moving = s->mosaic_counts + s->N_cap;
    GME_HIP_TRY(hipMemsetAsync(s->mosaic_counts, 0, (size_t)s->N_cap * 2 * sizeof(unsigned long long), ctx->stream));
    rc = launch_moving_masks(ctx, s->level[2], s->masks, first, count, s->mosaic_params, s->mosaic_usable, s->mosaic_sprite,
                             s->mosaic_count, s->mosaic_pitch, s->mosaic_Hc, s->mosaic_Wc, ox, oy, threshold, min_count, known,
                             moving);
    if (rc) return rc;
    if (known_out)
        GME_HIP_TRY(hipMemcpyAsync(known_out, known, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    if (moving_out)
        GME_HIP_TRY(hipMemcpyAsync(moving_out, moving, (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->masks_written.mark(first, count);
    return GME_OK;
}

extern "C" int gme_seq_read_masks_range(gme_seq* s, int first, int count, uint8_t* out)
{
    GME_REQUIRE(s != nullptr && out != nullptr, GME_ERR_ARG, "gme_seq_read_masks_range: null pointer");
    GME_ENTER(s->ctx);
    GME_REQUIRE(first >= 0 && count >= 0 && first + count <= s->N, GME_ERR_ARG,
                "gme_seq_read_masks_range: frames [%d, %d) outside [0, %d)", first, first + count, s->N);
    GME_REQUIRE(s->masks_written.all(first, count), GME_ERR_ARG, "gme_seq_read_masks_range: the masks of frames [%d, %d) were never computed", first,
                first + count);
    const int rc = read_planes(s->ctx, s->masks, first, count, out);
    return rc ? rc : ctx_finish(s->ctx);
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
    s->qmv_valid = false;
    rc = s->qmv.ensure(n * 2, "quarter-pel field");
    if (rc) return rc;
    rc = s->qcost.ensure(n, "quarter-pel costs");
    if (rc) return rc;
    const Plane& p = s->level[2];
    rc = launch_subpel_refine(ctx, p.at(0), p.at(fd), p.stride, s->mv_pairs, s->H, s->W, p.pitch, bs, pnorm, levels, s->mv, s->qmv,
                              s->qcost);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->qmv_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_qmv(gme_seq* s, int first_pair, int count, int32_t* qmf_out, int64_t* cost_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_qmv: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->mv_h * s->mv_w;
    return seq_read(s, "gme_seq_read_qmv", s->qmv_valid, "gme_seq_subpel", "pairs", first_pair, count, s->mv_pairs,
                    { { qmf_out, s->qmv.get(), per * 2 * sizeof(int32_t) }, { cost_out, s->qcost.get(), per * sizeof(long long) } });
}

extern "C" int gme_seq_compensate_qpel(gme_seq* s, int fd, int bs, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_compensate_qpel: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    GME_REQUIRE(s->qmv_valid, GME_ERR_STATE, "gme_seq_compensate_qpel before gme_seq_subpel");
    int rc = subpel_field(s, "gme_seq_compensate_qpel", fd, bs);
    if (rc) return rc;
    const int pairs = s->mv_pairs;
    const Plane& p = s->level[2];
    return seq_predict(s, fd, pairs, sse_out, [&] {
        return launch_compensate_qpel(ctx, p.at(0), p.at(fd), p.stride, pairs, s->H, s->W, p.pitch, bs, s->qmv, s->comp.ptr, s->comp.stride,
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
            rc = s->hier_mv[l].ensure(n * 2, "hierarchical fields");
            if (rc) return rc;
        }
        rc = s->hier_cost[l].ensure(n, "hierarchical costs");
        if (rc) return rc;
    }
    const Plane lv[3] = { s->level[0], s->level[1], s->level[2] };
    int32_t* const mf[3] = { s->hier_mv[0].get(), s->hier_mv[1].get(), s->mv.get() };
    long long* const cost[3] = { s->hier_cost[0].get(), s->hier_cost[1].get(), s->hier_cost[2].get() };
    rc = launch_hier(ctx, lv, 0, fd, pairs, bs, cw, radius, pnorm, levels, mf, cost);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->hier_levels = levels;
    s->hier_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_hier(gme_seq* s, int level, int first_pair, int count, int32_t* mf_out, int64_t* cost_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_hier: null sequence");
    GME_ENTER(s->ctx);
    // the level indexes the table below, and which levels there are is part of the result: both checks come before it
    GME_REQUIRE(s->hier_valid, GME_ERR_STATE, "gme_seq_read_hier before gme_seq_hier");
    GME_REQUIRE(level >= 3 - s->hier_levels && level <= 2, GME_ERR_ARG, "gme_seq_read_hier: level %d, the last gme_seq_hier used %d .. 2",
                level, 3 - s->hier_levels);
    const size_t per = (size_t)s->mv_h * s->mv_w;
    return seq_read(s, "gme_seq_read_hier", s->hier_valid, "gme_seq_hier", "pairs", first_pair, count, s->mv_pairs,
                    { { mf_out, level == 2 ? s->mv.get() : s->hier_mv[level].get(), per * 2 * sizeof(int32_t) },
                      { cost_out, s->hier_cost[level].get(), per * sizeof(long long) } });
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
    s->vbs_valid = false;
    rc = s->vbs_leaf.ensure(cells * 2, "variable-block-size field");
    if (rc) return rc;
    rc = s->vbs_dmap.ensure(cells, "variable-block-size depths");
    if (rc) return rc;
    rc = s->vbs_cost.ensure(n, "variable-block-size costs");
    if (rc) return rc;
    const Plane& p = s->level[2];
    rc = launch_vbs(ctx, p.at(0), p.at(fd), p.stride, s->mv_pairs, s->H, s->W, p.pitch, bs, depth, radius, pnorm, penalty, s->mv,
                    s->vbs_leaf, s->vbs_dmap, s->vbs_cost);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->vbs_depth = depth;
    s->vbs_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_vbs(gme_seq* s, int first_pair, int count, int32_t* leaf_out, uint8_t* depth_out, int64_t* cost_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_vbs: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->mv_h * s->mv_w, cells = per << (2 * s->vbs_depth);
    return seq_read(s, "gme_seq_read_vbs", s->vbs_valid, "gme_seq_vbs", "pairs", first_pair, count, s->mv_pairs,
                    { { leaf_out, s->vbs_leaf.get(), cells * 2 * sizeof(int32_t) }, { depth_out, s->vbs_dmap.get(), cells },
                      { cost_out, s->vbs_cost.get(), per * sizeof(long long) } });
}

extern "C" int gme_seq_compensate_vbs(gme_seq* s, int fd, int bs, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_compensate_vbs: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(fd >= 1 && fd < s->N, GME_ERR_ARG, "frame_distance %d needs at least %d frames", fd, fd + 1);
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    GME_REQUIRE(s->vbs_valid, GME_ERR_STATE, "gme_seq_compensate_vbs before gme_seq_vbs");
    int rc = subpel_field(s, "gme_seq_compensate_vbs", fd, bs);
    if (rc) return rc;
    const int pairs = s->mv_pairs;
    const Plane& p = s->level[2];
    return seq_predict(s, fd, pairs, sse_out, [&] {
        return launch_compensate_vbs(ctx, p.at(0), p.at(fd), p.stride, pairs, s->H, s->W, p.pitch, bs >> s->vbs_depth, s->mv_h << s->vbs_depth,
                                     s->mv_w << s->vbs_depth, s->vbs_leaf, s->comp.ptr, s->comp.stride, s->comp.pitch, s->sse);
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
    s->bp_valid = false;
    rc = dev_ensure_all("bidirectional prediction", { { s->bp_f0, n * 2 }, { s->bp_f1, n * 2 }, { s->bp_v0, n * 2 }, { s->bp_v1, n * 2 } });
    if (rc) return rc;
    rc = s->bp_mode.ensure(n, "bidirectional modes");
    if (rc) return rc;
    rc = dev_ensure_all("bidirectional costs", { { s->bp_cost, n }, { s->bp_costs, n * 3 } });
    if (rc) return rc;
    const Plane& p = s->level[2];
    // the anchor of both searches is the target frame t = fd + k; it is looked for in frame t - fd = k and in frame t + fd
    BbmeJob job = bbme_job(p, fd, 0, T, bs, sw, procedure, pnorm, s->bp_f0);
    job.cur = p.at(0);
    rc = seq_launch_bbme_from(s, 2, 0, job);
    if (rc) return rc;
    rc = seq_launch_bbme_from(s, 2, 2 * fd, bbme_job(p, fd, fd, T, bs, sw, procedure, pnorm, s->bp_f1));
    if (rc) return rc;
    rc = launch_bipred(ctx, p.at(0), p.at(fd), p.at(2 * fd), p.stride, T, s->H, s->W, p.pitch, bs, radius, rounds, pnorm, penalty, s->bp_f0,
                       s->bp_f1, s->bp_mode, s->bp_v0, s->bp_v1, s->bp_cost, s->bp_costs);
    if (rc) return rc;
    rc = ctx_finish(ctx);
    if (rc) return rc;
    s->bp_targets = T; s->bp_h = h; s->bp_w = w; s->bp_fd = fd; s->bp_bs = bs;
    s->bp_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_bipred(gme_seq* s, int first, int count, int32_t* f0_out, int32_t* f1_out, uint8_t* mode_out, int32_t* v0_out,
                                   int32_t* v1_out, int64_t* cost_out, int64_t* costs_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_bipred: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->bp_h * s->bp_w, vec = per * 2 * sizeof(int32_t);
    return seq_read(s, "gme_seq_read_bipred", s->bp_valid, "gme_seq_bipred", "targets", first, count, s->bp_targets,
                    { { f0_out, s->bp_f0.get(), vec }, { f1_out, s->bp_f1.get(), vec }, { mode_out, s->bp_mode.get(), per },
                      { v0_out, s->bp_v0.get(), vec }, { v1_out, s->bp_v1.get(), vec },
                      { cost_out, s->bp_cost.get(), per * sizeof(long long) }, { costs_out, s->bp_costs.get(), per * 3 * sizeof(long long) } });
}

extern "C" int gme_seq_predict_bipred(gme_seq* s, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_predict_bipred: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(s->bp_valid, GME_ERR_STATE, "gme_seq_predict_bipred before gme_seq_bipred");
    const int T = s->bp_targets, fd = s->bp_fd;
    GME_REQUIRE(T <= s->N - 2 * fd, GME_ERR_STATE, "gme_seq_predict_bipred: %d targets, the sequence has %d", T, s->N - 2 * fd);
    const Plane& p = s->level[2];
    return seq_predict(s, fd, T, sse_out, [&] {
        return launch_predict_bipred(ctx, p.at(0), p.at(fd), p.at(2 * fd), p.stride, T, s->H, s->W, p.pitch, s->bp_bs, s->bp_mode, s->bp_v0,
                                     s->bp_v1, s->comp.ptr, s->comp.stride, s->comp.pitch, s->sse);
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
    s->gm_valid = false;
    rc = s->gm_f.ensure(n * 2, "global motion compensation field");
    if (rc) return rc;
    rc = s->gm_h.ensure((size_t)P * 8, "global motion compensation warps");
    if (rc) return rc;
    rc = dev_ensure_all("global motion compensation modes", { { s->gm_usable, (size_t)P }, { s->gm_mode, n } });
    if (rc) return rc;
    rc = dev_ensure_all("global motion compensation costs", { { s->gm_cost, n }, { s->gm_costs, n * 2 } });
    if (rc) return rc;
    // unusable warps are found here, before the launch: the kernels take a flag per pair
    std::vector<uint8_t> usable((size_t)P);
    for (int k = 0; k < P; ++k) usable[(size_t)k] = gmc_usable(h + (size_t)k * 8, s->H, s->W) ? 1 : 0;
    GME_HIP_TRY(hipMemcpyAsync(s->gm_h, h, (size_t)P * 8 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    GME_HIP_TRY(hipMemcpyAsync(s->gm_usable, usable.data(), (size_t)P, hipMemcpyHostToDevice, ctx->stream));
    const Plane& p = s->level[2];
    // the anchor of the search is the predicted frame k + fd; it is looked for in frame k
    BbmeJob job = bbme_job(p, fd, 0, P, bs, sw, procedure, pnorm, s->gm_f);
    job.cur = p.at(0);
    rc = seq_launch_bbme_from(s, 2, 0, job);
    if (rc) return rc;
    rc = launch_gmc(ctx, p.at(0), p.at(fd), p.stride, P, s->H, s->W, p.pitch, bs, pnorm, penalty, s->gm_h, s->gm_usable, s->gm_f, s->gm_mode,
                    s->gm_cost, s->gm_costs);
    if (rc) return rc;
    rc = ctx_finish(ctx);                                      // `usable` is read by its copy until here
    if (rc) return rc;
    s->gm_pairs = P; s->gm_h_blocks = hb; s->gm_w_blocks = wb; s->gm_fd = fd; s->gm_bs = bs;
    s->gm_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_gmc(gme_seq* s, int first, int count, int32_t* f_out, uint8_t* mode_out, int64_t* cost_out, int64_t* costs_out,
                                uint8_t* usable_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_gmc: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->gm_h_blocks * s->gm_w_blocks;
    return seq_read(s, "gme_seq_read_gmc", s->gm_valid, "gme_seq_gmc", "pairs", first, count, s->gm_pairs,
                    { { f_out, s->gm_f.get(), per * 2 * sizeof(int32_t) }, { mode_out, s->gm_mode.get(), per },
                      { cost_out, s->gm_cost.get(), per * sizeof(long long) }, { costs_out, s->gm_costs.get(), per * 2 * sizeof(long long) },
                      { usable_out, s->gm_usable.get(), 1 } });                  // one flag per pair, whatever the block grid
}

extern "C" int gme_seq_predict_gmc(gme_seq* s, int64_t* sse_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_predict_gmc: null sequence");
    gme_ctx* ctx = s->ctx;
    GME_ENTER(ctx);
    GME_REQUIRE(s->gm_valid, GME_ERR_STATE, "gme_seq_predict_gmc before gme_seq_gmc");
    const int P = s->gm_pairs, fd = s->gm_fd;
    GME_REQUIRE(P <= s->N - fd, GME_ERR_STATE, "gme_seq_predict_gmc: %d pairs, the sequence has %d", P, s->N - fd);
    const Plane& p = s->level[2];
    return seq_predict(s, fd, P, sse_out, [&] {
        return launch_predict_gmc(ctx, p.at(0), p.at(fd), p.stride, P, s->H, s->W, p.pitch, s->gm_bs, s->gm_h, s->gm_usable, s->gm_mode, s->gm_f,
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
    s->prop_valid = false;
    rc = dev_ensure_all("vector propagation fields", { { s->prop_work[0], n * 2 }, { s->prop_work[1], n * 2 } });
    if (rc) return rc;
    if (g) {
        rc = s->prop_g.ensure(n * 2, "camera field");
        if (rc) return rc;
    }
    rc = s->prop_cost.ensure(n, "vector propagation costs");
    if (rc) return rc;
    rc = s->prop_source.ensure(n, "vector propagation sources");
    if (rc) return rc;
    if (n == 0) {
        s->prop_valid = true;
        return GME_OK;
    }
    seq_field_replaced(s);
    if (g) GME_HIP_TRY(hipMemcpyAsync(s->prop_g, g, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const Plane& p = s->level[2];
    int32_t* const work[2] = { s->prop_work[0].get(), s->prop_work[1].get() };
    int32_t* result = nullptr;
    rc = launch_prop(ctx, p.at(0), p.at(fd), p.stride, P, s->H, s->W, p.pitch, bs, pnorm, rounds, steps, s->mv, temporal ? s->mv.get() : nullptr,
                     -1, g ? s->prop_g.get() : nullptr, work, s->prop_cost, s->prop_source, &result);
    if (rc) return rc;
    GME_HIP_TRY(hipMemcpyAsync(s->mv, result, n * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    rc = ctx_finish(ctx);                                      // `g` is read by its copy until here
    if (rc) return rc;
    s->prop_valid = true;
    return GME_OK;
}

extern "C" int gme_seq_read_prop(gme_seq* s, int first_pair, int count, int32_t* mf_out, int64_t* cost_out, uint8_t* source_out)
{
    GME_REQUIRE(s != nullptr, GME_ERR_ARG, "gme_seq_read_prop: null sequence");
    GME_ENTER(s->ctx);
    const size_t per = (size_t)s->mv_h * s->mv_w;
    return seq_read(s, "gme_seq_read_prop", s->prop_valid, "gme_seq_prop", "pairs", first_pair, count, s->mv_pairs,
                    { { mf_out, s->mv.get(), per * 2 * sizeof(int32_t) }, { cost_out, s->prop_cost.get(), per * sizeof(long long) },
                      { source_out, s->prop_source.get(), per } });
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
    GME_REQUIRE(unit == 4 || s->qmv_valid, GME_ERR_STATE, "gme_seq_obmc with the quarter-pel field before gme_seq_subpel");
    rc = subpel_field(s, "gme_seq_obmc", fd, bs);
    if (rc) return rc;
    GME_REQUIRE(first_pair >= 0 && count >= 0 && first_pair + count <= s->mv_pairs, GME_ERR_ARG, "gme_seq_obmc: pairs [%d, %d) outside [0, %d)",
                first_pair, first_pair + count, s->mv_pairs);
    const size_t per = (size_t)s->mv_h * s->mv_w, image = (size_t)s->H * s->W;
    const int32_t* field = unit == 4 ? s->mv.get() : s->qmv.get();
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
