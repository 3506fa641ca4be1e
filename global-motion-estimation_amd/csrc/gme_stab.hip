// Video stabilization (host definition: stabilize.py).  The camera path and its smoothing are a
// little float64 host math; what runs here is the per-frame warp of every frame of the video and the squared error of
// consecutive frames the inter-frame fidelity (ITF) is computed from.
//
// Kernels:
//   k_warp_frames  out frame t = frames[t] warped by W_t (one float64[8] per frame, uniform per workgroup): bilinear
//                  sample where the sample point lies in the frame, the fill value or the clamped point elsewhere; valid
//                  samples counted per frame
//   k_frame_sse    exact sum of squared differences of consecutive frames of a plane stack
#include "gme_passes.h"
#include "gme_warp.h"

namespace {

constexpr int STAB_PX = 4;                                      // output pixels per lane: one 32-bit store
constexpr int STAB_ROWS = 4;                                    // rows per workgroup: one wave per row
constexpr int STAB_THREADS = 64 * STAB_ROWS;
constexpr int STAB_COLS = 64 * STAB_PX;                         // columns per workgroup
constexpr int SSE_THREADS = 256;
constexpr int SSE_WORDS_PER_THREAD = 4;                         // 16-byte words per thread and frame (grid-stride)

// grid (ceil(W / STAB_COLS), ceil(H / STAB_ROWS), frames).  The per-pixel float64 arithmetic is direct.warp's, evaluated
// afresh at every pixel (stepping the numerator and denominator along the row would round differently from the host
// definition).  Lanes whose four pixels start inside the row store all four at once; pixels at or past W are written as
// zero, the plane's padding (pitch is a multiple of 64, so the store stays inside the row).
__global__ void __launch_bounds__(STAB_THREADS) k_warp_frames(const uint8_t* src, long long stride, int pitch, int H, int W,
                                                              const double* params, uint8_t* out, long long out_stride,
                                                              int out_pitch, int border, int fill, unsigned long long* valid)
{
    const int f = blockIdx.z, lane = threadIdx.x & 63;
    const int v = blockIdx.y * STAB_ROWS + (threadIdx.x >> 6);
    const int u0 = blockIdx.x * STAB_COLS + lane * STAB_PX;
    unsigned n = 0;
    if (v < H && u0 < W) {
        double h[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = params[(long long)f * 8 + k];
        const uint8_t* p = src + (long long)f * stride;
        const double dv = (double)v, wm = (double)(W - 1), hm = (double)(H - 1);
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < STAB_PX; ++k) {
            const int u = u0 + k;
            if (u >= W) break;
            Sample sm = warp_at(h, (double)u, dv);
            int o = fill;
            if (inside(sm, H, W)) {
                ++n;
                o = (int)floor(__dadd_rn(sample(p, pitch, taps_at(sm, H, W)), 0.5));
            } else if (border == 1) {                            // replicate: the point clamped into the frame (NaN -> 0)
                sm.up = sm.up > 0.0 ? (sm.up < wm ? sm.up : wm) : 0.0;
                sm.vp = sm.vp > 0.0 ? (sm.vp < hm ? sm.vp : hm) : 0.0;
                o = (int)floor(__dadd_rn(sample(p, pitch, taps_at(sm, H, W)), 0.5));
            }
            packed |= (uint32_t)o << (8 * k);
        }
        *(uint32_t*)(out + (long long)f * out_stride + (long long)v * out_pitch + u0) = packed;
    }
    const uint32_t total = wave_sum_u32(n);
    if (lane == 0 && total) atomicAdd(&valid[f], (unsigned long long)total);
}

__device__ __forceinline__ uint32_t sq_diff4(uint32_t a, uint32_t b)
{
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = (int)((a >> (8 * k)) & 0xFF) - (int)((b >> (8 * k)) & 0xFF);
        s += (uint32_t)(d * d);
    }
    return s;
}

// sse[k] += sum over the plane of (frame k + 1 - frame k)^2; grid (blocks, pairs).  A plane is `words` 16-byte words (pitch
// times H bytes, pitch a multiple of 64); the padding bytes are zero in every plane, so whole rows are read unmasked.
__global__ void __launch_bounds__(SSE_THREADS) k_frame_sse(const uint8_t* frames, long long stride, long long words,
                                                           unsigned long long* sse)
{
    const int k = blockIdx.y;
    const uint4* a = (const uint4*)(frames + (long long)k * stride);
    const uint4* b = (const uint4*)(frames + (long long)(k + 1) * stride);
    unsigned long long acc = 0;
    for (long long i = (long long)blockIdx.x * SSE_THREADS + threadIdx.x; i < words; i += (long long)gridDim.x * SSE_THREADS) {
        const uint4 x = a[i], y = b[i];
        acc += sq_diff4(x.x, y.x) + sq_diff4(x.y, y.y) + sq_diff4(x.z, y.z) + sq_diff4(x.w, y.w);
    }
    for (int m = 32; m > 0; m >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, m, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&sse[k], acc);
}

}  // namespace

// ---- launchers --------------------------------------------------------------------------------------------------------
// frames first .. first + count - 1 of src warped by params[count][8] (device) into the same frames of dst; valid[count]
// (device) receives the number of in-frame samples per frame
int launch_warp_frames(gme_ctx* ctx, const Plane& src, const Plane& dst, int first, int count, const double* params, int border,
                       int fill, unsigned long long* valid)
{
    if (count == 0) return GME_OK;
    GME_HIP_TRY(hipMemsetAsync(valid, 0, sizeof(unsigned long long) * count, ctx->stream));
    const int step = max_grid_planes();
    for (int k = 0; k < count; k += step) {
        const int n = count - k < step ? count - k : step;
        const dim3 grid((src.W + STAB_COLS - 1) / STAB_COLS, (src.H + STAB_ROWS - 1) / STAB_ROWS, n);
        hipLaunchKernelGGL(k_warp_frames, grid, dim3(STAB_THREADS), 0, ctx->stream, src.at(first + k), (long long)src.stride,
                           src.pitch, src.H, src.W, params + (size_t)k * 8, dst.at(first + k), (long long)dst.stride, dst.pitch,
                           border, fill, valid + k);
    }
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}

// sse[k] = sum (p[first + k + 1] - p[first + k])^2 for k < count (device)
int launch_frame_sse(gme_ctx* ctx, const Plane& p, int first, int count, unsigned long long* sse)
{
    if (count == 0) return GME_OK;
    GME_HIP_TRY(hipMemsetAsync(sse, 0, sizeof(unsigned long long) * count, ctx->stream));
    const long long words = (long long)p.pitch * p.H / 16;
    const long long per_block = (long long)SSE_THREADS * SSE_WORDS_PER_THREAD;
    const unsigned blocks = (unsigned)((words + per_block - 1) / per_block);
    const int step = max_grid_planes();
    for (int k = 0; k < count; k += step) {
        const int n = count - k < step ? count - k : step;
        hipLaunchKernelGGL(k_frame_sse, dim3(blocks, n), dim3(SSE_THREADS), 0, ctx->stream, p.at(first + k), (long long)p.stride,
                           words, sse + k);
    }
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}
