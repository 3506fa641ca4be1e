// Full-frame stabilization (host definition: stabilize.warp_fill).  Where the corrected view of frame t
// leaves frame t, the pixel comes from the first of an ordered list of candidate frames whose own warp lands inside it; what
// no candidate reaches follows the border rule of k_warp_frames (gme_stab.hip) for candidate 0.
//
// The kernel lives in a translation unit of its own so that gme_stab.hip compiles to exactly what it did before.
//
// Kernels:
//   k_warp_fill   out frame t, pixel (u, v) = the first candidate j < n with sources[t][j] >= 0 whose sample point
//                 direct.warp(warps[t][j], u, v) lies in frame sources[t][j], sampled bilinearly; the winning j (255: none)
//                 per pixel where asked for; pixels won by candidate 0 and by a later one counted per frame
#include "gme_passes.h"
#include "gme_warp.h"

namespace {

// k_warp_frames' geometry (gme_stab.hip)
constexpr int FILL_PX = 4;                                      // output pixels per lane: one 32-bit store
constexpr int FILL_ROWS = 4;                                    // rows per workgroup: one wave per row
constexpr int FILL_THREADS = 64 * FILL_ROWS;
constexpr int FILL_COLS = 64 * FILL_PX;                         // columns per workgroup
constexpr uint32_t FILL_NONE = 255;                             // `source` of a pixel no candidate reaches

// grid (ceil(W / FILL_COLS), ceil(H / FILL_ROWS), output frames).  `src` is plane 0 of the resident frames: the candidates
// are absolute frame indices.  `sources` and `params` start at the launch's first output frame.  Candidate j's index and
// warp depend on blockIdx.z and j alone, so they come through scalar loads and stay in SGPRs; the loop over j is uniform
// per wave and ends once no lane of the wave has an unresolved pixel, so a row that candidate 0 covers costs what it costs
// k_warp_frames.  The per-pixel arithmetic is gme_warp.h's, evaluated afresh per pixel and candidate.
__global__ void __launch_bounds__(FILL_THREADS) k_warp_fill(const uint8_t* __restrict__ src, long long stride, int pitch, int H, int W,
                                                            const int* __restrict__ sources, const double* __restrict__ params, int n_cand,
                                                            uint8_t* __restrict__ out, uint8_t* __restrict__ who_out, long long out_stride,
                                                            int out_pitch, int border, int fill, unsigned long long* valid,
                                                            unsigned long long* filled)
{
    __shared__ uint32_t part[FILL_ROWS][2];
    const int f = blockIdx.z, lane = threadIdx.x & 63, row = threadIdx.x >> 6;
    const int v = blockIdx.y * FILL_ROWS + row;
    const int u0 = blockIdx.x * FILL_COLS + lane * FILL_PX;
    const bool live = v < H && u0 < W;
    const uint32_t want = live ? (W - u0 >= FILL_PX ? 0xFu : (1u << (W - u0)) - 1u) : 0u;     // this lane's pixels inside the row
    const double dv = (double)v;
    const int* cand = sources + (long long)f * n_cand;
    const double* warps = params + (long long)f * n_cand * 8;
    uint32_t done = 0;                                           // 4-bit mask: pixels a candidate has given
    uint32_t packed = 0, who = 0;
    unsigned n0 = 0, n1 = 0;                                     // pixels won by candidate 0 / by a later one
#pragma unroll
    for (int k = 0; k < FILL_PX; ++k)
        if (want >> k & 1) who |= FILL_NONE << (8 * k);
    for (int j = 0; j < n_cand; ++j) {
        if (__ballot(done != want) == 0) break;
        const int s = cand[j];
        if (s < 0) continue;
        double h[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = warps[j * 8 + k];
        const uint8_t* p = src + (long long)s * stride;
        if (done != want) {
            unsigned won = 0;
#pragma unroll
            for (int k = 0; k < FILL_PX; ++k) {
                if (!((want & ~done) >> k & 1)) continue;
                const Sample sm = warp_at(h, (double)(u0 + k), dv);
                if (inside(sm, H, W)) {
                    const int o = (int)floor(__dadd_rn(sample(p, pitch, taps_at(sm, H, W)), 0.5));
                    packed |= (uint32_t)o << (8 * k);
                    who = (who & ~(0xFFu << (8 * k))) | (uint32_t)j << (8 * k);
                    done |= 1u << k;
                    ++won;
                }
            }
            if (j == 0) n0 += won;
            else n1 += won;
        }
    }
    if (__ballot(done != want) != 0) {                           // what no candidate reached: the border rule on candidate 0
        if (border == 1) {                                       // replicate: the point clamped into the frame (NaN -> 0)
            double h[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) h[k] = warps[k];
            const uint8_t* p = src + (long long)cand[0] * stride;
            const double wm = (double)(W - 1), hm = (double)(H - 1);
            if (done != want) {
#pragma unroll
                for (int k = 0; k < FILL_PX; ++k) {
                    if (!((want & ~done) >> k & 1)) continue;
                    Sample sm = warp_at(h, (double)(u0 + k), dv);
                    sm.up = sm.up > 0.0 ? (sm.up < wm ? sm.up : wm) : 0.0;
                    sm.vp = sm.vp > 0.0 ? (sm.vp < hm ? sm.vp : hm) : 0.0;
                    packed |= (uint32_t)(int)floor(__dadd_rn(sample(p, pitch, taps_at(sm, H, W)), 0.5)) << (8 * k);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < FILL_PX; ++k)
                if ((want & ~done) >> k & 1) packed |= (uint32_t)fill << (8 * k);
        }
    }
    if (live) {
        const long long at = (long long)f * out_stride + (long long)v * out_pitch + u0;
        *(uint32_t*)(out + at) = packed;
        if (who_out) *(uint32_t*)(who_out + at) = who;
    }
    // per wave, then per workgroup through LDS: at most one atomic per counter and workgroup, none for a zero
    const uint32_t t0 = wave_sum_u32(n0), t1 = wave_sum_u32(n1);
    if (lane == 0) {
        part[row][0] = t0;
        part[row][1] = t1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t total = 0;
#pragma unroll
        for (int r = 0; r < FILL_ROWS; ++r) total += part[r][threadIdx.x];
        if (total) atomicAdd(threadIdx.x == 0 ? &valid[f] : &filled[f], (unsigned long long)total);
    }
}

}  // namespace

// ---- launcher -----------------------------------------------------------------------------------------------------------
// output frames 0 .. count - 1 of dst (and of who, where who.ptr is set: the same geometry) from the resident frames src;
// sources[count][n_cand], params[count][n_cand][8], valid[count] and filled[count] on the device.  Every source index is a
// frame of src or -1, and sources[k][0] is a frame: the caller has checked.
int launch_warp_fill(gme_ctx* ctx, const Plane& src, const Plane& dst, const Plane& who, int count, int n_cand, const int* sources,
                     const double* params, int border, int fill, unsigned long long* valid, unsigned long long* filled)
{
    if (count == 0) return GME_OK;
    GME_HIP_TRY(hipMemsetAsync(valid, 0, sizeof(unsigned long long) * count, ctx->stream));
    GME_HIP_TRY(hipMemsetAsync(filled, 0, sizeof(unsigned long long) * count, ctx->stream));
    const int step = max_grid_planes();
    for (int k = 0; k < count; k += step) {
        const int n = count - k < step ? count - k : step;
        const dim3 grid((src.W + FILL_COLS - 1) / FILL_COLS, (src.H + FILL_ROWS - 1) / FILL_ROWS, n);
        hipLaunchKernelGGL(k_warp_fill, grid, dim3(FILL_THREADS), 0, ctx->stream, src.ptr, (long long)src.stride, src.pitch, src.H, src.W,
                           sources + (size_t)k * n_cand, params + (size_t)k * n_cand * 8, n_cand, dst.at(k), who.ptr ? who.at(k) : nullptr,
                           (long long)dst.stride, dst.pitch, border, fill, valid + k, filled + k);
    }
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}
