// Background mosaic and moving-object masks from the camera path (host definition: mosaic.py).  The
// path, the canvas and the per-frame warps are float64 host math; what runs here is the sampling of every frame at every
// canvas pixel with the per-pixel lower median of the samples, and the per-frame comparison against that background.
//
// Kernels:
//   k_mosaic_median  one lane per canvas pixel, one wave per workgroup (64 pixels of one canvas row): frame t sampled at
//                    direct.warp(G_t, x + ox, y + oy) where that point lies in the frame, the rounded samples counted in a
//                    256-bin histogram per pixel in LDS, then a walk to rank (count - 1) / 2
//   k_moving_mask    frame t against the sprite sampled at direct.warp(A_t, u, v) - (ox, oy): residuals of a tile and its
//                    one-pixel halo staged in LDS, the 3x3 rule, known and moving pixels counted per frame
#include "gme_passes.h"
#include "gme_warp.h"

namespace {

constexpr int MED_LANES = 64;                                   // one wave: the histogram columns are lane-private
constexpr int MED_WORDS = 128;                                  // 256 bins of 16 bits, two to a word
constexpr double CULL_RANGE = 0x1p20;                           // see segment_misses

constexpr int MASK_COLS = 64, MASK_ROWS = 16;                   // output tile of a workgroup: four rows per wave
constexpr int MASK_THREADS = 256;
constexpr int MASK_TW = MASK_COLS + 2, MASK_TH = MASK_ROWS + 2; // the tile with its halo

// The cull of k_mosaic_median: true only where NO pixel of the canvas segment (xa .. xb, y) can sample the frame through h.
// Along the segment numerators and denominator of the warp are affine in x, so where d > 0 at both ends it is positive in
// between, and u' < -1 (u' > W, and the same for v') at both ends holds in between: the one-pixel guard band around the
// frame, [-1, W] x [-1, H] instead of [0, W-1] x [0, H-1], is what rounding may not cross.  It cannot where the terms of the
// sums stay below 2^20 times d (their rounding errors, a few 2^-53 of the terms, then move u' and v' by less than 2^-10); a
// warp beyond that, d <= 0 at an end or a NaN anywhere answers false, and the frame is sampled pixel by pixel.
__device__ __forceinline__ bool segment_misses(const double* h, double xa, double xb, double y, int H, int W)
{
    const Sample a = warp_at(h, xa, y), b = warp_at(h, xb, y);
    const double mx = fmax(fabs(xa), fabs(xb)), my = fabs(y);
    const double md = fabs(h[6]) * mx + fabs(h[7]) * my + 1.0;
    const double mu = fabs(h[0]) * mx + fabs(h[1]) * my + fabs(h[2]);
    const double mv = fabs(h[3]) * mx + fabs(h[4]) * my + fabs(h[5]);
    const double lim = fmin(a.d, b.d) * CULL_RANGE;             // fmin drops a NaN, the comparisons below do not pass one
    if (!(a.d > 0.0 && b.d > 0.0 && md < lim && mu < lim && mv < lim)) return false;
    const double wg = (double)W, hg = (double)H;
    return (a.up < -1.0 && b.up < -1.0) || (a.up > wg && b.up > wg) || (a.vp < -1.0 && b.vp < -1.0) || (a.vp > hg && b.vp > hg);
}

// grid (tiles_x * Hc), one wave each.  hist word w of lane l (bins 2w and 2w + 1 in its halves) lies at hist[w * 64 + l]:
// lane-minor, so a wave's 64 increments fall on 64 different banks whatever the sample values are, and a pixel's count
// (<= 65535 frames) cannot carry from one half into the other.  Frames are taken 64 at a time: lane i tests frame base + i
// against the segment (usable, and not culled), the ballot of the survivors is scalar, and the wave then samples them one
// by one with G_t uniform.  The float64 arithmetic per sample is direct.warp / direct.bilinear (gme_warp.h).
__global__ void __launch_bounds__(MED_LANES) k_mosaic_median(const uint8_t* src, long long stride, int pitch, int H, int W,
                                                             int count, const double* G, const uint8_t* usable, int ox, int oy,
                                                             int Wc, int tiles_x, int fill, int cull, uint8_t* sprite,
                                                             uint16_t* cnt, int out_pitch)
{
    __shared__ uint32_t hist[MED_WORDS * MED_LANES];
    const int lane = threadIdx.x;
    const int y = (int)(blockIdx.x / (unsigned)tiles_x), x0 = (int)(blockIdx.x % (unsigned)tiles_x) * MED_LANES, x = x0 + lane;
#pragma unroll 8
    for (int w = 0; w < MED_WORDS; ++w) hist[w * MED_LANES + lane] = 0;
    const double cx = (double)((long long)x + ox), cy = (double)((long long)y + oy);
    const double xa = (double)((long long)x0 + ox), xb = (double)((long long)min(x0 + MED_LANES - 1, Wc - 1) + ox);
    unsigned n = 0;
    for (int base = 0; base < count; base += MED_LANES) {
        const int t = base + lane;
        bool live = t < count && usable[t] != 0;
        if (live && cull) live = !segment_misses(G + (long long)t * 8, xa, xb, cy, H, W);
        unsigned long long todo = __ballot(live);
        while (todo) {
            const int k = base + __ffsll(todo) - 1;
            todo &= todo - 1;
            if (x < Wc) {
                const Sample sm = warp_at(G + (long long)k * 8, cx, cy);
                if (inside(sm, H, W)) {
                    int val = (int)floor(__dadd_rn(sample(src + (long long)k * stride, pitch, taps_at(sm, H, W)), 0.5));
                    val = min(max(val, 0), 255);                  // a blend of bytes is in range; the histogram index must be
                    atomicAdd(&hist[(val >> 1) * MED_LANES + lane], 1u << ((val & 1) * 16));     // one ds_add; no lane shares it
                    ++n;
                }
            }
        }
    }
    if (x >= Wc) return;
    int med = fill;
    if (n) {
        const unsigned rank = (n - 1) >> 1;
        unsigned below = 0;
        med = -1;
        for (int w = 0; w < MED_WORDS; ++w) {
            const uint32_t word = hist[w * MED_LANES + lane];
            const unsigned lo = word & 0xFFFFu, both = lo + (word >> 16);
            if (med < 0 && below + both > rank) med = 2 * w + (below + lo > rank ? 0 : 1);
            below += both;
        }
    }
    sprite[(long long)y * out_pitch + x] = (uint8_t)med;
    cnt[(long long)y * out_pitch + x] = (uint16_t)n;
}

// |frame - background| at frame pixel (u, v) of a usable frame, -1 where the background is not known there: the canvas
// point outside the canvas, or one of its four taps (the far tap clamped as direct.py does) built from fewer than min_count
// samples
__device__ __forceinline__ int residual_at(const uint8_t* frame, int pitch, const double* h, int u, int v, const uint8_t* sprite,
                                           const uint16_t* cnt, int sp_pitch, int Hc, int Wc, double fox, double foy, int min_count)
{
    Sample sm = warp_at(h, (double)u, (double)v);
    sm.up = __dsub_rn(sm.up, fox);
    sm.vp = __dsub_rn(sm.vp, foy);
    if (!inside(sm, Hc, Wc)) return -1;
    const Taps t = taps_at(sm, Hc, Wc);
    const long long r0 = (long long)t.y0 * sp_pitch, r1 = (long long)t.y1 * sp_pitch;
    if ((int)cnt[r0 + t.x0] < min_count || (int)cnt[r0 + t.x1] < min_count || (int)cnt[r1 + t.x0] < min_count ||
        (int)cnt[r1 + t.x1] < min_count)
        return -1;
    const int b = (int)floor(__dadd_rn(sample(sprite, sp_pitch, t), 0.5));
    return abs((int)frame[(long long)v * pitch + u] - b);
}

// grid (ceil(W / 64), ceil(H / 16), frames).  The residuals of the tile and of the one-pixel ring around it (-1 outside the
// frame) are computed once each into LDS, 66 x 18 of them by 256 threads; every thread then sums the known residuals of the
// 3x3 neighbourhoods of its four output pixels (rows r, r + 4, r + 8, r + 12 of its column) and writes their mask bytes.
__global__ void __launch_bounds__(MASK_THREADS) k_moving_mask(const uint8_t* src, long long stride, int pitch, int H, int W,
                                                              const double* A, const uint8_t* usable, const uint8_t* sprite,
                                                              const uint16_t* cnt, int sp_pitch, int Hc, int Wc, int ox, int oy, int threshold,
                                                              int min_count, uint8_t* out, long long out_stride, int out_pitch,
                                                              unsigned long long* known, unsigned long long* moving)
{
    __shared__ short res[MASK_TH * MASK_TW];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int u0 = blockIdx.x * MASK_COLS, v0 = blockIdx.y * MASK_ROWS;
    const uint8_t* frame = src + (long long)f * stride;
    const double* h = A + (long long)f * 8;
    const double fox = (double)ox, foy = (double)oy;
    const bool use = usable[f] != 0;                             // an unusable frame: nothing known, an all-zero mask
    for (int i = tid; i < MASK_TH * MASK_TW; i += MASK_THREADS) {
        const int u = u0 - 1 + i % MASK_TW, v = v0 - 1 + i / MASK_TW;
        int r = -1;
        if (use && u >= 0 && u < W && v >= 0 && v < H)
            r = residual_at(frame, pitch, h, u, v, sprite, cnt, sp_pitch, Hc, Wc, fox, foy, min_count);
        res[i] = (short)r;
    }
    __syncthreads();
    const int c = tid & 63, u = u0 + c;
    unsigned n_known = 0, n_moving = 0;
    if (u < W) {
#pragma unroll
        for (int q = 0; q < MASK_ROWS / 4; ++q) {
            const int r = (tid >> 6) + 4 * q, v = v0 + r;
            if (v >= H) break;
            int sum = 0, n = 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int e = res[(r + dy) * MASK_TW + c + dx];
                    if (e >= 0) { sum += e; ++n; }
                }
            const bool is_known = res[(r + 1) * MASK_TW + c + 1] >= 0;
            const bool m = is_known && sum > threshold * n;
            n_known += is_known;
            n_moving += m;
            out[(long long)f * out_stride + (long long)v * out_pitch + u] = (uint8_t)m;
        }
    }
    const uint32_t tk = wave_sum_u32(n_known), tm = wave_sum_u32(n_moving);
    if (c == 0 && tk) atomicAdd(&known[f], (unsigned long long)tk);
    if (c == 0 && tm) atomicAdd(&moving[f], (unsigned long long)tm);
}

}  // namespace

// ---- launchers --------------------------------------------------------------------------------------------------------
// sprite / cnt [Hc][out_pitch] = lower median / number of the in-frame samples of frames first .. first + count - 1 of src at
// every canvas pixel; G[count][8] and usable[count] on the device
int launch_mosaic_median(gme_ctx* ctx, const Plane& src, int first, int count, const double* G, const uint8_t* usable, int ox,
                         int oy, int Hc, int Wc, int fill, int cull, uint8_t* sprite, uint16_t* cnt, int out_pitch)
{
    const int tiles_x = (Wc + MED_LANES - 1) / MED_LANES;
    hipLaunchKernelGGL(k_mosaic_median, dim3((unsigned)tiles_x * (unsigned)Hc), dim3(MED_LANES), 0, ctx->stream, src.at(first),
                       (long long)src.stride, src.pitch, src.H, src.W, count, G, usable, ox, oy, Wc, tiles_x, fill, cull, sprite,
                       cnt, out_pitch);
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}

// masks of frames first .. first + count - 1 into dst, their known and moving pixels into known[count] and moving[count]
// (device, zeroed by the caller); A[count][8] and usable[count] on the device
int launch_moving_masks(gme_ctx* ctx, const Plane& src, const Plane& dst, int first, int count, const double* A,
                        const uint8_t* usable, const uint8_t* sprite, const uint16_t* cnt, int sp_pitch, int Hc, int Wc, int ox, int oy, int threshold,
                        int min_count, unsigned long long* known, unsigned long long* moving)
{
    if (count == 0) return GME_OK;
    const int step = max_grid_planes();
    for (int k = 0; k < count; k += step) {
        const int n = count - k < step ? count - k : step;
        const dim3 grid((src.W + MASK_COLS - 1) / MASK_COLS, (src.H + MASK_ROWS - 1) / MASK_ROWS, n);
        hipLaunchKernelGGL(k_moving_mask, grid, dim3(MASK_THREADS), 0, ctx->stream, src.at(first + k), (long long)src.stride,
                           src.pitch, src.H, src.W, A + (size_t)k * 8, usable + k, sprite, cnt, sp_pitch, Hc, Wc, ox, oy, threshold, min_count,
                           dst.at(first + k), (long long)dst.stride, dst.pitch, known + k, moving + k);
    }
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}
