// Second-order global motion models (roadmap.py: bilinear, pseudo-perspective, quadratic) for gfx950: the per-level
// robust fit with order-2 normal-equation sums, the order-2 model field, and the field the compensation reads.
//
// EXTENSION of motion.py:109-341 (the reference fits the affine part only; its parameter_projection docstring,
// motion.py:191-207, quotes the paper's second-order model).  Conventions ("Second-order models"):
//   basis      phi = [1, x, y, x^2, xy, y^2], x = 4 i (row), y = 4 j (column) as the fit sees them (motion.py:254-255)
//   params12   [a0 a1 a2 b0 b1 b2 | a3 a4 a5 b3 b4 b5]: the first six are the affine layout
//   field      d = ((p0 + p2 j) + p1 i) + ((a3 (i i) + a4 (i j)) + a5 (j j)) at the raw block indices (motion.py:139-157),
//              every product and sum rounded separately, round-half-even, int16 store wraps (model_component's rules):
//              with zero second-order terms this is the affine field bit for bit
//   sums27     the 15 moments sum w x^p y^q (p + q <= 4) in the order 1 x y x2 xy y2 x3 x2y xy2 y3 x4 x3y x2y2 xy3 y4,
//              then Sx[6] = sum w phi_k dx, Sy[6] = sum w phi_k dy -- each a sequential float64 sum over the inliers in
//              row-major order of terms (exact integer) * w, k_fit_level's discipline; so M[0..5], Sx[0..2], Sy[0..2] equal
//              k_fit_level's 15 affine sums bit for bit.
// The kernels of gme_kernels.hip are not touched: this file adds instances, it does not share code with them.
#include "gme_internal.h"

namespace {

__device__ __forceinline__ int16_t model2_component(double p0, double p1, double p2, double q0, double q1, double q2, int i, int j)
{
    const double di = (double)i, dj = (double)j;
    const double aff = __dadd_rn(__dadd_rn(p0, __dmul_rn(p2, dj)), __dmul_rn(p1, di));
    const double sec = __dadd_rn(__dadd_rn(__dmul_rn(q0, __dmul_rn(di, di)), __dmul_rn(q1, __dmul_rn(di, dj))), __dmul_rn(q2, __dmul_rn(dj, dj)));
    return (int16_t)(long long)rint(__dadd_rn(aff, sec));      // round-half-even, int16 store wraps
}

// The order-2 field of every pair: int16 for gme_model2_field, int32 (the int16 value, widened) for the mf32 path of
// k_compensate / k_compensate16.  params [P][12].
template <typename T>
__global__ void __launch_bounds__(256) k_model2_field(const double* params, int h, int w, T* out)
{
    const int n = h * w;
    const double* p = params + (long long)blockIdx.y * 12;
    T* o = out + (long long)blockIdx.y * n * 2;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int i = k / w, j = k - i * w;
    o[2 * k] = (T)model2_component(p[0], p[1], p[2], p[6], p[7], p[8], i, j);
    o[2 * k + 1] = (T)model2_component(p[3], p[4], p[5], p[9], p[10], p[11], i, j);
}

// ---------------------------------------------------------------------------
// motion.best_affine_parameters_robust minus BBME and solve (motion.py:232-279) for the order-2 models, one workgroup per
// pair.  Model field, threshold (radix select, `drop` as k_fit_level: drop < 0 = the unmasked fit), strict-> mask and the
// ordered inlier compaction are k_fit_level's steps with the order-2 field; params holds `pstride` doubles per pair (12, or
// 6 for the affine layout of k_project_first: second-order terms zero).
// ---------------------------------------------------------------------------
constexpr int FIT2_CHAINS = 27;
constexpr int FIT2_BATCH = 128;                // list entries per batch: 27 x 129 doubles of LDS beside a 40 KB inlier list
constexpr int FIT2_PITCH = FIT2_BATCH + 1;     // one double of padding: the 27 adding lanes read 27 different banks

__global__ void __launch_bounds__(256) k_fit_level2(const int32_t* gt_all, int h, int w, const double* params, int pstride,
                                                     int drop, double wgt, int16_t* model_all, uint8_t* mask_all,
                                                     int32_t* diff_all, int32_t* thr_all, double* sums_all, int4* list_all,
                                                     int list_lds)
{
    extern __shared__ int4 dyn_lds[];
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_rank;
    const int n = h * w;
    const int pair = blockIdx.x;
    const int32_t* gt = gt_all + (long long)pair * n * 2;
    int16_t* model = model_all + (long long)pair * n * 2;
    uint8_t* mask = mask_all + (long long)pair * n;
    int32_t* diff = diff_all + (long long)pair * n;
    const double* p = params + (long long)pair * pstride;
    const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4], p5 = p[5];
    const bool second = pstride >= 12;
    const double a3 = second ? p[6] : 0.0, a4 = second ? p[7] : 0.0, a5 = second ? p[8] : 0.0;
    const double b3 = second ? p[9] : 0.0, b4 = second ? p[10] : 0.0, b5 = second ? p[11] : 0.0;

    // model field and L1 difference (motion.py:232-239)
    for (int k = threadIdx.x; k < n; k += 256) {
        const int i = k / w, j = k - i * w;
        const int16_t m0 = model2_component(p0, p1, p2, a3, a4, a5, i, j), m1 = model2_component(p3, p4, p5, b3, b4, b5, i, j);
        model[2 * k] = m0; model[2 * k + 1] = m1;
        diff[k] = abs(gt[2 * k] - (int)m0) + abs(gt[2 * k + 1] - (int)m1);
    }
    // threshold = sorted(diff)[n - drop], or sorted(diff)[0] when drop == 0 (motion.py:240-243)
    if (threadIdx.x == 0) { sel_prefix = drop < 0 ? 0x7FFFFFFFu : 0u; sel_rank = drop <= 0 ? 0 : (unsigned)(n - drop); }
    __syncthreads();
    for (int shift = drop < 0 ? -1 : 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        const unsigned prefix = sel_prefix;
        const unsigned himask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int k = threadIdx.x; k < n; k += 256) {
            const unsigned v = (unsigned)diff[k];
            if ((v & himask) == prefix) atomicAdd(&hist[(v >> shift) & 255], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned rank = sel_rank, cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (rank < cum + hist[b]) break;
                cum += hist[b];
            }
            sel_rank = rank - cum;
            sel_prefix = prefix | ((unsigned)b << shift);
        }
        __syncthreads();
    }
    const int thr = (int)sel_prefix;
    if (threadIdx.x == 0) thr_all[pair] = thr;

    // mask (strict >, motion.py:244) and ordered compaction: entry e = the e-th inlier in row-major order, (4i, 4j, gt0, gt1)
    __shared__ int wave_count[4];
    __shared__ int list_base;
    int4* list = list_lds ? (int4*)dyn_lds : list_all + (long long)pair * n;
    if (threadIdx.x == 0) list_base = 0;
    __syncthreads();
    for (int k0 = 0; k0 < n; k0 += 256) {
        const int k = k0 + threadIdx.x;
        bool inl = false;
        if (k < n) {
            const bool out = diff[k] > thr;
            mask[k] = out;
            inl = !out;
        }
        const unsigned long long bal = __ballot(inl);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane == 0) wave_count[wv] = __popcll(bal);
        __syncthreads();
        int off = list_base;
        for (int q = 0; q < wv; ++q) off += wave_count[q];
        if (inl) {
            const int i = k / w, j = k - i * w;
            list[off + __popcll(bal & ((1ull << lane) - 1))] = make_int4(i * 4, j * 4, gt[2 * k], gt[2 * k + 1]);
        }
        __syncthreads();
        if (threadIdx.x == 0) list_base += wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
        __syncthreads();
    }
    const int m = list_base;

    // 27 sequential chains.  Per batch of 128 list entries the two halves of the workgroup form the terms (threads 0-127:
    // the 15 moments of entry t, threads 128-255: the 12 displacement terms of entry t - 128), then lanes 0-26 add them in
    // list order -- the serial depth of k_fit_level (m additions per chain), in half its LDS.
    __shared__ double terms[FIT2_CHAINS][FIT2_PITCH];
    double acc = 0.0;
    const int t = threadIdx.x & (FIT2_BATCH - 1), half = threadIdx.x >> 7;
    for (int e0 = 0; e0 < m; e0 += FIT2_BATCH) {
        const int e = e0 + t;
        if (e < m) {
            const int4 v = list[e];
            const double x = (double)v.x, y = (double)v.y;
            const double x2 = __dmul_rn(x, x), xy = __dmul_rn(x, y), y2 = __dmul_rn(y, y);      // exact integers
            if (half == 0) {
                const double mono[15] = { 1.0, x, y, x2, xy, y2, __dmul_rn(x2, x), __dmul_rn(x2, y), __dmul_rn(x, y2), __dmul_rn(y2, y),
                                          __dmul_rn(x2, x2), __dmul_rn(__dmul_rn(x2, x), y), __dmul_rn(x2, y2), __dmul_rn(x, __dmul_rn(y2, y)),
                                          __dmul_rn(y2, y2) };
#pragma unroll
                for (int c = 0; c < 15; ++c) terms[c][t] = __dmul_rn(mono[c], wgt);
            } else {
                const double phi[6] = { 1.0, x, y, x2, xy, y2 };
                const double g0 = (double)v.z, g1 = (double)v.w;
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    terms[15 + c][t] = __dmul_rn(__dmul_rn(phi[c], g0), wgt);
                    terms[21 + c][t] = __dmul_rn(__dmul_rn(phi[c], g1), wgt);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < FIT2_CHAINS) {
            const int cnt = min(FIT2_BATCH, m - e0);
            const double* tc = terms[threadIdx.x];
            for (int u = 0; u < cnt; ++u) acc = __dadd_rn(acc, tc[u]);
        }
        __syncthreads();
    }
    if (threadIdx.x < FIT2_CHAINS) sums_all[(long long)pair * FIT2_CHAINS + threadIdx.x] = acc;
}

}  // namespace

int launch_model2_field(gme_ctx* ctx, const double* params, int pairs, int h, int w, int16_t* out16, int32_t* out32)
{
    if (pairs == 0 || h * w == 0) return GME_OK;
    const int step = max_grid_planes();
    for (int first = 0; first < pairs; first += step) {
        const int n = pairs - first < step ? pairs - first : step;
        const dim3 grid((h * w + 255) / 256, n);
        if (out16)
            hipLaunchKernelGGL(k_model2_field<int16_t>, grid, dim3(256), 0, ctx->stream, params + (size_t)first * 12, h, w,
                               out16 + (size_t)first * h * w * 2);
        else
            hipLaunchKernelGGL(k_model2_field<int32_t>, grid, dim3(256), 0, ctx->stream, params + (size_t)first * 12, h, w,
                               out32 + (size_t)first * h * w * 2);
    }
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}

int launch_fit_level2(gme_ctx* ctx, const int32_t* gt, int pairs, int h, int w, const double* params, int pstride, int drop,
                      int level_H, int level_W, int16_t* model, uint8_t* mask, int32_t* diff, int32_t* thr, double* sums27,
                      void* list)
{
    if (pairs == 0) return GME_OK;
    const double wgt = 1.0 / ((double)level_H * (double)level_W);      // motion.py:250
    // inlier list: LDS when it fits beside a second resident workgroup (k_fit_level's rule), else the global buffer
    const size_t need = (size_t)h * w * sizeof(int4);
    const int in_lds = need <= 40 * 1024;
    hipLaunchKernelGGL(k_fit_level2, dim3(pairs), dim3(256), in_lds ? need : 0, ctx->stream, gt, h, w, params, pstride, drop, wgt,
                       model, mask, diff, thr, sums27, (int4*)list, in_lds);
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}
