// Global motion compensation (host definition: gmc.py).  A block of the frame `cur` is predicted from the
// frame `ref` either by the camera warp of the pair, pixel by pixel (mode 0, GLOBAL: direct.compensate's pixel), or by the block
// of `ref` its own integer vector points at (mode 1, LOCAL), whichever costs less, the local one carrying a penalty; a block
// with neither predictor gets mode 2.  The warp arithmetic is that of gme_warp.h, one rounding per operation in direct.py's
// order, so the device equals gmc.decide and gmc.predict byte for byte.
//
// Kernels:
//   k_gmc<BS>        one wave per block, four blocks to a 256-thread workgroup, each wave on its own LDS slice (no workgroup
//                    barrier).  The wave stages the BS x BS block of `cur` and the block of `ref` at the vector (stage_bytes), then
//                    sweeps the block's (row, dword) pairs over its lanes once: the local cost takes the two staged dwords, the
//                    global cost warps the dword's four pixels, samples `ref` straight from memory (the footprint of a block under
//                    a camera warp is a few rows of a few cache lines, and every tap is reused by the neighbouring pixels of the
//                    same wave; see DESIGN.md 7i for why it is not staged), rounds and packs them, and both go through the
//                    row-wise v_sad_u8 / v_dot4 forms of k_bipred.  Availability of the global candidate is a wave-wide AND, the
//                    costs are wave sums, lane 0 decides.  Where h6 = h7 = 0 the denominator is exactly 1.0 and x / 1.0 = x, so
//                    a wave-uniform branch skips the two divisions.  <16> and <32> are compiled; <0> takes the block size at run
//                    time (and rows that are no multiple of four bytes).
//   k_predict_gmc    gmc.predict, one wave per block-sized cell of the frame (the cells beyond the last whole block included),
//                    mode and vector read once per cell; the squared error against `cur` is summed per workgroup and added with
//                    one integer atomic.
#include "bbme_predict.h"
#include "bbme_wave_lds.h"
#include "gme_passes.h"
#include "gme_warp.h"

namespace {

constexpr int GM_MIN_BS = 4, GM_MAX_BS = 64, GM_MAX_PENALTY = 1 << 30;
constexpr long long GM_MAX_COST = (long long)GM_MAX_BS * GM_MAX_BS * 65025ll;
static_assert(GM_MAX_COST < (long long)NO_COST, "a cost in 32 bits, below the sentinel");
static_assert((long long)GM_MAX_PENALTY + GM_MAX_COST < (1ll << 31), "31-bit decisions");
static_assert(small_div_covers(GM_MAX_BS, row_dwords(GM_MAX_BS)), "range of small_div");
static_assert(BLK_WAVES * 2 * block_bytes(GM_MAX_BS) <= 64 * 1024, "LDS of a workgroup");
// the squared error of a workgroup of k_predict_gmc in 32 bits
static_assert((long long)BLK_WAVES * GM_MAX_COST < (1ll << 32), "a workgroup's squared error");

struct GmcArgs {
    const uint8_t* ref;           // first plane of each role; pair k reads the planes k * stride bytes on
    const uint8_t* cur;
    long long stride;
    int H, W, pitch;
    const double* h;              // [pairs][8]
    const uint8_t* usable;        // [pairs]: gmc.usable of h[k], found on the host
    const int32_t* f;             // [pairs][hb][wb][2]
    uint8_t* mode;                // [pairs][hb][wb]
    long long* cost;              // [pairs][hb][wb]
    long long* costs;             // [pairs][hb][wb][2]
    int hb, wb, bs, pnorm;
    uint32_t penalty;
    int block_bytes;              // LDS of a wave: the block of cur, then the block of ref at the vector
};

// warp_at where the caller knows h6 = h7 = 0: d = (0 u + 0 v) + 1 is exactly 1.0 and a quotient by 1.0 is its dividend
__device__ __forceinline__ Sample warp_px(const double* h, bool affine, double u, double v)
{
    if (!affine) return warp_at(h, u, v);
    Sample s;
    s.d = 1.0;
    s.up = __dadd_rn(__dadd_rn(__dmul_rn(h[0], u), __dmul_rn(h[1], v)), h[2]);
    s.vp = __dadd_rn(__dadd_rn(__dmul_rn(h[3], u), __dmul_rn(h[4], v)), h[5]);
    return s;
}

// the global predictor pixel of an in-frame sample point: k_compensate_proj's rounding
__device__ __forceinline__ uint32_t global_px(const uint8_t* p, int pitch, const Sample& s, int H, int W)
{
    return (uint32_t)(int)floor(__dadd_rn(sample(p, pitch, taps_at(s, H, W)), 0.5));
}

template <int BS>
__global__ void __launch_bounds__(BLK_THREADS) k_gmc(const GmcArgs A)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const WaveBlock w = wave_block(A.wb);
    if (w.none) return;
    const int wave = w.wave, lane = w.lane, bj = w.bj, bi = w.bi, pair = w.z;
    const int B = BS ? BS : A.bs;
    const int pnorm = A.pnorm;
    const long long blk = ((long long)pair * A.hb + bi) * A.wb + bj;
    const int fx = __builtin_amdgcn_readfirstlane(A.f[blk * 2]), fy = __builtin_amdgcn_readfirstlane(A.f[blk * 2 + 1]);
    const int x0 = bj * B, y0 = bi * B;
    const long long rxl = (long long)x0 + fx, ryl = (long long)y0 + fy;
    const bool local = rxl >= 0 && ryl >= 0 && rxl + B <= A.W && ryl + B <= A.H;
    const bool usable = __builtin_amdgcn_readfirstlane((int)A.usable[pair]) != 0;
    if (!local && !usable) {                                     // nothing to predict from
        if (lane == 0) {
            A.mode[blk] = 2;
            A.cost[blk] = -1;
            A.costs[blk * 2] = -1; A.costs[blk * 2 + 1] = -1;
        }
        return;
    }
    uint32_t* anc = (uint32_t*)(lds + (size_t)wave * 2 * A.block_bytes);
    uint32_t* loc = (uint32_t*)(lds + (size_t)wave * 2 * A.block_bytes + A.block_bytes);
    const int nd = row_dwords(B);
    const uint8_t* ref = A.ref + (long long)pair * A.stride;
    // both blocks start at their first byte and bytes at and past column B are zero: dword t of one lies over dword t of the other
    stage_bytes(anc, B, nd, B, A.cur + (long long)pair * A.stride, A.pitch, A.H, A.W, y0, x0, lane);
    if (local) stage_bytes(loc, B, nd, B, ref, A.pitch, A.H, A.W, (int)ryl, (int)rxl, lane);
    wave_lds_fence();

    double h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = A.h[(long long)pair * 8 + k];
    const bool affine = usable && h[6] == 0.0 && h[7] == 0.0;    // wave-uniform: h is the pair's
    RowScore sl, sg;
    bool ok = true;                                              // every global pixel of this lane exists so far
    for (int t = lane; t < B * nd; t += 64) {
        const int y = small_div(t, nd), k = t - y * nd;
        const uint32_t a = anc[t];
        if (local) sl.add(a, loc[t], pnorm);
        if (usable && ok) {
            uint32_t g = 0;
            const double v = (double)(y0 + y);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if ((BS && !(BS & 3)) || 4 * k + e < B) {
                    const Sample s = warp_px(h, affine, (double)(x0 + 4 * k + e), v);
                    if (inside(s, A.H, A.W)) g |= global_px(ref, A.pitch, s, A.H, A.W) << (8 * e);
                    else ok = false;
                }
            }
            sg.add(a, g, pnorm);
        }
    }
    const bool global = usable && __builtin_amdgcn_ballot_w64(!ok) == 0;
    uint32_t cg = NO_COST, cl = NO_COST;
    if (global) cg = wave_sum_u32(sg.value(pnorm));
    if (local) cl = wave_sum_u32(sl.value(pnorm));
    if (lane == 0) {
        // (mode 0, cg), (mode 1, cl + penalty) in that order, only a strictly smaller value replaces the best
        uint32_t best = NO_COST;
        int mode = 2;
        if (global) { mode = 0; best = cg; }
        if (local && (mode == 2 || cl + A.penalty < best)) { mode = 1; best = cl + A.penalty; }
        A.mode[blk] = (uint8_t)mode;
        A.cost[blk] = mode == 2 ? -1 : (long long)best;
        A.costs[blk * 2] = global ? (long long)cg : -1;
        A.costs[blk * 2 + 1] = local ? (long long)cl : -1;
    }
}

// n <= 4 pixels of a plane row from column x on, packed, the bytes from n on zero; pixels outside [0, W) read as zero
__device__ __forceinline__ uint32_t load_px(const uint8_t* row, int x, int n, int W, int pitch)
{
    uint32_t v = 0;
    if (x >= 0 && x + 4 <= pitch) {
        __builtin_memcpy(&v, row + x, 4);
        if (n < 4) v &= (1u << (8 * n)) - 1u;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n && x + e >= 0 && x + e < W) v |= (uint32_t)row[x + e] << (8 * e);
    }
    return v;
}

// grid (ceil(cw / BLK_WAVES), ch, pairs) with ch = ceil(H / bs), cw = ceil(W / bs) cells of bs x bs pixels, clipped to the frame.
// A cell that is a whole block (row < hb, column < wb) is, in mode 0, its global predictor pixels where the pair's warp is usable
// and the sample point lies in the frame and, in mode 1, the block of `ref` at the vector where that lies in the frame; every
// other pixel (mode 2, the cells beyond the last whole block, and what a mode cannot supply, which the modes of k_gmc never ask
// for) is the co-located pixel of `ref`.  Pixels at or past W are not written: they are the plane's padding.
__global__ void __launch_bounds__(BLK_THREADS) k_predict_gmc(const uint8_t* ref, const uint8_t* cur, long long plane_stride, int H, int W,
                                                            int pitch, int bs, int hb, int wb, int cw, const double* hs,
                                                            const uint8_t* usable, const uint8_t* mode, const int32_t* f, uint8_t* out,
                                                            long long out_stride, int out_pitch, unsigned long long* sse)
{
    __shared__ uint32_t part[BLK_WAVES];
    const WaveBlock w = wave_block(cw);                          // of cells: a wave without one stays for the barrier below
    const int wave = w.wave, lane = w.lane, cj = w.bj, ci = w.bi, pair = w.z;
    uint32_t err = 0;
    if (!w.none) {                                               // wave-uniform
        const int x0 = cj * bs, y0 = ci * bs;
        const int cols = min(bs, W - x0), rows = min(bs, H - y0), nd = row_dwords(cols);
        const uint8_t* p = ref + (long long)pair * plane_stride;
        const uint8_t* c = cur + (long long)pair * plane_stride;
        uint8_t* o = out + (long long)pair * out_stride;
        // mode and vector once per cell, in scalar registers
        int m = 2, fx = 0, fy = 0;
        if (ci < hb && cj < wb) {
            const long long blk = ((long long)pair * hb + ci) * wb + cj;
            m = __builtin_amdgcn_readfirstlane((int)mode[blk]);
            fx = __builtin_amdgcn_readfirstlane(f[blk * 2]);
            fy = __builtin_amdgcn_readfirstlane(f[blk * 2 + 1]);
        }
        const long long rxl = (long long)x0 + fx, ryl = (long long)y0 + fy;
        const bool local = m == 1 && rxl >= 0 && ryl >= 0 && rxl + bs <= W && ryl + bs <= H;
        const bool global = m == 0 && __builtin_amdgcn_readfirstlane((int)usable[pair]) != 0;
        double h[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = hs[(long long)pair * 8 + k];
        const bool affine = global && h[6] == 0.0 && h[7] == 0.0;
        for (int t = lane; t < rows * nd; t += 64) {
            const int y = small_div(t, nd), k = t - y * nd;
            const int x = x0 + 4 * k, n = min(4, cols - 4 * k);
            const long long row = (long long)(y0 + y) * pitch;
            uint32_t px;
            if (local) px = load_px(p + (ryl + y) * pitch, (int)rxl + 4 * k, n, W, pitch);
            else {
                px = load_px(p + row, x, n, W, pitch);
                if (global) {
                    const double v = (double)(y0 + y);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (e < n) {
                            const Sample s = warp_px(h, affine, (double)(x + e), v);
                            if (inside(s, H, W)) px = (px & ~(0xFFu << (8 * e))) | (global_px(p, pitch, s, H, W) << (8 * e));
                        }
                    }
                }
            }
            const uint32_t q = load_px(c + row, x, n, W, pitch);
            err += __builtin_amdgcn_udot4(px, px, 0u, false) + __builtin_amdgcn_udot4(q, q, 0u, false)
                   - 2u * __builtin_amdgcn_udot4(px, q, 0u, false);
            uint8_t* dst = o + (long long)(y0 + y) * out_pitch + x;
            if (n == 4 && !(x & 3)) *(uint32_t*)dst = px;
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n) dst[e] = (uint8_t)(px >> (8 * e));
            }
        }
    }
    const uint32_t total = wave_sum_u32(err);
    if (lane == 0) part[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {                                      // one error word per workgroup
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < BLK_WAVES; ++k) s += part[k];
        if (s) atomicAdd(&sse[pair], (unsigned long long)s);
    }
}

}  // namespace

// the argument rules of gmc.py
int gmc_check_args(const char* who, int bs, int pnorm, int penalty)
{
    GME_REQUIRE(bs >= GM_MIN_BS && bs <= GM_MAX_BS, GME_ERR_ARG, "%s: block_size %d (%d .. %d)", who, bs, GM_MIN_BS, GM_MAX_BS);
    if (int rc = require_pnorm(who, pnorm)) return rc;
    GME_REQUIRE(penalty >= 0 && penalty <= GM_MAX_PENALTY, GME_ERR_ARG, "%s: penalty %d (0 .. 2^30)", who, penalty);
    return GME_OK;
}

// gmc.usable: finite, and the denominator (h6 u + h7 v) + 1 positive at the four corners of the frame (one rounding per
// operation, as direct.corners_ok: the library builds with -ffp-contract=off)
bool gmc_usable(const double* h, int H, int W)
{
    for (int k = 0; k < 8; ++k)
        if (!std::isfinite(h[k])) return false;
    const double us[2] = { 0.0, (double)W - 1.0 }, vs[2] = { 0.0, (double)H - 1.0 };
    for (double v : vs)
        for (double u : us) {
            const double a = h[6] * u, b = h[7] * v;
            const double s = a + b;
            if (!(s + 1.0 > 0.0)) return false;
        }
    return true;
}

// gmc.decide of `pairs` pairs: pair k reads the planes ref + k * plane_stride and cur + k * plane_stride, the warp h[k] with its
// flag usable[k] and the field f[k] of [hb][wb][2], hb = H / bs and wb = W / bs; mode [pairs][hb][wb], cost [pairs][hb][wb] and
// costs [pairs][hb][wb][2] (all device)
int launch_gmc(gme_ctx* ctx, const uint8_t* ref, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
               int pnorm, int penalty, const double* h, const uint8_t* usable, const int32_t* f, uint8_t* mode, long long* cost,
               long long* costs)
{
    int rc = gmc_check_args("global motion compensation", bs, pnorm, penalty);
    if (rc) return rc;
    const int hb = H / bs, wb = W / bs;
    const bool compiled = bs == 16 || bs == 32;
    GmcArgs a;
    a.stride = plane_stride; a.H = H; a.W = W; a.pitch = pitch;
    a.hb = hb; a.wb = wb; a.bs = bs; a.pnorm = pnorm; a.penalty = (uint32_t)penalty;
    a.block_bytes = block_bytes(bs);
    const long long per = (long long)hb * wb;
    auto note = [&] {
        if (compiled) plan_note(ctx, 0, "k_gmc<%d> penalty %d, %d x %d blocks, one wave each", bs, penalty, hb, wb);
        else plan_note(ctx, 0, "k_gmc<0> bs %d penalty %d, %d x %d blocks, one wave each", bs, penalty, hb, wb);
    };
    return launch_wave_blocks(ctx, pairs, hb, wb, 2 * a.block_bytes, a, note, [&](int k) {
        const long long off = (long long)k * plane_stride;
        a.ref = ref + off; a.cur = cur + off;
        a.h = h + (size_t)k * 8; a.usable = usable + k;
        a.f = f + per * k * 2;
        a.mode = mode + per * k; a.cost = cost + per * k; a.costs = costs + per * k * 2;
        return !compiled ? k_gmc<0> : bs == 16 ? k_gmc<16> : k_gmc<32>;
    });
}

// out planes = gmc.predict of the ref planes by h, usable, mode and f of [pairs][H / bs][W / bs], sse[pairs] (device, zeroed here)
// = squared error of each against its cur plane
int launch_predict_gmc(gme_ctx* ctx, const uint8_t* ref, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch,
                       int bs, const double* h, const uint8_t* usable, const uint8_t* mode, const int32_t* f, uint8_t* out,
                       long long out_stride, int out_pitch, unsigned long long* sse)
{
    if (pairs == 0) return GME_OK;
    GME_REQUIRE(bs >= GM_MIN_BS && bs <= GM_MAX_BS, GME_ERR_ARG, "block_size %d (%d .. %d)", bs, GM_MIN_BS, GM_MAX_BS);
    const int hb = H / bs, wb = W / bs, ch = (H + bs - 1) / bs, cw = (W + bs - 1) / bs;
    GME_REQUIRE(ch <= 65535, GME_ERR_ARG, "%d block rows", ch);
    const long long per = (long long)hb * wb;
    return predict_planes(ctx, pairs, sse, [&](int k, int n) {
        const long long off = (long long)k * plane_stride;
        const dim3 grid((cw + BLK_WAVES - 1) / BLK_WAVES, ch, n);
        hipLaunchKernelGGL(k_predict_gmc, grid, dim3(BLK_THREADS), 0, ctx->stream, ref + off, cur + off, plane_stride, H, W, pitch, bs, hb,
                           wb, cw, h + (size_t)k * 8, usable + k, mode + per * k, f + per * k * 2, out + (long long)k * out_stride,
                           out_stride, out_pitch, sse + k);
    });
}
