// Motion-compensated frame interpolation (host definition: interp.py).  The frame halfway between `past`
// and `next` exists nowhere, so there is no target block to match against: block (i, j) of the new frame takes the vector v for
// which `past` at origin - v and `next` at origin + v differ least (bilateral search), J(v) = D(v) + bias (|vx| + |vy|), and is
// made as the rounded average of the two.  Coordinates are clamped to the frame (border replication), so no candidate is ever
// unavailable; a block depends on no neighbour and every candidate is always scored, so the work is fixed whatever the content.
// Everything is integer: the device equals interp.search and interp.interpolate byte for byte.
//
// Kernels:
//   k_interp<BS>        one wave per block, four blocks to a 256-thread workgroup, each wave on its own LDS slice (no workgroup
//                       barrier).  The wave stages the (BS + 2 sw)^2 windows of both frames around the block with clamped
//                       coordinates; spreads the (2 sw + 1)^2 candidates over its lanes (P lanes share the rows of one candidate
//                       where there are fewer than 33); scores a row four bytes at a time (v_alignbyte for both operands: the
//                       past window at (sw - ox, sw - oy), the next window at (sw + ox, sw + oy); then v_sad_u8, or three
//                       v_dot4 for aa + bb - 2ab); and selects the minimum of (J, position in the definition's order, centre
//                       = 0) in two wave-wide minima.  <16> and <32> are compiled; <0> takes the block size at run time (and
//                       rows that are no multiple of four bytes).
//   k_interp_frame      interp.interpolate per pixel, with the squared error of each frame against the true middle frame where
//                       there is one
#include "bbme_predict.h"
#include "bbme_wave_lds.h"

namespace {

constexpr int IP_THREADS = 256, IP_WAVES = IP_THREADS / 64;
constexpr int IP_MIN_BS = 4, IP_MAX_BS = 64, IP_MAX_SW = 8, IP_MAX_BIAS = 1 << 16;
constexpr long long IP_MAX_DIST = (long long)IP_MAX_BS * IP_MAX_BS * 65025ll;
constexpr uint32_t IP_NONE = 0xFFFFFFFFu;                       // no cost: above every J there is
// J is 32-bit in the kernel (int64 at the ABI): the largest is 64 * 64 * 255^2 + 2^16 * (8 + 8)
static_assert(IP_MAX_DIST + (long long)IP_MAX_BIAS * 2 * IP_MAX_SW < (1ll << 31), "31-bit J");
// a lane's share of sum a^2 + sum b^2 (RowScore, modulo 2^32 until its difference with 2 ab is taken) does not wrap either
static_assert(2 * IP_MAX_DIST < (1ll << 32), "sum a^2 + sum b^2 of a block in 32 bits");
// the order of a candidate: 0 for the centre, 1 + index in [-sw, sw]^2 (column offset outer) for the others; it needs 9 bits
// beside a J of 29, so J and order do not share a 32-bit key: two wave-wide minima
constexpr int IP_MAX_CAND = (2 * IP_MAX_SW + 1) * (2 * IP_MAX_SW + 1);
static_assert(IP_MAX_CAND + 1 <= (1 << 9) && (IP_MAX_DIST << 9) >= (1ll << 32), "J and order in one 32-bit key");
constexpr int IP_MAX_WINDOW = IP_MAX_BS + 2 * IP_MAX_SW;
constexpr int IP_MAX_WINDOW_DWORDS = (IP_MAX_WINDOW + 3) / 4 + 1;
static_assert(IP_MAX_WINDOW * IP_MAX_WINDOW_DWORDS < SMALL_DIV_T && IP_MAX_WINDOW_DWORDS <= SMALL_DIV_D && 2 * IP_MAX_SW + 1 <= SMALL_DIV_D &&
                  IP_MAX_CAND < SMALL_DIV_T, "range of small_div");
// a workgroup's LDS without an opt-in: both windows of four waves (52.5 KiB at B 64, sw 8: three workgroups to a CU)
static_assert(IP_WAVES * (2 * IP_MAX_WINDOW * IP_MAX_WINDOW_DWORDS * 4 + 32) <= 64 * 1024, "LDS of a workgroup");

struct InterpArgs {
    const uint8_t* past;          // first plane of each role; pair k reads the planes k * stride bytes on
    const uint8_t* next;
    long long stride;
    int H, W, pitch;
    int32_t* mv;                  // [pairs][hb][wb][2]
    long long* cost;              // [pairs][hb][wb]: J of the winner
    long long* dist;              // [pairs][hb][wb]: its D
    int hb, wb, bs, sw, pnorm;
    uint32_t bias;
    int window_bytes;             // LDS of a wave: the window of past, then the window of next
};

// grid (ceil(wb / IP_WAVES), hb, pairs)
template <int BS>
__global__ void __launch_bounds__(IP_THREADS) k_interp(const InterpArgs A)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int bj = blockIdx.x * IP_WAVES + wave, bi = blockIdx.y, pair = blockIdx.z;
    if (bj >= A.wb) return;                                      // the whole wave: nothing below synchronises across waves
    const int B = BS ? BS : A.bs;
    const int sw = A.sw, n = 2 * sw + 1, ncand = n * n, pnorm = A.pnorm;
    const int x0 = bj * B, y0 = bi * B;
    uint32_t* pw = (uint32_t*)(lds + (size_t)wave * 2 * A.window_bytes);
    uint32_t* nw = (uint32_t*)(lds + (size_t)wave * 2 * A.window_bytes + A.window_bytes);
    // window rows of one dword more than their bytes need: v_alignbyte reads the dword behind the last one it uses
    const int nd = (B + 3) >> 2, ws = B + 2 * sw, wd = ((ws + 3) >> 2) + 1;
    const uint32_t tail = (B & 3) ? (1u << (8 * (B & 3))) - 1u : 0xFFFFFFFFu;
    constexpr bool TAIL = !BS || (BS & 3);                       // the last dword of a row may hold bytes beyond the block
    const long long plane = (long long)pair * A.stride;
    stage_bytes_clamped(pw, ws, wd, ws, A.past + plane, A.pitch, A.H, A.W, y0 - sw, x0 - sw, lane);
    stage_bytes_clamped(nw, ws, wd, ws, A.next + plane, A.pitch, A.H, A.W, y0 - sw, x0 - sw, lane);
    wave_lds_fence();

    // P lanes to a candidate, each a share of the rows: as many as leave every candidate a slot in one round, at most 8
    int P = 1;
    while (P < 8 && ncand * (P * 2) <= 64) P *= 2;
    const int slots = 64 / P, slot = lane / P, q = lane - slot * P;
    uint32_t best = IP_NONE, best_order = IP_NONE;
    for (int c0 = 0; c0 < ncand; c0 += slots) {
        const int c = c0 + slot;
        const bool listed = c < ncand;
        const int cc = listed ? c : 0;                           // lanes beyond the list score candidate 0 and drop it
        const int nx = small_div(cc, n), ny = cc - nx * n;       // the candidate's block in the next window (column, row): sw + o
        const int px = 2 * sw - nx, py = 2 * sw - ny;            // ... and in the past window: sw - o
        const uint32_t psh = (uint32_t)px & 3u, nsh = (uint32_t)nx & 3u;
        RowScore s;
        for (int y = q; y < B; y += P) {
            const uint32_t* prow = pw + (py + y) * wd + (px >> 2);
            const uint32_t* nrow = nw + (ny + y) * wd + (nx >> 2);
#pragma unroll 4
            for (int k = 0; k < nd; ++k) {
                uint32_t a = __builtin_amdgcn_alignbyte(prow[k + 1], prow[k], psh);
                uint32_t v = __builtin_amdgcn_alignbyte(nrow[k + 1], nrow[k], nsh);
                if (TAIL) { if (k == nd - 1) { a &= tail; v &= tail; } }
                s.add(a, v, pnorm);
            }
        }
        uint32_t part = s.value(pnorm);
        for (int m = 1; m < P; m <<= 1) part += (uint32_t)__shfl_xor((int)part, m, 64);
        const int ox = nx - sw, oy = ny - sw;
        const uint32_t j = part + A.bias * (uint32_t)(abs(ox) + abs(oy));
        const uint32_t order = (ox == 0 && oy == 0) ? 0u : (uint32_t)c + 1u;
        if (listed && (j < best || (j == best && order < best_order))) { best = j; best_order = order; }
    }
    const uint32_t win_cost = wave_min_u32(best);
    const uint32_t win_order = wave_min_u32(best == win_cost ? best_order : IP_NONE);
    if (lane == 0) {
        int vx = 0, vy = 0;
        if (win_order != 0u) {
            const int c = (int)win_order - 1;
            vx = small_div(c, n) - sw;
            vy = c - small_div(c, n) * n - sw;
        }
        const long long blk = ((long long)pair * A.hb + bi) * A.wb + bj;
        A.mv[blk * 2] = vx;
        A.mv[blk * 2 + 1] = vy;
        A.cost[blk] = (long long)win_cost;
        A.dist[blk] = (long long)(win_cost - A.bias * (uint32_t)(abs(vx) + abs(vy)));
    }
}

// The pixel of k_interp_frame.  Output pixel (u, v) of block (v / bs, u / bs) inside the hb x wb grid is the rounded average of
// `past` at (u - vx, v - vy) and `next` at (u + vx, v + vy), both clamped to the frame; beyond the last whole block the vector is
// zero.
struct InterpPixel {
    const uint8_t* p;             // the pair's `past` and `next` planes
    const uint8_t* q;
    const int32_t* mv;            // its vectors [hb][wb][2]
    int H, W, pitch, bs, hb, wb;
    __device__ __forceinline__ int operator()(int u, int v) const
    {
        const int i = v / bs, j = u / bs;
        int vx = 0, vy = 0;
        if (i < hb && j < wb) {
            const long long b = (long long)i * wb + j;
            vx = min(max(mv[b * 2], -IP_MAX_SW), IP_MAX_SW);     // k_interp's vectors lie within the window: the clamp keeps
            vy = min(max(mv[b * 2 + 1], -IP_MAX_SW), IP_MAX_SW); // the sums below in range whatever the buffer holds
        }
        const int pu = min(max(u - vx, 0), W - 1), pv = min(max(v - vy, 0), H - 1);
        const int qu = min(max(u + vx, 0), W - 1), qv = min(max(v + vy, 0), H - 1);
        return ((int)p[(long long)pv * pitch + pu] + (int)q[(long long)qv * pitch + qu] + 1) >> 1;
    }
};

// the row frame of bbme_predict.h, one plane per pair; `cur` is the true middle frame, or any plane where there is none (the
// squared error is then not used)
__global__ void __launch_bounds__(PRED_THREADS) k_interp_frame(const uint8_t* past, const uint8_t* next, const uint8_t* cur,
                                                               long long plane_stride, int H, int W, int pitch, int bs, int hb, int wb,
                                                               const int32_t* mv, uint8_t* out, long long out_stride, int out_pitch,
                                                               unsigned long long* sse)
{
    const int f = blockIdx.z;
    const long long plane = (long long)f * plane_stride, blocks = (long long)f * hb * wb;
    const InterpPixel px = { past + plane, next + plane, mv + blocks * 2, H, W, pitch, bs, hb, wb };
    predict_rows(px, cur + plane, H, W, pitch, out + (long long)f * out_stride, out_pitch, sse + f);
}

template <int BS>
void interp_launch(hipStream_t stream, const InterpArgs& a, int pairs)
{
    hipLaunchKernelGGL((k_interp<BS>), dim3((unsigned)((a.wb + IP_WAVES - 1) / IP_WAVES), (unsigned)a.hb, (unsigned)pairs),
                       dim3(IP_THREADS), (size_t)IP_WAVES * 2 * a.window_bytes, stream, a);
}

}  // namespace

// the argument rules of interp.py
int interp_check_args(const char* who, int H, int W, int bs, int sw, int pnorm, int bias)
{
    GME_REQUIRE(bs >= IP_MIN_BS && bs <= IP_MAX_BS, GME_ERR_ARG, "%s: block_size %d (%d .. %d)", who, bs, IP_MIN_BS, IP_MAX_BS);
    GME_REQUIRE(sw >= 0 && sw <= IP_MAX_SW, GME_ERR_ARG, "%s: search_window %d (0 .. %d)", who, sw, IP_MAX_SW);
    GME_REQUIRE(pnorm == 0 || pnorm == 1, GME_ERR_ARG, "%s: pnorm_distance %d out of range (bbme.py:60)", who, pnorm);
    GME_REQUIRE(bias >= 0 && bias <= IP_MAX_BIAS, GME_ERR_ARG, "%s: bias %d (0 .. 2^16)", who, bias);
    GME_REQUIRE(H >= bs && W >= bs, GME_ERR_ARG, "%s: a %d x %d frame holds no block of %d", who, H, W, bs);
    return GME_OK;
}

// interp.search of `pairs` pairs: pair k reads the planes past + k * plane_stride and next + k * plane_stride; mv
// [pairs][hb][wb][2], cost and dist [pairs][hb][wb] (device), hb = H / bs and wb = W / bs
int launch_interp(gme_ctx* ctx, const uint8_t* past, const uint8_t* next, long long plane_stride, int pairs, int H, int W, int pitch,
                  int bs, int sw, int pnorm, int bias, int32_t* mv, long long* cost, long long* dist)
{
    int rc = interp_check_args("frame interpolation", H, W, bs, sw, pnorm, bias);
    if (rc) return rc;
    const int hb = H / bs, wb = W / bs;
    ctx->plan[0] = 0; ctx->plan_patches = 0;
    const bool compiled = bs == 16 || bs == 32;
    if (compiled) plan_note(ctx, 0, "k_interp<%d> sw %d bias %d, %d x %d blocks, one wave each", bs, sw, bias, hb, wb);
    else plan_note(ctx, 0, "k_interp<0> bs %d sw %d bias %d, %d x %d blocks, one wave each", bs, sw, bias, hb, wb);
    if (pairs == 0) return GME_OK;
    GME_REQUIRE(hb <= 65535, GME_ERR_ARG, "%d block rows", hb);
    InterpArgs a;
    a.stride = plane_stride; a.H = H; a.W = W; a.pitch = pitch;
    a.hb = hb; a.wb = wb; a.bs = bs; a.sw = sw; a.pnorm = pnorm; a.bias = (uint32_t)bias;
    const int side = bs + 2 * sw;
    a.window_bytes = (side * ((side + 3) / 4 + 1) * 4 + 15) & ~15;
    const long long per = (long long)hb * wb;
    for_plane_chunks(pairs, [&](int k, int n) {
        const long long off = (long long)k * plane_stride;
        a.past = past + off; a.next = next + off;
        a.mv = mv + per * k * 2; a.cost = cost + per * k; a.dist = dist + per * k;
        if (!compiled) interp_launch<0>(ctx->stream, a, n);
        else if (bs == 16) interp_launch<16>(ctx->stream, a, n);
        else interp_launch<32>(ctx->stream, a, n);
    });
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}

// out planes = interp.interpolate of the past and next planes by mv [pairs][H / bs][W / bs][2], sse[pairs] (device, zeroed here) =
// squared error of each against its `cur` plane (the true middle frame; any plane of the stack where there is none)
int launch_interp_frame(gme_ctx* ctx, const uint8_t* past, const uint8_t* next, const uint8_t* cur, long long plane_stride, int pairs,
                        int H, int W, int pitch, int bs, const int32_t* mv, uint8_t* out, long long out_stride, int out_pitch,
                        unsigned long long* sse)
{
    if (pairs == 0) return GME_OK;
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    const int hb = H / bs, wb = W / bs;
    const long long per = (long long)hb * wb;
    return predict_planes(ctx, pairs, sse, [&](int k, int n) {
        const long long off = (long long)k * plane_stride;
        hipLaunchKernelGGL(k_interp_frame, predict_grid(H, W, n), dim3(PRED_THREADS), 0, ctx->stream, past + off, next + off, cur + off,
                           plane_stride, H, W, pitch, bs, hb, wb, mv + per * k * 2, out + (long long)k * out_stride, out_stride,
                           out_pitch, sse + k);
    });
}
