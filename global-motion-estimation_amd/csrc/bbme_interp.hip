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
#include "gme_passes.h"

namespace {

constexpr int IP_MIN_BS = 4, IP_MAX_BS = 64, IP_MAX_SW = 8, IP_MAX_BIAS = 1 << 16;
constexpr long long IP_MAX_DIST = (long long)IP_MAX_BS * IP_MAX_BS * 65025ll;
// J is 32-bit in the kernel (int64 at the ABI): the largest is 64 * 64 * 255^2 + 2^16 * (8 + 8)
static_assert(IP_MAX_DIST + (long long)IP_MAX_BIAS * 2 * IP_MAX_SW < (1ll << 31), "31-bit J");
// a lane's share of sum a^2 + sum b^2 (RowScore, modulo 2^32 until its difference with 2 ab is taken) does not wrap either
static_assert(2 * IP_MAX_DIST < (1ll << 32), "sum a^2 + sum b^2 of a block in 32 bits");
// the order of a candidate: 0 for the centre, 1 + index in [-sw, sw]^2 (column offset outer) for the others; it needs 9 bits
// beside a J of 29, so J and order do not share a 32-bit key: two wave-wide minima
constexpr int IP_MAX_CAND = (2 * IP_MAX_SW + 1) * (2 * IP_MAX_SW + 1);
static_assert(IP_MAX_CAND + 1 <= (1 << 9) && (IP_MAX_DIST << 9) >= (1ll << 32), "J and order in one 32-bit key");
constexpr int IP_MAX_WINDOW = IP_MAX_BS + 2 * IP_MAX_SW;
static_assert(small_div_covers(IP_MAX_WINDOW, window_row_dwords(IP_MAX_WINDOW), 2 * IP_MAX_SW + 1), "range of small_div");
// a workgroup's LDS without an opt-in: both windows of four waves (52.5 KiB at B 64, sw 8: three workgroups to a CU)
static_assert(BLK_WAVES * 2 * window_bytes(IP_MAX_WINDOW) <= 64 * 1024, "LDS of a workgroup");

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

template <int BS>
__global__ void __launch_bounds__(BLK_THREADS) k_interp(const InterpArgs A)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const WaveBlock w = wave_block(A.wb);
    if (w.none) return;
    const int wave = w.wave, lane = w.lane, bj = w.bj, bi = w.bi, pair = w.z;
    const int B = BS ? BS : A.bs;
    const int sw = A.sw, pnorm = A.pnorm;
    const int x0 = bj * B, y0 = bi * B;
    uint32_t* pw = (uint32_t*)(lds + (size_t)wave * 2 * A.window_bytes);
    uint32_t* nw = (uint32_t*)(lds + (size_t)wave * 2 * A.window_bytes + A.window_bytes);
    const int nd = row_dwords(B), ws = B + 2 * sw, wd = window_row_dwords(ws);
    const uint32_t tail = tail_mask(B);
    constexpr bool TAIL = !BS || (BS & 3);                       // the last dword of a row may hold bytes beyond the block
    const long long plane = (long long)pair * A.stride;
    stage_bytes_clamped(pw, ws, wd, ws, A.past + plane, A.pitch, A.H, A.W, y0 - sw, x0 - sw, lane);
    stage_bytes_clamped(nw, ws, wd, ws, A.next + plane, A.pitch, A.H, A.W, y0 - sw, x0 - sw, lane);
    wave_lds_fence();

    const Square sq(sw);
    // lanes_for_one_round and LaneSplit written out, slot and share by division: with the shared forms this kernel carries two
    // window values in vector registers across the staging loops and takes about 1 % longer at 1920 x 1080
    int P = 1;
    while (P < 8 && sq.ncand * (P * 2) <= 64) P *= 2;
    const int slots = 64 / P, slot = lane / P, q = lane - slot * P;
    Least best;
    for (int c0 = 0; c0 < sq.ncand; c0 += slots) {
        const int c = c0 + slot;
        const bool listed = c < sq.ncand;                        // lanes beyond the list score candidate 0 and drop it
        int nx, ny;                                              // the candidate's block in the next window (column, row): sw + o
        sq.at(listed ? c : 0, &nx, &ny);
        const int px = 2 * sw - nx, py = 2 * sw - ny;            // ... and in the past window: sw - o
        const uint32_t psh = (uint32_t)px & 3u, nsh = (uint32_t)nx & 3u;
        RowScore s;
        for (int y = q; y < B; y += P) {
            const uint32_t* prow = pw + (py + y) * wd + (px >> 2);
            const uint32_t* nrow = nw + (ny + y) * wd + (nx >> 2);
#pragma unroll 4
            for (int k = 0; k < nd; ++k) {
                uint32_t a = window_dword(prow, k, psh);
                uint32_t v = window_dword(nrow, k, nsh);
                if (TAIL) { if (k == nd - 1) { a &= tail; v &= tail; } }
                s.add(a, v, pnorm);
            }
        }
        const uint32_t j = lanes_sum(s.value(pnorm), P) + A.bias * (uint32_t)(abs(nx - sw) + abs(ny - sw));
        if (listed) best.take(j, sq.order(c, nx, ny));
    }
    const Least win = wave_least(best.cost, best.order);
    if (lane == 0) {
        int vx, vy;
        sq.offset(win.order, &vx, &vy);
        const long long blk = ((long long)pair * A.hb + bi) * A.wb + bj;
        A.mv[blk * 2] = vx;
        A.mv[blk * 2 + 1] = vy;
        A.cost[blk] = (long long)win.cost;
        A.dist[blk] = (long long)(win.cost - A.bias * (uint32_t)(abs(vx) + abs(vy)));
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

}  // namespace

// the argument rules of interp.py
int interp_check_args(const char* who, int H, int W, int bs, int sw, int pnorm, int bias)
{
    GME_REQUIRE(bs >= IP_MIN_BS && bs <= IP_MAX_BS, GME_ERR_ARG, "%s: block_size %d (%d .. %d)", who, bs, IP_MIN_BS, IP_MAX_BS);
    GME_REQUIRE(sw >= 0 && sw <= IP_MAX_SW, GME_ERR_ARG, "%s: search_window %d (0 .. %d)", who, sw, IP_MAX_SW);
    if (int rc = require_pnorm(who, pnorm)) return rc;
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
    const bool compiled = bs == 16 || bs == 32;
    InterpArgs a;
    a.stride = plane_stride; a.H = H; a.W = W; a.pitch = pitch;
    a.hb = hb; a.wb = wb; a.bs = bs; a.sw = sw; a.pnorm = pnorm; a.bias = (uint32_t)bias;
    a.window_bytes = window_bytes(bs + 2 * sw);
    const long long per = (long long)hb * wb;
    auto note = [&] {
        if (compiled) plan_note(ctx, 0, "k_interp<%d> sw %d bias %d, %d x %d blocks, one wave each", bs, sw, bias, hb, wb);
        else plan_note(ctx, 0, "k_interp<0> bs %d sw %d bias %d, %d x %d blocks, one wave each", bs, sw, bias, hb, wb);
    };
    return launch_wave_blocks(ctx, pairs, hb, wb, 2 * a.window_bytes, a, note, [&](int k) {   // H, W >= bs: there are blocks
        const long long off = (long long)k * plane_stride;
        a.past = past + off; a.next = next + off;
        a.mv = mv + per * k * 2; a.cost = cost + per * k; a.dist = dist + per * k;
        return !compiled ? k_interp<0> : bs == 16 ? k_interp<16> : k_interp<32>;
    });
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
