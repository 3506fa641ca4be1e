// Frame interpolation at any phase (host definition: retime.py).  The new frame lies at phase n / d between
// `past` and `next`, 1 <= n < d <= 64.  A candidate V in [-sw, sw]^2, in whole pixels, is how far content moves from `past` to
// `next`; it reads `past` displaced by a(V) and `next` by b(V) = a(V) + 4 V quarter pixels per component, a(V) = -4 n V / d rounded
// to the nearest quarter (halves up), through the four-tap quarter-pel sampler of obmc.py with every tap clamped to the frame.
// J(V) = D(V) + bias (|Vx| + |Vy|) in interp.search's order; the pixel is ((d - n) P + n N + d / 2) / d.  No candidate is ever
// unavailable, a block depends on no neighbour and every candidate is always scored, so the work is fixed whatever the content.
// Everything is integer: the device equals retime.search and retime.interpolate byte for byte.
//
// Kernels:
//   k_retime<BS>        one wave per block, four blocks to a 256-thread workgroup, each wave on its own LDS slice (no workgroup
//                       barrier).  Both sides of a candidate share one fractional part, (a(Vx) & 3, a(Vy) & 3), so the candidates
//                       fall into at most 16 classes.  Per class the wave stages the interpolated window of `past` and of `next`
//                       (the four clamped taps straight from the frame), then scores the class's candidates at whole-pixel
//                       offsets a >> 2 and (a >> 2) + V into those windows, a row four bytes at a time (v_alignbyte, then
//                       v_sad_u8, or three v_dot4), P lanes to a candidate where a class has fewer than 33.  The windows are as
//                       large as the phase makes them: the past side reaches sw n / d, the next side sw (d - n) / d.  A lane
//                       keeps the least (J, position in the definition's order, centre = 0) across the classes; two wave-wide
//                       minima select the winner.  <16> and <32> are compiled; <0> takes the block size at run time.  Every
//                       output of a launch has its own row of the phase table (RT_*): pair, n, d, a(V) and the classes.
//   k_retime_frame      retime.interpolate per pixel, with the squared error of each frame against a true frame where there is
//                       one
#include "bbme_predict.h"
#include "bbme_wave_lds.h"
#include "gme_passes.h"

namespace {

constexpr int RT_MIN_BS = 4, RT_MAX_BS = 64, RT_MAX_SW = 16, RT_MAX_BIAS = 1 << 16, RT_MAX_D = 64;
constexpr long long RT_MAX_DIST = (long long)RT_MAX_BS * RT_MAX_BS * 65025ll;
// J is 32-bit in the kernel (int64 at the ABI): the largest is 64 * 64 * 255^2 + 2^16 * (16 + 16)
static_assert(RT_MAX_DIST + (long long)RT_MAX_BIAS * 2 * RT_MAX_SW < (1ll << 31), "31-bit J");
// a lane's share of sum a^2 + sum b^2 (RowScore, modulo 2^32 until its difference with 2 ab is taken) does not wrap either
static_assert(2 * RT_MAX_DIST < (1ll << 32), "sum a^2 + sum b^2 of a block in 32 bits");

// a(V) of the definition: -floor((8 n V + d) / (2 d))
constexpr int retime_a(int V, int n, int d)
{
    const int num = 8 * n * V + d, den = 2 * d;
    return -(num >= 0 ? num / den : -((-num + den - 1) / den));
}
constexpr int floor4(int q) { return q >= 0 ? q / 4 : -((-q + 3) / 4); }      // q >> 2 of a quarter offset

// The windows of a phase: the whole-pixel offsets of the past side span [pmin, pmax] (a falls as V grows), those of the next
// side [bmin, bmax] (b rises), so the windows are B + pmax - pmin and B + bmax - bmin to a side.
struct RetimeSpan {
    int pmin, pmax, bmin, bmax;
};
constexpr RetimeSpan retime_span(int sw, int n, int d)
{
    return { floor4(retime_a(sw, n, d)), floor4(retime_a(-sw, n, d)), floor4(retime_a(-sw, n, d)) - sw, floor4(retime_a(sw, n, d)) + sw };
}
// LDS of a wave: the window of past, then the window of next
constexpr int retime_wave_lds(int bs, int sw, int n, int d)
{
    const RetimeSpan s = retime_span(sw, n, d);
    return window_bytes(bs + s.pmax - s.pmin) + window_bytes(bs + s.bmax - s.bmin);
}
constexpr int retime_worst_lds()
{
    int worst = 0;
    for (int d = 2; d <= RT_MAX_D; ++d)
        for (int n = 1; n < d; ++n) {
            const int b = retime_wave_lds(RT_MAX_BS, RT_MAX_SW, n, d);
            if (b > worst) worst = b;
        }
    return worst;
}
// a workgroup's LDS without an opt-in: both windows of four waves at B 64, sw 16 and the most lopsided phase
static_assert(BLK_WAVES * retime_worst_lds() <= 64 * 1024, "LDS of a workgroup");

// t / q as the high half of t * (floor((2^32 - 1) / q) + 1), q >= 2: the factor is 2^32 / q itself for a power of two and
// floor(2^32 / q) + 1 otherwise, exact while t * q < 2^32 (the error term t / 2^32 stays below 1 / q)
constexpr uint32_t recip32(int q) { return 0xFFFFFFFFu / (uint32_t)q + 1u; }
__device__ __forceinline__ int div_recip(int t, uint32_t r) { return (int)__umulhi((uint32_t)t, r); }
constexpr int RT_MAX_SIDE = RT_MAX_BS + 2 * RT_MAX_SW + 2;
// the staging index of the largest window by its row dwords, a candidate's index in a class by the class's rows, and the blend's
// numerator (d - n) P + n N + d / 2 <= 64 * 255 + 32 by d
static_assert((long long)RT_MAX_SIDE * window_row_dwords(RT_MAX_SIDE) * window_row_dwords(RT_MAX_SIDE) < (1ll << 32), "range of div_recip");
static_assert((long long)(2 * RT_MAX_SW + 1) * (2 * RT_MAX_SW + 1) * (2 * RT_MAX_SW + 1) < (1ll << 32), "range of div_recip");
static_assert((long long)(RT_MAX_D * 255 + RT_MAX_D / 2) * RT_MAX_D < (1ll << 32), "range of div_recip");

// The row of the phase table of one output, int32[RT_ROW], written by retime_row on the host
constexpr int RT_PLANE = 0;       // the plane of `past` in the stack; `next` is the one behind it
constexpr int RT_N = 1, RT_D = 2;
constexpr int RT_RECIP_D = 3;     // recip32(d)
constexpr int RT_START = 4;       // [5]: class f = a & 3 holds RT_PERM[RT_START + f .. RT_START + f + 1)
constexpr int RT_RECIP_COUNT = 9; // [4]: recip32 of a class's size (unused where the size is below 2)
constexpr int RT_RECIP_ROW = 13;  // [2]: recip32 of the row dwords of the past and of the next window
constexpr int RT_A = 16;          // [33]: a(V), V = -16 .. 16
constexpr int RT_PERM = 52;       // [2 sw + 1]: the V of [-sw, sw] grouped by class, ascending inside a class
constexpr int RT_ROW = 88;
static_assert(RT_A + 2 * RT_MAX_SW + 1 <= RT_PERM && RT_PERM + 2 * RT_MAX_SW + 1 <= RT_ROW, "layout of a table row");

struct RetimeArgs {
    const uint8_t* frames;        // plane 0 of the stack the rows' planes count from
    long long stride;
    int H, W, pitch;
    const int32_t* table;         // [outputs][RT_ROW]
    int32_t* mv;                  // [outputs][hb][wb][2]
    long long* cost;              // [outputs][hb][wb]: J of the winner
    long long* dist;              // [outputs][hb][wb]: its D
    int hb, wb, bs, sw, pnorm;
    uint32_t bias;
    int wave_lds;                 // LDS of a wave: the largest retime_wave_lds of the launch's outputs
};

// obmc.sample at the quarter position (X, Y): each of the four taps clamped to the frame
__device__ __forceinline__ int quarter_sample(const uint8_t* f, int pitch, int H, int W, int X, int Y)
{
    const int x0 = X >> 2, fx = X & 3, y0 = Y >> 2, fy = Y & 3;
    const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
    const uint8_t* ra = f + (long long)min(max(y0, 0), H - 1) * pitch;
    const uint8_t* rb = f + (long long)min(max(y0 + 1, 0), H - 1) * pitch;
    return ((4 - fx) * (4 - fy) * ra[xa] + fx * (4 - fy) * ra[xb] + (4 - fx) * fy * rb[xa] + fx * fy * rb[xb] + 8) >> 4;
}

// The interpolated window of one class: byte (r, c), c < side, is obmc.sample at (4 (x0 + c) + fx, 4 (y0 + r) + fy).  Bytes at
// c >= side are zero.  A dword whose five source columns lie in [0, W) reads them at once, the others byte by byte, clamped.
__device__ __forceinline__ void stage_quarter(uint32_t* dst, int side, int rd, uint32_t recip_rd, const uint8_t* f, int pitch, int H, int W,
                                              int y0, int x0, int fx, int fy, int lane)
{
    const int w00 = (4 - fx) * (4 - fy), w01 = fx * (4 - fy), w10 = (4 - fx) * fy, w11 = fx * fy;
    for (int t = lane; t < side * rd; t += 64) {
        const int r = div_recip(t, recip_rd), k = t - r * rd;
        const int x = x0 + 4 * k, left = side - 4 * k;
        uint32_t v = 0;
        if (left > 0) {
            const uint8_t* ra = f + (long long)min(max(y0 + r, 0), H - 1) * pitch;
            const uint8_t* rb = f + (long long)min(max(y0 + r + 1, 0), H - 1) * pitch;
            uint32_t a = 0, b = 0, a4, b4;                       // columns x .. x + 3 of the two rows, and column x + 4
            if (x >= 0 && x + 5 <= W) {
                __builtin_memcpy(&a, ra + x, 4);
                __builtin_memcpy(&b, rb + x, 4);
                a4 = ra[x + 4]; b4 = rb[x + 4];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int xc = min(max(x + e, 0), W - 1);
                    a |= (uint32_t)ra[xc] << (8 * e);
                    b |= (uint32_t)rb[xc] << (8 * e);
                }
                const int xc = min(max(x + 4, 0), W - 1);
                a4 = ra[xc]; b4 = rb[xc];
            }
            const uint32_t as = (a >> 8) | (a4 << 24), bs = (b >> 8) | (b4 << 24);       // the same rows one column on
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t s = w00 * ((a >> (8 * e)) & 255u) + w01 * ((as >> (8 * e)) & 255u) + w10 * ((b >> (8 * e)) & 255u) +
                                   w11 * ((bs >> (8 * e)) & 255u) + 8u;
                v |= (s >> 4) << (8 * e);
            }
            if (left < 4) v &= (1u << (8 * left)) - 1u;
        }
        dst[t] = v;
    }
}

template <int BS>
__global__ void __launch_bounds__(BLK_THREADS) k_retime(const RetimeArgs A)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const WaveBlock w = wave_block(A.wb);
    if (w.none) return;
    const int wave = w.wave, lane = w.lane, bj = w.bj, bi = w.bi;
    const int B = BS ? BS : A.bs;
    const int sw = A.sw, pnorm = A.pnorm;
    const int x0 = bj * B, y0 = bi * B;
    const int32_t* row = A.table + (long long)w.z * RT_ROW;
    const int32_t* a_of = row + RT_A + RT_MAX_SW;                // a(V) at a_of[V]
    const uint8_t* past = A.frames + (long long)row[RT_PLANE] * A.stride;
    const uint8_t* next = past + A.stride;
    const int pmin = a_of[sw] >> 2, pmax = a_of[-sw] >> 2, bmin = pmax - sw, bmax = pmin + sw;
    const int ps = B + pmax - pmin, ns = B + bmax - bmin;        // the sides of the two windows
    const int pwd = window_row_dwords(ps), nwd = window_row_dwords(ns);
    const uint32_t recip_pwd = (uint32_t)row[RT_RECIP_ROW], recip_nwd = (uint32_t)row[RT_RECIP_ROW + 1];
    uint32_t* pw = (uint32_t*)(lds + (size_t)wave * A.wave_lds);
    uint32_t* nw = pw + window_bytes(ps) / 4;
    const int nd = row_dwords(B), n1 = 2 * sw + 1;
    const uint32_t tail = tail_mask(B);
    constexpr bool TAIL = !BS || (BS & 3);                       // the last dword of a row may hold bytes beyond the block

    Least best;
    for (int cls = 0; cls < 16; ++cls) {
        const int fx = cls >> 2, fy = cls & 3;
        const int xs = row[RT_START + fx], nx = row[RT_START + fx + 1] - xs;
        const int ys = row[RT_START + fy], ny = row[RT_START + fy + 1] - ys;
        if (nx == 0 || ny == 0) continue;
        wave_lds_fence();                                    // the last class's reads are behind the writes below
        stage_quarter(pw, ps, pwd, recip_pwd, past, A.pitch, A.H, A.W, y0 + pmin, x0 + pmin, fx, fy, lane);
        stage_quarter(nw, ns, nwd, recip_nwd, next, A.pitch, A.H, A.W, y0 + bmin, x0 + bmin, fx, fy, lane);
        wave_lds_fence();
        const int ncand = nx * ny;
        const uint32_t recip_ny = (uint32_t)row[RT_RECIP_COUNT + fy];
        const LaneSplit ls(lanes_for_one_round(ncand), lane);
        for (int c0 = 0; c0 < ncand; c0 += ls.slots) {
            const int c = c0 + ls.slot;
            const bool listed = c < ncand;                   // lanes beyond the list score candidate 0 and drop it
            const int cc = listed ? c : 0;
            const int ix = ny == 1 ? cc : div_recip(cc, recip_ny), iy = cc - ix * ny;
            const int Vx = row[RT_PERM + xs + ix], Vy = row[RT_PERM + ys + iy];
            const int ax = a_of[Vx] >> 2, ay = a_of[Vy] >> 2;
            const int px = ax - pmin, py = ay - pmin;        // the candidate's block in the past window (column, row)
            const int qx = ax + Vx - bmin, qy = ay + Vy - bmin;      // ... and in the next window
            const uint32_t psh = (uint32_t)px & 3u, qsh = (uint32_t)qx & 3u;
            RowScore s;
            for (int y = ls.q; y < B; y += ls.P) {
                const uint32_t* prow = pw + (py + y) * pwd + (px >> 2);
                const uint32_t* qrow = nw + (qy + y) * nwd + (qx >> 2);
#pragma unroll 4
                for (int k = 0; k < nd; ++k) {
                    uint32_t a = window_dword(prow, k, psh);
                    uint32_t v = window_dword(qrow, k, qsh);
                    if (TAIL) { if (k == nd - 1) { a &= tail; v &= tail; } }
                    s.add(a, v, pnorm);
                }
            }
            const uint32_t j = ls.sum(s.value(pnorm)) + A.bias * (uint32_t)(abs(Vx) + abs(Vy));
            // the order of the definition: 0 for the centre, 1 + index in [-sw, sw]^2 (column offset outer) for the others
            const uint32_t order = (Vx | Vy) == 0 ? 0u : 1u + (uint32_t)((Vx + sw) * n1 + (Vy + sw));
            if (listed) best.take(j, order);
        }
    }
    const Least win = wave_least(best.cost, best.order);
    if (lane == 0) {
        int vx = 0, vy = 0;
        if (win.order != 0u) {
            vx = ((int)win.order - 1) / n1;
            vy = (int)win.order - 1 - vx * n1 - sw;
            vx -= sw;
        }
        const long long blk = ((long long)w.z * A.hb + bi) * A.wb + bj;
        A.mv[blk * 2] = vx;
        A.mv[blk * 2 + 1] = vy;
        A.cost[blk] = (long long)win.cost;
        A.dist[blk] = (long long)(win.cost - A.bias * (uint32_t)(abs(vx) + abs(vy)));
    }
}

// The pixel of k_retime_frame.  Output pixel (u, v) of block (v / bs, u / bs) inside the hb x wb grid is the blend of `past` at
// (4 u + a(Vx), 4 v + a(Vy)) and `next` at (4 u + b(Vx), 4 v + b(Vy)) quarter pixels; beyond the last whole block the vector is
// zero.
struct RetimePixel {
    const uint8_t* p;             // the output's `past` and `next` planes
    const uint8_t* q;
    const int32_t* mv;            // its vectors [hb][wb][2]
    const int32_t* a_of;          // a(V) at a_of[V], V = -16 .. 16
    int H, W, pitch, bs, hb, wb, n, d;
    uint32_t recip_d;
    __device__ __forceinline__ int operator()(int u, int v) const
    {
        const int i = v / bs, j = u / bs;
        int Vx = 0, Vy = 0;
        if (i < hb && j < wb) {
            const long long b = (long long)i * wb + j;
            Vx = min(max(mv[b * 2], -RT_MAX_SW), RT_MAX_SW);     // k_retime's vectors lie within the window: the clamp keeps
            Vy = min(max(mv[b * 2 + 1], -RT_MAX_SW), RT_MAX_SW); // the table index in range whatever the buffer holds
        }
        const int ax = a_of[Vx], ay = a_of[Vy];
        const int P = quarter_sample(p, pitch, H, W, 4 * u + ax, 4 * v + ay);
        const int N = quarter_sample(q, pitch, H, W, 4 * u + ax + 4 * Vx, 4 * v + ay + 4 * Vy);
        return div_recip((d - n) * P + n * N + (d >> 1), recip_d);
    }
};

// the row frame of bbme_predict.h, one plane per output; `cur` is the first true frame (they lie cur_stride apart), or any plane
// where there is none (the squared error is then not used)
__global__ void __launch_bounds__(PRED_THREADS) k_retime_frame(const uint8_t* frames, long long plane_stride, const int32_t* table,
                                                               const uint8_t* cur, long long cur_stride, int H, int W, int pitch, int bs,
                                                               int hb, int wb, const int32_t* mv, uint8_t* out, long long out_stride,
                                                               int out_pitch, unsigned long long* sse)
{
    const int f = blockIdx.z;
    const int32_t* row = table + (long long)f * RT_ROW;
    const uint8_t* past = frames + (long long)row[RT_PLANE] * plane_stride;
    const RetimePixel px = { past, past + plane_stride, mv + (long long)f * hb * wb * 2, row + RT_A + RT_MAX_SW, H, W, pitch, bs, hb, wb,
                             row[RT_N], row[RT_D], (uint32_t)row[RT_RECIP_D] };
    predict_rows(px, cur + (long long)f * cur_stride, H, W, pitch, out + (long long)f * out_stride, out_pitch, sse + f);
}

}  // namespace

// the argument rules of retime.py
int retime_check_args(const char* who, int H, int W, int bs, int sw, int pnorm, int bias)
{
    GME_REQUIRE(bs >= RT_MIN_BS && bs <= RT_MAX_BS, GME_ERR_ARG, "%s: block_size %d (%d .. %d)", who, bs, RT_MIN_BS, RT_MAX_BS);
    GME_REQUIRE(sw >= 0 && sw <= RT_MAX_SW, GME_ERR_ARG, "%s: search_window %d (0 .. %d)", who, sw, RT_MAX_SW);
    if (int rc = require_pnorm(who, pnorm)) return rc;
    GME_REQUIRE(bias >= 0 && bias <= RT_MAX_BIAS, GME_ERR_ARG, "%s: bias %d (0 .. 2^16)", who, bias);
    GME_REQUIRE(H >= bs && W >= bs, GME_ERR_ARG, "%s: a %d x %d frame holds no block of %d", who, H, W, bs);
    return GME_OK;
}

// retime.check_phase: n / d reduced in place
int retime_check_phase(const char* who, int* n, int* d)
{
    GME_REQUIRE(*d >= 1 && *n >= 1 && *n < *d, GME_ERR_ARG, "%s: phase %d/%d (0 < n / d < 1)", who, *n, *d);
    int a = *n, b = *d;
    while (b) { const int t = a % b; a = b; b = t; }
    GME_REQUIRE(*d / a <= RT_MAX_D, GME_ERR_ARG, "%s: phase %d/%d: denominator above %d", who, *n / a, *d / a, RT_MAX_D);
    *n /= a; *d /= a;
    return GME_OK;
}

int retime_row_ints() { return RT_ROW; }

// the table row of one output: `past` is plane `plane`, the phase n / d is reduced and checked; -> the LDS its wave needs
int retime_row(int32_t* row, int plane, int n, int d, int bs, int sw)
{
    for (int k = 0; k < RT_ROW; ++k) row[k] = 0;
    row[RT_PLANE] = plane; row[RT_N] = n; row[RT_D] = d;
    row[RT_RECIP_D] = (int32_t)recip32(d);
    for (int V = -RT_MAX_SW; V <= RT_MAX_SW; ++V) row[RT_A + RT_MAX_SW + V] = retime_a(V, n, d);
    int at = 0;
    for (int f = 0; f < 4; ++f) {
        row[RT_START + f] = at;
        for (int V = -sw; V <= sw; ++V)
            if ((retime_a(V, n, d) & 3) == f) row[RT_PERM + at++] = V;
        const int count = at - row[RT_START + f];
        row[RT_RECIP_COUNT + f] = count >= 2 ? (int32_t)recip32(count) : 0;
    }
    row[RT_START + 4] = at;
    const RetimeSpan s = retime_span(sw, n, d);
    row[RT_RECIP_ROW] = (int32_t)recip32(window_row_dwords(bs + s.pmax - s.pmin));
    row[RT_RECIP_ROW + 1] = (int32_t)recip32(window_row_dwords(bs + s.bmax - s.bmin));
    return retime_wave_lds(bs, sw, n, d);
}

// retime.search of `outputs` outputs under their table rows (device; wave_lds the largest retime_row of them): output k reads
// the planes row[RT_PLANE] and the next of the stack at `frames`; mv [outputs][hb][wb][2], cost and dist [outputs][hb][wb]
// (device), hb = H / bs and wb = W / bs
int launch_retime(gme_ctx* ctx, const uint8_t* frames, long long plane_stride, int outputs, int H, int W, int pitch, int bs, int sw,
                  int pnorm, int bias, const int32_t* table, int wave_lds, int32_t* mv, long long* cost, long long* dist)
{
    int rc = retime_check_args("frame retiming", H, W, bs, sw, pnorm, bias);
    if (rc) return rc;
    const int hb = H / bs, wb = W / bs;
    const bool compiled = bs == 16 || bs == 32;
    GME_REQUIRE(wave_lds > 0 && BLK_WAVES * wave_lds <= 64 * 1024, GME_ERR_ARG, "frame retiming: %d bytes of LDS to a wave", wave_lds);
    RetimeArgs a;
    a.frames = frames; a.stride = plane_stride; a.H = H; a.W = W; a.pitch = pitch;
    a.hb = hb; a.wb = wb; a.bs = bs; a.sw = sw; a.pnorm = pnorm; a.bias = (uint32_t)bias;
    a.wave_lds = wave_lds;
    const long long per = (long long)hb * wb;
    auto note = [&] {
        if (compiled) plan_note(ctx, 0, "k_retime<%d> sw %d bias %d, %d x %d blocks, one wave each", bs, sw, bias, hb, wb);
        else plan_note(ctx, 0, "k_retime<0> bs %d sw %d bias %d, %d x %d blocks, one wave each", bs, sw, bias, hb, wb);
    };
    return launch_wave_blocks(ctx, outputs, hb, wb, wave_lds, a, note, [&](int k) {           // H, W >= bs: there are blocks
        a.table = table + (long long)k * RT_ROW;
        a.mv = mv + per * k * 2; a.cost = cost + per * k; a.dist = dist + per * k;
        return !compiled ? k_retime<0> : bs == 16 ? k_retime<16> : k_retime<32>;
    });
}

// out planes = retime.interpolate of each output's planes by mv [outputs][H / bs][W / bs][2], sse[outputs] (device, zeroed here) =
// squared error of each against its `cur` plane (cur + k * cur_stride; any plane where there is no true frame)
int launch_retime_frame(gme_ctx* ctx, const uint8_t* frames, long long plane_stride, int outputs, int H, int W, int pitch, int bs,
                        const int32_t* table, const int32_t* mv, const uint8_t* cur, long long cur_stride, uint8_t* out,
                        long long out_stride, int out_pitch, unsigned long long* sse)
{
    if (outputs == 0) return GME_OK;
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    const int hb = H / bs, wb = W / bs;
    const long long per = (long long)hb * wb;
    return predict_planes(ctx, outputs, sse, [&](int k, int n) {
        hipLaunchKernelGGL(k_retime_frame, predict_grid(H, W, n), dim3(PRED_THREADS), 0, ctx->stream, frames, plane_stride,
                           table + (long long)k * RT_ROW, cur + (long long)k * cur_stride, cur_stride, H, W, pitch, bs, hb, wb,
                           mv + per * k * 2, out + (long long)k * out_stride, out_stride, out_pitch, sse + k);
    });
}
