// Bidirectional block prediction (host definition: bipred.py).  A block of the frame `mid` is predicted
// from the frame before it (`past`, vector f0), from the frame after it (`next`, vector f1) or from the rounded average of
// both, whichever costs least; the pair of vectors behind the average is refined in alternating passes of +-radius.  A block
// depends on no neighbour and every candidate of every pass is always scored, so the work is fixed whatever the content.
// Everything is integer: the device equals bipred.decide and bipred.predict byte for byte.
//
// Kernels:
//   k_bipred<BS>        one wave per block, four blocks to a 256-thread workgroup, each wave on its own LDS slice (no workgroup
//                       barrier).  The wave stages the BS x BS block of `mid` and the (BS + 2 rounds r)^2 windows of `past`
//                       around f0 and of `next` around f1 once: a centre moves by at most r per pass, so every candidate of
//                       every pass lies in them.  The three starting costs share one sweep over the block's dwords.  A pass
//                       spreads its candidates over the lanes, BP_P lanes to the rows of one candidate; a row is scored four
//                       bytes at a time (v_alignbyte for both references, v_lerp_u8 for the four rounded averages, then
//                       v_sad_u8, or three v_dot4 for aa + bb - 2ab).  A 64 x 64 MSE cost needs 29 bits, so cost and candidate
//                       order do not share a 32-bit key: a pass ends with two wave reductions, the least cost and then the
//                       least order among the lanes that hold it (the incumbent has order 0, so a tie keeps it).  The passes
//                       depend on each other and all run in the one wave; the vectors stay in scalar registers.  <16> and <32>
//                       are compiled; <0> takes the block size at run time (and rows that are no multiple of four bytes).
//   k_predict_bipred    bipred.predict per pixel, with the squared error of each predicted frame against its `mid`
#include "bbme_predict.h"
#include "bbme_wave_lds.h"
#include "gme_passes.h"

namespace {

constexpr int BP_MIN_BS = 4, BP_MAX_BS = 64, BP_MAX_R = 2, BP_MAX_ROUNDS = 2, BP_MAX_PENALTY = 1 << 30;
constexpr int BP_P = 8;                                         // lanes to a candidate, whatever the radius: 64 / BP_P scored at once
constexpr int BP_MAX_CAND = (2 * BP_MAX_R + 1) * (2 * BP_MAX_R + 1);
constexpr long long BP_MAX_COST = (long long)BP_MAX_BS * BP_MAX_BS * 65025ll;
static_assert(BP_MAX_COST < (long long)NO_COST, "a cost in 32 bits, below the sentinel");
// the order of a candidate needs 5 bits beside a cost of 29: no 32-bit key, hence the two reductions of a pass
static_assert(BP_MAX_CAND + 1 <= (1 << 5) && (BP_MAX_COST << 5) >= (1ll << 32), "cost and order in one 32-bit key");
// every sum of a decision in 32 bits
static_assert((long long)BP_MAX_PENALTY + BP_MAX_COST < (1ll << 31), "31-bit decisions");
constexpr int BP_MAX_WINDOW = BP_MAX_BS + 2 * BP_MAX_ROUNDS * BP_MAX_R;
static_assert(small_div_covers(BP_MAX_WINDOW, window_row_dwords(BP_MAX_WINDOW), 2 * BP_MAX_R + 1), "range of small_div");
// a workgroup's LDS without an opt-in: the block and both windows of four waves
static_assert(BLK_WAVES * (block_bytes(BP_MAX_BS) + 2 * window_bytes(BP_MAX_WINDOW)) <= 64 * 1024, "LDS of a workgroup");

struct BipredArgs {
    const uint8_t* past;          // first plane of each role; target k reads the planes k * stride bytes on
    const uint8_t* mid;
    const uint8_t* next;
    long long stride;
    int H, W, pitch;
    const int32_t* f0;            // [targets][hb][wb][2]
    const int32_t* f1;
    uint8_t* mode;                // [targets][hb][wb]
    int32_t* v0;                  // [targets][hb][wb][2]
    int32_t* v1;
    long long* cost;              // [targets][hb][wb]
    long long* costs;             // [targets][hb][wb][3]
    int hb, wb, bs, radius, rounds, pnorm;
    uint32_t penalty;
    int anchor_bytes, window_bytes, slice_bytes;      // LDS of a wave: the block of mid, the window of past, the window of next
};

constexpr uint32_t BP_ROUND_UP = 0x01010101u;                   // v_lerp_u8's third operand: (p + n + 1) >> 1 in every byte

template <int BS>
__global__ void __launch_bounds__(BLK_THREADS) k_bipred(const BipredArgs A)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const WaveBlock w = wave_block(A.wb);
    if (w.none) return;
    const int wave = w.wave, lane = w.lane, bj = w.bj, bi = w.bi, target = w.z;
    const int B = BS ? BS : A.bs;
    const int r = A.radius, pnorm = A.pnorm;
    const Square sq(r);
    const int m = A.rounds * r;                                  // how far a refined vector can lie from its input
    const long long blk = ((long long)target * A.hb + bi) * A.wb + bj;
    const int ax = __builtin_amdgcn_readfirstlane(A.f0[blk * 2]), ay = __builtin_amdgcn_readfirstlane(A.f0[blk * 2 + 1]);
    const int bx = __builtin_amdgcn_readfirstlane(A.f1[blk * 2]), by = __builtin_amdgcn_readfirstlane(A.f1[blk * 2 + 1]);
    const int x0 = bj * B, y0 = bi * B;
    const long long pxl = (long long)x0 + ax, pyl = (long long)y0 + ay, nxl = (long long)x0 + bx, nyl = (long long)y0 + by;
    const bool in0 = pxl >= 0 && pyl >= 0 && pxl + B <= A.W && pyl + B <= A.H;
    const bool in1 = nxl >= 0 && nyl >= 0 && nxl + B <= A.W && nyl + B <= A.H;
    const bool both = in0 && in1;
    if (!in0 && !in1) {                                          // nothing to predict from: mode 3, the vectors as they came
        if (lane == 0) {
            A.mode[blk] = 3;
            A.v0[blk * 2] = ax; A.v0[blk * 2 + 1] = ay;
            A.v1[blk * 2] = bx; A.v1[blk * 2 + 1] = by;
            A.cost[blk] = -1;
            A.costs[blk * 3] = -1; A.costs[blk * 3 + 1] = -1; A.costs[blk * 3 + 2] = -1;
        }
        return;
    }
    // the displaced blocks in their frames (meaningful where the vector is inside)
    const int px = (int)pxl, py = (int)pyl, nx = (int)nxl, ny = (int)nyl;

    uint32_t* anc = (uint32_t*)(lds + (size_t)wave * A.slice_bytes);
    uint32_t* pw = (uint32_t*)(lds + (size_t)wave * A.slice_bytes + A.anchor_bytes);
    uint32_t* nw = (uint32_t*)(lds + (size_t)wave * A.slice_bytes + A.anchor_bytes + A.window_bytes);
    const int nd = row_dwords(B), ws = B + 2 * m, wd = window_row_dwords(ws);
    const uint32_t tail = tail_mask(B);
    constexpr bool TAIL = !BS || (BS & 3);                       // the last dword of a row may hold bytes beyond the block
    const long long plane = (long long)target * A.stride;
    stage_bytes(anc, B, nd, B, A.mid + plane, A.pitch, A.H, A.W, y0, x0, lane);
    if (in0) stage_bytes(pw, ws, wd, ws, A.past + plane, A.pitch, A.H, A.W, py - m, px - m, lane);
    if (in1) stage_bytes(nw, ws, wd, ws, A.next + plane, A.pitch, A.H, A.W, ny - m, nx - m, lane);
    wave_lds_fence();

    // the starting costs: the block's (row, dword) pairs over the lanes, every dword read once for all three
    uint32_t c0 = NO_COST, c1 = NO_COST, cb = NO_COST;
    {
        RowScore s0, s1, sb;
        for (int t = lane; t < B * nd; t += 64) {
            const int y = small_div(t, nd), k = t - y * nd;
            const uint32_t a = anc[t];                           // bytes at and past column B are zero
            const int at = (m + y) * wd + (m >> 2) + k;
            uint32_t p = 0, q = 0;
            if (in0) p = window_dword(pw, at, (uint32_t)m & 3u);
            if (in1) q = window_dword(nw, at, (uint32_t)m & 3u);
            if (TAIL) { if (k == nd - 1) { p &= tail; q &= tail; } }
            if (in0) s0.add(a, p, pnorm);
            if (in1) s1.add(a, q, pnorm);
            if (both) sb.add(a, __builtin_amdgcn_lerp(p, q, BP_ROUND_UP), pnorm);   // masked bytes average to (0 + 0 + 1) >> 1 = 0
        }
        if (in0) c0 = wave_sum_u32(s0.value(pnorm));
        if (in1) c1 = wave_sum_u32(s1.value(pnorm));
        if (both) cb = wave_sum_u32(sb.value(pnorm));
    }

    // the refined vectors minus their inputs, wave-uniform: |.| <= (passes of that side so far) * r <= m
    int r0x = 0, r0y = 0, r1x = 0, r1y = 0;
    if (both && r > 0) {
        const LaneSplit ls(BP_P, lane);
#pragma unroll 1
        for (int pass = 0; pass < 2 * A.rounds; ++pass) {
            const bool side = pass & 1;                          // 0: the past vector moves, 1: the next vector
            const uint32_t* mw = side ? nw : pw;                 // the moving side's window, the held side's window
            const uint32_t* hw = side ? pw : nw;
            const int cx = side ? r1x : r0x, cy = side ? r1y : r0y;              // the centre, relative
            const int hx = m + (side ? r0x : r1x), hy = m + (side ? r0y : r1y);  // the held block in its window
            const int ox0 = side ? nx : px, oy0 = side ? ny : py;                // the moving side's input block in the frame
            const uint32_t hsh = (uint32_t)hx & 3u;
            uint32_t bestc = cb, besto = 0;                      // the incumbent: order 0
            for (int i0 = 0; i0 < sq.ncand; i0 += ls.slots) {
                const int c = i0 + ls.slot;
                int ox, oy;                                      // the candidate's offset + r (column, row); lanes beyond
                sq.at(c < sq.ncand ? c : 0, &ox, &oy);           // the list score candidate 0 and drop it
                const bool listed = c < sq.ncand && !sq.centre(ox, oy);          // the centre is the incumbent
                const int dx = cx + ox - r, dy = cy + oy - r;    // within [-m, m] of the input vector
                const int gx = ox0 + dx, gy = oy0 + dy;          // the candidate's block in the frame
                const bool ok = listed && gx >= 0 && gy >= 0 && gx + B <= A.W && gy + B <= A.H;
                const int wx = m + dx, wy = m + dy;              // ... and in the window: 0 <= wx, wx + B <= ws
                const uint32_t wsh = (uint32_t)wx & 3u;
                RowScore s;
                for (int y = ls.q; y < B; y += BP_P) {
                    const uint32_t* arow = anc + y * nd;
                    const uint32_t* mrow = mw + (wy + y) * wd + (wx >> 2);
                    const uint32_t* hrow = hw + (hy + y) * wd + (hx >> 2);
#pragma unroll 4
                    for (int k = 0; k < nd; ++k) {
                        const uint32_t u = window_dword(mrow, k, wsh);
                        const uint32_t h = window_dword(hrow, k, hsh);
                        uint32_t v = __builtin_amdgcn_lerp(u, h, BP_ROUND_UP);
                        if (TAIL) { if (k == nd - 1) v &= tail; }
                        s.add(arow[k], v, pnorm);
                    }
                }
                const uint32_t cost = ls.sum(s.value(pnorm));
                // a lane meets its candidates in ascending order, so "strictly smaller" keeps the first of equal costs
                if (ok && cost < bestc) { bestc = cost; besto = sq.order_beside_centre(c); }
            }
            const Least win = wave_least(bestc, besto);
            if (win.order != 0u) {
                int ox, oy;
                sq.offset(win.order, &ox, &oy);
                if (side) { r1x += ox; r1y += oy; }
                else { r0x += ox; r0y += oy; }
                cb = win.cost;
            }
        }
    }

    if (lane == 0) {
        // (mode 0, c0), (mode 1, c1), (mode 2, cb + penalty) in that order, only a strictly smaller value replaces the best
        uint32_t best = NO_COST;
        int mode = 3;
        if (in0) { mode = 0; best = c0; }
        if (in1 && (mode == 3 || c1 < best)) { mode = 1; best = c1; }
        if (both && cb + A.penalty < best) { mode = 2; best = cb + A.penalty; }
        const bool refined = mode == 2;
        A.mode[blk] = (uint8_t)mode;
        A.v0[blk * 2] = ax + (refined ? r0x : 0); A.v0[blk * 2 + 1] = ay + (refined ? r0y : 0);
        A.v1[blk * 2] = bx + (refined ? r1x : 0); A.v1[blk * 2 + 1] = by + (refined ? r1y : 0);
        A.cost[blk] = (long long)best;
        A.costs[blk * 3] = in0 ? (long long)c0 : -1;
        A.costs[blk * 3 + 1] = in1 ? (long long)c1 : -1;
        A.costs[blk * 3 + 2] = both ? (long long)cb : -1;
    }
}

// The pixel of k_predict_bipred.  Output pixel (u, v) of block (v / bs, u / bs) inside the hb x wb grid is the pixel of `past` at
// (u + v0x, v + v0y) in mode 0, of `next` at (u + v1x, v + v1y) in mode 1 and their rounded average in mode 2; in mode 3, beyond
// the last whole block, and wherever a pixel it would read lies outside the frame (never with the modes of k_bipred), the
// co-located pixel of `past`.
struct BipredPixel {
    const uint8_t* p;             // the target's `past` and `next` planes
    const uint8_t* q;
    const uint8_t* mode;          // its modes [hb][wb] and vector pairs [hb][wb][2]
    const int32_t* v0;
    const int32_t* v1;
    int H, W, pitch, bs, hb, wb;
    __device__ __forceinline__ int operator()(int u, int v) const
    {
        const int i = v / bs, j = u / bs;
        int o = p[(long long)v * pitch + u];
        if (i < hb && j < wb) {
            const long long b = (long long)i * wb + j;
            const int md = mode[b];
            const long long pu = (long long)u + v0[b * 2], pv = (long long)v + v0[b * 2 + 1];
            const long long qu = (long long)u + v1[b * 2], qv = (long long)v + v1[b * 2 + 1];
            const bool pin = pu >= 0 && pu < W && pv >= 0 && pv < H, qin = qu >= 0 && qu < W && qv >= 0 && qv < H;
            if (md == 0 && pin) o = p[pv * pitch + pu];
            else if (md == 1 && qin) o = q[qv * pitch + qu];
            else if (md == 2 && pin && qin) o = ((int)p[pv * pitch + pu] + (int)q[qv * pitch + qu] + 1) >> 1;
        }
        return o;
    }
};

// the row frame of bbme_predict.h, one plane per target
__global__ void __launch_bounds__(PRED_THREADS) k_predict_bipred(const uint8_t* past, const uint8_t* mid, const uint8_t* next,
                                                                 long long plane_stride, int H, int W, int pitch, int bs, int hb, int wb,
                                                                 const uint8_t* mode, const int32_t* v0, const int32_t* v1, uint8_t* out,
                                                                 long long out_stride, int out_pitch, unsigned long long* sse)
{
    const int f = blockIdx.z;
    const long long plane = (long long)f * plane_stride, blocks = (long long)f * hb * wb;
    const BipredPixel px = { past + plane, next + plane, mode + blocks, v0 + blocks * 2, v1 + blocks * 2, H, W, pitch, bs, hb, wb };
    predict_rows(px, mid + plane, H, W, pitch, out + (long long)f * out_stride, out_pitch, sse + f);
}

}  // namespace

// the argument rules of bipred.py
int bipred_check_args(const char* who, int bs, int radius, int rounds, int pnorm, int penalty)
{
    GME_REQUIRE(bs >= BP_MIN_BS && bs <= BP_MAX_BS, GME_ERR_ARG, "%s: block_size %d (%d .. %d)", who, bs, BP_MIN_BS, BP_MAX_BS);
    GME_REQUIRE(radius >= 0 && radius <= BP_MAX_R, GME_ERR_ARG, "%s: radius %d (0 .. %d)", who, radius, BP_MAX_R);
    GME_REQUIRE(rounds >= 0 && rounds <= BP_MAX_ROUNDS, GME_ERR_ARG, "%s: rounds %d (0 .. %d)", who, rounds, BP_MAX_ROUNDS);
    if (int rc = require_pnorm(who, pnorm)) return rc;
    GME_REQUIRE(penalty >= 0 && penalty <= BP_MAX_PENALTY, GME_ERR_ARG, "%s: penalty %d (0 .. 2^30)", who, penalty);
    return GME_OK;
}

// bipred.decide of `targets` triples: target k reads the planes past + k * plane_stride, mid + k * plane_stride and
// next + k * plane_stride and the fields f0[k], f1[k] of [hb][wb][2], hb = H / bs and wb = W / bs; mode [targets][hb][wb], v0 and
// v1 [targets][hb][wb][2], cost [targets][hb][wb] and costs [targets][hb][wb][3] (device)
int launch_bipred(gme_ctx* ctx, const uint8_t* past, const uint8_t* mid, const uint8_t* next, long long plane_stride, int targets,
                  int H, int W, int pitch, int bs, int radius, int rounds, int pnorm, int penalty, const int32_t* f0, const int32_t* f1,
                  uint8_t* mode, int32_t* v0, int32_t* v1, long long* cost, long long* costs)
{
    int rc = bipred_check_args("bidirectional prediction", bs, radius, rounds, pnorm, penalty);
    if (rc) return rc;
    const int hb = H / bs, wb = W / bs;
    const bool compiled = bs == 16 || bs == 32;
    BipredArgs a;
    a.stride = plane_stride; a.H = H; a.W = W; a.pitch = pitch;
    a.hb = hb; a.wb = wb; a.bs = bs; a.radius = radius; a.rounds = rounds; a.pnorm = pnorm; a.penalty = (uint32_t)penalty;
    a.anchor_bytes = block_bytes(bs);
    a.window_bytes = window_bytes(bs + 2 * rounds * radius);
    a.slice_bytes = a.anchor_bytes + 2 * a.window_bytes;
    const long long per = (long long)hb * wb;
    auto note = [&] {
        if (compiled) plan_note(ctx, 0, "k_bipred<%d> r %d rounds %d penalty %d, %d x %d blocks, one wave each", bs, radius, rounds, penalty, hb, wb);
        else plan_note(ctx, 0, "k_bipred<0> bs %d r %d rounds %d penalty %d, %d x %d blocks, one wave each", bs, radius, rounds, penalty, hb, wb);
    };
    return launch_wave_blocks(ctx, targets, hb, wb, a.slice_bytes, a, note, [&](int k) {
        const long long off = (long long)k * plane_stride;
        a.past = past + off; a.mid = mid + off; a.next = next + off;
        a.f0 = f0 + per * k * 2; a.f1 = f1 + per * k * 2;
        a.mode = mode + per * k; a.v0 = v0 + per * k * 2; a.v1 = v1 + per * k * 2;
        a.cost = cost + per * k; a.costs = costs + per * k * 3;
        return !compiled ? k_bipred<0> : bs == 16 ? k_bipred<16> : k_bipred<32>;
    });
}

// out planes = bipred.predict of the past and next planes by mode, v0 and v1 of [targets][H / bs][W / bs], sse[targets] (device,
// zeroed here) = squared error of each against its mid plane
int launch_predict_bipred(gme_ctx* ctx, const uint8_t* past, const uint8_t* mid, const uint8_t* next, long long plane_stride,
                          int targets, int H, int W, int pitch, int bs, const uint8_t* mode, const int32_t* v0, const int32_t* v1,
                          uint8_t* out, long long out_stride, int out_pitch, unsigned long long* sse)
{
    if (targets == 0) return GME_OK;
    GME_REQUIRE(bs >= 1, GME_ERR_ARG, "block_size %d", bs);
    const int hb = H / bs, wb = W / bs;
    const long long per = (long long)hb * wb;
    return predict_planes(ctx, targets, sse, [&](int k, int n) {
        const long long off = (long long)k * plane_stride;
        hipLaunchKernelGGL(k_predict_bipred, predict_grid(H, W, n), dim3(PRED_THREADS), 0, ctx->stream, past + off, mid + off, next + off,
                           plane_stride, H, W, pitch, bs, hb, wb, mode + per * k, v0 + per * k * 2, v1 + per * k * 2,
                           out + (long long)k * out_stride, out_stride, out_pitch, sse + k);
    });
}
