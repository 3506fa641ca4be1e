// Hierarchical block matching (host definition: hier.py).  Block (i, j) exists at every pyramid level with
// half the side of the level below and depends on no neighbour, so its whole coarse-to-fine search runs in one wave of one
// kernel: +-coarse_window around (0, 0) at the coarsest level used, then +-radius around twice the parent vector at each finer
// level.  Everything is integer: the device equals hier.search bit for bit.
//
// Kernel:
//   k_hier<BS, LEVELS>  one wave per block, four blocks to a 256-thread workgroup, each wave on its own LDS slice (no workgroup
//                       barrier).  Per level the wave stages the anchor block and the (b + 2R)^2 window of `current` around
//                       the clamped centre in LDS, a dword per lane and step; spreads the (2R + 1)^2 candidates over its
//                       lanes (P lanes share the rows of one candidate where there are fewer than 33); scores a row four
//                       bytes at a time (v_alignbyte on two window dwords, then v_sad_u8, or three v_dot4 for
//                       aa + bb - 2ab); and selects the minimum of (cost, position in the definition's order, centre = 0)
//                       in two wave-wide minima.  BS, LEVELS: the halving chains 16-8-4, 32-16-8 and 64-32-16 as
//                       compile-time constants; <0, 0> takes block size and level count at run time (and rows that are no
//                       multiple of four bytes).
#include <type_traits>

#include "bbme_wave_lds.h"
#include "gme_passes.h"

namespace {

constexpr int HIER_MAX_BS = 64, HIER_MAX_CW = 8, HIER_MAX_R = 3, HIER_MIN_TOP = 4;
// costs are 32-bit in the kernel (int64 at the ABI): the largest is 64 * 64 * 255^2
static_assert((long long)HIER_MAX_BS * HIER_MAX_BS * 65025ll < (1ll << 28), "28-bit block costs");
// the order of a candidate within a level: 0 for the centre, 1 + index in [-R, R]^2 (column offset outer) for the others
static_assert((2 * HIER_MAX_CW + 1) * (2 * HIER_MAX_CW + 1) < (1 << 9), "9-bit candidate order");

struct HierLevel {
    const uint8_t* prev;          // first "previous" plane of the level
    const uint8_t* cur;           // first "current" plane
    long long stride;             // bytes between consecutive pairs' planes
    int H, W, pitch, pad;
    int32_t* mf;                  // [pairs][hb][wb][2]
    long long* cost;              // [pairs][hb][wb]
};
struct HierArgs {
    HierLevel lv[3];              // [2] = full resolution; levels below the first one used are not read
    int hb, wb, bs, levels, cw, radius, pnorm;
    int anchor_bytes;             // LDS of a wave: the anchor block (rows of round_up(b, 4) bytes), then the window
    int slice_bytes;
};

constexpr int HIER_MAX_WINDOW = HIER_MAX_BS + 2 * HIER_MAX_CW;
static_assert(small_div_covers(HIER_MAX_WINDOW, window_row_dwords(HIER_MAX_WINDOW), 2 * HIER_MAX_CW + 1), "range of small_div");

// One level of one block: centre (cx, cy) already clamped, candidates within R of it; the level's vector into (vx, vy), its
// cost returned.  B: the block side where it is a compile-time constant (0: b_rt).
template <int B>
__device__ __forceinline__ uint32_t level_search(const HierLevel& L, int pair, int b_rt, int R, int pnorm, int bi, int bj, int cx,
                                                 int cy, uint32_t* anc, uint32_t* win, int lane, int* vx, int* vy)
{
    const int b = B ? B : b_rt;
    const Square sq(R);
    const int nd = row_dwords(b), wside = b + 2 * R, wd = window_row_dwords(wside);
    const int x0 = bj * b, y0 = bi * b;
    const uint8_t* pp = L.prev + (long long)pair * L.stride;
    const uint8_t* cp = L.cur + (long long)pair * L.stride;
    stage_bytes(anc, b, nd, b, pp, L.pitch, L.H, L.W, y0, x0, lane);
    stage_bytes(win, wside, wd, wside, cp, L.pitch, L.H, L.W, y0 + cy - R, x0 + cx - R, lane);
    wave_lds_fence();

    const LaneSplit ls(lanes_for_one_round(sq.ncand), lane);
    const uint32_t tail = tail_mask(b);
    Least best;
    for (int c0 = 0; c0 < sq.ncand; c0 += ls.slots) {
        const int c = c0 + ls.slot;
        const bool listed = c < sq.ncand;
        int wx, wy;                                               // the candidate's origin in the window (column, row)
        sq.at(listed ? c : 0, &wx, &wy);
        const int gx = x0 + cx - R + wx, gy = y0 + cy - R + wy;   // ... and in the level
        const bool inside = listed && gx >= 0 && gy >= 0 && gx + b <= L.W && gy + b <= L.H;
        const uint32_t sh = (uint32_t)wx & 3u;
        RowScore s;
        for (int y = ls.q; y < b; y += ls.P) {
            const uint32_t* arow = anc + y * nd;
            const uint32_t* wrow = win + (wy + y) * wd + (wx >> 2);
#pragma unroll 4
            for (int k = 0; k < nd; ++k) {
                uint32_t v = window_dword(wrow, k, sh);
                if (!B || (B & 3)) { if (k == nd - 1) v &= tail; }
                s.add(arow[k], v, pnorm);
            }
        }
        const uint32_t cost = ls.sum(s.value(pnorm));             // of this lane's rows, then of the candidate
        if (inside) best.take(cost, sq.order(c, wx, wy));
    }
    const Least won = wave_least(best.cost, best.order);
    int ox, oy;
    sq.offset(won.order, &ox, &oy);
    *vx = cx + ox;
    *vy = cy + oy;
    wave_lds_fence();                                            // the next level overwrites the slice
    return won.cost;
}

template <int BS, int LEVELS>
__global__ void __launch_bounds__(BLK_THREADS) k_hier(const HierArgs A)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const WaveBlock w = wave_block<false>(A.wb);                 // in vector registers: faster here, see wave_block
    if (w.none) return;
    const int wave = w.wave, lane = w.lane, bj = w.bj, bi = w.bi, pair = w.z;
    const int bs = BS ? BS : A.bs, levels = LEVELS ? LEVELS : A.levels;
    uint32_t* anc = (uint32_t*)(lds + (size_t)wave * A.slice_bytes);
    uint32_t* win = (uint32_t*)(lds + (size_t)wave * A.slice_bytes + A.anchor_bytes);
    const long long slot = ((long long)pair * A.hb + bi) * A.wb + bj;
    int vx = 0, vy = 0;
    auto level = [&](auto lc) {
        constexpr int l = decltype(lc)::value;
        if (l < 3 - levels) return;
        const HierLevel& L = A.lv[l];
        const int b = bs >> (2 - l);
        const bool top = l == 3 - levels;
        const int R = top ? A.cw : A.radius;
        const int cx = min(max(top ? 0 : 2 * vx, -bj * b), L.W - b - bj * b);
        const int cy = min(max(top ? 0 : 2 * vy, -bi * b), L.H - b - bi * b);
        const uint32_t cost = level_search<(BS >> (2 - l))>(L, pair, b, R, A.pnorm, bi, bj, cx, cy, anc, win, lane, &vx, &vy);
        if (lane == 0) {
            L.mf[slot * 2] = vx;
            L.mf[slot * 2 + 1] = vy;
            L.cost[slot] = (long long)cost;
        }
    };
    level(std::integral_constant<int, 0>());
    level(std::integral_constant<int, 1>());
    level(std::integral_constant<int, 2>());
}

}  // namespace

// the argument rules of hier.py
int hier_check_args(const char* who, int bs, int cw, int radius, int pnorm, int levels)
{
    GME_REQUIRE(levels >= 1 && levels <= 3, GME_ERR_ARG, "%s: levels %d (1 .. 3)", who, levels);
    if (int rc = require_pnorm(who, pnorm)) return rc;
    GME_REQUIRE(bs >= 1 && bs <= HIER_MAX_BS && bs % (1 << (levels - 1)) == 0 && (bs >> (levels - 1)) >= HIER_MIN_TOP, GME_ERR_ARG,
                "%s: block_size %d with %d levels (a multiple of %d, at most %d, at least %d at the coarsest level)", who, bs, levels,
                1 << (levels - 1), HIER_MAX_BS, HIER_MIN_TOP);
    GME_REQUIRE(cw >= 0 && cw <= HIER_MAX_CW, GME_ERR_ARG, "%s: coarse_window %d (0 .. %d)", who, cw, HIER_MAX_CW);
    GME_REQUIRE(radius >= 0 && radius <= HIER_MAX_R, GME_ERR_ARG, "%s: radius %d (0 .. %d)", who, radius, HIER_MAX_R);
    return GME_OK;
}

// hier.search of `pairs` pairs: level[l] holds the planes of pyramid level l (pair k = planes first_prev + k and first_cur + k
// of the stack), mf[l] / cost[l] the level's outputs [pairs][hb][wb][2] / [pairs][hb][wb] for l >= 3 - levels; hb, wb = the
// blocks of level 2
int launch_hier(gme_ctx* ctx, const Plane (&level)[3], int first_prev, int first_cur, int pairs, int bs, int cw, int radius,
                int pnorm, int levels, int32_t* const (&mf)[3], long long* const (&cost)[3])
{
    int rc = hier_check_args("hierarchical search", bs, cw, radius, pnorm, levels);
    if (rc) return rc;
    const int hb = level[2].H / bs, wb = level[2].W / bs;
    const bool compiled = levels == 3 && (bs == 16 || bs == 32 || bs == 64);
    HierArgs a;
    a.hb = hb; a.wb = wb; a.bs = bs; a.levels = levels; a.cw = cw; a.radius = radius; a.pnorm = pnorm;
    a.anchor_bytes = block_bytes(bs);
    a.slice_bytes = 0;                                            // the anchor and the largest window of a level
    for (int l = 3 - levels; l < 3; ++l) {
        const int bytes = a.anchor_bytes + window_bytes((bs >> (2 - l)) + 2 * (l == 3 - levels ? cw : radius));
        if (bytes > a.slice_bytes) a.slice_bytes = bytes;
    }
    const long long per = (long long)hb * wb;
    auto note = [&] {
        if (compiled) plan_note(ctx, 0, "k_hier<%d,3> cw %d r %d, %d x %d blocks, one wave each", bs, cw, radius, hb, wb);
        else plan_note(ctx, 0, "k_hier<0,0> bs %d levels %d cw %d r %d, %d x %d blocks, one wave each", bs, levels, cw, radius, hb, wb);
    };
    return launch_wave_blocks(ctx, pairs, hb, wb, a.slice_bytes, a, note, [&](int k) {
        for (int l = 0; l < 3; ++l) {
            HierLevel& L = a.lv[l];
            const Plane& p = level[l];
            L = HierLevel();
            if (l < 3 - levels) continue;
            L.prev = p.at(first_prev + k); L.cur = p.at(first_cur + k); L.stride = p.stride;
            L.H = p.H; L.W = p.W; L.pitch = p.pitch;
            L.mf = mf[l] + per * k * 2; L.cost = cost[l] + per * k;
        }
        return !compiled ? k_hier<0, 0> : bs == 16 ? k_hier<16, 3> : bs == 32 ? k_hier<32, 3> : k_hier<64, 3>;
    });
}
