// Variable-block-size motion (host definition: vbs.py).  A root block of the sequence's motion field is
// split in four, each quarter refined within +-radius of its parent's vector, to `depth` levels; a node keeps its split only
// where the children's costs plus the penalty lie strictly below its own cost.  A root depends on no neighbour and every node
// of its tree is always scored, so the work is fixed whatever the content.  Everything is integer: the device equals vbs.tree
// byte for byte.
//
// Kernels:
//   k_vbs<BS, DEPTH>    one wave per root, four roots to a 256-thread workgroup, each wave on its own LDS slice (no workgroup
//                       barrier).  The wave stages the BS x BS anchor and the (BS + 2 DEPTH r)^2 window of `current` around the
//                       root's displaced block once: the centres move by at most r per depth, so every candidate of every
//                       descendant lies in it.  Depth by depth the (child, candidate) items are spread over the lanes (P lanes
//                       share the rows of one item), a row is scored four bytes at a time (v_alignbyte, then v_sad_u8, or three
//                       v_dot4 for aa + bb - 2ab), and every item lowers its child's key (cost << 6 | position in the
//                       definition's order, centre = 0) with one LDS minimum.  The bottom-up decision is made from the 21 keys
//                       in registers; the lanes then write the root's cells.  <16,2> and <32,2> are compiled; <0,0> takes
//                       block size and depth at run time (and leaf rows that are no multiple of four bytes).
//   k_compensate_vbs    subpel.compensate_integer at an explicit cell size (the integer compensation kernels derive theirs from
//                       H / h, which is another size when H is no multiple of the root), with the squared error per pair
#include "bbme_predict.h"
#include "bbme_wave_lds.h"
#include "gme_passes.h"

namespace {

constexpr int VBS_MAX_BS = 64, VBS_MAX_DEPTH = 2, VBS_MAX_R = 3, VBS_MIN_LEAF = 4, VBS_MAX_PENALTY = 1 << 30;
constexpr int VBS_NODE_SLOTS = 24;                              // 1 + 4 + 16 nodes, rounded up: key, then the vector's two parts
constexpr int VBS_ROUND_STEPS = 8;                              // what a round of items costs beside its rows, in dword steps (an estimate)
constexpr int VBS_MAX_CAND = (2 * VBS_MAX_R + 1) * (2 * VBS_MAX_R + 1), VBS_MAX_ITEMS = 16 * VBS_MAX_CAND;
// a child's key: cost in the upper 26 bits (side at most 32), the candidate's order in the lower 6
static_assert((long long)(VBS_MAX_BS / 2) * (VBS_MAX_BS / 2) * 65025ll < (1ll << 26) && VBS_MAX_CAND + 1 <= (1 << 6), "32-bit keys");
// every sum of a decision in 32 bits
static_assert((long long)VBS_MAX_PENALTY + 4ll * (VBS_MAX_BS / 2) * (VBS_MAX_BS / 2) * 65025ll < (1ll << 31), "31-bit decisions");
static_assert((long long)VBS_MAX_BS * VBS_MAX_BS * 65025ll < (1ll << 31), "31-bit root costs");
constexpr int VBS_MAX_WINDOW = VBS_MAX_BS + 2 * VBS_MAX_DEPTH * VBS_MAX_R;
static_assert(small_div_covers(VBS_MAX_WINDOW, window_row_dwords(VBS_MAX_WINDOW), 2 * VBS_MAX_R + 1), "range of small_div");

// item / ncand for the items of one depth: 0 <= t < 16 * 49, d = (2r + 1)^2
__host__ __device__ constexpr int item_div(int t, int d) { return (int)(((uint32_t)t * ((1u << 16) / (uint32_t)d + 1u)) >> 16); }
constexpr bool item_div_exact()
{
    for (int r = 0; r <= VBS_MAX_R; ++r)
        for (int t = 0; t < VBS_MAX_ITEMS; ++t)
            if (item_div(t, (2 * r + 1) * (2 * r + 1)) != t / ((2 * r + 1) * (2 * r + 1))) return false;
    return true;
}
static_assert(item_div_exact(), "range of item_div");

struct VbsArgs {
    const uint8_t* prev;          // first "previous" plane
    const uint8_t* cur;           // first "current" plane
    long long stride;             // bytes between consecutive pairs' planes
    int H, W, pitch;
    const int32_t* mf;            // [pairs][hb][wb][2]
    int32_t* leaf;                // [pairs][hb << depth][wb << depth][2]
    uint8_t* dmap;                // [pairs][hb << depth][wb << depth]
    long long* cost;              // [pairs][hb][wb]
    int hb, wb, bs, depth, radius, pnorm;
    uint32_t penalty;
    int anchor_bytes, window_bytes, slice_bytes;      // LDS of a wave: anchor, window, then 3 * VBS_NODE_SLOTS words of nodes
};

template <int BS, int DEPTH>
__global__ void __launch_bounds__(BLK_THREADS) k_vbs(const VbsArgs A)
{
    extern __shared__ __align__(16) uint8_t lds[];
    const WaveBlock w = wave_block(A.wb);
    if (w.none) return;
    const int wave = w.wave, lane = w.lane, bj = w.bj, bi = w.bi, pair = w.z;
    const int B = BS ? BS : A.bs, D = BS ? DEPTH : A.depth;
    const int r = A.radius, pnorm = A.pnorm;
    const Square sq(r);
    const int m = D * r;                                         // how far a descendant's vector can lie from the root's
    const int cells = 1 << D;                                    // cells of the leaf grid along a root's side
    const long long root = ((long long)pair * A.hb + bi) * A.wb + bj;
    const int vx = __builtin_amdgcn_readfirstlane(A.mf[root * 2]), vy = __builtin_amdgcn_readfirstlane(A.mf[root * 2 + 1]);
    const int x0 = bj * B, y0 = bi * B;
    const long long sxl = (long long)x0 + vx, syl = (long long)y0 + vy;
    const bool inside = sxl >= 0 && syl >= 0 && sxl + B <= A.W && syl + B <= A.H;
    const int cr = lane >> D, cc = lane & (cells - 1);           // this lane's cell of the root (lane < cells * cells)
    const long long cell = (((long long)pair * A.hb + bi) * cells + cr) * ((long long)A.wb * cells) + (long long)bj * cells + cc;
    if (!inside) {                                               // a leaf of depth 0 that keeps its vector, cost -1
        if (lane < cells * cells) {
            A.leaf[cell * 2] = vx;
            A.leaf[cell * 2 + 1] = vy;
            A.dmap[cell] = 0;
        }
        if (lane == 0) A.cost[root] = -1;
        return;
    }
    const int sx = (int)sxl, sy = (int)syl;                      // the root's displaced block in `current`

    uint32_t* anc = (uint32_t*)(lds + (size_t)wave * A.slice_bytes);
    uint32_t* win = (uint32_t*)(lds + (size_t)wave * A.slice_bytes + A.anchor_bytes);
    uint32_t* key = (uint32_t*)(lds + (size_t)wave * A.slice_bytes + A.anchor_bytes + A.window_bytes);
    int* relx = (int*)key + VBS_NODE_SLOTS;                      // a node's vector minus the root's
    int* rely = relx + VBS_NODE_SLOTS;
    // the anchor has window rows too: a child's rows are read from it at the child's byte offset
    const int na = window_row_dwords(B), ws = B + 2 * m, wd = window_row_dwords(ws);
    stage_bytes(anc, B, na, B, A.prev + (long long)pair * A.stride, A.pitch, A.H, A.W, y0, x0, lane);
    stage_bytes(win, ws, wd, ws, A.cur + (long long)pair * A.stride, A.pitch, A.H, A.W, sy - m, sx - m, lane);
    if (lane < VBS_NODE_SLOTS) { key[lane] = NO_COST; relx[lane] = 0; rely[lane] = 0; }
    wave_lds_fence();

    // the root's own cost: its (row, dword) pairs over the lanes
    uint32_t c0;
    {
        const int nd = row_dwords(B);
        const uint32_t tail = tail_mask(B);
        RowScore s;
        for (int t = lane; t < B * nd; t += 64) {
            const int y = small_div(t, nd), k = t - y * nd;
            uint32_t v = window_dword(win + (m + y) * wd + (m >> 2), k, (uint32_t)m & 3u);
            if (!BS || (BS & 3)) { if (k == nd - 1) v &= tail; }
            s.add(anc[y * na + k], v, pnorm);                    // anchor bytes at and past column B are zero
        }
        c0 = wave_sum_u32(s.value(pnorm));
    }

    // depth d: 4^d children of side B >> d, nodes 1 .. 4 (child k of the root) and 5 .. 20 (child k2 of node 1 + k1 at
    // 5 + 4 k1 + k2), each with (2r + 1)^2 candidates around its parent's vector
#pragma unroll 1
    for (int d = 1; d <= D; ++d) {
        const int b = B >> d, items = sq.ncand << (2 * d), base = d == 1 ? 1 : 5;
        const int nd = row_dwords(b);
        const uint32_t tail = tail_mask(b);
        // P lanes to an item, each a share of its rows: the P with the least work per lane over all rounds, a round counted as
        // its dword steps plus VBS_ROUND_STEPS for the indices, the reduction and the minimum
        int P = 1, steps = ((items + 63) >> 6) * (b * nd + VBS_ROUND_STEPS);
        for (int p = 2; p <= 8 && p <= b; p *= 2) {
            const int s = ((items * p + 63) >> 6) * (((b + p - 1) / p) * nd + VBS_ROUND_STEPS);
            if (s < steps) { steps = s; P = p; }
        }
        const LaneSplit ls(P, lane);
        for (int i0 = 0; i0 < items; i0 += ls.slots) {
            const int it = i0 + ls.slot;
            const bool listed = it < items;
            const int ii = listed ? it : 0;
            const int child = item_div(ii, sq.ncand), c = ii - child * sq.ncand;
            int ox, oy;                                          // the candidate's offset + r (column, row)
            sq.at(c, &ox, &oy);
            int cx, cy, parent = 0;                              // the child's origin in the root
            if (d == 1) { cx = (child & 1) * b; cy = (child >> 1) * b; }
            else {
                const int k1 = child >> 2, k2 = child & 3;
                cx = (k1 & 1) * 2 * b + (k2 & 1) * b;
                cy = (k1 >> 1) * 2 * b + (k2 >> 1) * b;
                parent = 1 + k1;
            }
            const int dx = relx[parent] + ox - r, dy = rely[parent] + oy - r;      // within [-d r, d r] of the root's vector
            const int gx = sx + cx + dx, gy = sy + cy + dy;      // the candidate's block in the frame
            const bool ok = listed && gx >= 0 && gy >= 0 && gx + b <= A.W && gy + b <= A.H;
            const int wx = m + cx + dx, wy = m + cy + dy;        // ... and in the window: 0 <= wx, wx + b <= ws
            const uint32_t wsh = (uint32_t)wx & 3u, ash = (uint32_t)cx & 3u;
            RowScore s;
            for (int y = ls.q; y < b; y += ls.P) {
                const uint32_t* arow = anc + (cy + y) * na + (cx >> 2);
                const uint32_t* wrow = win + (wy + y) * wd + (wx >> 2);
#pragma unroll 4
                for (int k = 0; k < nd; ++k) {
                    uint32_t a = arow[k];
                    uint32_t v = window_dword(wrow, k, wsh);
                    if (!BS) {                                   // a child may start and end inside a dword
                        a = window_dword(arow, k, ash);
                        if (k == nd - 1) { a &= tail; v &= tail; }
                    }
                    s.add(a, v, pnorm);
                }
            }
            const uint32_t cost = ls.sum(s.value(pnorm));
            if (ok && ls.q == 0) atomicMin(&key[base + child], (cost << 6) | sq.order(c, ox, oy));
        }
        wave_lds_fence();
        if (lane < (1 << (2 * d))) {                             // the winners' vectors, for the next depth and the cells
            const int parent = d == 1 ? 0 : 1 + (lane >> 2);
            int ox, oy;
            sq.offset(key[base + lane] & 63u, &ox, &oy);
            relx[base + lane] = relx[parent] + ox;
            rely[base + lane] = rely[parent] + oy;
        }
        wave_lds_fence();
    }

    // bottom-up, the same in every lane: bit 0 of `split` for the root, bit 1 + k for node 1 + k
    uint32_t F0 = c0, split = 0;
    if (D >= 1) {
        uint32_t S0 = A.penalty;
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) {
            const uint32_t c1 = key[1 + k1] >> 6;
            uint32_t F1 = c1;
            if (D == 2) {
                uint32_t S1 = A.penalty;
#pragma unroll
                for (int k2 = 0; k2 < 4; ++k2) S1 += key[5 + 4 * k1 + k2] >> 6;
                if (S1 < c1) { F1 = S1; split |= 2u << k1; }
            }
            S0 += F1;
        }
        if (S0 < c0) { F0 = S0; split |= 1u; }
    }
    if (lane < cells * cells) {
        int node = 0, dep = 0;
        if (split & 1u) {
            const int k1 = ((cr >> (D - 1)) << 1) | (cc >> (D - 1));
            node = 1 + k1; dep = 1;
            if (D == 2 && ((split >> (1 + k1)) & 1u)) { node = 5 + 4 * k1 + (((cr & 1) << 1) | (cc & 1)); dep = 2; }
        }
        A.leaf[cell * 2] = vx + relx[node];
        A.leaf[cell * 2 + 1] = vy + rely[node];
        A.dmap[cell] = (uint8_t)dep;
    }
    if (lane == 0) A.cost[root] = (long long)F0;
}

// The pixel of k_compensate_vbs.  Output pixel (u, v) of cell (v / g, u / g) inside the hg x wg field is the pixel of `previous`
// at (u - d0, v - d1) where that lies in the frame; elsewhere, and beyond the last whole cell, the pixel is kept.
struct VbsPixel {
    const uint8_t* p;             // the pair's `previous` plane
    const int32_t* q;             // its leaf field [hg][wg][2]
    int H, W, pitch, g, hg, wg;
    __device__ __forceinline__ int operator()(int u, int v) const
    {
        const int i = v / g, j = u / g;
        int o = p[(long long)v * pitch + u];
        if (i < hg && j < wg) {
            const long long su = (long long)u - q[((long long)i * wg + j) * 2];
            const long long sv = (long long)v - q[((long long)i * wg + j) * 2 + 1];
            if (su >= 0 && su < W && sv >= 0 && sv < H) o = p[sv * pitch + su];
        }
        return o;
    }
};

// the row frame of bbme_predict.h, one plane per pair
__global__ void __launch_bounds__(PRED_THREADS) k_compensate_vbs(const uint8_t* prev, const uint8_t* cur, long long plane_stride, int H,
                                                                 int W, int pitch, int g, int hg, int wg, const int32_t* leaf,
                                                                 uint8_t* out, long long out_stride, int out_pitch,
                                                                 unsigned long long* sse)
{
    const int f = blockIdx.z;
    const VbsPixel px = { prev + (long long)f * plane_stride, leaf + (long long)f * hg * wg * 2, H, W, pitch, g, hg, wg };
    predict_rows(px, cur + (long long)f * plane_stride, H, W, pitch, out + (long long)f * out_stride, out_pitch, sse + f);
}

}  // namespace

// the argument rules of vbs.py
int vbs_check_args(const char* who, int bs, int depth, int radius, int pnorm, int penalty)
{
    GME_REQUIRE(depth >= 0 && depth <= VBS_MAX_DEPTH, GME_ERR_ARG, "%s: depth %d (0 .. %d)", who, depth, VBS_MAX_DEPTH);
    if (int rc = require_pnorm(who, pnorm)) return rc;
    GME_REQUIRE(bs >= 1 && bs <= VBS_MAX_BS && bs % (1 << depth) == 0 && (bs >> depth) >= VBS_MIN_LEAF, GME_ERR_ARG,
                "%s: block_size %d with depth %d (a multiple of %d, at most %d, leaves of at least %d)", who, bs, depth, 1 << depth,
                VBS_MAX_BS, VBS_MIN_LEAF);
    GME_REQUIRE(radius >= 0 && radius <= VBS_MAX_R, GME_ERR_ARG, "%s: radius %d (0 .. %d)", who, radius, VBS_MAX_R);
    GME_REQUIRE(penalty >= 0 && penalty <= VBS_MAX_PENALTY, GME_ERR_ARG, "%s: penalty %d (0 .. 2^30)", who, penalty);
    return GME_OK;
}

// vbs.tree of `pairs` pairs: pair k reads the planes prev + k * plane_stride and cur + k * plane_stride and the field
// mf[k][hb][wb][2], hb = H / bs and wb = W / bs; leaf [pairs][hb << depth][wb << depth][2], dmap of the same grid and
// cost [pairs][hb][wb] (device)
int launch_vbs(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch,
               int bs, int depth, int radius, int pnorm, int penalty, const int32_t* mf, int32_t* leaf, uint8_t* dmap,
               long long* cost)
{
    int rc = vbs_check_args("variable-block-size tree", bs, depth, radius, pnorm, penalty);
    if (rc) return rc;
    const int hb = H / bs, wb = W / bs;
    const bool compiled = depth == 2 && (bs == 16 || bs == 32);
    VbsArgs a;
    a.stride = plane_stride; a.H = H; a.W = W; a.pitch = pitch;
    a.hb = hb; a.wb = wb; a.bs = bs; a.depth = depth; a.radius = radius; a.pnorm = pnorm; a.penalty = (uint32_t)penalty;
    a.anchor_bytes = window_bytes(bs);
    a.window_bytes = window_bytes(bs + 2 * depth * radius);
    a.slice_bytes = a.anchor_bytes + a.window_bytes + ((3 * VBS_NODE_SLOTS * 4 + 15) & ~15);
    const long long per = (long long)hb * wb, per_cells = per << (2 * depth);
    auto note = [&] {
        if (compiled) plan_note(ctx, 0, "k_vbs<%d,2> r %d penalty %d, %d x %d roots, one wave each", bs, radius, penalty, hb, wb);
        else plan_note(ctx, 0, "k_vbs<0,0> bs %d depth %d r %d penalty %d, %d x %d roots, one wave each", bs, depth, radius, penalty, hb, wb);
    };
    return launch_wave_blocks(ctx, pairs, hb, wb, a.slice_bytes, a, note, [&](int k) {
        a.prev = prev + (long long)k * plane_stride; a.cur = cur + (long long)k * plane_stride;
        a.mf = mf + per * k * 2; a.cost = cost + per * k;
        a.leaf = leaf + per_cells * k * 2; a.dmap = dmap + per_cells * k;
        return !compiled ? k_vbs<0, 0> : bs == 16 ? k_vbs<16, 2> : k_vbs<32, 2>;
    });
}

// out planes = subpel.compensate_integer of the prev planes by leaf[pairs][hg][wg][2] at cell size g, sse[pairs] (device, zeroed
// here) = squared error of each against its cur plane
int launch_compensate_vbs(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                          int pitch, int g, int hg, int wg, const int32_t* leaf, uint8_t* out, long long out_stride, int out_pitch,
                          unsigned long long* sse)
{
    if (pairs == 0) return GME_OK;
    return predict_planes(ctx, pairs, sse, [&](int k, int n) {
        hipLaunchKernelGGL(k_compensate_vbs, predict_grid(H, W, n), dim3(PRED_THREADS), 0, ctx->stream, prev + (long long)k * plane_stride,
                           cur + (long long)k * plane_stride, plane_stride, H, W, pitch, g, hg, wg,
                           leaf + (long long)hg * wg * 2 * k, out + (long long)k * out_stride, out_stride, out_pitch, sse + k);
    });
}
