// Exhaustive MAE search, bs = 16, with exact successive elimination -- same answer as the brute
// force kernel (bbme_fast.hip: k_exh_qsad16, bbme.py:105-179), a fraction of the SAD work.
//
// For a candidate block B and the anchor A, each split into four 8x8 quadrants,
//     LB(B) = sum_q |sum(A_q) - sum(B_q)|  <=  SAD(A, B)                  (triangle inequality).
// Once some candidate's true SAD is known (UB), every candidate with LB > UB has SAD > UB >= the
// minimum: it can neither win nor tie, so skipping it keeps the reference's "first strict
// minimum in scan order" result bit for bit.
//
// Two kernels run the same phases: k_exh_sea16 (one tile per workgroup, bbme_sea_common.h: one_tile) and k_exh_sea16p
// (persistent workgroups that prefetch the next tile into registers, bbme_sea_common.h: persistent_tiles).
// Per tile (NB adjacent macroblocks, one wave each, as in k_exh_qsad16):
//   A  stage the search window of `cur` and the anchors in LDS; quadrant sums of each anchor;
//   A' 8x8 box sums S8 of the staged window, in LDS: per lane and window row one v_qsad_pk_u16_u8
//      against a zero reference (four sliding 4-byte sums) whose accumulator adds up the rows; an
//      output row is the difference of two of those cumulative sums plus the neighbour lane's
//      (DPP wave_shl:1), i.e. the other 4-byte half -- no per-frame table, no extra HBM traffic;
//   B  LB for all NC^2 candidates of the wave's block: per lane and candidate row 2 (R + 2) S8 reads and 4 (R + 2)
//      v_perm_b32 that pair S8(y, x) with S8(y + 8, x) -- the right-hand pair of candidate column x is the left-hand
//      pair of column x + 8 -- and two v_sad_u16 per candidate; per lane: the smallest LB of each of its R patches
//      (R rows x 4 columns), the bound alone, no candidate index;
//   C  UB := SAD of three real candidates (64 lanes x 1 dword): the zero vector, the vector the workgroup's previous tile
//      ended with, and the candidate with the smallest LB -- a wave minimum over (LB, lane) names the first lane that
//      holds it, the wave's lanes then recompute that lane's candidates, one each, and a ballot names the first one;
//   D  patches with min LB <= UB go to a workgroup-wide list (LDS atomics);
//   E  the list is processed 64*NB patches at a time, one patch per lane (R x 16 x 4
//      v_qsad_pk_u16_u8 against the anchor read from LDS -- lanes of one wave may serve different
//      blocks), best keys merged with LDS atomicMin; before each chunk entries whose LB exceeds
//      the tightened UB are dropped; four lanes per patch from R = 3 on (larger windows);
//   F  lane 0 of each wave stores its block's vector.
// On the synthetic and the reference's doc frames 2-6 % of the patches survive.
#include "bbme_sea_common.h"

namespace {

using namespace sea;

// B: lower bounds of the 4R x R candidates of one lane (candidate rows prow*R + i, columns
// q*4R + 4k + e).  GUARD_NONE is the body for blocks whose whole window is inside the frame (84 % of
// them at 720x480, sw = 16).  The others decide validity once per lane, before the row loop, and let it ride
// on an operand the body has anyway, so that every candidate keeps the unguarded instructions:
//   GUARD_ROWS (all columns valid: blocks at the top and bottom edge)  the inner v_sad_u16 of a candidate row
//       outside [lo_r, hi_r] starts from PENALTY instead of 0;
//   GUARD_ALL  (frame corners, left and right edge, partial size classes with their padding candidates)  the start
//       value also takes PENALTY for a column above hi_c: one v_cndmask_b32 per candidate on a lane mask formed
//       once per column; below lo_c whole patches go (lo_c is a multiple of 4), after the loop.
// A penalised bound lies above 65280, the largest real one (and SAD), and below 2^18.  The table rows and quads such a
// candidate reads exist (the table is sized by R, not by the frame); what they hold does not matter.  pmin[k] is the
// smallest bound of patch k, without an index; a patch whose smallest bound is a penalised one has no valid candidate:
// 0xFFFFFFFF, as if no bound had been formed.  Shifted by 13 that is 0xFFFFE000, above every real key
// (FIRST_INVALID_KEY = FIRST_INVALID_BOUND << 13), which is what everything downstream keeps seeing.
constexpr int GUARD_NONE = 0, GUARD_ROWS = 1, GUARD_ALL = 2;
constexpr uint32_t PENALTY = 1u << 17;
constexpr uint32_t FIRST_INVALID_KEY = 65536u << 13;     // above every real key, not above any penalised one
constexpr uint32_t FIRST_INVALID_BOUND = FIRST_INVALID_KEY >> 13;
// *p += v in LDS by the calling lanes, each on its own; returns what the word held.  Written out, because an atomicAdd is
// rewritten into a wave-wide aggregation (ballot, v_mbcnt, multiply, one lane's add, broadcast) even where the caller has
// aggregated already and calls it from one lane.  The wait is part of it: the compiler does not count this instruction.
__device__ __forceinline__ uint32_t lds_add_rtn(uint32_t* p, uint32_t v)
{
    uint32_t old;
    const uint32_t addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)p;
    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(old) : "v"(addr), "v"(v) : "memory");
    return old;
}
// A list entry (phase D's list, phase C2's own slots): bound | k << 16 | lane << 19 | wave << 25 -- the patch of phase B's
// lane (prow, q), column group k, of the block of wave `wave` (at most 16: bits 25 .. 28) -- and in bit 29 whether that
// block's whole window lies inside the frame with no padding candidates (phase B's GUARD_NONE case).  The listing wave
// knows that as a wave-uniform value; the lanes that score the entry serve different blocks and would each have to
// work it out from the block's position.
constexpr uint32_t ENT_INTERIOR = 1u << 29;
// wave / tc for a wave number below 16 (a list entry's): a shift where the tile's width is a compile-time power of two
// (the geometry-fixed 2x4 instance), the multiply-shift division otherwise
__device__ __forceinline__ int wave_row(const SeaGeo& d, int w)
{
    if (__builtin_constant_p(d.tc) && (d.tc & (d.tc - 1)) == 0) return w >> __builtin_ctz((unsigned)d.tc);
    return div_small(w, d.magic_tc);
}
// some value, at no instruction: for registers whose content is exchanged but never used (lanes without work in a DPP sum)
__device__ __forceinline__ uint64_t any_u64()
{
    uint32_t lo, hi;
    asm volatile("" : "=v"(lo), "=v"(hi));
    return ((uint64_t)hi << 32) | lo;
}
// [lo(t), lo(b)] (odd = false) or [hi(t), hi(b)] of two packed u16 pairs
__device__ __forceinline__ uint32_t pair_u16(uint32_t t, uint32_t b, bool odd)
{
    return __builtin_amdgcn_perm(b, t, odd ? 0x07060302u : 0x05040100u);
}
// The two operand pairs of the candidate whose quadrant sums are tl, tr (row y, columns x and x + 8) and bl, br (row y + 8), each
// in the halves `odd` picks: vertically ([tl, bl], [tr, br]) against the anchor sums [A0, A2] and [A1, A3], or horizontally
// ([tl, tr], [bl, br]) against [A0, A1] and [A2, A3].  pa / pb below are the anchor sums in the packing of the instance.
template <bool VERT>
__device__ __forceinline__ void candidate_pairs(uint32_t tl, uint32_t tr, uint32_t bl, uint32_t br, bool odd, uint32_t* first, uint32_t* second)
{
    *first = VERT ? pair_u16(tl, bl, odd) : pair_u16(tl, tr, odd);
    *second = VERT ? pair_u16(tr, br, odd) : pair_u16(bl, br, odd);
}
template <int R, int GUARD, bool VERT>
__device__ __forceinline__ void lower_bounds(const uint64_t* sp0, int XQ, int prow, int q, uint32_t pa, uint32_t pb,
                                             int lo_r, int hi_r, int lo_c, int hi_c, uint32_t (&pmin)[R])
{
    // R >= 4 keeps the earlier form for every edge block (GUARD_ALL there; GUARD_ROWS is not used), which skips invalid
    // rows and candidates by compares of their own: in the <5, 7, 38> instance, at 80 VGPRs when that was tried, the column
    // masks spilled three VGPRs and GUARD_ROWS beside the earlier form one ("Trimmed").  It builds both
    // operand pairs per candidate, as every instance without vertical pairs does (vertical_pairs below)
    constexpr bool SKIP = GUARD == GUARD_ALL && R >= 4;
#pragma unroll
    for (int k = 0; k < R; ++k) pmin[k] = 0xFFFFFFFFu;
    constexpr uint32_t penalty = PENALTY;
    uint32_t seed[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int ri = prow * R + i;
        seed[i] = (GUARD == GUARD_NONE || SKIP || (ri >= lo_r && ri <= hi_r)) ? 0u : penalty;
    }
    // the lane's valid columns j = 4k + e are nlo .. nhi (none: nhi < nlo).  nlo is a multiple of 4 (sw is, block
    // columns are multiples of 16): on the low side whole patches go, after the loop.
    const int nlo = lo_c - q * 4 * R, nhi = hi_c - q * 4 * R;
    const uint64_t* top = sp0;
    const uint64_t* bot = sp0 + 8 * XQ;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int ri = prow * R + i;
        if (!SKIP || (ri >= lo_r && ri <= hi_r)) {
            uint64_t t[R + 2], b[R + 2];                   // quads k and k + 2 for k < R: R + 2 distinct ones
#pragma unroll
            for (int k = 0; k < R + 2; ++k) { t[k] = top[k]; b[k] = bot[k]; }
            if constexpr (SKIP || !VERT) {
                // both pairs built per candidate (the skip form decides per lane which candidates it needs at all)
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    if (SKIP && (4 * k > nhi || 4 * k + 3 < nlo)) continue;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (SKIP && (4 * k + e < nlo || 4 * k + e > nhi)) continue;
                        const int sh = 32 * (e >> 1);
                        uint32_t first, second;
                        candidate_pairs<VERT>((uint32_t)(t[k] >> sh), (uint32_t)(t[k + 2] >> sh), (uint32_t)(b[k] >> sh), (uint32_t)(b[k + 2] >> sh), e & 1, &first, &second);
                        const uint32_t start = (GUARD != GUARD_ALL || SKIP || 4 * k + e <= nhi) ? seed[i] : penalty;
                        pmin[k] = min(pmin[k], __builtin_amdgcn_sad_u16(first, pa, __builtin_amdgcn_sad_u16(second, pb, start)));
                    }
                }
            } else {
                // vertical pairs: column c = 4m + e of the row gives vp[m][e] = [S(y, c), S(y+8, c)]; candidate column j
                // matches vp of column j against [A0, A2] and vp of column j + 8 against [A1, A3], so the right-hand pairs
                // of column group k are the left-hand pairs of group k + 2: 4 (R + 2) pairs per row, each built once, in
                // the order the groups need them (quads 2 .. R - 1 stay live until their second use)
                uint32_t vp[R + 2][4];
#pragma unroll
                for (int k = 0; k < R; ++k) {
#pragma unroll
                    for (int m = (k < 2 ? k : k + 2); m <= k + 2; m += 2)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            vp[m][e] = pair_u16((uint32_t)(t[m] >> (32 * (e >> 1))), (uint32_t)(b[m] >> (32 * (e >> 1))), e & 1);
                    uint32_t lb[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t start = (GUARD != GUARD_ALL || 4 * k + e <= nhi) ? seed[i] : penalty;
                        lb[e] = __builtin_amdgcn_sad_u16(vp[k][e], pa, __builtin_amdgcn_sad_u16(vp[k + 2][e], pb, start));
                    }
                    pmin[k] = min(min(pmin[k], lb[0]), lb[1]);
                    pmin[k] = min(min(pmin[k], lb[2]), lb[3]);
                }
            }
        }
        top += XQ;
        bot += XQ;
    }
    if constexpr (GUARD != GUARD_NONE && !SKIP) {
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (pmin[k] >= FIRST_INVALID_BOUND || (GUARD == GUARD_ALL && 4 * k < nlo)) pmin[k] = 0xFFFFFFFFu;
    }
}

// C: the candidate phase B's minimum names, recovered once per wave.  `bl` is the first lane that holds the block's
// smallest bound `mb`; lane l of the wave recomputes candidate `local = l` of that lane ((4k + e) R + i, the numbering the
// per-candidate keys used; two rounds at R = 5, where a lane has 100) from the four table entries, with the validity the
// lane applied, and the first lane that finds `mb` on a valid candidate names it: smallest bound, then smallest lane,
// then smallest local index.  Returns the scan index.  Wave-uniform; every lane must call it (ballot).
template <int R, bool VERT>
__device__ __forceinline__ int min_bound_candidate(const uint64_t* s8blk, int XQ, int NC, int bl, uint32_t mb, uint32_t pa, uint32_t pb,
                                                   int lo_r, int hi_r, int lo_c, int hi_c, int lane)
{
    const int col0 = (bl & 3) * 4 * R, row0 = (bl >> 2) * R;
    const uint16_t* tab = (const uint16_t*)(s8blk + row0 * XQ + (bl & 3) * R);     // S8 as u16: 4 XQ per row
    int loc = 0;
    bool found = false;
#pragma unroll
    for (int base = 0; base < 4 * R * R; base += 64) {
        const int l = base + lane;
        const int ce = l / R, li = l - ce * R;
        bool hit = false;
        if (4 * R * R - base >= 64 || l < 4 * R * R) {
            const uint16_t* p = tab + li * 4 * XQ + ce;
            uint32_t first, second;
            candidate_pairs<VERT>(p[0], p[8], p[32 * XQ], p[32 * XQ + 8], false, &first, &second);
            const uint32_t lb = __builtin_amdgcn_sad_u16(first, pa, __builtin_amdgcn_sad_u16(second, pb, 0u));
            const int ci = col0 + ce, ri = row0 + li;
            hit = lb == mb && ci >= lo_c && ci <= hi_c && ri >= lo_r && ri <= hi_r;
        }
        const unsigned long long m = __ballot(hit);
        if (!found && m) {
            loc = base + __builtin_ctzll(m);
            found = true;
        }
    }
    const int ce = loc / R, li = loc - ce * R;
    return (col0 + ce) * NC + row0 + li;
}

// C2's evaluation, four lanes per patch: lane `sub` of a quad takes anchor rows 4*sub .. 4*sub+3 of the patch's block (R+3 window rows,
// 16*R QSADs); the four partial u16x4 sums are added inside the quad with DPP moves, then lane `sub` turns column `sub`
// of the patch into keys (sad << 13 | scan index).  Returns the quad's smallest key (0xFFFFFFFF: none).  Every lane of
// the wave must call it (DPP); a quad is uniform in `ent` and `active`.
// ent: a list entry (ENT_INTERIOR above).
template <int R>
__device__ __forceinline__ uint32_t eval_patch_quad(const SeaGeo& d, int H, int W, const uint32_t* win, const uint32_t* anchor, uint32_t ent,
                                                    bool active, int sub, int trow, int bcol0, int NC)
{
    const int w2 = (ent >> 25) & 15, l2 = (ent >> 19) & 63, k2 = (ent >> 16) & 7;
    const int wr2 = wave_row(d, w2), wc2 = w2 - wr2 * d.tc;     // the patch's block inside the tile
    const int prow2 = l2 >> 2, q2 = l2 & 3;
    uint64_t acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = any_u64();          // idle quads add and exchange whatever they hold; nobody reads it
    if (active) {
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = 0;
        const uint32_t* lrow = win + (16 * wr2 + prow2 * R + 4 * sub) * d.pitch_dw + wc2 * 4 + q2 * R + k2;
        const uint32_t* an = anchor + w2 * ANCHOR_STRIDE + 16 * sub;
#pragma unroll
        for (int t = 0; t < R + 3; ++t) {
            uint64_t w[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) w[s] = *(const u64_a4*)(lrow + t * d.pitch_dw + s);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int a = t - i;                   // anchor row 4*sub + a
                if (a < 0 || a > 3) continue;
                const u32x4 ar = *(const u32x4*)(an + a * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i] = __builtin_amdgcn_qsad_pk_u16_u8(w[j], ar[j], acc[i]);
            }
        }
    }
    // sum over the quad: plain 32-bit adds on the packed u16 pairs (a 16x16 SAD is at most 65280, so no partial
    // sum carries into the upper half) -- they take the DPP operand directly, v_pk_add_u16 needs a move first
#pragma unroll
    for (int i = 0; i < R; ++i) {
        uint32_t lo = (uint32_t)acc[i], hi = (uint32_t)(acc[i] >> 32);
        lo += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0xB1, 0xF, 0xF, false);            // quad_perm [1,0,3,2]
        hi += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0xB1, 0xF, 0xF, false);
        lo += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0x4E, 0xF, 0xF, false);            // quad_perm [2,3,0,1]
        hi += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0x4E, 0xF, 0xF, false);
        asm volatile("" : "+v"(lo), "+v"(hi));     // pinned here: sunk under `active` the adds leave their DPP moves behind
        acc[i] = ((uint64_t)hi << 32) | lo;
    }
    uint32_t key = 0xFFFFFFFFu;
    if (active) {
        // every lane of the quad holds the patch's R x 4 sums now; lane `sub` turns column `sub` into keys
        // (R candidates instead of 4 R on one lane)
        const int ci = q2 * 4 * R + 4 * k2 + sub, ri0 = prow2 * R;
        const uint32_t shift = (uint32_t)(sub & 1) * 16u;
        if (ent & ENT_INTERIOR) {
            // whole window inside the frame: keys relative to the column's first candidate, base added once
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const uint32_t word = (sub & 2) ? (uint32_t)(acc[i] >> 32) : (uint32_t)acc[i];
                const uint32_t sad = __builtin_amdgcn_ubfe(word, shift, 16u);
                key = min(key, (sad << 13) + (uint32_t)i);
            }
            key += (uint32_t)(ci * NC + ri0);
        } else {
            // an edge block: the window limits are formed here only (lanes of one wave serve different blocks)
            const int c02 = (bcol0 + wc2) * 16, r02 = (trow * d.tr + wr2) * 16;
            const int lo_c = max(0, d.sw - c02), hi_c = min(NC - 1, W - 16 - c02 + d.sw);
            const int lo_r2 = max(0, d.sw - r02), hi_r2 = min(NC - 1, H - 16 - r02 + d.sw);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int ri = ri0 + i;
                if (ci < lo_c || ci > hi_c || ri < lo_r2 || ri > hi_r2) continue;
                const uint32_t word = (sub & 2) ? (uint32_t)(acc[i] >> 32) : (uint32_t)acc[i];
                const uint32_t sad = __builtin_amdgcn_ubfe(word, shift, 16u);
                key = min(key, (sad << 13) | (uint32_t)(ci * NC + ri));
            }
        }
        // quad minimum (a disabled source lane would hand back the minimum's identity; quads are uniform in `active`)
        key = min(key, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)key, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
        key = min(key, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)key, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    }
    return key;
}

// Phases A' .. F of one tile.  On entry the window and the anchors are staged, *count == 0 and the
// workgroup has passed a barrier; there is no barrier after F.
// Returns true (workgroup-uniform) when the tile was handed to the redo kernel instead (SeaDev::redo_list).
// `d` is the geometry; frame size, ordered evaluation, redo list and result plane come from the argument segment
// (bbme_sea_common.h: launch_args), once for phases A' .. D and once behind phase D's barrier for the rest.
// behind_box_sums: what the driver has every wave do right behind the barrier that follows phase A' (Kern, bbme_sea_common.h).
template <int R, bool FIXED, bool VERT, class Behind>
__device__ __forceinline__ bool tile_phases(const SeaGeo& d, uint32_t* lds, const Layout& L, int pair, int trow, int bcol0,
                                            uint32_t mine, uint32_t pa, uint32_t pb, int tid, int tile_id, PhaseClock& clk,
                                            Behind&& behind_box_sums)
{
    // phase C2 and phase E with four lanes per patch (a quarter of the latency the other waves wait for) from R = 3 on:
    // +11 % at sw 32, +3 % at sw 16
    constexpr bool E4 = R >= 3;
    const int T = blockDim.x;
    const int NC = 2 * d.sw + 16, XQ = d.xq;
    uint32_t* win = lds + L.win;                           // [win_rows][pitch_dw]
    uint32_t* anchor = lds + L.anchor;                     // [NB][ANCHOR_STRIDE]
    uint32_t* best = lds + L.best;                         // [NB] keys, 8 bytes apart (low dword used here)
    uint32_t* count = lds + L.count;
    uint64_t* s8 = (uint64_t*)(lds + L.s8);                // [s8_rows][XQ] packed u16 x 4: S8(y, 4s .. 4s+3)
    uint32_t* work = lds + L.work;                         // [NB*64*R] entries: interior<<29 | wave<<25 | lane<<19 | k<<16 | LB
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const SeaArgs c = launch_args();
    const WaveBlock wb = wave_block(d, c, trow, bcol0, wave);
    const int brow = wb.brow, bcol = wb.bcol;
    const bool wave_ok = wb.ok;                            // ragged last tile of a block row / column
    const int r0 = brow * 16, c0 = bcol * 16;
    const int prow = lane >> 2, q = lane & 3;

    // ---- A': 8x8 box sums of the window (bbme_sea_common.h) ------------------------------------
    box_sums8<R, FIXED>(d, win, s8, tid);
    clk.mark(ST_BOX, lane);
    __syncthreads();
    clk.mark(ST_BOX_WAIT, lane);
    behind_box_sums();                                     // persistent_tiles: the next tile's prefetch of the waves that held chunks

    // ---- B: lower bounds of the wave's own block --------------------------------------------
    const int lo_r = max(0, d.sw - r0), hi_r = min(NC - 1, c->H - 16 - r0 + d.sw);
    const bool rows_inside = NC == 16 * R && lo_r == 0 && hi_r == NC - 1;   // and no padding candidates
    uint32_t ub_key = 0xFFFFFFFFu;
    if (wave_ok) {
        const int lo_c = max(0, d.sw - c0), hi_c = min(NC - 1, c->W - 16 - c0 + d.sw);
        // per patch k: the smallest bound of its candidates, no index (a patch without valid candidates: 0xFFFFFFFF)
        uint32_t pmin[R];
        const uint64_t* s8blk = s8 + 16 * wb.wr * XQ + wb.wc * 4;                        // the block's corner of the table
        const uint64_t* sp0 = s8blk + prow * R * XQ + q * R;
        const bool cols_inside = NC == 16 * R && lo_c == 0 && hi_c == NC - 1;           // and no padding candidates
        if (rows_inside && cols_inside)                                                // wave-uniform, all three
            lower_bounds<R, GUARD_NONE, VERT>(sp0, XQ, prow, q, pa, pb, lo_r, hi_r, lo_c, hi_c, pmin);
        else if (R <= 3 && cols_inside)                                                // R >= 4: see lower_bounds
            lower_bounds<R, GUARD_ROWS, VERT>(sp0, XQ, prow, q, pa, pb, lo_r, hi_r, lo_c, hi_c, pmin);
        else
            lower_bounds<R, GUARD_ALL, VERT>(sp0, XQ, prow, q, pa, pb, lo_r, hi_r, lo_c, hi_c, pmin);
        // pkd[k] = (smallest bound of patch k) << 13 | scan index of the patch's FIRST candidate: no candidate of the
        // patch can have a smaller key (sad << 13 | scan index).  A patch without valid candidates keeps 0xFFFFE000 | index,
        // above every real key (sad <= 65280 < 2^16).
        const uint32_t first_idx = (uint32_t)((q * 4 * R) * NC + prow * R);
        // what this lane's list entries share (ENT_INTERIOR above)
        const uint32_t ent0 = (rows_inside && cols_inside ? ENT_INTERIOR : 0u) | ((uint32_t)wave << 25) | ((uint32_t)lane << 19);
        uint32_t pkd[R], lane_min = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            pkd[k] = (pmin[k] << 13) | (first_idx + (uint32_t)(4 * k * NC));
            lane_min = min(lane_min, pmin[k]);
        }
        const uint32_t lane_lb = lane_min << 13;                       // this lane's smallest bound << 13 (none: 0xFFFFE000)
        uint32_t lb_key = lane_min != 0xFFFFFFFFu ? lane_lb + ((uint32_t)lane << 7) : 0xFFFFFFFFu;
        // ---- C: upper bound from three real candidates (cooperative 16x16 SAD, one dword per lane)
        lb_key = wave_min_u32(lb_key);                                 // smallest bound << 13 | first lane that holds it << 7
        {
            // the zero vector is always valid, so the minimum is a real bound and one of the lane's candidates has it
            const int idx1 = min_bound_candidate<R, VERT>(s8blk, XQ, NC, (int)(lb_key >> 7) & 63, lb_key >> 13, pa, pb,
                                                          lo_r, hi_r, lo_c, hi_c, lane);   // min-LB candidate
            const int idx0 = d.sw * NC + d.sw;                                       // zero vector
            const int arow = lane >> 2, aj = lane & 3;
            uint32_t packed = 0;                           // two 16x16 SADs (<= 65280 each) in one register
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                const int idx = which ? idx1 : idx0;
                const int ci = idx / NC, ri = idx - ci * NC;
                const int byte = wb.wc * 16 + ci + 4 * aj;
                const uint32_t* p = win + (16 * wb.wr + ri + arow) * d.pitch_dw + (byte >> 2);
                const uint32_t v = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)byte & 3u);
                packed += __builtin_amdgcn_sad_u8(v, mine, 0u) << (16 * which);
            }
            packed = wave_sum_u32(packed);
            ub_key = min(((packed & 0xFFFFu) << 13) | (uint32_t)idx0, ((packed >> 16) << 13) | (uint32_t)idx1);
            // third probe: the vector this wave's block of the PREVIOUS tile of the workgroup ended with (the block one
            // tile to the left, or wherever the schedule came from): spatial coherence makes it a good guess when the
            // smallest bound does not name the best candidate.  Skipped (wave-uniform) when it is one of the two candidates
            // above or lies outside this block's valid window.  Surviving patches 5.4 -> 4.8 % on the synthetic pan, 9.3 ->
            // 8.6 % / 16.8 -> 15.7 % on the real frames; +0.6 .. +1.8 % pairs/s (same-box A/B, round 3).
            const int idxp = (int)(best[2 * wave + 1] & 0x1FFFu);
            const int cip = idxp / NC, rip = idxp - cip * NC;
            if (idxp != idx0 && idxp != idx1 && cip >= lo_c && cip <= hi_c && rip >= lo_r && rip <= hi_r) {
                const int byte = wb.wc * 16 + cip + 4 * aj;
                const uint32_t* p = win + (16 * wb.wr + rip + arow) * d.pitch_dw + (byte >> 2);
                const uint32_t v = __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)byte & 3u);
                const uint32_t sadp = wave_sum_u32(__builtin_amdgcn_sad_u8(v, mine, 0u));
                ub_key = min(ub_key, (sadp << 13) | (uint32_t)idxp);
            }
        }
        // ---- C2 (round 4): ordered evaluation inside a crowded block.  Where the first upper bound leaves more than
        // SeaDev::quota patches (real content: the smallest bound does not name the best candidate, but the best one sits
        // among the small bounds, tools/ub_study.py), the wave scores the up to 16 patches with the smallest bounds itself,
        // four lanes each, before anything is listed: no barrier, a full wave, and phase D then tests the rest against
        // (almost) the block's true minimum.  Any upper bound that is a real candidate's key keeps the result exact
        // (bbme.py:171: only a smaller key replaces the best one).
        uint32_t own_lim = 0;                              // keys below it were scored here (wave-uniform)
        int n_w = 0;                                       // patches the first upper bound leaves (statistics)
        clk.mark(ST_BC, lane);
        if constexpr (E4) {
            // crowded?  Lanes with a surviving patch are counted first (one ballot); the exact count only where it matters
            const int engage = c->engage;
            if (c->quota > 0 && __popcll(__ballot(lane_lb < ub_key)) > engage / 3) {
#pragma unroll
                for (int k = 0; k < R; ++k) n_w += __popcll(__ballot(pkd[k] < ub_key));
                if (n_w > engage) {
                    own_lim = first_round_limit(c, lb_key >> 13, ub_key >> 13, 13, [&](uint32_t lim) {
                        int c = 0;
#pragma unroll
                        for (int k = 0; k < R; ++k) c += __popcll(__ballot(pkd[k] < lim));
                        return c;
                    });
                    own_lim = min(own_lim, ub_key);
                    // the chosen patches -> this wave's 16 slots (ties at the smallest bound may exceed them: the surplus
                    // keeps own_rank >= 16 and is listed by phase D like everything else)
                    uint32_t* own = lds + L.own + 16 * wave;
                    int base_rank = 0;
                    uint32_t listed_here = 0;              // bit k: patch k of this lane was scored here
#pragma unroll
                    for (int k = 0; k < R; ++k) {
                        const bool sel = pkd[k] < own_lim;
                        const unsigned long long m = __ballot(sel);
                        const int rank = base_rank + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        if (sel && rank < 16) {
                            own[rank] = ent0 | ((uint32_t)k << 16) | (pkd[k] >> 13);
                            listed_here |= 1u << k;
                        }
                        base_rank += __popcll(m);
                    }
                    const int n_own = min(base_rank, 16);
                    const bool act = (lane >> 2) < n_own;
                    const uint32_t ent = act ? own[lane >> 2] : 0u;
                    uint32_t key = eval_patch_quad<R>(d, c->H, c->W, win, anchor, ent, act, lane & 3, trow, bcol0, NC);
                    ub_key = min(ub_key, wave_min_u32(key));
#pragma unroll
                    for (int k = 0; k < R; ++k)
                        if (listed_here & (1u << k)) pkd[k] = 0xFFFFFFFFu;       // done: never listed
                    if (lane == 0) atomicAdd(count + 5, (uint32_t)n_own);      // statistics
                }
            }
        }
        clk.mark(ST_C2, lane);
        if (lane == 0) best[2 * wave] = ub_key;
        // ---- D: surviving patches -> workgroup list.  A candidate replaces the best one only with a smaller
        // key (sad << 13 | scan index: bbme.py:171 keeps the FIRST strict minimum), and its key is at least
        // LB << 13 | index, so a patch whose smallest possible key -- its bound with the scan index of its first
        // candidate -- does not undercut ub_key holds no winner.  On flat content (every cost ties) this
        // leaves nothing behind the first candidate in scan order instead of everything.
        // One reservation per wave and tile: the R ballots give the wave's total, lane 0 adds it to the list's length, and
        // lane l writes entry k behind the entries of column groups j < k and of the lanes below it.  (One atomicAdd(count, 1)
        // per column group is expanded into a ballot, two v_mbcnt, the add by one lane, a wait and a v_readfirstlane each:
        // R LDS round trips in a row.)  Only the order inside the list differs, which no result depends on.
        unsigned long long pushes[R];
        int pushed = 0;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            pushes[k] = __ballot(pkd[k] < ub_key);
            pushed += __popcll(pushes[k]);
        }
        if (pushed) {                                      // wave-uniform
            uint32_t base = 0;
            if (lane == 0) base = lds_add_rtn(count, (uint32_t)pushed);
            uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
            for (int k = 0; k < R; ++k) {
                if (pkd[k] < ub_key)
                    work[__builtin_amdgcn_mbcnt_hi((uint32_t)(pushes[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pushes[k], slot))] =
                        ent0 | ((uint32_t)k << 16) | (pkd[k] >> 13);   // LB <= 65280
                slot += (uint32_t)__popcll(pushes[k]);
            }
        }
        // statistics: what the first bound had left and C2 took or pruned
        if (own_lim && lane == 0) atomicAdd(count + 4, (uint32_t)(n_w - pushed));
    }
    clk.mark(ST_D, lane);
    __syncthreads();
    clk.mark(ST_D_WAIT, lane);
    const SeaArgs ce = launch_args();                      // phases E and F, and the test in front of them
    if (ce->redo_list && (int)*count > ce->redo_threshold) {     // workgroup-uniform: hostile tile, brute force is cheaper
        if (tid == 0) push_redo(ce, tile_id, (int)(blockIdx.x & 7));
        return true;
    }
    const int H = ce->H, W = ce->W;

    if constexpr (E4) {
        // ---- E, R >= 3: four lanes per patch (the body of eval_patch_quad, kept inline here: the
        // shared function cost this loop 1.2 % in register allocation, same-box A/B round 4) ---------------------------------------------------
        // Lane `sub` of a quad takes anchor rows 4*sub .. 4*sub+3 (R+3 window rows, 16*R QSADs); the four
        // partial u16x4 sums are added inside the quad with DPP moves.
        const int n = (int)*count;
        const int sub = lane & 3;
        for (int base = 0; base < n; base += T / 4) {
            const int e = base + (tid >> 2);
            bool active = e < n;
            uint32_t ent = 0;
            if (active) ent = work[e];
            const int w2 = (ent >> 25) & 15, l2 = (ent >> 19) & 63, k2 = (ent >> 16) & 7;
            const int wr2 = wave_row(d, w2), wc2 = w2 - wr2 * d.tc;     // the patch's block inside the tile
            const int prow2 = l2 >> 2, q2 = l2 & 3;
            // dropped by a tightened UB (same key rule as phase D); the quad is uniform in `active` (same entry),
            // so the DPP exchange below is safe
            const uint32_t first2 = (uint32_t)((q2 * 4 * R + 4 * k2) * NC + prow2 * R);     // scan index of the patch's first candidate
            active = active && (((ent & 0xFFFFu) << 13) | first2) < best[2 * w2];
            uint64_t acc[R];
    #pragma unroll
            for (int i = 0; i < R; ++i) acc[i] = any_u64();  // idle quads add and exchange whatever they hold; nobody reads it
            if (active) {
    #pragma unroll
                for (int i = 0; i < R; ++i) acc[i] = 0;
                const uint32_t* lrow = win + (16 * wr2 + prow2 * R + 4 * sub) * d.pitch_dw + wc2 * 4 + q2 * R + k2;
                const uint32_t* an = anchor + w2 * ANCHOR_STRIDE + 16 * sub;
    #pragma unroll
                for (int t = 0; t < R + 3; ++t) {
                    uint64_t w[4];
    #pragma unroll
                    for (int s = 0; s < 4; ++s) w[s] = *(const u64_a4*)(lrow + t * d.pitch_dw + s);
    #pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const int a = t - i;                   // anchor row 4*sub + a
                        if (a < 0 || a > 3) continue;
                        const u32x4 ar = *(const u32x4*)(an + a * 4);
    #pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[i] = __builtin_amdgcn_qsad_pk_u16_u8(w[j], ar[j], acc[i]);
                    }
                }
            }
            // sum over the quad: plain 32-bit adds on the packed u16 pairs (a 16x16 SAD is at most 65280, so no partial
            // sum carries into the upper half) -- they take the DPP operand directly, v_pk_add_u16 needs a move first
    #pragma unroll
            for (int i = 0; i < R; ++i) {
                uint32_t lo = (uint32_t)acc[i], hi = (uint32_t)(acc[i] >> 32);
                lo += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0xB1, 0xF, 0xF, false);            // quad_perm [1,0,3,2]
                hi += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0xB1, 0xF, 0xF, false);
                lo += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0x4E, 0xF, 0xF, false);            // quad_perm [2,3,0,1]
                hi += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0x4E, 0xF, 0xF, false);
                asm volatile("" : "+v"(lo), "+v"(hi));     // pinned here: sunk under `active` the adds leave their DPP moves behind
                acc[i] = ((uint64_t)hi << 32) | lo;
            }
            if (active) {
                // every lane of the quad holds the patch's R x 4 sums now; lane `sub` turns column `sub` into keys
                // (R candidates instead of 4 R on one lane), the quad's minimum goes to the block's best key
                const int ci = q2 * 4 * R + 4 * k2 + sub, ri0 = prow2 * R;
                const uint32_t shift = (uint32_t)(sub & 1) * 16u;
                uint32_t key = 0xFFFFFFFFu;
                if (ent & ENT_INTERIOR) {
                    // whole window inside the frame: keys relative to the column's first candidate, base added once
    #pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const uint32_t word = (sub & 2) ? (uint32_t)(acc[i] >> 32) : (uint32_t)acc[i];
                        const uint32_t sad = __builtin_amdgcn_ubfe(word, shift, 16u);
                        key = min(key, (sad << 13) + (uint32_t)i);
                    }
                    key += first2 + (uint32_t)(sub * NC);
                } else {
                    // an edge block: the window limits are formed here only (lanes of one wave serve different blocks)
                    const int c02 = (bcol0 + wc2) * 16, r02 = (trow * d.tr + wr2) * 16;
                    const int lo_c = max(0, d.sw - c02), hi_c = min(NC - 1, W - 16 - c02 + d.sw);
                    const int lo_r2 = max(0, d.sw - r02), hi_r2 = min(NC - 1, H - 16 - r02 + d.sw);
    #pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const int ri = ri0 + i;
                        if (ci < lo_c || ci > hi_c || ri < lo_r2 || ri > hi_r2) continue;
                        const uint32_t word = (sub & 2) ? (uint32_t)(acc[i] >> 32) : (uint32_t)acc[i];
                        const uint32_t sad = __builtin_amdgcn_ubfe(word, shift, 16u);
                        key = min(key, (sad << 13) | (uint32_t)(ci * NC + ri));
                    }
                }
                // quad minimum (a disabled source lane would hand back the minimum's identity; quads are uniform in `active`)
                key = min(key, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)key, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
                key = min(key, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)key, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
                if (sub == 0 && key != 0xFFFFFFFFu) atomicMin(&best[2 * w2], key);
            }
            clk.mark(ST_E, lane);
            __syncthreads();
            clk.mark(ST_E_WAIT, lane);
        }
    } else {
        // ---- E: evaluate the listed patches, one per lane ---------------------------------------
        const int n = (int)*count;
        for (int base = 0; base < n; base += T) {
            const int e = base + tid;
            bool active = e < n;
            uint32_t ent = 0;
            if (active) {
                ent = work[e];
                const uint32_t first = (uint32_t)(((int)((ent >> 19) & 3) * 4 * R + 4 * (int)((ent >> 16) & 7)) * NC + (int)((ent >> 21) & 15) * R);
                active = (((ent & 0xFFFFu) << 13) | first) < best[2 * ((ent >> 25) & 15)];      // dropped by a tightened UB
            }
            if (active) {
                const int w2 = (ent >> 25) & 15, l2 = (ent >> 19) & 63, k2 = (ent >> 16) & 7;
                const int wr2 = wave_row(d, w2), wc2 = w2 - wr2 * d.tc;     // the patch's block inside the tile
                const int prow2 = l2 >> 2, q2 = l2 & 3;
                const uint32_t* lrow = win + (16 * wr2 + prow2 * R) * d.pitch_dw + wc2 * 4 + q2 * R + k2;
                const uint32_t* an = anchor + w2 * ANCHOR_STRIDE;
                uint64_t acc[R];
    #pragma unroll
                for (int i = 0; i < R; ++i) acc[i] = 0;
    #pragma unroll
                for (int t = 0; t < R + 15; ++t) {
                    uint64_t w[4];
    #pragma unroll
                    for (int s = 0; s < 4; ++s) w[s] = *(const u64_a4*)(lrow + t * d.pitch_dw + s);
    #pragma unroll
                    for (int i = 0; i < R; ++i) {
                        const int a = t - i;
                        if (a < 0 || a > 15) continue;
                        const u32x4 ar = *(const u32x4*)(an + a * 4);
    #pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[i] = __builtin_amdgcn_qsad_pk_u16_u8(w[j], ar[j], acc[i]);
                    }
                }
                const int ci0 = q2 * 4 * R + 4 * k2, ri0 = prow2 * R;
                uint32_t key = 0xFFFFFFFFu;
                if (ent & ENT_INTERIOR) {
                    // whole window inside the frame: keys relative to the patch's first candidate, base added once
    #pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4)
    #pragma unroll
                        for (int i = 0; i < R; ++i) {
                            const uint32_t sad = (uint32_t)(acc[i] >> (16 * e4)) & 0xFFFFu;
                            key = min(key, (sad << 13) + (uint32_t)(e4 * NC + i));
                        }
                    key += (uint32_t)(ci0 * NC + ri0);
                } else {
                    const int c02 = (bcol0 + wc2) * 16, r02 = (trow * d.tr + wr2) * 16;
                    const int lo_c = max(0, d.sw - c02), hi_c = min(NC - 1, W - 16 - c02 + d.sw);
                    const int lo_r2 = max(0, d.sw - r02), hi_r2 = min(NC - 1, H - 16 - r02 + d.sw);
    #pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                        const int ci = ci0 + e4;
                        if (ci < lo_c || ci > hi_c) continue;
    #pragma unroll
                        for (int i = 0; i < R; ++i) {
                            const int ri = ri0 + i;
                            if (ri < lo_r2 || ri > hi_r2) continue;
                            const uint32_t sad = (uint32_t)(acc[i] >> (16 * e4)) & 0xFFFFu;
                            key = min(key, (sad << 13) | (uint32_t)(ci * NC + ri));
                        }
                    }
                }
                if (key != 0xFFFFFFFFu) atomicMin(&best[2 * w2], key);
            }
            clk.mark(ST_E, lane);
            __syncthreads();
            clk.mark(ST_E_WAIT, lane);
        }

    }
    // ---- F: result ------------------------------------------------------------------------------
    if (wave_ok && lane == 0) {
        const int idx = (int)(best[2 * wave] & 0x1FFF);
        const int ci = idx / NC, ri = idx - ci * NC;
        int32_t* o = ce->mf + (((long long)pair * ce->nbr + brow) * ce->nbc + bcol) * 2;
        o[0] = ci - d.sw;
        o[1] = ri - d.sw;
        best[2 * wave + 1] = (uint32_t)idx;                   // next tile's third probe
    }
    return false;
}

// What the shared tile drivers (bbme_sea_common.h: one_tile, persistent_tiles) need from this kernel.
// FIXED: the geometry-fixed instances (fix_geometry), whose strides are compile-time constants
// VERT: phase B pairs its operands vertically (lower_bounds); the anchor sums are packed to match
template <int R, bool FIXED = false, bool VERT = true>
struct MaeTile {
    struct Pre { uint32_t pa, pb; };                       // anchor quadrant sums: [A0, A2], [A1, A3] (VERT) or [A0, A1], [A2, A3]
    static __device__ __forceinline__ Pre prep(uint32_t* lds, const Layout& L, int wave, int lane, bool wave_ok, uint32_t mine)
    {
        Pre p = { 0, 0 };
        if (wave_ok) {
            lds[L.anchor + wave * ANCHOR_STRIDE + lane] = mine;
            uint32_t a01, a23;
            anchor_quadrants(mine, &a01, &a23);            // shared with the MSE kernel, which pairs horizontally
            p.pa = VERT ? pair_u16(a01, a23, false) : a01;
            p.pb = VERT ? pair_u16(a01, a23, true) : a23;
        }
        return p;
    }
    template <class Behind>
    static __device__ __forceinline__ bool phases(const SeaGeo& d, uint32_t* lds, const Layout& L, int pair, int trow, int bcol0,
                                                  uint32_t mine, const Pre& p, int tid, int tile_id, PhaseClock& clk, Behind&& behind_box_sums)
    {
        return tile_phases<R, FIXED, VERT>(d, lds, L, pair, trow, bcol0, mine, p.pa, p.pb, tid, tile_id, clk, behind_box_sums);
    }
    static __device__ __forceinline__ bool holds_chunks(const SeaGeo& d, int wave) { return holds_box_chunks<R>(d, wave); }
    static __device__ __forceinline__ int probe_word(const Layout& L, int wave) { return L.best + 2 * wave + 1; }
};

template <int R>
__global__ void __launch_bounds__(1024) k_exh_sea16(SeaDev d)
{
    extern __shared__ uint32_t lds[];
    const SeaGeo g = d;                                    // the by-value copy is read for its geometry only
    one_tile<MaeTile<R>>(g, lds, layout_of(g, R));
}

// Which persistent instances pair vertically ("Bound minima"): all but the ones the shared pairs would
// cost a spilled VGPR of the prefetched tile
constexpr bool vertical_pairs(int R, int NV) { return !(R == 5 && NV == 16); }

// Which persistent instances order the next tile's prefetch by who holds box-sum chunks (persistent_tiles, LATE): all but the
// run-time-geometry ones of R = 3.  Those sit at the 64 VGPRs and 80 SGPRs of eight waves per SIMD: for the second copy of
// the prefetch <3, 6, 0> spills 20 more SGPRs to VGPR lanes (read back on every tile), <3, 8, 0> three VGPRs, <3, 16, 0>
// eight ("Order")
constexpr bool late_prefetch(int R, int GEO) { return !(R == 3 && GEO == 0); }

template <int R, int NV, int GEO = 0>
__global__ void __launch_bounds__(1024, (R <= 3 ? 8 : 6)) k_exh_sea16p(SeaDev d)
{
    extern __shared__ uint32_t lds[];
    SeaGeo g = d;                                          // the by-value copy is read for its geometry only
    fix_geometry<R, GEO>(g);
    const Layout L = layout_of(g, R);
    if ((threadIdx.x & 63) == 0) lds[L.best + 2 * (threadIdx.x >> 6) + 1] = (uint32_t)(g.sw * (2 * g.sw + 16) + g.sw);   // third probe of the first tile: the zero vector
    persistent_tiles<NV, MaeTile<R, GEO != 0, vertical_pairs(R, NV)>, late_prefetch(R, GEO)>(g, lds, L);
}

// What the shared host launcher (bbme_sea_common.h: launch_sea) needs from this norm.
struct MaeLaunch {
    static constexpr const char* persistent_name = "k_exh_sea16p";
    static constexpr const char* one_tile_name = "k_exh_sea16";
    static int no_plan()
    {
        gme_set_error("search window too large for LDS");
        return GME_ERR_ARG;
    }
    static void tables(SeaDev& d, const BbmeJob&) { d.sqbox = nullptr; d.sqbox_stride = 0; }
    // ordered evaluation inside crowded blocks (phase C2; bbme_sea_common.h: SeaDev::quota); GME_SEA_QUOTA=0 switches it off
    static void ordered(SeaDev& d)
    {
        d.quota = getenv("GME_SEA_QUOTA") ? atoi(getenv("GME_SEA_QUOTA")) : SEA_DEFAULT_QUOTA;
        d.bisect = getenv("GME_SEA_BISECT") ? atoi(getenv("GME_SEA_BISECT")) : SEA_DEFAULT_BISECT;
        d.engage = getenv("GME_SEA_ENGAGE") ? atoi(getenv("GME_SEA_ENGAGE")) : SEA_DEFAULT_ENGAGE;
        if (d.engage < d.quota) d.engage = d.quota;
    }
    // R = 2, 3 with more than 8 staging rows per thread would spill the prefetched tile (64 VGPRs at
    // 8 waves/SIMD); those shapes keep the one-tile kernel
    static bool fits(int R, int nv) { return R <= 1 || R >= 4 || nv <= 8; }
    template <int R, int NV, int GEO = 0>
    static void persistent(dim3 grid, dim3 block, size_t lds, hipStream_t s, const SeaDev& d)
    {
        hipLaunchKernelGGL((k_exh_sea16p<R, NV, GEO>), grid, block, lds, s, d);
    }
    template <int R>
    static void one_tile(dim3 grid, dim3 block, size_t lds, hipStream_t s, const SeaDev& d)
    {
        hipLaunchKernelGGL((k_exh_sea16<R>), grid, block, lds, s, d);
    }
};

}  // namespace

bool bbme_sea_applies(int bs, int sw, int procedure, int pnorm)
{
    if (procedure != GME_SEARCH_EXHAUSTIVE || bs != 16 || pnorm != GME_NORM_MAE) return false;
    if (sw < 0 || sw % 4 != 0) return false;
    const int NC = 2 * sw + 16;
    return (NC + 15) / 16 <= 5 && NC * NC <= 8192 && !getenv("GME_FORCE_GENERIC") && !getenv("GME_EXH_BRUTE");
}

#ifdef SEA_PHASE_STAMPS
// Phase-stamp variant only (bbme_sea_common.h: PhaseClock): the totals of the persistent kernels since the last reset,
// out[16 waves][ST_SLOTS] cycles; norm 0: MAE, 1: MSE
int sea_stamps_read_mse(unsigned long long* out, int reset);
extern "C" GME_API int gme_sea_phase_stamps(int norm, unsigned long long* out, int reset)
{
    return norm ? sea_stamps_read_mse(out, reset) : sea::sea_stamps_read(out, reset);
}
#endif

int launch_bbme_sea(gme_ctx* ctx, const BbmeJob& job, bool* handled)
{
    *handled = false;
    if (!bbme_sea_applies(job.bs, job.sw, job.procedure, job.pnorm)) return GME_OK;
    return launch_sea<MaeLaunch>(ctx, job, handled);
}
