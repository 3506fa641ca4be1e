// Shared pieces of the successive-elimination exhaustive kernels (bbme_sea.hip: MAE,
// bbme_sea_mse.hip: MSE): launch descriptor, LDS layout, tile shapes, window staging, 8x8 box sums,
// the one-tile and persistent tile drivers, the host launcher both norms share.
#pragma once
#include <stdlib.h>

#include "gme_internal.h"

namespace sea {

// weight of window sharing in the tile-shape score (plan()); tuned by same-box sweeps
constexpr double SHARE_WEIGHT = 0.5;

// The launch descriptor is the kernels' only parameter, by value.  It has two parts.
//
// SeaGeo: tile geometry and search range -- what the hot bodies use per candidate or per row.  A kernel copies this part
// into registers (a geometry-fixed instance folds all of it to constants, fix_geometry).
struct SeaGeo {
    int sw;
    int tr, tc, nb;               // a tile is tr x tc macroblocks, one wave each: nb = tr * tc waves per workgroup
    uint32_t magic_tc;            // wave / tc (div_small)
    int pitch_dw, win_rows;       // staged window: 16R + 15 + 16 (tr - 1) rows of pitch_dw dwords
    int s8_rows;                  // rows of the box-sum table: 16R + 8 + 16 (tr - 1)
    int rstep;                    // staging: window rows covered by one sweep of the workgroup (T / pitch_dw)
    uint32_t magic_pitch;         // n / pitch_dw == (n * magic_pitch) >> 20 for n < 4096 (div_small)
    uint32_t magic_xq;            // same for n / xq
    int xq;                       // S8 quads (4 columns each) per window row
};

// SeaDev adds everything a tile needs a few times at most: planes, frame size, schedule, lists, statistics.  Device code
// never reads these from the by-value copy -- held in SGPRs across the persistent kernels' tile loop they do not fit
// the 80 SGPRs of 8 waves per SIMD and were spilled to VGPR lanes, to be read back one v_readlane_b32 each on every
// tile.  It reads them from the kernel-argument segment where it needs them (SeaArgs, launch_args() below): scalar
// loads, no vector instruction.  The fields are ordered so that what one block of the tile loop reads is contiguous
// (the offsets are asserted behind the struct):
//   [48, 112)   the prefetch: tile number -> pair, tile row, block column; planes; frame rows
//   [100, 152)  the phases: frame size, ordered evaluation, redo list, result
//   [152, 184)  schedule, statistics, MSE table
struct SeaDev : SeaGeo {
    unsigned long long magic_wpp; // persistent kernel: n / wg_per_pair == (n * magic_wpp) >> 40 for n < 2^21
    unsigned long long magic_wpr; // same for n / wg_per_row
    const uint8_t* cur;
    const uint8_t* prev;
    long long plane_stride;
    int wg_per_pair, wg_per_row;  // tiles per pair / per block row
    int pitch, H;
    int nbr, nbc;
    int W, pairs;
    int32_t* mf;
    // Hostile content (nothing correlates: a scene cut, noise): the bound prunes little and phase E's one-patch-
    // per-lane evaluation costs more than evaluating everything in the regular layout of k_exh_qsad16 / k_exh_dot16.
    // A tile whose list is longer than redo_threshold skips phases E and F and goes to redo_list instead
    // (entry = tile number inside its XCD's tiles << 3 | xcd); the redo kernel launched behind this one searches it.
    uint32_t* redo_list;          // or null: no fallback
    int redo_threshold;
    // Ordered evaluation (round 4, phase C2 of the kernels): a block whose first upper bound leaves more than `quota`
    // patches scores those with the smallest bounds inside its own wave first (threshold by `bisect` halvings of [smallest
    // bound, UB], at most `quota` <= 16 pass) and lists the rest against the upper bound that leaves.  On real content the
    // smallest bound does not name the best candidate, but the best one sits among the small bounds: phase D then sees
    // (almost) the block's true minimum (tools/ub_study.py).  quota <= 0: off.  `engage`: survivors from which a block
    // counts as crowded (>= quota).
    int quota, bisect, engage;
    int dynamic;                  // persistent kernel: draw tiles from the per-XCD counters (else a static stride)
    int tile_rows;                // tile rows per pair (host: grid_for)
    uint32_t* status;             // the context's status words (gme_internal.h: GME_STATUS_*):
                                  //   + GME_STATUS_TILECTR  persistent kernel, dynamic schedule: one tile counter per XCD, 16 words apart
                                  //   + GME_STATUS_STATS    per XCD, 16 words apart: [0] patches evaluated exactly (phase E), [1] tiles handed to
                                  //                         the brute-force redo kernel, [2] patches phase D listed (what one
                                  //                         round would have evaluated; == [0] without ordered evaluation)
                                  //   + GME_STATUS_REDO     [0] length of redo_list
    const uint32_t* sqbox;        // MSE only: 16x16 box sums of squares of `cur`, [pairs][H][pitch]
    long long sqbox_stride;
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"     // a base and a derived class with members: not standard-layout, offsets still fixed
static_assert(sizeof(SeaGeo) == 48 && __builtin_offsetof(SeaDev, magic_wpp) == 48 && __builtin_offsetof(SeaDev, nbc) == 108 &&
              __builtin_offsetof(SeaDev, H) == 100 && __builtin_offsetof(SeaDev, engage) == 148 && sizeof(SeaDev) == 184,
              "SeaDev: the groups a block of the tile loop reads with one wide scalar load");
#pragma clang diagnostic pop

// The kernel's own argument segment, seen as the SeaDev it holds (the only parameter: offset 0).  Every call returns a
// pointer the compiler knows nothing about (the empty asm), so the loads through it stay where they are written: they
// are neither hoisted out of the tile loop nor shared between two calls, and nothing read through it stays live
// longer than its block.  Take one per block of work (a prefetch, a tile's phases, the loop tail), never one per kernel.
typedef const __attribute__((address_space(4))) SeaDev* SeaArgs;
__device__ __forceinline__ SeaArgs launch_args()
{
    SeaArgs p = (SeaArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
// gridDim.x from the same pointer: the hidden arguments follow the explicit ones in the segment (8-byte aligned), and
// their first word is the grid's workgroup count in x (hidden_block_count_x, code object v5 and later; the kernels
// read blockDim.x too, so the hidden block is always part of their segment).  One load with a constant offset: going
// through __builtin_amdgcn_implicitarg_ptr() would put a second base register into the loop.
static_assert(sizeof(SeaDev) % 8 == 0, "the hidden arguments start right behind SeaDev");
__device__ __forceinline__ int launch_groups_x(SeaArgs c)
{
    return (int)*(const __attribute__((address_space(4))) uint32_t*)(c + 1);
}

typedef uint64_t u64_a4 __attribute__((aligned(4)));

// Phase stamps (diagnostic variant, tools/build_variant.sh <name> -DSEA_PHASE_STAMPS; tools/sea_phase_stamps.py prints the table):
// where a wave's time goes inside a tile.  Lane 0 of every wave reads the shader clock (s_memtime) at the end of each span
// below and adds the cycles since the previous reading to the wave's total of that span, in LDS behind the tile's own
// data (Layout::stamps, [nb][ST_SLOTS]); persistent_tiles adds the workgroup's totals to stamp_totals (a device array per
// norm, [16 waves][ST_SLOTS]) when it has walked its tiles, and sea_stamps_read() hands that to the host.  Every reading
// waits for the wave's outstanding LDS and scalar loads (s_waitcnt lgkmcnt(0)), so the stamped kernel is slower than the
// tree's and its figures attribute time, they do not measure it.  Without the macro PhaseClock is empty and every mark()
// compiles to nothing: the tree's library has neither the array nor the reader.
enum {
    ST_HEAD,        // tile head: prefetched registers -> LDS, anchor statistics, thread 0's counters
    ST_HEAD_WAIT,   // the barrier behind it
    ST_FETCH,       // the next tile's number and the issue of its prefetch
    ST_BOX,         // A': box sums
    ST_BOX_WAIT,    // A's barrier
    ST_BC,          // B and C: bounds, the three probes
    ST_C2,          // C2: ordered evaluation of a crowded block (0 where it does not engage)
    ST_D,           // D: listing
    ST_D_WAIT,      // D's barrier
    ST_E,           // E: the chunks' work (MSE: with level 2 of the bound)
    ST_E_WAIT,      // E: the chunks' barriers
    ST_F_TAIL,      // F, the loop tail (hostile streaks), up to the next tile's head
    ST_TILES,       // tiles this wave walked
    ST_SLOTS = 16
};
#ifdef SEA_PHASE_STAMPS
static __device__ unsigned long long stamp_totals[16 * ST_SLOTS];
struct PhaseClock {
    uint32_t slot, last;                                   // LDS byte address of the wave's totals; the previous reading (both wave-uniform)
    __device__ __forceinline__ void start(uint32_t* totals, int wave)
    {
        slot = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)(totals + wave * ST_SLOTS);
        last = (uint32_t)__builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void add(int span, int lane, uint32_t v)
    {
        // written out: an atomicAdd from one lane is rewritten into a wave-wide aggregation (lds_add_rtn in bbme_sea.hip)
        if (lane == 0) asm volatile("ds_add_u32 %0, %1" : : "v"(slot + 4u * (uint32_t)span), "v"(v) : "memory");
    }
    __device__ __forceinline__ void mark(int span, int lane)
    {
        const uint32_t now = (uint32_t)__builtin_amdgcn_s_memtime();
        add(span, lane, now - last);
        last = now;
    }
};
// static: each norm's file reads its own stamp_totals (as one inline function of both files the linker kept a single copy,
// and the MSE reader returned the MAE array)
static inline int sea_stamps_read(unsigned long long* out, int reset)
{
    GME_HIP_TRY(hipDeviceSynchronize());
    GME_HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(stamp_totals), sizeof(stamp_totals)));
    if (reset) {
        void* p = nullptr;
        GME_HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(stamp_totals)));
        GME_HIP_TRY(hipMemset(p, 0, sizeof(stamp_totals)));
    }
    return GME_OK;
}
#else
struct PhaseClock {
    __device__ __forceinline__ void add(int, int, uint32_t) {}
    __device__ __forceinline__ void mark(int, int) {}
};
#endif


// wave_min_u32 / wave_sum_u32 (DPP reductions): gme_internal.h
#define SEA_DPP(v, ctrl) GME_DPP(v, ctrl)

// n / dv for n < 4096 and dv < 256 without the 20-odd instructions of an emulated division:
// magic = 2^20 / dv + 1 overshoots the reciprocal by < 2^-20, so the product is off by < 2^-8 < 1 / dv.
constexpr uint32_t div_magic(int dv) { return (1u << 20) / (uint32_t)dv + 1u; }
// same idea for n < 2^21, dv < 2^18: (n * magic40) >> 40, error < 2^21 / 2^40 < 1 / dv
inline unsigned long long div_magic40(int dv) { return (1ull << 40) / (unsigned long long)dv + 1ull; }
__device__ __forceinline__ int div_small(int n, uint32_t magic) { return (int)(__umul24((uint32_t)n, magic) >> 20); }

// Workgroup -> (pair, tile row, first block column).  Grid = (8 * wg_per_row, tile_rows, ceil(pairs / 8)):
// workgroups go to the 8 XCDs round robin in x-fastest order, so the low 3 bits of blockIdx.x pick
// the pair inside a group of 8 and all tiles of one pair land on one XCD (its L2 holds the pair).
__device__ __forceinline__ bool locate(const SeaGeo& d, SeaArgs c, int* pair, int* trow, int* bcol0)
{
    *pair = (int)blockIdx.z * 8 + (int)(blockIdx.x & 7);
    *trow = (int)blockIdx.y;
    *bcol0 = (int)(blockIdx.x >> 3) * d.tc;
    return *pair < c->pairs;
}

inline bool grid_for(const SeaDev& d, dim3* grid)
{
    const long long gz = ((long long)d.pairs + 7) / 8;
    if (gz > 65535 || d.tile_rows > 65535) return false;
    *grid = dim3((unsigned)(8 * d.wg_per_row), (unsigned)d.tile_rows, (unsigned)gz);
    return true;
}

// Anchors sit 68 dwords apart, not 64: phase E lanes serving different blocks read the same anchor
// element of "their" block at once, and a 64-dword stride would put all of those in one LDS bank.
constexpr int ANCHOR_STRIDE = 68;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Layout {
    int win, anchor, best, count, a2, prev, own, s8, work, total;
#ifdef SEA_PHASE_STAMPS
    int stamps;                                            // [nb][ST_SLOTS] PhaseClock totals, behind everything else
#endif
};

__host__ __device__ constexpr Layout make_layout(int R, int nb, int win_rows, int pitch_dw, int xq, int s8_rows)
{
    Layout l{};
    l.win = 0;
    l.anchor = (win_rows * pitch_dw + 3) & ~3;         // 16-byte aligned: anchor rows are read as b128
    l.best = (l.anchor + nb * ANCHOR_STRIDE + 1) & ~1; // 8-byte aligned
    l.count = l.best + 2 * nb;                         // [0] list length, [1] next tile, [3] streak of hostile tiles (persistent_tiles),
                                                       // [4] patches phase C2 took off the list (scored or pruned), [5] patches C2 scored,
                                                       // [7] MSE: length of the second list (level 2 of the bound)
    l.a2 = l.count + 8;
    l.prev = l.a2 + nb;                                // [nb] scan index each wave's block of the previous tile ended with (third probe)
    l.own = l.prev + nb;                               // [nb][16] phase C2: the patches a crowded block's wave scores itself
    l.s8 = (l.own + 16 * nb + 1) & ~1;                 // 8-byte aligned, [s8_rows][xq] u16x4
    l.work = l.s8 + 2 * s8_rows * xq;                  // [nb*64*R] entries
    l.total = l.work + nb * 64 * R;
#ifdef SEA_PHASE_STAMPS
    l.stamps = l.total;
    l.total += nb * ST_SLOTS;
#endif
    return l;
}

__device__ __forceinline__ Layout layout_of(const SeaGeo& d, int R)
{
    return make_layout(R, d.nb, d.win_rows, d.pitch_dw, d.xq, d.s8_rows);
}

// The macroblock a wave owns inside its tile (waves are numbered row-major over the tile).
struct WaveBlock {
    int wr, wc;                   // position inside the tile
    int brow, bcol;               // block coordinates in the frame
    bool ok;                      // inside the frame's block grid (ragged last tile of a row / column)
};
__device__ __forceinline__ WaveBlock wave_block(const SeaGeo& d, SeaArgs c, int trow, int bcol0, int wave)
{
    WaveBlock b;
    b.wr = div_small(wave, d.magic_tc);
    b.wc = wave - b.wr * d.tc;
    b.brow = trow * d.tr + b.wr;
    b.bcol = bcol0 + b.wc;
    b.ok = b.bcol < c->nbc && b.brow < c->nbr;
    return b;
}

// A: stage the common search window of the workgroup's blocks (coalesced dword loads; rows and
// columns outside the frame -> 0).  Thread -> one dword column and every rstep-th row, loads in
// batches of four so that their latencies overlap.
__device__ __forceinline__ void stage_window(const SeaGeo& d, SeaArgs c, uint32_t* win, const uint8_t* cur, int bcol0, int r0)
{
    const int pitch = c->pitch, H = c->H;
    const int gx0 = bcol0 * 16 - d.sw, gy0 = r0 - d.sw;
    const int rstep = d.rstep;
    const int row0 = div_small((int)threadIdx.x, d.magic_pitch), dw = (int)threadIdx.x - row0 * d.pitch_dw;
    const int gx = gx0 + 4 * dw;
    const bool colok = gx >= 0 && gx < pitch;
    if (row0 < rstep) {
        const uint8_t* src = cur + (long long)(gy0 + row0) * pitch + gx;
        const long long sstep = (long long)rstep * pitch;
        uint32_t* dst = win + threadIdx.x;                     // == row0 * pitch_dw + dw
        const int dstep = rstep * d.pitch_dw;
        for (int row = row0; row < d.win_rows; row += 4 * rstep, src += 4 * sstep, dst += 4 * dstep) {
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int gy = gy0 + row + u * rstep;
                v[u] = 0;
                if (colok && row + u * rstep < d.win_rows && gy >= 0 && gy < H) v[u] = *(const uint32_t*)(src + u * sstep);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (row + u * rstep < d.win_rows) dst[u * dstep] = v[u];
        }
    }
}

// How the box-sum pass below (box_sums8_ch, "Lanes") deals its work to the waves, from shape_of's constants alone: compile-time
// in a geometry-fixed instance.  In one place, because holds_box_chunks() asks the same question for the tile driver.
struct BoxDeal {
    int SL;                       // lanes per segment: its quads, and a donor if the last one is read
    bool wide;                    // pieces: one per wave and pass
    uint32_t magic_sl;
    int SEG;                      // whole segments per wave
    int units;                    // pieces (unit = piece * 8 + chunk) or chunks
};
__device__ __forceinline__ BoxDeal box_deal(const SeaGeo& d, int need)
{
    BoxDeal b;
    const int XQ = d.xq;
    b.SL = XQ == need ? XQ + 1 : XQ;
    b.wide = b.SL > 64;
    b.magic_sl = XQ == need ? div_magic(b.SL) : d.magic_xq;
    b.SEG = b.wide ? 1 : div_small(64, b.magic_sl);
    b.units = b.wide ? 8 * div_small(XQ + 62, div_magic(63)) : 8;
    return b;
}

// A': 8x8 box sums of the staged window.  Lane (row chunk ch, column quad sq) walks CH+7 window rows.  Per row ONE
// QSAD against a zero reference gives the four sliding 4-byte sums h4(4sq .. 4sq+3) of the lane's own quad (packed
// u16), and its accumulator operand adds them up over the rows for nothing: C(r) = h4 of rows 0 .. r (at most 24 rows
// x 1020 < 2^16).  An output row takes V = C(y+7) - C(y-1) from a ring of 8 cumulative sums in registers -- the
// vertical 8-row sum of the lane's own 4-byte columns -- and adds the V of quad sq + 1, which the next lane has just
// formed, with a DPP wave_shl:1: S8(y, x) = V(x) + V(x + 4).  All of that is 32-bit subtracts and adds on the packed
// pairs (component-wise C grows and V <= 8160, so nothing borrows from or carries into the upper half).  Each add is one
// v_add_u32_dpp (wave_shl:1, bound_ctrl) executed by every lane: the sum is pinned in front of the store's predicate
// (an empty asm), because an add sunk under `if (stores)` leaves a v_mov_b32 0 and a v_mov_b32_dpp behind.  A lane
// without a source adds 0; its value is never stored or read.  s8[y][sq] = packed S8(y, 4sq .. 4sq+3).
// In a geometry-fixed instance (FIXED) both strides are constants: the window reads are ds_read2_b32 with instruction
// offsets from one base register per 254 / pitch + 1 rows (the second offset ends at 255 dwords), the table stores
// ds_write_b64 with byte offsets from a single one.  Run-time geometry keeps running offsets.
// Each lane used to compute both 4-byte halves of its 8-byte sums itself (two QSADs, 16 window bytes per row) and to
// slide the vertical sum by a packed subtract and add per row: half of the QSADs and window reads repeated the
// neighbour's, and the warm-up rows paid for sums nobody stored.
//
// Lanes: a row segment (the quads of one chunk) lies on consecutive lanes of one wave, 64 / SL segments per wave
// (XQ = 28: two chunks on lanes 0 .. 55, four waves hold the eight chunks).  The last lane of a segment has no
// neighbour -- what wave_shl hands it belongs to another chunk, or to nobody.  Where its quad is padding (XQ > need)
// that value is never read and the segment is the XQ quads themselves; where the bound phase reads it (XQ == need) the
// segment gets one more lane, a donor for quad XQ (window dwords XQ, XQ + 1 < pitch: what the second QSAD of quad
// XQ - 1 used to read) that stores nothing: SL = XQ + (XQ == need), from shape_of's constants.  A segment longer than
// a wave is cut into pieces 63 quads apart: lane 63 of a piece only donates, the next piece starts with its quad.
// Every lane of the wave runs the row loop (DPP reads disabled lanes as invalid), idle ones on window dword 0; only
// the store is predicated.  The trip count is wave-uniform.
// CH = s8_rows / 8 is a template parameter so that the ring indices and the warm-up are resolved
// at compile time (a run-time row count cost 5 % of the whole search in guards).
template <int CH, bool FIXED>
__device__ __forceinline__ void box_sums8_ch(const SeaGeo& d, const uint32_t* win, uint64_t* s8, int tid, int need)
{
    static_assert((CH + 7) * 1020 < 65536, "cumulative 4-byte sums must fit 16 bits");
    const int XQ = d.xq;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const BoxDeal deal = box_deal(d, need);
    const int SL = deal.SL, SEG = deal.SEG, units = deal.units;
    const bool wide = deal.wide;
    const uint32_t magic_sl = deal.magic_sl;
    const int ls = wide ? 0 : div_small(lane, magic_sl);           // the lane's segment inside its wave
    // FIXED: rows a ds_read2_b32 reaches from one base register (its second offset, in dwords, ends at 255)
    const int RB = FIXED ? 254 / d.pitch_dw + 1 : 1;
    for (int u = wave * SEG; u < units; u += d.nb * SEG) {
        // A wave that holds chunks is one the whole workgroup waits for at the barrier behind this pass (at the 2x4 tiles
        // of R = 3: waves 0 .. 3, the other four go straight there), and it shares its SIMD's vector issue, by priority
        // first and age second, with the waves of other workgroups whom nobody waits for: it runs the pass at priority 1.
        // `u`, SEG and `units` are scalars (the wave number is a v_readfirstlane_b32), so the loop is a scalar branch and
        // only such a wave executes the pair; the lower is the last instruction of every trip, in front of the barrier.
        __builtin_amdgcn_s_setprio(1);
        const int ch = wide ? (u & 7) : u + ls;
        const int sq = wide ? (u >> 3) * 63 + lane : lane - ls * SL;
        const bool active = wide ? sq < SL : (ls < SEG && ch < 8);
        const bool stores = active && sq < XQ && (!wide || lane < 63);
        // run-time geometry: running offsets (adds, no r * pitch multiplies), kept in registers by the empty asm.
        // FIXED: both strides are constants, so the reads go by instruction offsets from one base per RB rows and
        // the stores by instruction offsets from a single one.
        int pi = active ? (ch * CH) * d.pitch_dw + sq : 0, oi = (ch * CH) * XQ + sq;
        // FIXED: the window rows are read a batch of eight ahead of the rows being summed (all 16 of them at once where a
        // chunk has no more): every predicated store below is a basic block of its own, which the next read does not
        // cross, so rows read one by one behind the first store each wait out an LDS round trip.  Run-time geometry
        // reads row by row: its instances have no registers for rows in flight (the persistent ones would spill).
        constexpr int ROWS = CH + 7, STEP = FIXED ? 8 : 1, AHEAD = FIXED ? 16 : 1;
        uint64_t ring[8], acc = 0, w[ROWS];
        int read = 0;                                              // rows read so far (a constant once unrolled)
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (r % STEP == 0) {
#pragma unroll
                for (; read < ROWS && read < r + AHEAD; ++read) {
                    if constexpr (FIXED) {
                        if (read > 0 && read % RB == 0) {
                            pi += RB * d.pitch_dw;
                            asm volatile("" : "+v"(pi));           // a base register, not an offset too large for the encoding
                        }
                        w[read] = *(const u64_a4*)(win + pi + (read % RB) * d.pitch_dw);
                    } else {
                        w[read] = *(const u64_a4*)(win + pi);
                        pi += d.pitch_dw;
                        asm volatile("" : "+v"(pi));
                    }
                }
            }
            acc = __builtin_amdgcn_qsad_pk_u16_u8(w[r], 0u, acc);
            if (r >= 7) {
                uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
                if (r >= 8) { lo -= (uint32_t)ring[r & 7]; hi -= (uint32_t)(ring[r & 7] >> 32); }
                lo += SEA_DPP(lo, 0x130);                          // wave_shl:1 -- lane + 1's
                hi += SEA_DPP(hi, 0x130);
                // the sums are pinned here, for every lane: left to itself the compiler sinks the adds under the store's
                // predicate, where they no longer fuse with the DPP moves (one v_add_u32_dpp each)
                asm volatile("" : "+v"(lo), "+v"(hi));
                if constexpr (FIXED) {
                    if (stores) s8[oi + (r - 7) * XQ] = ((uint64_t)hi << 32) | lo;
                } else {
                    if (stores) s8[oi] = ((uint64_t)hi << 32) | lo;
                    oi += XQ;
                    asm volatile("" : "+v"(oi));
                }
            }
            ring[r & 7] = acc;
        }
        __builtin_amdgcn_s_setprio(0);
    }
}

// s8_rows = 16R + 8 + 16 (tr - 1) is a multiple of 8 for every tile height: 8 chunks of 2R + 2 tr - 1 rows
// (four chunks of twice the rows for two-row tiles were measured too -- 7 warm-up rows per chunk are 44 % of a 9-row
// chunk's work and 28 % of an 18-row one's, but half as many lanes share it; A/B in DESIGN.md)
// FIXED: the caller is a geometry-fixed instance (fix_geometry): d.pitch_dw and d.xq are compile-time constants there
template <int R>
__device__ __forceinline__ int box_quads_needed(const SeaGeo& d) { return 4 * R + 4 * (d.tc - 1) + 2; }     // quads per row the bound phase reads (shape_of); XQ >= need
template <int R, bool FIXED>
__device__ __forceinline__ void box_sums8(const SeaGeo& d, const uint32_t* win, uint64_t* s8, int tid)
{
    const int need = box_quads_needed<R>(d);
    if (d.tr == 1) box_sums8_ch<2 * R + 1, FIXED>(d, win, s8, tid, need);
    else if (d.tr == 2) box_sums8_ch<2 * R + 3, FIXED>(d, win, s8, tid, need);
    else box_sums8_ch<2 * R + 7, FIXED>(d, win, s8, tid, need);
}

// Whether a wave holds chunks of the pass: box_sums8_ch's unit loop has a trip for it.  Wave-uniform, from shape_of's
// constants and the wave number alone.  Such a wave is one the workgroup waits for at the barrier behind the pass; the
// others go straight there (persistent_tiles orders the next tile's prefetch by it).
template <int R>
__device__ __forceinline__ bool holds_box_chunks(const SeaGeo& d, int wave)
{
    const BoxDeal deal = box_deal(d, box_quads_needed<R>(d));
    return wave * deal.SEG < deal.units;
}

// quadrant sums of the anchor held one dword per lane (lane = row * 4 + dword): the quad swap pairs
// the two dwords of a half row, row_ror 4 and 8 add the four rows inside a 16-lane DPP row, the two
// DPP rows of each half are added on the scalar side.
__device__ __forceinline__ void anchor_quadrants(uint32_t mine, uint32_t* a01, uint32_t* a23)
{
    uint32_t s = __builtin_amdgcn_sad_u8(mine, 0u, 0u);
    s += SEA_DPP(s, 0xB1);                                 // quad_perm [1,0,3,2]
    s += SEA_DPP(s, 0x124);                                // row_ror 4
    s += SEA_DPP(s, 0x128);                                // row_ror 8
    const uint32_t q0 = (uint32_t)__builtin_amdgcn_readlane((int)s, 0) + (uint32_t)__builtin_amdgcn_readlane((int)s, 16);
    const uint32_t q1 = (uint32_t)__builtin_amdgcn_readlane((int)s, 2) + (uint32_t)__builtin_amdgcn_readlane((int)s, 18);
    const uint32_t q2 = (uint32_t)__builtin_amdgcn_readlane((int)s, 32) + (uint32_t)__builtin_amdgcn_readlane((int)s, 48);
    const uint32_t q3 = (uint32_t)__builtin_amdgcn_readlane((int)s, 34) + (uint32_t)__builtin_amdgcn_readlane((int)s, 50);
    *a01 = q0 | (q1 << 16);
    *a23 = q2 | (q3 << 16);
}

// LDS pitches from bank models of the reads that dominate (MI355X_MICROARCH.md, LDS: a wave's 8-byte reads are
// served 32 lanes at a time over 64 four-byte banks, 4-byte reads over 32; lanes conflict only on different
// addresses of one bank).
//
// Box-sum table pitch XQ (8-byte quads per row): phase B's lane (prow, q) reads quads (prow * R + i) * XQ + q * R + k,
// so the 32 lanes of a half wave sit prow * R * XQ + q * R quads apart.  An odd pitch (the first choice) left a
// two-way conflict on every one of those reads at R = 3 and a three-way one at R = 5; the pitch is now the
// smallest one >= need with the fewest conflicts (28 and 44 quads: none).
constexpr int box_conflicts(int xq, int R)
{
    int worst = 0, hits[64] = {};
    for (int b = 0; b < 64; ++b) hits[b] = 0;
    for (int prow = 0; prow < 8; ++prow)
        for (int q = 0; q < 4; ++q) {
            const int dw = 2 * ((prow * R) * xq + q * R);
            ++hits[dw & 63]; ++hits[(dw + 1) & 63];             // distinct lanes read distinct quads here
        }
    for (int b = 0; b < 64; ++b) worst = hits[b] > worst ? hits[b] : worst;
    return worst;
}
constexpr int pick_xq(int need, int R)
{
    int best = need, best_c = 1 << 30;
    for (int x = need; x < need + 12; ++x) {
        const int c = box_conflicts(x, R);
        if (c < best_c) { best_c = c; best = x; }
    }
    return best;
}

// Window pitch (dwords).  Phase E, four lanes per patch: the lanes of a quad read the same columns of window rows
// 4 apart, i.e. 4 * pitch dwords apart -- with pitch % 8 == 4 (the first choice, made for the brute-force kernel's
// access pattern, which this kernel does not have) lanes 0/2 and 1/3 of every quad hit the same bank.  Phase C's two
// probes (lane = 4 * row + dword, rows `pitch` apart) are rare and weigh little.
constexpr int pick_pitch(int need, int R)
{
    int best_p = need, best_c = 1 << 30;
    for (int p = need; p < need + 16; ++p) {
        int quad = 0, seen[32] = {};
        for (int i = 0; i < 32; ++i) seen[i] = 0;
        for (int sub = 0; sub < 4; ++sub) { quad += seen[(4 * sub * p) & 31]; ++seen[(4 * sub * p) & 31]; quad += seen[(4 * sub * p + 1) & 31]; }
        int probe = 0;
        for (int i = 0; i < 32; ++i) seen[i] = 0;
        for (int row = 0; row < 8; ++row)
            for (int dw = 0; dw < 4; ++dw) probe += seen[(row * p + dw) & 31]++;
        // a wider row also costs staging loads per thread (rows per sweep = threads / pitch) and LDS
        const int c = 64 * quad + probe + 2 * (p - need);
        if (c < best_c) { best_c = c; best_p = p; }
    }
    (void)R;
    return best_p;
}

// Host: tile shape (tr x tc macroblocks = waves per workgroup) and the LDS it needs.  A larger tile
// shares more of the staged window and of the box-sum pass between its blocks (window bytes per
// block: 1193 for 1 x 16, 864 for 2 x 8 at sw = 16), but LDS per workgroup grows.  The score is the
// number of waves a CU keeps resident (160 KiB LDS, 32 waves), discounted by the idle waves of
// ragged last tiles and by SIMD imbalance, with a bonus for the sharing.  Returns false if nothing fits.
// LDS geometry of a tile shape: depends on (R, tr, tc) only, so a kernel instantiated for one shape
// (fix_geometry below) gets every stride, row count and division constant at compile time.
struct Shape { int tr, tc, pitch, xq; size_t bytes; };
constexpr Shape shape_of(int R, int tr, int tc)
{
    Shape s{};
    s.tr = tr; s.tc = tc;
    s.xq = pick_xq(4 * R + 4 * (tc - 1) + 2, R);                    // S8 quads per row
    const int need_dw = (tc - 1) * 4 + 3 * R + (R - 1) + 5;         // base + k + 4 pairs of two dwords
    s.pitch = pick_pitch(need_dw > s.xq + 2 ? need_dw : s.xq + 2, R);
    s.bytes = (size_t)make_layout(R, tr * tc, 16 * R + 15 + 16 * (tr - 1), s.pitch, s.xq, 16 * R + 8 + 16 * (tr - 1)).total * 4;
    return s;
}

// Kernels instantiated for one tile shape (GEO = tr * 16 + tc, 0 = any shape at run time) overwrite the
// geometry part of their by-value launch descriptor (SeaGeo) with constants: the compiler then folds every use
// (strides become immediates, the multiply-shift divisions constants, ~15 SGPRs are never loaded).
// The host launches such an instance only when plan() chose exactly that shape (geometry_matches).
template <int R, int GEO>
__device__ __forceinline__ void fix_geometry(SeaGeo& d)
{
    if constexpr (GEO != 0) {
        constexpr int TR = GEO / 16, TC = GEO % 16;
        constexpr Shape s = shape_of(R, TR, TC);
        d.tr = TR; d.tc = TC; d.nb = TR * TC;
        d.magic_tc = div_magic(TC);
        d.win_rows = 16 * R + 15 + 16 * (TR - 1);
        d.s8_rows = 16 * R + 8 + 16 * (TR - 1);
        d.pitch_dw = s.pitch; d.xq = s.xq;
        d.rstep = 64 * TR * TC / s.pitch;
        d.magic_pitch = div_magic(s.pitch);
        d.magic_xq = div_magic(s.xq);
        d.sw = 8 * R - 8;                                  // the full window of the size class: NC = 16 R, also a constant now
    }
}

inline bool geometry_matches(const SeaDev& d, int R, int geo)
{
    if (geo == 0) return true;
    const Shape s = shape_of(R, geo / 16, geo % 16);
    return d.tr == geo / 16 && d.tc == geo % 16 && d.pitch_dw == s.pitch && d.xq == s.xq && d.sw == 8 * R - 8;
}

inline bool plan(int R, int nbr, int nbc, int sw, SeaDev* d, size_t* lds_bytes)
{
    auto shape = [&](int tr, int tc) { return shape_of(R, tr, tc); };
    Shape best = shape(1, 1);
    double best_score = -1.0;
    // resident waves per CU: 32 slots at <= 64 VGPRs (R <= 3); the R >= 4 kernels are held to 80 VGPRs -> 24
    const int wave_cap = R <= 3 ? 32 : 24;
    for (int pass = 0; pass < 2 && best_score < 0; ++pass)      // pass 0: SIMD-balanced wave counts only
        for (int tr = 1; tr <= 4; tr *= 2)
            for (int tc = 1; tc * tr <= 16; ++tc) {
                if (tc > nbc || (tr > 1 && tr > nbr) || (pass == 0 && (tr * tc) % 4 != 0)) continue;
                const Shape s = shape(tr, tc);
                if (s.bytes > 160 * 1024 || s.pitch >= 256 || s.xq >= 256) continue;
                const int nb = tr * tc;
                int wgs = (int)((160 * 1024) / (s.bytes + 1024));       // allocation granularity slack
                if (wgs * nb > wave_cap) wgs = wave_cap / nb;
                if (wgs < 1) wgs = 1;
                const int waves = wgs * nb;
                const double cover = ((double)nbc / (((nbc + tc - 1) / tc) * tc)) * ((double)nbr / (((nbr + tr - 1) / tr) * tr));
                // A workgroup's waves are dealt round robin to the CU's 4 SIMDs, so a wave count that is not a
                // multiple of 4 leaves one SIMD with an extra wave for the whole search (measured: 16 vs 15
                // waves +13 % at 720x480 sw 16; 8 vs 9 +17 %, 8 vs 12 (VGPR-limited to one workgroup) +30 %
                // at 1080p sw 32): such shapes are only used when nothing else fits.
                const double simd_eff = (double)nb / (4 * ((nb + 3) / 4));
                // staged window bytes per block, relative to a block's own (16 + 2 sw + 15)^2 window
                const double area = (double)(16 * tr + 2 * sw + 15) * (16 * tc + 2 * sw + 15) / nb;
                const double own = (double)(2 * sw + 31) * (2 * sw + 31);
                const double share = 1.0 + SHARE_WEIGHT * (1.0 - area / own);
                // a lone workgroup per CU has nobody to cover its barriers (measured 2-5 % at 1080p sw 32); four
                // 8-wave workgroups interleave better than two 16-wave ones (2 x 4 vs 2 x 8 tiles: +4.5 % at sw 16)
                const double together = wgs == 1 ? 0.93 : 1.0 + 0.03 * ((wgs > 4 ? 4 : wgs) - 2);
                // four-row tiles measured 3 % (720x480: 4 x 2 vs 2 x 4) to 15 % (1080p sw 32: 4 x 3 vs 2 x 6) slower
                // than two-row tiles of the same size: their windows are tall, staging rows are short
                const double tall = tr == 4 ? 0.95 : 1.0;
                const double score = waves * cover * simd_eff * share * together * tall + nb * 1e-3;
                if (score > best_score) { best_score = score; best = s; }
            }
    if (best_score < 0) return false;
    d->tr = best.tr; d->tc = best.tc; d->nb = best.tr * best.tc;
    d->magic_tc = div_magic(d->tc);
    d->wg_per_row = (nbc + d->tc - 1) / d->tc;
    d->tile_rows = (nbr + d->tr - 1) / d->tr;
    d->wg_per_pair = d->wg_per_row * d->tile_rows;
    d->win_rows = 16 * R + 15 + 16 * (d->tr - 1);
    d->s8_rows = 16 * R + 8 + 16 * (d->tr - 1);
    d->pitch_dw = best.pitch; d->xq = best.xq;
    *lds_bytes = best.bytes;
    d->rstep = 64 * d->nb / d->pitch_dw;
    d->magic_pitch = div_magic(d->pitch_dw);
    d->magic_xq = div_magic(d->xq);
    d->magic_wpp = div_magic40(d->wg_per_pair);
    d->magic_wpr = div_magic40(d->wg_per_row);
    return d->rstep >= 1;
}

constexpr int SEA_DEFAULT_QUOTA = 16, SEA_DEFAULT_BISECT = 5, SEA_DEFAULT_ENGAGE = 24;     // tools/ub_study.py; same-box A/B in DESIGN.md
constexpr int REDO_BURST = 15;
constexpr double REDO_DEFAULT_FRAC = 0.75;     // break-even measured on noise content

__device__ __forceinline__ void push_redo(SeaArgs c, int tile_in_xcd, int xcd)
{
    uint32_t* status = c->status;
    const uint32_t slot = atomicAdd(status + GME_STATUS_REDO, 1u);
    c->redo_list[slot] = ((uint32_t)tile_in_xcd << 3) | (uint32_t)xcd;
    atomicAdd(status + GME_STATUS_STATS + 16 * xcd + 1, 1u);
}

// Phase C2's choice of a crowded block's first patches (wave-uniform): keys below the returned limit are scored first.
// `below(lim)` counts the wave's patches whose key is below lim; lo / hi are the smallest bound and the UB (same unit,
// `shift` = position of the bound inside a key).  Invariant: at most `quota` keys lie below (lo + 1) << shift, or lo is
// the smallest bound itself (ties may exceed the quota: they all go first).
template <class Below>
__device__ __forceinline__ uint32_t first_round_limit(SeaArgs c, uint32_t lo, uint32_t hi, int shift, Below below)
{
    const int bisect = c->bisect, quota = c->quota;
    if (bisect < 0) return (lo + ((hi - lo) >> -bisect) + 1) << shift;      // no search: the lowest 1 / 2^n of the range
    for (int s = 0; s < bisect && lo < hi; ++s) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((int)below((mid + 1) << shift) > quota) hi = mid; else lo = mid;
    }
    return (lo + 1) << shift;
}

// tile number (inside its XCD's tiles) of the one-tile kernels' workgroup: what persistent_tiles calls `t`
__device__ __forceinline__ int tile_number(const SeaGeo& d, SeaArgs c, int pair, int trow, int bcol0)
{
    return (pair >> 3) * c->wg_per_pair + trow * c->wg_per_row + div_small(bcol0, d.magic_tc);
}

// Kern (MaeTile in bbme_sea.hip, MseTile in bbme_sea_mse.hip) supplies what the two drivers below call per tile:
//   Pre prep(lds, L, wave, lane, wave_ok, mine)             the wave's anchor dword -> LDS, per-wave anchor statistics
//   bool phases(d, lds, L, pair, trow, bcol0, mine, pre, tid, tile_id, clk, behind_box_sums)
//                                                           phases A' .. F; true: the tile went to redo_list.  It calls
//                                                           behind_box_sums() once, in every wave, right behind the barrier
//                                                           that follows phase A' (persistent_tiles: the late prefetch)
//   bool holds_chunks(d, wave)                              holds_box_chunks of the kernel's size class
//   int probe_word(L, wave)                                 LDS word of the wave's third probe: the vector its block of the
//                                                           previous tile ended with (one_tile seeds it with the zero
//                                                           vector; the persistent kernels seed the same word themselves)
// `d` is the geometry part alone; what else a phase needs it reads through launch_args().
// Count words (Layout::count) both drivers clear per tile and fold into the statistics (SeaDev::status, GME_STATUS_STATS):
// [0] list length, [4] / [5] what phase C2 took off the list / scored, [7] MSE: length of the second list.

// One-tile form of a search kernel: one workgroup per tile (grid_for, locate), the third probe seeded with the zero vector.
template <class Kern>
__device__ __forceinline__ void one_tile(const SeaGeo& d, uint32_t* lds, const Layout L)
{
    const SeaArgs c = launch_args();
    int pair, trow, bcol0;
    if (!locate(d, c, &pair, &trow, &bcol0)) return;       // whole workgroup
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // ---- A: window, anchor
    const long long plane = (long long)pair * c->plane_stride;
    stage_window(d, c, lds + L.win, c->cur + plane, bcol0, trow * d.tr * 16);
    uint32_t mine = 0;
    const WaveBlock wb = wave_block(d, c, trow, bcol0, wave);
    if (wb.ok) {
        const int pitch = c->pitch;
        const uint8_t* aptr = c->prev + plane + (long long)(wb.brow * 16) * pitch + wb.bcol * 16;
        mine = *(const uint32_t*)(aptr + (uint32_t)((lane >> 2) * pitch + (lane & 3) * 4));
    }
    const typename Kern::Pre pre = Kern::prep(lds, L, wave, lane, wb.ok, mine);
    if (lane == 0) lds[Kern::probe_word(L, wave)] = (uint32_t)(d.sw * (2 * d.sw + 16) + d.sw);      // no previous tile: the zero vector
    if (threadIdx.x == 0) { lds[L.count] = 0; lds[L.count + 4] = 0; lds[L.count + 5] = 0; lds[L.count + 7] = 0; }
    __syncthreads();
    PhaseClock clk;
#ifdef SEA_PHASE_STAMPS
    clk.start(lds + L.stamps, wave);                       // totals nobody reads: the one-tile form has no flush
#endif
    Kern::phases(d, lds, L, pair, trow, bcol0, mine, pre, (int)threadIdx.x, tile_number(d, c, pair, trow, bcol0), clk, [] {});      // no prefetch
    if (threadIdx.x == 0) {                                // the counts are final behind phase D's barrier
        uint32_t* stats = launch_args()->status + GME_STATUS_STATS + 16 * (blockIdx.x & 7);
        atomicAdd(stats, lds[L.count] + lds[L.count + 5]);
        atomicAdd(stats + 2, lds[L.count] + lds[L.count + 4]);
    }
}

// tiles of the pairs with pair % 8 == xcd: what a persistent workgroup of that XCD walks
__device__ __forceinline__ int tiles_of_xcd(SeaArgs c, int xcd) { return ((c->pairs - xcd + 7) >> 3) * c->wg_per_pair; }
// the XCD's tile counter (dynamic schedule), or null (static)
__device__ __forceinline__ uint32_t* tile_counter(SeaArgs c, int xcd) { return c->dynamic ? c->status + GME_STATUS_TILECTR + 16 * xcd : nullptr; }

// Persistent form of a search kernel: G workgroups (as many as fit on the chip at once) walk the
// tiles of "their" XCD's pairs.  The window and anchor of the next tile are fetched into registers
// while the current one is searched, so the HBM/L2 latency of phase A overlaps phases A' .. F
// instead of idling the workgroup's waves.
//
// Schedule: static (tile += G/8) or, with SeaDev::dynamic, dynamic: after its first tile a workgroup
// draws tile numbers G/8 + n from its XCD's counter.  Thread 0 asks one tile ahead, so the
// atomic's round trip is waited for together with the prefetched window (same vmcnt).  It is an
// atomicInc, not atomicAdd: LLVM would aggregate an add over the wave and wait for its result at once.
//
// Everything derived from the thread index is recomputed per tile from an opaque copy (the empty
// asm): hoisted out of the tile loop those values cost more registers than the 64 that eight
// waves per SIMD allow, and a spill reload (vmcnt) would wait for the prefetch it sits behind.
// The launch constants get the same treatment on the scalar side.  The loop carries the geometry (`d`: constants in
// a geometry-fixed instance), the LDS layout, the workgroup's number and the current tile; planes, frame size, the
// schedule's constants, counters and lists are read from the argument segment (launch_args()) by the block that uses
// them -- the prefetch, the tile's phases, the loop's head and tail -- and what follows from them alone (tiles of this
// XCD, G / 8, the counter's address, the plane's extent, the staging stride) is recomputed there by scalar
// instructions.  Carried, they were 44 to 95 spilled SGPRs per instance, read back from VGPR lanes on every tile.
// The loop tail's first half of persistent_tiles: the next tile's number and, if there is one, its prefetch and thread 0's
// draw.  A function with reference parameters, not a closure of the driver: called from two sites through a closure the
// instances at their register limit compiled to more spilled VGPRs, or a wave per SIMD less, than with the block in place.
template <class Fetch>
__device__ __forceinline__ void next_tile_of(const uint32_t* lds, const Layout& L, int xcd, int tid, int& tile, bool& more, bool& dynamic,
                                             uint32_t& drawn, Fetch& fetch)
{
    const SeaArgs c = launch_args();
    dynamic = c->dynamic != 0;
    tile = dynamic ? (int)lds[L.count + 1] : tile + (launch_groups_x(c) >> 3);
    more = tile < tiles_of_xcd(c, xcd);                    // workgroup-uniform
    if (more) {
        fetch(tile, tid);
        if (dynamic && tid == 0) drawn = atomicInc(c->status + GME_STATUS_TILECTR + 16 * xcd, 0xFFFFFFFFu);
    }
}

// LATE: whether the waves that hold box-sum chunks prefetch behind that pass's barrier (below); false keeps every wave's
// prefetch in front of the pass (`holds` is then false for every wave), for the instances where the second copy of the
// prefetch would cost spilled registers.
template <int NV, class Kern, bool LATE = true>
__device__ __forceinline__ void persistent_tiles(const SeaGeo& d, uint32_t* lds, const Layout L)
{
    const int xcd = blockIdx.x & 7;
    int tile = blockIdx.x >> 3;
    if (tile >= tiles_of_xcd(launch_args(), xcd)) return;
    // the thread index, made opaque again at every use: ONE register carries it through the loop (a copy per tile
    // beside threadIdx.x itself would be two), and nothing derived from it -- a lane mask such as `thread 0` is two
    // SGPRs -- is kept across the phases
    int tid_carried = (int)threadIdx.x;
    auto opaque_tid = [&]() {
        asm volatile("" : "+v"(tid_carried));
        return tid_carried;
    };

    uint32_t wv[NV], an_next = 0;
    int pair = 0, trow = 0, bcol0 = 0;
    auto fetch = [&](int t, int tid) {
        const SeaArgs c = launch_args();
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int row0 = div_small(tid, d.magic_pitch), dw = tid - row0 * d.pitch_dw;
        const int lp = (int)(((unsigned long long)(unsigned)t * c->magic_wpp) >> 40);
        const int wg = t - lp * c->wg_per_pair;
        const int wpr = c->wg_per_row;
        trow = (int)(((unsigned long long)(unsigned)wg * c->magic_wpr) >> 40);
        bcol0 = (wg - trow * wpr) * d.tc;
        pair = lp * 8 + xcd;
        // Window rows through a buffer resource over the pair's `cur` plane (H * pitch bytes): rows above or below
        // the frame give offsets outside it and the hardware range check returns 0 -- what the search wants there
        // (bbme.py:157-162 skips such candidates; they never form keys) -- so no per-row guard or branch is left.
        // Columns outside the plane and threads beyond the staging sweep get an offset that is out of range by itself,
        // 2^31, and stays so with the row steps added (u * sstep is far below 2^31; the offset is compared unsigned): no
        // select per row.  The row step stays in the vector offset -- the range check does not cover the instruction's
        // scalar offset.
        const int pitch = c->pitch;
        const long long plane = (long long)pair * c->plane_stride;
        const uint8_t* cur = c->cur + plane;
        const unsigned long long cur_bits = (unsigned long long)cur;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(cur_bits >> 32)) << 32) |
                    (unsigned)__builtin_amdgcn_readfirstlane((int)cur_bits)),
            (short)0, __builtin_amdgcn_readfirstlane(c->H * pitch), 0x00020000);
        const int gx0 = bcol0 * 16 - d.sw + 4 * dw, gy0 = trow * d.tr * 16 - d.sw + row0;
        const bool colok = row0 < d.rstep && gx0 >= 0 && gx0 < pitch;
        int outside = (int)0x80000000;                      // formed here, per prefetch: hoisted, the constant holds a VGPR across the phases
        asm volatile("" : "+v"(outside));
        const int off0 = colok ? gy0 * pitch + gx0 : outside;
        const int sstep = d.rstep * pitch;
#pragma unroll
        for (int u = 0; u < NV; ++u)
            wv[u] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, off0 + u * sstep, 0, 0);
        an_next = 0;
        const WaveBlock wb = wave_block(d, c, trow, bcol0, wave);
        if (wb.ok) {
            // the block's corner is wave-uniform; the lane's dword lies 15 rows and 12 bytes behind it at most: a 32-bit
            // offset on a scalar base, no 64-bit multiply-add per lane
            const uint8_t* aptr = c->prev + plane + (long long)(wb.brow * 16) * pitch + wb.bcol * 16;
            an_next = *(const uint32_t*)(aptr + (uint32_t)((lane >> 2) * pitch + (lane & 3) * 4));
        }
    };
    fetch(tile, opaque_tid());
    uint32_t drawn = 0;
    if (opaque_tid() == 0) {
        if (uint32_t* ctr = tile_counter(launch_args(), xcd)) drawn = atomicInc(ctr, 0xFFFFFFFFu);
        lds[L.count] = 0; lds[L.count + 3] = 0; lds[L.count + 4] = 0; lds[L.count + 5] = 0; lds[L.count + 7] = 0;
    }
    uint32_t stat_scored = 0, stat_listed = 0;             // thread 0's: patches scored exactly / left by the first upper bounds
    PhaseClock clk;
#ifdef SEA_PHASE_STAMPS
    {
        const int tid = opaque_tid();
        if (tid < d.nb * ST_SLOTS) lds[L.stamps + tid] = 0;
        __syncthreads();
        clk.start(lds + L.stamps, __builtin_amdgcn_readfirstlane(tid >> 6));
    }
#endif
    for (;;) {
        const int tid = opaque_tid();
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int gx = launch_groups_x(launch_args()) >> 3;             // G / 8, for thread 0 below: asked for here, ahead of the LDS stores
        {   // registers -> LDS
            const int row0 = div_small(tid, d.magic_pitch);
            if (row0 < d.rstep) {
                uint32_t* dst = lds + L.win + tid;
                const int dstep = d.rstep * d.pitch_dw;
#pragma unroll
                for (int u = 0; u < NV; ++u)
                    if (row0 + u * d.rstep < d.win_rows) dst[u * dstep] = wv[u];
            }
        }
        const int pair_c = pair, trow_c = trow, bcol0_c = bcol0, tile_c = tile;
        const uint32_t mine = an_next;
        const typename Kern::Pre pre = Kern::prep(lds, L, wave, lane, wave_block(d, launch_args(), trow_c, bcol0_c, wave).ok, mine);
        if (tid == 0) {
            // the finished tile's counts (final behind its phase D barrier) -> statistics, then cleared for this tile
            const uint32_t listed = lds[L.count], c2_off = lds[L.count + 4], c2_scored = lds[L.count + 5];
            stat_scored += listed + c2_scored;
            stat_listed += listed + c2_off;
            lds[L.count] = 0; lds[L.count + 4] = 0; lds[L.count + 5] = 0; lds[L.count + 7] = 0;
            lds[L.count + 1] = (uint32_t)gx + drawn;       // dynamic schedule: the next tile (static: not read)
        }
        clk.mark(ST_HEAD, lane);
        __syncthreads();
        clk.mark(ST_HEAD_WAIT, lane);
        // Loop tail, first half: the next tile, prefetched behind this one's phases.  Nothing up to phase D reads what it
        // fetches, but it is 1.5 to 2 thousand cycles of a wave's own time (a chain of scalar loads, two 64-bit
        // multiply-shift divisions, the buffer descriptor), and the whole workgroup waits at the barrier behind the box-sum
        // pass for the waves that hold its chunks (holds_box_chunks).  Those waves run the pass first and prefetch behind
        // its barrier, out of time they would otherwise spend waiting at phase D's; the others, with nothing to do until
        // that barrier, prefetch in front of it.  Every wave runs it exactly once per tile and reads the same words (thread 0
        // wrote count[1] in front of the head barrier and nobody writes it again before the next head), so `more`,
        // `dynamic` and the next `tile` stay workgroup-uniform.  Thread 0's draw goes with wave 0's prefetch, which holds
        // chunks: behind the barrier, still ahead of the hostile-streak code below that replaces `drawn`.
        bool more = false, dynamic = false;
        bool holds = false;                                // wave-uniform
        if constexpr (LATE) holds = Kern::holds_chunks(d, wave);
        if (!holds) {
            next_tile_of(lds, L, xcd, tid, tile, more, dynamic, drawn, fetch);
            clk.mark(ST_FETCH, lane);                      // charged where the wave runs it
        }
        auto behind_box_sums = [&]() __attribute__((always_inline)) {      // Kern::phases calls it behind the barrier that follows phase A'
            if constexpr (LATE) {
                if (holds) {
                    next_tile_of(lds, L, xcd, tid, tile, more, dynamic, drawn, fetch);
                    clk.mark(ST_FETCH, lane);
                }
            }
        };
        // A hostile tile is handed to the redo kernel.  When the tile this workgroup processed just before was
        // hostile too (a scene cut, a noisy shot: not an isolated occlusion), thread 0's wave also draws the next
        // tile numbers of this XCD -- consecutive tiles of the same pairs -- and lists them unseen: 3 of them, then
        // 7, then REDO_BURST while the streak lasts.  Where every tile is hostile only one in REDO_BURST + 1 pays
        // for the bound phases before brute force does the work anyway; friendly content never takes the branch.
        if (!Kern::phases(d, lds, L, pair_c, trow_c, bcol0_c, mine, pre, tid, tile_c, clk, behind_box_sums)) {
            if (tid == 0) lds[L.count + 3] = 0;            // streak of hostile tiles (thread 0's word)
        } else if (dynamic && wave == 0) {
            const int streak = (int)lds[L.count + 3];      // same address for the whole wave; only thread 0 writes it
            const int burst = streak == 0 ? 0 : streak == 1 ? 3 : streak == 2 ? 7 : REDO_BURST;
            if (burst) {
                // lane 0 lists the tile it had drawn already, lanes 1 .. burst draw one each (one wave-aggregated
                // atomic); the last of those becomes thread 0's new `drawn`, the others are listed
                const SeaArgs c = launch_args();
                uint32_t got = 0;
                if (lane >= 1 && lane <= burst) got = atomicAdd(c->status + GME_STATUS_TILECTR + 16 * xcd, 1u);
                const int t = (launch_groups_x(c) >> 3) + (int)(lane == 0 ? drawn : got);
                if (lane < burst && t < tiles_of_xcd(c, xcd)) push_redo(c, t, xcd);
                drawn = (uint32_t)__builtin_amdgcn_readlane((int)got, __builtin_amdgcn_readfirstlane(burst));   // burst is wave-uniform
            }
            if (lane == 0) lds[L.count + 3] = (uint32_t)(streak + 1);
        }
        clk.mark(ST_F_TAIL, lane);
        clk.add(ST_TILES, lane, 1u);
        if (!more) break;
        // No barrier here (round 4): every wave has passed phase D's barrier, and phase E's chunks end in one each, so
        // nobody still reads the window, the anchors, the box sums or the list when the next tile's staging overwrites them;
        // what is touched between here and the next tile's first barrier is per wave (best[], prev[]) or thread 0's
        // (the count words: a wave that has not read the list length yet can only be in a tile whose list is empty).
    }
#ifdef SEA_PHASE_STAMPS
    {   // the workgroup's totals -> stamp_totals
        asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory");            // PhaseClock::add's ds_add_u32: the compiler does not count it
        __syncthreads();
        const int tid = opaque_tid();
        if (tid < d.nb * ST_SLOTS) atomicAdd(stamp_totals + tid, (unsigned long long)lds[L.stamps + tid]);
    }
#endif
    // thread 0 has passed the barrier behind phase D: the last tile's counts are final
    if (opaque_tid() == 0) {
        uint32_t* stats = launch_args()->status + GME_STATUS_STATS + 16 * xcd;
        atomicAdd(stats, stat_scored + lds[L.count] + lds[L.count + 5]);
        atomicAdd(stats + 2, stat_listed + lds[L.count] + lds[L.count + 4]);
    }
}

// Host side of the persistent form: resident workgroups per XCD (what LDS and the 32 wave slots of
// a CU allow, on every CU) and whether the launch qualifies.  GME_SEA_PERSIST = 0 forces the
// one-tile-per-workgroup kernel, 1 / 2 force the persistent one (static / dynamic schedule);
// unset: persistent with the dynamic schedule once every resident workgroup gets several tiles.
struct PersistPlan { bool use; bool dynamic; long long g; int nv; };
inline PersistPlan plan_persistent(const SeaDev& d, size_t lds_bytes, int pairs, int cu_count)
{
    PersistPlan p;
    const long long tiles_x = (((long long)pairs + 7) / 8) * d.wg_per_pair;          // per XCD
    p.nv = (d.win_rows + d.rstep - 1) / d.rstep;
    const char* pmode = getenv("GME_SEA_PERSIST");
    const int pm = pmode ? atoi(pmode) : -1;
    int per_cu = (int)((160 * 1024) / (lds_bytes + 1024));
    if (per_cu * d.nb > 32) per_cu = 32 / d.nb;
    if (per_cu < 1) per_cu = 1;
    p.g = (long long)per_cu * cu_count / 8;
    const bool can = tiles_x < (1ll << 21) && d.wg_per_pair < (1 << 18) && p.nv <= 16 && p.g >= 1;
    p.use = can && (pm > 0 || (pm < 0 && tiles_x >= 4 * p.g));
    p.dynamic = pm != 1;
    if (p.g > tiles_x) p.g = tiles_x;
    return p;
}

// The persistent instance <R, NV> for staging rows per thread nv <= NV (NV = 6, 8, 12, 16), or the one-tile instance <R>.
template <class Norm, int R>
inline void launch_class(bool persistent, int nv, dim3 grid, dim3 block, size_t lds, hipStream_t s, const SeaDev& d)
{
    if (!persistent) Norm::template one_tile<R>(grid, block, lds, s, d);
    else if (nv <= 6) Norm::template persistent<R, 6>(grid, block, lds, s, d);
    else if (nv <= 8) Norm::template persistent<R, 8>(grid, block, lds, s, d);
    else if (nv <= 12) Norm::template persistent<R, 12>(grid, block, lds, s, d);
    else Norm::template persistent<R, 16>(grid, block, lds, s, d);
}

// Host launcher of both norms, for a job the caller's gate accepted.  Norm (MaeLaunch in bbme_sea.hip, MseLaunch in
// bbme_sea_mse.hip) supplies what differs between them:
//   int no_plan()                        what a window plan() cannot fit returns (*handled stays false)
//   void tables(SeaDev&, job)            the box-sum table of squares (MSE)
//   void ordered(SeaDev&)                phase C2's quota / bisect / engage (SeaDev::quota)
//   bool fits(R, nv)                     whether the persistent form holds the prefetched tile in registers
//   persistent<R, NV[, GEO]>, one_tile<R>(grid, block, lds, stream, d)      kernel launches
//   persistent_name, one_tile_name       the kernels' names in plan_note
template <class Norm>
int launch_sea(gme_ctx* ctx, const BbmeJob& job, bool* handled)
{
    *handled = false;
    const int NC = 2 * job.sw + 16, R = (NC + 15) / 16;
    const int nbr = job.H / 16, nbc = job.W / 16;
    if (nbr == 0 || nbc == 0) return GME_OK;
    SeaDev d;
    d.status = (uint32_t*)ctx->status; d.dynamic = 0;
    d.prev = job.prev; d.cur = job.cur; d.plane_stride = job.plane_stride;
    d.pairs = job.pairs; d.H = job.H; d.W = job.W; d.pitch = job.pitch; d.sw = job.sw;
    d.nbr = nbr; d.nbc = nbc; d.mf = job.mf;
    Norm::tables(d, job);
    size_t lds = 0;
    if (!plan(R, nbr, nbc, job.sw, &d, &lds)) return Norm::no_plan();
    const dim3 block(64 * d.nb);
    // hostile tiles (bound prunes little) -> brute-force redo kernel behind this one; GME_SEA_REDO=0 switches it off,
    // GME_SEA_REDO_FRAC sets the share of a tile's patches from which phase E costs more than evaluating everything
    d.redo_list = nullptr; d.redo_threshold = 0x7FFFFFFF;
    Norm::ordered(d);
    const bool redo = !(getenv("GME_SEA_REDO") && atoi(getenv("GME_SEA_REDO")) == 0);
    if (redo) {
        int rc = ctx_redo_list(ctx, (size_t)job.pairs * d.wg_per_pair, &d.redo_list);
        if (rc) return rc;
        const double frac = getenv("GME_SEA_REDO_FRAC") ? atof(getenv("GME_SEA_REDO_FRAC")) : REDO_DEFAULT_FRAC;
        d.redo_threshold = (int)(frac * d.nb * 64 * R);
        if (!job.status_fresh) GME_HIP_TRY(hipMemsetAsync(d.status + GME_STATUS_REDO, 0, 2 * sizeof(uint32_t), ctx->stream));
    }
    const PersistPlan pp = plan_persistent(d, lds, job.pairs, ctx->prop.multiProcessorCount);
    const int nv = pp.nv;
    const long long patches = (long long)job.pairs * nbr * nbc * 64 * R;
    const bool persistent = pp.use && Norm::fits(R, nv);
    dim3 grid;
    bool fix3 = false, fix5 = false;
    if (persistent) {
        grid = dim3((unsigned)(8 * pp.g));
        if (pp.dynamic) {
            d.dynamic = 1;
            if (!job.status_fresh) GME_HIP_TRY(hipMemsetAsync(d.status + GME_STATUS_TILECTR, 0, 8 * 16 * sizeof(uint32_t), ctx->stream));
        }
        // the two BASELINE shapes (720x480 sw 16: 2x4 tiles; 1080p sw 32: 2x6 tiles) have instances with the tile
        // geometry folded in at compile time
        fix3 = R == 3 && nv <= 5 && geometry_matches(d, 3, 2 * 16 + 4);
        fix5 = R == 5 && nv <= 7 && geometry_matches(d, 5, 2 * 16 + 6);
        plan_note(ctx, patches, "%s<%d,%d> tiles %dx%d persistent-%s%s grid %u lds %zu", Norm::persistent_name,
                  R, fix3 ? 5 : fix5 ? 7 : nv <= 6 ? 6 : nv <= 8 ? 8 : nv <= 12 ? 12 : 16, d.tr, d.tc, pp.dynamic ? "dynamic" : "static", (fix3 || fix5) ? " geometry-fixed" : "", grid.x, lds);
    } else {
        GME_REQUIRE(grid_for(d, &grid), GME_ERR_ARG, "too many workgroups in one launch");
        plan_note(ctx, patches, "%s<%d> tiles %dx%d one-tile grid %ux%ux%u lds %zu", Norm::one_tile_name, R, d.tr, d.tc,
                  grid.x, grid.y, grid.z, lds);
    }
    if (fix3) Norm::template persistent<3, 5, 2 * 16 + 4>(grid, block, lds, ctx->stream, d);
    else if (fix5) Norm::template persistent<5, 7, 2 * 16 + 6>(grid, block, lds, ctx->stream, d);
    else if (R == 1) launch_class<Norm, 1>(persistent, nv, grid, block, lds, ctx->stream, d);
    else if (R == 2) launch_class<Norm, 2>(persistent, nv, grid, block, lds, ctx->stream, d);
    else if (R == 3) launch_class<Norm, 3>(persistent, nv, grid, block, lds, ctx->stream, d);
    else if (R == 4) launch_class<Norm, 4>(persistent, nv, grid, block, lds, ctx->stream, d);
    else launch_class<Norm, 5>(persistent, nv, grid, block, lds, ctx->stream, d);
    GME_HIP_TRY(hipGetLastError());
    *handled = true;
    if (redo) return launch_exh_redo(ctx, job, R, d.tr, d.tc, d.wg_per_row, d.wg_per_pair, d.redo_list, d.status + GME_STATUS_REDO, d.status + GME_STATUS_REDO + 1);
    return GME_OK;
}

}  // namespace sea
