// Vector propagation search (host definition: propagate.py).  A block scores the vectors it inherits --
// its own, its eight neighbours', the previous pair's, the camera's and zero -- keeps the cheapest and refines it by one pixel
// per pass.  A round reads the field of the round before and writes a new one (Jacobi), so a launch is one round and the
// rounds ping-pong between two fields on the stream.  Everything is integer: the device equals propagate.search byte for byte.
//
// Kernel:
//   k_prop<BS>    one wave per block, four blocks to a 256-thread workgroup, no LDS and no barrier.  The BS x BS anchor block of
//                 `previous` stays in registers, its (row, dword) pairs spread over the lanes; a candidate block of `current` is
//                 read straight from the frame, four bytes per lane and step (rows of a displaced block start at any byte: the
//                 loads are unaligned), and scored with v_sad_u8 or three v_dot4 (aa + bb - 2ab), then summed over the wave.
//                 The up to twelve inherited vectors are fetched by twelve lanes at once; a vector that an earlier candidate
//                 already holds is not scored again (its first occurrence keeps its class, and an equal cost never replaces the
//                 best), which on a settled field leaves two or three block costs of the twelve.  A refinement pass skips the
//                 positions the pass before has scored (all of them cost at least the best).  <16> and <32> are compiled and
//                 issue the loads of all listed candidates, then of all positions of a pass, before they sum the first cost (a
//                 block of 16 is one dword per lane: scored one by one, a wave would wait for memory twenty times in a row);
//                 <0> takes the block size at run time (and rows that are no multiple of four bytes) and scores one by one.
#include "bbme_wave_lds.h"
#include "gme_passes.h"

namespace {

constexpr int PR_MIN_BS = 4, PR_MAX_BS = 64, PR_MAX_ROUNDS = 4, PR_MAX_STEPS = 4, PR_MAX_COMPONENT = 1 << 14;
constexpr int PR_MAX_DWORDS = row_dwords(PR_MAX_BS);
constexpr int PR_CANDS = 12;                                    // own, eight neighbours, temporal, camera, zero
constexpr int PR_MOVED = 8;
static_assert((long long)PR_MAX_BS * PR_MAX_BS * 65025ll < (1ll << 31), "31-bit costs");
static_assert(small_div_covers(PR_MAX_BS, PR_MAX_DWORDS, 3), "range of small_div");

struct PropArgs {
    const uint8_t* prev;          // first "previous" plane; pair k reads the planes k * stride bytes on
    const uint8_t* cur;           // first "current" plane
    long long stride;
    int H, W, pitch;
    const int32_t* fin;           // [pairs][hb][wb][2]: the field of the round before
    const int32_t* t;             // fields of [hb][wb][2], or null: pair k reads field k + t_shift where that is not negative
    const int32_t* g;             // [pairs][hb][wb][2], or null
    int32_t* fout;                // [pairs][hb][wb][2]
    long long* cost;              // [pairs][hb][wb]
    uint8_t* source;              // [pairs][hb][wb]
    int t_shift;
    int hb, wb, bs, pnorm, steps;
};

// the dwords of a block a lane holds: BS * (BS / 4) over 64 lanes, or the most a block of 64 needs
template <int BS>
constexpr int lane_dwords() { return BS ? (BS * row_dwords(BS) + 63) / 64 : PR_MAX_BS * PR_MAX_DWORDS / 64; }

// What a lane knows of its share of the block: the anchor's dwords, where each lies in a block (byte offset from the block's
// first pixel) and which of its bytes belong to the block.  A dword is always read whole: its bytes past the block's last
// column are masked away, and where they lie past the row's pitch they are the first bytes of the next row, or of the guard row
// every plane stack has behind it (gme_internal.h: plane_shape).  A slot past the block's last dword reads the first one under
// an empty mask.  So the loads need no branch.
template <int BS>
struct Anchor {
    static constexpr int N = lane_dwords<BS>();
    uint32_t a[N], mask[N];
    int off[N];
    int total;

    // the B x B block at `base`, which lies inside the frame
    __device__ __forceinline__ void load(const uint8_t* base, int pitch, int B, int lane)
    {
        const int nd = row_dwords(B);
        total = B * nd;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int t = lane + 64 * i;
            const int y = small_div(t < total ? t : 0, nd), x = 4 * ((t < total ? t : 0) - y * nd);
            off[i] = y * pitch + x;
            mask[i] = t >= total ? 0u : B - x >= 4 ? 0xFFFFFFFFu : (1u << (8 * (B - x))) - 1u;
        }
#pragma unroll
        for (int i = 0; i < N; ++i) a[i] = dword(base, i);
    }

    // dword i of this lane of the block whose first pixel is at `base`
    __device__ __forceinline__ uint32_t dword(const uint8_t* base, int i) const
    {
        uint32_t v;
        __builtin_memcpy(&v, base + off[i], 4);
        return v & mask[i];
    }

    // the cost of the block at `base` against the anchor, in every lane
    __device__ __forceinline__ uint32_t score(const uint8_t* base, int pnorm) const
    {
        RowScore s;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (!BS && 64 * i >= total) break;                   // wave-uniform
            s.add(a[i], dword(base, i), pnorm);
        }
        return wave_sum_u32(s.value(pnorm));
    }

    // the same in two halves, for the compiled sizes: the loads of several blocks are issued before the first cost is summed, so
    // that a wave waits for memory once per batch and not once per block
    // (the masks are applied when the cost is summed: nothing between the loads uses what they return)
    __device__ __forceinline__ void fetch(const uint8_t* base, uint32_t (&v)[N]) const
    {
#pragma unroll
        for (int i = 0; i < N; ++i) __builtin_memcpy(&v[i], base + off[i], 4);
    }
    __device__ __forceinline__ uint32_t score(const uint32_t (&v)[N], int pnorm) const
    {
        RowScore s;
#pragma unroll
        for (int i = 0; i < N; ++i) s.add(a[i], v[i] & mask[i], pnorm);
        return wave_sum_u32(s.value(pnorm));
    }
};

// propagate.available: the magnitude first
__device__ __forceinline__ bool available(int H, int W, int y0, int x0, int B, int vx, int vy)
{
    if (vx < -PR_MAX_COMPONENT || vx > PR_MAX_COMPONENT || vy < -PR_MAX_COMPONENT || vy > PR_MAX_COMPONENT) return false;
    return x0 + vx >= 0 && y0 + vy >= 0 && x0 + vx + B <= W && y0 + vy + B <= H;
}

template <int BS>
__global__ void __launch_bounds__(BLK_THREADS) k_prop(const PropArgs A)
{
    const WaveBlock w = wave_block(A.wb);
    if (w.none) return;
    const int lane = w.lane, bj = w.bj, bi = w.bi, pair = w.z;
    const int B = BS ? BS : A.bs, pnorm = A.pnorm;
    const int x0 = bj * B, y0 = bi * B;
    const long long per = (long long)A.hb * A.wb, blk = (long long)pair * per + (long long)bi * A.wb + bj;
    const uint8_t* cur = A.cur + (long long)pair * A.stride;

    Anchor<BS> anc;
    anc.load(A.prev + (long long)pair * A.stride + (long long)y0 * A.pitch + x0, A.pitch, B, lane);

    // lane c < 12 fetches candidate c: 0 own, 1 .. 8 the neighbours in the definition's order, 9 temporal, 10 camera, 11 zero
    int vx = 0, vy = 0;
    bool have = false;
    if (lane <= 8) {
        const int n = lane == 0 ? 4 : lane <= 4 ? lane - 1 : lane;      // position in the 3 x 3 neighbourhood, row-major
        const int di = small_div(n, 3) - 1, dj = n - small_div(n, 3) * 3 - 1;
        const int i = bi + di, j = bj + dj;
        if (i >= 0 && i < A.hb && j >= 0 && j < A.wb) {
            const long long q = (long long)pair * per + (long long)i * A.wb + j;
            vx = A.fin[q * 2]; vy = A.fin[q * 2 + 1];
            have = true;
        }
    } else if (lane == 9) {
        if (A.t != nullptr && pair + A.t_shift >= 0) {
            const long long q = (long long)(pair + A.t_shift) * per + (long long)bi * A.wb + bj;
            vx = A.t[q * 2]; vy = A.t[q * 2 + 1];
            have = true;
        }
    } else if (lane == 10) {
        if (A.g != nullptr) {
            vx = A.g[blk * 2]; vy = A.g[blk * 2 + 1];
            have = true;
        }
    } else if (lane == 11) have = true;
    have = have && available(A.H, A.W, y0, x0, B, vx, vy);
    const uint32_t avail = (uint32_t)__builtin_amdgcn_ballot_w64(have);
    // a vector an earlier available candidate holds is scored there
#pragma unroll
    for (int k = 0; k < PR_CANDS - 1; ++k) {
        const int kx = __builtin_amdgcn_readlane(vx, k), ky = __builtin_amdgcn_readlane(vy, k);
        if (lane > k && ((avail >> k) & 1u) && vx == kx && vy == ky) have = false;
    }
    uint32_t todo = (uint32_t)__builtin_amdgcn_ballot_w64(have) & ((1u << PR_CANDS) - 1u);

    // the zero vector is available to every block, so there is a first one
    int bx = 0, by = 0, src = 4;
    uint32_t best = NO_COST;                                     // costs lie below it: the first one is taken
    const uint8_t* at = cur + (long long)y0 * A.pitch + x0;      // the co-located block: a vector (x, y) adds y * pitch + x
    if constexpr (BS != 0) {
        uint32_t px[PR_CANDS][Anchor<BS>::N];
#pragma unroll
        for (int c = 0; c < PR_CANDS; ++c)
            if ((todo >> c) & 1u)
                anc.fetch(at + (long long)__builtin_amdgcn_readlane(vy, c) * A.pitch + __builtin_amdgcn_readlane(vx, c), px[c]);
#pragma unroll
        for (int c = 0; c < PR_CANDS; ++c) {
            if (!((todo >> c) & 1u)) continue;
            const uint32_t v = anc.score(px[c], pnorm);
            if (v < best) {
                best = v; bx = __builtin_amdgcn_readlane(vx, c); by = __builtin_amdgcn_readlane(vy, c);
                src = c == 0 ? 0 : c <= 8 ? 1 : c - 7;
            }
        }
    } else {
        while (todo) {
            const int c = __builtin_ctz(todo);
            todo &= todo - 1u;
            const int cx = __builtin_amdgcn_readlane(vx, c), cy = __builtin_amdgcn_readlane(vy, c);
            const uint32_t v = anc.score(at + (long long)cy * A.pitch + cx, pnorm);
            if (v < best) {
                best = v; bx = cx; by = cy;
                src = c == 0 ? 0 : c <= 8 ? 1 : c - 7;
            }
        }
    }

    // refinement: the eight positions around the pass's centre, column offset in the outer loop
    int lx = 0, ly = 0;                                          // the centre of the pass before
#pragma unroll 1
    for (int p = 0; p < A.steps; ++p) {
        const int cx = bx, cy = by;
        bool moved = false;
        // o = 3 (ox + 1) + oy + 1.  A position is left out where it is the centre or not available, and where the pass before has
        // scored it: it cannot lie below the best
        auto listed = [&](int o, int qx, int qy) {
            return o != 4 && available(A.H, A.W, y0, x0, B, qx, qy) &&
                   !(p > 0 && qx >= lx - 1 && qx <= lx + 1 && qy >= ly - 1 && qy <= ly + 1);
        };
        if constexpr (BS != 0) {
            uint32_t px[9][Anchor<BS>::N];
            uint32_t want = 0;
#pragma unroll
            for (int o = 0; o < 9; ++o) {
                const int qx = cx + o / 3 - 1, qy = cy + o % 3 - 1;
                if (listed(o, qx, qy)) {
                    want |= 1u << o;
                    anc.fetch(at + (long long)qy * A.pitch + qx, px[o]);
                }
            }
#pragma unroll
            for (int o = 0; o < 9; ++o) {
                if (!((want >> o) & 1u)) continue;
                const uint32_t v = anc.score(px[o], pnorm);
                if (v < best) { best = v; bx = cx + o / 3 - 1; by = cy + o % 3 - 1; moved = true; }
            }
        } else {
#pragma unroll 1
            for (int o = 0; o < 9; ++o) {
                const int qx = cx + small_div(o, 3) - 1, qy = cy + o - small_div(o, 3) * 3 - 1;
                if (!listed(o, qx, qy)) continue;
                const uint32_t v = anc.score(at + (long long)qy * A.pitch + qx, pnorm);
                if (v < best) { best = v; bx = qx; by = qy; moved = true; }
            }
        }
        if (!moved) break;
        src |= PR_MOVED;
        lx = cx; ly = cy;
    }
    if (lane == 0) {
        A.fout[blk * 2] = bx;
        A.fout[blk * 2 + 1] = by;
        A.cost[blk] = (long long)best;
        A.source[blk] = (uint8_t)src;
    }
}

}  // namespace

// the argument rules of propagate.py
int prop_check_args(const char* who, int bs, int pnorm, int rounds, int steps)
{
    GME_REQUIRE(bs >= PR_MIN_BS && bs <= PR_MAX_BS, GME_ERR_ARG, "%s: block_size %d (%d .. %d)", who, bs, PR_MIN_BS, PR_MAX_BS);
    if (int rc = require_pnorm(who, pnorm)) return rc;
    GME_REQUIRE(rounds >= 1 && rounds <= PR_MAX_ROUNDS, GME_ERR_ARG, "%s: rounds %d (1 .. %d)", who, rounds, PR_MAX_ROUNDS);
    GME_REQUIRE(steps >= 0 && steps <= PR_MAX_STEPS, GME_ERR_ARG, "%s: steps %d (0 .. %d)", who, steps, PR_MAX_STEPS);
    return GME_OK;
}

// propagate.search of `pairs` pairs: pair k reads the planes prev + k * plane_stride and cur + k * plane_stride, the prior field
// f[k] of [hb][wb][2] (hb = H / bs, wb = W / bs), the temporal field t[k + t_shift] where t is given and k + t_shift >= 0, and the
// camera field g[k] where g is given.  Round r writes work[(r - 1) & 1], each of [pairs][hb][wb][2]; f is only read, so t may
// lie in it.  *result is the field of the last round (one of work[]), cost [pairs][hb][wb] and source [pairs][hb][wb] are its
// (all device).  Nothing waits for the device between the rounds.
int launch_prop(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
                int pnorm, int rounds, int steps, const int32_t* f, const int32_t* t, int t_shift, const int32_t* g, int32_t* const work[2],
                long long* cost, uint8_t* source, int32_t** result)
{
    int rc = prop_check_args("vector propagation", bs, pnorm, rounds, steps);
    if (rc) return rc;
    const int hb = H / bs, wb = W / bs;
    const bool compiled = bs == 16 || bs == 32;
    *result = work[(rounds - 1) & 1];
    PropArgs a;
    a.stride = plane_stride; a.H = H; a.W = W; a.pitch = pitch;
    a.hb = hb; a.wb = wb; a.bs = bs; a.pnorm = pnorm; a.steps = steps;
    a.t = t;
    const long long per = (long long)hb * wb;
    auto note = [&] {
        if (compiled) plan_note(ctx, 0, "k_prop<%d> rounds %d steps %d, %d x %d blocks, one wave each", bs, rounds, steps, hb, wb);
        else plan_note(ctx, 0, "k_prop<0> bs %d rounds %d steps %d, %d x %d blocks, one wave each", bs, rounds, steps, hb, wb);
    };
    for (int r = 0; r < rounds; ++r) {                           // a launch frame per round, each with the same plan
        const int32_t* in = r == 0 ? f : work[(r - 1) & 1];
        int32_t* out = work[r & 1];
        rc = launch_wave_blocks(ctx, pairs, hb, wb, 0, a, note, [&](int k) {
            a.prev = prev + (long long)k * plane_stride; a.cur = cur + (long long)k * plane_stride;
            a.fin = in + per * k * 2; a.fout = out + per * k * 2;
            a.t_shift = k + t_shift;
            a.g = g ? g + per * k * 2 : nullptr;
            a.cost = cost + per * k; a.source = source + per * k;
            return !compiled ? k_prop<0> : bs == 16 ? k_prop<16> : k_prop<32>;
        });
        if (rc) return rc;
    }
    return GME_OK;
}
