// What the one-wave-per-block kernels share (bbme_hier.hip, bbme_vbs.hip, bbme_bipred.hip, bbme_gmc.hip, bbme_prop.hip, bbme_interp.hip;
// DESIGN.md section 7n): the workgroup of four waves with its prologue and its launch, a wave's own LDS slice, filled and read by
// that wave alone without a workgroup barrier, the geometry of a block and of a search window in it, the cost of a row, the
// candidate list of a square with its order, the selection of the winner and the split of a wave's lanes over candidates.
#pragma once
#include "gme_internal.h"

// ---- the workgroup: one wave per block, four blocks of a block row side by side ----

constexpr int BLK_THREADS = 256, BLK_WAVES = BLK_THREADS / 64;

// which block a wave works on: grid (ceil(wb / BLK_WAVES), hb, planes).  `none`: the block row ends before this wave's block;
// the whole wave returns then, nothing in these kernels synchronises across waves.  UNIFORM: the wave index goes through
// v_readfirstlane, so that what follows from the block's position is kept in scalar registers.  k_hier alone declines: with it
// the kernel needs 9 VGPRs fewer and takes 6 to 7 % longer (measured).
struct WaveBlock {
    int wave, lane, bj, bi, z;
    bool none;
};
template <bool UNIFORM = true>
__device__ __forceinline__ WaveBlock wave_block(int wb)
{
    const int wave = UNIFORM ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
    const int bj = (int)blockIdx.x * BLK_WAVES + wave;
    return { wave, (int)(threadIdx.x & 63), bj, (int)blockIdx.y, (int)blockIdx.z, bj >= wb };
}

// The launch frame of such a kernel over `count` planes (pairs, targets) of hb x wb blocks, `wave_lds` bytes of LDS to a wave.
// note() writes the launch plan; pick(k) points the caller's `a` at plane k, the first of a chunk of one launch, and returns
// the kernel instance to run: `a` is read here after every pick.  Which instances there are is the caller's business.
template <typename Args, typename Note, typename Pick>
int launch_wave_blocks(gme_ctx* ctx, int count, int hb, int wb, int wave_lds, Args& a, Note note, Pick pick)
{
    ctx->plan[0] = 0; ctx->plan_patches = 0;
    note();
    if (count == 0 || hb == 0 || wb == 0) return GME_OK;
    GME_REQUIRE(hb <= 65535, GME_ERR_ARG, "%d block rows", hb);
    for_plane_chunks(count, [&](int k, int n) {
        void (*kernel)(Args) = pick(k);
        hipLaunchKernelGGL(kernel, dim3((unsigned)((wb + BLK_WAVES - 1) / BLK_WAVES), (unsigned)hb, (unsigned)n), dim3(BLK_THREADS),
                           (size_t)BLK_WAVES * wave_lds, ctx->stream, a);
    });
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}

// the norm of every block cost: 0 for sum |a - v|, 1 for sum (a - v)^2
inline int require_pnorm(const char* who, int pnorm)
{
    GME_REQUIRE(pnorm == 0 || pnorm == 1, GME_ERR_ARG, "%s: pnorm_distance %d out of range (bbme.py:60)", who, pnorm);
    return GME_OK;
}

// LDS reads of one wave behind its own LDS writes: the hardware keeps a wave's LDS operations in order, this keeps the compiler
// from moving them across
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- geometry: a block row of b bytes, a window row of `side` bytes that blocks are read from at any byte offset ----

// dwords of a block row
__host__ __device__ constexpr int row_dwords(int b) { return (b + 3) >> 2; }
// dwords of a window row: one more than its bytes need, v_alignbyte reads the dword behind the last one it uses (window_dword)
__host__ __device__ constexpr int window_row_dwords(int side) { return row_dwords(side) + 1; }
// LDS bytes of a b x b block (an anchor nothing is read from at an offset) and of a side x side window, each rounded to 16: the
// launcher's sizes and the kernel's row pitches come from the same two functions above
__host__ __device__ constexpr int block_bytes(int b) { return (b * row_dwords(b) * 4 + 15) & ~15; }
__host__ __device__ constexpr int window_bytes(int side) { return (side * window_row_dwords(side) * 4 + 15) & ~15; }
// the bytes of a block row's last dword that belong to the block
__host__ __device__ constexpr uint32_t tail_mask(int b) { return (b & 3) ? (1u << (8 * (b & 3))) - 1u : 0xFFFFFFFFu; }
// dword k of a block row that starts `sh` bytes (0 .. 3) into row[0]
__device__ __forceinline__ uint32_t window_dword(const uint32_t* row, int k, uint32_t sh) { return __builtin_amdgcn_alignbyte(row[k + 1], row[k], sh); }

// t / d for 0 <= t < SMALL_DIV_T and 1 <= d <= SMALL_DIV_D: the candidate and staging indices of a block
constexpr int SMALL_DIV_T = 1700, SMALL_DIV_D = 21;
__host__ __device__ constexpr int small_div(int t, int d) { return (int)(((uint32_t)t * ((1u << 20) / (uint32_t)d + 1u)) >> 20); }
constexpr bool small_div_exact()
{
    for (int d = 1; d <= SMALL_DIV_D; ++d)
        for (int t = 0; t < SMALL_DIV_T; ++t)
            if (small_div(t, d) != t / d) return false;
    return true;
}
static_assert(small_div_exact(), "range of small_div");
// whether that range holds what a kernel divides: the staging index of the largest thing it stages, `rows` rows of `dwords`
// dwords, by `dwords`, and the index in its largest square of candidates, n to a side, by n
constexpr bool small_div_covers(int rows, int dwords, int n = 1)
{
    return rows * dwords <= SMALL_DIV_T && dwords <= SMALL_DIV_D && n * n <= SMALL_DIV_T && n <= SMALL_DIV_D;
}

// `rows` rows of `rd` dwords into LDS: byte (r, c), c < cols, is plane[(y0 + r) * pitch + x0 + c] where that pixel lies
// inside the H x W level.  Bytes at c >= cols are zero; a byte outside the level is zero or whatever the plane holds beside
// it: it only ever enters the cost of a candidate that is not inside, which is dropped.  A dword whose four bytes lie in
// columns [0, pitch) of a row of the level is read at once, the others byte by byte.
__device__ __forceinline__ void stage_bytes(uint32_t* dst, int rows, int rd, int cols, const uint8_t* plane, int pitch,
                                            int H, int W, int y0, int x0, int lane)
{
    for (int t = lane; t < rows * rd; t += 64) {
        const int r = small_div(t, rd), k = t - r * rd;
        const int y = y0 + r, x = x0 + 4 * k, left = cols - 4 * k;
        uint32_t v = 0;
        if (y >= 0 && y < H && left > 0) {
            const uint8_t* src = plane + (long long)y * pitch;
            if (x >= 0 && x + 4 <= pitch) __builtin_memcpy(&v, src + x, 4);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (x + e >= 0 && x + e < W) v |= (uint32_t)src[x + e] << (8 * e);
            }
            if (left < 4) v &= (1u << (8 * left)) - 1u;
        }
        dst[t] = v;
    }
}

// The clamping sibling of stage_bytes (k_interp): byte (r, c), c < cols, is plane[clamp(y0 + r, 0, H - 1) * pitch +
// clamp(x0 + c, 0, W - 1)], the border replicated, so every byte of the window is a pixel of the level and nothing read from it
// has to be dropped.  Bytes at c >= cols are zero.  A dword whose four bytes lie in columns [0, W) is read at once, the others
// byte by byte.
__device__ __forceinline__ void stage_bytes_clamped(uint32_t* dst, int rows, int rd, int cols, const uint8_t* plane, int pitch,
                                                    int H, int W, int y0, int x0, int lane)
{
    for (int t = lane; t < rows * rd; t += 64) {
        const int r = small_div(t, rd), k = t - r * rd;
        const int x = x0 + 4 * k, left = cols - 4 * k;
        uint32_t v = 0;
        if (left > 0) {
            const uint8_t* src = plane + (long long)min(max(y0 + r, 0), H - 1) * pitch;
            if (x >= 0 && x + 4 <= W) __builtin_memcpy(&v, src + x, 4);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v |= (uint32_t)src[min(max(x + e, 0), W - 1)] << (8 * e);
            }
            if (left < 4) v &= (1u << (8 * left)) - 1u;
        }
        dst[t] = v;
    }
}

// ---- the cost ----

// The cost of block rows four bytes at a time: v_sad_u8 for sum |a - v|, three v_dot4 for sum (a - v)^2 as aa + bb - 2 ab.
struct RowScore {
    uint32_t sad = 0, aa = 0, bb = 0, ab = 0;
    __device__ __forceinline__ void add(uint32_t a, uint32_t v, int pnorm)
    {
        if (pnorm == 0) sad = __builtin_amdgcn_sad_u8(a, v, sad);
        else {
            aa = __builtin_amdgcn_udot4(a, a, aa, false);
            bb = __builtin_amdgcn_udot4(v, v, bb, false);
            ab = __builtin_amdgcn_udot4(a, v, ab, false);
        }
    }
    // sum |a - v| or sum (a - v)^2 of what was added (the latter modulo 2^32 until the lanes' parts are summed)
    __device__ __forceinline__ uint32_t value(int pnorm) const { return pnorm == 0 ? sad : aa + bb - 2u * ab; }
};

constexpr uint32_t NO_COST = 0xFFFFFFFFu;                       // no cost: above every cost there is, and above every order

// ---- P lanes to a candidate, each a share of its rows: lane = slot * P + q, P a power of two ----

// the sum of the parts of the P lanes of a candidate, in each of them
__device__ __forceinline__ uint32_t lanes_sum(uint32_t part, int P)
{
    for (int m = 1; m < P; m <<= 1) part += (uint32_t)__shfl_xor((int)part, m, 64);
    return part;
}
struct LaneSplit {
    int P, shift, slots, slot, q;
    __device__ __forceinline__ LaneSplit(int P_, int lane) : P(P_), shift(__builtin_ctz(P_)), slots(64 >> shift), slot(lane >> shift), q(lane & (P_ - 1)) {}
    __device__ __forceinline__ uint32_t sum(uint32_t part) const { return lanes_sum(part, P); }
};
// as many lanes as leave every one of ncand candidates a slot in one round, at most 8 (k_interp writes this rule and its split
// out: see there)
__device__ __forceinline__ int lanes_for_one_round(int ncand)
{
    int P = 1;
    while (P < 8 && ncand * (P * 2) <= 64) P *= 2;
    return P;
}

// ---- the candidates of a square [-r, r]^2 and the choice among them ----

// Candidate c of n * n, n = 2r + 1, lies at column c / n and row c % n of the square (the column offset is the outer loop of
// the definitions).  Its order decides among equal costs, the least wins: 0 for the centre, c + 1 for the others.  A kernel
// whose centre is the incumbent (k_bipred) gives that order 0, does not list the centre and asks for the others' orders only.
struct Square {
    int r, n, ncand;
    __device__ __forceinline__ explicit Square(int r_) : r(r_), n(2 * r_ + 1), ncand(n * n) {}
    // candidate c's position: its offset + r (column, row)
    __device__ __forceinline__ void at(int c, int* col, int* row) const { *col = small_div(c, n); *row = c - *col * n; }
    __device__ __forceinline__ bool centre(int col, int row) const { return col == r && row == r; }
    __device__ __forceinline__ uint32_t order_beside_centre(int c) const { return (uint32_t)c + 1u; }
    __device__ __forceinline__ uint32_t order(int c, int col, int row) const { return centre(col, row) ? 0u : order_beside_centre(c); }
    // the offset (column, row) of the candidate with that order
    __device__ __forceinline__ void offset(uint32_t order, int* ox, int* oy) const
    {
        *ox = 0; *oy = 0;
        if (order != 0u) {
            at((int)order - 1, ox, oy);
            *ox -= r; *oy -= r;
        }
    }
};

// The least (cost, order): first a lane's own over the candidates it meets, then the wave's in two minima, the least cost and
// the least order among the lanes that hold it.
struct Least {
    uint32_t cost = NO_COST, order = NO_COST;
    __device__ __forceinline__ void take(uint32_t c, uint32_t o)
    {
        if (c < cost || (c == cost && o < order)) { cost = c; order = o; }
    }
};
__device__ __forceinline__ Least wave_least(uint32_t cost, uint32_t order)
{
    Least w;
    w.cost = wave_min_u32(cost);
    w.order = wave_min_u32(cost == w.cost ? order : NO_COST);
    return w;
}
