// Motion-compensated temporal denoising (host definition: denoise.py).  A target plane is averaged with up to
// four predictions of it (the overlapped predictions of bbme_obmc.hip from its neighbour frames); a prediction weighs
// max(0, 9 s - D) at a pixel, D the sum of absolute differences against the target over the pixel's 3 x 3 window with the border
// replicated, the target itself 9 s.  Everything is integer: the device equals denoise.blend byte for byte.
//
// Kernel:
//   k_denoise   the geometry of the row frame of bbme_predict.h (one wave per row, four pixels per lane, one 32-bit store per
//               lane) with a row body of its own.  A lane holds the columns u0 - 1 .. u0 + 4 of the rows v - 1, v, v + 1 as one
//               32-bit word and two neighbour bytes per row; row and column clamps happen at the load addresses and in one byte
//               permute that replicates the last column into a word's tail, never by a bounds branch.  A pixel's three bytes of a
//               row are one v_alignbyte of the six, masked to three bytes; the nine differences of a pixel and a reference are
//               three accumulating v_sad_u8.  The target's twelve groups are formed once and kept across the R references, whose
//               plane pointers stay scalar.  The squared difference against the comparison plane is summed per workgroup (16 bytes
//               of LDS) and added with one atomic.
#include "bbme_predict.h"
#include "gme_passes.h"

namespace {

constexpr int DN_MAX_REFS = 4, DN_MAX_STRENGTH = 64, DN_WINDOW = 9;
// tot <= 5 * 9 * 64 and the largest numerator 255 tot + tot / 2 below 2^20: the quotient is a 24-bit division
static_assert((DN_MAX_REFS + 1) * DN_WINDOW * DN_MAX_STRENGTH == 2880, "the largest total weight");
static_assert(255 * 2880 + 2880 / 2 < (1 << 20), "numerators below 2^20");

// The six columns u0 - 1 .. u0 + 4 of one row as the four 3-byte groups of the lane's pixels.  `plane` is the (scalar) plane, at
// its (clamped) row's 32-bit offset + u0, left and right are the offsets of the clamped neighbour columns, tail the permute that
// replicates column W - 1 into the bytes past it.
struct RowGroups {
    uint32_t g[PRED_PX];
    uint32_t word;                // columns u0 .. u0 + 3, the tail replicated
};

__device__ __forceinline__ RowGroups load_groups(const uint8_t* plane, uint32_t at, uint32_t left, uint32_t right, uint32_t tail)
{
    RowGroups r;
    const uint32_t w = __builtin_amdgcn_perm(0u, *(const uint32_t*)(plane + at), tail);
    const uint32_t lo = (w << 8) | plane[left];                    // columns u0 - 1 .. u0 + 2
    const uint32_t hi = (w >> 24) | ((uint32_t)plane[right] << 8); // columns u0 + 3, u0 + 4, then zero
    r.word = w;
    r.g[0] = lo & 0xFFFFFFu;
    r.g[1] = w & 0xFFFFFFu;
    r.g[2] = __builtin_amdgcn_alignbyte(hi, lo, 2u) & 0xFFFFFFu;
    r.g[3] = __builtin_amdgcn_alignbyte(hi, lo, 3u);             // its top byte is the zero of hi
    return r;
}

// grid (ceil(W / PRED_COLS), ceil(H / PRED_ROWS), targets): target f reads cur + f * cur_stride, its prediction r at
// preds + f * plane_stride + r * pred_stride and its comparison plane truth + f * truth_stride, all of row pitch `pitch`
__global__ void __launch_bounds__(PRED_THREADS) k_denoise(const uint8_t* cur, long long cur_stride, const uint8_t* preds, long long pred_stride,
                                                          long long plane_stride, int R, int H, int W, int pitch, int S,
                                                          const uint8_t* truth, long long truth_stride, uint8_t* out, long long out_stride,
                                                          int out_pitch, unsigned long long* sse)
{
    const int f = blockIdx.z;
    const int lane = threadIdx.x & 63;
    const int v = __builtin_amdgcn_readfirstlane(blockIdx.y * PRED_ROWS + (threadIdx.x >> 6));      // one wave per row: scalar
    const int u0 = blockIdx.x * PRED_COLS + lane * PRED_PX;
    uint32_t err = 0;
    if (v < H && u0 < W) {
        // the three rows of the window, clamped; the neighbour columns, clamped; the bytes of the word that lie in the row
        // (a plane is below 2^31 bytes: launch_denoise)
        const uint32_t row[3] = { (uint32_t)(max(v - 1, 0) * pitch), (uint32_t)(v * pitch), (uint32_t)(min(v + 1, H - 1) * pitch) };
        const uint32_t left = (uint32_t)max(u0 - 1, 0), right = (uint32_t)min(u0 + PRED_PX, W - 1);
        const int valid = min(W - u0, PRED_PX);                     // 1 .. 4
        const uint32_t tail = valid == 4 ? 0x03020100u : valid == 3 ? 0x02020100u : valid == 2 ? 0x01010100u : 0u;
        const uint8_t* c = cur + (long long)f * cur_stride;
        RowGroups cg[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) cg[a] = load_groups(c, row[a] + u0, row[a] + left, row[a] + right, tail);
        uint32_t tot[PRED_PX], n[PRED_PX];
#pragma unroll
        for (int k = 0; k < PRED_PX; ++k) {
            tot[k] = (uint32_t)S;
            n[k] = (uint32_t)S * ((cg[1].word >> (8 * k)) & 0xFFu);
        }
        const uint8_t* p = preds + (long long)f * plane_stride;
        for (int r = 0; r < R; ++r, p += pred_stride) {             // R is uniform: the plane pointer stays scalar
            uint32_t D[PRED_PX] = { 0u, 0u, 0u, 0u };
            uint32_t mid = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const RowGroups pg = load_groups(p, row[a] + u0, row[a] + left, row[a] + right, tail);
                if (a == 1) mid = pg.word;
#pragma unroll
                for (int k = 0; k < PRED_PX; ++k) D[k] = __builtin_amdgcn_sad_u8(pg.g[k], cg[a].g[k], D[k]);
            }
#pragma unroll
            for (int k = 0; k < PRED_PX; ++k) {
                const uint32_t w = (uint32_t)max(S - (int)D[k], 0);
                tot[k] += w;
                n[k] += w * ((mid >> (8 * k)) & 0xFFu);
            }
        }
        const uint32_t t = *(const uint32_t*)(truth + (long long)f * truth_stride + row[1] + u0);
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < PRED_PX; ++k) {
            // 24-bit operands: the division is the short one
            const uint32_t o = ((n[k] + (tot[k] >> 1)) & 0xFFFFFFu) / (tot[k] & 0xFFFu);
            if (k < valid) {                                        // the padding past W is written as zero
                const int d = (int)o - (int)((t >> (8 * k)) & 0xFFu);
                err += (uint32_t)(d * d);
                packed |= o << (8 * k);
            }
        }
        *(uint32_t*)(out + (long long)f * out_stride + (long long)v * out_pitch + u0) = packed;
    }
    // one atomic per workgroup, and none where nothing changed: every wave of a plane adds to the same word, and in a kernel trace
    // one atomic per wave took four fifths of the kernel's time.  A wave's sum is at most 256 * 255^2.
    __shared__ uint32_t part[PRED_ROWS];
    const uint32_t total = wave_sum_u32(err);
    if (lane == 0) part[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int a = 0; a < PRED_ROWS; ++a) sum += part[a];
        if (sum) atomicAdd(sse + f, (unsigned long long)sum);
    }
}

}  // namespace

// the argument rules of denoise.py (GME_ERR_ARG)
int denoise_check_args(const char* who, int R, int strength)
{
    GME_REQUIRE(R >= 1 && R <= DN_MAX_REFS, GME_ERR_ARG, "%s: %d references (1 .. %d)", who, R, DN_MAX_REFS);
    GME_REQUIRE(strength >= 1 && strength <= DN_MAX_STRENGTH, GME_ERR_ARG, "%s: strength %d (1 .. %d)", who, strength, DN_MAX_STRENGTH);
    return GME_OK;
}

// out planes = denoise.blend of the cur planes with their R prediction planes, sse[targets] (device, zeroed here) = squared
// difference of each output against its truth plane
int launch_denoise(gme_ctx* ctx, const uint8_t* cur, long long cur_stride, const uint8_t* preds, long long pred_stride, long long plane_stride,
                   int targets, int R, int H, int W, int pitch, int strength, const uint8_t* truth, long long truth_stride, uint8_t* out,
                   long long out_stride, int out_pitch, unsigned long long* sse)
{
    const int rc = denoise_check_args("temporal denoising", R, strength);
    if (rc) return rc;
    GME_REQUIRE(H > 0 && W > 0 && pitch >= W && pitch % 4 == 0 && out_pitch >= W && out_pitch % 4 == 0 && (long long)H * pitch < (1ll << 31),
                GME_ERR_ARG, "temporal denoising: a %d x %d plane of pitch %d into pitch %d", H, W, pitch, out_pitch);
    ctx->plan[0] = 0; ctx->plan_patches = 0;
    plan_note(ctx, 0, "k_denoise R %d strength %d, %d x %d, one wave per row", R, strength, H, W);
    if (targets == 0) return GME_OK;
    return predict_planes(ctx, targets, sse, [&](int k, int n) {
        hipLaunchKernelGGL(k_denoise, predict_grid(H, W, n), dim3(PRED_THREADS), 0, ctx->stream, cur + (long long)k * cur_stride, cur_stride,
                           preds + (long long)k * plane_stride, pred_stride, plane_stride, R, H, W, pitch, DN_WINDOW * strength,
                           truth + (long long)k * truth_stride, truth_stride, out + (long long)k * out_stride, out_stride, out_pitch,
                           sse + k);
    });
}
