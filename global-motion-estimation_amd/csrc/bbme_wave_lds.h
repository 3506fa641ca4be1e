// What the one-wave-per-block kernels share (bbme_hier.hip, bbme_vbs.hip, bbme_bipred.hip, bbme_gmc.hip, bbme_interp.hip): a wave's own LDS slice, filled and read by that wave
// alone, without a workgroup barrier.
#pragma once
#include "gme_internal.h"

// LDS reads of one wave behind its own LDS writes: the hardware keeps a wave's LDS operations in order, this keeps the compiler
// from moving them across
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// t / d for 0 <= t < 1700 and 1 <= d <= 21 (checked exhaustively on the host): the candidate and staging indices of a block
constexpr int SMALL_DIV_T = 1700, SMALL_DIV_D = 21;
__device__ __forceinline__ int small_div(int t, int d) { return (int)(((uint32_t)t * ((1u << 20) / (uint32_t)d + 1u)) >> 20); }

// `rows` rows of `row_dwords` dwords into LDS: byte (r, c), c < cols, is plane[(y0 + r) * pitch + x0 + c] where that pixel lies
// inside the H x W level.  Bytes at c >= cols are zero; a byte outside the level is zero or whatever the plane holds beside
// it: it only ever enters the cost of a candidate that is not inside, which is dropped.  A dword whose four bytes lie in
// columns [0, pitch) of a row of the level is read at once, the others byte by byte.
__device__ __forceinline__ void stage_bytes(uint32_t* dst, int rows, int row_dwords, int cols, const uint8_t* plane, int pitch,
                                            int H, int W, int y0, int x0, int lane)
{
    for (int t = lane; t < rows * row_dwords; t += 64) {
        const int r = small_div(t, row_dwords), k = t - r * row_dwords;
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
__device__ __forceinline__ void stage_bytes_clamped(uint32_t* dst, int rows, int row_dwords, int cols, const uint8_t* plane, int pitch,
                                                    int H, int W, int y0, int x0, int lane)
{
    for (int t = lane; t < rows * row_dwords; t += 64) {
        const int r = small_div(t, row_dwords), k = t - r * row_dwords;
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

// The cost of block rows four bytes at a time (k_bipred, k_gmc): v_sad_u8 for sum |a - v|, three v_dot4 for sum (a - v)^2 as
// aa + bb - 2 ab.
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
