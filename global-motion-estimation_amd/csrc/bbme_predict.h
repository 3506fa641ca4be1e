// What the predict-a-plane passes share (bbme_subpel.hip, bbme_vbs.hip, bbme_bipred.hip, bbme_gmc.hip, bbme_interp.hip): the row
// frame of the four kernels that differ only in how one pixel is predicted, and the launch over the planes that all five
// launchers make.
#pragma once
#include "gme_internal.h"

// The row frame: grid (ceil(W / PRED_COLS), ceil(H / PRED_ROWS), planes)
constexpr int PRED_PX = 4;                                      // output pixels per lane: one 32-bit store
constexpr int PRED_ROWS = 4;                                    // rows per workgroup: one wave per row
constexpr int PRED_THREADS = 64 * PRED_ROWS;
constexpr int PRED_COLS = 64 * PRED_PX;
inline dim3 predict_grid(int H, int W, int planes) { return dim3((W + PRED_COLS - 1) / PRED_COLS, (H + PRED_ROWS - 1) / PRED_ROWS, planes); }

// One plane of the frame: px(u, v) is the predicted pixel at column u < W of row v < H.  Lanes store four pixels at once; pixels
// at or past W are written as zero, the plane's padding (pitch is a multiple of 64).  The squared error against `cur` is summed
// per wave and added to *sse with one atomic.
template <class Pixel>
__device__ __forceinline__ void predict_rows(const Pixel& px, const uint8_t* cur, int H, int W, int pitch, uint8_t* out, int out_pitch,
                                             unsigned long long* sse)
{
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.y * PRED_ROWS + (threadIdx.x >> 6);
    const int u0 = blockIdx.x * PRED_COLS + lane * PRED_PX;
    uint32_t err = 0;
    if (v < H && u0 < W) {
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < PRED_PX; ++k) {
            const int u = u0 + k;
            if (u >= W) break;
            const int o = px(u, v);
            const int d = o - (int)cur[(long long)v * pitch + u];
            err += (uint32_t)(d * d);
            packed |= (uint32_t)o << (8 * k);
        }
        *(uint32_t*)(out + (long long)v * out_pitch + u0) = packed;
    }
    const uint32_t total = wave_sum_u32(err);
    if (lane == 0 && total) atomicAdd(sse, (unsigned long long)total);
}

// A predict launch over `count` planes: sse[count] (device) zeroed on the context's stream, then launch(first, n) for every
// chunk of planes one grid carries
template <class Launch>
int predict_planes(gme_ctx* ctx, int count, unsigned long long* sse, Launch launch)
{
    GME_HIP_TRY(hipMemsetAsync(sse, 0, sizeof(unsigned long long) * count, ctx->stream));
    for_plane_chunks(count, launch);
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}
