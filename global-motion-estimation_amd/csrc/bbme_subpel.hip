// Quarter-pel block matching (host definition: subpel.py).  The integer search leaves one vector per
// block; what runs here refines it to half and quarter pixels and compensates a frame with the refined field.  Everything is
// integer: the device equals subpel.refine / subpel.compensate bit for bit.
//
// Kernels:
//   k_subpel_refine     one lane group per block (a wave; a 16-lane DPP row where the block has at most 16 pixels, four blocks
//                       to a wave).  All 17 positions of a block lie within one pixel of the integer match, so the (bs + 2)^2
//                       window of `current` around it and the anchor are staged once in LDS; each lane then reads the 3 x 3
//                       neighbourhood of its pixels once per stage and scores the nine positions of the stage from registers.
//                       Nine DPP sums per stage, then the selection in the definition's own order.
//   k_compensate_qpel   one lane per four output pixels: the interpolated pixel of `previous` where its block's displaced
//                       origin is inside the frame, the copy elsewhere; squared error against `current` per pair
#include <type_traits>

#include "bbme_predict.h"
#include "gme_passes.h"

namespace {

constexpr int SUB_THREADS = 256;
constexpr int SUB_STAGED_MAX_BS = 64;                           // blocks up to this size go through LDS
// the staged instances sum a block's cost in 32 bits: bs^2 * 255^2 must stay below 2^31 (subpel.py: int64 at the ABI)
static_assert((long long)SUB_STAGED_MAX_BS * SUB_STAGED_MAX_BS * 65025ll < (1ll << 31), "32-bit block costs");

// sum over the lanes of a group, left in every lane of it: four DPP steps inside a 16-lane row, the wave-wide sum otherwise
template <int G>
__device__ __forceinline__ uint32_t group_sum(uint32_t v)
{
    if (G == 64) return wave_sum_u32(v);
    v += GME_DPP(v, 0xB1);
    v += GME_DPP(v, 0x4E);
    v += GME_DPP(v, 0x141);
    v += GME_DPP(v, 0x140);
    return v;
}
template <int G>
__device__ __forceinline__ unsigned long long group_sum(unsigned long long v)
{
    static_assert(G == 64, "64-bit sums are wave-wide");
    for (int m = 32; m > 0; m >>= 1) v += (unsigned long long)__shfl_xor((long long)v, m, 64);
    return v;
}

// one axis of the three positions centre - step, centre, centre + step of a stage (quarter units relative to the integer
// match, within [-3, 3]): first tap relative to the pixel (-1 or 0), weight of the second tap, and whether a block of bs
// pixels that starts at `start` + tap lies inside [0, n)
struct Axis {
    int tap[3], frac[3];
    bool in[3];
};
__device__ __forceinline__ Axis axis_of(int centre, int step, int start, int bs, int n)
{
    Axis a;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int q = centre + (k - 1) * step;
        a.tap[k] = q >> 2;
        a.frac[k] = q & 3;
        const int p0 = start + a.tap[k];
        a.in[k] = p0 >= 0 && p0 + bs - 1 + (a.frac[k] != 0) <= n - 1;
    }
    return a;
}

// The nine costs of a stage for the pixels of one lane.  `fetch(r, c)` is the pixel of `current` at row r, column c of the
// window whose origin is one pixel up and left of the integer match; `anchor(a, b)` the anchor pixel.  Horizontal blends first
// ((4 - fx) left + fx right, no rounding), then the vertical blend with the definition's single rounding: the same integer as
// the four-tap formula.  acc[3 * kx + ky]: column position outer, as the definition orders its candidates.
template <int G, int BS, typename Acc, typename Fetch, typename Anchor>
__device__ __forceinline__ void stage_costs(int bs_rt, int lane, const Axis& ax, const Axis& ay, int pnorm, bool with_centre,
                                            Fetch fetch, Anchor anchor, Acc (&acc)[9])
{
    const int bs = BS ? BS : bs_rt;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0;
    for (int p = lane; p < bs * bs; p += G) {
        const int a = p / bs, b = p - a * bs;
        int n[3][3];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) n[dy][dx] = fetch(a + dy, b + dx);
        const int ref = anchor(a, b);
        int hv[3][3];                                            // [row][x position]
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const bool left = ax.tap[kx] < 0;
            const int fx = ax.frac[kx];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int l = left ? n[dy][0] : n[dy][1], r = left ? n[dy][1] : n[dy][2];
                hv[dy][kx] = (4 - fx) * l + fx * r;
            }
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                if (kx == 1 && ky == 1 && !with_centre) continue;
                const bool up = ay.tap[ky] < 0;
                const int fy = ay.frac[ky];
                const int t = up ? hv[0][kx] : hv[1][kx], u = up ? hv[1][kx] : hv[2][kx];
                const int d = (((4 - fy) * t + fy * u + 8) >> 4) - ref;
                acc[3 * kx + ky] += (Acc)(pnorm ? d * d : abs(d));
            }
    }
}

// grid (ceil(blocks / groups per workgroup), pairs).  G lanes per block; BS the block size where it is a compile-time
// constant (0: bs_rt); STAGED: window and anchor through LDS and 32-bit costs (bs <= SUB_STAGED_MAX_BS), else every tap is
// read from global memory with its coordinates clamped into the frame (a clamped tap only ever enters the cost of a
// candidate that is not inside, which is dropped) and the costs are summed in 64 bits.
template <int G, int BS, bool STAGED>
__global__ void __launch_bounds__(SUB_THREADS) k_subpel_refine(const uint8_t* prev, const uint8_t* cur, long long plane_stride,
                                                               int H, int W, int pitch, int bs_rt, int hb, int wb, int pnorm,
                                                               int levels, const int32_t* mf, int32_t* qmf, long long* cost)
{
    typedef typename std::conditional<STAGED, uint32_t, unsigned long long>::type Acc;
    extern __shared__ __align__(16) uint8_t lds[];
    constexpr int GROUPS = SUB_THREADS / G;
    const int bs = BS ? BS : bs_rt;
    const int wp = bs + 2;                                       // window pitch
    const int group = threadIdx.x / G, lane = threadIdx.x % G;
    const int nb = hb * wb;
    const long long gid = (long long)blockIdx.x * GROUPS + group;
    const int pair = blockIdx.y;
    const bool have = gid < nb;
    const int bi = have ? (int)(gid / wb) : 0, bj = have ? (int)(gid - (long long)bi * wb) : 0;
    const int r0 = bi * bs, c0 = bj * bs;
    const long long slot = (long long)pair * nb + gid;
    int mvx = 0, mvy = 0;
    if (have) { mvx = mf[slot * 2]; mvy = mf[slot * 2 + 1]; }
    const long long sxl = (long long)c0 + mvx, syl = (long long)r0 + mvy;
    const bool start_inside = have && sxl >= 0 && syl >= 0 && sxl + bs <= W && syl + bs <= H;
    const int sx = start_inside ? (int)sxl : 0, sy = start_inside ? (int)syl : 0;
    const uint8_t* pp = prev + (long long)pair * plane_stride;
    const uint8_t* cp = cur + (long long)pair * plane_stride;
    const int group_bytes = (wp * wp + bs * bs + 3) & ~3;
    uint8_t* win = lds + (STAGED ? group * group_bytes : 0);
    uint8_t* anc = win + wp * wp;

    if (STAGED) {
        if (start_inside) {
            for (int i = lane; i < wp * wp; i += G) {
                const int r = i / wp, c = i - r * wp;
                const int y = sy - 1 + r, x = sx - 1 + c;
                win[i] = (y >= 0 && y < H && x >= 0 && x < W) ? cp[(long long)y * pitch + x] : (uint8_t)0;
            }
            for (int i = lane; i < bs * bs; i += G) {
                const int r = i / bs, c = i - r * bs;
                anc[i] = pp[(long long)(r0 + r) * pitch + c0 + c];
            }
        }
        __syncthreads();
    }
    if (!have) return;
    if (!start_inside) {
        if (lane == 0) {
            qmf[slot * 2] = (int32_t)(4u * (uint32_t)mvx);
            qmf[slot * 2 + 1] = (int32_t)(4u * (uint32_t)mvy);
            cost[slot] = -1;
        }
        return;
    }

    auto fetch = [&](int r, int c) -> int {
        if (STAGED) return win[r * wp + c];
        const int y = min(max(sy - 1 + r, 0), H - 1), x = min(max(sx - 1 + c, 0), W - 1);
        return cp[(long long)y * pitch + x];
    };
    auto anchor = [&](int a, int b) -> int {
        if (STAGED) return anc[a * bs + b];
        return pp[(long long)(r0 + a) * pitch + c0 + b];
    };

    int bx = 0, by = 0;                                          // best position, quarter units relative to the integer match
    long long best = 0;
    Acc acc[9];
#pragma unroll 1
    for (int level = 0; level < 2; ++level) {
        if (level > 0 && level >= levels) break;
        const int step = 2 >> level, cx = bx, cy = by;
        const Axis ax = axis_of(cx, step, sx, bs, W), ay = axis_of(cy, step, sy, bs, H);
        stage_costs<G, BS, Acc>(bs_rt, lane, ax, ay, pnorm, level == 0, fetch, anchor, acc);
        long long sum[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) sum[k] = (k == 4 && level > 0) ? 0 : (long long)group_sum<G>(acc[k]);
        if (level == 0) best = sum[4];
        if (level < levels) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    if (kx == 1 && ky == 1) continue;
                    if (ax.in[kx] && ay.in[ky] && sum[3 * kx + ky] < best) {
                        best = sum[3 * kx + ky];
                        bx = cx + (kx - 1) * step;
                        by = cy + (ky - 1) * step;
                    }
                }
        }
    }
    if (lane == 0) {
        qmf[slot * 2] = (int32_t)(4u * (uint32_t)mvx + (uint32_t)bx);
        qmf[slot * 2 + 1] = (int32_t)(4u * (uint32_t)mvy + (uint32_t)by);
        cost[slot] = best;
    }
}

// The pixel of k_compensate_qpel.  Output pixel (u, v) of block (i, j) = (v / bs, u / bs), i < hb and j < wb: the block's origin
// moves to (4 j bs - q0, 4 i bs - q1) quarter units; where that block is inside, the pixel is the definition's four-tap blend at
// its place in it, else (and beyond the last whole block) the pixel of `previous`.
struct QpelPixel {
    const uint8_t* p;             // the pair's `previous` plane
    const int32_t* q;             // its field [hb][wb][2], quarter units
    int H, W, pitch, bs, hb, wb;
    __device__ __forceinline__ int operator()(int u, int v) const
    {
        const int i = v / bs, j = u / bs;
        int o = p[(long long)v * pitch + u];
        if (i < hb && j < wb) {
            const long long X = 4ll * j * bs - q[((long long)i * wb + j) * 2];
            const long long Y = 4ll * i * bs - q[((long long)i * wb + j) * 2 + 1];
            const long long x0 = X >> 2, y0 = Y >> 2;
            const int fx = (int)(X & 3), fy = (int)(Y & 3);
            if (x0 >= 0 && y0 >= 0 && x0 + bs - 1 + (fx != 0) <= W - 1 && y0 + bs - 1 + (fy != 0) <= H - 1) {
                const uint8_t* s = p + (y0 + (v - i * bs)) * pitch + x0 + (u - j * bs);
                // a tap of weight zero may lie past the last row or column: it is not read
                const int p00 = s[0], p01 = fx ? s[1] : 0, p10 = fy ? s[pitch] : 0, p11 = (fx && fy) ? s[pitch + 1] : 0;
                o = ((4 - fx) * (4 - fy) * p00 + fx * (4 - fy) * p01 + (4 - fx) * fy * p10 + fx * fy * p11 + 8) >> 4;
            }
        }
        return o;
    }
};

// the row frame of bbme_predict.h, one plane per pair
__global__ void __launch_bounds__(PRED_THREADS) k_compensate_qpel(const uint8_t* prev, const uint8_t* cur, long long plane_stride,
                                                                  int H, int W, int pitch, int bs, int hb, int wb,
                                                                  const int32_t* qmf, uint8_t* out, long long out_stride,
                                                                  int out_pitch, unsigned long long* sse)
{
    const int f = blockIdx.z;
    const QpelPixel px = { prev + (long long)f * plane_stride, qmf + (long long)f * hb * wb * 2, H, W, pitch, bs, hb, wb };
    predict_rows(px, cur + (long long)f * plane_stride, H, W, pitch, out + (long long)f * out_stride, out_pitch, sse + f);
}

template <int G, int BS, bool STAGED>
void refine_launch(hipStream_t stream, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                   int pitch, int bs, int hb, int wb, int pnorm, int levels, const int32_t* mf, int32_t* qmf, long long* cost)
{
    constexpr int GROUPS = SUB_THREADS / G;
    const long long nb = (long long)hb * wb;
    const size_t lds = STAGED ? (size_t)GROUPS * (((bs + 2) * (bs + 2) + bs * bs + 3) & ~3) : 0;
    hipLaunchKernelGGL((k_subpel_refine<G, BS, STAGED>), dim3((unsigned)((nb + GROUPS - 1) / GROUPS), (unsigned)pairs),
                       dim3(SUB_THREADS), lds, stream, prev, cur, plane_stride, H, W, pitch, bs, hb, wb, pnorm, levels, mf, qmf,
                       cost);
}

}  // namespace

// ---- launchers --------------------------------------------------------------------------------------------------------
// qmf[pairs][hb][wb][2], cost[pairs][hb][wb] = subpel.refine of mf[pairs][hb][wb][2] for pair k = planes prev + k * stride,
// cur + k * stride (device); hb = H / bs, wb = W / bs
int launch_subpel_refine(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                         int pitch, int bs, int pnorm, int levels, const int32_t* mf, int32_t* qmf, long long* cost)
{
    const int hb = H / bs, wb = W / bs;
    if (pairs == 0 || hb == 0 || wb == 0) return GME_OK;
    GME_REQUIRE((long long)hb * wb <= 0x7FFFFFFFll, GME_ERR_ARG, "%d x %d blocks", hb, wb);
    const long long per = (long long)hb * wb;
    for_plane_chunks(pairs, [&](int k, int n) {
        const uint8_t* p = prev + (long long)k * plane_stride;
        const uint8_t* c = cur + (long long)k * plane_stride;
        const int32_t* m = mf + per * k * 2;
        int32_t* q = qmf + per * k * 2;
        long long* o = cost + per * k;
#define SUB_GO(G, BS, STAGED) refine_launch<G, BS, STAGED>(ctx->stream, p, c, plane_stride, n, H, W, pitch, bs, hb, wb, pnorm, levels, m, q, o)
        if (bs > SUB_STAGED_MAX_BS) SUB_GO(64, 0, false);
        else if (bs == 16) SUB_GO(64, 16, true);
        else if (bs == 12) SUB_GO(64, 12, true);
        else if (bs == 8) SUB_GO(64, 8, true);
        else if (bs == 4) SUB_GO(16, 4, true);
        else if (bs < 4) SUB_GO(16, 0, true);
        else SUB_GO(64, 0, true);
#undef SUB_GO
    });
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}

// out planes = subpel.compensate of the prev planes by qmf[pairs][hb][wb][2], sse[pairs] (device, zeroed here) = squared error
// of each against its cur plane
int launch_compensate_qpel(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                           int pitch, int bs, const int32_t* qmf, uint8_t* out, long long out_stride, int out_pitch,
                           unsigned long long* sse)
{
    if (pairs == 0) return GME_OK;
    const int hb = H / bs, wb = W / bs;
    return predict_planes(ctx, pairs, sse, [&](int k, int n) {
        hipLaunchKernelGGL(k_compensate_qpel, predict_grid(H, W, n), dim3(PRED_THREADS), 0, ctx->stream, prev + (long long)k * plane_stride,
                           cur + (long long)k * plane_stride, plane_stride, H, W, pitch, bs, hb, wb,
                           qmf + (long long)hb * wb * 2 * k, out + (long long)k * out_stride, out_stride, out_pitch, sse + k);
    });
}
