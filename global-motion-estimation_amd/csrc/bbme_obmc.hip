// Overlapped block motion compensation (host definition: obmc.py).  Every other compensation of the library
// copies one displaced block per block, so the prediction jumps wherever two neighbours disagree.  Here a pixel is blended from
// the predictions of its own block and of the nearest vertical, horizontal and diagonal neighbour under a linear ramp.
// Everything is integer: the device equals obmc.compensate byte for byte.
//
// Kernel:
//   k_obmc   the row frame of bbme_predict.h: one wave per row, four pixels per lane.  The row is wave-uniform, and with it the
//            block row, the neighbour row, both row weights and the two field rows, which stay scalar.  A pixel whose four
//            vectors agree is the single sample; a wave in which every pixel is of that kind (the blocks of a pan) skips the
//            other three samples as a whole, and a mixed wave takes them for all lanes and selects.  Every read is clamped, field
//            indices and pixel coordinates alike: no vector can lead outside a plane.
#include "bbme_predict.h"
#include "gme_passes.h"

namespace {

constexpr int OB_MIN_BS = 4, OB_MAX_BS = 64;
// the largest numerator 255 * 4 B^2 + 2 B^2 in 32 bits, and the reciprocal ceil(2^37 / (4 B^2)) in 32 bits from B = 4 on
static_assert(255ll * 4 * OB_MAX_BS * OB_MAX_BS + 2 * OB_MAX_BS * OB_MAX_BS < (1ll << 22), "numerators below 2^22");
static_assert(((1ll << 37) + 4 * OB_MIN_BS * OB_MIN_BS - 1) / (4 * OB_MIN_BS * OB_MIN_BS) <= 0xFFFFFFFFll, "a 32-bit reciprocal");

// The pixel of k_obmc.  q is the pair's field [hb][wb][2] in units of unit / 4 pixels; recip = ceil(2^37 / (4 B^2)), with which
// (mulhi(n, recip)) >> 5 == n / (4 B^2) for every numerator n there is (obmc.py: reciprocal, checked exhaustively by the host
// tests).
struct ObmcPixel {
    const uint8_t* p;             // the pair's `previous` plane
    const int32_t* q;             // its field [hb][wb][2]
    int unit;                     // 4: whole pixels, 1: quarter pixels
    int H, W, pitch, bs, hb, wb;
    uint32_t recip;

    // the definition's P(4 u - qx, 4 v - qy): the four-tap blend with each tap's coordinates clamped into the plane
    __device__ __forceinline__ int sample(int qx, int qy, int u, int v) const
    {
        const long long X = 4ll * u - (long long)qx * unit, Y = 4ll * v - (long long)qy * unit;
        const int fx = (int)(X & 3), fy = (int)(Y & 3);
        // first taps within [-1, W] and [-1, H]: beyond them both taps of the axis clamp to the same border pixel anyway
        const int x0 = (int)min(max(X >> 2, -1ll), (long long)W), y0 = (int)min(max(Y >> 2, -1ll), (long long)H);
        const int xa = min(max(x0, 0), W - 1), xb = min(max(x0 + 1, 0), W - 1);
        const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
        const uint8_t* ra = p + (long long)ya * pitch;
        const uint8_t* rb = p + (long long)yb * pitch;
        return ((4 - fx) * (4 - fy) * ra[xa] + fx * (4 - fy) * ra[xb] + (4 - fx) * fy * rb[xa] + fx * fy * rb[xb] + 8) >> 4;
    }

    __device__ __forceinline__ int operator()(int u, int row) const
    {
        const int v = __builtin_amdgcn_readfirstlane(row);      // one wave per row: scalar from here on
        const int i = v / bs, j = u / bs;
        if (i >= hb || j >= wb) return p[(long long)v * pitch + u];
        const int ty = 2 * (v - i * bs) + 1 - bs, tx = 2 * (u - j * bs) + 1 - bs;
        const int i2 = min(max(i + (ty < 0 ? -1 : 1), 0), hb - 1), j2 = min(max(j + (tx < 0 ? -1 : 1), 0), wb - 1);
        const int wy1 = abs(ty), wy0 = 2 * bs - wy1, wx1 = abs(tx), wx0 = 2 * bs - wx1;
        const int32_t* r0 = q + (long long)i * wb * 2;           // the two field rows of this wave
        const int32_t* r1 = q + (long long)i2 * wb * 2;
        const int ax = r0[2 * j], ay = r0[2 * j + 1], bx = r0[2 * j2], by = r0[2 * j2 + 1];
        const int cx = r1[2 * j], cy = r1[2 * j + 1], dx = r1[2 * j2], dy = r1[2 * j2 + 1];
        const int own = sample(ax, ay, u, v);
        const bool same = ax == bx && ax == cx && ax == dx && ay == by && ay == cy && ay == dy;
        int o = own;
        if (__builtin_amdgcn_ballot_w64(!same) != 0) {            // wave-uniform: some pixel of this wave blends
            const int s01 = sample(bx, by, u, v), s10 = sample(cx, cy, u, v), s11 = sample(dx, dy, u, v);
            const uint32_t n = (uint32_t)(wy0 * (wx0 * own + wx1 * s01) + wy1 * (wx0 * s10 + wx1 * s11) + 2 * bs * bs);
            o = same ? own : (int)(__umulhi(n, recip) >> 5);
        }
        return o;
    }
};

// the row frame of bbme_predict.h, one plane per pair
__global__ void __launch_bounds__(PRED_THREADS) k_obmc(const uint8_t* prev, const uint8_t* cur, long long plane_stride, int H, int W,
                                                       int pitch, int bs, int hb, int wb, const int32_t* field, int unit,
                                                       uint32_t recip, uint8_t* out, long long out_stride, int out_pitch,
                                                       unsigned long long* sse)
{
    const int f = blockIdx.z;
    const ObmcPixel px = { prev + (long long)f * plane_stride, field + (long long)f * hb * wb * 2, unit, H, W, pitch, bs, hb, wb, recip };
    predict_rows(px, cur + (long long)f * plane_stride, H, W, pitch, out + (long long)f * out_stride, out_pitch, sse + f);
}

}  // namespace

// the argument rules of obmc.py (GME_ERR_ARG)
int obmc_check_args(const char* who, int H, int W, int bs, int unit)
{
    GME_REQUIRE(bs >= OB_MIN_BS && bs <= OB_MAX_BS, GME_ERR_ARG, "%s: block_size %d (%d .. %d)", who, bs, OB_MIN_BS, OB_MAX_BS);
    GME_REQUIRE(unit == 1 || unit == 4, GME_ERR_ARG, "%s: unit %d (4: whole pixels, 1: quarter pixels)", who, unit);
    GME_REQUIRE(H >= bs && W >= bs, GME_ERR_ARG, "%s: a %d x %d frame holds no block of %d", who, H, W, bs);
    return GME_OK;
}

// out planes = obmc.compensate of the prev planes by field[pairs][hb][wb][2], sse[pairs] (device, zeroed here) = squared error of
// each against its cur plane.  negate: by the negated field (the product with the unit is formed in 64 bits, so INT32_MIN negates
// too): the field is anchored at the predicted frame, as denoise.predict takes it.
int launch_obmc(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
                const int32_t* field, int unit, uint8_t* out, long long out_stride, int out_pitch, unsigned long long* sse, bool negate)
{
    int rc = obmc_check_args("overlapped compensation", H, W, bs, unit);
    if (rc) return rc;
    const int hb = H / bs, wb = W / bs;
    ctx->plan[0] = 0; ctx->plan_patches = 0;
    plan_note(ctx, 0, "k_obmc bs %d unit %d, %d x %d blocks, one wave per row", bs, unit, hb, wb);
    if (pairs == 0) return GME_OK;
    const long long area = 4ll * bs * bs;
    const uint32_t recip = (uint32_t)(((1ll << 37) + area - 1) / area);
    return predict_planes(ctx, pairs, sse, [&](int k, int n) {
        const long long off = (long long)k * plane_stride;
        hipLaunchKernelGGL(k_obmc, predict_grid(H, W, n), dim3(PRED_THREADS), 0, ctx->stream, prev + off, cur + off, plane_stride, H, W,
                           pitch, bs, hb, wb, field + (long long)hb * wb * 2 * k, negate ? -unit : unit, recip, out + (long long)k * out_stride, out_stride,
                           out_pitch, sse + k);
    });
}
