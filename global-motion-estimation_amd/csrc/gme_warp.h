// The per-pixel arithmetic of direct.py (warp, taps, blend), shared by the direct refinement (gme_direct.hip) and the
// per-frame warps of the stabilizer (gme_stab.hip, gme_stab_fill.hip): one rounding per operation, in the order direct.py writes it, so that
// host and device agree bit for bit (the library builds with -ffp-contract=off).
#pragma once
#include "gme_internal.h"

namespace {

struct Sample {
    double up, vp, d;
};

__device__ __forceinline__ Sample warp_at(const double* h, double u, double v)
{
    Sample s;
    s.d = __dadd_rn(__dadd_rn(__dmul_rn(h[6], u), __dmul_rn(h[7], v)), 1.0);
    s.up = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(h[0], u), __dmul_rn(h[1], v)), h[2]), s.d);
    s.vp = __ddiv_rn(__dadd_rn(__dadd_rn(__dmul_rn(h[3], u), __dmul_rn(h[4], v)), h[5]), s.d);
    return s;
}

__device__ __forceinline__ bool inside(const Sample& s, int H, int W)
{
    return s.up >= 0.0 && s.up <= (double)(W - 1) && s.vp >= 0.0 && s.vp <= (double)(H - 1);
}

__device__ __forceinline__ double blend(double g00, double g01, double g10, double g11, double ax, double ay)
{
    const double bx = __dsub_rn(1.0, ax);
    const double top = __dadd_rn(__dmul_rn(bx, g00), __dmul_rn(ax, g01));
    const double bot = __dadd_rn(__dmul_rn(bx, g10), __dmul_rn(ax, g11));
    return __dadd_rn(__dmul_rn(__dsub_rn(1.0, ay), top), __dmul_rn(ay, bot));
}

// taps of an in-frame sample point; the far tap of a coordinate on the last row / column is clamped
struct Taps {
    int x0, y0, x1, y1;
    double ax, ay;
};

__device__ __forceinline__ Taps taps_at(const Sample& s, int H, int W)
{
    Taps t;
    const double fx = floor(s.up), fy = floor(s.vp);
    t.ax = __dsub_rn(s.up, fx);
    t.ay = __dsub_rn(s.vp, fy);
    t.x0 = (int)fx;
    t.y0 = (int)fy;
    t.x1 = min(t.x0 + 1, W - 1);
    t.y1 = min(t.y0 + 1, H - 1);
    return t;
}

__device__ __forceinline__ double sample(const uint8_t* p, int pitch, const Taps& t)
{
    return blend((double)p[(long long)t.y0 * pitch + t.x0], (double)p[(long long)t.y0 * pitch + t.x1],
                 (double)p[(long long)t.y1 * pitch + t.x0], (double)p[(long long)t.y1 * pitch + t.x1], t.ax, t.ay);
}

}  // namespace
