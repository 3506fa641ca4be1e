// Direct projective refinement (host definition: direct.py).  A projective warp per pair, estimated
// from the pixels of the resident pyramids (gme_seq::level) coarse to fine by Gauss-Newton with step halving under a
// truncated quadratic, and the dense sub-pixel compensation under it.
//
// Kernels:
//   k_direct_hist      warp, bilinear sample, residual: per-pair histogram of |e| (integer atomics, order-independent)
//   k_direct_sums      warp, bilinear sample, gradient taps: per-workgroup slab of the 44 Gauss-Newton sums, sum e^2 and
//                      the valid / inlier counts (no float atomics)
//   k_direct_state     one workgroup per pair: threshold, ordered reduction of the slabs, accept / halve / solve, flags
//   k_compensate_proj  compensation + squared error
// Every launch of a refinement is queued up front (launch counts depend on max_iters only); a pair whose level has ended
// returns at the top of each kernel.
#include "gme_passes.h"
#include "gme_warp.h"

namespace {

constexpr int DIRECT_THREADS = 256;
constexpr int DIRECT_PPT = 32;                                  // pixels per thread of a hist / sums workgroup
constexpr int DIRECT_TILE = DIRECT_THREADS * DIRECT_PPT;        // pixels per workgroup (row-major pixel index order)
constexpr int HIST_BINS = 4096;                                 // |e| bins of width 1/16
constexpr int N_GN = 44;                                        // JtJ upper triangle (36, row by row) | Jte (8)
constexpr int SLAB = 48;                                        // N_GN | sum e^2 over the inliers | n_valid | n_in | 0
constexpr int STATE_THREADS = 128;                              // >= 8 x 9: one element of the augmented system each
constexpr int MAX_HALVINGS = 4;
constexpr double CONVERGED_PX = 1e-3;

enum { PH_START = 0, PH_TRY = 1, PH_FINAL = 2, PH_EVAL = 3 };
enum { ST_BEGIN = 0, ST_THRESHOLD = 1, ST_STEP = 2, ST_FINAL_PREP = 3, ST_FINAL = 4, ST_EVAL_BEGIN = 5, ST_EVAL_OUT = 6 };

struct DirectState {
    double init[8];               // full-resolution start (returned under flags 1, 2, 4, 8)
    double h[8];                  // accepted parameters, in the current level's coordinates
    double trial[8];              // what the next hist / sums pass evaluates
    double step[8];               // the step trial - h
    double cost, t;               // accepted cost; the level's threshold
    int flags, finished, level_done, phase, iters, halvings, trial_bad, pad;
};

// central differences with replicated edges, at an integer pixel
__device__ __forceinline__ void grad_at(const uint8_t* p, int pitch, int H, int W, int y, int x, double& gx, double& gy)
{
    const uint8_t* row = p + (long long)y * pitch;
    gx = __dmul_rn((double)((int)row[min(x + 1, W - 1)] - (int)row[max(x - 1, 0)]), 0.5);
    gy = __dmul_rn((double)((int)p[(long long)min(y + 1, H - 1) * pitch + x] - (int)p[(long long)max(y - 1, 0) * pitch + x]), 0.5);
}

__device__ __forceinline__ bool corners_ok(const double* h, int H, int W)
{
    const double us[2] = { 0.0, (double)(W - 1) }, vs[2] = { 0.0, (double)(H - 1) };
    bool ok = true;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            ok = ok && __dadd_rn(__dadd_rn(__dmul_rn(h[6], us[b]), __dmul_rn(h[7], vs[a])), 1.0) > 0.0;
    return ok;
}

__device__ __forceinline__ double corner_shift(const double* a, const double* b, int H, int W)
{
    const double us[2] = { 0.0, (double)(W - 1) }, vs[2] = { 0.0, (double)(H - 1) };
    double m = 0.0;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            const Sample sa = warp_at(a, us[j], vs[i]), sb = warp_at(b, us[j], vs[i]);
            m = fmax(m, fmax(fabs(__dsub_rn(sb.up, sa.up)), fabs(__dsub_rn(sb.vp, sa.vp))));
        }
    return m;
}

// a pass evaluates the pair's trial parameters unless the pair or its level is done, or the trial is not evaluable
__device__ __forceinline__ bool pass_skips(const DirectState& s)
{
    return s.finished || s.level_done || s.trial_bad;
}

// ---------------------------------------------------------------------------------------------------------------------
// Histogram of |e| at the trial parameters; grid (tiles, pairs), hist[P][4096] zeroed by the launcher.
__global__ void __launch_bounds__(DIRECT_THREADS) k_direct_hist(const uint8_t* prev, const uint8_t* cur, long long stride,
                                                                int pitch, int H, int W, const DirectState* st, uint32_t* hist)
{
    __shared__ uint32_t lh[HIST_BINS];
    const int pair = blockIdx.y;
    const DirectState& s = st[pair];
    if (pass_skips(s)) return;
    for (int b = threadIdx.x; b < HIST_BINS; b += DIRECT_THREADS) lh[b] = 0;
    __syncthreads();
    double h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = s.trial[k];
    const uint8_t* p = prev + (long long)pair * stride;
    const uint8_t* c = cur + (long long)pair * stride;
    const long long n = (long long)H * W, base = (long long)blockIdx.x * DIRECT_TILE;
    for (int k = 0; k < DIRECT_PPT; ++k) {
        const long long idx = base + (long long)k * DIRECT_THREADS + threadIdx.x;
        if (idx >= n) break;
        const int v = (int)(idx / W), u = (int)(idx - (long long)v * W);
        const Sample sm = warp_at(h, (double)u, (double)v);
        if (!inside(sm, H, W)) continue;
        const double e = __dsub_rn((double)c[(long long)v * pitch + u], sample(p, pitch, taps_at(sm, H, W)));
        const int bin = min((int)floor(__dmul_rn(fabs(e), 16.0)), HIST_BINS - 1);
        atomicAdd(&lh[bin], 1u);
    }
    __syncthreads();
    uint32_t* out = hist + (long long)pair * HIST_BINS;
    for (int b = threadIdx.x; b < HIST_BINS; b += DIRECT_THREADS)
        if (lh[b]) atomicAdd(&out[b], lh[b]);
}

// ---------------------------------------------------------------------------------------------------------------------
// One Gauss-Newton pass at the trial parameters under the level's threshold; grid (tiles, pairs).  Each thread keeps
// float64 partials (fma-accumulated) over its pixels, the wave folds them by a fixed xor butterfly, the four waves' rows
// are added in wave order: slab[pair][tile][48] is a deterministic function of the pair's data.
__global__ void __launch_bounds__(DIRECT_THREADS) k_direct_sums(const uint8_t* prev, const uint8_t* cur, long long stride,
                                                                int pitch, int H, int W, const DirectState* st, double* slab,
                                                                int tiles)
{
    __shared__ double red[DIRECT_THREADS / 64][SLAB];
    const int pair = blockIdx.y;
    const DirectState& s = st[pair];
    if (pass_skips(s)) return;
    double h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = s.trial[k];
    const double t = s.t;
    const uint8_t* p = prev + (long long)pair * stride;
    const uint8_t* c = cur + (long long)pair * stride;
    double acc[N_GN + 1];
#pragma unroll
    for (int k = 0; k <= N_GN; ++k) acc[k] = 0.0;
    int n_valid = 0, n_in = 0;
    const long long n = (long long)H * W, base = (long long)blockIdx.x * DIRECT_TILE;
    for (int k = 0; k < DIRECT_PPT; ++k) {
        const long long idx = base + (long long)k * DIRECT_THREADS + threadIdx.x;
        if (idx >= n) break;
        const int v = (int)(idx / W), u = (int)(idx - (long long)v * W);
        const double du = (double)u, dv = (double)v;
        const Sample sm = warp_at(h, du, dv);
        if (!inside(sm, H, W)) continue;
        ++n_valid;
        const Taps tp = taps_at(sm, H, W);
        const double e = __dsub_rn((double)c[(long long)v * pitch + u], sample(p, pitch, tp));
        if (!(fabs(e) < t)) continue;
        ++n_in;
        double gx00, gy00, gx01, gy01, gx10, gy10, gx11, gy11;
        grad_at(p, pitch, H, W, tp.y0, tp.x0, gx00, gy00);
        grad_at(p, pitch, H, W, tp.y0, tp.x1, gx01, gy01);
        grad_at(p, pitch, H, W, tp.y1, tp.x0, gx10, gy10);
        grad_at(p, pitch, H, W, tp.y1, tp.x1, gx11, gy11);
        const double sx = blend(gx00, gx01, gx10, gx11, tp.ax, tp.ay);
        const double sy = blend(gy00, gy01, gy10, gy11, tp.ax, tp.ay);
        const double q = __dadd_rn(__dmul_rn(sx, sm.up), __dmul_rn(sy, sm.vp));
        const double r = __ddiv_rn(1.0, sm.d);
        double j[8];
        j[0] = __dmul_rn(__dmul_rn(sx, du), r);
        j[1] = __dmul_rn(__dmul_rn(sx, dv), r);
        j[2] = __dmul_rn(sx, r);
        j[3] = __dmul_rn(__dmul_rn(sy, du), r);
        j[4] = __dmul_rn(__dmul_rn(sy, dv), r);
        j[5] = __dmul_rn(sy, r);
        j[6] = __dmul_rn(-__dmul_rn(q, du), r);
        j[7] = __dmul_rn(-__dmul_rn(q, dv), r);
        int m = 0;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = a; b < 8; ++b, ++m) acc[m] = __fma_rn(j[a], j[b], acc[m]);
#pragma unroll
        for (int a = 0; a < 8; ++a) acc[36 + a] = __fma_rn(j[a], e, acc[36 + a]);
        acc[N_GN] = __fma_rn(e, e, acc[N_GN]);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k <= N_GN; ++k) {
        double x = acc[k];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) x = __dadd_rn(x, __shfl_xor(x, m, 64));
        if (lane == 0) red[wave][k] = x;
    }
    int nv = n_valid, ni = n_in;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        nv += __shfl_xor(nv, m, 64);
        ni += __shfl_xor(ni, m, 64);
    }
    if (lane == 0) {
        red[wave][N_GN + 1] = (double)nv;
        red[wave][N_GN + 2] = (double)ni;
        red[wave][N_GN + 3] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < SLAB) {
        double x = red[0][threadIdx.x];
        for (int w = 1; w < DIRECT_THREADS / 64; ++w) x = __dadd_rn(x, red[w][threadIdx.x]);
        slab[((long long)pair * tiles + blockIdx.x) * SLAB + threadIdx.x] = x;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The per-pair state machine (direct.refine): one workgroup per pair.
__device__ __forceinline__ int upper_index(int a, int b) { return 8 * a - a * (a - 1) / 2 + (b - a); }      // a <= b

__device__ __forceinline__ double cost_of(const double* S, double t)
{
    const double nv = S[N_GN + 1], ni = S[N_GN + 2];
    if (nv == 0.0) return INFINITY;
    return __ddiv_rn(__dadd_rn(S[N_GN], __dmul_rn(__dsub_rn(nv, ni), __dmul_rn(t, t))), nv);
}

__device__ __forceinline__ void scale_to_finer(double* h)
{
    h[2] = __dmul_rn(h[2], 2.0); h[5] = __dmul_rn(h[5], 2.0);
    h[6] = __dmul_rn(h[6], 0.5); h[7] = __dmul_rn(h[7], 0.5);
}

__device__ __forceinline__ void set_trial(DirectState& s, int H, int W)
{
    for (int k = 0; k < 8; ++k) s.trial[k] = __dadd_rn(s.h[k], s.step[k]);
    s.trial_bad = corners_ok(s.trial, H, W) ? 0 : 1;
}

__global__ void __launch_bounds__(STATE_THREADS) k_direct_state(DirectState* st_all, int mode, int level, int H, int W,
                                                                const double* params_in, const uint32_t* hist,
                                                                const double* slab, int tiles, double frac, int max_iters,
                                                                double* params_out, int32_t* flags_out, double* eval_out)
{
    __shared__ DirectState s;
    __shared__ double S[SLAB];
    __shared__ long long chunk[STATE_THREADS];
    __shared__ double a[SOLVE2_ROWS][SOLVE2_COLS];
    __shared__ double dsc[SOLVE2_ROWS];
    __shared__ double z[2][SOLVE2_ROWS];
    __shared__ int bad, solve;
    const int pair = blockIdx.x, t = threadIdx.x;
    DirectState& g = st_all[pair];
    if (t == 0) {
        s = g;
        solve = 0;
        bad = 0;
    }
    __syncthreads();

    if (mode == ST_BEGIN || mode == ST_EVAL_BEGIN) {
        if (t == 0) {
            if (mode == ST_EVAL_BEGIN || level == 0) {
                for (int k = 0; k < 8; ++k) s.init[k] = params_in[(long long)pair * 8 + k];
                s.flags = 0; s.finished = 0;
                for (int k = 0; k < 8; ++k) s.h[k] = s.init[k];
                if (mode == ST_BEGIN) {                           // full resolution -> level 0: h2, h5 / 4, h6, h7 x 4
                    s.h[2] = __dmul_rn(s.h[2], 0.25); s.h[5] = __dmul_rn(s.h[5], 0.25);
                    s.h[6] = __dmul_rn(s.h[6], 4.0); s.h[7] = __dmul_rn(s.h[7], 4.0);
                }
            } else if (!s.finished) {
                scale_to_finer(s.h);
            }
            s.level_done = 0; s.iters = 0; s.halvings = 0; s.trial_bad = 0;
            s.phase = mode == ST_EVAL_BEGIN ? PH_EVAL : PH_START;
            for (int k = 0; k < 8; ++k) { s.trial[k] = s.h[k]; s.step[k] = 0.0; }
            if (mode == ST_BEGIN && !s.finished && !corners_ok(s.h, H, W)) { s.flags |= 4; s.finished = 1; }
            g = s;
        }
        return;
    }
    if (s.finished || (s.level_done && mode == ST_STEP)) {
        if (mode == ST_FINAL && t == 0) {
            for (int k = 0; k < 8; ++k) params_out[(long long)pair * 8 + k] = s.init[k];
            flags_out[pair] = s.flags;
        }
        return;
    }

    if (mode == ST_THRESHOLD) {
        // n_valid and the first bin at which the cumulative count reaches ceil((1 - f) n_valid): chunk sums, then a walk
        const uint32_t* hp = hist + (long long)pair * HIST_BINS;
        constexpr int per = HIST_BINS / STATE_THREADS;
        long long cs = 0;
        for (int b = 0; b < per; ++b) cs += hp[t * per + b];
        chunk[t] = cs;
        __syncthreads();
        if (t == 0) {
            long long nv = 0;
            for (int k = 0; k < STATE_THREADS; ++k) nv += chunk[k];
            double thr = 0.0;
            if (nv > 0) {
                long long need = (long long)ceil(__dmul_rn(__dsub_rn(1.0, frac), (double)nv));
                need = need < 1 ? 1 : need > nv ? nv : need;
                long long cum = 0;
                int k = 0;
                while (cum + chunk[k] < need) cum += chunk[k++];
                int b = k * per;
                while (cum + hp[b] < need) cum += hp[b++];
                thr = (double)(b + 1) / 16.0;
            }
            s.t = thr;
            if (s.phase != PH_EVAL && 4 * nv < (long long)H * W) { s.flags |= 2; s.finished = 1; }
            g = s;
        }
        return;
    }

    if (mode == ST_FINAL_PREP) {
        if (t == 0) {
            for (int k = 0; k < 8; ++k) s.trial[k] = s.init[k];
            s.trial_bad = corners_ok(s.trial, H, W) ? 0 : 1;
            s.level_done = 0;
            s.phase = PH_FINAL;
            g = s;
        }
        return;
    }

    // the pass's sums, reduced over the tiles in order
    const bool evaluated = !s.trial_bad;
    if (evaluated && t < SLAB) {
        const double* sp = slab + (long long)pair * tiles * SLAB + t;
        double x = sp[0];
        for (int k = 1; k < tiles; ++k) x = __dadd_rn(x, sp[(long long)k * SLAB]);
        S[t] = x;
    }
    __syncthreads();

    if (mode == ST_EVAL_OUT) {
        if (t < N_GN) eval_out[(long long)pair * 48 + 4 + t] = S[t];
        if (t == 0) {
            double* o = eval_out + (long long)pair * 48;
            o[0] = s.t; o[1] = S[N_GN + 1]; o[2] = S[N_GN + 2]; o[3] = cost_of(S, s.t);
        }
        return;
    }
    double c = INFINITY;
    if (evaluated && 4 * (long long)S[N_GN + 1] >= (long long)H * W) c = cost_of(S, s.t);
    if (mode == ST_FINAL) {
        if (t == 0) {
            const bool gain = s.cost < c;
            if (!gain) s.flags |= 8;
            for (int k = 0; k < 8; ++k) params_out[(long long)pair * 8 + k] = gain ? s.h[k] : s.init[k];
            flags_out[pair] = s.flags;
        }
        return;
    }

    // ST_STEP
    if (t == 0) {
        if (s.phase == PH_START) {
            s.cost = c;
            solve = 1;
        } else if (c <= s.cost) {                                 // accepted
            const double moved = corner_shift(s.h, s.trial, H, W);
            for (int k = 0; k < 8; ++k) s.h[k] = s.trial[k];
            s.cost = c;
            s.iters += 1;
            if (moved <= CONVERGED_PX) {
                s.level_done = 1;
            } else if (s.iters >= max_iters) {
                s.level_done = 1;
                if (level == 2) s.flags |= 16;
            } else {
                solve = 1;
            }
        } else if (++s.halvings > MAX_HALVINGS) {
            s.level_done = 1;
        } else {
            for (int k = 0; k < 8; ++k) s.step[k] = __dmul_rn(s.step[k], 0.5);
            set_trial(s, H, W);
        }
    }
    __syncthreads();
    if (solve) {
        const int tr = t / 9, tc = t - tr * 9;
        if (tr < 8) a[tr][tc] = tc < 8 ? S[upper_index(min(tr, tc), max(tr, tc))] : S[36 + tr];
        __syncthreads();
        double pmin, pmax;
        equilibrated_solve(a, dsc, z, 8, 1, t, &bad, &pmin, &pmax);
        if (t == 0) {
            if (bad || pmin == 0.0 || !(__ddiv_rn(pmin, pmax) >= 1e-12)) {
                s.flags |= 1;
                s.finished = 1;
            } else {
                for (int k = 0; k < 8; ++k) s.step[k] = __dmul_rn(z[0][k], dsc[k]);
                s.halvings = 0;
                s.phase = PH_TRY;
                set_trial(s, H, W);
            }
        }
    }
    if (t == 0) g = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// out[v][u] = floor(bilinear(prev)(u', v') + 0.5) where the sample point is in the frame, prev[v][u] elsewhere; sse[pair]
// += (cur - out)^2 (integer atomics).  grid ((W + 255) / 256, H, pairs).
__global__ void __launch_bounds__(256) k_compensate_proj(const uint8_t* prev, const uint8_t* cur, long long stride, int pitch,
                                                         int H, int W, const double* params, uint8_t* out,
                                                         long long out_stride, int out_pitch, unsigned long long* sse)
{
    const int pair = blockIdx.z, v = blockIdx.y, u = blockIdx.x * 256 + threadIdx.x;
    unsigned err = 0;
    if (u < W) {
        double h[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = params[(long long)pair * 8 + k];
        const uint8_t* p = prev + (long long)pair * stride;
        const Sample sm = warp_at(h, (double)u, (double)v);
        int o = p[(long long)v * pitch + u];
        if (inside(sm, H, W)) o = (int)floor(__dadd_rn(sample(p, pitch, taps_at(sm, H, W)), 0.5));
        out[(long long)pair * out_stride + (long long)v * out_pitch + u] = (uint8_t)o;
        const int df = (int)cur[(long long)pair * stride + (long long)v * pitch + u] - o;
        err = (unsigned)(df * df);
    }
    for (int m = 32; m > 0; m >>= 1) err += (unsigned)__shfl_xor((int)err, m, 64);
    if ((threadIdx.x & 63) == 0 && err) atomicAdd(&sse[pair], (unsigned long long)err);
}

}  // namespace

// ---- launchers --------------------------------------------------------------------------------------------------------
static int direct_tiles(int H, int W) { return (int)(((long long)H * W + DIRECT_TILE - 1) / DIRECT_TILE); }

// the sequence's workspace for `pairs` pairs: state | hist | slab | io (params in, params out, flags, eval rows)
struct DirectWs : DirectIo {
    DirectState* st;
    uint32_t* hist;
    double* slab;
    int tiles;
};

static int direct_ws(gme_seq* s, int pairs, DirectWs* ws)
{
    const int tiles = direct_tiles(s->level[2].H, s->level[2].W);
    const size_t P = (size_t)(pairs > 0 ? pairs : 1);
    const size_t b_st = P * sizeof(DirectState), b_hist = P * HIST_BINS * sizeof(uint32_t), b_slab = P * tiles * SLAB * sizeof(double);
    const size_t b_io = P * (8 + 8 + 48) * sizeof(double) + P * sizeof(int32_t);
    const size_t want = b_st + b_hist + b_slab + b_io;
    const int rc = s->passes->direct.ensure(want, "direct refinement workspace");
    if (rc) return rc;
    char* b = (char*)s->passes->direct.get();
    ws->st = (DirectState*)b; b += b_st;
    ws->hist = (uint32_t*)b; b += b_hist;
    ws->slab = (double*)b; b += b_slab;
    ws->in = (double*)b; b += P * 8 * sizeof(double);
    ws->out = (double*)b; b += P * 8 * sizeof(double);
    ws->eval = (double*)b; b += P * 48 * sizeof(double);
    ws->flags = (int32_t*)b;
    ws->tiles = tiles;
    return GME_OK;
}

int direct_io(gme_seq* s, int pairs, DirectIo* io)
{
    DirectWs ws;
    const int rc = direct_ws(s, pairs, &ws);
    if (rc) return rc;
    *io = ws;
    return GME_OK;
}

// one hist or sums pass of level l over all pairs, in chunks of max_grid_planes() pairs
static int direct_pass(gme_seq* s, int fd, int l, int pairs, const DirectWs& ws, bool hist)
{
    const Plane& p = s->level[l];
    const int tiles = direct_tiles(p.H, p.W), step = max_grid_planes();
    for (int first = 0; first < pairs; first += step) {
        const int n = pairs - first < step ? pairs - first : step;
        if (hist)
            hipLaunchKernelGGL(k_direct_hist, dim3(tiles, n), dim3(DIRECT_THREADS), 0, s->ctx->stream, p.at(first), p.at(first + fd),
                               (long long)p.stride, p.pitch, p.H, p.W, ws.st + first, ws.hist + (size_t)first * HIST_BINS);
        else
            hipLaunchKernelGGL(k_direct_sums, dim3(tiles, n), dim3(DIRECT_THREADS), 0, s->ctx->stream, p.at(first), p.at(first + fd),
                               (long long)p.stride, p.pitch, p.H, p.W, ws.st + first, ws.slab + (size_t)first * tiles * SLAB, tiles);
    }
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}

static int direct_state(gme_seq* s, int mode, int l, int pairs, const DirectWs& ws, double frac, int max_iters)
{
    const Plane& p = s->level[l];
    hipLaunchKernelGGL(k_direct_state, dim3((unsigned)pairs), dim3(STATE_THREADS), 0, s->ctx->stream, ws.st, mode, l, p.H, p.W,
                       ws.in, ws.hist, ws.slab, direct_tiles(p.H, p.W), frac, max_iters, ws.out, ws.flags, ws.eval);
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}

static int direct_threshold(gme_seq* s, int fd, int l, int pairs, const DirectWs& ws, double frac)
{
    GME_HIP_TRY(hipMemsetAsync(ws.hist, 0, (size_t)pairs * HIST_BINS * sizeof(uint32_t), s->ctx->stream));
    int rc = direct_pass(s, fd, l, pairs, ws, true);
    if (rc) return rc;
    return direct_state(s, ST_THRESHOLD, l, pairs, ws, frac, 0);
}

// gme_seq_refine_projective: ws.in[P][8] (full resolution) -> ws.out[P][8], ws.flags[P]; pyramids built, ws from direct_io
int launch_direct_refine(gme_seq* s, int fd, int pairs, double frac, int max_iters)
{
    if (pairs == 0) return GME_OK;
    DirectWs ws;
    int rc = direct_ws(s, pairs, &ws);
    if (rc) return rc;
    const int passes = 1 + (MAX_HALVINGS + 1) * max_iters;       // the start pass + at most 5 trials per iteration
    for (int l = 0; l <= 2 && !rc; ++l) {
        rc = direct_state(s, ST_BEGIN, l, pairs, ws, frac, max_iters);
        if (!rc) rc = direct_threshold(s, fd, l, pairs, ws, frac);
        for (int k = 0; k < passes && !rc; ++k) {
            rc = direct_pass(s, fd, l, pairs, ws, false);
            if (!rc) rc = direct_state(s, ST_STEP, l, pairs, ws, frac, max_iters);
        }
    }
    if (!rc) rc = direct_state(s, ST_FINAL_PREP, 2, pairs, ws, frac, max_iters);
    if (!rc) rc = direct_pass(s, fd, 2, pairs, ws, false);
    if (!rc) rc = direct_state(s, ST_FINAL, 2, pairs, ws, frac, max_iters);
    return rc;
}

// gme_seq_direct_eval: ws.in[P][8] (level l) -> ws.eval[P][48] = threshold, n_valid, n_in, cost, sums[44]
int launch_direct_eval(gme_seq* s, int fd, int l, int pairs, double frac)
{
    if (pairs == 0) return GME_OK;
    DirectWs ws;
    int rc = direct_ws(s, pairs, &ws);
    if (!rc) rc = direct_state(s, ST_EVAL_BEGIN, l, pairs, ws, frac, 0);
    if (!rc) rc = direct_threshold(s, fd, l, pairs, ws, frac);
    if (!rc) rc = direct_pass(s, fd, l, pairs, ws, false);
    if (!rc) rc = direct_state(s, ST_EVAL_OUT, l, pairs, ws, frac, 0);
    return rc;
}

// gme_seq_compensate_projective: params[P][8] (device) -> s->comp, s->sse
int launch_compensate_proj(gme_seq* s, int fd, int pairs, const double* params)
{
    if (pairs == 0) return GME_OK;
    const Plane& p = s->level[2];
    GME_HIP_TRY(hipMemsetAsync(s->sse, 0, sizeof(unsigned long long) * pairs, s->ctx->stream));
    const int step = max_grid_planes();
    for (int first = 0; first < pairs; first += step) {
        const int n = pairs - first < step ? pairs - first : step;
        hipLaunchKernelGGL(k_compensate_proj, dim3((p.W + 255) / 256, p.H, n), dim3(256), 0, s->ctx->stream, p.at(first),
                           p.at(first + fd), (long long)p.stride, p.pitch, p.H, p.W, params + (size_t)first * 8,
                           s->comp.at(first), (long long)s->comp.stride, s->comp.pitch, s->sse + first);
    }
    GME_HIP_TRY(hipGetLastError());
    return GME_OK;
}
