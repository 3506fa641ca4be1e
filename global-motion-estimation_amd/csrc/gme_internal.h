// Internal declarations shared by the translation units of libgme_hip.so: contexts, planes, the resident sequence, the block
// search, the global-motion stages and the compensation.  bench.py hashes this file into the identity of every benchmarked
// kernel (COMMON_SOURCES), so what only the passes built on this core need is declared in gme_passes.h instead.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gme_hip.h"
#include "dev_buf.h"

#define GME_HIP_TRY(expr)                                                                  \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) {                                                           \
            gme_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, \
                          __LINE__);                                                       \
            return GME_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define GME_REQUIRE(cond, code, ...)       \
    do {                                   \
        if (!(cond)) {                     \
            gme_set_error(__VA_ARGS__);    \
            return (code);                 \
        }                                  \
    } while (0)

// An image plane (or a stack of equally sized planes) in HBM: a view that is copied freely and owns nothing.
// pitch is a multiple of 64 bytes; bytes between W and pitch are zero.
struct Plane {
    uint8_t* ptr = nullptr;
    int H = 0, W = 0, pitch = 0;
    int64_t stride = 0;   // bytes between consecutive planes of a stack
    int count = 0;
    size_t bytes() const { return (size_t)stride * (size_t)count; }
    uint8_t* at(int i) const { return ptr + (int64_t)i * stride; }
};

// A plane stack with its memory (plane_alloc).  Wherever a Plane is wanted it is the view of the whole stack.
struct PlaneBuf : Plane {
    DevBuf<uint8_t> mem;
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The plane geometry of the library as a view without memory.  Whoever gives it memory adds a guard row of `pitch` bytes
// behind the stack where dword loads near the last row must stay inside (plane_alloc; gme_bbme_u8, gme_subpel_u8).
inline Plane plane_shape(int H, int W, int count)
{
    Plane v;
    v.H = H; v.W = W; v.count = count; v.pitch = round_up(W, 64);
    v.stride = (int64_t)round_up(v.pitch * H, 256);
    return v;
}

// Which planes of a stack a call has written (the compensated and the warped frames, the masks): empty until the stack has
// memory.
struct WrittenFrames {
    std::vector<uint8_t> flag;
    void mark(int first, int count) { for (int k = first; k < first + count; ++k) flag[(size_t)k] = 1; }
    bool all(int first, int count) const
    {
        for (int k = first; k < first + count; ++k)
            if ((size_t)k >= flag.size() || !flag[(size_t)k]) return false;
        return true;
    }
};

struct gme_ctx {
    std::mutex mu;                // held by every C-ABI entry point for the whole call (GME_ENTER below)
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipDeviceProp_t prop;
    // growable device scratch for the single-pair convenience calls
    DevBuf<uint8_t> scratch;
    DevBuf<int> status;           // device words (GME_STATUS_WORDS): [0] set by kernels whose safety guards trip;
                                  // [GME_STATUS_TILECTR ..] per-XCD tile counters of the persistent search kernels,
                                  // [GME_STATUS_STATS ..] per-XCD statistics of the last block-matching call (16 words apart)
    void* comm = nullptr;         // RCCL communicator (gme_comm.hip), one per context = per rank
    int comm_rank = 0, comm_world = 0;
    hipStream_t copy_stream = nullptr, back_stream = nullptr;   // gme_seq_bbme_streamed: uploads / read-backs beside the kernels
    DevBuf<uint8_t> stage;        // device staging of tight host frames (gme_seq_bbme_streamed), repacked into the planes
    DevBuf<uint32_t> redo_list;   // tiles the elimination kernels hand to the brute-force redo kernel (grown on demand)
    char plan[192] = "";          // kernel / tile shape / schedule the last block-matching call chose (gme_last_bbme_info)
    long long plan_patches = 0;   // candidate patches that call's bound was applied to (0: a kernel without elimination)
};
constexpr int GME_STATUS_WORDS = 1024, GME_STATUS_TILECTR = 64, GME_STATUS_STATS = 256;
constexpr int GME_STATUS_REDO = 512;           // [0] tiles listed for the redo kernel, [1] items it has drawn
int ctx_redo_list(gme_ctx* ctx, size_t entries, uint32_t** out);

void plan_note(gme_ctx* ctx, long long patches, const char* fmt, ...);

int ctx_scratch(gme_ctx* ctx, size_t bytes, void** out);
int plane_alloc(gme_ctx* ctx, PlaneBuf* p, int count, int H, int W);      // a failure leaves *p empty (no memory, a null view)

struct FitLevelBuf {
    int h = 0, w = 0;             // motion-field shape at this level
    int32_t* gt = nullptr;        // [P][h][w][2]: gt_own, or a field the fit only reads (gme_seq::fit_mv borrows gme_seq::mv)
    DevBuf<int32_t> gt_own;
    DevBuf<int16_t> model;        // [P][h][w][2]
    DevBuf<uint8_t> mask;         // [P][h][w]
    DevBuf<int32_t> diff;         // [P][h][w] L1 distance gt vs model
    DevBuf<int4> list;            // [P][h][w] inlier list, only for fields too large for LDS
    DevBuf<int32_t> thr;          // [P]
    DevBuf<double> sums;          // [P][15]
    DevBuf<double> sums2;         // [P][27] order-2 sums (gme_seq_gme_fit2)
};
// the fit kernels keep a level's inlier list in LDS up to this size (two workgroups per CU), in `list` above it
constexpr size_t FIT_LIST_LDS_BYTES = 40 * 1024;

struct SeqPasses;                 // gme_passes.h

struct gme_seq {
    gme_ctx* ctx = nullptr;
    int N = 0, H = 0, W = 0;      // N: frames in use (gme_seq_set_frames), <= N_cap
    int N_cap = 0;                // frames the sequence was created for: every buffer is sized for it
    PlaneBuf level[3];            // level[2] = full resolution, [1], [0] = pyramid
    bool pyramids_valid = false;
    // generic BBME result
    DevBuf<int32_t> mv;           // [P][h][w][2]
    int mv_h = 0, mv_w = 0, mv_pairs = 0;
    int mv_fd = 0, mv_bs = 0;     // frame distance and block size of the search that wrote `mv`
    DevBuf<uint32_t> sqbox[3];    // per level: 16x16 box sums of squares per frame (MSE fast path)
    bool sqbox_valid[3] = { false, false, false };
    int sqbox_kind[3] = { 0, 0, 0 };
    // GME state
    int gme_fd = 0, gme_bs = 0, gme_pairs = 0;
    int gme_procedure = 0, gme_sw = 0;
    bool bbme_pending[3] = { false, false, false };   // level searches gme_seq_gme_begin deferred (see there)
    bool split_phase = false;     // gme_seq_set_split_phase: begin / fit / compensate return once their work is queued
    hipEvent_t ready = nullptr;   // recorded behind the last result copy of such a call; gme_seq_wait waits on it
    hipEvent_t upload_gate = nullptr, uploaded = nullptr;   // split-phase gme_seq_upload: ties the shared upload stream to this context's stream
    FitLevelBuf fit[3];           // fit[0].gt = dense field
    FitLevelBuf fit_mv;           // stage buffers for fitting `mv` directly: its gt is mv, gt_own stays empty
    int fit_mv_pairs = 0;
    DevBuf<double> mv_params;     // [P][6] parameters for fit_mv ([P][12] after gme_seq_gme_fit2)
    // sized together with fit[] by gme_begin_common: params0 holds 6 floats for each pair they were allocated for
    DevBuf<float> params0;        // [P][6]
    DevBuf<double> params_in;     // [P][6], or [P][12] for gme_seq_gme_fit2 (room for 12 per pair)
    DevBuf<int32_t> solve_flags;  // [P] gme_seq_gme_device_solve: pairs whose device solve must be redone on the host
    // compensation
    PlaneBuf comp;                // [P] compensated frames: one stack for every compensating / predicting call
    WrittenFrames comp_written;   // the planes the last of those calls wrote (ensure_comp clears, comp_wrote marks)
    DevBuf<double> comp_params;   // [P][6], or [P][12] for gme_seq_compensate2 (room for 12 per pair)
    DevBuf<int32_t> comp_mf;      // [P][h][w][2] order-2 field gme_seq_compensate2 compensates with
    DevBuf<unsigned long long> sse;      // [P]
    // per-pair summary rows of `mv` (gme_seq_mv_summary) and their all-gather over the ranks (gme_seq_mv_summary_gather)
    DevBuf<double> summary;       // [n_max][6], zero-padded behind mv_pairs rows
    DevBuf<double> gathered;      // [world][n_max][6]
    // Everything the passes built on this core keep between calls (gme_passes.h): made by gme_seq_create with passes_create,
    // freed by gme_seq_destroy with passes_destroy.  A pass that keeps a result adds it there, not here.
    SeqPasses* passes = nullptr;
    DevBuf<uint8_t> synth_canvas;
    uint64_t synth_seed = 0;
    bool synth_valid = false;
};

// ---- kernel launchers (bbme_kernels.hip) -----------------------------------
struct BbmeJob {
    const uint8_t* prev = nullptr;        // first "previous" plane
    const uint8_t* cur = nullptr;         // first "current" plane
    int64_t plane_stride = 0;     // bytes between consecutive pairs' planes (same for prev/cur)
    int pairs = 0;
    int H = 0, W = 0, pitch = 0;
    int bs = 0, sw = 0, procedure = 0, pnorm = 0;
    int32_t* mf = nullptr;        // [pairs][H/bs][W/bs][2]
    const uint32_t* sqbox_cur = nullptr;  // optional, matches `cur` planes: [pairs][H][pitch] uint32 (SqTable)
    int64_t sqbox_stride = 0;     // elements between consecutive planes
    int sqbox_kind = 0;           // what sqbox_cur holds (bbme_aux_kind): each kernel that reads it declines the other kind
    bool chained = false;         // a later chunk of one streamed call: keep the plan text and the statistics
    bool status_fresh = false;    // launch_bbme has just cleared the tile counters and redo words (first chunk of a call)
};
int launch_bbme(gme_ctx* ctx, const BbmeJob& job);
// the most pairs one kernel launch of launch_bbme carries for `pairs` pairs of H x W at block size bs
long long bbme_pairs_per_launch(int H, int W, int bs, long long pairs);
int launch_exh_redo(gme_ctx* ctx, const BbmeJob& job, int R, int tr, int tc, int tile_wg_per_row, int tile_wg_per_pair,
                    const uint32_t* list, const uint32_t* count, uint32_t* head);
// The table of 16x16 box sums of squares (exhaustive MSE, bs 16): uint32 [H][pitch] per frame, positions are those of the
// frame (row * pitch + column); rows > H - 16 and columns > W - 16 hold nothing.  The four positions x .. x+3 of a row
// (x % 4 == 0) come with one 16-byte read.  (A 24-bit layout -- 16-bit and 8-bit planes, 3 instead of 4 bytes per position --
// was tried in round 3: the table kernel's two narrower stores per row made IT 17 % slower, 1.43 against 1.22 ms per 2049
// frames of 720x480, and the whole MSE search 4 %.)
#ifdef __HIPCC__
// Wave-wide reductions without LDS traffic: four DPP steps leave every lane with the result of its 16-lane row (xor 1,
// xor 2 inside quads, then the two mirrors); row_bcast:15 folds rows 0 and 2 into rows 1 and 3, row_bcast:31 folds row 1
// into row 3, and one v_readlane of lane 63 makes the result scalar (round 4: 7 instead of 11 instructions; rounds 1-3
// read one lane of every row and combined them on the scalar side).
#define GME_DPP(v, ctrl) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), 0xF, 0xF, false))
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
    v = min(v, GME_DPP(v, 0xB1));                          // quad_perm [1,0,3,2]
    v = min(v, GME_DPP(v, 0x4E));                          // quad_perm [2,3,0,1]
    v = min(v, GME_DPP(v, 0x141));                         // row_half_mirror
    v = min(v, GME_DPP(v, 0x140));                         // row_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x142, 0xA, 0xF, false));     // row_bcast:15 -> rows 1, 3
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, 0x143, 0xC, 0xF, false));     // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    v += GME_DPP(v, 0xB1);
    v += GME_DPP(v, 0x4E);
    v += GME_DPP(v, 0x141);
    v += GME_DPP(v, 0x140);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);             // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);             // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The small symmetric systems of the device solves (k_solve_model2, gme_kernels.hip; k_direct_state, gme_direct.hip): the n x n
// normal matrix in a[0:n][0:n] with nrhs <= 2 right-hand sides in columns n .. n + nrhs - 1, held in LDS, solved by the
// threads t = threadIdx.x of one workgroup (at least n * (n + nrhs) of them).  Jacobi equilibration D N D z = D rhs with
// dsc = D = 1 / sqrt(diag) (a non-positive diagonal ORs 4 into *bad), then Gaussian elimination with partial pivoting (the
// first largest |a[r][k]|, as LAPACK's idamax) and back substitution into z[rhs][0:n]; x = z * dsc.  *pmin / *pmax: the
// smallest and largest |pivot|.  Every operation is rounded on its own (*_rn).  Ends with a barrier.
constexpr int SOLVE2_ROWS = 8, SOLVE2_COLS = 10;     // pseudo-perspective / projective: 8 unknowns; quadratic: 6 + two right-hand sides
__device__ __forceinline__ void equilibrated_solve(double (&a)[SOLVE2_ROWS][SOLVE2_COLS], double (&dsc)[SOLVE2_ROWS],
                                                   double (&z)[2][SOLVE2_ROWS], int n, int nrhs, int t, int* bad,
                                                   double* pmin_out, double* pmax_out)
{
    const int ncol = n + nrhs, tr = t / ncol, tc = t - tr * ncol;  // this thread's element of the augmented system
    if (t < n) {
        const double d = a[t][t];
        if (!(d > 0.0)) atomicOr(bad, 4);
        dsc[t] = __ddiv_rn(1.0, __dsqrt_rn(d));
    }
    __syncthreads();
    if (tr < n) a[tr][tc] = tc < n ? __dmul_rn(__dmul_rn(a[tr][tc], dsc[tr]), dsc[tc]) : __dmul_rn(a[tr][tc], dsc[tr]);
    __syncthreads();

    double pmin = INFINITY, pmax = 0.0;
    for (int k = 0; k < n; ++k) {
        int piv = k;
        double big = fabs(a[k][k]);
        for (int r = k + 1; r < n; ++r) {
            const double v = fabs(a[r][k]);
            if (v > big) { big = v; piv = r; }
        }
        pmin = fmin(pmin, big);
        pmax = fmax(pmax, big);
        __syncthreads();                                         // column k read by all before rows move
        if (piv != k && t < ncol) { const double u = a[k][t]; a[k][t] = a[piv][t]; a[piv][t] = u; }
        __syncthreads();
        // row k + 1 + tr: only columns > k change; column k and row k are read, never written, in this step
        const int r = k + 1 + tr;
        if (r < n && tc > k) a[r][tc] = __dsub_rn(a[r][tc], __dmul_rn(__ddiv_rn(a[r][k], a[k][k]), a[k][tc]));
        __syncthreads();
    }
    if (t < nrhs) {
        for (int k = n - 1; k >= 0; --k) {
            double u = a[k][n + t];
            for (int c = k + 1; c < n; ++c) u = __dsub_rn(u, __dmul_rn(a[k][c], z[t][c]));
            z[t][k] = __ddiv_rn(u, a[k][k]);
        }
    }
    __syncthreads();
    *pmin_out = pmin;
    *pmax_out = pmax;
}

typedef const uint32_t* SqTable;
__device__ __forceinline__ SqTable sq_table(const uint32_t* slot, int, int) { return slot; }
__device__ __forceinline__ uint32_t sq1(SqTable t, long long idx) { return t[idx]; }
__device__ __forceinline__ void sq4(SqTable t, long long idx, uint32_t (&out)[4])       // idx % 4 == 0
{
    const uint4 v = *(const uint4*)(t + idx);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
}
#endif
int launch_sqbox16(gme_ctx* ctx, const uint8_t* src, long long src_stride, int count, int H, int W, int pitch,
                   uint32_t* out, long long stride, bool sgn);
// per-frame auxiliary table a fast exhaustive kernel wants for `cur` (BbmeJob::sqbox_cur, BbmeJob::sqbox_kind) when
// launch_bbme searches `pairs` pairs of H x W planes with row pitch `pitch`:
// 0 none, 1 = 16x16 box sums of squares (MSE, k_exh_dot16 and the elimination kernels), 2 = 16x16 box sums of the squares
// of (byte - 128) (MSE on the matrix cores, bbme_mfma.hip: exactly the jobs bbme_mfma_takes)
int bbme_aux_kind(int H, int W, int pitch, long long pairs, int bs, int sw, int procedure, int pnorm);
int launch_aux_table(gme_ctx* ctx, int kind, const uint8_t* src, long long src_stride, int count, int H, int W,
                     int pitch, uint32_t* out, long long stride);
bool bbme_sea_applies(int bs, int sw, int procedure, int pnorm);
// ---- bbme_mfma.hip: exhaustive MSE at bs 16 as an int8 correlation on the matrix cores
bool bbme_mfma_wanted(int sw);                // search windows it takes (and GME_EXH_MFMA has not switched it off)
// exhaustive MSE at bs 16 that k_exh_mfma16 searches: a wanted window and a geometry its grid and its 32-bit table offsets
// hold; `pairs` = the most pairs one launch carries (bbme_pairs_per_launch)
bool bbme_mfma_takes(int H, int W, int pitch, long long pairs, int sw);
int launch_bbme_mfma(gme_ctx* ctx, const BbmeJob& job, bool* handled);

int bbme_check_args(int H, int W, int bs, int sw, int procedure, int pnorm);

// ---- gme_kernels.hip --------------------------------------------------------
int max_grid_planes();
// fn(first, n) for every chunk of `count` planes that one launch carries in its grid
template <class Fn>
void for_plane_chunks(int count, Fn fn)
{
    const int step = max_grid_planes();
    for (int k = 0; k < count; k += step) fn(k, count - k < step ? count - k : step);
}
int launch_repack(gme_ctx* ctx, hipStream_t stream, const uint8_t* src, int count, int H, int W, uint8_t* dst, int pitch,
                  long long dst_stride);
int launch_pyrdown(gme_ctx* ctx, const Plane& src, const Plane& dst);
int launch_first_params(gme_ctx* ctx, const int32_t* dense, int pairs, int n_blocks, float* params0);
int launch_project_first(gme_ctx* ctx, const float* params0, int pairs, double* params_in);
// model field, mask, threshold and sums of one level's fit, into f: order 1 -> f.sums [P][15] (params [P][6]), order 2 ->
// f.sums2 [P][27] (params of pstride doubles per pair: 12, or 6 for the affine layout with zero second-order terms)
int launch_fit_level(gme_ctx* ctx, const FitLevelBuf& f, int order, int pairs, const double* params, int pstride, int drop,
                     int level_H, int level_W);
int launch_affine_field(gme_ctx* ctx, const double* params, int pairs, int h, int w, int16_t* out);
// order-2 field, params [P][12]; exactly one of out16 / out32 is non-null
int launch_model2_field(gme_ctx* ctx, const double* params, int pairs, int h, int w, int16_t* out16, int32_t* out32);
int launch_solve3(gme_ctx* ctx, const double* sums, int pairs, int project, int h, int w, double* params_out, int32_t* flags, int flag_bit);
// order-2 counterpart: sums [P][27] of one of the GME_MODEL_* second-order models -> params_out [P][12] (projected if
// `project`), flags |= 4 (singular), 8 (ill-conditioned), flag_bit (a displacement of the h x w field near a rounding tie)
int launch_solve_model2(gme_ctx* ctx, const double* sums, int model, int pairs, int project, int h, int w, double* params_out,
                        int32_t* flags, int flag_bit);
int launch_mv_summary(gme_ctx* ctx, const int32_t* mf, int pairs, int n_blocks, double* rows);
int launch_compensate(gme_ctx* ctx, const uint8_t* frames, int64_t frame_stride, int pairs, int H,
                      int W, int pitch, const int32_t* mf32, const double* params, int h, int w,
                      uint8_t* out, int64_t out_stride, int out_pitch, const uint8_t* cur,
                      int64_t cur_stride, unsigned long long* sse);
int launch_sse(gme_ctx* ctx, const uint8_t* a, int64_t a_stride, int a_pitch, const uint8_t* b,
               int64_t b_stride, int b_pitch, int pairs, int H, int W, unsigned long long* sse);

// ---- synth_kernels.hip ------------------------------------------------------
int launch_synth_canvas(gme_ctx* ctx, uint64_t seed, uint8_t* canvas);
int launch_synth_frames(gme_ctx* ctx, uint64_t seed, int t0, const uint8_t* canvas, const Plane& dst);

// ---- gme_api.hip: what the C ABI of the core lends to the entry points of the passes (gme_api_passes.hip, gme_api_frames.hip) ----
// The launchers, argument rules and state of those passes are declared in gme_passes.h, not here.

// Every entry point that touches a context holds its mutex for the whole call: the context owns ONE
// stream and ONE growable scratch buffer, and ctypes releases the GIL, so two Python threads inside
// the module-level bbme/motion/utils functions (one shared default context) would otherwise carve
// the same scratch offsets or free the buffer under each other's kernels.  Calls on one context
// serialise; use one context per thread (sequence.ShardedSequence does) for concurrency.
#define GME_ENTER(c)                                                  \
    GME_REQUIRE((c) != nullptr, GME_ERR_ARG, "null context");         \
    std::lock_guard<std::mutex> gme_lock__((c)->mu);                  \
    GME_HIP_TRY(hipSetDevice((c)->device))

// The scratch of a single-pair call: take() sub-buffers (256-byte aligned, in order), then commit() gets the block from the
// context and sets every pointer handed to take().
struct Carver {
    void* var[8];
    size_t at[8], off = 0;
    int n = 0;
    template <class T> void take(T** v, size_t count)
    {
        var[n] = v; at[n++] = off;
        off = (off + count * sizeof(T) + 255) & ~(size_t)255;
    }
    // a plane of plane_shape(); guard: with the guard row behind it
    void take(Plane* v, bool guard) { take(&v->ptr, v->bytes() + (guard ? v->pitch : 0)); }
    int commit(gme_ctx* ctx)
    {
        void* base = nullptr;
        const int rc = ctx_scratch(ctx, off, &base);
        if (rc) return rc;
        for (int i = 0; i < n; ++i) {
            void* ptr = (uint8_t*)base + at[i];
            memcpy(var[i], &ptr, sizeof(ptr));                 // whatever T, *var[i] is an object pointer
        }
        return GME_OK;
    }
};

// a host image with rows `stride` bytes apart into plane 0 of v, queued on the context's stream
inline hipError_t put_plane(gme_ctx* ctx, const Plane& v, const uint8_t* host, int stride)
{
    return hipMemcpy2DAsync(v.ptr, v.pitch, host, stride, v.W, v.H, hipMemcpyHostToDevice, ctx->stream);
}

// host images with rows `stride` bytes apart into planes 0, 1, ... of a stack, queued on the context's stream
inline int put_planes(gme_ctx* ctx, const Plane& st, std::initializer_list<const uint8_t*> host, int stride)
{
    int k = 0;
    for (const uint8_t* image : host) {
        Plane one = st;
        one.ptr = st.at(k++);
        GME_HIP_TRY(put_plane(ctx, one, image, stride));
    }
    return GME_OK;
}

// planes first .. first + count - 1 of a stack into out[count][H][W] (tight), queued on the context's stream
inline int read_planes(gme_ctx* ctx, const Plane& p, int first, int count, uint8_t* out)
{
    for (int k = 0; k < count; ++k)
        GME_HIP_TRY(hipMemcpy2DAsync(out + (size_t)k * p.H * p.W, p.W, p.at(first + k), p.pitch, p.W, p.H, hipMemcpyDeviceToHost,
                                     ctx->stream));
    return GME_OK;
}

// the pointer and shape rules of a single-pair call `who` on host images; `pointers`: none of those it needs is null
inline int oneshot_check(const char* who, bool pointers, int H, int W, int stride)
{
    GME_REQUIRE(pointers, GME_ERR_ARG, "%s: null pointer", who);
    GME_REQUIRE(H > 0 && W > 0 && stride >= W, GME_ERR_ARG, "%s: bad shape H=%d W=%d stride=%d", who, H, W, stride);
    return GME_OK;
}

// Defined in gme_api.hip, where each is described:
int ctx_finish(gme_ctx* ctx);                              // wait for the stream and report a tripped in-kernel guard
// the search of the pairs (first + k, first + k + fd), k < pairs, of a plane stack into mf
BbmeJob bbme_job(const Plane& p, int first, int fd, int pairs, int bs, int sw, int procedure, int pnorm, int32_t* mf);
// launch_bbme of a job over the resident frames of one level whose first "current" plane is frame first_cur of the level
int seq_launch_bbme_from(gme_seq* s, int level, int first_cur, BbmeJob job);
int seq_levels(gme_seq* s);                                // the pyramid planes, sized for the sequence ...
int seq_pyramids(gme_seq* s);                              // ... and their contents, unless they are current
// the compensated planes (gme_seq::comp) for a writer of `pairs` planes, which marks them with comp_wrote once it is queued
int ensure_comp(gme_seq* s, int fd, int pairs);
void comp_wrote(gme_seq* s, int pairs);
void seq_field_replaced(gme_seq* s);                       // every writer of gme_seq::mv calls it: ends what was derived from the field

// Defined in gme_api_passes.hip, the only four calls the core makes into the passes: their state for a new sequence (null: out
// of memory) and its end, and the two places where the results they keep end (seq_field_replaced and, with new frame data or
// another frame count, seq_frames_changed; the second ends what the first ends, too).
SeqPasses* passes_create();
void passes_destroy(SeqPasses* p);
void passes_field_replaced(SeqPasses* p);
void passes_frames_changed(SeqPasses* p);
