// Internal declarations shared by the translation units of libgme_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
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
    std::mutex mu;                // held by every C-ABI entry point for the whole call (gme_api.hip: GME_ENTER)
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
    DevBuf<uint8_t> direct;       // gme_direct.hip: per-pair refinement state, histograms, slabs and parameters
    // stabilization (gme_stab.hip): the warped frames (N_cap, allocated by the first gme_seq_warp_frames), which of them a
    // warp has written, and N_cap rows of parameters and counts
    PlaneBuf warped;
    WrittenFrames warped_written;
    DevBuf<double> warp_params;          // [N_cap][8]
    DevBuf<unsigned long long> warp_counts;      // [N_cap] valid samples, or squared errors of gme_seq_frame_sse
    // background mosaic (gme_mosaic.hip): sprite and sample counts [Hc][pitch] of the last gme_seq_mosaic, the masks of
    // gme_seq_moving_masks (N_cap planes, allocated by its first call) with which of them were written, and N_cap rows of
    // parameters, usable flags and known / moving counts
    DevBuf<uint8_t> mosaic_sprite;       // both hold the same number of pixels
    DevBuf<uint16_t> mosaic_count;
    int mosaic_Hc = 0, mosaic_Wc = 0, mosaic_pitch = 0;
    bool mosaic_valid = false;
    PlaneBuf masks;
    WrittenFrames masks_written;
    DevBuf<double> mosaic_params;        // [N_cap][8]
    DevBuf<uint8_t> mosaic_usable;       // [N_cap]
    DevBuf<unsigned long long> mosaic_counts;    // [2][N_cap] known, moving
    // Result lifetimes of the block-field passes below, in one place (gme_api.hip): seq_field_replaced ends what was derived from
    // `mv`, and every writer of `mv` calls it; seq_frames_changed (new frame data, another frame count) calls it too and then ends
    // the results that keep fields of their own.
    // quarter-pel refinement (bbme_subpel.hip): the refined field and its costs of the last gme_seq_subpel, allocated by
    // its first call; valid until seq_field_replaced
    DevBuf<int32_t> qmv;                 // [P][h][w][2], quarter units
    DevBuf<long long> qcost;             // [P][h][w]
    bool qmv_valid = false;
    // hierarchical search (bbme_hier.hip): fields of the levels above the frame and the costs of every level of the last
    // gme_seq_hier (its level-2 field is `mv`), allocated by its first call; valid until seq_field_replaced
    DevBuf<int32_t> hier_mv[2];          // [P][h][w][2] of levels 0 and 1
    DevBuf<long long> hier_cost[3];      // [P][h][w]
    int hier_levels = 0;                 // levels the last gme_seq_hier used
    bool hier_valid = false;
    // variable-block-size tree (bbme_vbs.hip): leaf field, depth map and root costs of the last gme_seq_vbs on `mv`, allocated
    // by its first call; valid until seq_field_replaced
    DevBuf<int32_t> vbs_leaf;            // [P][h << D][w << D][2]
    DevBuf<uint8_t> vbs_dmap;            // [P][h << D][w << D]
    DevBuf<long long> vbs_cost;          // [P][h][w]
    int vbs_depth = 0;                   // D of the last gme_seq_vbs
    bool vbs_valid = false;
    // bidirectional prediction (bbme_bipred.hip): both fields of gme_seq_bipred's own searches, the modes, the vector pairs and
    // the costs of its T = N - 2 fd targets, allocated by its first call; valid until seq_frames_changed.  No other call reads or
    // writes them, and gme_seq_bipred writes nothing else of the sequence.
    DevBuf<int32_t> bp_f0, bp_f1;        // [T][h][w][2]
    DevBuf<uint8_t> bp_mode;             // [T][h][w]
    DevBuf<int32_t> bp_v0, bp_v1;        // [T][h][w][2]
    DevBuf<long long> bp_cost;           // [T][h][w]
    DevBuf<long long> bp_costs;          // [T][h][w][3]
    int bp_targets = 0, bp_h = 0, bp_w = 0, bp_fd = 0, bp_bs = 0;
    bool bp_valid = false;
    // global motion compensation (bbme_gmc.hip): the field of gme_seq_gmc's own search, the warps it was given with their usable
    // flags, the modes and the costs of its P = N - fd pairs, allocated by its first call; valid until seq_frames_changed.  No other
    // call reads or writes them, and gme_seq_gmc writes nothing else of the sequence.
    DevBuf<int32_t> gm_f;                // [P][h][w][2]
    DevBuf<double> gm_h;                 // [P][8]
    DevBuf<uint8_t> gm_usable;           // [P]
    DevBuf<uint8_t> gm_mode;             // [P][h][w]
    DevBuf<long long> gm_cost;           // [P][h][w]
    DevBuf<long long> gm_costs;          // [P][h][w][2]
    int gm_pairs = 0, gm_h_blocks = 0, gm_w_blocks = 0, gm_fd = 0, gm_bs = 0;
    bool gm_valid = false;
    // vector propagation (bbme_prop.hip): the two fields the rounds of gme_seq_prop alternate between (the last one is copied
    // into `mv`), the camera field it was given, and the costs and sources of the last round, allocated by its first call;
    // valid until seq_field_replaced
    DevBuf<int32_t> prop_work[2];        // [P][h][w][2]
    DevBuf<int32_t> prop_g;              // [P][h][w][2]
    DevBuf<long long> prop_cost;         // [P][h][w]
    DevBuf<uint8_t> prop_source;         // [P][h][w]
    bool prop_valid = false;
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

// ---- gme_direct.hip: direct projective refinement ---------------------------------------------
// device blocks of the sequence's workspace for `pairs` pairs: in[P][8] (parameters the calls below read), out[P][8],
// flags[P] (refinement results), eval[P][48] = threshold, n_valid, n_in, cost, sums[44] (gme_seq_direct_eval)
struct DirectIo {
    double *in = nullptr, *out = nullptr, *eval = nullptr;
    int32_t* flags = nullptr;
};
int direct_io(gme_seq* s, int pairs, DirectIo* io);
// the whole refinement of in[] (full-resolution start) into out[] / flags[], every launch queued, no wait
int launch_direct_refine(gme_seq* s, int fd, int pairs, double outlier_fraction, int max_iters);
// one evaluation of in[] (level-`level` coordinates) with a fresh threshold into eval[]
int launch_direct_eval(gme_seq* s, int fd, int level, int pairs, double outlier_fraction);
// compensation of every pair under params[P][8] (device) into s->comp, squared errors into s->sse
int launch_compensate_proj(gme_seq* s, int fd, int pairs, const double* params);

// ---- gme_stab.hip: video stabilization -------------------------------------------------------
// frames first .. first + count - 1 of src warped by params[count][8] (device; border 0 constant fill, 1 replicate) into the
// same frames of dst, in-frame samples per frame into valid[count] (device)
int launch_warp_frames(gme_ctx* ctx, const Plane& src, const Plane& dst, int first, int count, const double* params, int border,
                       int fill, unsigned long long* valid);
// sse[k] = sum (p[first + k + 1] - p[first + k])^2, k < count (device)
int launch_frame_sse(gme_ctx* ctx, const Plane& p, int first, int count, unsigned long long* sse);

// ---- gme_stab_fill.hip: full-frame stabilization ----------------------------------------------
// output frames 0 .. count - 1 of dst, each pixel from the first of its frame's n_cand candidates (sources[count][n_cand]
// absolute frames of src or -1, params[count][n_cand][8]; device) whose sample point lies in its frame, the border rule on
// candidate 0 elsewhere; who (same geometry as dst; no memory: not wanted) the winning candidate or 255 per pixel;
// valid / filled [count] (device) the pixels won by candidate 0 / by a later one.  The caller has checked the indices.
int launch_warp_fill(gme_ctx* ctx, const Plane& src, const Plane& dst, const Plane& who, int count, int n_cand, const int* sources,
                     const double* params, int border, int fill, unsigned long long* valid, unsigned long long* filled);

// ---- gme_mosaic.hip: background mosaic and moving-object masks --------------------------------
// sprite / cnt [Hc][out_pitch] = lower median / number of the in-frame samples of frames first .. first + count - 1 of src at
// every canvas pixel (fill where there is none); G[count][8] and usable[count] on the device; cull 0 samples every frame
// at every pixel
int launch_mosaic_median(gme_ctx* ctx, const Plane& src, int first, int count, const double* G, const uint8_t* usable, int ox,
                         int oy, int Hc, int Wc, int fill, int cull, uint8_t* sprite, uint16_t* cnt, int out_pitch);
// masks of frames first .. first + count - 1 into dst, their known and moving pixels into known[count] and moving[count]
// (device, zeroed by the caller); A[count][8] and usable[count] on the device
int launch_moving_masks(gme_ctx* ctx, const Plane& src, const Plane& dst, int first, int count, const double* A,
                        const uint8_t* usable, const uint8_t* sprite, const uint16_t* cnt, int sp_pitch, int Hc, int Wc, int ox,
                        int oy, int threshold, int min_count, unsigned long long* known, unsigned long long* moving);

// ---- bbme_subpel.hip: quarter-pel refinement and compensation ------------------------------------
// qmf[pairs][H / bs][W / bs][2] (quarter units) and cost[pairs][H / bs][W / bs] = subpel.refine of the integer field mf of the
// same shape; pair k reads the planes prev + k * plane_stride and cur + k * plane_stride (device)
int launch_subpel_refine(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                         int pitch, int bs, int pnorm, int levels, const int32_t* mf, int32_t* qmf, long long* cost);
// out planes = subpel.compensate of the prev planes by qmf, sse[pairs] (device) = squared error of each against its cur plane
int launch_compensate_qpel(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                           int pitch, int bs, const int32_t* qmf, uint8_t* out, long long out_stride, int out_pitch,
                           unsigned long long* sse);

// ---- bbme_hier.hip: hierarchical block matching ----------------------------------------------------
// the argument rules of hier.py (GME_ERR_ARG)
int hier_check_args(const char* who, int bs, int cw, int radius, int pnorm, int levels);
// hier.search of `pairs` pairs: level[l] holds the planes of pyramid level l ([2] = the frames), pair k = planes first_prev + k
// and first_cur + k of each stack; mf[l] [pairs][hb][wb][2] and cost[l] [pairs][hb][wb] (device) for the levels
// l >= 3 - levels, hb = H / bs and wb = W / bs of level 2.  Names the kernel instance in the context's plan.
int launch_hier(gme_ctx* ctx, const Plane (&level)[3], int first_prev, int first_cur, int pairs, int bs, int cw, int radius,
                int pnorm, int levels, int32_t* const (&mf)[3], long long* const (&cost)[3]);

// ---- bbme_vbs.hip: variable-block-size motion -------------------------------------------------------
// the argument rules of vbs.py (GME_ERR_ARG)
int vbs_check_args(const char* who, int bs, int depth, int radius, int pnorm, int penalty);
// vbs.tree of `pairs` pairs on the field mf[pairs][H / bs][W / bs][2]: pair k reads the planes prev + k * plane_stride and
// cur + k * plane_stride; leaf [pairs][hb << depth][wb << depth][2], dmap of the same grid, cost [pairs][hb][wb] (device).
// Names the kernel instance in the context's plan.
int launch_vbs(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch,
               int bs, int depth, int radius, int pnorm, int penalty, const int32_t* mf, int32_t* leaf, uint8_t* dmap,
               long long* cost);
// out planes = subpel.compensate_integer of the prev planes by leaf[pairs][hg][wg][2] at cell size g, sse[pairs] (device) =
// squared error of each against its cur plane
int launch_compensate_vbs(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W,
                          int pitch, int g, int hg, int wg, const int32_t* leaf, uint8_t* out, long long out_stride, int out_pitch,
                          unsigned long long* sse);

// ---- bbme_bipred.hip: bidirectional block prediction ------------------------------------------------
// the argument rules of bipred.py (GME_ERR_ARG)
int bipred_check_args(const char* who, int bs, int radius, int rounds, int pnorm, int penalty);
// bipred.decide of `targets` triples on the fields f0, f1 [targets][H / bs][W / bs][2]: target k reads the planes
// past + k * plane_stride, mid + k * plane_stride and next + k * plane_stride; mode [targets][hb][wb], v0 and v1
// [targets][hb][wb][2], cost [targets][hb][wb], costs [targets][hb][wb][3] (device).  Names the kernel instance in the
// context's plan.
int launch_bipred(gme_ctx* ctx, const uint8_t* past, const uint8_t* mid, const uint8_t* next, long long plane_stride, int targets,
                  int H, int W, int pitch, int bs, int radius, int rounds, int pnorm, int penalty, const int32_t* f0, const int32_t* f1,
                  uint8_t* mode, int32_t* v0, int32_t* v1, long long* cost, long long* costs);
// out planes = bipred.predict of the past and next planes, sse[targets] (device) = squared error of each against its mid plane
int launch_predict_bipred(gme_ctx* ctx, const uint8_t* past, const uint8_t* mid, const uint8_t* next, long long plane_stride,
                          int targets, int H, int W, int pitch, int bs, const uint8_t* mode, const int32_t* v0, const int32_t* v1,
                          uint8_t* out, long long out_stride, int out_pitch, unsigned long long* sse);

// ---- bbme_gmc.hip: global motion compensation -------------------------------------------------------
// the argument rules of gmc.py (GME_ERR_ARG)
int gmc_check_args(const char* who, int bs, int pnorm, int penalty);
// gmc.usable of one warp of an H x W frame (host): the per-pair flag the two launchers take
bool gmc_usable(const double* h, int H, int W);
// gmc.decide of `pairs` pairs on the fields f [pairs][H / bs][W / bs][2] under the warps h [pairs][8] with their flags usable
// [pairs]: pair k reads the planes ref + k * plane_stride and cur + k * plane_stride; mode [pairs][hb][wb], cost [pairs][hb][wb],
// costs [pairs][hb][wb][2] (all device).  Names the kernel instance in the context's plan.
int launch_gmc(gme_ctx* ctx, const uint8_t* ref, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
               int pnorm, int penalty, const double* h, const uint8_t* usable, const int32_t* f, uint8_t* mode, long long* cost,
               long long* costs);
// out planes = gmc.predict of the ref planes, sse[pairs] (device) = squared error of each against its cur plane
int launch_predict_gmc(gme_ctx* ctx, const uint8_t* ref, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch,
                       int bs, const double* h, const uint8_t* usable, const uint8_t* mode, const int32_t* f, uint8_t* out,
                       long long out_stride, int out_pitch, unsigned long long* sse);

// ---- bbme_prop.hip: vector propagation search --------------------------------------------------------
// the argument rules of propagate.py (GME_ERR_ARG)
int prop_check_args(const char* who, int bs, int pnorm, int rounds, int steps);
// propagate.search of `pairs` pairs on the prior fields f [pairs][H / bs][W / bs][2]: pair k reads the planes
// prev + k * plane_stride and cur + k * plane_stride, the temporal field t[k + t_shift] (t null: none; neither where
// k + t_shift < 0) and the camera field g[k] (null: none).  The rounds alternate between work[0] and work[1] (each
// [pairs][hb][wb][2]) and only read f, so t may lie in it; *result is the one the last round wrote, cost [pairs][hb][wb] and
// source [pairs][hb][wb] are that round's (all device).  Names the kernel instance in the context's plan.
int launch_prop(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
                int pnorm, int rounds, int steps, const int32_t* f, const int32_t* t, int t_shift, const int32_t* g, int32_t* const work[2],
                long long* cost, uint8_t* source, int32_t** result);

// ---- bbme_interp.hip: motion-compensated frame interpolation -----------------------------------------
// the argument rules of interp.py for H x W frames (GME_ERR_ARG)
int interp_check_args(const char* who, int H, int W, int bs, int sw, int pnorm, int bias);
// interp.search of `pairs` pairs: pair k reads the planes past + k * plane_stride and next + k * plane_stride; mv
// [pairs][H / bs][W / bs][2], cost (J) and dist (D) [pairs][H / bs][W / bs] (device).  Names the kernel instance in the context's
// plan.
int launch_interp(gme_ctx* ctx, const uint8_t* past, const uint8_t* next, long long plane_stride, int pairs, int H, int W, int pitch,
                  int bs, int sw, int pnorm, int bias, int32_t* mv, long long* cost, long long* dist);
// out planes = interp.interpolate of the past and next planes by mv, sse[pairs] (device) = squared error of each against its cur
// plane (the true middle frame; any plane of the stack where there is none)
int launch_interp_frame(gme_ctx* ctx, const uint8_t* past, const uint8_t* next, const uint8_t* cur, long long plane_stride, int pairs,
                        int H, int W, int pitch, int bs, const int32_t* mv, uint8_t* out, long long out_stride, int out_pitch,
                        unsigned long long* sse);

// ---- bbme_retime.hip: frame interpolation at any phase ------------------------------------------------
// the argument rules of retime.py for H x W frames (GME_ERR_ARG), and retime.check_phase: n / d reduced in place
int retime_check_args(const char* who, int H, int W, int bs, int sw, int pnorm, int bias);
int retime_check_phase(const char* who, int* n, int* d);
// The phase table: one row of retime_row_ints() int32 per output, written on the host by retime_row for the output whose `past`
// is plane `plane` of the stack (`next` the plane behind it) at the reduced phase n / d -> the LDS a wave of that output needs
int retime_row_ints();
int retime_row(int32_t* row, int plane, int n, int d, int bs, int sw);
// retime.search of `outputs` outputs under their table rows (device; wave_lds: the largest retime_row of them); mv
// [outputs][H / bs][W / bs][2], cost (J) and dist (D) [outputs][H / bs][W / bs] (device).  Names the kernel instance in the
// context's plan.
int launch_retime(gme_ctx* ctx, const uint8_t* frames, long long plane_stride, int outputs, int H, int W, int pitch, int bs, int sw,
                  int pnorm, int bias, const int32_t* table, int wave_lds, int32_t* mv, long long* cost, long long* dist);
// out planes = retime.interpolate of each output's planes by mv, sse[outputs] (device) = squared error of each against its cur
// plane (cur + k * cur_stride: the true frame; any plane where there is none)
int launch_retime_frame(gme_ctx* ctx, const uint8_t* frames, long long plane_stride, int outputs, int H, int W, int pitch, int bs,
                        const int32_t* table, const int32_t* mv, const uint8_t* cur, long long cur_stride, uint8_t* out,
                        long long out_stride, int out_pitch, unsigned long long* sse);

// ---- bbme_obmc.hip: overlapped block motion compensation ---------------------------------------------
// the argument rules of obmc.py for H x W frames (GME_ERR_ARG)
int obmc_check_args(const char* who, int H, int W, int bs, int unit);
// out planes = obmc.compensate of the prev planes by field [pairs][H / bs][W / bs][2] in units of unit / 4 pixels (4: whole
// pixels, 1: quarter pixels), sse[pairs] (device) = squared error of each against its cur plane.  Names the kernel in the context's
// plan.  negate: by the negated field, for a field anchored at the predicted frame (denoise.predict).
int launch_obmc(gme_ctx* ctx, const uint8_t* prev, const uint8_t* cur, long long plane_stride, int pairs, int H, int W, int pitch, int bs,
                const int32_t* field, int unit, uint8_t* out, long long out_stride, int out_pitch, unsigned long long* sse,
                bool negate = false);

// ---- bbme_denoise.hip: motion-compensated temporal denoising -----------------------------------------
// the argument rules of denoise.py (GME_ERR_ARG)
int denoise_check_args(const char* who, int R, int strength);
// out planes = denoise.blend of the cur planes (cur_stride apart) with R prediction planes each: target k reads prediction r at
// preds + k * plane_stride + r * pred_stride; sse[targets] (device) = squared difference of each output against its truth plane
// (truth_stride apart).  Every input plane has the row pitch `pitch`.  Names the kernel in the context's plan; GME_OK for zero
// targets.
int launch_denoise(gme_ctx* ctx, const uint8_t* cur, long long cur_stride, const uint8_t* preds, long long pred_stride, long long plane_stride,
                   int targets, int R, int H, int W, int pitch, int strength, const uint8_t* truth, long long truth_stride, uint8_t* out,
                   long long out_stride, int out_pitch, unsigned long long* sse);

// ---- synth_kernels.hip ------------------------------------------------------
int launch_synth_canvas(gme_ctx* ctx, uint64_t seed, uint8_t* canvas);
int launch_synth_frames(gme_ctx* ctx, uint64_t seed, int t0, const uint8_t* canvas, const Plane& dst);
