// emi_ctx.hpp -- the context behind emi_ctx_t and what every part of the C ABI's implementation (emi_api*.hip) and the two drivers
// that take a context (emi_ipm_solve.hip, emi_ipm_ladder.hip) need of it.  Private to csrc/: not part of include/, and no run-time
// compiled model program sees it.  A context owns the HIP stream, the mesh constants on the device (w, node times, diag(D), D), the
// path/track tables and scratch for the cost partials.  Trajectory and result arrays belong to the caller (device pointers), except
// in the *_host forms, which stage through context-owned buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "emi355x.h"
#include "emi_device_array.hpp"
#include "emi_keep_record.hpp"
#include "emi_kernels.hpp"

namespace emi_api {

using DevBuf = emi::DeviceArray<unsigned char>;    // untyped bytes: the context's real type is chosen at run time (f32 / f64)

// the events of one profiled launch.  Sequential form: E0 | node | E1 | defect | E2; overlapped forms: E0 fork, E1 join, the MFMA
// kernel K0..K1 (its stream), the node kernel K2..K3 (its stream)
enum ProfMark { E0, E1, E2, K0, K1, K2, K3, PROF_MARKS };
struct ProfEvents {
    hipEvent_t ev[PROF_MARKS] = {};     // null until created (next_prof_record); the context's destructor destroys what is not
    bool has_node = false, has_defect = false, fused = false;
    int level = 0;          // 1: every bracket; 2: the defect (MFMA) kernel only; 3: the node kernel only; -1: one bracket K0..K1, the pass kernel
};

// The work tables of the one-launch pass on the device (emi_pass_work.hpp), by key: batch, mesh and plan stay the same from call to
// call, so a steady-state emi_eval_dev only compares keys.  A few slots, because the pieces of a large batch (and its remainder) and
// the rungs of a ladder are separate launches with tables of their own; the least recently used one gives way.  A slot owns the
// device copy AND the host copy the asynchronous upload reads from, which therefore outlives that copy.
struct PassWorkCache {
    static constexpr int SLOTS = 8;
    struct Slot {
        bool used = false;
        emi::PassWorkKey key;
        std::vector<emi::PassWork> host;
        emi::DeviceArray<emi::PassWork> dev;
        unsigned long long stamp = 0;
    };
    Slot slot[SLOTS];
    unsigned long long clock = 0;
    unsigned long long uploads = 0;     // tables built and uploaded so far (emi_debug_pass_work_uploads)
};

}  // namespace emi_api
using emi_api::DevBuf, emi_api::ProfEvents;

struct emi_ctx_s {
    int device = 0;
    bool f32 = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t stream2 = nullptr;          // the node kernel runs here while the MFMA defect kernel runs on `stream`
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;
    // "cu_split" option: the two kernels of the overlapped pass on disjoint CU sets (CU-masked streams)
    int cu_split = 0;                       // CUs given to the MFMA defect kernel; 0 = both kernels share every CU
    hipStream_t s_mfma = nullptr, s_node = nullptr;
    std::string err;
    std::string last_defect_kernel;

    // mesh
    int M = 0;
    double t0 = 0, tf = 0;
    DevBuf d_w, d_t, d_Ddiag, d_D, d_De, d_Do;
    bool symmetric = false;   // D is exactly centro-antisymmetric and M is even: De/Do are valid
    DevBuf d_Dfrag;           // De / Do in the MFMA role's fragment order (emi::operator_fragments), as large as the two together
    bool has_dfrag = false;   // ... valid: a symmetric D on a mesh of whole 128-node tiles (rebuilt by every emi_set_mesh)
    bool points_only = false; // emi_set_mesh(D = NULL): abscissae without a differentiation matrix
    int allow_fused = 1;          // "overlap" option: even/odd MFMA defect kernel || node kernel on two streams
    int sym_ct = 0;               // MFMA kernel variant (emi_symdefect.hip): 0 = chosen from the batch, 3 = LDS-DMA ring, 5..8 state-split ring, 1/2 = register-staged
    int sym_order = 1;
    int sym_ablate = 0;
    int small_rows = 24;          // "small_rows": up to this many rows B*ns the skinny defect kernel replaces the MFMA ones
                                  // (measured at 1024 nodes, 6 states: B = 1 / 2 / 4: 21 / 29 / 53 us per pass against 83 us)
    int overlap_mode = 0;         // 0: by batch size (3 below 192 tiles, else 2); 1: one stream, back to back; 2: two streams; 3: one launch
    int node_store = -1;          // cache policy of the node kernel's stores on the overlapped path: 0 plain, 1 sc1, 2 nt, -1 by size
    unsigned fused_attr_mask = 0;
    std::vector<double> h_tau, h_w;
    // model
    int model = -1, ns = 0, nc = 0, maximize = 0;
    double params[EMI_MAX_PARAMS] = {0};
    int nparams = 0;            // ... how many of them the model takes
    // per-instance parameter table (emi_set_model_params_batch): row b is the parameter set of instance b, in place of `params`.
    // While it is in force every kernel that evaluates the model runs in its tabled instantiation and the pass takes the sequential
    // route (has_param_table below).  Survives mesh, path table, tracks and stream; dropped by a new model and by another batch size
    int ptab_sets = 0;          // 0: none; else B
    DevBuf d_ptab;              // [B][EMI_MAX_PARAMS] in the context's real type, rows zero padded
    std::vector<double> h_ptab; // [B][nparams] as given (emi_get_model_params_batch)
    emi::KktWorkspace* kkt = nullptr;   // Newton-step workspace (emi_kkt_factor)
    std::vector<emi::KktWorkspace*> kkt_shard;  // one more per instance of the batch (emi_kkt_*_shard_dev), created on demand; apart from `kkt`
    int kkt_method = 1;                 // 1: Schur complement + Cholesky (falls back to 0 if not quasi-definite); 0: LU of K
    emi::RtcModel* rtc = nullptr;   // model == EMI_MODEL_SOURCE: code object compiled at emi_set_model_source
    // batch / path
    int B = 0;
    int np = 0, path_sets = 0, px = 0, py = 1;
    int np_model = 0;           // path rows computed by the model itself (emi_set_model_source npath)
    std::vector<int> pvars;     // node variables those rows depend on (PW of them): PW partials per traced row in VALS
    DevBuf d_path;
    int ntracks = 0, track_sets = 0;
    DevBuf d_trkx, d_trky;
    // waypoint tables of the tracks (emi_set_track_waypoints): what emi_tracks_from_waypoints_dev makes the centres of, on whatever
    // mesh the context is on.  Always doubles; independent of mesh, model and batch (only wp_ntracks = 0 drops them)
    int wp_ntracks = 0, wp_sets = 0, wp_ld = 0;
    emi::DeviceArray<double> d_wp;          // t | x | y, each [wp_sets][wp_ntracks][wp_ld]
    emi::DeviceArray<int> d_wp_cnt;         // [wp_sets][wp_ntracks] waypoints of each track (2 .. wp_ld)
    emi::DeviceArray<double> d_wp_nt;       // f32 contexts: the node times as doubles (d_t holds them rounded), rebuilt after emi_set_mesh
    bool wp_nt_dirty = true;
    DevBuf d_cost_part;
    DevBuf d_slab;              // partial sums of a split-K defect launch
    DevBuf d_tile_ticket;       // ... and the tickets of its in-kernel combine (zero between launches)
    DevBuf d_cost_part2;        // cost partials of the values-only pre-kernel of the overlapped f32 pass (discarded)
    DevBuf d_ticket;            // [B] arrival counters of the in-kernel COST finish (zeroed once, self-resetting)
    int cost_in_kernel = 1;     // "cost_in_kernel": the node kernel of the overlapped pass finishes COST itself (ticket), no emi_cost_finish_kernel
    int sym_nst = 3;            // "sym_nst": ring stages of the one-launch pass (3 or 4)
    int sym_hs = 0;             // "sym_hs": 2: K range of a tile in two halves inside the workgroup (512 threads); 1: undivided; 0: by batch size
    int sym_ctc = 0;            // "sym_ctc": 64-column sub-tiles per MFMA workgroup of the one-launch pass (1 or 2; 0: by batch size, plan_pass)
    int sym_bk = 0;             // "sym_bk": depth of a K tile of the one-launch pass (8 or 16; 0: by batch size, plan_pass)
    int sym_dop = 0;            // "sym_dop": where the MFMA role's De / Do fragments come from: 1 through the operand ring, 2 straight from L2
                                // (unsplit 16-deep form, SW 1 / 2); 0: by batch size, plan_pass
    int sym_res = 0;            // "sym_res": resident workgroups per CU the one-launch pass states: 2, or 3 (the De / Do from L2 forms only); 0: by
                                // batch size, plan_pass
    // delayed values (emi_set_delays): x_horizon - 1 delayed copies of every state and u_horizon of every control, appended to the
    // controls the node functions see: nc = nc_free + nch; W[d] = interpolation matrix of delay (d + 1) dt on this mesh
    int xh = 0, uh = 0, nch = 0;
    double delay_dt = 0.0;
    bool delay_dirty = true;    // W must be rebuilt (mesh or delays changed)
    DevBuf d_W;                 // [max(xh - 1, uh)][M][M]
    bool adjw_dirty = true;     // ... and so must its transposed stack for the adjoint pass (set wherever delay_dirty is)
    DevBuf d_adjWT;             // [M][max(xh - 1, uh) * ldt]: WT[n][s * ldt + j] = W[s][j][n], segments zero padded to the even ldt
    DevBuf d_adj_Gx;            // [B][ns+nc][M] gradient on the extended node variables (emi_lagr_grad_total_*)
    int adj_fold_tile = 0;      // "adj_fold_tile": tile shape of the fold product, 0 by size, 1 = 48 x 64, 2 = 96 x 128
    DevBuf d_uext;              // [B][nc][M]: the caller's controls, then the delayed values
    int f32_ring_wgs = 2;       // "f32_ring_wgs": workgroups of the fp32 ring kernel per CU (1: room for a node kernel's waves beside it, overlap_mode 2)
    int f32_ring = 1;           // "f32_ring": the fp32 MFMA defect kernel in its LDS-DMA ring form (0: register-staged operands, the round-2 form)
    int f32_one_launch = 0;     // "f32_one_launch": fp32 contexts take the one-launch pass (emi_pass_f32_kernel) by themselves where it applies.
                                // Off: measured at config 5 (256 instances, 4096 nodes) 1.12 - 1.26 ms per pass in every block order against
                                // 1.04 ms for the node kernel followed by the MFMA kernel (profiles/r03_notes.md section 6)
    int slice = 0;              // "slice" option: > 0: batches above 2 * slice instances are evaluated in pieces of this many; 0: one launch (see emi_eval_dev)
    int sym_ksplit = 0;         // "sym_ksplit" option: K slices per tile of the state-split ring kernel (0: by batch size)
    int sym_cpart = 0;          // "sym_cpart" option: column partitions of the tile order (0: by mesh size, -1: plain order, 1/2/4/8)
    int sym_gblk = 0, sym_cx = 0;   // "sym_gblk" / "sym_cx" options: grouped tile order, instance groups per super-block (0: off) and column tiles per block (0: 2)
    int pass_order = -1;        // "pass_order" option: one-launch pass, MFMA workgroups of an XCD first (1), interleaved with the node
                                // workgroups (0), or by batch size (-1: first for small batches)
    int sym_combine = 1;        // "sym_combine" option: 1 slices combined in-kernel by ticket, 0 by emi_symdefect_combine_kernel
    emi_api::PassWorkCache pass_work;   // work tables of the one-launch pass on the device, by key (freed with the context, after its streams drained)
    emi::KeepRecord keep;       // which VALS buffer holds this problem's model-invariant rows (EMI_EVAL_KEEP_INVARIANT)
    // host-form staging: named buffers of the evaluation and adjoint host forms, slots of every other one (HostStager)
    DevBuf s_X, s_U, s_RES, s_VALS, s_COST, s_LF, s_LC, s_H;
    std::vector<DevBuf> host_stage;
    // adjoint pass (emi_lagr_grad_* / emi_kkt_certificate_*): workspace grown on demand
    DevBuf d_adjDT;             // [M][ldt] transposed operator without its diagonal (emi_adjoint.hip), rebuilt after emi_set_mesh
    bool adj_dirty = true;
    DevBuf d_adj_pvars;         // pvars on the device ...
    std::vector<int> adj_pvars; // ... and what it holds
    DevBuf d_adj_c;             // [2][np] path-row bounds of the last certificate call
    DevBuf d_adj_G;             // G of a certificate call that does not return it
    DevBuf d_adj_op;            // [B][ns][M] operator term of the side-by-side form (large batches)
    DevBuf s_G, s_cert, s_zl, s_zu, s_Gdel;
    // relative local ODE error (emi_ode_error_*): the stacked operator [E | E' | D] of the mesh in force with rows of the even
    // length M + (M & 1), the point times and interval scales, the control bounds of the last call and the workspace
    bool ode_dirty = true;      // operator and times must be rebuilt (set wherever adj_dirty is)
    emi::DeviceArray<double> d_ode_op;      // [2 * 5 (M-1) + M][ldk]
    emi::DeviceArray<double> d_ode_tq;      // [5 (M-1)] times of the points, then [M-1] interval scales (tau_k+1 - tau_k) / 2 * h
    emi::DeviceArray<double> d_ode_ub;      // [2][nc]: ul, uu
    emi::DeviceArray<double> d_ode_ws;      // [B ns][2 * 5 (M-1) + M] | [B nc][5 (M-1)] | eta [B][ns][M-1]
    // ... of a context with delays (emi_ode_error_total_*): the stacked operators of the mesh and the delays in force, rows of the
    // same even length; the workspace above holds [B ns][(2 + max(xh-1, 0)) 5 (M-1) + M] | [B ncf][(1 + uh) 5 (M-1)] | eta then
    bool odel_dirty = true;     // the stacks must be rebuilt (set wherever ode_dirty or delay_dirty is)
    emi::DeviceArray<double> d_odel_ops;    // [E | E' | D | Edel(dt) .. Edel((xh-1) dt)]: the state rows' operator
    emi::DeviceArray<double> d_odel_opc;    // [E | Edel(dt) .. Edel(uh dt)]: the free controls'
    // node blocks of the Newton step (emi_kkt_blocks_*): the (variable, VALS entry) pairs of the path rows, the per-entry term
    // lists built from them (uploaded once per list) and the workspace of the kernels, grown on demand
    bool blk_rows_set = false;          // emi_kkt_blocks_rows was called (else: the layout's default for table rows)
    std::vector<int> blk_row_ptr, blk_var, blk_entry;
    std::vector<int> blk_key;           // what the uploaded term lists were built from ({} = nothing uploaded)
    emi::DeviceArray<int> blk_term_ptr, blk_term_row, blk_term_ea, blk_term_eb, blk_flag, blk_list, blk_nflag, blk_cnt;
    emi::DeviceArray<double> blk_tdelta, blk_tvec, blk_tworst;
    int blk_generic = 0;                // "blocks_generic": 1 = the run-time-nv assembly kernel also where a templated one exists
    // interior-point arithmetic (emi_ipm_*): the path-row lists by row and by variable (one array: rptr | rvar | rent | vptr | vrow |
    // vent), the row bounds as the kernels read them, the partials of the reducing kernels
    std::vector<int> ipm_key;           // what the uploaded lists were built from
    emi::DeviceArray<int> ipm_lists;
    int ipm_npairs = 0;
    std::vector<double> ipm_crow_h;     // [5][np]: cl, cu, cscale cl, cscale cu, cscale (what ipm_crow holds)
    emi::DeviceArray<double> ipm_crow, ipm_part;
    emi::IpmSolveWs* ipm_solve = nullptr;   // device arrays of the lock-step driver (emi_ipm_solve_shard_*), created at its first call
    emi::IpmLadderWs* ipm_ladder = nullptr; // ... and of the mesh ladder over it (emi_ipm_solve_ladder_*, emi_ipm_solve_refine_*)
    emi::StartGuessWs* start_guess = nullptr;   // ... and of the starts of the batch (emi_start_guess_*): grids, distances, paths
    bool path_has_track = false;            // the record table holds a row of kind EMI_PATH_TRACK
    // measurement
    hipEvent_t t_start = nullptr, t_stop = nullptr;
    int profile = 0;          // emi_profile_enable level (0 off)
    std::vector<ProfEvents> prof;
    size_t prof_used = 0;
    bool attr_set = false;

    // everything above that is a handle: streams drained and destroyed (the caller's own stream is only drained), then the events,
    // the run-time compiled model and the Newton-step workspace; the buffers free themselves after this body
    ~emi_ctx_s() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (ProfEvents& pe : prof)
            for (hipEvent_t e : pe.ev)
                if (e) (void)hipEventDestroy(e);
        for (hipStream_t s : {stream2, s_mfma, s_node})
            if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        for (hipEvent_t e : {ev_join2, ev_fork, ev_join, t_start, t_stop})
            if (e) (void)hipEventDestroy(e);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
        emi::rtc_destroy(rtc);
        emi::kkt_destroy(kkt);
        for (emi::KktWorkspace* w : kkt_shard) emi::kkt_destroy(w);
        emi::ipm_solve_destroy(ipm_solve);
        emi::ipm_ladder_destroy(ipm_ladder);
        emi::start_guess_destroy(start_guess);
    }
};

#define HIP_TRY(c, call)                                                                                                                  \
    do {                                                                                                                                  \
        hipError_t e_ = (call);                                                                                                           \
        if (e_ != hipSuccess) return emi_api::fail((c), EMI_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
// ... in a driver, whose messages name the entry point (`who`) instead of the source line
#define HIP_TRY_AS(c, who, call)                                                                                        \
    do {                                                                                                                \
        const hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess) return emi_api::fail((c), EMI_ERR_HIP, "%s: %s failed: %s", who, #call, hipGetErrorString(e_)); \
    } while (0)

// a step that returns an EMI_* status: anything but EMI_OK ends the calling function with it
#define EMI_TRY(call)              \
    do {                           \
        const int st_ = (call);    \
        if (st_) return st_;       \
    } while (0)

namespace emi_api {

// ---- defined in emi_api.hip; those that every pass goes through, here ----
int fail(emi_ctx_t c, int code, const char* fmt, ...);
inline int ensure(emi_ctx_t c, DevBuf& b, size_t bytes) {
    HIP_TRY(c, b.reserve(bytes));
    return EMI_OK;
}
// the tickets of the in-kernel combines are zero between launches (a kernel resets what it draws), so a buffer is zeroed when it
// is made and again whenever it grows (reserve keeps no contents), on the stream its next reader runs on
inline int ensure_zeroed(emi_ctx_t c, DevBuf& b, size_t bytes, hipStream_t s) {
    if (b.bytes() >= bytes) return EMI_OK;
    EMI_TRY(ensure(c, b, bytes));
    HIP_TRY(c, hipMemsetAsync(b.p, 0, bytes, s));
    return EMI_OK;
}
// host -> context buffer on the context's stream, complete on return (the source may be a local of the caller)
int upload_bytes(emi_ctx_t c, DevBuf& b, const void* src, size_t bytes);
// upload a host double array in the context's real type
int upload_real(emi_ctx_t c, DevBuf& b, const double* src, size_t n);
int download_real(emi_ctx_t c, double* dst, const void* dsrc, size_t n);
// the even / odd halves De, Do ([M/2][M/2] each) of a differentiation matrix; false (nothing written) unless M is even and D exactly
// centro-antisymmetric
bool even_odd_halves(int M, const double* D, std::vector<double>& De, std::vector<double>& Do);
// the staging buffer of VALS (host forms): a buffer that has to grow is a new, unwritten one -- also where the allocator hands
// back the old address, so the record is told before the old one goes
int ensure_vals_staging(emi_ctx_t c, size_t bytes);

inline int np_total(emi_ctx_t c) { return c->np + c->np_model; }     // rows of the record table, then the model's own (traced) rows
inline int nvals_of(emi_ctx_t c) { return c->ns * (c->ns + c->nc) + 2 * c->np + c->np_model * (int)c->pvars.size() + (c->ns + c->nc); }
inline int nres_of(emi_ctx_t c) { return c->ns + np_total(c); }
inline int nhess_of(emi_ctx_t c) { const int nv = c->ns + c->nc; return nv * (nv + 1) / 2; }
inline bool has_param_table(emi_ctx_t c) { return c->ptab_sets > 0; }
// the rows of the table from instance `first` on, as the tabled kernels take them (null without a table)
template <typename T> inline const T* param_rows(emi_ctx_t c, int first) {
    return has_param_table(c) ? (const T*)c->d_ptab.p + (size_t)first * EMI_MAX_PARAMS : nullptr;
}
inline int ready(emi_ctx_t c) {
    if (!c) return EMI_ERR_ARG;
    if (c->M <= 0) return fail(c, EMI_ERR_STATE, "emi_set_mesh has not been called");
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_set_model has not been called");
    if (c->B <= 0) return fail(c, EMI_ERR_STATE, "emi_set_batch has not been called");
    if (c->np > 0 && c->path_sets != 1 && c->path_sets != c->B)
        return fail(c, EMI_ERR_STATE, "path table has %d sets, batch is %d", c->path_sets, c->B);
    if (c->ntracks > 0 && c->track_sets != 1 && c->track_sets != c->B)
        return fail(c, EMI_ERR_STATE, "track table has %d sets, batch is %d", c->track_sets, c->B);
    if (c->ptab_sets > 0 && c->ptab_sets != c->B)
        return fail(c, EMI_ERR_STATE, "parameter table has %d sets, batch is %d", c->ptab_sets, c->B);
    return EMI_OK;
}

// Staging of one call of a host form that keeps no state between calls (the node blocks, the interior-point calls, the lock-step
// solve and the ladder): device twins of the caller's host arrays in the context's slots (host_stage), taken in the order of the
// place() calls -- a null array stays null --, copied asynchronously, the outputs copied back and the stream drained by finish().
// A slot holds whatever the last host form left in it.  That is why emi_eval_host, emi_hess_host and the adjoint host forms keep
// their named buffers (s_X ... s_Gdel): solve() calls the first two every iteration; s_VALS is the buffer whose address the
// KeepRecord tracks, and a slot that another host form may overwrite cannot hold invariant rows; kkt_certificate_host evaluates
// into the same s_RES / s_VALS that it then reads.
struct HostStager {
    emi_ctx_t c;
    size_t slot = 0;
    int status = EMI_OK;
    struct Out { void* host; void* dev; size_t bytes; };
    std::vector<Out> outs;
    explicit HostStager(emi_ctx_t c_) : c(c_) {}
    void* place(const void* host, size_t bytes, bool in, bool out);
    int finish();
};
// the _dev form of a staged call: an error ends the call only after the copies from the caller's arrays have drained
#define HOST_STAGED_TRY(s, call)                                                          \
    if ((s).status) { (void)hipStreamSynchronize((s).c->stream); return (s).status; }     \
    if (const int st_ = (call)) { (void)hipStreamSynchronize((s).c->stream); return st_; }

// ---- what one part calls in another ----
int ensure_delay_matrices(emi_ctx_t c);     // emi_api_pass.hip: W[d] of the delays on the mesh in force
int need_stream2(emi_ctx_t c);              // emi_api_pass.hip: the second stream of the two-stream forms
int path_row_list(emi_ctx_t c, const char* what, std::vector<int>& ptr, std::vector<int>& var, std::vector<int>& ent);     // emi_api_kkt.hip
int shard_check(emi_ctx_t c, const char* what);     // emi_api_kkt.hip: what the shard calls refuse
// emi_api_ipm.hip: an array kernel of emi_ipm.hip that has no entry point of its own (IPM_LAMC) on the context's row bounds
int ctx_ipm_launch(emi_ctx_t c, int what, const emi_ipm_bounds_t* bd, const void* dPar, emi::IpmArgs& a);

}  // namespace emi_api
