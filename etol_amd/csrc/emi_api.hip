// emi_api.hip -- device side of the C ABI declared in include/emi355x.h.
//
// A context owns: the HIP stream, the mesh constants on the device (w, node
// times, diag(D), D), the path/track tables, and scratch for the cost
// partials.  Trajectory and result arrays belong to the caller (device
// pointers), except in the *_host forms which stage through context-owned
// buffers.
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

namespace {

using DevBuf = emi::DeviceArray<unsigned char>;    // untyped bytes: the context's real type is chosen at run time (f32 / f64)

// the events of one profiled launch.  Sequential form: E0 | node | E1 | defect | E2; overlapped forms: E0 fork, E1 join, the MFMA
// kernel K0..K1 (its stream), the node kernel K2..K3 (its stream)
enum ProfMark { E0, E1, E2, K0, K1, K2, K3, PROF_MARKS };
struct ProfEvents {
    hipEvent_t ev[PROF_MARKS] = {};     // null until created (next_prof_record); the context's destructor destroys what is not
    bool has_node = false, has_defect = false, fused = false;
    int level = 0;          // 1: every bracket; 2: the defect (MFMA) kernel only; 3: the node kernel only; -1: one bracket K0..K1, the pass kernel
};

}  // namespace

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
    emi::KeepRecord keep;       // which VALS buffer holds this problem's model-invariant rows (EMI_EVAL_KEEP_INVARIANT)
    // host-form staging
    DevBuf s_X, s_U, s_RES, s_VALS, s_COST, s_LF, s_LC, s_H;
    // adjoint pass (emi_lagr_grad_* / emi_kkt_certificate_*): workspace grown on demand
    DevBuf d_adjDT;             // [M][ldt] transposed operator without its diagonal (emi_adjoint.hip), rebuilt after emi_set_mesh
    bool adj_dirty = true;
    DevBuf d_adj_pvars;         // pvars on the device ...
    std::vector<int> adj_pvars; // ... and what it holds
    DevBuf d_adj_c;             // [2][np] path-row bounds of the last certificate call
    DevBuf d_adj_G;             // G of a certificate call that does not return it
    DevBuf d_adj_op;            // [B][ns][M] operator term of the side-by-side form (large batches)
    DevBuf s_G, s_cert, s_zl, s_zu, s_Gdel;
    // node blocks of the Newton step (emi_kkt_blocks_*): the (variable, VALS entry) pairs of the path rows, the per-entry term
    // lists built from them (uploaded once per list) and the workspace of the kernels, grown on demand
    bool blk_rows_set = false;          // emi_kkt_blocks_rows was called (else: the layout's default for table rows)
    std::vector<int> blk_row_ptr, blk_var, blk_entry;
    std::vector<int> blk_key;           // what the uploaded term lists were built from ({} = nothing uploaded)
    emi::DeviceArray<int> blk_term_ptr, blk_term_row, blk_term_ea, blk_term_eb, blk_flag, blk_list, blk_nflag, blk_cnt;
    emi::DeviceArray<double> blk_tdelta, blk_tvec, blk_tworst;
    int blk_generic = 0;                // "blocks_generic": 1 = the run-time-nv assembly kernel also where a templated one exists
    DevBuf sb_H, sb_V, sb_Sg, sb_St, sb_fx, sb_Qx, sb_Q, sb_cnt, sb_node, sb_delta, sb_vec, sb_worst;   // host-form staging
    // interior-point arithmetic (emi_ipm_*): the path-row lists by row and by variable (one array: rptr | rvar | rent | vptr | vrow |
    // vent), the row bounds as the kernels read them, the partials of the reducing kernels, the staging of the host forms
    std::vector<int> ipm_key;           // what the uploaded lists were built from
    emi::DeviceArray<int> ipm_lists;
    int ipm_npairs = 0;
    std::vector<double> ipm_crow_h;     // [5][np]: cl, cu, cscale cl, cscale cu, cscale (what ipm_crow holds)
    emi::DeviceArray<double> ipm_crow, ipm_part;
    std::vector<DevBuf> ipm_stage;
    emi::IpmSolveWs* ipm_solve = nullptr;   // device arrays of the lock-step driver (emi_ipm_solve_shard_*), created at its first call
    emi::IpmLadderWs* ipm_ladder = nullptr; // ... and of the mesh ladder over it (emi_ipm_solve_ladder_*)
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
    }
};

namespace {

int fail(emi_ctx_t c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIP_TRY(c, call)                                                              \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess)                                                         \
            return fail((c), EMI_ERR_HIP, "%s failed: %s (%s:%d)", #call,             \
                        hipGetErrorString(e_), __FILE__, __LINE__);                   \
    } while (0)

// a step that returns an EMI_* status: anything but EMI_OK ends the calling function with it
#define EMI_TRY(call)              \
    do {                           \
        const int st_ = (call);    \
        if (st_) return st_;       \
    } while (0)

int ensure(emi_ctx_t c, DevBuf& b, size_t bytes) {
    HIP_TRY(c, b.reserve(bytes));
    return EMI_OK;
}

// the tickets of the in-kernel combines are zero between launches (a kernel resets what it draws), so a buffer is zeroed when it
// is made and again whenever it grows (reserve keeps no contents), on the stream its next reader runs on
int ensure_zeroed(emi_ctx_t c, DevBuf& b, size_t bytes, hipStream_t s) {
    if (b.bytes() >= bytes) return EMI_OK;
    EMI_TRY(ensure(c, b, bytes));
    HIP_TRY(c, hipMemsetAsync(b.p, 0, bytes, s));
    return EMI_OK;
}

// host -> context buffer on the context's stream, complete on return (the source may be a local of the caller)
int upload_bytes(emi_ctx_t c, DevBuf& b, const void* src, size_t bytes) {
    EMI_TRY(ensure(c, b, bytes));
    if (bytes == 0) return EMI_OK;
    HIP_TRY(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

// upload a host double array in the context's real type
int upload_real(emi_ctx_t c, DevBuf& b, const double* src, size_t n) {
    if (!c->f32) return upload_bytes(c, b, src, n * 8);
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = (float)src[i];
    return upload_bytes(c, b, tmp.data(), n * 4);
}

int download_real(emi_ctx_t c, double* dst, const void* dsrc, size_t n) {
    if (!dst || n == 0) return EMI_OK;
    std::vector<float> tmp(c->f32 ? n : 0);
    HIP_TRY(c, hipMemcpyAsync(c->f32 ? (void*)tmp.data() : (void*)dst, dsrc, n * (c->f32 ? 4 : 8), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < tmp.size(); ++i) dst[i] = tmp[i];
    return EMI_OK;
}

// the even/odd MFMA defect kernel beside the node kernel: needs an exactly centro-antisymmetric D
bool overlapped_path(emi_ctx_t c) {
    if (c->f32 || !c->allow_fused || !c->symmetric || c->M <= 0 || c->model < 0) return false;
    if (c->model == EMI_MODEL_SOURCE) return emi::rtc_has_symdefect(c->rtc) && c->M % 128 == 0;
    return emi::fused_supported(c->model, c->M, c->sym_ct);
}

// the one-launch pass in its small-batch form (SW = 1, plain stores) is available to this context by the default dispatch
bool pass_takes_small_batches(emi_ctx_t c, int B) {
    if (!overlapped_path(c) || (c->overlap_mode != 0 && c->overlap_mode != 3) || c->M % 128 != 0) return false;
    if (c->rtc) return emi::rtc_pass_supported(c->rtc, B, c->M, 1, 1, 0);
    const emi::SymPlan p = emi::plan_symdefect(c->ns, B, c->M, 7, 1, c->sym_cpart, c->sym_gblk, c->sym_cx);
    return emi::pass_supported(c->model, c->ns, B, c->M, p);
}

int np_total(emi_ctx_t c) { return c->np + c->np_model; }     // rows of the record table, then the model's own (traced) rows
int nvals_of(emi_ctx_t c) { return c->ns * (c->ns + c->nc) + 2 * c->np + c->np_model * (int)c->pvars.size() + (c->ns + c->nc); }
int nres_of(emi_ctx_t c) { return c->ns + np_total(c); }
int nhess_of(emi_ctx_t c) { const int nv = c->ns + c->nc; return nv * (nv + 1) / 2; }

// the staging buffer of VALS (host forms): a buffer that has to grow is a new, unwritten one -- also where the allocator hands
// back the old address, so the record is told before the old one goes
int ensure_vals_staging(emi_ctx_t c, size_t bytes) {
    if (c->s_VALS.bytes() < bytes) c->keep.written(c->s_VALS.p);
    return ensure(c, c->s_VALS, bytes);
}

int ready(emi_ctx_t c) {
    if (!c) return EMI_ERR_ARG;
    if (c->M <= 0) return fail(c, EMI_ERR_STATE, "emi_set_mesh has not been called");
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_set_model has not been called");
    if (c->B <= 0) return fail(c, EMI_ERR_STATE, "emi_set_batch has not been called");
    if (c->np > 0 && c->path_sets != 1 && c->path_sets != c->B)
        return fail(c, EMI_ERR_STATE, "path table has %d sets, batch is %d", c->path_sets, c->B);
    if (c->ntracks > 0 && c->track_sets != 1 && c->track_sets != c->B)
        return fail(c, EMI_ERR_STATE, "track table has %d sets, batch is %d", c->track_sets, c->B);
    return EMI_OK;
}

// Result-store flavour of the node role for a launch of B instances ("node_store" forces it).  Non-temporal once a pass writes
// about what the Infinity Cache holds (256 MB; RES + VALS above 230 MiB): measured on the one-launch pass, M = 1024
// (profiles/r03_mid_sweep.json): 256 instances (244 MiB) 0.0581 ms against 0.0720 with plain stores, 320: 0.0749 / 0.0973,
// 384: 0.0879 / 0.1050; 224 instances (214 MiB): plain 0.0557 / nt 0.0606, 128: 0.0338 / 0.0354.  (Round 2 switched at 300 MB of
// VALS, i.e. above 384 instances: the 256 .. 384 band ran 20 % slow.)
// Below that: write-through (sc1) stores for the built-in fp64 models since the end of round 4 -- plain stores leave a small pass's results
// dirty in L2 for the write-back at the end of the kernel, write-through streams them out while the kernel runs.  One box, ms per pass plain /
// sc1 (profiles/r04_mid_sweep_sc1_stores.jsonl): 1 instance 0.0125 / 0.0105, 16: 0.0149 / 0.0128, 32: 0.0176 / 0.0172, 64: 0.0209 / 0.0215,
// 80: 0.0233 / 0.0221, 112: 0.0290 / 0.0283, 128: 0.0291 / 0.0286, 144: 0.0305 / 0.0296, 192: 0.0434 / 0.0430, 224: 0.0532 / 0.0505.
// (Run-time compiled models hold a plain and a non-temporal instantiation only.)
int store_mode_for(emi_ctx_t c, int B) {
    if (c->node_store >= 0) return c->node_store;
    if ((size_t)B * (nvals_of(c) + nres_of(c)) * c->M * (c->f32 ? 4 : 8) > ((size_t)230 << 20)) return 2;
    // (17 .. 32 tiles -- 33 .. 64 instances at 1024 nodes, the two-slice band -- are the one place where plain stores stay ahead: 48 instances
    // 0.0197 / 0.0203, 64: 0.0209 / 0.0215)
    const int tiles16 = ((B + 15) / 16) * (c->M / 128);
    if (tiles16 > 16 && tiles16 <= 32) return 0;
    return (!c->rtc && !c->f32) ? 1 : 0;
}

// Everything the default dispatch decides about ONE launch of the evaluation pass as emi_pass_f64_kernel, in one place:
// plan_pass() is what choose_form / form_pass_f64 launch by and what emi_plan_pass reports (tests and tools read the policy from the
// library instead of restating it).
struct PassPlan {
    bool one_launch = false;    // the pass goes out as ONE launch (MFMA-role + node-role workgroups)
    emi::SymPlan sym;           // MFMA role: states per workgroup, K slices per tile, ring stages, tile order
    int tiles16 = 0;            // 16-instance x 128-node tiles of the launch (what the thresholds below are written in)
    int store_mode = 0;         // node role: 0 plain, 1 sc1, 2 non-temporal, 3 nt sc1
    int mfma_first = 0;         // block order (pass_role_of): 1 MFMA workgroups first, 0 evenly interleaved, >= 100: at that % of the even density
};

// The pass as ONE launch: MFMA-role and node-role workgroups in one grid, COST finished in-kernel -- since round 3 at EVERY
// batch size (round 2: two streams between 384 and 767 instances, which ran 20 - 25 % under the rest).  One box, interleaved
// rounds, M = 1024, ms per pass, best one-launch form against the round-2 choice (profiles/r03_mid_sweep.json): 256: 0.0581 /
// 0.0731, 320: 0.0749 / 0.0927, 384: 0.0879 / 0.1177 (two streams), 448: 0.1035 / 0.1038, 512: 0.1188 / 0.1162, 576: 0.1332 /
// 0.1777, 640: 0.146 / 0.155, 704: 0.160 / 0.181.
//   * SW (states per MFMA workgroup): 1 below 128 sixteen-instance x 128-node tiles (more workgroups than CUs), else 2;
//   * K slices per tile ("sym_ksplit"; partial sums combined in-kernel by ticket, in slice order).  By itself only where the MFMA
//     role has fewer workgroups than the chip has places for them, i.e. where a pass waits for one 64-tile dependency chain per
//     workgroup: 4 slices while that keeps the role within 256 workgroups, 2 within 512.  One box, M = 1024, ms per pass
//     unsplit / 2 / 4 slices (tools/mid_sweep.py, profiles/r03_notes.md section 7): B = 8: 0.0204 / 0.0148 / 0.0140,
//     16: 0.0235 / 0.0179 / 0.0155, 32: 0.0242 / 0.0190 / 0.0192, 64: 0.0257 / 0.0218 / 0.0261, 80: 0.0263 / 0.0249 / 0.0312,
//     96: 0.0288 / 0.0290 / 0.0407, 128: 0.0333 / 0.0387 / 0.0496 (from ~500 workgroups the split loses: three and more MFMA
//     waves per SIMD share the matrix pipe and the node role starts behind them);
//   * block order (pass_role_of): MFMA workgroups first below 208 tiles (their 64-tile dependency chains start at once, the
//     streaming workgroups fill in behind; since the end of round 4 only below 144 tiles: 1.5 x the even density from there, see
//     deep_band below), at 1.25 x the even density up to 384 tiles, at 1.1 x up to 768, evenly interleaved
//     from there (B >= 768, where "first" would hold the node role back: 0.288 against 0.222 at 1024).  (Round 2 measured
//     "first" against "interleaved" WITH PLAIN STORES at 256 instances and found interleaved ahead, 0.0727 / 0.0748; with
//     non-temporal stores "first" wins up to 448 instances: 256: 0.0581 against 0.0756 interleaved.  End of round 3, one box,
//     e9 node-evals/s at first / 1.25 x / 1.5 x / even: 448 instances 4.21 / 4.41 / 4.22 / 4.31, 512: 3.60 / 4.32 / 4.38 / 4.22,
//     640: 3.76 / 4.48 / 4.37 / 4.37, 704: 3.89 / 4.63 / 4.45 / 4.50; ms per pass at even / 1.1 x / 1.25 x: 768: 0.1747 /
//     0.1696 / 0.1760, 896: 0.1964 / 0.1959 / 0.2022, 1024: 0.2230 / 0.2200 / 0.2304, 1536: 0.3215 / 0.3219 / 0.3411,
//     2048: 0.4239 / 0.4227 / 0.4415);
//   * tile order: grouped (an XCD's MFMA tiles and node workgroups walk the same instance groups together) for launches of more
//     than 2048 instances in whole super-blocks, else column partitions by mesh size (plan_symdefect);
//   * stores: store_mode_for (non-temporal from about 256 instances).
// Every choice can be forced through emi_set_option (sym_ct, sym_ksplit, sym_cpart, sym_gblk, sym_cx, sym_nst, pass_order,
// node_store); a run-time compiled model holds two instantiations of the pass kernel -- SW = 1 with plain stores (small batches)
// and SW = 2 (1 for an odd number of states) with non-temporal stores (large ones) -- and is planned within those.
PassPlan plan_pass(emi_ctx_t c, int B, bool jac) {
    PassPlan p;
    p.tiles16 = ((B + 15) / 16) * (c->M / 128);
    p.store_mode = store_mode_for(c, B);
    const bool auto_mode = c->overlap_mode == 0;
    if (!((c->overlap_mode == 3 || auto_mode) && jac) || c->M % 128 != 0) return p;
    const bool auto_ct = auto_mode && (c->sym_ct == 0 || c->sym_ct == 4);
    const int gblk = (c->sym_gblk == 0 && c->sym_cpart == 0 && B > 2048 && B % 256 == 0) ? 2 : c->sym_gblk;
    const int gblk_first = (auto_ct || c->rtc) ? gblk : c->sym_gblk;
    int ct = c->sym_ct;                                  // 5 / 6 / 7 / 8 = SW NS / 2 / 1 / 3 (plan_symdefect)
    // Round 4: between 64 and 127 tiles (128 .. 255 instances at 1024 nodes: the shard of config 4) two states per workgroup with K
    // tiles of 16 -- half the barriers and counted waits of the MFMA role's dependency chain, which is what such a pass waits for.
    // One box, ms per pass, SW = 1 / 8-deep (the round-3 choice) against SW = 2 / 16-deep (profiles/r04_mid_sweep.jsonl): 128 instances
    // 0.0320 / 0.0300, 192: 0.0482 / 0.0442; at 64 instances the sliced SW = 1 form stays ahead (0.0210 / 0.0269), from 256 the 8-deep
    // SW = 2 form (0.0548 / 0.0617).
    // End of round 4 (profiles/r04_mid_sweep_small_72_120.jsonl, one box, ms per pass): the rule "2 K slices while the MFMA role stays within
    // 512 workgroups" held up to 80 instances, where the finer sweep found 0.0324 ms against 0.0208 at 64 and 0.0277 at 96.  SW = 1 with 2
    // slices / SW = 1 unsplit 8-deep / SW = 1 unsplit 16-deep / SW = 2 unsplit 16-deep: 72 instances 0.0323 / 0.0246 / 0.0231 / 0.0261, 80:
    // 0.0324 / 0.0248 / 0.0234 / 0.0267, 96: 0.0363 / 0.0278 / 0.0266 / 0.0278, 112: 0.0411 / 0.0338 / 0.0335 / 0.0291.  So: above 32 tiles
    // (64 instances) no slices any more; 33 .. 48 tiles one state per workgroup with 16-deep K tiles (deep_small), from 49 tiles two states
    // (deep_mid, which began at 64 tiles).
    const bool deep_base = auto_ct && !c->rtc && c->sym_bk == 0 && c->sym_ksplit == 0 && c->sym_nst == 3;
    // (both for an even number of states above two, where they were measured: the 6-state quadrotor)
    const bool deep_mid = deep_base && c->ns % 2 == 0 && c->ns > 2 && p.tiles16 >= 49 && p.tiles16 < 128;
    const bool deep_small = deep_base && c->ns % 2 == 0 && c->ns > 2 && p.tiles16 >= 33 && p.tiles16 < 49;
    if (c->rtc) ct = (p.store_mode == 2 && emi::rtc_pass_sw_large(c->rtc) == 2) ? 6 : 7;
    else if (auto_ct) ct = (p.tiles16 < 128 && !deep_mid) ? 7 : 6;
    emi::SymPlan plan = emi::plan_symdefect(c->ns, B, c->M, ct, 1, c->sym_cpart, gblk_first, c->sym_cx);
    if (plan.ring1) plan = emi::plan_symdefect(c->ns, B, c->M, 5, 1, c->sym_cpart, c->sym_gblk, c->sym_cx);
    int ks_want = c->sym_ksplit;
    if (ks_want == 0 && auto_ct && !deep_mid && !deep_small) ks_want = plan.tiles * 4 <= 256 ? 4 : (plan.tiles * 2 <= 512 ? 2 : 1);
    if (ks_want > 1) {
        const int ct_now = plan.sw == c->ns ? 5 : (plan.sw == 2 ? 6 : (plan.sw == 3 ? 8 : 7));
        plan = emi::plan_symdefect(c->ns, B, c->M, ct_now, ks_want, c->sym_cpart, c->rtc ? gblk : c->sym_gblk, c->sym_cx);
    } else {
        plan.ks = 1;
    }
    plan.nst = c->rtc ? 3 : c->sym_nst;
    // K tiles of 16 (built-in models, SW 1 or 2, three stages, unsplit): "sym_bk" 16 forces them
    // ... and between 208 and 767 tiles (416 .. 1535 instances, SW = 2 at 1.25 x / 1.1 x the even MFMA density): one box, ms per pass 8- /
    // 16-deep, 448 instances 0.1112 / 0.1018, 512: 0.1226 / 0.1151, 576: 0.1351 / 0.1277, 640: 0.1492 / 0.1431, 768: 0.1675 / 0.1649,
    // 896: 0.1921 / 0.1896, 1024: 0.2164 / 0.2143; not at 256 .. 384 instances (MFMA workgroups first: 320: 0.0752 / 0.0924) nor from 2048
    // (0.4147 / 0.4205; 4096 in the grouped order 1.081 / 1.175)
    // (up to 1024 tiles -- 2048 instances -- since the end of round 4: with the pass kernel's register allocation stated, 8- / 16-deep at 1536
    // instances 0.3204 / 0.3117, 1792: 0.3725 / 0.3611, 2048: 0.4441 / 0.4322, profiles/r04_mid_sweep_1280_2048.jsonl)
    const bool deep_large = auto_ct && !c->rtc && c->sym_bk == 0 && c->sym_nst == 3 && c->pass_order < 0 && p.tiles16 >= 208 && p.tiles16 <= 1024;
    // ... and between 144 and 207 tiles (288 .. 415 instances) TOGETHER with the MFMA workgroups at 1.5 x the even density instead of all
    // of them first: from ~300 instances the role's 3 x tiles workgroups no longer fit beside the node role (64 places per XCD), which then
    // starts a workgroup generation late.  End of round 4, one box, ms per pass, first + 8-deep (the choice until then) / 1.5 x + 16-deep:
    // 288 instances 0.0730 / 0.0699, 320: 0.0859 / 0.0754, 352: 0.1004 / 0.0820, 384: 0.1022 / 0.0875; 272: 0.0644 / 0.0698 (stays),
    // 416 (1.25 x + 16-deep already): 0.0946 / 0.0951 (profiles/r04_mid_sweep_band_288_416.jsonl)
    const bool deep_band = auto_ct && !c->rtc && c->sym_bk == 0 && c->sym_nst == 3 && c->pass_order < 0 && c->ns % 2 == 0 && c->ns > 2 &&
                           p.tiles16 >= 144 && p.tiles16 < 208;
    const int bk_want = c->sym_bk ? c->sym_bk : ((deep_mid || deep_small || deep_large || deep_band) ? 16 : 8);
    if (bk_want == 16 && !c->rtc && plan.ks == 1 && (plan.sw == 1 || plan.sw == 2) && plan.nst == 3) plan.bk = 16;
    // two column sub-tiles per MFMA workgroup ("sym_ctc" 2; built-in models, SW = 2, unsplit, three stages): the plan is made again with
    // the wider tiles (tile counts and tile order change with the column width)
    // By itself for launches of more than 2048 instances (the grouped tile order; inputs beyond the Infinity Cache, where every operand
    // read is an HBM read): one box, ms per pass one / two sub-tiles, 4096 instances 1.181 / 1.101, 16384: 4.407 / 4.044 (3.81e9 -> 4.15e9
    // node-evals/s) with column blocks of one 128-column tile; at 2048 instances 0.4736 / 0.4636, at 1024 and below the narrow form is ahead
    // (0.2222 / 0.2425: the wide workgroups need 60 KB of LDS and 160 registers) (profiles/r04_mid_sweep.jsonl)
    const bool wide_large = auto_ct && c->sym_ctc == 0 && B > 2048 && B % 256 == 0 && c->sym_cpart == 0;
    const int ctc_want = c->sym_ctc ? c->sym_ctc : (wide_large ? 2 : 1);
    if (ctc_want == 2 && !c->rtc && plan.ks == 1 && plan.sw == 2 && plan.nst == 3 && c->M % 256 == 0) {
        const int bk_keep = plan.bk;
        plan = emi::plan_symdefect(c->ns, B, c->M, 6, 1, c->sym_cpart, gblk_first, (wide_large && c->sym_cx == 0) ? 1 : c->sym_cx, bk_keep, 2);
        plan.ks = 1;
        plan.nst = 3;
        plan.bk = bk_keep;
    }
    // the K range in two halves inside the workgroup ("sym_hs" 2; built-in models, SW 1 or 2, unsplit, one sub-tile, three stages)
    const int hs_want = c->sym_hs ? c->sym_hs : 1;
    if (hs_want == 2 && !c->rtc && plan.ks == 1 && plan.ct == 1 && (plan.sw == 1 || plan.sw == 2) && plan.nst == 3 &&
        ((c->M / 2) / plan.bk) % 4 == 0)
        plan.hs = 2;
    p.sym = plan;
    p.mfma_first = c->pass_order >= 0 ? c->pass_order
                                      : (deep_band ? 150 : (p.tiles16 < 208 ? 1 : (p.tiles16 < 384 ? 125 : (p.tiles16 < 768 ? 110 : 0))));
    p.one_launch = c->rtc ? emi::rtc_pass_supported(c->rtc, B, c->M, plan.sw, plan.ks, p.store_mode)
                          : emi::pass_supported(c->model, c->ns, B, c->M, plan);
    return p;
}

// Large batches: the instances one launch of emi_eval_dev's default dispatch takes (0: the whole batch in one).  Round 2 cut
// everything above 2048 instances into 1024-instance launches (the two-stream form drifted apart on long launches); with the pass
// as ONE launch that buys nothing, and inputs of more than ~256 MB no longer stay in the Infinity Cache from one pass to the next,
// which is what really slows a large batch (B = 16384: 3.47e9 node-evals/s sliced or not, profiles/r03_notes.md).  Now: one launch
// over the whole batch in the GROUPED tile order: 4.10e9 /s at 16384 instances, 4.13e9 at 4096.  Pieces remain only where
// something forces them: the "slice" option (> 0: pieces of that many instances once B > 2 slice), the 32-bit operand offsets of
// the MFMA role (X of a launch below 4 GB), and a remainder that is not a multiple of 256 instances (the grouped order wants whole
// super-blocks on every XCD) as a second launch.
int plan_piece(emi_ctx_t c, int B) {
    const long long cap = ((0xFFFFFFFFLL / ((long long)c->ns * c->M * 8)) / 256) * 256;     // instances whose X stays below 4 GB
    int piece = 0;
    if (c->slice > 0) { if (B > 2 * c->slice) piece = c->slice; }
    else if (B > 2048) piece = (int)std::min<long long>(cap > 0 ? cap : 256, B - B % 256);
    return piece >= B ? 0 : piece;
}

// One launch of the evaluation pass: instances [first, first + B) of the context's batch.  The whole batch as a rule; pieces of it
// where plan_piece says so.  The context is not written to on the way: the batch of a launch is this argument.
struct Launch { int first, B; bool keep = false; };      // keep: the model-invariant VALS rows are in place already (emi_eval_dev decides)
// ... and its arrays (device memory, in the context's real type), already at the launch's first instance
struct PassIO { const void *X, *U; void *RES, *VALS, *COST; };

PassIO io_at(emi_ctx_t c, const PassIO& io, int first) {
    const size_t row = (size_t)first * c->M * (c->f32 ? 4 : 8);
    return PassIO{(const char*)io.X + row * c->ns, (const char*)io.U + row * c->nc, (char*)io.RES + row * nres_of(c),
                  io.VALS ? (char*)io.VALS + row * nvals_of(c) : nullptr, (char*)io.COST + (size_t)first * (c->f32 ? 4 : 8)};
}

template <typename T>
void fill_node_args(emi_ctx_t c, Launch L, emi::NodeArgs<T>& a, const PassIO& io) {
    a.X = (const T*)io.X;
    a.U = (const T*)io.U;
    a.RES = (T*)io.RES;
    a.VALS = (T*)io.VALS;
    a.cost_part = (T*)c->d_cost_part.p + (size_t)L.first * emi::node_chunks(c->M);
    a.cost = (T*)io.COST;
    a.cost_ticket = nullptr;
    a.w = (const T*)c->d_w.p;
    a.node_t = (const T*)c->d_t.p;
    a.Ddiag = (const T*)c->d_Ddiag.p;
    a.path = (const T*)c->d_path.p + (c->path_sets > 1 ? (size_t)L.first * c->np * EMI_PATH_REC : 0);
    a.track_x = (const T*)c->d_trkx.p + (c->track_sets > 1 ? (size_t)L.first * c->ntracks * c->M : 0);
    a.track_y = (const T*)c->d_trky.p + (c->track_sets > 1 ? (size_t)L.first * c->ntracks * c->M : 0);
    a.M = c->M;
    a.B = L.B;
    a.np = np_total(c);
    a.nres = nres_of(c);
    a.nvals = nvals_of(c);
    a.path_sets = c->path_sets;
    a.track_sets = c->track_sets;
    a.ntracks = c->ntracks;
    a.px = c->px;
    a.py = c->py;
    a.store_mode = store_mode_for(c, L.B);
    a.keep = L.keep ? 1 : 0;
    a.h = (T)((c->tf - c->t0) / 2.0);
    a.sgn = c->maximize ? T(-1) : T(1);
    for (int i = 0; i < EMI_MAX_PARAMS; ++i) a.P.p[i] = (T)c->params[i];
}

// Delayed values.  Row k of W(delay) holds the Lagrange basis of the LGL nodes at the node coordinate of max(t_k - delay, t0):
// what PSOPT's get_delayed_state / get_delayed_control hand ePSOPT::dae (reference src/ePSOPT/ePSOPT.cpp:231-248) -- the value
// at t - delay of the polynomial that interpolates the variable's node values ("Legendre" collocation: Lagrange interpolation).
// PSOPT 5.0.0 is not in the reference tree; times before t0 are CLAMPED to t0 here (the history of a delayed variable is its
// initial value), which is an assumption of this build, stated in include/emi355x.h and DESIGN.md section 5.
// Barycentric form with the LGL weights lambda_j ~ (-1)^j sqrt(w_j) (w_j = 2 / (N (N+1) P_N(tau_j)^2)).
void delay_matrix(const std::vector<double>& tau, const std::vector<double>& w, double t0, double tf, double delay, double* W) {
    const int M = (int)tau.size();
    std::vector<double> lam(M);
    for (int j = 0; j < M; ++j) lam[j] = ((j & 1) ? -1.0 : 1.0) * std::sqrt(w[j]);
    const double hh = (tf - t0) / 2.0;
    for (int k = 0; k < M; ++k) {
        double ts = t0 + hh * (tau[k] + 1.0) - delay;
        if (ts < t0) ts = t0;
        const double x = (ts - t0) / hh - 1.0;
        double* row = W + (size_t)k * M;
        int hit = -1;
        for (int j = 0; j < M; ++j)
            if (x == tau[j]) hit = j;
        if (ts <= t0) hit = 0;
        if (hit >= 0) {
            for (int j = 0; j < M; ++j) row[j] = j == hit ? 1.0 : 0.0;
            continue;
        }
        double den = 0.0;
        for (int j = 0; j < M; ++j) {
            row[j] = lam[j] / (x - tau[j]);
            den += row[j];
        }
        for (int j = 0; j < M; ++j) row[j] /= den;
    }
}

// W[d] = W((d + 1) dt) of the mesh in force on the device, for the evaluations and for the adjoint pass (whichever comes first)
int ensure_delay_matrices(emi_ctx_t c) {
    if (!c->delay_dirty) return EMI_OK;
    const int M = c->M, nd = std::max(c->xh - 1, c->uh);
    std::vector<double> W((size_t)nd * M * M);
    for (int d = 0; d < nd; ++d) delay_matrix(c->h_tau, c->h_w, c->t0, c->tf, (d + 1) * c->delay_dt, W.data() + (size_t)d * M * M);
    EMI_TRY(upload_real(c, c->d_W, W.data(), W.size()));       // (complete on return: W is a local)
    c->delay_dirty = false;
    return EMI_OK;
}

// dU_free [B][nc - nch][M] -> *dU_ext [B][nc][M] = [U | x(t - dt) .. x(t - (xh-1) dt) | u(t - dt) .. u(t - uh dt)], the delayed
// rows as products with W on the general MFMA defect kernel (rows += Z . W^T onto zeroed rows)
int extend_controls(emi_ctx_t c, const void* dX, const void* dU_free, const void** dU_ext) {
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "delayed values: f64 contexts only");
    if (c->points_only) return fail(c, EMI_ERR_STATE, "delayed values need a collocation mesh (this context holds a points-only mesh)");
    const int M = c->M, ncf = c->nc - c->nch;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->attr_set) {
        HIP_TRY(c, emi::defect_f64_set_attr());
        c->attr_set = true;
    }
    int st;
    if ((st = ensure_delay_matrices(c))) return st;
    const size_t row = (size_t)M * 8;
    if ((st = ensure(c, c->d_uext, (size_t)c->B * c->nc * row))) return st;
    HIP_TRY(c, hipMemsetAsync(c->d_uext.p, 0, (size_t)c->B * c->nc * row, c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(c->d_uext.p, (size_t)c->nc * row, dU_free, (size_t)ncf * row, (size_t)ncf * row, c->B, hipMemcpyDeviceToDevice, c->stream));
    double* base = (double*)c->d_uext.p + (size_t)ncf * M;
    for (int i = 1; i < c->xh; ++i) {       // x(t - i dt): all states against W[i-1]
        emi::DefectArgs a{(const double*)dX, (const double*)c->d_W.p + (size_t)(i - 1) * M * M, base + (size_t)(i - 1) * c->ns * M,
                          c->B * c->ns, M, c->ns, c->nc};
        HIP_TRY(c, emi::launch_defect_f64(a, c->stream));
    }
    base += (size_t)std::max(c->xh - 1, 0) * c->ns * M;
    for (int i = 1; i <= c->uh; ++i) {      // u(t - i dt): the caller's controls against W[i-1]
        emi::DefectArgs a{(const double*)dU_free, (const double*)c->d_W.p + (size_t)(i - 1) * M * M, base + (size_t)(i - 1) * ncf * M,
                          c->B * ncf, M, ncf, c->nc};
        HIP_TRY(c, emi::launch_defect_f64(a, c->stream));
    }
    *dU_ext = c->d_uext.p;
    return EMI_OK;
}

// ---- emi_set_option: the plain options, one row each (what the name means is said at the member it sets) -------------------
struct OptionRow {
    const char* name;
    int emi_ctx_s::*member;
    bool (*accepts)(int);       // the range or set of values taken ...
    int (*stored)(int);         // ... what an accepted value is stored as ...
    const char* message;        // ... and what emi_last_error says about any other
};
template <int LO, int HI> bool within(int v) { return v >= LO && v <= HI; }
template <int... VS> bool one_of(int v) { return ((v == VS) || ...); }
bool any_value(int) { return true; }
bool at_least_0(int v) { return v >= 0; }
bool whole_tiles(int v) { return v >= 0 && v % 16 == 0; }
int as_given(int v) { return v; }
int as_flag(int v) { return v != 0; }
int ring_wgs(int v) { return v == 1 ? 1 : 2; }
int block_order(int v) { return v < 0 ? -1 : (v >= 100 ? v : (v != 0)); }

const OptionRow OPTIONS[] = {
    {"overlap", &emi_ctx_s::allow_fused, any_value, as_flag, nullptr},
    {"fused", &emi_ctx_s::allow_fused, any_value, as_flag, nullptr},
    {"sym_ct", &emi_ctx_s::sym_ct, within<0, 8>, as_given,
     "sym_ct must be 0..8 (0/4 = chosen from the batch, 3 = LDS-DMA ring, 5..8 = state-split ring with SW = NS/2/1/3)"},
    {"small_rows", &emi_ctx_s::small_rows, at_least_0, as_given, "small_rows must be >= 0 (0 disables the skinny defect kernel)"},
    {"sym_order", &emi_ctx_s::sym_order, any_value, as_flag, nullptr},
    {"f32_ring", &emi_ctx_s::f32_ring, any_value, as_flag, nullptr},
    {"f32_ring_wgs", &emi_ctx_s::f32_ring_wgs, any_value, ring_wgs, nullptr},
    {"f32_one_launch", &emi_ctx_s::f32_one_launch, any_value, as_flag, nullptr},
    {"slice", &emi_ctx_s::slice, whole_tiles, as_given, "slice must be 0 (never) or a multiple of 16 instances"},
    {"pass_order", &emi_ctx_s::pass_order, any_value, block_order, nullptr},
    {"sym_ablate", &emi_ctx_s::sym_ablate, any_value, as_given, nullptr},   // diagnostics only
    {"adj_fold_tile", &emi_ctx_s::adj_fold_tile, within<0, 2>, as_given, "adj_fold_tile must be 0 (by size), 1 (48 x 64) or 2 (96 x 128)"},
    {"cost_in_kernel", &emi_ctx_s::cost_in_kernel, any_value, as_flag, nullptr},
    {"sym_nst", &emi_ctx_s::sym_nst, one_of<3, 4>, as_given, "sym_nst must be 3 or 4"},
    {"sym_hs", &emi_ctx_s::sym_hs, within<0, 2>, as_given, "sym_hs must be 0 (by batch size), 1 or 2"},
    {"sym_ctc", &emi_ctx_s::sym_ctc, within<0, 2>, as_given, "sym_ctc must be 0 (by batch size), 1 or 2"},
    {"sym_bk", &emi_ctx_s::sym_bk, one_of<0, 8, 16>, as_given, "sym_bk must be 0 (by batch size), 8 or 16"},
    {"sym_cpart", &emi_ctx_s::sym_cpart, one_of<-1, 0, 1, 2, 4, 8>, as_given, "sym_cpart must be -1 (plain order), 0 (by mesh size), 1, 2, 4 or 8"},
    {"sym_gblk", &emi_ctx_s::sym_gblk, within<0, 64>, as_given, "sym_gblk must be 0 (off) .. 64 instance groups per super-block"},
    {"sym_cx", &emi_ctx_s::sym_cx, within<0, 64>, as_given, "sym_cx must be 0 (default) .. 64 column tiles per block"},
    {"sym_combine", &emi_ctx_s::sym_combine, any_value, as_flag, nullptr},
    {"sym_ksplit", &emi_ctx_s::sym_ksplit, one_of<0, 1, 2, 4, 8>, as_given, "sym_ksplit must be 0 (by batch size), 1, 2, 4 or 8"},
    {"node_store", &emi_ctx_s::node_store, within<-1, 3>, as_given,
     "node_store must be -1 (by size), 0 (plain), 1 (write-through sc1), 2 (non-temporal) or 3 (nt sc1; the one-launch pass only)"},
    {"overlap_mode", &emi_ctx_s::overlap_mode, within<0, 3>, as_given,
     "overlap_mode must be 0 (by batch size), 1 (one stream), 2 (two streams) or 3 (one launch)"},
};

// ---- the evaluation pass: one chooser (choose_form), one function per launch form ------------------------------------------

// the second stream of the two-stream forms (node kernel beside the MFMA defect kernel), created on first use
int need_stream2(emi_ctx_t c) {
    if (c->stream2) return EMI_OK;
    if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess) {
        c->stream2 = nullptr;
        return fail(c, EMI_ERR_HIP, "cannot create the second stream of the two-stream pass");
    }
    return EMI_OK;
}

// The forms a launch of the pass can take.  choose_form is the one place that picks among them; emi_last_path asks it too.
enum class Form {
    PassF64,        // form_pass_f64: emi_pass_f64_kernel, MFMA-role and node-role workgroups in one grid
    TwoKernelF64,   // form_two_kernel_f64: even/odd MFMA defect kernel and node kernel, on one or two streams or on CU-split streams
    PassF32,        // form_pass_f32: emi_pass_f32_kernel, the fp32 pass as one launch
    TwoStreamF32,   // form_two_stream_f32: fp32 MFMA defect kernel beside the full node kernel ("overlap_mode" 2)
    Sequential,     // form_sequential: node kernel, then the general (or skinny) defect kernel, on the context's stream
};
struct FormChoice {
    Form form = Form::Sequential;
    bool small = false;     // Sequential: the skinny streaming defect kernel instead of the MFMA one
    PassPlan plan;          // PassF64 (and TwoKernelF64, which it declined): what plan_pass decided
    bool overlapped() const { return form == Form::PassF64 || form == Form::TwoKernelF64; }
};

FormChoice choose_form(emi_ctx_t c, Launch L, unsigned flags) {
    const bool nodes = flags & EMI_EVAL_NODES, defect = flags & EMI_EVAL_DEFECT, jac = !(flags & EMI_EVAL_NOJAC);
    FormChoice ch;
    // a handful of instances: the stand-alone MFMA kernels would have a few workgroups to run and a skinny streaming product wins
    // (21 us at B = 1) -- unless the whole pass can go as ONE launch with its K range sliced, which is faster still (13 - 15 us for
    // any batch up to 16 instances: profiles/r03_notes.md section 7)
    ch.small = defect && !c->f32 && L.B > 0 && L.B * c->ns <= c->small_rows && emi::defect_small_supported(L.B * c->ns) &&
               !(nodes && jac && pass_takes_small_batches(c, L.B));
    if (nodes && defect && !ch.small && overlapped_path(c)) {
        ch.plan = plan_pass(c, L.B, jac);
        ch.form = ch.plan.one_launch ? Form::PassF64 : Form::TwoKernelF64;
    } else if (c->f32 && nodes && defect && jac && !c->rtc && c->allow_fused) {
        if ((c->overlap_mode == 3 || (c->overlap_mode == 0 && c->f32_one_launch)) && emi::pass_f32_supported(c->model, L.B * c->ns, c->M, L.B))
            ch.form = Form::PassF32;
        else if (c->overlap_mode == 2 && emi::defect_f32_mfma_supported(c->M))
            ch.form = Form::TwoStreamF32;
    }
    return ch;
}

// the record of the next profiled launch; the list owns every event from the moment it exists (a record whose events could not
// all be created is completed by the next call)
int next_prof_record(emi_ctx_t c, ProfEvents** out) {
    if (c->prof_used == c->prof.size()) c->prof.emplace_back();
    ProfEvents& pe = c->prof[c->prof_used];
    for (hipEvent_t& e : pe.ev)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    ++c->prof_used;
    *out = &pe;
    return EMI_OK;
}

// One side of a profiling bracket: event `which` of the launch's record on stream s, when the launch is profiled (pe) at one of
// the levels in `levels` (emi_profile_enable: AT1 every bracket, AT2 the defect kernel only, AT3 the node kernel only)
constexpr unsigned AT1 = 1u << 1, AT2 = 1u << 2, AT3 = 1u << 3, AT_ANY = AT1 | AT2 | AT3;
int prof_mark(emi_ctx_t c, ProfEvents* pe, ProfMark which, unsigned levels, hipStream_t s) {
    if (pe && pe->level > 0 && ((levels >> pe->level) & 1u)) HIP_TRY(c, hipEventRecord(pe->ev[which], s));
    return EMI_OK;
}

// ---- what emi_last_defect_kernel reports (the names a rocprofv3 kernel trace shows), each built here and nowhere else
const char* const NAME_PASS_F32 = "emi_pass_f32_kernel (MFMA + node roles, one launch)";
const char* const NAME_RING1_F64 = "emi_symdefect_ring_f64_kernel";
const char* name_defect_f32(emi_ctx_t c, bool mfma) {
    return !mfma ? "emi_defect_f32_kernel" : (c->f32_ring ? "emi_defect_f32_ring_kernel" : "emi_defect_f32_mfma_kernel");
}
const char* name_defect_f64(bool small) { return small ? "emi_defect_small_f64_kernel" : "emi_defect_f64_kernel"; }
std::string name_pass_f64(const emi::SymPlan& plan) {
    return "emi_pass_f64_kernel<SW=" + std::to_string(plan.sw) + "> (MFMA + node roles, one launch" +
           (plan.ks > 1 ? ", " + std::to_string(plan.ks) + " K slices per tile" : "") + ")" +
           (plan.bk == 16 ? " [K tiles of 16]" : "") + (plan.ct == 2 ? " [128-column tiles]" : "") + (plan.hs == 2 ? " [K range in two halves per workgroup]" : "");
}
std::string name_symdefect(emi_ctx_t c, const emi::SymPlan& plan, bool in_kernel_combine) {
    if (plan.ring1) return c->sym_ct == 1 || c->sym_ct == 2 ? "emi_symdefect_f64_kernel" : NAME_RING1_F64;
    return "emi_symdefect_ring2_f64_kernel<SW=" + std::to_string(plan.sw) + ">" +
           (plan.ks > 1 ? " x" + std::to_string(plan.ks) + (in_kernel_combine ? " K slices (in-kernel combine)" : " K slices + emi_symdefect_combine_kernel") : "");
}

// arguments of the even/odd MFMA role for a launch, unsplit and in the plain tile order (the forms set what their plan changes)
emi::SymDefectArgs sym_defect_args(emi_ctx_t c, Launch L, const PassIO& io) {
    emi::SymDefectArgs sa;
    sa.X = (const double*)io.X;
    sa.U = (const double*)io.U;
    sa.RES = (double*)io.RES;
    sa.node_t = (const double*)c->d_t.p;
    sa.De = (const double*)c->d_De.p;
    sa.Do = (const double*)c->d_Do.p;
    sa.M = c->M;
    sa.B = L.B;
    sa.nres = nres_of(c);
    sa.h = (c->tf - c->t0) / 2.0;
    sa.order = c->sym_order;
    sa.ablate = c->sym_ablate;
    sa.ksplit = 1;
    sa.slab = nullptr;
    sa.tile_ticket = nullptr;
    sa.cpart = sa.cx = 0;
    sa.mfma_first = 0;
    for (int i = 0; i < EMI_MAX_PARAMS; ++i) sa.P.p[i] = c->params[i];
    return sa;
}

emi::DefectArgsF32 defect_args_f32(emi_ctx_t c, Launch L, const PassIO& io) {
    return emi::DefectArgsF32{(const float*)io.X, (const float*)c->d_D.p, (float*)io.RES, L.B * c->ns, c->M, c->ns, nres_of(c)};
}

// The fp64 pass as ONE launch, by the plan the chooser made: MFMA-role and node-role workgroups in one grid, K slices combined
// and COST finished in-kernel by ticket.
int form_pass_f64(emi_ctx_t c, Launch L, const PassIO& io, const PassPlan& pp, ProfEvents* pe) {
    const emi::SymPlan& plan = pp.sym;
    emi::SymDefectArgs sa = sym_defect_args(c, L, io);
    emi::NodeArgs<double> na;
    fill_node_args(c, L, na, io);
    sa.mfma_first = pp.mfma_first;
    sa.cpart = plan.cpart;
    sa.cx = plan.cx;
    if (plan.ks > 1) {
        EMI_TRY(ensure(c, c->d_slab, plan.slab_bytes));
        EMI_TRY(ensure_zeroed(c, c->d_tile_ticket, (size_t)plan.tiles * 4, c->stream));
        sa.ksplit = plan.ks;
        sa.slab = (double*)c->d_slab.p;
        sa.tile_ticket = (unsigned*)c->d_tile_ticket.p;
    }
    EMI_TRY(ensure_zeroed(c, c->d_ticket, (size_t)L.B * 4, c->stream));
    na.cost_ticket = (unsigned*)c->d_ticket.p;
    EMI_TRY(prof_mark(c, pe, K0, AT_ANY, c->stream));
    if (c->rtc) HIP_TRY(c, emi::rtc_launch_pass(c->rtc, sa, na, plan.sw, c->stream));
    else HIP_TRY(c, emi::launch_pass(c->model, sa, na, c->stream, plan));
    EMI_TRY(prof_mark(c, pe, K1, AT_ANY, c->stream));
    if (pe) pe->level = -1;                 // one bracket: the pass kernel
    c->last_defect_kernel = name_pass_f64(plan);
    return EMI_OK;
}

// the stand-alone even/odd MFMA defect kernel of the two-kernel form on stream s, K slices by "sym_ksplit"
int launch_symdefect_f64(emi_ctx_t c, Launch L, emi::SymDefectArgs& sa, hipStream_t s) {
    if (c->rtc) {
        HIP_TRY(c, emi::rtc_launch_symdefect(c->rtc, sa, s));
        c->last_defect_kernel = NAME_RING1_F64;
        return EMI_OK;
    }
    const emi::SymPlan plan = emi::plan_symdefect(c->ns, L.B, c->M, c->sym_ct, c->sym_ksplit, c->sym_cpart, c->sym_gblk, c->sym_cx);
    if (plan.slab_bytes) EMI_TRY(ensure(c, c->d_slab, plan.slab_bytes));
    sa.ksplit = plan.ring1 ? 1 : plan.ks;
    sa.slab = (double*)c->d_slab.p;
    sa.cpart = plan.cpart;
    sa.cx = plan.cx;
    if (sa.ksplit > 1 && c->sym_combine) {
        EMI_TRY(ensure_zeroed(c, c->d_tile_ticket, (size_t)plan.tiles * 4, s));
        sa.tile_ticket = (unsigned*)c->d_tile_ticket.p;
    }
    const unsigned bit = 1u << c->sym_ct;
    HIP_TRY(c, emi::launch_symdefect(c->model, sa, s, !(c->fused_attr_mask & bit), c->sym_ct, plan));
    c->fused_attr_mask |= bit;
    c->last_defect_kernel = name_symdefect(c, plan, sa.tile_ticket != nullptr);
    return EMI_OK;
}

// The fp64 pass as two kernels that read X, U and write disjoint outputs.  "overlap_mode" 1: back to back on the context's stream;
// otherwise forked onto a second stream (or, with "cu_split", onto two CU-masked streams) and joined again.  The MFMA kernel goes
// first and takes one workgroup per CU (LDS-shaped); the streaming kernel's waves fill the rest of every CU.
int form_two_kernel_f64(emi_ctx_t c, Launch L, const PassIO& io, bool jac, ProfEvents* pe) {
    emi::SymDefectArgs sa = sym_defect_args(c, L, io);
    emi::NodeArgs<double> na;
    fill_node_args(c, L, na, io);
    const bool two = c->overlap_mode != 1;
    const bool split = two && c->cu_split > 0;
    if (two && !split) EMI_TRY(need_stream2(c));
    hipStream_t s1 = split ? c->s_mfma : c->stream;
    hipStream_t s2 = split ? c->s_node : (two ? c->stream2 : c->stream);
    if (two) {
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(s2, c->ev_fork, 0));
        if (split) HIP_TRY(c, hipStreamWaitEvent(s1, c->ev_fork, 0));
    }
    EMI_TRY(prof_mark(c, pe, K0, AT1 | AT2, s1));
    EMI_TRY(launch_symdefect_f64(c, L, sa, s1));
    EMI_TRY(prof_mark(c, pe, K1, AT1 | AT2, s1));
    // COST is finished inside the node kernel (last workgroup of an instance, by ticket, in chunk order): one launch
    // and one kernel boundary less at the end of every pass (emi_cost_finish_kernel alone was 5 us)
    if (c->cost_in_kernel) {
        EMI_TRY(ensure_zeroed(c, c->d_ticket, (size_t)L.B * 4, s2));
        na.cost_ticket = (unsigned*)c->d_ticket.p;
    }
    EMI_TRY(prof_mark(c, pe, K2, AT1 | AT3, s2));
    if (c->rtc && jac && na.store_mode == 2 && c->M % 2 == 0) HIP_TRY(c, emi::rtc_launch_nodes_nt(c->rtc, na, s2));
    else if (c->rtc) HIP_TRY(c, emi::rtc_launch_nodes<double>(c->rtc, na, jac, false, s2));
    else HIP_TRY(c, emi::launch_nodes<double>(c->model, na, jac, false, s2));
    EMI_TRY(prof_mark(c, pe, K3, AT1 | AT3, s2));
    if (!c->cost_in_kernel) HIP_TRY(c, emi::launch_cost_finish<double>(na.cost_part, na.cost, L.B, emi::node_chunks(c->M), na.sgn * na.h, s2));
    if (two) {
        HIP_TRY(c, hipEventRecord(c->ev_join, s2));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        if (split) {
            HIP_TRY(c, hipEventRecord(c->ev_join2, s1));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join2, 0));
        }
    }
    EMI_TRY(prof_mark(c, pe, E1, AT1, c->stream));
    EMI_TRY(prof_mark(c, pe, E2, AT1, c->stream));
    return EMI_OK;
}

// fp32 contexts (config 5): the pass as ONE launch -- MFMA-role and node-role workgroups in one grid, the defect rows zeroed
// here and completed by float atomics from both roles (emi_defect_f32.hip), COST finished in-kernel by ticket
int form_pass_f32(emi_ctx_t c, Launch L, const PassIO& io, ProfEvents* pe) {
    emi::NodeArgs<float> na;
    fill_node_args(c, L, na, io);
    const size_t rowb = (size_t)c->M * 4;
    HIP_TRY(c, hipMemset2DAsync(io.RES, (size_t)nres_of(c) * rowb, 0, (size_t)c->ns * rowb, L.B, c->stream));
    EMI_TRY(ensure_zeroed(c, c->d_ticket, (size_t)L.B * 4, c->stream));
    na.cost_ticket = (unsigned*)c->d_ticket.p;
    EMI_TRY(prof_mark(c, pe, K0, AT_ANY, c->stream));
    HIP_TRY(c, emi::launch_pass_f32(c->model, defect_args_f32(c, L, io), na, c->pass_order >= 0 ? c->pass_order : 0, c->stream));
    EMI_TRY(prof_mark(c, pe, K1, AT_ANY, c->stream));
    if (pe) { pe->level = -1; pe->fused = true; }
    c->last_defect_kernel = NAME_PASS_F32;
    return EMI_OK;
}

// fp32 contexts (config 5), only when asked for ("overlap_mode" 2): the f32 MFMA defect kernel ACCUMULATES onto
// -h f, so a values-only node kernel writes -h f first and the MFMA kernel follows it on the context's stream, while
// the full node kernel (Jacobian values, cost; no defect rows) runs beside them on the second stream.  Measured at
// B = 256, M = 4096: 1.076 ms against 1.082 ms back to back -- both kernels stretch (MFMA 0.93 -> 1.03 ms, node
// 0.16 -> 0.80 ms), nothing is gained, so the default stays sequential (profiles/r02_notes.md)
int form_two_stream_f32(emi_ctx_t c, Launch L, const PassIO& io, ProfEvents* pe) {
    emi::NodeArgs<float> pre, full;
    PassIO values_only = io;
    values_only.VALS = nullptr;
    fill_node_args(c, L, pre, values_only);
    fill_node_args(c, L, full, io);
    EMI_TRY(ensure(c, c->d_cost_part2, (size_t)L.B * emi::node_chunks(c->M) * 4));
    EMI_TRY(need_stream2(c));
    pre.cost_part = (float*)c->d_cost_part2.p;      // its cost partials go nowhere
    pre.np = 0;                                      // ... and it leaves the path rows to the full kernel
    // (round 4, "f32_ring_wgs" 1: the ring kernel at one workgroup per CU, which costs it nothing, leaves the node kernel's waves
    // room on every SIMD; the node kernel is then released only once the values-only kernel is through, so that it does not fill the
    // chip before the ring kernel's workgroups arrive)
    const bool fork_late = c->f32_ring_wgs == 1;
    if (!fork_late) {
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    }
    HIP_TRY(c, emi::launch_nodes<float>(c->model, pre, false, true, c->stream));
    if (fork_late) {
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    }
    EMI_TRY(prof_mark(c, pe, K0, AT1 | AT2, c->stream));
    HIP_TRY(c, emi::launch_defect_f32_mfma(defect_args_f32(c, L, io), c->stream, c->f32_ring, c->f32_ring_wgs));
    EMI_TRY(prof_mark(c, pe, K1, AT1 | AT2, c->stream));
    c->last_defect_kernel = name_defect_f32(c, true);
    EMI_TRY(prof_mark(c, pe, K2, AT1 | AT3, c->stream2));
    HIP_TRY(c, emi::launch_nodes<float>(c->model, full, true, false, c->stream2));
    EMI_TRY(prof_mark(c, pe, K3, AT1 | AT3, c->stream2));
    HIP_TRY(c, emi::launch_cost_finish<float>(full.cost_part, full.cost, L.B, emi::node_chunks(c->M), full.sgn * full.h, c->stream2));
    HIP_TRY(c, hipEventRecord(c->ev_join, c->stream2));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    if (pe) pe->fused = true;
    EMI_TRY(prof_mark(c, pe, E1, AT1, c->stream));
    EMI_TRY(prof_mark(c, pe, E2, AT1, c->stream));
    return EMI_OK;
}

// the node kernel by itself (it writes -h f into the defect rows, which the defect kernel then adds D X onto), then COST
template <typename T>
int launch_nodes_alone(emi_ctx_t c, Launch L, const PassIO& io, bool jac) {
    emi::NodeArgs<T> a;
    fill_node_args(c, L, a, io);
    if (c->rtc) HIP_TRY(c, emi::rtc_launch_nodes<T>(c->rtc, a, jac, true, c->stream));
    else HIP_TRY(c, emi::launch_nodes<T>(c->model, a, jac, true, c->stream));
    HIP_TRY(c, emi::launch_cost_finish<T>(a.cost_part, a.cost, L.B, emi::node_chunks(c->M), a.sgn * a.h, c->stream));
    return EMI_OK;
}

// The general sequence on the context's stream: node kernel, then defect kernel (either alone where the flags ask for one).
int form_sequential(emi_ctx_t c, Launch L, const PassIO& io, unsigned flags, bool small, ProfEvents* pe) {
    const bool jac = !(flags & EMI_EVAL_NOJAC);
    if (flags & EMI_EVAL_NODES) EMI_TRY(c->f32 ? launch_nodes_alone<float>(c, L, io, jac) : launch_nodes_alone<double>(c, L, io, jac));
    EMI_TRY(prof_mark(c, pe, E1, AT_ANY, c->stream));
    if ((flags & EMI_EVAL_DEFECT) && c->f32) {
        const bool mfma = emi::defect_f32_mfma_supported(c->M) && c->allow_fused;
        if (mfma) HIP_TRY(c, emi::launch_defect_f32_mfma(defect_args_f32(c, L, io), c->stream, c->f32_ring, c->f32_ring_wgs));
        else HIP_TRY(c, emi::launch_defect_f32(defect_args_f32(c, L, io), c->stream));
        c->last_defect_kernel = name_defect_f32(c, mfma);
    } else if (flags & EMI_EVAL_DEFECT) {
        emi::DefectArgs a{(const double*)io.X, (const double*)c->d_D.p, (double*)io.RES, L.B * c->ns, c->M, c->ns, nres_of(c)};
        if (small) HIP_TRY(c, emi::launch_defect_small_f64(a, c->stream));
        else HIP_TRY(c, emi::launch_defect_f64(a, c->stream));
        c->last_defect_kernel = name_defect_f64(small);
    }
    EMI_TRY(prof_mark(c, pe, E2, AT1 | AT2, c->stream));
    return EMI_OK;
}

// One launch of the pass: the argument checks, the profiling record, then the form the chooser names.
int eval_launch(emi_ctx_t c, Launch L, const PassIO& io, unsigned flags) {
    const bool nodes = flags & EMI_EVAL_NODES, defect = flags & EMI_EVAL_DEFECT;
    const bool jac = !(flags & EMI_EVAL_NOJAC);
    if (!nodes && !defect) return fail(c, EMI_ERR_ARG, "emi_eval: empty flags");
    if (defect && c->points_only) return fail(c, EMI_ERR_STATE, "emi_eval: the mesh has no differentiation matrix (points-only mesh): EMI_EVAL_NODES only");
    if (!io.X || !io.RES || (nodes && (!io.U || !io.COST || (jac && !io.VALS))))
        return fail(c, EMI_ERR_ARG, "emi_eval: null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->attr_set) {
        HIP_TRY(c, emi::defect_f64_set_attr());
        c->attr_set = true;
    }
    const FormChoice ch = choose_form(c, L, flags);
    ProfEvents* pe = nullptr;
    if (c->profile) {
        EMI_TRY(next_prof_record(c, &pe));
        pe->has_node = nodes;
        pe->has_defect = defect;
        pe->fused = ch.overlapped();
        pe->level = c->profile;
        EMI_TRY(prof_mark(c, pe, E0, pe->fused ? AT1 : AT1 | AT3, c->stream));
    }
    switch (ch.form) {
        case Form::PassF64: return form_pass_f64(c, L, io, ch.plan, pe);
        case Form::TwoKernelF64: return form_two_kernel_f64(c, L, io, jac, pe);
        case Form::PassF32: return form_pass_f32(c, L, io, pe);
        case Form::TwoStreamF32: return form_two_stream_f32(c, L, io, pe);
        case Form::Sequential: break;
    }
    return form_sequential(c, L, io, flags, ch.small, pe);
}

}  // namespace

extern "C" {

int emi_device_count(int* count) {
    if (!count) return EMI_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return EMI_OK;
}

static int create_impl(int device_id, bool f32, emi_ctx_t* out) {
    if (!out) return EMI_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return EMI_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= n) return EMI_ERR_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return EMI_ERR_HIP;
    // gfx950 only: the code object holds no other ISA
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return EMI_ERR_NO_DEVICE;
    if (hipSetDevice(device_id) != hipSuccess) return EMI_ERR_HIP;
    emi_ctx_t c = new emi_ctx_s();
    c->device = device_id;
    c->f32 = f32;
    c->own_stream = true;
    // (stream2 is created when a two-stream form first asks for it, need_stream2: every stream takes a share of one of the runtime's few
    // hardware queues, and a Monte-Carlo run has a context per host thread)
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&c->t_start) != hipSuccess || hipEventCreate(&c->t_stop) != hipSuccess) {
        delete c;               // (the destructor releases what was created before the failure)
        return EMI_ERR_HIP;
    }
    *out = c;
    return EMI_OK;
}

int emi_create(int device_id, emi_ctx_t* out) { return create_impl(device_id, false, out); }
int emi_create_f32(int device_id, emi_ctx_t* out) { return create_impl(device_id, true, out); }

int emi_destroy(emi_ctx_t c) {
    if (!c) return EMI_ERR_ARG;
    delete c;
    return EMI_OK;
}

const char* emi_last_error(emi_ctx_t c) { return c ? c->err.c_str() : "null context"; }

int emi_set_stream(emi_ctx_t c, void* s) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (s == nullptr) {
        if (!c->own_stream) {
            HIP_TRY(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
            c->own_stream = true;
        }
        return EMI_OK;
    }
    if (c->own_stream) { HIP_TRY(c, hipStreamDestroy(c->stream)); c->own_stream = false; }
    c->stream = (hipStream_t)s;
    return EMI_OK;
}

int emi_get_stream(emi_ctx_t c, void** s) {
    if (!c || !s) return EMI_ERR_ARG;
    *s = (void*)c->stream;
    return EMI_OK;
}

int emi_synchronize(emi_ctx_t c) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

// the differentiation matrix of a collocation mesh on the device: D itself (fp32 contexts: a copy whose rows sum to zero), and for
// an exactly centro-antisymmetric D on an even number of nodes its even/odd halves De / Do (c->symmetric says whether they are valid)
static int upload_operator(emi_ctx_t c, int M, const double* D) {
    if (c->f32) {
        // f32 copy of D whose rows sum to EXACTLY zero in f32 arithmetic terms: off-diagonals rounded,
        // diagonal = -(f64 sum of the rounded off-diagonals), rounded.  The shifted-difference form of
        // the f32 defect kernel (emi_defect_f32.hip) relies on it.
        std::vector<float> Df((size_t)M * M);
        for (int i = 0; i < M; ++i) {
            double rs = 0.0;
            for (int j = 0; j < M; ++j) {
                if (j == i) continue;
                Df[(size_t)i * M + j] = (float)D[(size_t)i * M + j];
                rs += (double)Df[(size_t)i * M + j];
            }
            Df[(size_t)i * M + i] = (float)(-rs);
        }
        return upload_bytes(c, c->d_D, Df.data(), Df.size() * 4);
    }
    EMI_TRY(upload_real(c, c->d_D, D, (size_t)M * M));
    // even/odd split of D for the fused kernel: valid only for an exactly centro-antisymmetric D
    if (M % 2 != 0) return EMI_OK;
    const int N = M - 1, Hh = M / 2;
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < M; ++j)
            if (D[(size_t)i * M + j] != -D[(size_t)(N - i) * M + (N - j)]) return EMI_OK;
    std::vector<double> De((size_t)Hh * Hh), Do((size_t)Hh * Hh);
    for (int i = 0; i < Hh; ++i)
        for (int j = 0; j < Hh; ++j) {
            const double p = D[(size_t)i * M + j], q = D[(size_t)i * M + (N - j)];
            De[(size_t)i * Hh + j] = 0.5 * (p + q);
            Do[(size_t)i * Hh + j] = 0.5 * (p - q);
        }
    EMI_TRY(upload_real(c, c->d_De, De.data(), De.size()));
    EMI_TRY(upload_real(c, c->d_Do, Do.data(), Do.size()));
    c->symmetric = true;
    return EMI_OK;
}

int emi_set_mesh(emi_ctx_t c, int M, const double* tau, const double* w, const double* D, double t0,
                 double tf) {
    if (!c || M < 2 || !tau || !w) return fail(c, EMI_ERR_ARG, "emi_set_mesh: bad argument");
    if (!(tf > t0)) return fail(c, EMI_ERR_ARG, "emi_set_mesh: tf must exceed t0");
    c->keep.bump();             // h, D_kk and the weights enter the invariant rows of VALS
    HIP_TRY(c, hipSetDevice(c->device));
    // D == NULL is a points-only mesh: the node functions are evaluated at arbitrary abscissae (the ODE-error estimate between
    // the collocation nodes); there is no differentiation matrix, so EMI_EVAL_DEFECT and the KKT entry points refuse
    const double h = (tf - t0) / 2.0;
    std::vector<double> nt(M), dd(M, 0.0);
    for (int k = 0; k < M; ++k) {
        nt[k] = t0 + h * (tau[k] + 1.0);
        if (D) dd[k] = D[(size_t)k * M + k];
    }
    EMI_TRY(upload_real(c, c->d_w, w, M));
    EMI_TRY(upload_real(c, c->d_t, nt.data(), M));
    EMI_TRY(upload_real(c, c->d_Ddiag, dd.data(), M));
    c->symmetric = false;
    if (D) EMI_TRY(upload_operator(c, M, D));
    c->points_only = !D;
    c->h_tau.assign(tau, tau + M);
    c->h_w.assign(w, w + M);
    c->M = M;
    c->t0 = t0;
    c->tf = tf;
    c->adj_dirty = true;
    c->delay_dirty = true;      // W(delay) is built for one mesh: [nd][M][M] on these nodes and this horizon
    c->adjw_dirty = true;
    emi::kkt_mesh_changed(c->kkt);
    for (emi::KktWorkspace* w : c->kkt_shard) emi::kkt_mesh_changed(w);
    // tables sized by M are stale now
    c->ntracks = 0;
    c->track_sets = 0;
    // the per-block cost partials are sized B * node_chunks(M): keep them valid for the batch already set
    if (c->B > 0) EMI_TRY(ensure(c, c->d_cost_part, (size_t)c->B * emi::node_chunks(M) * (c->f32 ? 4 : 8)));
    return EMI_OK;
}

// A new model is in force: its dimensions, the traced rows it computes itself (run-time compiled models) and its parameters.
// What was declared for the previous model goes: delayed values (emi_set_delays again) and the path rows, which name states
// (px, py) that this model may not have.
static void model_in_force(emi_ctx_t c, int model, int ns, int nc, int npath, const int* path_vars, int n_path_vars,
                           const double* params, int nparams, int maximize) {
    c->keep.bump();             // the model, its parameters and the cost sign
    c->model = model;
    c->ns = ns;
    c->nc = nc;
    c->xh = c->uh = c->nch = 0;
    c->np_model = npath;
    c->pvars.assign(path_vars, path_vars + n_path_vars);
    c->maximize = maximize ? 1 : 0;
    memset(c->params, 0, sizeof c->params);
    for (int i = 0; i < nparams; ++i) c->params[i] = params[i];
    c->np = 0;
    c->path_sets = 0;
    c->path_has_track = false;
}

int emi_set_model(emi_ctx_t c, int model, const double* params, int nparams, int maximize) {
    if (!c) return EMI_ERR_ARG;
    int ns, nc, np_expected;
    if (emi_model_dims(model, &ns, &nc, &np_expected)) return fail(c, EMI_ERR_ARG, "unknown model %d", model);
    if (nparams != np_expected || (nparams > 0 && !params))
        return fail(c, EMI_ERR_ARG, "model %d takes %d parameters, got %d", model, np_expected, nparams);
    if (c->rtc) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        emi::rtc_destroy(c->rtc);
        c->rtc = nullptr;
    }
    model_in_force(c, model, ns, nc, 0, nullptr, 0, params, nparams, maximize);
    return EMI_OK;
}

int emi_set_model_source(emi_ctx_t c, const char* struct_name, const char* source, int ns, int nc, int npath,
                         const int* path_vars, int n_path_vars, const double* params, int nparams, int maximize) {
    if (!c) return EMI_ERR_ARG;
    if (npath < 0 || npath > 64) return fail(c, EMI_ERR_ARG, "emi_set_model_source: npath must be in [0, 64]");
    if (npath > 0 && (!path_vars || n_path_vars < 1 || n_path_vars > ns + nc))
        return fail(c, EMI_ERR_ARG, "emi_set_model_source: %d traced rows need the list of variables they depend on", npath);
    for (int q = 0; q < (npath > 0 ? n_path_vars : 0); ++q)
        if (path_vars[q] < 0 || path_vars[q] >= ns + nc || (q > 0 && path_vars[q] <= path_vars[q - 1]))
            return fail(c, EMI_ERR_ARG, "emi_set_model_source: path_vars must be ascending node-variable indices below %d", ns + nc);
    if (nparams < 0 || nparams > EMI_MAX_PARAMS || (nparams > 0 && !params))
        return fail(c, EMI_ERR_ARG, "emi_set_model_source: at most %d parameters", EMI_MAX_PARAMS);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    emi::RtcModel* m = nullptr;
    std::string log;
    const int st = emi::rtc_build(c->f32, struct_name, source, ns, nc, npath, npath > 0 ? n_path_vars : 0, &m, &log);
    if (st) {
        c->err = log;
        return st;
    }
    emi::rtc_destroy(c->rtc);
    c->rtc = m;
    model_in_force(c, EMI_MODEL_SOURCE, ns, nc, npath, path_vars, npath > 0 ? n_path_vars : 0, params, nparams, maximize);
    return EMI_OK;
}

int emi_check_model_source(const char* struct_name, const char* source, int ns, int nc, int npath, int n_path_vars, int f32,
                           char* log, size_t log_len) {
    std::string l;
    const int st = emi::rtc_check(f32 != 0, struct_name, source, ns, nc, npath, npath > 0 ? n_path_vars : 0, &l);
    if (log && log_len) {
        strncpy(log, l.c_str(), log_len - 1);
        log[log_len - 1] = '\0';
    }
    return st;
}

int emi_set_batch(emi_ctx_t c, int B) {
    if (!c || B < 1) return fail(c, EMI_ERR_ARG, "emi_set_batch: B must be >= 1");
    if (c->M <= 0) return fail(c, EMI_ERR_STATE, "emi_set_mesh must precede emi_set_batch");
    c->keep.bump();
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t rb = c->f32 ? 4 : 8;
    int st = ensure(c, c->d_cost_part, (size_t)B * emi::node_chunks(c->M) * rb);
    if (st) return st;
    c->B = B;
    return EMI_OK;
}

int emi_set_delays(emi_ctx_t c, int x_horizon, int u_horizon, double dt) {
    if (!c || x_horizon < 0 || u_horizon < 0) return fail(c, EMI_ERR_ARG, "emi_set_delays: horizons must be >= 0");
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_set_model / emi_set_model_source must precede emi_set_delays");
    c->keep.bump();
    const int nxd = std::max(x_horizon - 1, 0) * c->ns;
    // nc_free + nxd + uh * nc_free = nc  (the model's control count includes the delayed values)
    const int rest = c->nc - nxd;
    if (nxd + u_horizon == 0) { c->xh = x_horizon; c->uh = 0; c->nch = 0; return EMI_OK; }
    if (!(dt > 0)) return fail(c, EMI_ERR_ARG, "emi_set_delays: dt must be positive");
    if (rest < 1 || rest % (1 + u_horizon) != 0)
        return fail(c, EMI_ERR_ARG, "emi_set_delays: the model has %d controls, which is not nc + %d delayed states + %d x nc delayed controls for any nc >= 1",
                    c->nc, nxd, u_horizon);
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "emi_set_delays: f64 contexts only");
    c->xh = x_horizon;
    c->uh = u_horizon;
    c->nch = c->nc - rest / (1 + u_horizon);
    c->delay_dt = dt;
    c->delay_dirty = true;
    c->adjw_dirty = true;
    return EMI_OK;
}

int emi_get_delays(emi_ctx_t c, int* x_horizon, int* u_horizon, int* n_delayed) {
    if (!c) return EMI_ERR_ARG;
    if (x_horizon) *x_horizon = c->xh;
    if (u_horizon) *u_horizon = c->uh;
    if (n_delayed) *n_delayed = c->nch;
    return EMI_OK;
}

int emi_delay_matrix(int M, const double* tau, const double* w, double t0, double tf, double delay, double* W) {
    if (M < 2 || !tau || !w || !W || !(tf > t0) || delay < 0) return EMI_ERR_ARG;
    delay_matrix(std::vector<double>(tau, tau + M), std::vector<double>(w, w + M), t0, tf, delay, W);
    return EMI_OK;
}

int emi_set_path(emi_ctx_t c, int np, int nsets, const double* recs, int px_state, int py_state) {
    if (!c || np < 0) return fail(c, EMI_ERR_ARG, "emi_set_path: bad argument");
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_set_model must precede emi_set_path");
    c->keep.bump();             // the row layout of VALS
    if (np > 0 && (!recs || nsets < 1)) return fail(c, EMI_ERR_ARG, "emi_set_path: null table");
    if (px_state < 0 || px_state >= c->ns || py_state < 0 || py_state >= c->ns || px_state == py_state)
        return fail(c, EMI_ERR_ARG, "emi_set_path: state indices (%d,%d) out of range", px_state, py_state);
    HIP_TRY(c, hipSetDevice(c->device));
    bool has_track = false;
    for (size_t i = 0; i < (size_t)np * nsets; ++i) {
        const int kind = (int)recs[i * EMI_PATH_REC];
        if (kind != EMI_PATH_ELLIPSE && kind != EMI_PATH_DISC && kind != EMI_PATH_TRACK)
            return fail(c, EMI_ERR_ARG, "emi_set_path: record %zu has unknown kind %d", i, kind);
        has_track = has_track || kind == EMI_PATH_TRACK;
    }
    int st = upload_real(c, c->d_path, recs, (size_t)np * nsets * EMI_PATH_REC);
    if (st) return st;
    c->path_has_track = has_track;
    c->np = np;
    c->path_sets = np > 0 ? nsets : 0;
    c->px = px_state;
    c->py = py_state;
    return EMI_OK;
}

int emi_set_tracks(emi_ctx_t c, int ntracks, int nsets, const double* xc, const double* yc) {
    if (!c || ntracks < 0) return fail(c, EMI_ERR_ARG, "emi_set_tracks: bad argument");
    if (c->M <= 0) return fail(c, EMI_ERR_STATE, "emi_set_mesh must precede emi_set_tracks");
    c->keep.bump();
    if (ntracks > 0 && (!xc || !yc || nsets < 1)) return fail(c, EMI_ERR_ARG, "emi_set_tracks: null table");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)ntracks * nsets * c->M;
    int st;
    if ((st = upload_real(c, c->d_trkx, xc, n))) return st;
    if ((st = upload_real(c, c->d_trky, yc, n))) return st;
    c->ntracks = ntracks;
    c->track_sets = ntracks > 0 ? nsets : 0;
    return EMI_OK;
}

int emi_get_layout(emi_ctx_t c, emi_layout_t* o) {
    if (!c || !o) return EMI_ERR_ARG;
    o->model = c->model;
    o->ns = c->ns;
    o->nc = c->nc;
    o->np = np_total(c);
    o->M = c->M;
    o->B = c->B;
    o->nres = nres_of(c);
    o->nvals = nvals_of(c);
    o->nhess = nhess_of(c);
    o->real_bytes = c->f32 ? 4 : 8;
    o->px = c->px;
    o->py = c->py;
    o->t0 = c->t0;
    o->tf = c->tf;
    return EMI_OK;
}

// Per-instance NLP numbering (DESIGN.md "NLP layout"):
//   variables   z: state i node k -> i*M + k ; control c node k -> (ns+c)*M + k
//   constraints g: defect (i,k) -> i*M + k ; events ns*M + e (e < 2 ns) ;
//                  path (j,k) -> ns*M + 2 ns + j*M + k
int emi_jac_structure(emi_ctx_t c, int* rows, int* cols) {
    if (!c || !rows || !cols) return EMI_ERR_ARG;
    if (c->M <= 0 || c->model < 0) return fail(c, EMI_ERR_STATE, "mesh and model must be set");
    const int M = c->M, ns = c->ns, nv = c->ns + c->nc;
    size_t e = 0;
    for (int i = 0; i < ns; ++i)
        for (int v = 0; v < nv; ++v)
            for (int k = 0; k < M; ++k, ++e) { rows[e] = i * M + k; cols[e] = v * M + k; }
    for (int j = 0; j < c->np; ++j)                      // rows of the record table: two partials, (px, py)
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < M; ++k, ++e) {
                rows[e] = ns * M + 2 * ns + j * M + k;
                cols[e] = (s == 0 ? c->px : c->py) * M + k;
            }
    for (int j = 0; j < c->np_model; ++j)                // traced rows: one partial per variable of the model's list
        for (size_t q = 0; q < c->pvars.size(); ++q)
            for (int k = 0; k < M; ++k, ++e) {
                rows[e] = ns * M + 2 * ns + (c->np + j) * M + k;
                cols[e] = c->pvars[q] * M + k;
            }
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < M; ++k, ++e) { rows[e] = -1; cols[e] = v * M + k; }
    return EMI_OK;
}

int emi_invariant_rows(int model, int np, unsigned char* mask, int* nvals) {
    int ns, nc;
    if (np < 0 || emi_model_dims(model, &ns, &nc, nullptr)) return EMI_ERR_ARG;
    if (nvals) *nvals = ns * (ns + nc) + 2 * np + (ns + nc);
    if (mask && !emi::invariant_rows(model, np, mask)) return EMI_ERR_ARG;
    return EMI_OK;
}

int emi_dev_alloc(emi_ctx_t c, size_t bytes, void** dptr) {
    if (!c || !dptr) return EMI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMalloc(dptr, bytes));
    return EMI_OK;
}
int emi_dev_free(emi_ctx_t c, void* dptr) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipFree(dptr));
    return EMI_OK;
}
int emi_h2d(emi_ctx_t c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return EMI_ERR_ARG;
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}
int emi_d2h(emi_ctx_t c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return EMI_ERR_ARG;
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

int emi_eval_dev(emi_ctx_t c, const void* dX, const void* dU, void* dRES, void* dVALS, void* dCOST,
                 unsigned flags) {
    int st = ready(c);
    if (st) return st;
    if (c->nch > 0 && dX && dU && (st = extend_controls(c, dX, dU, &dU))) return st;     // delayed values appended to the controls
    // large batches go out in pieces only where something forces them (plan_piece); not while per-kernel profiling is on
    int piece = 0;
    if (!c->profile && !c->f32 && (flags & EMI_EVAL_ALL) == EMI_EVAL_ALL && overlapped_path(c) && dX && dU && dRES && dCOST &&
        (dVALS || (flags & EMI_EVAL_NOJAC)))
        piece = plan_piece(c, c->B);
    const PassIO io{dX, dU, dRES, dVALS, dCOST};
    // EMI_EVAL_KEEP_INVARIANT: honoured where this pass writes the Jacobian into the buffer the record names, under the generation
    // it was made in; any other Jacobian pass writes everything and renews the record -- once ALL its pieces are out.  Passes that
    // write no Jacobian (line searches interleave them) leave the record alone.
    const emi::KeepRecord::Pass kp = c->keep.begin_pass((flags & EMI_EVAL_NODES) && !(flags & EMI_EVAL_NOJAC),
                                                        flags & EMI_EVAL_KEEP_INVARIANT, dVALS);
    flags &= ~(unsigned)EMI_EVAL_KEEP_INVARIANT;
    if (piece <= 0) st = eval_launch(c, Launch{0, c->B, kp.keep}, io, flags);
    for (int first = 0; piece > 0 && first < c->B && st == EMI_OK; first += piece)
        st = eval_launch(c, Launch{first, std::min(piece, c->B - first), kp.keep}, io_at(c, io, first), flags);
    c->keep.end_pass(kp, dVALS, st == EMI_OK);
    return st;
}

int emi_eval_host(emi_ctx_t c, const double* X, const double* U, double* RES, double* VALS,
                  double* COST, unsigned flags) {
    int st = ready(c);
    if (st) return st;
    if (!X || !U) return fail(c, EMI_ERR_ARG, "emi_eval_host: null input");
    const size_t rb = c->f32 ? 4 : 8;
    const size_t nX = (size_t)c->B * c->ns * c->M, nU = (size_t)c->B * (c->nc - c->nch) * c->M;
    const size_t nR = (size_t)c->B * nres_of(c) * c->M, nV = (size_t)c->B * nvals_of(c) * c->M;
    if ((st = upload_real(c, c->s_X, X, nX))) return st;
    if ((st = upload_real(c, c->s_U, U, nU))) return st;
    if ((st = ensure(c, c->s_RES, nR * rb))) return st;
    if ((st = ensure_vals_staging(c, nV * rb))) return st;
    if ((st = ensure(c, c->s_COST, (size_t)c->B * rb))) return st;
    if (!(flags & EMI_EVAL_NODES)) {
        // accumulate-only form: the caller's RES is the starting value
        if (!RES) return fail(c, EMI_ERR_ARG, "emi_eval_host: defect-only needs RES in/out");
        if ((st = upload_real(c, c->s_RES, RES, nR))) return st;
    }
    // (the staging buffer is the context's own: the record knows whether it still holds the invariant rows)
    if ((st = emi_eval_dev(c, c->s_X.p, c->s_U.p, c->s_RES.p, c->s_VALS.p, c->s_COST.p, flags | EMI_EVAL_KEEP_INVARIANT))) return st;
    if ((st = download_real(c, RES, c->s_RES.p, nR))) return st;
    if (!(flags & EMI_EVAL_NOJAC) && (flags & EMI_EVAL_NODES))
        if ((st = download_real(c, VALS, c->s_VALS.p, nV))) return st;
    if (flags & EMI_EVAL_NODES)
        if ((st = download_real(c, COST, c->s_COST.p, c->B))) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

int emi_hess_dev(emi_ctx_t c, const void* dX, const void* dU, const void* dLamF, const void* dLamC,
                 double sigma, void* dH) {
    int st = ready(c);
    if (st) return st;
    if (!dX || !dU || !dLamF || !dH || (np_total(c) > 0 && !dLamC))
        return fail(c, EMI_ERR_ARG, "emi_hess: null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->nch > 0 && (st = extend_controls(c, dX, dU, &dU))) return st;
    auto fill = [&](auto& a) {
        using T = typename std::remove_reference<decltype(a.h)>::type;
        a.X = (const T*)dX; a.U = (const T*)dU; a.lamF = (const T*)dLamF; a.lamC = (const T*)dLamC;
        a.H = (T*)dH; a.w = (const T*)c->d_w.p; a.node_t = (const T*)c->d_t.p;
        a.path = (const T*)c->d_path.p;
        a.M = c->M; a.B = c->B; a.np = np_total(c); a.path_sets = c->path_sets; a.px = c->px; a.py = c->py;
        a.h = (T)((c->tf - c->t0) / 2.0); a.sgn = c->maximize ? T(-1) : T(1); a.sigma = (T)sigma;
        for (int i = 0; i < EMI_MAX_PARAMS; ++i) a.P.p[i] = (T)c->params[i];
    };
    if (c->f32) {
        emi::HessArgs<float> a;
        fill(a);
        if (c->rtc) HIP_TRY(c, emi::rtc_launch_hess<float>(c->rtc, a, c->stream));
        else HIP_TRY(c, emi::launch_hess<float>(c->model, a, c->stream));
    } else {
        emi::HessArgs<double> a;
        fill(a);
        if (c->rtc) HIP_TRY(c, emi::rtc_launch_hess<double>(c->rtc, a, c->stream));
        else HIP_TRY(c, emi::launch_hess<double>(c->model, a, c->stream));
    }
    return EMI_OK;
}

int emi_hess_host(emi_ctx_t c, const double* X, const double* U, const double* LamF,
                  const double* LamC, double sigma, double* H) {
    int st = ready(c);
    if (st) return st;
    if (!X || !U || !LamF || !H || (np_total(c) > 0 && !LamC)) return fail(c, EMI_ERR_ARG, "emi_hess_host: null pointer");
    const size_t rb = c->f32 ? 4 : 8;
    const size_t nX = (size_t)c->B * c->ns * c->M, nU = (size_t)c->B * (c->nc - c->nch) * c->M;
    const size_t nC = (size_t)c->B * np_total(c) * c->M, nH = (size_t)c->B * nhess_of(c) * c->M;
    if ((st = upload_real(c, c->s_X, X, nX))) return st;
    if ((st = upload_real(c, c->s_U, U, nU))) return st;
    if ((st = upload_real(c, c->s_LF, LamF, nX))) return st;
    if (nC && (st = upload_real(c, c->s_LC, LamC, nC))) return st;
    if ((st = ensure(c, c->s_H, nH * rb))) return st;
    if ((st = emi_hess_dev(c, c->s_X.p, c->s_U.p, c->s_LF.p, c->s_LC.p, sigma, c->s_H.p))) return st;
    return download_real(c, H, c->s_H.p, nH);
}

// ---- the adjoint pass: Lagrangian gradient and KKT certificate (emi_adjoint.hip) ----
// a null context on a box without a device is "no device", not a bad argument: there is no host path to fall back to
static int adj_null_ctx() {
    int n = 0;
    return (hipGetDeviceCount(&n) != hipSuccess || n <= 0) ? EMI_ERR_NO_DEVICE : EMI_ERR_ARG;
}

// total: the caller is one of the emi_*_total_* entry points, which fold the delayed values' adjoints onto their sources
static int adj_ready(emi_ctx_t c, const char* who, bool total = false) {
    int st = ready(c);
    if (st) return st;
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: fp32 contexts have no adjoint pass (the certificate is an fp64 figure)", who);
    if (c->nch > 0 && !total)
        return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts with delays (emi_set_delays) take emi_lagr_grad_total_* / emi_kkt_certificate_total_*, "
                    "which fold the adjoints of the delayed values onto their sources", who);
    if (c->points_only) return fail(c, EMI_ERR_STATE, "%s: the mesh has no differentiation matrix (points-only mesh)", who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->adj_dirty) {
        const int M = c->M, ldt = M + (M & 1);
        if ((st = ensure(c, c->d_adjDT, (size_t)M * ldt * 8))) return st;
        HIP_TRY(c, emi::launch_adjoint_transpose((const double*)c->d_D.p, (double*)c->d_adjDT.p, M, ldt, ldt, 1, false, c->stream));
        c->adj_dirty = false;
    }
    if (c->nch > 0 && (c->adjw_dirty || c->delay_dirty)) {      // (an adjoint call may be the first use of W on this mesh)
        const int M = c->M, ldt = M + (M & 1), nd = std::max(c->xh - 1, c->uh);
        if ((st = ensure_delay_matrices(c))) return st;
        if ((st = ensure(c, c->d_adjWT, (size_t)M * nd * ldt * 8))) return st;
        HIP_TRY(c, emi::launch_adjoint_transpose((const double*)c->d_W.p, (double*)c->d_adjWT.p, M, ldt, nd * ldt, nd, true, c->stream));
        c->adjw_dirty = false;
    }
    if (c->adj_pvars != c->pvars || (!c->pvars.empty() && !c->d_adj_pvars.p)) {
        if ((st = upload_bytes(c, c->d_adj_pvars, c->pvars.data(), c->pvars.size() * sizeof(int)))) return st;
        c->adj_pvars = c->pvars;
    }
    return EMI_OK;
}

// G[B][ns+nc][M] on the node variables of the model (the extended ones of a context with delays); the context is adj_ready
static int lagr_grad_launch(emi_ctx_t c, const void* dVALS, const void* dLamF, const void* dLamC, double sigma, void* dG) {
    int st;
    emi::AdjointArgs a;
    a.VALS = (const double*)dVALS; a.lamF = (const double*)dLamF; a.lamC = np_total(c) > 0 ? (const double*)dLamC : nullptr;
    a.DT = (const double*)c->d_adjDT.p; a.pvars = (const int*)c->d_adj_pvars.p; a.G = (double*)dG;
    a.B = c->B; a.M = c->M; a.ldt = c->M + (c->M & 1); a.ns = c->ns; a.nc = c->nc;
    a.np_table = c->np; a.np_traced = c->np_model; a.pw = c->np_model > 0 ? (int)c->pvars.size() : 0;
    a.px = c->px; a.py = c->py; a.nvals = nvals_of(c); a.sigma = sigma; a.add_op = 1;
    if (!emi::adjoint_side_by_side(c->B, c->ns, c->M)) {
        HIP_TRY(c, emi::launch_adjoint_op(a, c->stream));
        HIP_TRY(c, emi::launch_adjoint_nodes(a, c->stream));
        return EMI_OK;
    }
    // Large batches: the product (matrix pipe) on the second stream BESIDE the node kernel (HBM) -- they share nothing until the last
    // addition.  The product writes its own [B][ns][M] block; a third, short kernel adds it onto the state rows: the same last
    // addition as in the back-to-back form, so both forms give the same bits.
    if ((st = need_stream2(c))) return st;
    if ((st = ensure(c, c->d_adj_op, (size_t)c->B * c->ns * c->M * 8))) return st;
    emi::AdjointArgs op = a;
    op.G = (double*)c->d_adj_op.p;
    op.nc = 0;                                       // rows (instance * ns + state) of the block
    a.add_op = 0;
    HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));          // the inputs (and the previous call's last addition) are done
    HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    HIP_TRY(c, emi::launch_adjoint_op(op, c->stream2));
    HIP_TRY(c, hipEventRecord(c->ev_join, c->stream2));
    HIP_TRY(c, emi::launch_adjoint_nodes(a, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    HIP_TRY(c, emi::launch_adjoint_add((const double*)c->d_adj_op.p, (double*)dG, c->B, c->ns, c->ns + c->nc, c->M, c->stream));
    return EMI_OK;
}

int emi_lagr_grad_dev(emi_ctx_t c, const void* dVALS, const void* dLamF, const void* dLamC, double sigma, void* dG) {
    if (!c) return adj_null_ctx();
    int st = adj_ready(c, "emi_lagr_grad");
    if (st) return st;
    if (!dVALS || !dLamF || !dG || (np_total(c) > 0 && !dLamC)) return fail(c, EMI_ERR_ARG, "emi_lagr_grad: null device pointer");
    return lagr_grad_launch(c, dVALS, dLamF, dLamC, sigma, dG);
}

// The gradient with respect to the trajectory of a context with delays.  Gx on the extended variables as above (workspace), then
// per class of sources one product on the matrix pipe: rows (instance, source), K = the node ranges of the delay indices one after
// the other against the transposed stack of W, last addition Gx[source] + product, stored into the caller's G[B][ns+ncf][M].
// One stream, back to back; every entry has one writer and a fixed summation order.
int emi_lagr_grad_total_dev(emi_ctx_t c, const void* dVALS, const void* dLamF, const void* dLamC, double sigma, void* dG, void* dGdel) {
    if (!c) return adj_null_ctx();
    int st = adj_ready(c, "emi_lagr_grad_total", true);
    if (st) return st;
    if (!dVALS || !dLamF || !dG || (np_total(c) > 0 && !dLamC)) return fail(c, EMI_ERR_ARG, "emi_lagr_grad_total: null device pointer");
    if (c->nch == 0) return lagr_grad_launch(c, dVALS, dLamF, dLamC, sigma, dG);
    const int M = c->M, B = c->B, ns = c->ns, nv = c->ns + c->nc, ncf = c->nc - c->nch, nf = ns + ncf, ldt = M + (M & 1);
    const int nd = std::max(c->xh - 1, c->uh), nxs = std::max(c->xh - 1, 0);
    if ((st = ensure(c, c->d_adj_Gx, (size_t)B * nv * M * 8))) return st;
    const double* Gx = (const double*)c->d_adj_Gx.p;
    if ((st = lagr_grad_launch(c, dVALS, dLamF, dLamC, sigma, c->d_adj_Gx.p))) return st;
    const size_t row = (size_t)M * 8;
    // rows [row0, row0 + n) of every instance of Gx -> rows [dst0, ..) of a [B][dst_rows][M] array
    auto copy_rows = [&](void* dst, int dst_rows, int dst0, int row0, int n) {
        return hipMemcpy2DAsync((double*)dst + (size_t)dst0 * M, (size_t)dst_rows * row, Gx + (size_t)row0 * M, (size_t)nv * row, (size_t)n * row, B,
                                hipMemcpyDeviceToDevice, c->stream);
    };
    auto fold = [&](int src0, int nsrc, int slot0, int nseg) {
        emi::AdjointOpArgs o;
        o.A = Gx; o.Bop = (const double*)c->d_adjWT.p; o.add = Gx; o.out = (double*)dG;
        o.R = B * nsrc; o.rpi = nsrc; o.M = M; o.ldt = ldt; o.nseg = nseg; o.ldb = nd * ldt;
        o.a_inst = nv; o.a_row0 = slot0; o.a_seg = nsrc; o.out_inst = nf; o.out_row0 = src0; o.add_inst = nv; o.add_row0 = src0;
        return emi::launch_adjoint_product(o, c->adj_fold_tile, c->stream);
    };
    if (nxs > 0) HIP_TRY(c, fold(0, ns, nf, nxs));              // states: copies x(t - i dt), i = 1 .. xh - 1, in slots nf + (i - 1) ns + state
    else HIP_TRY(c, copy_rows(dG, nf, 0, 0, ns));
    if (c->uh > 0) HIP_TRY(c, fold(ns, ncf, nf + nxs * ns, c->uh));   // controls: u(t - i dt), i = 1 .. uh, behind the states' copies
    else HIP_TRY(c, copy_rows(dG, nf, ns, ns, ncf));
    if (dGdel) HIP_TRY(c, copy_rows(dGdel, c->nch, 0, nf, c->nch));
    return EMI_OK;
}

// total: emi_lagr_grad_total_host (G on the free variables, Gdel the adjoints of the delayed values); a context the plain form
// accepts has no delayed values, so the sizes below are the same figures for both
static int lagr_grad_host(emi_ctx_t c, bool total, const double* VALS, const double* LamF, const double* LamC, double sigma, double* G,
                          double* Gdel) {
    if (!c) return adj_null_ctx();
    const char* who = total ? "emi_lagr_grad_total_host" : "emi_lagr_grad_host";
    int st = adj_ready(c, who, total);
    if (st) return st;
    if (!VALS || !LamF || !G || (np_total(c) > 0 && !LamC)) return fail(c, EMI_ERR_ARG, "%s: null pointer", who);
    const size_t M = c->M, B = c->B, nf = c->ns + c->nc - c->nch;
    const size_t nV = B * nvals_of(c) * M, nF = B * c->ns * M, nC = B * np_total(c) * M, nG = B * nf * M, nGd = B * c->nch * M;
    c->keep.written(c->s_VALS.p);           // the caller's VALS replace what an evaluation left in the staging buffer
    if ((st = upload_real(c, c->s_VALS, VALS, nV))) return st;
    c->keep.written(c->s_VALS.p);
    if ((st = upload_real(c, c->s_LF, LamF, nF))) return st;
    if (nC && (st = upload_real(c, c->s_LC, LamC, nC))) return st;
    if ((st = ensure(c, c->s_G, nG * 8))) return st;
    const bool del = total && Gdel && nGd > 0;
    if (del && (st = ensure(c, c->s_Gdel, nGd * 8))) return st;
    if ((st = total ? emi_lagr_grad_total_dev(c, c->s_VALS.p, c->s_LF.p, c->s_LC.p, sigma, c->s_G.p, del ? c->s_Gdel.p : nullptr)
                    : emi_lagr_grad_dev(c, c->s_VALS.p, c->s_LF.p, c->s_LC.p, sigma, c->s_G.p)))
        return st;
    if (del && (st = download_real(c, Gdel, c->s_Gdel.p, nGd))) return st;
    return download_real(c, G, c->s_G.p, nG);
}

int emi_lagr_grad_total_host(emi_ctx_t c, const double* VALS, const double* LamF, const double* LamC, double sigma, double* G, double* Gdel) {
    return lagr_grad_host(c, true, VALS, LamF, LamC, sigma, G, Gdel);
}

int emi_lagr_grad_host(emi_ctx_t c, const double* VALS, const double* LamF, const double* LamC, double sigma, double* G) {
    return lagr_grad_host(c, false, VALS, LamF, LamC, sigma, G, nullptr);
}

// the certificate on the free variables: G, U, zl, zu hold nf = ns + nc - n_delayed variables (total: the folded gradient)
static int kkt_certificate_launch(emi_ctx_t c, bool total, const void* dX, const void* dU, const void* dRES, const void* dVALS,
                                  const void* dLamF, const void* dLamC, double sigma, const void* dZl, const void* dZu, int nsets,
                                  const double* cl, const double* cu, void* dCert, void* dG, void* dGdel) {
    if (!c) return adj_null_ctx();
    int st = adj_ready(c, total ? "emi_kkt_certificate_total" : "emi_kkt_certificate", total);
    if (st) return st;
    const int np = np_total(c), ncf = c->nc - c->nch;
    if (!dX || !dU || !dRES || !dVALS || !dLamF || !dZl || !dZu || !dCert || (np > 0 && (!dLamC || !cl || !cu)))
        return fail(c, EMI_ERR_ARG, "emi_kkt_certificate: null pointer");
    if (nsets != 1 && nsets != c->B) return fail(c, EMI_ERR_ARG, "emi_kkt_certificate: %d bound sets, batch is %d", nsets, c->B);
    if (!dG) {
        if ((st = ensure(c, c->d_adj_G, (size_t)c->B * (c->ns + ncf) * c->M * 8))) return st;
        dG = c->d_adj_G.p;
    }
    if (np > 0) {
        if ((st = ensure(c, c->d_adj_c, (size_t)2 * np * 8))) return st;
        // pageable host memory: the copies are staged before the calls return, the caller's arrays are free again
        HIP_TRY(c, hipMemcpyAsync(c->d_adj_c.p, cl, (size_t)np * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync((double*)c->d_adj_c.p + np, cu, (size_t)np * 8, hipMemcpyHostToDevice, c->stream));
    }
    if ((st = total ? emi_lagr_grad_total_dev(c, dVALS, dLamF, dLamC, sigma, dG, dGdel) : emi_lagr_grad_dev(c, dVALS, dLamF, dLamC, sigma, dG)))
        return st;
    emi::CertArgs a;
    a.X = (const double*)dX; a.U = (const double*)dU; a.RES = (const double*)dRES; a.VALS = (const double*)dVALS;
    a.lamF = (const double*)dLamF; a.lamC = np > 0 ? (const double*)dLamC : nullptr; a.G = (const double*)dG;
    a.zl = (const double*)dZl; a.zu = (const double*)dZu;
    a.cl = (const double*)c->d_adj_c.p; a.cu = np > 0 ? (const double*)c->d_adj_c.p + np : nullptr;
    a.cert = (double*)dCert;
    a.B = c->B; a.M = c->M; a.ns = c->ns; a.nc = ncf; a.np = np; a.nres = nres_of(c); a.nvals = nvals_of(c); a.nsets = nsets;
    a.ncg = c->ns + c->nc;                             // gmax: a scale figure, over the cost gradient on all node variables
    a.sigma = sigma;
    HIP_TRY(c, emi::launch_kkt_certificate(a, c->stream));
    return EMI_OK;
}

int emi_kkt_certificate_dev(emi_ctx_t c, const void* dX, const void* dU, const void* dRES, const void* dVALS, const void* dLamF,
                            const void* dLamC, double sigma, const void* dZl, const void* dZu, int nsets, const double* cl,
                            const double* cu, void* dCert, void* dG) {
    return kkt_certificate_launch(c, false, dX, dU, dRES, dVALS, dLamF, dLamC, sigma, dZl, dZu, nsets, cl, cu, dCert, dG, nullptr);
}

int emi_kkt_certificate_total_dev(emi_ctx_t c, const void* dX, const void* dU, const void* dRES, const void* dVALS, const void* dLamF,
                                  const void* dLamC, double sigma, const void* dZl, const void* dZu, int nsets, const double* cl,
                                  const double* cu, void* dCert, void* dG, void* dGdel) {
    return kkt_certificate_launch(c, true, dX, dU, dRES, dVALS, dLamF, dLamC, sigma, dZl, dZu, nsets, cl, cu, dCert, dG, dGdel);
}

static int kkt_certificate_host(emi_ctx_t c, bool total, const double* X, const double* U, const double* LamF, const double* LamC,
                                double sigma, const double* zl, const double* zu, int nsets, const double* cl, const double* cu,
                                double* cert, double* G, double* Gdel) {
    if (!c) return adj_null_ctx();
    int st = adj_ready(c, total ? "emi_kkt_certificate_total_host" : "emi_kkt_certificate_host", total);
    if (st) return st;
    const int np = np_total(c);
    if (!X || !U || !LamF || !zl || !zu || !cert || (np > 0 && (!LamC || !cl || !cu)))
        return fail(c, EMI_ERR_ARG, "emi_kkt_certificate_host: null pointer");
    if (nsets != 1 && nsets != c->B) return fail(c, EMI_ERR_ARG, "emi_kkt_certificate_host: %d bound sets, batch is %d", nsets, c->B);
    const size_t M = c->M, B = c->B, ncf = c->nc - c->nch, nv = c->ns + ncf;      // the free variables: what X, U, zl, zu and G hold
    const size_t nX = B * c->ns * M, nU = B * ncf * M, nR = B * nres_of(c) * M, nV = B * nvals_of(c) * M, nC = B * np * M, nG = B * nv * M;
    const size_t nGd = B * c->nch * M;
    const bool del = total && Gdel && nGd > 0;
    if (del && (st = ensure(c, c->s_Gdel, nGd * 8))) return st;
    if ((st = upload_real(c, c->s_X, X, nX))) return st;
    if ((st = upload_real(c, c->s_U, U, nU))) return st;
    if ((st = upload_real(c, c->s_LF, LamF, nX))) return st;
    if (nC && (st = upload_real(c, c->s_LC, LamC, nC))) return st;
    if ((st = upload_real(c, c->s_zl, zl, (size_t)nsets * nv * M))) return st;
    if ((st = upload_real(c, c->s_zu, zu, (size_t)nsets * nv * M))) return st;
    if ((st = ensure(c, c->s_RES, nR * 8))) return st;
    if ((st = ensure_vals_staging(c, nV * 8))) return st;
    if ((st = ensure(c, c->s_COST, B * 8))) return st;
    if ((st = ensure(c, c->s_G, nG * 8))) return st;
    if ((st = ensure(c, c->s_cert, B * 6 * 8))) return st;
    if ((st = emi_eval_dev(c, c->s_X.p, c->s_U.p, c->s_RES.p, c->s_VALS.p, c->s_COST.p, EMI_EVAL_ALL))) return st;
    if ((st = kkt_certificate_launch(c, total, c->s_X.p, c->s_U.p, c->s_RES.p, c->s_VALS.p, c->s_LF.p, c->s_LC.p, sigma, c->s_zl.p, c->s_zu.p,
                                     nsets, cl, cu, c->s_cert.p, c->s_G.p, del ? c->s_Gdel.p : nullptr))) return st;
    if ((st = download_real(c, cert, c->s_cert.p, B * 6))) return st;
    if (G && (st = download_real(c, G, c->s_G.p, nG))) return st;
    if (del && (st = download_real(c, Gdel, c->s_Gdel.p, nGd))) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

int emi_kkt_certificate_host(emi_ctx_t c, const double* X, const double* U, const double* LamF, const double* LamC, double sigma,
                             const double* zl, const double* zu, int nsets, const double* cl, const double* cu, double* cert,
                             double* G) {
    return kkt_certificate_host(c, false, X, U, LamF, LamC, sigma, zl, zu, nsets, cl, cu, cert, G, nullptr);
}

int emi_kkt_certificate_total_host(emi_ctx_t c, const double* X, const double* U, const double* LamF, const double* LamC, double sigma,
                                   const double* zl, const double* zu, int nsets, const double* cl, const double* cu, double* cert,
                                   double* G, double* Gdel) {
    return kkt_certificate_host(c, true, X, U, LamF, LamC, sigma, zl, zu, nsets, cl, cu, cert, G, Gdel);
}

// emi_kkt_factor / emi_kkt_factor_dev: the blocks in host or in device memory, everything else the same
static int kkt_factor_from(emi_ctx_t c, const char* what, const void* Qblk, const void* Jblk, const void* fixed, double dc, int* info,
                           bool blocks_on_device) {
    if (!c) return EMI_ERR_ARG;
    if (c->M <= 0 || c->model < 0) return fail(c, EMI_ERR_STATE, "%s: mesh and model must be set", what);
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->points_only) return fail(c, EMI_ERR_STATE, "%s: the mesh has no differentiation matrix", what);
    if (!Qblk || !Jblk || !fixed || !info || !(dc >= 0.0)) return fail(c, EMI_ERR_ARG, "%s: bad argument", what);
    HIP_TRY(c, hipSetDevice(c->device));
    std::string err;
    const int st = emi::kkt_factor(&c->kkt, c->stream, (const double*)c->d_D.p, c->M, c->ns, c->ns + c->nc, (const double*)Qblk,
                                   (const double*)Jblk, (const unsigned char*)fixed, dc, c->kkt_method, info, &err, blocks_on_device);
    if (st) c->err = err;
    return st;
}

int emi_kkt_factor(emi_ctx_t c, const double* Qblk, const double* Jblk, const unsigned char* fixed, double dc,
                   int* info) {
    return kkt_factor_from(c, "emi_kkt_factor", Qblk, Jblk, fixed, dc, info, false);
}

int emi_kkt_factor_dev(emi_ctx_t c, const void* dQblk, const void* dJblk, const void* dFixed, double dc, int* info) {
    return kkt_factor_from(c, "emi_kkt_factor_dev", dQblk, dJblk, dFixed, dc, info, true);
}

// ---- node blocks of the Newton step: assembly, screen and eigen-fix over [instance][node] (emi_kkt_blocks.hip) -----------------
int emi_kkt_blocks_rows(emi_ctx_t c, int np, const int* row_ptr, const int* var, const int* entry) {
    if (!c) return EMI_ERR_ARG;
    if (c->model < 0) return fail(c, EMI_ERR_STATE, "emi_kkt_blocks_rows: the model must be set");
    if (np < 0 || !row_ptr || row_ptr[0] != 0) return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_rows: bad argument");
    const int nv = c->ns + c->nc, nvals = nvals_of(c);
    for (int j = 0; j < np; ++j)
        if (row_ptr[j + 1] < row_ptr[j]) return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_rows: row_ptr decreases at row %d", j);
    const int n = row_ptr[np];
    if (n > 0 && (!var || !entry)) return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_rows: bad argument");
    for (int a = 0; a < n; ++a)
        if (var[a] < 0 || var[a] >= nv || entry[a] < 0 || entry[a] >= nvals)
            return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_rows: pair %d (variable %d, VALS entry %d) is out of range (%d variables, %d entries)",
                        a, var[a], entry[a], nv, nvals);
    c->blk_row_ptr.assign(row_ptr, row_ptr + np + 1);
    c->blk_var.assign(var, var + n);
    c->blk_entry.assign(entry, entry + n);
    c->blk_rows_set = true;
    c->blk_key.clear();
    return EMI_OK;
}

namespace {

// the per-entry term lists of the assembly kernel on the device: for every packed entry of the block, the products
// SigT[row] VALS[ea] VALS[eb] that the host loop adds to it, in that loop's order (rows ascending, pairs (a, b <= a) in list order)
// the (variable, VALS entry) pairs of every path row: the caller's list (emi_kkt_blocks_rows) or the record table's default
int path_row_list(emi_ctx_t c, const char* what, std::vector<int>& ptr, std::vector<int>& var, std::vector<int>& ent) {
    const int nv = c->ns + c->nc, np = np_total(c), nvals = nvals_of(c);
    if (c->blk_rows_set) {
        if ((int)c->blk_row_ptr.size() != np + 1)
            return fail(c, EMI_ERR_STATE, "%s: the row list (emi_kkt_blocks_rows) has %d rows, the context %d", what, (int)c->blk_row_ptr.size() - 1, np);
        ptr = c->blk_row_ptr; var = c->blk_var; ent = c->blk_entry;
        for (size_t a = 0; a < var.size(); ++a)         // (the model may have changed since the list was given)
            if (var[a] >= nv || ent[a] >= nvals) return fail(c, EMI_ERR_STATE, "%s: the row list does not fit the context's layout any more", what);
    } else {
        if (c->np_model > 0)
            return fail(c, EMI_ERR_STATE, "%s: the context has traced path rows and no row list (emi_kkt_blocks_rows)", what);
        ptr.push_back(0);
        for (int j = 0; j < c->np; ++j) {
            var.push_back(c->px); ent.push_back(c->ns * nv + 2 * j);
            var.push_back(c->py); ent.push_back(c->ns * nv + 2 * j + 1);
            ptr.push_back((int)var.size());
        }
    }
    return EMI_OK;
}

int blocks_terms(emi_ctx_t c, const char* what) {
    const int nv = c->ns + c->nc, nh = nv * (nv + 1) / 2, np = np_total(c), nvals = nvals_of(c);
    std::vector<int> ptr, var, ent;
    EMI_TRY(path_row_list(c, what, ptr, var, ent));
    std::vector<int> key = {nv, np, nvals, (int)c->blk_rows_set};
    key.insert(key.end(), ptr.begin(), ptr.end());
    key.insert(key.end(), var.begin(), var.end());
    key.insert(key.end(), ent.begin(), ent.end());
    if (key == c->blk_key) return EMI_OK;
    std::vector<std::vector<int>> per(nh);      // (row, ea, eb) triples of every entry
    for (int j = 0; j < np; ++j)
        for (int a = ptr[j]; a < ptr[j + 1]; ++a)
            for (int b = ptr[j]; b <= a; ++b) {
                const int hi = std::max(var[a], var[b]), lo = std::min(var[a], var[b]);
                std::vector<int>& t = per[hi * (hi + 1) / 2 + lo];
                t.push_back(j); t.push_back(ent[a]); t.push_back(ent[b]);
            }
    std::vector<int> tp(nh + 1, 0), tr, ta, tb;
    for (int e = 0; e < nh; ++e) {
        for (size_t i = 0; i < per[e].size(); i += 3) { tr.push_back(per[e][i]); ta.push_back(per[e][i + 1]); tb.push_back(per[e][i + 2]); }
        tp[e + 1] = (int)tr.size();
    }
    const size_t nt = std::max<size_t>(tr.size(), 1);
    tr.resize(nt); ta.resize(nt); tb.resize(nt);
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // a launch in flight may still read the old lists
    HIP_TRY(c, c->blk_term_ptr.reserve(tp.size()));
    HIP_TRY(c, c->blk_term_row.reserve(nt));
    HIP_TRY(c, c->blk_term_ea.reserve(nt));
    HIP_TRY(c, c->blk_term_eb.reserve(nt));
    HIP_TRY(c, hipMemcpyAsync(c->blk_term_ptr.p, tp.data(), tp.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->blk_term_row.p, tr.data(), nt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->blk_term_ea.p, ta.data(), nt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->blk_term_eb.p, tb.data(), nt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // (the sources are locals)
    c->blk_key = key;
    return EMI_OK;
}

int blocks_check(emi_ctx_t c, const char* what) {
    if (c->M <= 0 || c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: mesh, model and batch must be set", what);
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->ns + c->nc > 16) return fail(c, EMI_ERR_UNSUPPORTED, "%s: node blocks of up to 16 variables (this model has %d)", what, c->ns + c->nc);
    return EMI_OK;
}

}  // namespace

int emi_kkt_blocks_dev(emi_ctx_t c, const void* dH, const void* dVALS, const void* dSigma, const void* dSigT, const void* dFixed,
                       double dw_shift, void* dQexact, void* dQ, int max_mods, void* dCount, void* dNode, void* dDelta, void* dVec,
                       void* dWorst) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(blocks_check(c, "emi_kkt_blocks_dev"));
    const int nv = c->ns + c->nc, np = np_total(c);
    if (!dH || !dVALS || !dSigma || !dFixed || !dQ || !dCount || !dWorst || max_mods < 0 || (np > 0 && !dSigT) ||
        (max_mods > 0 && (!dNode || !dDelta || !dVec)) || !(dw_shift >= 0.0))
        return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_dev: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    EMI_TRY(blocks_terms(c, "emi_kkt_blocks_dev"));
    const size_t BM = (size_t)c->B * c->M;
    HIP_TRY(c, c->blk_flag.reserve(BM));
    HIP_TRY(c, c->blk_list.reserve(BM));
    HIP_TRY(c, c->blk_cnt.reserve(BM));
    HIP_TRY(c, c->blk_nflag.reserve((size_t)c->B));
    HIP_TRY(c, c->blk_tworst.reserve(BM));
    HIP_TRY(c, c->blk_tdelta.reserve(BM * nv));
    // (room for EVERY block failing with all nv eigenvalues negative: how many fail is known on the device only, and a host
    //  round trip to size it is what this call avoids.  B M nv^2 doubles: 34 MB at 64 x 1024 nodes x 8, 2 GiB at 1024 x 1024 x 16)
    HIP_TRY(c, c->blk_tvec.reserve(BM * nv * nv));
    emi::BlocksArgs a{};
    a.H = (const double*)dH; a.VALS = (const double*)dVALS; a.Sigma = (const double*)dSigma; a.SigT = (const double*)dSigT;
    a.fixed = (const unsigned char*)dFixed; a.dw_shift = dw_shift; a.Qexact = (double*)dQexact; a.Q = (double*)dQ;
    a.max_mods = max_mods; a.count = (int*)dCount; a.node = (int*)dNode; a.delta = (double*)dDelta; a.vec = (double*)dVec;
    a.worst = (double*)dWorst;
    a.B = c->B; a.M = c->M; a.nv = nv; a.np = np; a.nvals = nvals_of(c); a.generic = c->blk_generic;
    a.term_ptr = c->blk_term_ptr.p; a.term_row = c->blk_term_row.p; a.term_ea = c->blk_term_ea.p; a.term_eb = c->blk_term_eb.p;
    a.flag = c->blk_flag.p; a.list = c->blk_list.p; a.nflag = c->blk_nflag.p; a.cnt = c->blk_cnt.p;
    a.tdelta = c->blk_tdelta.p; a.tvec = c->blk_tvec.p; a.tworst = c->blk_tworst.p;
    HIP_TRY(c, emi::launch_kkt_blocks(a, c->stream));
    return EMI_OK;
}

int emi_kkt_blocks_host(emi_ctx_t c, const double* H, const double* VALS, const double* Sigma, const double* SigT,
                        const unsigned char* fixed, double dw_shift, double* Qexact, double* Q, int max_mods, int* count, int* node,
                        double* delta, double* vec, double* worst) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(blocks_check(c, "emi_kkt_blocks_host"));
    const size_t B = (size_t)c->B, M = (size_t)c->M, nv = (size_t)(c->ns + c->nc), nh = nv * (nv + 1) / 2, np = (size_t)np_total(c);
    if (!H || !VALS || !Sigma || !fixed || !Q || !count || !worst || max_mods < 0 || (np > 0 && !SigT) ||
        (max_mods > 0 && (!node || !delta || !vec)))
        return fail(c, EMI_ERR_ARG, "emi_kkt_blocks_host: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t mm = (size_t)max_mods;
    EMI_TRY(upload_bytes(c, c->sb_H, H, B * nh * M * 8));
    EMI_TRY(upload_bytes(c, c->sb_V, VALS, B * nvals_of(c) * M * 8));
    EMI_TRY(upload_bytes(c, c->sb_Sg, Sigma, B * nv * M * 8));
    if (np) EMI_TRY(upload_bytes(c, c->sb_St, SigT, B * np * M * 8));
    EMI_TRY(upload_bytes(c, c->sb_fx, fixed, B * nv * M));
    EMI_TRY(ensure(c, c->sb_Qx, B * nh * M * 8));
    EMI_TRY(ensure(c, c->sb_Q, B * nh * M * 8));
    EMI_TRY(ensure(c, c->sb_cnt, B * sizeof(int)));
    EMI_TRY(ensure(c, c->sb_worst, B * 8));
    EMI_TRY(ensure(c, c->sb_node, std::max<size_t>(B * mm, 1) * sizeof(int)));
    EMI_TRY(ensure(c, c->sb_delta, std::max<size_t>(B * mm, 1) * 8));
    EMI_TRY(ensure(c, c->sb_vec, std::max<size_t>(B * mm * nv, 1) * 8));
    EMI_TRY(emi_kkt_blocks_dev(c, c->sb_H.p, c->sb_V.p, c->sb_Sg.p, np ? c->sb_St.p : nullptr, c->sb_fx.p, dw_shift,
                               Qexact ? c->sb_Qx.p : nullptr, c->sb_Q.p, max_mods, c->sb_cnt.p, c->sb_node.p, c->sb_delta.p, c->sb_vec.p,
                               c->sb_worst.p));
    auto down = [&](void* dst, const DevBuf& src, size_t bytes) {
        return !dst || !bytes ? hipSuccess : hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, c->stream);
    };
    HIP_TRY(c, down(Qexact, c->sb_Qx, B * nh * M * 8));
    HIP_TRY(c, down(Q, c->sb_Q, B * nh * M * 8));
    HIP_TRY(c, down(count, c->sb_cnt, B * sizeof(int)));
    HIP_TRY(c, down(worst, c->sb_worst, B * 8));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // only what the kernels wrote: the first min(count, max_mods) entries of every instance
    for (size_t b = 0; b < B && mm > 0; ++b) {
        const size_t n = std::min<size_t>((size_t)std::max(count[b], 0), mm);
        if (n == 0) continue;
        HIP_TRY(c, hipMemcpyAsync(node + b * mm, (const int*)c->sb_node.p + b * mm, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(delta + b * mm, (const double*)c->sb_delta.p + b * mm, n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(vec + b * mm * nv, (const double*)c->sb_vec.p + b * mm * nv, n * nv * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EMI_OK;
}

// ---- the array arithmetic of an interior-point iteration over [instance][node] (emi_ipm.hip) ---------------------------------------
namespace {

int ipm_check(emi_ctx_t c, const char* what) {
    if (c->M <= 0 || c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: mesh, model and batch must be set", what);
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->nch > 0) return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts with delays are not taken", what);
    if (c->ns + c->nc > 16) return fail(c, EMI_ERR_UNSUPPORTED, "%s: up to 16 variables per node (this model has %d)", what, c->ns + c->nc);
    return EMI_OK;
}

// the path-row lists by row and by variable on the device (built once per list)
int ipm_lists(emi_ctx_t c, const char* what, emi::IpmArgs& a) {
    const int nv = c->ns + c->nc, np = np_total(c);
    std::vector<int> ptr, var, ent;
    EMI_TRY(path_row_list(c, what, ptr, var, ent));
    std::vector<int> key = {nv, np, nvals_of(c)};
    key.insert(key.end(), ptr.begin(), ptr.end());
    key.insert(key.end(), var.begin(), var.end());
    key.insert(key.end(), ent.begin(), ent.end());
    const int n = (int)var.size();
    if (key != c->ipm_key) {
        std::vector<int> all(ptr);                                  // rptr [np + 1]
        all.insert(all.end(), var.begin(), var.end());              // rvar [n]
        all.insert(all.end(), ent.begin(), ent.end());              // rent [n]
        std::vector<int> vptr(nv + 1, 0), vrow, vent;
        for (int v = 0; v < nv; ++v) {
            for (int j = 0; j < np; ++j)
                for (int t = ptr[j]; t < ptr[j + 1]; ++t)
                    if (var[t] == v) { vrow.push_back(j); vent.push_back(ent[t]); }
            vptr[v + 1] = (int)vrow.size();
        }
        all.insert(all.end(), vptr.begin(), vptr.end());
        all.insert(all.end(), vrow.begin(), vrow.end());
        all.insert(all.end(), vent.begin(), vent.end());
        HIP_TRY(c, hipStreamSynchronize(c->stream));        // a launch in flight may still read the old lists
        HIP_TRY(c, c->ipm_lists.reserve(all.size()));
        HIP_TRY(c, hipMemcpyAsync(c->ipm_lists.p, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));        // (the source is a local)
        c->ipm_key = key;
        c->ipm_npairs = n;
    }
    const int* p = c->ipm_lists.p;
    a.rptr = p; a.rvar = p + np + 1; a.rent = a.rvar + n;
    a.vptr = a.rent + n; a.vrow = a.vptr + nv + 1; a.vent = a.vrow + n;
    return EMI_OK;
}

// sizes, bounds and per-instance scalars of a call; the row bounds go to the device when they differ from what is there
int ipm_common(emi_ctx_t c, const char* what, const emi_ipm_bounds_t* bd, const void* dPar, emi::IpmArgs& a) {
    const int np = np_total(c);
    a.B = c->B; a.M = c->M; a.ns = c->ns; a.nc = c->nc; a.np = np; a.nvals = nvals_of(c);
    a.par = (const double*)dPar;
    if (!bd) return EMI_OK;
    if (!bd->zl || !bd->zu || (bd->nsets != 1 && bd->nsets != c->B) || (np > 0 && (!bd->cl || !bd->cu)))
        return fail(c, EMI_ERR_ARG, "%s: bad bounds (zl, zu [nsets][nv][M] with nsets 1 or the batch; cl, cu [np])", what);
    a.zl = (const double*)bd->zl; a.zu = (const double*)bd->zu; a.nsets = bd->nsets;
    if (np > 0) {
        std::vector<double> h((size_t)5 * np);
        for (int j = 0; j < np; ++j) {
            const double cs = bd->cscale ? bd->cscale[j] : 1.0;
            if (!(cs > 0.0)) return fail(c, EMI_ERR_ARG, "%s: cscale[%d] must be positive", what, j);
            h[j] = bd->cl[j]; h[np + j] = bd->cu[j];
            h[2 * np + j] = bd->cl[j] > -1e19 ? cs * bd->cl[j] : bd->cl[j];
            h[3 * np + j] = bd->cu[j] < 1e19 ? cs * bd->cu[j] : bd->cu[j];
            h[4 * np + j] = cs;
        }
        if (h != c->ipm_crow_h || !c->ipm_crow.p) {
            // new bounds (once per problem, not per iteration): the launches that read the old values are drained before the buffer
            // may move, and the copy is complete before its source is touched again
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, c->ipm_crow.reserve(h.size()));
            c->ipm_crow_h = h;
            HIP_TRY(c, hipMemcpyAsync(c->ipm_crow.p, c->ipm_crow_h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        a.crow = c->ipm_crow.p;
    }
    return EMI_OK;
}

int ipm_partials(emi_ctx_t c, emi::IpmArgs& a) {
    HIP_TRY(c, c->ipm_part.reserve((size_t)c->B * emi::ipm_chunks(c->M) * emi::IPM_MAX_PARTIALS));
    a.part = c->ipm_part.p;
    return EMI_OK;
}

bool ipm_has_point(const emi_ipm_point_t* p, int nc, int np) { return p && p->X && (nc == 0 || p->U) && (np == 0 || (p->S && p->E1 && p->E2)); }
bool ipm_has_duals(const emi_ipm_duals_t* d, int np) {
    return d && d->LamF && d->ZL && d->ZU && (np == 0 || (d->Y && d->VL && d->VU && d->W1 && d->W2));
}
bool ipm_has_step(const emi_ipm_step_t* s, int np) {
    return s && s->DZLam && s->DZL && s->DZU && (np == 0 || (s->DS && s->DY && s->DE1 && s->DE2 && s->DVL && s->DVU && s->DW1 && s->DW2));
}
bool ipm_has_elim(const emi_ipm_elim_t* e, int np) { return e && e->Sigma && (np == 0 || (e->SigT && e->SigS && e->RhatS && e->Rt)); }
void ipm_set_point(emi::IpmArgs& a, const emi_ipm_point_t* p) { a.X = (double*)p->X; a.U = (double*)p->U; a.S = (double*)p->S; a.E1 = (double*)p->E1; a.E2 = (double*)p->E2; }
void ipm_set_trial(emi::IpmArgs& a, const emi_ipm_point_t* p) { a.tX = (double*)p->X; a.tU = (double*)p->U; a.tS = (double*)p->S; a.tE1 = (double*)p->E1; a.tE2 = (double*)p->E2; }
void ipm_set_duals(emi::IpmArgs& a, const emi_ipm_duals_t* d) {
    a.LF = (double*)d->LamF; a.Y = (double*)d->Y; a.ZL = (double*)d->ZL; a.ZU = (double*)d->ZU;
    a.VL = (double*)d->VL; a.VU = (double*)d->VU; a.W1 = (double*)d->W1; a.W2 = (double*)d->W2;
}
void ipm_set_step(emi::IpmArgs& a, const emi_ipm_step_t* s) {
    a.DZ = (double*)s->DZLam; a.DS = (double*)s->DS; a.DY = (double*)s->DY; a.DE1 = (double*)s->DE1; a.DE2 = (double*)s->DE2;
    a.DZL = (double*)s->DZL; a.DZU = (double*)s->DZU; a.DVL = (double*)s->DVL; a.DVU = (double*)s->DVU; a.DW1 = (double*)s->DW1; a.DW2 = (double*)s->DW2;
}
void ipm_set_elim(emi::IpmArgs& a, const emi_ipm_elim_t* e) {
    a.Sigma = (double*)e->Sigma; a.SigT = (double*)e->SigT; a.SigS = (double*)e->SigS; a.RhatS = (double*)e->RhatS; a.Rt = (double*)e->Rt;
}

}  // namespace

int emi_ipm_reduce_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dVALS, const void* dG,
                       const emi_ipm_bounds_t* bd, const void* dPar, const void* dDefRes, const void* dRowRes, const emi_ipm_elim_t* out,
                       void* dRhs) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_reduce_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !dRES || !dVALS || !dG || !bd || !dPar || !ipm_has_elim(out, np) || !dRhs)
        return fail(c, EMI_ERR_ARG, "emi_ipm_reduce_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_reduce_dev", bd, dPar, a));
    EMI_TRY(ipm_lists(c, "emi_ipm_reduce_dev", a));
    ipm_set_point(a, pt); ipm_set_duals(a, du); ipm_set_elim(a, out);
    a.RES = (const double*)dRES; a.VALS = (const double*)dVALS; a.G = (const double*)dG;
    a.DefRes = (const double*)dDefRes; a.RowRes = (const double*)dRowRes; a.Rhs = (double*)dRhs;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_REDUCE, a, c->stream));
    return EMI_OK;
}

int emi_ipm_expand_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dVALS, const emi_ipm_bounds_t* bd,
                       const void* dPar, const emi_ipm_elim_t* el, const void* dRs, const emi_ipm_step_t* st, void* dScal) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_expand_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !dVALS || !bd || !dPar || !ipm_has_elim(el, np) || !ipm_has_step(st, np) || !dScal)
        return fail(c, EMI_ERR_ARG, "emi_ipm_expand_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_expand_dev", bd, dPar, a));
    EMI_TRY(ipm_lists(c, "emi_ipm_expand_dev", a));
    EMI_TRY(ipm_partials(c, a));
    ipm_set_point(a, pt); ipm_set_duals(a, du); ipm_set_elim(a, el); ipm_set_step(a, st);
    a.VALS = (const double*)dVALS; a.rs = (const double*)dRs; a.out = (double*)dScal;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_EXPAND, a, c->stream));
    return EMI_OK;
}

int emi_ipm_trial_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_step_t* st, const void* dAlpha, const emi_ipm_point_t* trial) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_trial_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_point(trial, c->nc, np) || !st || !st->DZLam || (np > 0 && (!st->DS || !st->DE1 || !st->DE2)) || !dAlpha)
        return fail(c, EMI_ERR_ARG, "emi_ipm_trial_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_trial_dev", nullptr, nullptr, a));
    ipm_set_point(a, pt); ipm_set_trial(a, trial); ipm_set_step(a, st);
    a.apr = (const double*)dAlpha;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_TRIAL, a, c->stream));
    return EMI_OK;
}

int emi_ipm_merit_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const void* dRES, const void* dCOST, const emi_ipm_bounds_t* bd, const void* dPar,
                      const void* dRs, int reset, void* dOut) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_merit_dev"));
    if (!ipm_has_point(pt, c->nc, np_total(c)) || !dRES || !dCOST || !bd || !dPar || !dOut) return fail(c, EMI_ERR_ARG, "emi_ipm_merit_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_merit_dev", bd, dPar, a));
    EMI_TRY(ipm_partials(c, a));
    ipm_set_point(a, pt);
    a.RES = (const double*)dRES; a.COST = (const double*)dCOST; a.rs = (const double*)dRs; a.reset = reset ? 1 : 0; a.out = (double*)dOut;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_MERIT, a, c->stream));
    return EMI_OK;
}

int emi_ipm_accept_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_point_t* trial, const emi_ipm_duals_t* du, const emi_ipm_step_t* st,
                       const emi_ipm_bounds_t* bd, const void* dPar, const void* dApr, const void* dAdu, const void* dMask) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_accept_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_point(trial, c->nc, np) || !ipm_has_duals(du, np) || !ipm_has_step(st, np) || !bd || !dPar || !dApr || !dAdu)
        return fail(c, EMI_ERR_ARG, "emi_ipm_accept_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_accept_dev", bd, dPar, a));
    ipm_set_point(a, pt); ipm_set_trial(a, trial); ipm_set_duals(a, du); ipm_set_step(a, st);
    a.apr = (const double*)dApr; a.adu = (const double*)dAdu; a.mask = (const unsigned char*)dMask;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_ACCEPT, a, c->stream));
    return EMI_OK;
}

int emi_ipm_error_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dG,
                      const emi_ipm_bounds_t* bd, const void* dPar, void* dOut) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_error_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !dRES || !dG || !bd || !dPar || !dOut) return fail(c, EMI_ERR_ARG, "emi_ipm_error_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_error_dev", bd, dPar, a));
    EMI_TRY(ipm_partials(c, a));
    ipm_set_point(a, pt); ipm_set_duals(a, du);
    a.RES = (const double*)dRES; a.G = (const double*)dG; a.out = (double*)dOut;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_ERROR, a, c->stream));
    return EMI_OK;
}

int emi_ipm_start_dev(emi_ctx_t c, int phase, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const emi_ipm_bounds_t* bd,
                      const void* dPar, double bound_push, double bound_frac, void* dFixed, const void* dMask) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_start_dev"));
    const int np = np_total(c);
    bool ok = pt && du && bd && phase >= 0 && phase <= 2;
    if (ok && phase == 0) ok = pt->X && (c->nc == 0 || pt->U) && du->LamF && dFixed && bound_push > 0 && bound_frac > 0;
    if (ok && phase == 1) ok = ipm_has_point(pt, c->nc, np) && ipm_has_duals(du, np) && dRES && dPar && bound_push > 0 && bound_frac > 0;
    if (ok && phase == 2) ok = dPar && (np == 0 || (du->Y && du->W1 && du->W2));
    if (!ok) return fail(c, EMI_ERR_ARG, "emi_ipm_start_dev: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_start_dev", bd, dPar, a));
    ipm_set_point(a, pt); ipm_set_duals(a, du);
    a.RES = (const double*)dRES; a.fixedb = (unsigned char*)dFixed; a.mask = (const unsigned char*)dMask; a.push = bound_push; a.frac = bound_frac;
    HIP_TRY(c, emi::launch_ipm(phase == 0 ? emi::IPM_START_PUSH : phase == 1 ? emi::IPM_START_ROWS : emi::IPM_RESET_W, a, c->stream));
    return EMI_OK;
}

int emi_ipm_error_parts_dev(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dG,
                            const emi_ipm_bounds_t* bd, const void* dPar, void* dOut) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_error_parts_dev"));
    const int np = np_total(c);
    if (!ipm_has_point(pt, c->nc, np) || !ipm_has_duals(du, np) || !dRES || !dG || !bd || !dPar || !dOut)
        return fail(c, EMI_ERR_ARG, "emi_ipm_error_parts_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    emi::IpmArgs a{};
    EMI_TRY(ipm_common(c, "emi_ipm_error_parts_dev", bd, dPar, a));
    EMI_TRY(ipm_partials(c, a));
    ipm_set_point(a, pt); ipm_set_duals(a, du);
    a.RES = (const double*)dRES; a.G = (const double*)dG; a.out = (double*)dOut;
    HIP_TRY(c, emi::launch_ipm(emi::IPM_ERROR_PARTS, a, c->stream));
    return EMI_OK;
}

// ---- the _host forms: every array copied in, the _dev form run, what it writes copied out, synchronised -------------------------------
namespace {

// staging of one host-form call: device twins of the caller's host arrays (null stays null), the outputs copied back by finish()
struct IpmStager {
    emi_ctx_t c;
    size_t slot = 0;
    int status = EMI_OK;
    struct Out { void* host; void* dev; size_t bytes; };
    std::vector<Out> outs;
    explicit IpmStager(emi_ctx_t c_) : c(c_) {}
    void* place(const void* host, size_t bytes, bool in, bool out) {
        if (!host || status) return nullptr;
        if (slot == c->ipm_stage.size()) c->ipm_stage.emplace_back();
        DevBuf& b = c->ipm_stage[slot++];
        if (b.reserve(std::max<size_t>(bytes, 8)) != hipSuccess) { status = fail(c, EMI_ERR_HIP, "staging of a host-form call: out of device memory"); return nullptr; }
        if (in && bytes && hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            status = fail(c, EMI_ERR_HIP, "staging of a host-form call: copy failed");
            return nullptr;
        }
        if (out) outs.push_back({const_cast<void*>(host), b.p, bytes});
        return b.p;
    }
    int finish() {
        for (const Out& o : outs)
            if (o.bytes) HIP_TRY(c, hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return EMI_OK;
    }
};

struct IpmSizes {
    size_t X, U, row, var, kkt, res, vals, bnd, inst;
    IpmSizes(emi_ctx_t c, int nsets) {
        const size_t B = (size_t)c->B, M = (size_t)c->M, nv = (size_t)(c->ns + c->nc), np = (size_t)np_total(c);
        X = B * c->ns * M * 8; U = B * c->nc * M * 8; row = B * np * M * 8; var = B * nv * M * 8; kkt = B * (nv + c->ns) * M * 8;
        res = B * (c->ns + np) * M * 8; vals = B * (size_t)nvals_of(c) * M * 8; bnd = (size_t)std::max(nsets, 0) * nv * M * 8; inst = B * 8;
    }
};
emi_ipm_point_t stage_point(IpmStager& s, const IpmSizes& z, const emi_ipm_point_t* p, bool in, bool out) {
    emi_ipm_point_t d{};
    if (!p) return d;
    d.X = s.place(p->X, z.X, in, out); d.U = s.place(p->U, z.U, in, out);
    d.S = s.place(p->S, z.row, in, out); d.E1 = s.place(p->E1, z.row, in, out); d.E2 = s.place(p->E2, z.row, in, out);
    return d;
}
emi_ipm_duals_t stage_duals(IpmStager& s, const IpmSizes& z, const emi_ipm_duals_t* p, bool in, bool out) {
    emi_ipm_duals_t d{};
    if (!p) return d;
    d.LamF = s.place(p->LamF, z.X, in, out); d.Y = s.place(p->Y, z.row, in, out);
    d.ZL = s.place(p->ZL, z.var, in, out); d.ZU = s.place(p->ZU, z.var, in, out);
    d.VL = s.place(p->VL, z.row, in, out); d.VU = s.place(p->VU, z.row, in, out);
    d.W1 = s.place(p->W1, z.row, in, out); d.W2 = s.place(p->W2, z.row, in, out);
    return d;
}
// dz_in / dz_out: the solved step goes in and comes back with the fixed variables zeroed; the rest as `in` / `out` say
emi_ipm_step_t stage_step(IpmStager& s, const IpmSizes& z, const emi_ipm_step_t* p, bool dz_in, bool dz_out, bool in, bool out) {
    emi_ipm_step_t d{};
    if (!p) return d;
    d.DZLam = s.place(p->DZLam, z.kkt, dz_in, dz_out);
    d.DS = s.place(p->DS, z.row, in, out); d.DY = s.place(p->DY, z.row, in, out);
    d.DE1 = s.place(p->DE1, z.row, in, out); d.DE2 = s.place(p->DE2, z.row, in, out);
    d.DZL = s.place(p->DZL, z.var, in, out); d.DZU = s.place(p->DZU, z.var, in, out);
    d.DVL = s.place(p->DVL, z.row, in, out); d.DVU = s.place(p->DVU, z.row, in, out);
    d.DW1 = s.place(p->DW1, z.row, in, out); d.DW2 = s.place(p->DW2, z.row, in, out);
    return d;
}
emi_ipm_elim_t stage_elim(IpmStager& s, const IpmSizes& z, const emi_ipm_elim_t* p, bool in, bool out) {
    emi_ipm_elim_t d{};
    if (!p) return d;
    d.Sigma = s.place(p->Sigma, z.var, in, out); d.SigT = s.place(p->SigT, z.row, in, out); d.SigS = s.place(p->SigS, z.row, in, out);
    d.RhatS = s.place(p->RhatS, z.row, in, out); d.Rt = s.place(p->Rt, z.row, in, out);
    return d;
}
emi_ipm_bounds_t stage_bounds(IpmStager& s, const IpmSizes& z, const emi_ipm_bounds_t* p) {
    emi_ipm_bounds_t d{};
    if (!p) return d;
    d = *p;
    d.zl = s.place(p->zl, z.bnd, true, false); d.zu = s.place(p->zu, z.bnd, true, false);
    return d;
}

}  // namespace

#define IPM_HOST_BEGIN(what, nsets)                  \
    if (!c) return EMI_ERR_ARG;                      \
    EMI_TRY(ipm_check(c, what));                     \
    HIP_TRY(c, hipSetDevice(c->device));             \
    IpmStager s(c);                                  \
    const IpmSizes z(c, nsets)
// (an error ends the call only after the copies from the caller's arrays have drained)
#define IPM_HOST_END(call)                                               \
    if (s.status) { (void)hipStreamSynchronize(c->stream); return s.status; } \
    if (const int st_ = (call)) { (void)hipStreamSynchronize(c->stream); return st_; } \
    return s.finish()

int emi_ipm_reduce_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* VALS, const double* G,
                        const emi_ipm_bounds_t* bd, const double* par, const double* DefRes, const double* RowRes, const emi_ipm_elim_t* out,
                        double* Rhs) {
    IPM_HOST_BEGIN("emi_ipm_reduce_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const emi_ipm_elim_t de = stage_elim(s, z, out, false, true);
    const void *dR = s.place(RES, z.res, true, false), *dV = s.place(VALS, z.vals, true, false), *dG = s.place(G, z.var, true, false);
    const void *dP = s.place(par, z.inst * 4, true, false), *dDef = s.place(DefRes, z.X, true, false), *dRow = s.place(RowRes, z.row, true, false);
    void* dRhs = s.place(Rhs, z.kkt, false, true);
    IPM_HOST_END(emi_ipm_reduce_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, dR, dV, dG, bd ? &db : nullptr, dP, dDef, dRow, out ? &de : nullptr, dRhs));
}

int emi_ipm_expand_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* VALS, const emi_ipm_bounds_t* bd,
                        const double* par, const emi_ipm_elim_t* el, const double* rs, const emi_ipm_step_t* st, double* scal) {
    IPM_HOST_BEGIN("emi_ipm_expand_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const emi_ipm_elim_t de = stage_elim(s, z, el, true, false);
    const emi_ipm_step_t ds = stage_step(s, z, st, true, true, false, true);
    const void *dV = s.place(VALS, z.vals, true, false), *dP = s.place(par, z.inst * 4, true, false), *dRs = s.place(rs, z.X, true, false);
    void* dS = s.place(scal, z.inst * 4, false, true);
    IPM_HOST_END(emi_ipm_expand_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, dV, bd ? &db : nullptr, dP, el ? &de : nullptr, dRs, st ? &ds : nullptr, dS));
}

int emi_ipm_trial_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_step_t* st, const double* alpha, const emi_ipm_point_t* trial) {
    IPM_HOST_BEGIN("emi_ipm_trial_host", 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false), dt = stage_point(s, z, trial, false, true);
    const emi_ipm_step_t ds = stage_step(s, z, st, true, false, true, false);
    const void* dA = s.place(alpha, z.inst, true, false);
    IPM_HOST_END(emi_ipm_trial_dev(c, pt ? &dp : nullptr, st ? &ds : nullptr, dA, trial ? &dt : nullptr));
}

int emi_ipm_merit_host(emi_ctx_t c, const emi_ipm_point_t* pt, const double* RES, const double* COST, const emi_ipm_bounds_t* bd, const double* par,
                       const double* rs, int reset, double* out) {
    IPM_HOST_BEGIN("emi_ipm_merit_host", bd ? bd->nsets : 0);
    emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    if (pt && reset) s.outs.push_back({pt->S, dp.S, pt->S ? z.row : 0});        // the slack reset updates S in place
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const void *dR = s.place(RES, z.res, true, false), *dC = s.place(COST, z.inst, true, false), *dP = s.place(par, z.inst * 4, true, false);
    const void* dRs = s.place(rs, z.X, true, false);
    void* dO = s.place(out, z.inst * 2, false, true);
    IPM_HOST_END(emi_ipm_merit_dev(c, pt ? &dp : nullptr, dR, dC, bd ? &db : nullptr, dP, dRs, reset, dO));
}

int emi_ipm_accept_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_point_t* trial, const emi_ipm_duals_t* du, const emi_ipm_step_t* st,
                        const emi_ipm_bounds_t* bd, const double* par, const double* a_pr, const double* a_du, const unsigned char* mask) {
    IPM_HOST_BEGIN("emi_ipm_accept_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, true), dt = stage_point(s, z, trial, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, true);
    const emi_ipm_step_t ds = stage_step(s, z, st, true, false, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const void *dP = s.place(par, z.inst * 4, true, false), *dA = s.place(a_pr, z.inst, true, false), *dD = s.place(a_du, z.inst, true, false);
    const void* dM = s.place(mask, (size_t)c->B, true, false);
    IPM_HOST_END(emi_ipm_accept_dev(c, pt ? &dp : nullptr, trial ? &dt : nullptr, du ? &dd : nullptr, st ? &ds : nullptr, bd ? &db : nullptr, dP, dA, dD, dM));
}

int emi_ipm_error_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* G,
                       const emi_ipm_bounds_t* bd, const double* par, double* out) {
    IPM_HOST_BEGIN("emi_ipm_error_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const void *dR = s.place(RES, z.res, true, false), *dG = s.place(G, z.var, true, false), *dP = s.place(par, z.inst * 4, true, false);
    void* dO = s.place(out, z.inst * 3, false, true);
    IPM_HOST_END(emi_ipm_error_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, dR, dG, bd ? &db : nullptr, dP, dO));
}

int emi_ipm_error_parts_host(emi_ctx_t c, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* G,
                             const emi_ipm_bounds_t* bd, const double* par, double* out) {
    IPM_HOST_BEGIN("emi_ipm_error_parts_host", bd ? bd->nsets : 0);
    const emi_ipm_point_t dp = stage_point(s, z, pt, true, false);
    const emi_ipm_duals_t dd = stage_duals(s, z, du, true, false);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    const void *dR = s.place(RES, z.res, true, false), *dG = s.place(G, z.var, true, false), *dP = s.place(par, z.inst * 4, true, false);
    void* dO = s.place(out, z.inst * 8, false, true);
    IPM_HOST_END(emi_ipm_error_parts_dev(c, pt ? &dp : nullptr, du ? &dd : nullptr, dR, dG, bd ? &db : nullptr, dP, dO));
}

int emi_kkt_lowrank(emi_ctx_t c, int r, const int* node, const double* vec, const double* delta, int* exact) {
    if (!c || r < 0 || !exact || (r > 0 && (!node || !vec || !delta))) return fail(c, EMI_ERR_ARG, "emi_kkt_lowrank: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    for (int a = 0; a < r; ++a)
        if (node[a] < 0 || node[a] >= c->M || !(delta[a] > 0.0))
            return fail(c, EMI_ERR_ARG, "emi_kkt_lowrank: column %d has node %d / delta %g", a, node[a], delta[a]);
    std::string err;
    const int st = emi::kkt_lowrank(c->kkt, c->stream, (c->ns + c->nc) * c->M, r, node, vec, delta, exact, &err);
    if (st) c->err = err;
    return st;
}

// ---- batched Newton steps: n contexts (one scenario each) on the same mesh and model ---------------------------------------
static int batch_compatible(int n, const emi_ctx_t* ctxs, const char* what, bool factorising) {
    if (n < 1 || !ctxs || !ctxs[0]) return EMI_ERR_ARG;
    emi_ctx_t c0 = ctxs[0];
    for (int b = 0; b < n; ++b) {
        emi_ctx_t c = ctxs[b];
        if (!c) return EMI_ERR_ARG;
        if (c->M <= 0 || c->model < 0 || c->f32 || c->points_only)
            return fail(c0, EMI_ERR_STATE, "%s: context %d is not an f64 context with a collocation mesh and a model", what, b);
        if (factorising && c->kkt_method != 1)
            return fail(c0, EMI_ERR_UNSUPPORTED, "%s: context %d is set to the LU method (\"kkt_method\" 0): emi_kkt_factor", what, b);
        if (c->device != c0->device || c->M != c0->M || c->ns != c0->ns || c->nc != c0->nc)
            return fail(c0, EMI_ERR_ARG, "%s: context %d differs from context 0 in device, mesh size or model dimensions", what, b);
        for (int a = 0; a < b; ++a)
            if (ctxs[a] == c) return fail(c0, EMI_ERR_ARG, "%s: context %d appears twice", what, b);
    }
    return EMI_OK;
}

int emi_kkt_factor_batch(int n, const emi_ctx_t* ctxs, const double* const* Qblk, const double* const* Jblk,
                         const unsigned char* const* fixed, const double* dc, int* info) {
    int st = batch_compatible(n, ctxs, "emi_kkt_factor_batch", true);
    if (st) return st;
    emi_ctx_t c0 = ctxs[0];
    if (!Qblk || !Jblk || !fixed || !dc || !info) return fail(c0, EMI_ERR_ARG, "emi_kkt_factor_batch: null argument");
    for (int b = 0; b < n; ++b)
        if (!Qblk[b] || !Jblk[b] || !fixed[b] || !(dc[b] >= 0.0)) return fail(c0, EMI_ERR_ARG, "emi_kkt_factor_batch: bad argument for scenario %d", b);
    HIP_TRY(c0, hipSetDevice(c0->device));
    std::vector<emi::KktWorkspace**> pws(n);
    std::vector<const double*> dD(n);
    for (int b = 0; b < n; ++b) {
        HIP_TRY(c0, hipStreamSynchronize(ctxs[b]->stream));     // whatever the scenario's own stream still holds (its last evaluation)
        pws[b] = &ctxs[b]->kkt;
        dD[b] = (const double*)ctxs[b]->d_D.p;
    }
    std::string err;
    st = emi::kkt_factor_batch(n, pws.data(), c0->stream, dD.data(), c0->M, c0->ns, c0->ns + c0->nc, Qblk, Jblk, fixed, dc, info, &err);
    if (st) { c0->err = err; return st; }
    // scenarios the batch could not take (a node block not positive definite, the ladder exhausted, more than 16 variables per node):
    // the single path with its LU
    for (int b = 0; b < n; ++b)
        if (info[b] < 0) {
            const int s1 = emi_kkt_factor(ctxs[b], Qblk[b], Jblk[b], fixed[b], dc[b], &info[b]);
            if (s1) { c0->err = ctxs[b]->err; return s1; }
        }
    return EMI_OK;
}

int emi_kkt_solve_batch(int n, const emi_ctx_t* ctxs, double* const* rhs) {
    int st = batch_compatible(n, ctxs, "emi_kkt_solve_batch", false);
    if (st) return st;
    emi_ctx_t c0 = ctxs[0];
    if (!rhs) return fail(c0, EMI_ERR_ARG, "emi_kkt_solve_batch: null argument");
    HIP_TRY(c0, hipSetDevice(c0->device));
    // scenarios whose factorisation is the LU fallback (or none) go through the single entry point; the rest as one batch
    std::vector<emi::KktWorkspace*> ws;
    std::vector<double*> rb;
    for (int b = 0; b < n; ++b) {
        if (!rhs[b]) return fail(c0, EMI_ERR_ARG, "emi_kkt_solve_batch: null right-hand side %d", b);
        HIP_TRY(c0, hipStreamSynchronize(ctxs[b]->stream));
        if (emi::kkt_is_schur(ctxs[b]->kkt)) { ws.push_back(ctxs[b]->kkt); rb.push_back(rhs[b]); }
        else if ((st = emi_kkt_solve(ctxs[b], rhs[b], 1))) { c0->err = ctxs[b]->err; return st; }
    }
    if (ws.empty()) return EMI_OK;
    std::string err;
    st = emi::kkt_solve_batch((int)ws.size(), ws.data(), c0->stream, (c0->ns + c0->nc) * c0->M, rb.data(), &err);
    if (st) c0->err = err;
    return st;
}

int emi_kkt_solve_refined_batch(int n, const emi_ctx_t* ctxs, double* const* rhs, const double* dc_nominal, int max_steps, double* rel,
                                int* nsolve, int* reverted, int* status) {
    int st = batch_compatible(n, ctxs, "emi_kkt_solve_refined_batch", false);
    if (st) return st;
    emi_ctx_t c0 = ctxs[0];
    if (!rhs || !dc_nominal || !rel || !nsolve || !reverted || !status || max_steps < 0)
        return fail(c0, EMI_ERR_ARG, "emi_kkt_solve_refined_batch: bad argument");
    HIP_TRY(c0, hipSetDevice(c0->device));
    std::vector<emi::KktWorkspace*> ws(n);
    for (int b = 0; b < n; ++b) {
        if (!rhs[b] || !(dc_nominal[b] >= 0.0)) return fail(c0, EMI_ERR_ARG, "emi_kkt_solve_refined_batch: bad argument for scenario %d", b);
        if (!emi::kkt_is_schur(ctxs[b]->kkt))
            return fail(c0, EMI_ERR_UNSUPPORTED, "emi_kkt_solve_refined_batch: scenario %d holds no factorisation of the Schur path (the LU fallback "
                                                 "is refined by the caller: emi_kkt_solve)", b);
        HIP_TRY(c0, hipStreamSynchronize(ctxs[b]->stream));
        ws[b] = ctxs[b]->kkt;
    }
    std::string err;
    st = emi::kkt_solve_refined_batch(n, ws.data(), c0->stream, rhs, dc_nominal, max_steps, rel, nsolve, reverted, status, &err);
    if (st) c0->err = err;
    return st;
}

int emi_kkt_solve_refined(emi_ctx_t c, double* rhs, double dc_nominal, int max_steps, double* rel, int* nsolve, int* reverted, int* status) {
    if (!c) return EMI_ERR_ARG;
    double* r1 = rhs;
    return emi_kkt_solve_refined_batch(1, &c, &r1, &dc_nominal, max_steps, rel, nsolve, reverted, status);
}

int emi_kkt_is_schur(emi_ctx_t c) { return c && emi::kkt_is_schur(c->kkt) ? 1 : 0; }

int emi_kkt_last_regularisation(emi_ctx_t c, double* dc, double* dw) {
    if (!c || (!dc && !dw)) return EMI_ERR_ARG;
    if (!c->kkt) return fail(c, EMI_ERR_STATE, "emi_kkt_last_regularisation: no factorisation");
    emi::kkt_last_regularisation(c->kkt, dc, dw);
    return EMI_OK;
}

// emi_kkt_solve / emi_kkt_solve_dev: the right-hand sides in host or in device memory, everything else the same
static int kkt_solve_from(emi_ctx_t c, void* rhs, int nrhs, bool on_device) {
    if (!c || !rhs || nrhs < 1) return EMI_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    std::string err;
    const int st = emi::kkt_solve(c->kkt, c->stream, (c->ns + c->nc) * c->M, (double*)rhs, nrhs, &err, on_device);
    if (st) c->err = err;
    return st;
}

int emi_kkt_solve(emi_ctx_t c, double* rhs, int nrhs) { return kkt_solve_from(c, rhs, nrhs, false); }

int emi_kkt_solve_dev(emi_ctx_t c, void* dRhs, int nrhs) { return kkt_solve_from(c, dRhs, nrhs, true); }

// ---- the Newton steps of a context's whole batch, device arrays in and out (the workspaces of c->kkt_shard) ------------------
namespace {

int shard_check(emi_ctx_t c, const char* what) {
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->M <= 0 || c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: mesh, model and batch must be set", what);
    if (c->points_only) return fail(c, EMI_ERR_STATE, "%s: the mesh has no differentiation matrix", what);
    if (c->nch > 0) return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts without delays only", what);
    if (c->ns + c->nc > 16) return fail(c, EMI_ERR_UNSUPPORTED, "%s: node blocks of up to 16 variables (this model has %d)", what, c->ns + c->nc);
    if (c->kkt_method != 1)
        return fail(c, EMI_ERR_UNSUPPORTED, "%s: the context is set to the LU method (\"kkt_method\" 0): emi_kkt_factor_dev per instance", what);
    return EMI_OK;
}

// the unmasked instances of the batch; need > 0: every one of them must hold a factorisation for the context's mesh and model
// (1: any, 2: of the Schur path)
int shard_members(emi_ctx_t c, const char* what, const unsigned char* mask, int need, std::vector<int>& inst) {
    const int nv = c->ns + c->nc;
    for (int b = 0; b < c->B; ++b) {
        if (mask && !mask[b]) continue;
        if (need) {
            const int held = b < (int)c->kkt_shard.size() ? emi::kkt_holds(c->kkt_shard[b], c->M, c->ns, nv) : 0;
            if (held == 0)
                return fail(c, EMI_ERR_STATE, "%s: instance %d holds no factorisation for this mesh and model (emi_kkt_factor_shard_dev)", what, b);
            if (need == 2 && held != 1)
                return fail(c, EMI_ERR_UNSUPPORTED, "%s: instance %d holds no factorisation of the Schur path (the LU fallback is refined by "
                                                    "the caller: emi_kkt_solve_shard_dev)", what, b);
        }
        inst.push_back(b);
    }
    return EMI_OK;
}

}  // namespace

int emi_kkt_factor_shard_dev(emi_ctx_t c, const void* dQ, const void* dVALS, const void* dFixed, const double* dc, const unsigned char* mask,
                             int* info) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(shard_check(c, "emi_kkt_factor_shard_dev"));
    if (!dQ || !dVALS || !dFixed || !dc || !info) return fail(c, EMI_ERR_ARG, "emi_kkt_factor_shard_dev: null argument");
    std::vector<int> inst;
    EMI_TRY(shard_members(c, "emi_kkt_factor_shard_dev", mask, 0, inst));
    for (int b : inst)
        if (!(dc[b] >= 0.0)) return fail(c, EMI_ERR_ARG, "emi_kkt_factor_shard_dev: dc[%d] = %g", b, dc[b]);
    if (inst.empty()) return EMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if ((int)c->kkt_shard.size() < c->B) c->kkt_shard.resize((size_t)c->B, nullptr);
    const int n = (int)inst.size(), M = c->M, ns = c->ns, nv = c->ns + c->nc, nh = nv * (nv + 1) / 2;
    const size_t vals_stride = (size_t)nvals_of(c) * M;
    std::vector<emi::KktWorkspace**> pws(n);
    std::vector<const double*> dD(n, (const double*)c->d_D.p);
    std::vector<double> dcs(n);
    std::vector<int> inf(n, -1);
    for (int a = 0; a < n; ++a) { pws[a] = &c->kkt_shard[inst[a]]; dcs[a] = dc[inst[a]]; }
    const emi::KktShardSrc src{(const double*)dQ, (const double*)dVALS, (const unsigned char*)dFixed, vals_stride, inst.data()};
    std::string err;
    int st = emi::kkt_factor_batch(n, pws.data(), c->stream, dD.data(), M, ns, nv, nullptr, nullptr, nullptr, dcs.data(), inf.data(), &err, &src);
    if (st) { c->err = err; return st; }
    // instances the batch could not take (a node block not positive definite, the ladder exhausted): the single path with its LU,
    // on the instance's own workspace and slices
    for (int a = 0; a < n; ++a) {
        const int b = inst[a];
        if (inf[a] < 0) {
            st = emi::kkt_factor(&c->kkt_shard[b], c->stream, (const double*)c->d_D.p, M, ns, nv, (const double*)dQ + (size_t)b * nh * M,
                                 (const double*)dVALS + (size_t)b * vals_stride, (const unsigned char*)dFixed + (size_t)b * nv * M, dc[b], 1,
                                 &inf[a], &err, true);
            if (st) { c->err = err; return st; }
        }
        info[b] = inf[a];
    }
    return EMI_OK;
}

int emi_kkt_lowrank_shard_dev(emi_ctx_t c, int max_mods, const void* dCount, const void* dNode, const void* dDelta, const void* dVec,
                              const unsigned char* mask, int* exact) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(shard_check(c, "emi_kkt_lowrank_shard_dev"));
    if (max_mods < 0 || !exact || (max_mods > 0 && (!dCount || !dNode || !dDelta || !dVec)))
        return fail(c, EMI_ERR_ARG, "emi_kkt_lowrank_shard_dev: bad argument");
    std::vector<int> inst;
    EMI_TRY(shard_members(c, "emi_kkt_lowrank_shard_dev", mask, 1, inst));
    if (inst.empty()) return EMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int n = (int)inst.size();
    std::vector<int> all((size_t)c->B, 0), cnt(n, 0), ex(n, 0);
    if (max_mods > 0) {             // the counts: the one download of this call
        HIP_TRY(c, hipMemcpyAsync(all.data(), dCount, (size_t)c->B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    std::vector<emi::KktWorkspace*> ws(n);
    for (int a = 0; a < n; ++a) {
        ws[a] = c->kkt_shard[inst[a]];
        // max_mods == 0 clears: no list is read, every instance is taken as unmodified (exact, no correction), as emi_kkt_lowrank with r = 0
        cnt[a] = max_mods > 0 ? std::max(all[inst[a]], 0) : 0;
    }
    std::string err;
    const int st = emi::kkt_lowrank_shard(n, ws.data(), c->stream, max_mods, inst.data(), cnt.data(), (const int*)dNode, (const double*)dDelta,
                                          (const double*)dVec, ex.data(), &err);
    if (st) { c->err = err; return st; }
    for (int a = 0; a < n; ++a) exact[inst[a]] = ex[a];
    return EMI_OK;
}

int emi_kkt_solve_shard_dev(emi_ctx_t c, void* dRhs, const unsigned char* mask) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(shard_check(c, "emi_kkt_solve_shard_dev"));
    if (!dRhs) return fail(c, EMI_ERR_ARG, "emi_kkt_solve_shard_dev: null argument");
    std::vector<int> inst;
    EMI_TRY(shard_members(c, "emi_kkt_solve_shard_dev", mask, 1, inst));
    HIP_TRY(c, hipSetDevice(c->device));
    const int nv = c->ns + c->nc, nz = nv * c->M;
    const size_t N = (size_t)(nv + c->ns) * c->M;
    // instances that hold the LU fallback go through the single solve; the rest as one batch
    std::vector<emi::KktWorkspace*> ws;
    std::vector<double*> rb;
    std::string err;
    for (int b : inst) {
        emi::KktWorkspace* w = c->kkt_shard[b];
        double* x = (double*)dRhs + (size_t)b * N;
        if (emi::kkt_is_schur(w)) { ws.push_back(w); rb.push_back(x); }
        else if (int st = emi::kkt_solve(w, c->stream, nz, x, 1, &err, true)) { c->err = err; return st; }
    }
    if (ws.empty()) return EMI_OK;
    const int st = emi::kkt_solve_batch((int)ws.size(), ws.data(), c->stream, nz, rb.data(), &err, true);
    if (st) c->err = err;
    return st;
}

int emi_kkt_solve_refined_shard_dev(emi_ctx_t c, void* dRhs, const unsigned char* mask, const double* dc_nominal, int max_steps, double* rel,
                                    int* nsolve, int* reverted, int* status) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(shard_check(c, "emi_kkt_solve_refined_shard_dev"));
    if (!dRhs || !dc_nominal || !rel || !nsolve || !reverted || !status || max_steps < 0)
        return fail(c, EMI_ERR_ARG, "emi_kkt_solve_refined_shard_dev: bad argument");
    std::vector<int> inst;
    EMI_TRY(shard_members(c, "emi_kkt_solve_refined_shard_dev", mask, 2, inst));
    for (int b : inst)
        if (!(dc_nominal[b] >= 0.0)) return fail(c, EMI_ERR_ARG, "emi_kkt_solve_refined_shard_dev: dc_nominal[%d] = %g", b, dc_nominal[b]);
    if (inst.empty()) return EMI_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int n = (int)inst.size();
    const size_t N = (size_t)(2 * c->ns + c->nc) * c->M;
    std::vector<emi::KktWorkspace*> ws(n);
    std::vector<double*> rb(n);
    std::vector<double> dcn(n), r(n);
    std::vector<int> nsv(n), rev(n), sta(n);
    for (int a = 0; a < n; ++a) { ws[a] = c->kkt_shard[inst[a]]; rb[a] = (double*)dRhs + (size_t)inst[a] * N; dcn[a] = dc_nominal[inst[a]]; }
    std::string err;
    const int st = emi::kkt_solve_refined_batch(n, ws.data(), c->stream, rb.data(), dcn.data(), max_steps, r.data(), nsv.data(), rev.data(),
                                                sta.data(), &err, true);
    if (st) { c->err = err; return st; }
    for (int a = 0; a < n; ++a) { rel[inst[a]] = r[a]; nsolve[inst[a]] = nsv[a]; reverted[inst[a]] = rev[a]; status[inst[a]] = sta[a]; }
    return EMI_OK;
}

// ---- lock-step interior-point solve of the whole batch (the driver: emi_ipm_solve.hip) -------------------------------------------
extern "C++" {
namespace emi {

int ctx_shard_holds(emi_ctx_t c, int b) {
    return b < (int)c->kkt_shard.size() ? kkt_holds(c->kkt_shard[b], c->M, c->ns, c->ns + c->nc) : 0;
}

void ctx_shard_forget_ladders(emi_ctx_t c) {
    for (KktWorkspace* w : c->kkt_shard) kkt_forget_ladder(w);
}

int ctx_ipm_launch(emi_ctx_t c, int what, const emi_ipm_bounds_t* bd, const void* dPar, IpmArgs& a) {
    EMI_TRY(ipm_common(c, "emi_ipm_solve_shard_dev", bd, dPar, a));
    HIP_TRY(c, launch_ipm(what, a, c->stream));
    return EMI_OK;
}

}  // namespace emi
}  // extern "C++"

int emi_ipm_solve_shard_dev(emi_ctx_t c, void* dX, void* dU, const emi_ipm_bounds_t* bd, const emi_ipm_options_t* opt, void* dLamF,
                            void* dLamC, emi_ipm_result_t* results) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ipm_check(c, "emi_ipm_solve_shard_dev"));
    EMI_TRY(shard_check(c, "emi_ipm_solve_shard_dev"));
    EMI_TRY(ready(c));
    const int np = np_total(c);
    if (!dX || (c->nc > 0 && !dU) || !bd || !opt || !dLamF || (np > 0 && !dLamC) || !results)
        return fail(c, EMI_ERR_ARG, "emi_ipm_solve_shard_dev: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const emi::IpmSolveDims d{c->device, c->B, c->M, c->ns, c->nc, np, nvals_of(c), nhess_of(c), c->stream};
    std::string err;
    const int st = emi::ipm_solve_shard(c, &c->ipm_solve, d, dX, dU, bd, *opt, dLamF, dLamC, results, &err);
    if (st && !err.empty()) c->err = err;
    return st;
}

int emi_ipm_solve_shard_host(emi_ctx_t c, double* X, double* U, const emi_ipm_bounds_t* bd, const emi_ipm_options_t* opt, double* LamF,
                             double* LamC, emi_ipm_result_t* results) {
    IPM_HOST_BEGIN("emi_ipm_solve_shard_host", bd ? bd->nsets : 0);
    void *dX = s.place(X, z.X, true, true), *dU = s.place(U, z.U, true, true);
    void *dLF = s.place(LamF, z.X, false, true), *dLC = s.place(LamC, z.row, false, true);
    const emi_ipm_bounds_t db = stage_bounds(s, z, bd);
    IPM_HOST_END(emi_ipm_solve_shard_dev(c, dX, dU, bd ? &db : nullptr, opt, dLF, dLC, results));
}

// ---- the mesh ladder over the lock-step solve (kernels and driver: emi_ipm_ladder.hip) ---------------------------------------------
int emi_prolong_dev(emi_ctx_t c, int Mc, int Mf, const void* dPT, const void* dVc, int R, void* dVf) {
    if (!c) return EMI_ERR_ARG;
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "emi_prolong_dev: f64 contexts only");
    if (Mc < 2 || Mf < 2 || R < 0 || !dPT || (R > 0 && (!dVc || !dVf))) return fail(c, EMI_ERR_ARG, "emi_prolong_dev: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, emi::launch_prolong((const double*)dPT, (const double*)dVc, (double*)dVf, Mc, Mf, R, c->stream));
    return EMI_OK;
}

int emi_repair_guess_dev(emi_ctx_t c, void* dX) {
    if (!c) return EMI_ERR_ARG;
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "emi_repair_guess_dev: f64 contexts only");
    EMI_TRY(ready(c));
    if (!dX) return fail(c, EMI_ERR_ARG, "emi_repair_guess_dev: null argument");
    if (c->B > 65535) return fail(c, EMI_ERR_UNSUPPORTED, "emi_repair_guess_dev: up to 65535 instances");
    if (c->np > 0 && c->path_has_track && c->ntracks <= 0)
        return fail(c, EMI_ERR_STATE, "emi_repair_guess_dev: the table has rows of kind EMI_PATH_TRACK: emi_set_tracks must follow emi_set_mesh");
    HIP_TRY(c, hipSetDevice(c->device));
    const emi::RepairArgs a{(double*)dX, (const double*)c->d_path.p, (const double*)c->d_trkx.p, (const double*)c->d_trky.p, c->B, c->ns, c->M,
                            c->np, c->path_sets, c->px, c->py, c->ntracks, c->track_sets};
    HIP_TRY(c, emi::launch_repair_guess(a, c->stream));
    return EMI_OK;
}

namespace {

// what the ladder refuses before it touches the context (the mesh need not be set: the call sets it)
int ladder_check(emi_ctx_t c, const char* what, int nrungs, const emi_ipm_rung_t* rungs) {
    if (c->f32) return fail(c, EMI_ERR_UNSUPPORTED, "%s: f64 contexts only", what);
    if (c->model < 0 || c->B <= 0) return fail(c, EMI_ERR_STATE, "%s: model and batch must be set", what);
    if (c->nch > 0) return fail(c, EMI_ERR_UNSUPPORTED, "%s: contexts with delays are not taken", what);
    if (c->ns + c->nc > 16) return fail(c, EMI_ERR_UNSUPPORTED, "%s: up to 16 variables per node (this model has %d)", what, c->ns + c->nc);
    if (c->kkt_method != 1) return fail(c, EMI_ERR_UNSUPPORTED, "%s: the context is set to the LU method (\"kkt_method\" 0)", what);
    if (nrungs < 1 || !rungs) return fail(c, EMI_ERR_ARG, "%s: no rungs", what);
    bool track = c->np > 0 && c->path_has_track;
    for (int r = 0; r < nrungs; ++r) {
        if (rungs[r].M < 2) return fail(c, EMI_ERR_ARG, "%s: rung %d has %d nodes", what, r, rungs[r].M);
        if (!rungs[r].bd.zl || !rungs[r].bd.zu) return fail(c, EMI_ERR_ARG, "%s: rung %d has no bounds", what, r);
        if (!rungs[r].recs) continue;
        if (c->np <= 0) return fail(c, EMI_ERR_ARG, "%s: rung %d brings a record table and the context has none", what, r);
        for (size_t i = 0; i < (size_t)c->np * c->path_sets; ++i) track = track || (int)rungs[r].recs[i * EMI_PATH_REC] == EMI_PATH_TRACK;
    }
    if (track)
        return fail(c, EMI_ERR_UNSUPPORTED, "%s: rows of kind EMI_PATH_TRACK have their centres per mesh, which this call cannot supply", what);
    return EMI_OK;
}

}  // namespace

int emi_ipm_solve_ladder_dev(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const void* dX0, const void* dU0,
                             void* dX, void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ladder_check(c, "emi_ipm_solve_ladder_dev", nrungs, rungs));
    const int np = np_total(c);
    if (!dX0 || !dX || (c->nc > 0 && (!dU0 || !dU)) || !dLamF || (np > 0 && !dLamC) || !results)
        return fail(c, EMI_ERR_ARG, "emi_ipm_solve_ladder_dev: null argument");
    if (!(tf > t0)) return fail(c, EMI_ERR_ARG, "emi_ipm_solve_ladder_dev: tf must exceed t0");
    HIP_TRY(c, hipSetDevice(c->device));
    const emi::IpmLadderDims d{c->B, c->ns, c->nc, np, c->np, c->path_sets, c->px, c->py, c->stream};
    std::string err;
    const int st = emi::ipm_solve_ladder(c, &c->ipm_ladder, d, nrungs, rungs, t0, tf, dX0, dU0, dX, dU, dLamF, dLamC, results, &err);
    if (st && !err.empty()) c->err = err;
    return st;
}

int emi_ipm_solve_ladder_host(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const double* X0, const double* U0,
                              double* X, double* U, double* LamF, double* LamC, emi_ipm_result_t* results) {
    if (!c) return EMI_ERR_ARG;
    EMI_TRY(ladder_check(c, "emi_ipm_solve_ladder_host", nrungs, rungs));
    HIP_TRY(c, hipSetDevice(c->device));
    IpmStager s(c);
    const size_t B = (size_t)c->B, nv = (size_t)(c->ns + c->nc), M0 = (size_t)rungs[0].M, ML = (size_t)rungs[nrungs - 1].M;
    const void *dX0 = s.place(X0, B * c->ns * M0 * 8, true, false), *dU0 = s.place(U0, B * c->nc * M0 * 8, true, false);
    void *dX = s.place(X, B * c->ns * ML * 8, false, true), *dU = s.place(U, B * c->nc * ML * 8, false, true);
    void *dLF = s.place(LamF, B * c->ns * ML * 8, false, true), *dLC = s.place(LamC, B * (size_t)np_total(c) * ML * 8, false, true);
    std::vector<emi_ipm_rung_t> dr(rungs, rungs + nrungs);
    for (emi_ipm_rung_t& g : dr) {
        const size_t bytes = (size_t)std::max(g.bd.nsets, 0) * nv * (size_t)g.M * 8;
        g.bd.zl = s.place(g.bd.zl, bytes, true, false);
        g.bd.zu = s.place(g.bd.zu, bytes, true, false);
    }
    IPM_HOST_END(emi_ipm_solve_ladder_dev(c, nrungs, dr.data(), t0, tf, dX0, dU0, dX, dU, dLF, dLC, results));
}

int emi_timer_start(emi_ctx_t c) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipEventRecord(c->t_start, c->stream));
    return EMI_OK;
}

int emi_timer_stop(emi_ctx_t c, float* ms) {
    if (!c || !ms) return EMI_ERR_ARG;
    HIP_TRY(c, hipEventRecord(c->t_stop, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->t_stop));
    HIP_TRY(c, hipEventElapsedTime(ms, c->t_start, c->t_stop));
    return EMI_OK;
}

int emi_profile_enable(emi_ctx_t c, int on) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->profile = (on >= 0 && on <= 3) ? on : 1;
    c->prof_used = 0;
    return EMI_OK;
}

int emi_profile_read(emi_ctx_t c, float* node_ms, int* node_launches, float* defect_ms,
                     int* defect_launches, float* pass_ms, int* overlapped_passes) {
    if (!c) return EMI_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->stream2) HIP_TRY(c, hipStreamSynchronize(c->stream2));
    float nm = 0, dm = 0, fm = 0;
    int nl = 0, dl = 0, fl = 0;
    for (size_t i = 0; i < c->prof_used; ++i) {
        ProfEvents& pe = c->prof[i];
        float ms = 0;
        if (pe.fused && pe.level == -1) {
            HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[K0], pe.ev[K1]));
            dm += ms; ++dl; fm += ms; ++fl;
            continue;
        }
        if (pe.fused) {
            if (pe.level == 1) {
                HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[E0], pe.ev[E1]));
                fm += ms;
            }
            ++fl;
            if (pe.level == 1 || pe.level == 2) {
                HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[K0], pe.ev[K1]));
                dm += ms;
                ++dl;
            }
            if (pe.level == 1 || pe.level == 3) {
                HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[K2], pe.ev[K3]));
                nm += ms;
                ++nl;
            }
            continue;
        }
        if (pe.has_node && pe.level != 2) {
            HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[E0], pe.ev[E1]));
            nm += ms;
            ++nl;
        }
        if (pe.has_defect && pe.level != 3) {
            HIP_TRY(c, hipEventElapsedTime(&ms, pe.ev[E1], pe.ev[E2]));
            dm += ms;
            ++dl;
        }
    }
    c->prof_used = 0;
    if (node_ms) *node_ms = nm;
    if (node_launches) *node_launches = nl;
    if (defect_ms) *defect_ms = dm;
    if (defect_launches) *defect_launches = dl;
    if (pass_ms) *pass_ms = fm;
    if (overlapped_passes) *overlapped_passes = fl;
    return EMI_OK;
}

int emi_set_option(emi_ctx_t c, const char* name, int value) {
    if (!c || !name) return EMI_ERR_ARG;
    if (strcmp(name, "cu_split") == 0) {
        // experiment: spatial instead of temporal sharing of the chip between the MFMA and the streaming kernel
        hipDeviceProp_t prop;
        HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
        const int ncu = prop.multiProcessorCount;
        if (value < 0 || value >= ncu) return fail(c, EMI_ERR_ARG, "cu_split must be in [0, %d)", ncu);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->s_mfma) { HIP_TRY(c, hipStreamDestroy(c->s_mfma)); c->s_mfma = nullptr; }
        if (c->s_node) { HIP_TRY(c, hipStreamDestroy(c->s_node)); c->s_node = nullptr; }
        c->cu_split = value;
        if (value > 0) {
            const int words = (ncu + 31) / 32;
            std::vector<uint32_t> m1(words, 0u), m2(words, 0u);
            for (int i = 0; i < ncu; ++i) (i < value ? m1 : m2)[i / 32] |= 1u << (i % 32);
            HIP_TRY(c, hipExtStreamCreateWithCUMask(&c->s_mfma, words, m1.data()));
            HIP_TRY(c, hipExtStreamCreateWithCUMask(&c->s_node, words, m2.data()));
            if (!c->ev_join2) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming));
        }
        return EMI_OK;
    }
    if (strcmp(name, "blocks_generic") == 0) {      // emi_kkt_blocks_*: the run-time-nv assembly kernel also where a templated one exists
        if (value != 0 && value != 1) return fail(c, EMI_ERR_ARG, "blocks_generic must be 0 or 1");
        c->blk_generic = value;
        return EMI_OK;
    }
    if (strcmp(name, "kkt_method") == 0) {
        if (value != 0 && value != 1) return fail(c, EMI_ERR_ARG, "kkt_method must be 0 (LU) or 1 (Schur complement + Cholesky)");
        c->kkt_method = value;
        return EMI_OK;
    }
    if (strncmp(name, "kkt_", 4) == 0) {        // the process-wide switches of the Newton step (emi_kkt.hip)
        if (strcmp(name, "kkt_cholesky") == 0 && value != 1 && value != 2)
            return fail(c, EMI_ERR_ARG, "kkt_cholesky must be 1 (one-level blocked Cholesky) or 2 (two-level form from 1024 rows)");
        if (emi::kkt_set_option(name, value)) return EMI_OK;
        return fail(c, EMI_ERR_ARG, "unknown option %s", name);
    }
    for (const OptionRow& o : OPTIONS) {
        if (strcmp(name, o.name) != 0) continue;
        if (!o.accepts(value)) return fail(c, EMI_ERR_ARG, "%s", o.message);
        c->*o.member = o.stored(value);
        return EMI_OK;
    }
    return fail(c, EMI_ERR_ARG, "unknown option '%s'", name);
}

int emi_plan_pass(emi_ctx_t c, int B, emi_pass_plan_t* out) {
    if (!c || !out || B < 1) return EMI_ERR_ARG;
    if (c->M <= 0 || c->model < 0) return fail(c, EMI_ERR_STATE, "emi_plan_pass: mesh and model must be set");
    memset(out, 0, sizeof *out);
    const int piece = (!c->f32 && overlapped_path(c)) ? plan_piece(c, B) : 0;
    const int first = piece > 0 ? piece : B;    // instances of the first launch
    out->piece = piece;
    out->tail = piece > 0 ? B % piece : 0;
    if (!c->f32 && overlapped_path(c)) {
        const PassPlan p = plan_pass(c, first, true);
        out->one_launch = p.one_launch ? 1 : 0;
        out->sw = p.sym.sw;
        out->ksplit = p.sym.ks;
        out->ring_stages = p.sym.nst;
        out->k_tile = p.sym.bk;
        out->column_tiles = p.sym.ct;
        out->k_halves = p.sym.hs;
        out->cpart = p.sym.cpart;
        out->cx = p.sym.cx;
        out->mfma_workgroups = p.sym.tiles * p.sym.ks;
        out->store_mode = p.store_mode;
        out->block_order = p.mfma_first;
        out->tiles16 = p.tiles16;
    }
    return EMI_OK;
}

int emi_last_path(emi_ctx_t c, int* fused) {
    if (!c || !fused) return EMI_ERR_ARG;
    *fused = choose_form(c, Launch{0, c->B}, EMI_EVAL_ALL).overlapped() ? 1 : 0;
    return EMI_OK;
}

int emi_debug_pass_roles(int nm, int nn, int order, int* out_role, int out_cap) {
    if (nm < 0 || nn < 0 || nm + nn < 1 || !out_role || out_cap < nm + nn) return EMI_ERR_ARG;
    for (int j = 0; j < nm + nn; ++j) {
        const emi::PassRole r = emi::pass_role_of(j, nm, nn, order);
        out_role[j] = r.mfma ? r.index : -1 - r.index;
    }
    return EMI_OK;
}

int emi_debug_tile_order(int ns, int B, int M, int sym_ct, int sym_cpart, int* out_tile, int out_cap, int* ntiles_total, int* cpart,
                         int* cx) {
    return emi_debug_tile_order2(ns, B, M, sym_ct, sym_cpart, 0, 0, out_tile, out_cap, ntiles_total, cpart, cx);
}

int emi_debug_tile_order2(int ns, int B, int M, int sym_ct, int sym_cpart, int sym_gblk, int sym_cx, int* out_tile, int out_cap,
                          int* ntiles_total, int* cpart, int* cx) {
    if (ns < 1 || B < 1 || M < 128 || M % 128 != 0 || !ntiles_total) return EMI_ERR_ARG;
    const emi::SymPlan p = emi::plan_symdefect(ns, B, M, sym_ct, 1, sym_cpart, sym_gblk, sym_cx);
    if (p.ring1 || p.sw < 1) return EMI_ERR_UNSUPPORTED;
    const int ntiles = (M / 2) / 64, ngrp = ((B + 15) / 16) * (ns / p.sw), total = ntiles * ngrp;
    *ntiles_total = total;
    if (cpart) *cpart = p.cpart;
    if (cx) *cx = p.cx;
    for (int t = 0; t < total && t < out_cap && out_tile; ++t) {
        const emi::RingTile rt = emi::ring_tile_of(t, ntiles, ngrp, p.cpart, p.cx, ns / p.sw);
        out_tile[t] = rt.ntile + ntiles * rt.grp;
    }
    return EMI_OK;
}

/* name of the kernel that produced the defect rows in the last emi_eval_dev of this context (for reports) */
const char* emi_last_defect_kernel(emi_ctx_t c) {
    if (!c) return "";
    return c->last_defect_kernel.c_str();
}

}  // extern "C"
