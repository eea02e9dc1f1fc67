// emi_kernels.hpp -- launcher prototypes shared by the kernel translation units and the C-ABI
// implementation (emi_api*.hip, which share the context through emi_ctx.hpp).  Argument blocks and tile constants: emi_args.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

#include "emi355x.h"
#include "emi_args.hpp"
#include "emi_pass_plan.hpp"

// emi_args.hpp repeats these for run-time compiled model programs
static_assert(EMI_PATH_ELLIPSE == 0 && EMI_PATH_DISC == 1 && EMI_PATH_TRACK == 2 && EMI_PATH_REC == 8,
              "emi_args.hpp and emi355x.h disagree");

namespace emi {

static_assert(PASS_TI == FUSED_TI, "emi_pass_plan.hpp and emi_args.hpp disagree");

int node_chunks(int M);
bool invariant_rows(int model, int np, unsigned char* mask);    // [ns nv + 2 np + nv] bytes, 1 = row invariant; false: not a built-in model
template <typename T>
hipError_t launch_nodes(int model, const NodeArgs<T>& a, bool jac, bool defect_rows, hipStream_t s);
template <typename T> hipError_t launch_hess(int model, const HessArgs<T>& a, hipStream_t s);
// ... of a context with a per-instance parameter table (emi_kernels_tab.hip): tab [a.B][EMI_MAX_PARAMS] at the launch's first instance.
// The node kernel always with the defect rows and plain stores: such a context takes the sequential route
template <typename T> hipError_t launch_nodes_tab(int model, const NodeArgs<T>& a, const T* tab, bool jac, hipStream_t s);
template <typename T> hipError_t launch_hess_tab(int model, const HessArgs<T>& a, const T* tab, hipStream_t s);
hipError_t launch_defect_f64(const DefectArgs& a, hipStream_t s);
bool defect_small_supported(int R);
hipError_t launch_defect_small_f64(const DefectArgs& a, hipStream_t s);
hipError_t launch_defect_f32(const DefectArgsF32& a, hipStream_t s);
bool defect_f32_mfma_supported(int M);
hipError_t launch_defect_f32_mfma(const DefectArgsF32& a, hipStream_t s, int ring = 0, int wgs_per_cu = 2);    // ring: the LDS-DMA operand ring form
// the fp32 pass as one launch (MFMA role + node role, defect rows by float atomics onto zeroed rows): emi_defect_f32.hip
bool pass_f32_supported(int model, int R, int M, int B);
hipError_t launch_pass_f32(int model, const DefectArgsF32& d, const NodeArgs<float>& n, int order, hipStream_t s);
hipError_t defect_f64_set_attr();
template <typename T>
hipError_t launch_cost_finish(const T* part, T* cost, int B, int nchunks, T scale, hipStream_t s);
bool fused_supported(int model, int M, int ct);
// SymPlan (which even/odd MFMA defect kernel a launch uses) and plan_symdefect: emi_pass_plan.hpp
hipError_t launch_symdefect(int model, const SymDefectArgs& a, hipStream_t s, bool set_attr, int ct, const SymPlan& plan);
// The fragment-order copy of De / Do, for 16-deep K tiles and 64-column tiles: the 16 bytes lane `lane` of wave w loads as piece q of K tile
// kt of column tile ct are double2 number (((ct*4 + w)*nkt + kt)*4 + q)*64 + lane, nkt = M/32, q = 2h + odd, lane = 16 kq + r16; they hold
// P[64 ct + 16 w + r16][16 kt + 8 h + 2 kq] and its right neighbour, P = De (odd = 0) or Do (odd = 1) -- the bits and the k order that the
// fragment reads of the staged form take out of the ring.  One function for the upload and for emi_debug_operator_fragments.
inline void operator_fragments(int M, const double* De, const double* Do, double* out) {
    const int Hh = M / 2, nkt = Hh / 16;
    for (int ct = 0; ct < Hh / 64; ++ct)
        for (int w = 0; w < 4; ++w)
            for (int kt = 0; kt < nkt; ++kt)
                for (int q = 0; q < 4; ++q)
                    for (int lane = 0; lane < 64; ++lane) {
                        const double* row = ((q & 1) ? Do : De) + (size_t)(64 * ct + 16 * w + (lane & 15)) * Hh + 16 * kt + 8 * (q >> 1) + 2 * (lane >> 4);
                        double* o = out + ((((size_t)(ct * 4 + w) * nkt + kt) * 4 + q) * 64 + lane) * 2;
                        o[0] = row[0];
                        o[1] = row[1];
                    }
}

// the whole pass as one launch (MFMA-role and node-role workgroups in one grid; COST finished in-kernel), in the form of the plan: a row
// of EMI_PASS_FORMS (emi_pass_plan.hpp), anything else is an error
bool pass_model_supported(int model);
// (work: the device copy of the work table of `key`, pass_work_for in emi_pass_plan.hpp -- a table built for other counts is an error)
hipError_t launch_pass(int model, const SymDefectArgs& sa, const NodeArgs<double>& na, hipStream_t s, const SymPlan& plan, const PassWorkKey& key,
                       const PassWork* work);

// the adjoint pass (emi_adjoint.hip): Lagrangian gradient G[B][ns+nc][M] and the per-instance KKT certificate, fp64
struct AdjointArgs {
    const double* VALS;     // [B][nvals][M]
    const double* lamF;     // [B][ns][M]
    const double* lamC;     // [B][np_table + np_traced][M] (may be null without path rows)
    const double* DT;       // [M][ldt]: DT[n][j] = D[j][n], zero diagonal, zero padding
    const int* pvars;       // [pw] node variables of the traced rows' partials (device)
    double* G;              // [B][ns+nc][M]
    int B, M, ldt, ns, nc, np_table, np_traced, pw, px, py, nvals;
    int add_op;             // node kernels: 1 = add the operator term already in the state rows of G, 0 = write the node terms alone
    double sigma;
};
struct CertArgs {
    const double *X, *U, *RES, *VALS, *lamF, *lamC, *G;
    const double *zl, *zu;  // [nsets][ns+nc][M]   (nc: the controls G, U, zl and zu hold -- the free ones of a context with delays)
    const double *cl, *cu;  // [np] (device)
    double* cert;           // [B][6]
    int B, M, ns, nc, np, nres, nvals, nsets;
    int ncg;                // cost-gradient entries at the end of VALS that gmax runs over (>= ns + nc: the delayed inputs' too)
    double sigma;
};
// One product of the adjoint pass on the matrix pipe (emi_adjoint_op_kernel): out rows r = (instance, j), j < rpi,
//     out[r][n] = (epilogue: add[r][n] +) sum over segments s < nseg, k < M of A[r, s][k] * Bop[n][s * ldt + k].
// The operator term of G takes one segment (A = lamF, Bop = DT), the fold of the delayed values one segment per delay index
// (A = the rows of the delayed copies in Gx, Bop = the transposed stack of W).
struct AdjointOpArgs {
    const double* A;        // row (r, s) at A + ((size_t)instance * a_inst + a_row0 + s * a_seg + j) * M
    const double* Bop;      // [M][ldb], ldb even, rows zero padded: segment s in columns s * ldt .. s * ldt + ldt - 1
    const double* add;      // epilogue 1: add + ((size_t)instance * add_inst + add_row0 + j) * M is added last (null: plain stores)
    double* out;            // out + ((size_t)instance * out_inst + out_row0 + j) * M
    int R, rpi, M, ldt, nseg, ldb;
    int a_inst, a_row0, a_seg, out_inst, out_row0, add_inst, add_row0;
};
// dst[n][seg * ldt + j] = src[seg][j][n] (diagonal kept or zeroed), rows of dst ld_dst long, each segment padded with zeros to ldt
hipError_t launch_adjoint_transpose(const double* dSrc, double* dDst, int M, int ldt, int ld_dst, int nseg, bool keep_diag, hipStream_t s);
bool adjoint_side_by_side(int B, int ns, int M);                      // batch large enough for the product to run beside the node kernel
hipError_t launch_adjoint_op(const AdjointArgs& a, hipStream_t s);    // operator term into the state rows of a.G ([B][ns+nc][M])
// tile: 0 = by the number of workgroups the rows give (as the operator term), 1 = 48 x 64, 2 = 96 x 128
hipError_t launch_adjoint_product(const AdjointOpArgs& a, int tile, hipStream_t s);
hipError_t launch_adjoint_nodes(const AdjointArgs& a, hipStream_t s);
hipError_t launch_adjoint_add(const double* dGop, double* dG, int B, int ns, int nv, int M, hipStream_t s);
hipError_t launch_kkt_certificate(const CertArgs& a, hipStream_t s);

// the relative local ODE error of a batch (emi_ode_error.hip; the model's residual kernel: emi_node_kernels.hpp)
// out[r][c] = sum_j V[r][j] OP[c][j]: V [R][K] rows one after the other, OP [N][ldk] (ldk even, >= K, rows zero padded), out rows
// ldo long, columns N .. ldo-1 untouched
struct InterpOpArgs {
    const double* V;
    const double* OP;
    double* out;
    int R, K, N, ldk, ldo;
};
hipError_t launch_interp_op(const InterpOpArgs& a, hipStream_t s);
// dst[k][j] = D[k][j], rows padded with a zero to the even ldk: the D block of the stacked operator [E | E' | D]
hipError_t launch_ode_copy_D(const double* D, double* dst, int M, int ldk, hipStream_t s);
hipError_t launch_ode_resid(int model, const OdeResidArgs<double>& a, hipStream_t s);
struct RtcModel;
hipError_t rtc_launch_ode_resid(RtcModel* m, const OdeResidArgs<double>& a, hipStream_t s);
hipError_t launch_ode_resid_tab(int model, const OdeResidArgs<double>& a, const double* tab, hipStream_t s);     // per-instance parameter table
hipError_t rtc_launch_ode_resid_tab(RtcModel* m, const OdeResidArgs<double>& a, const double* tab, hipStream_t s);
// ... of a context with delays (emi_ode_resid_delay_kernel)
hipError_t launch_ode_resid_delay(int model, const OdeResidDelayArgs<double>& a, hipStream_t s);
hipError_t rtc_launch_ode_resid_delay(RtcModel* m, const OdeResidDelayArgs<double>& a, hipStream_t s);
struct OdeFinishArgs {
    const double* X;        // [B][ns][M]
    const double* Zs;       // [B*ns][lds]: the D x block starts at column dcol
    const double* eta;      // [B][ns][M-1]
    double* err;            // [B]
    int B, M, ns, lds, dcol;
    double h;
};
hipError_t launch_ode_finish(const OdeFinishArgs& a, hipStream_t s);

// node blocks of the Newton step, assembled and made positive definite over [instance][node] (emi_kkt_blocks.hip)
struct BlocksArgs {
    const double *H, *VALS, *Sigma, *SigT;      // [B][nh][M], [B][nvals][M], [B][nv][M], [B][np][M]
    const unsigned char* fixed;                 // [B][nv][M]
    double dw_shift;
    double *Qexact, *Q;                         // [B][nh][M]; Qexact may be null
    int max_mods;
    int* count;                                 // [B] recorded pairs (the true number, also beyond max_mods)
    int* node;                                  // [B][max_mods]
    double *delta, *vec, *worst;                // [B][max_mods], [B][max_mods][nv], [B]
    int B, M, nv, np, nvals;
    int generic;                                // 1: the run-time-nv assembly kernel whatever nv is
    // path-row terms of every packed entry e, in row order then pair order: Q[e] += SigT[row] VALS[ea] VALS[eb]
    const int *term_ptr, *term_row, *term_ea, *term_eb;
    // workspace: [B][M] screen flags, flagged nodes (ascending), their number [B], pairs per flagged node; per flagged node the
    // pairs in eigenvalue order [B][M][nv] / [B][M][nv][nv] and the node's worst shift [B][M]
    int *flag, *list, *nflag, *cnt;
    double *tdelta, *tvec, *tworst;
};
hipError_t launch_kkt_blocks(const BlocksArgs& a, hipStream_t s);

// the array arithmetic of an interior-point iteration over [instance][node] (emi_ipm.hip).  One argument block for the six calls;
// each kernel reads and writes the members its call names (include/emi355x.h), the rest stay null.
struct IpmArgs {
    int B, M, ns, nc, np, nvals, nsets, reset;
    double *X, *U, *S, *E1, *E2;                            // point [B][ns][M], [B][nc][M], [B][np][M] x 3
    double *tX, *tU, *tS, *tE1, *tE2;                       // trial point
    double *LF, *Y, *ZL, *ZU, *VL, *VU, *W1, *W2;           // multipliers
    double *DZ, *DS, *DY, *DE1, *DE2, *DZL, *DZU, *DVL, *DVU, *DW1, *DW2;   // step; DZ [B][nv+ns][M] in the KKT unknown order
    double *Sigma, *SigT, *SigS, *RhatS, *Rt, *Rhs;         // what the reduction leaves
    const double *RES, *VALS, *G, *COST, *DefRes, *RowRes, *rs;
    const double *zl, *zu;                                  // [nsets][nv][M]
    const double* crow;                                     // [5][np]: cl, cu as given; cscale cl, cscale cu; cscale
    const double *par, *apr, *adu;                          // [B][4] = {mu, rho, tau, nu}; step lengths [B]
    const unsigned char* mask;                              // [B] or null
    const int *vptr, *vrow, *vent;                          // per variable: the path rows it enters and the VALS entries, in row order
    const int *rptr, *rvar, *rent;                          // per path row: (variable, VALS entry)
    double *part, *out;                                     // [B][chunks][<= 9] partials; the call's per-instance result
    // the lock-step driver's own array kernels (IPM_START_*, IPM_LAMC)
    unsigned char* fixedb;                                  // [B][nv][M] bytes: 1 where a variable is fixed (written by IPM_START_PUSH)
    double* LamC;                                           // [B][np][M] = cscale Y
    double push, frac;                                      // bound_push, bound_frac of the interior push
};
// IPM_START_PUSH: z pushed inside its bounds (fixed variables set to their bound), the fixed bytes, LamF = 0;  IPM_START_ROWS, after
// the first evaluation: S, E1, E2 from the path values, Y = 0, bound multipliers 1 where a bound exists, W1 / W2 from rho;
// IPM_RESET_W: W1 / W2 = max(1e-8, rho -+ Y) at the instances of `mask`;  IPM_LAMC: LamC = cscale Y;
// IPM_ERROR_PARTS: out[B][8], the components of the scaled KKT error (emi_ipm_error_parts_*)
enum { IPM_REDUCE, IPM_EXPAND, IPM_TRIAL, IPM_MERIT, IPM_ACCEPT, IPM_ERROR, IPM_ERROR_PARTS, IPM_START_PUSH, IPM_START_ROWS, IPM_RESET_W, IPM_LAMC };
constexpr int IPM_MAX_PARTIALS = 9;
int ipm_chunks(int M);
hipError_t launch_ipm(int what, const IpmArgs& a, hipStream_t s);

// model programs compiled at run time (emi_rtc.hip); the int results are EMI_* status codes
struct RtcModel;
int rtc_check(bool f32, const char* struct_name, const char* source, int ns, int nc, int npath, int pw, std::string* log);
int rtc_build(bool f32, const char* struct_name, const char* source, int ns, int nc, int npath, int pw, RtcModel** out, std::string* log);
void rtc_destroy(RtcModel* m);
bool rtc_has_symdefect(const RtcModel* m);
template <typename T>
hipError_t rtc_launch_nodes(RtcModel* m, const NodeArgs<T>& a, bool jac, bool defect_rows, hipStream_t s);
template <typename T> hipError_t rtc_launch_hess(RtcModel* m, const HessArgs<T>& a, hipStream_t s);
// ... with a per-instance parameter table (the tabled kernels of the model program; the node kernel with the defect rows)
template <typename T> hipError_t rtc_launch_nodes_tab(RtcModel* m, const NodeArgs<T>& a, const T* tab, bool jac, hipStream_t s);
template <typename T> hipError_t rtc_launch_hess_tab(RtcModel* m, const HessArgs<T>& a, const T* tab, hipStream_t s);
hipError_t rtc_launch_symdefect(RtcModel* m, const SymDefectArgs& a, hipStream_t s);
// the one-launch pass of a run-time compiled model: which state split it was compiled with for large batches (small ones take
// SW = 1), whether (sw, store mode) is available, and the launch
int rtc_pass_sw_large(const RtcModel* m);
hipError_t rtc_launch_pass(RtcModel* m, const SymDefectArgs& sa, const NodeArgs<double>& na, int sw, hipStream_t s, const PassWorkKey& key, const PassWork* work);
hipError_t rtc_launch_nodes_nt(RtcModel* m, const NodeArgs<double>& a, hipStream_t s);   // vec2, Jacobian, no defect rows, non-temporal stores

// Newton step on the device (emi_kkt.hip)
struct KktWorkspace;
int kkt_factor(KktWorkspace** w, hipStream_t stream, const double* dD, int M, int ns, int nv, const double* Qblk,
               const double* Jblk, const unsigned char* fixed, double dc, int method, int* info, std::string* err,
               bool blocks_on_device = false);      // Qblk, Jblk, fixed in device memory (copied on `stream`)
int kkt_solve(KktWorkspace* w, hipStream_t stream, int nz, double* rhs, int nrhs, std::string* err,
              bool rhs_on_device = false);          // rhs in device memory: solved in place, no copies, no synchronisation
bool kkt_set_option(const char* name, int value);   // process-wide diagnostics of the factorisation ("kkt_cholesky", ...)
int kkt_lowrank(KktWorkspace* w, hipStream_t stream, int nz, int r, const int* node, const double* vec, const double* delta,
                int* exact, std::string* err);
void kkt_destroy(KktWorkspace* w);
void kkt_last_regularisation(const KktWorkspace* w, double* dc, double* dw);
void kkt_mesh_changed(KktWorkspace* w);
bool kkt_is_schur(const KktWorkspace* w);            // holds a factorisation of the Schur path (what the batched solve takes)
// the Newton steps of n scenarios on one mesh at once (emi_kkt.hip, "Batched entry points")
// src != nullptr: the blocks of scenario b are instance src->inst[b] of one context's device arrays (Qblk / Jblk / fixed unused)
struct KktShardSrc {
    const double* Q;            // [B][nh][M]
    const double* VALS;         // [B][nvals][M]: the first ns nv rows of an instance are its Jacobian node entries
    const unsigned char* fixed; // [B][nv][M]
    size_t vals_stride;         // nvals M
    const int* inst;            // [n]
};
int kkt_factor_batch(int n, KktWorkspace** const* pws, hipStream_t stream, const double* const* dD, int M, int ns, int nv,
                     const double* const* Qblk, const double* const* Jblk, const unsigned char* const* fixed, const double* dc, int* info,
                     std::string* err, const KktShardSrc* src = nullptr);
// rhs_on_device: rhs[b] are device arrays, solved in place (kkt_solve_batch then does not synchronise)
int kkt_solve_batch(int n, KktWorkspace* const* ws, hipStream_t stream, int nz, double* const* rhs, std::string* err,
                    bool rhs_on_device = false);
int kkt_solve_refined_batch(int n, KktWorkspace* const* ws, hipStream_t stream, double* const* rhs, const double* dc_nominal, int max_steps,
                            double* rel, int* nsolve, int* reverted, int* status, std::string* err, bool rhs_on_device = false);
// the instances of one context (emi_kkt_*_shard_dev)
int kkt_holds(const KktWorkspace* w, int M, int ns, int nv);      // 0 nothing for this shape, 1 Schur factorisation, 2 LU
int kkt_lowrank_shard(int n, KktWorkspace* const* ws, hipStream_t stream, int max_mods, const int* inst, const int* count, const int* dNode,
                      const double* dDelta, const double* dVec, int* exact, std::string* err);
void kkt_forget_ladder(KktWorkspace* w);        // the next factorisation starts at the nominal regularisation level again

// the lock-step interior-point driver of one context's batch (emi_ipm_solve.hip); its device arrays live in an IpmSolveWs the
// context owns
struct IpmSolveWs;
void ipm_solve_destroy(IpmSolveWs* w);
// dX .. dLamC device arrays; returns an EMI_* status with the context's message set (its own, or that of the emi_*_dev call that failed)
int ipm_solve_shard(emi_ctx_t c, void* dX, void* dU, const emi_ipm_bounds_t* bd, const emi_ipm_options_t& opt, void* dLamF, void* dLamC,
                    emi_ipm_result_t* results);

// the iterate of the instances of `mask` copied between the live arrays and a kept set (emi_ipm_solve.hip: emi_ipm_keep_kernel).
// live / kept in the order X U S E1 E2 LamF Y ZL ZU VL VU W1 W2; mask [B] device bytes or null; restore: kept -> live
struct IpmKeepArgs {
    double* live[13];
    double* kept[13];
    const unsigned char* mask;
    int B, M, ns, nc, np, restore;
};
hipError_t launch_ipm_keep(const IpmKeepArgs& a, hipStream_t s);

// the mesh ladder of one context's batch (emi_ipm_ladder.hip): prolongation Vf[r] = P Vc[src(r)] from PT[Mc][Mf] for R rows of Mf
// values, src(r) = map[r / group] * group + r % group (map null: src(r) = r; group: rows that share one entry of the map); the repair
// of the position states X[B][ns][M] against the record table (recs [path_sets][np][EMI_PATH_REC], tracks [track_sets][ntracks][M]);
// and the driver over the rungs, whose device arrays live in an IpmLadderWs the context owns
hipError_t launch_prolong_rows(const double* PT, const double* Vc, const int* map, int group, double* Vf, int Mc, int Mf, int R, hipStream_t s);
struct RepairArgs {
    double* X;
    const double *recs, *trkx, *trky;
    int B, ns, M, np, path_sets, px, py, ntracks, track_sets;
};
hipError_t launch_repair_guess(const RepairArgs& a, hipStream_t s);
// the centres of the track rows on a mesh from waypoint tables t, x, y [sets][ntracks][ld] (cnt [sets][ntracks] waypoints each):
// xc, yc [n][ntracks][M] of type T at the node times node_t [M], result set i from waypoint set map[i] (a null map: i).  The
// arithmetic of emi_track_centres (csrc/emi_host.cpp) per (set, track, node), in double, stored as T
struct TrackWaypointArgs {
    const double *t, *x, *y, *node_t;
    const int *cnt, *map;
    void *xc, *yc;
    int n, ntracks, ld, M, first;       // first: the (set, track) pair of blockIdx.y == 0 (more pairs than one grid go out in pieces)
};
template <typename T> hipError_t launch_track_waypoints(TrackWaypointArgs a, hipStream_t s);
struct IpmLadderWs;
void ipm_ladder_destroy(IpmLadderWs* w);
// the starts of one context's batch (emi_start_guess.hip): line, bend and planned route into X[B][ns][M].  par: per set xa [ns] |
// xb [ns] | box [4]; tau, sine [M]; cost, dist, extra, cells, bits: [B][N^2] of the context's StartGuessWs (PLANNED only)
struct StartArgs {
    double* X;
    int* level;
    const double *recs, *par, *tau, *sine;
    double *cost, *dist, *extra;
    int* cells;
    unsigned char* bits;
    int B, ns, M, np, path_sets, px, py, nsets, kind, N, has_box;
    double bend, clearance;
};
struct StartGuessWs;
void start_guess_destroy(StartGuessWs* w);
// the call after its checks: uploads the parameters (that copy drains the stream), launches the kernels, returns an EMI_* status
int start_guess(emi_ctx_t c, const emi_start_t& st, void* dX, void* dLevel);
int ipm_solve_ladder(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const void* dX0, const void* dU0, void* dX,
                     void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results);
// the move of the instances of a list between two sets of arrays [instance][rows][ld], entry i: instance sidx[i] of src -> instance
// didx[i] of dst (a null list: i), the first `len` values of every row; and the same driver with the instances that meet the ODE
// tolerance retired rung by rung (emi_ipm_solve_refine_*)
constexpr int SHARD_MOVE_ARRAYS = 4;
struct ShardMoveArgs {
    const double* src[SHARD_MOVE_ARRAYS];
    double* dst[SHARD_MOVE_ARRAYS];
    int rows[SHARD_MOVE_ARRAYS], sld[SHARD_MOVE_ARRAYS], dld[SHARD_MOVE_ARRAYS];
    const int *sidx, *didx;
    int n, narrays, len, first;         // first: the list entry of blockIdx.y == 0 (lists beyond one grid go out in pieces)
};
hipError_t launch_shard_move(ShardMoveArgs a, hipStream_t s);
int ipm_solve_refine(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t& rf, const void* dX0,
                     const void* dU0, int ldm, void* dX, void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results, double* err,
                     emi_ipm_refine_result_t* out);
// ... and that driver once per attempt, from one start after another, on the instances no earlier attempt solved (emi_ipm_solve_restart_*)
int ipm_solve_restart(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                      const emi_ipm_restart_t& rs, const void* dX0, const void* dU0, int ldm, void* dX, void* dU, void* dLamF, void* dLamC,
                      emi_ipm_result_t* results, double* err, emi_ipm_restart_result_t* out);

}  // namespace emi
