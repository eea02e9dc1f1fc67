/*
 * emi355x.h -- C ABI of libemi355x, the MI355X (gfx950) collocation evaluator.
 *
 * This is the drop-in boundary of the eMI355X eSolver.  It is the only thing
 * `src/eMI355X/eMI355X.cpp` (our ETOL::TrajectoryOptimizer peer of ePSOPT)
 * calls to reach the GPU.  Plain pointers and sizes only: no C++ types, no
 * torch types, no exceptions cross this boundary; every call returns an int
 * status (EMI_OK == 0) and the text of the last failure is kept per context.
 *
 * What each entry point replaces in the reference (paths under the ETOL tree;
 * "[PSOPT]" marks arithmetic that the reference delegates to PSOPT 5.0.0,
 * whose sources are not part of the reference tree):
 *
 *   emi_lgl            [PSOPT] LGL nodes / weights / differentiation matrix
 *                      selected by  src/ePSOPT/ePSOPT.cpp:68
 *                      (collocation_method = "Legendre"), node count :44-45
 *   emi_set_mesh       the (t0,tf) fixed-horizon mapping, ePSOPT.cpp:151-154
 *   emi_set_model      the per-node callbacks installed at ePSOPT.cpp:76-80
 *                      (integrand_cost :186-216, dae :218-276) -- the user's
 *                      f_t closures cannot run on the device, so a model id
 *                      + parameter block selects a hand-written kernel
 *   emi_set_model_source  the same callbacks for a model the library has no
 *                      kernel for: where ePSOPT records the user's closures on
 *                      an ADOL-C tape and interprets it at every evaluation
 *                      (derivatives = "automatic", ePSOPT.cpp:64), the host
 *                      records them once, differentiates the trace and hands
 *                      over the text of a model struct; it is compiled for
 *                      gfx950 at this call and runs in the same kernels
 *   emi_set_path       the path rows counted at ePSOPT.cpp:58 and produced
 *                      at :261-270; row formulas follow
 *                      src/Examples/PSOPT/etol_psopt_example1.cpp:163-182
 *                      (ellipse per polygon edge) and :243-247 (disc)
 *   emi_set_tracks     moving-disc centres, etol_psopt_example1.cpp:233-241
 *   emi_eval_*         one pass of the hot loop of ::psopt (ePSOPT.cpp:84):
 *                      dae + integrand_cost at every node, the defect
 *                      D.X - (tf-t0)/2.F, the cost quadrature, and what
 *                      ADOL-C's sparse_jac/gradient drivers return [PSOPT]
 *   emi_hess_*         what ADOL-C's sparse_hess returns for hessian="exact"
 *                      (ePSOPT.cpp:65) [PSOPT]
 *   emi_jac_structure  the sparsity pattern IPOPT is given [PSOPT]
 *   emi_kkt_factor/_solve  the linear solve of IPOPT's Newton step, reached
 *                      through ::psopt at ePSOPT.cpp:84 with nlp_method "IPOPT"
 *                      (:62) [IPOPT]: the primal-dual KKT matrix is assembled
 *                      and factorised on the device
 *   emi_kkt_solve_refined  the iterative refinement IPOPT wraps around that
 *                      solve [IPOPT]: residual, correction and the revert of
 *                      a correction that made it worse stay on the device
 *   emi_kkt_*_batch    no counterpart: the reference runs one trajectory per
 *                      process; the Newton steps of several scenarios on one
 *                      mesh go through one sequence of batched launches
 *   emi_lagr_grad_* / emi_kkt_certificate_*  the derivative checks and the dual_inf / compl_inf figures IPOPT
 *                      reports behind ePSOPT.cpp:62-67 [IPOPT]: the gradient of the Lagrangian
 *                      grad f + J^T lambda of a batch of trajectories (the adjoint of the defect pass, D^T on
 *                      the matrix pipe) and, per trajectory, stationarity / complementarity / feasibility
 *                      maxima in the caller's units, without an activity tolerance
 *   emi_lagr_grad_total_* / emi_kkt_certificate_total_*  the same for a problem with delayed states / controls
 *                      (ePSOPT.cpp:231-248): the adjoints of the delayed values folded onto the trajectory
 *                      through the transposes of the interpolation operators W(i dt), on the matrix pipe
 *   emi_plan_pass      no counterpart: the launch form emi_eval_* takes for a
 *                      batch size, so that tests and tools query the policy
 *                      instead of restating it
 *
 * Threading: a context must be driven by one caller thread at a time
 * (the reference is single-threaded throughout).
 * Different contexts may be driven by different threads concurrently (each
 * owns its streams, rocBLAS handle and workspaces); results do not depend
 * on what runs beside a context (tests/test_gpu_kkt.py,
 * test_concurrent_contexts_give_reproducible_factorisations).
 *
 * Data layout (all arrays dense, real type = double unless the context was
 * created with emi_create_f32):
 *   X     [B][ns][M]   state trajectories, node index fastest
 *   U     [B][nc][M]   control trajectories
 *   RES   [B][ns+np][M]  rows 0..ns-1  : defect  (D.X)_i,k - h f_i(x_k,u_k,t_k)
 *                        rows ns..     : path constraint values c_j(x_k,t_k)
 *   VALS  [B][nvals][M], nvals = ns*(ns+nc) + 2*np + (ns+nc):
 *           entry i*(ns+nc)+v        : d defect_(i,k) / d z_(v,k)
 *                                      = -h df_i/dz_v + (v==i ? D_kk : 0)
 *           entry ns*(ns+nc)+2j+{0,1}: d c_j / d (px, py) at node k   (rows of the record table, emi_set_path)
 *           then PW entries per row traced from callbacks (emi_set_model_source)
 *           last ns+nc entries        : d cost / d z_(v,k) = sgn h w_k dL/dz_v
 *   COST  [B]          sgn h sum_k w_k L(x_k,u_k)   (sgn=-1 when maximising,
 *                      ePSOPT.cpp:212-213)
 *   h = (tf - t0)/2,  z_(v,k): v<ns -> state v, else control v-ns.
 */
#ifndef EMI355X_H_
#define EMI355X_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMI_ABI_VERSION 2

typedef struct emi_ctx_s* emi_ctx_t;

/* status codes */
enum {
    EMI_OK = 0,
    EMI_ERR_ARG = 1,          /* bad argument (null pointer, size mismatch) */
    EMI_ERR_STATE = 2,        /* call made before its prerequisites */
    EMI_ERR_HIP = 3,          /* a HIP runtime call failed */
    EMI_ERR_NO_DEVICE = 4,    /* no usable gfx950 device */
    EMI_ERR_UNSUPPORTED = 5,  /* valid request this build has no kernel for */
    EMI_ERR_COMM = 6          /* RCCL failure */
};

/* built-in node models (emi_set_model) */
enum {
    EMI_MODEL_POINTMASS2D = 0,  /* ns=2 nc=2: etol_psopt_example1.cpp:101-138 */
    EMI_MODEL_QUADROTOR2D = 1,  /* ns=6 nc=2: planar quadrotor (build-defined) */
    EMI_MODEL_FIXEDWING12 = 2,  /* ns=12 nc=4: rigid-body fixed wing (build-defined) */
    EMI_MODEL_SOURCE = 100      /* installed by emi_set_model_source (emi_layout_t.model)  */
};

/* path-row kinds; one record = EMI_PATH_REC reals: {kind, c0..c6} */
enum {
    EMI_PATH_ELLIPSE = 0, /* c = {xc, yc, cos tt, sin tt, a^2, b^2, -}      */
    EMI_PATH_DISC = 1,    /* c = {xc, yc, r^2, -, -, -, -}                  */
    EMI_PATH_TRACK = 2    /* c = {track index, r^2, -, ...}: centre per node */
};
#define EMI_PATH_REC 8

/* emi_eval flags */
enum {
    EMI_EVAL_NODES = 1u,   /* K1+K2+K3+K5: node functions, Jacobian values   */
    EMI_EVAL_DEFECT = 2u,  /* K4: accumulate D.X into the defect rows        */
    EMI_EVAL_ALL = 3u,
    EMI_EVAL_NOJAC = 4u,   /* values only (line-search evaluations)          */
    EMI_EVAL_KEEP_INVARIANT = 8u  /* leave the model-invariant VALS rows as they are: see emi_eval_dev */
};

typedef struct {
    int model, ns, nc, np, M, B;
    int nres;    /* ns + np                        */
    int nvals;   /* ns*(ns+nc) + 2*np_table + PW*np_traced + (ns+nc) */
    int nhess;   /* (ns+nc)*(ns+nc+1)/2            */
    int real_bytes; /* 8 (f64) or 4 (f32)          */
    int px, py;  /* state indices the keep-outs act on */
    double t0, tf;
} emi_layout_t;

/* ---- library ---------------------------------------------------------- */
int emi_abi_version(void);
const char* emi_status_string(int status);
int emi_device_count(int* count);

/* ---- host-side mesh construction (no device needed) -------------------- */
/* LGL nodes tau[M] (ascending, -1..1), weights w[M], D[M*M] row-major.     */
int emi_lgl(int M, double* tau, double* w, double* D);
int emi_model_dims(int model, int* ns, int* nc, int* nparams);
/* ellipse record from one polygon edge (a->b); follows the arithmetic of
 * etol_psopt_example1.cpp:163-182 term by term.                            */
int emi_edge_ellipse(double xa, double ya, double xb, double yb, double* rec8);
/* linear interpolation of a waypoint table at the node times; follows
 * TrajectoryOptimizer.hpp:239-258 (bracket search) term by term.           */
int emi_track_centres(int nway, const double* t, const double* x, const double* y,
                      int M, const double* node_t, double* xc, double* yc);

/* ---- context ------------------------------------------------------------ */
int emi_create(int device_id, emi_ctx_t* out);       /* f64 arithmetic */
int emi_create_f32(int device_id, emi_ctx_t* out);   /* f32 arithmetic */
int emi_destroy(emi_ctx_t ctx);
const char* emi_last_error(emi_ctx_t ctx);
int emi_set_stream(emi_ctx_t ctx, void* hip_stream); /* NULL = own stream */
int emi_get_stream(emi_ctx_t ctx, void** hip_stream);
int emi_synchronize(emi_ctx_t ctx);

/* ---- problem definition ------------------------------------------------- */
/* D may be NULL: a points-only mesh (abscissae tau and weights w without a
 * differentiation matrix), for evaluating the node functions BETWEEN the collocation
 * nodes (the ODE-error estimate of the mesh refinement); such a context accepts
 * EMI_EVAL_NODES only.                                                            */
int emi_set_mesh(emi_ctx_t ctx, int M, const double* tau, const double* w,
                 const double* D, double t0, double tf);
/* Selects a built-in model.  emi_set_model and emi_set_model_source DROP the path-row
 * table of the context (np = 0: its px / py name states of the previous model, which
 * the new one need not have): emi_set_path, and emi_set_tracks where rows of kind
 * EMI_PATH_TRACK are used, must follow every model change.                        */
int emi_set_model(emi_ctx_t ctx, int model, const double* params, int nparams,
                  int maximize);
/* Model given as C++ text: the definition of
 *     template <typename T> struct <struct_name> { NS, NC, NV, f, jac, cost, grad, hess };
 * with the interface of the built-in models (etol_amd/csrc/emi_models.hpp; the
 * text may use EMI_DEV, ModelParams<T> and the emi_sin/cos/tan/exp/log/sqrt/pow
 * helpers).  It is compiled for gfx950 here (hiprtc) together with the
 * library's kernel templates; on a compile error the status is EMI_ERR_ARG and
 * emi_last_error() holds the compiler log.  params (<= 16) reach the struct as
 * ModelParams<T>.  npath = number of path rows the struct computes itself
 * (NPATH, PW, pvar(), path() / path_hess(): constraint callbacks traced by the
 * host); they follow the rows of emi_set_path in RES.  A traced row may depend on
 * any states and controls of its node: path_vars[n_path_vars] (ascending variable
 * indices, states first) is the union over the rows, and VALS holds n_path_vars
 * partials per traced row (entry ns*(ns+nc) + 2*np_table + j*n_path_vars + q =
 * d c_j / d z_path_vars[q]) between the table rows' pairs and the cost gradient.
 * Replaces a previous emi_set_model / emi_set_model_source (and, like them, drops
 * the table of emi_set_path).                                                  */
int emi_set_model_source(emi_ctx_t ctx, const char* struct_name, const char* source,
                         int ns, int nc, int npath, const int* path_vars, int n_path_vars,
                         const double* params, int nparams, int maximize);
/* Compile-only check of such a text (no device needed): EMI_OK or EMI_ERR_ARG
 * with up to log_len-1 characters of the compiler log in log (may be NULL).   */
int emi_check_model_source(const char* struct_name, const char* source, int ns,
                           int nc, int npath, int n_path_vars, int f32, char* log, size_t log_len);
int emi_set_batch(emi_ctx_t ctx, int B);
/* PER-INSTANCE MODEL PARAMETERS: params host [nsets][nparams], row b the parameter set of instance b (mass, inertia, aero
 * coefficients, cost weights of a dispersion study) in place of the one set of emi_set_model*.  nsets == B and nparams the
 * model's count (emi_model_dims; what emi_set_model_source was given), else EMI_ERR_ARG; no model or no batch yet:
 * EMI_ERR_STATE.  The context keeps the table on the device in its own real type, rounded once as emi_set_model rounds its set.
 * nsets == 0 (params may be NULL) removes the table: the context has the shared set again, with the launch policy and the bits
 * of a context that never had a table.
 * While a table is in force every kernel that evaluates the model (node, Hessian and ODE-residual kernels, built-in and run-time
 * compiled models, both precisions) runs in an instantiation that reads row b once per workgroup, by scalar loads, and an
 * evaluation pass takes the sequential route -- node kernel, then defect kernel: what the option "overlap" 0 selects, at every
 * mesh and batch size (the one-launch pass and the MFMA defect forms evaluate f for 16 instances per tile and have no tabled
 * form); emi_plan_pass and emi_last_path report that.  Instance b has the bits of a context of the same B, M and tables that
 * holds row b as its shared set under "overlap" 0.  emi_eval_*, emi_hess_*, emi_ode_error_*, emi_ipm_solve_shard_* and
 * emi_ipm_solve_ladder_* take such a context; emi_ipm_solve_refine_* and emi_ipm_solve_restart_*, which compact the batch,
 * return EMI_ERR_UNSUPPORTED.  Contexts with delays: EMI_ERR_UNSUPPORTED here, and from emi_set_delays once a table is set.
 * The table survives emi_set_mesh, emi_set_path, emi_set_tracks, emi_set_track_waypoints and emi_set_stream; emi_set_model,
 * emi_set_model_source and an emi_set_batch to another B drop it.  Setting or removing it voids the record of
 * EMI_EVAL_KEEP_INVARIANT (the model-invariant Jacobian rows depend on the parameters).  Synchronises, as emi_set_path does.
 * emi_get_model_params_batch: what is in force -- *nsets 0 (none) or B, *nparams the model's count, params (NULL: not wanted)
 * the rows as they were given, [nsets][nparams].                                                                          */
int emi_set_model_params_batch(emi_ctx_t ctx, const double* params, int nsets, int nparams);
int emi_get_model_params_batch(emi_ctx_t ctx, double* params, int* nsets, int* nparams);
/* Delayed states and controls -- what ePSOPT::dae appends to the callbacks' x and u through PSOPT's get_delayed_state /
 * get_delayed_control (reference src/ePSOPT/ePSOPT.cpp:231-248): x(t - i dt) of every state for i = 1 .. x_horizon - 1 and
 * u(t - i dt) of every control for i = 1 .. u_horizon.  On the device they are extra INPUTS of the node functions: the model
 * (emi_set_model_source) is written with nc_model = nc + (x_horizon - 1) ns + u_horizon nc controls, ordered
 *     [ u (nc) | x(t - dt) (ns) | .. | x(t - (x_horizon-1) dt) | u(t - dt) (nc) | .. | u(t - u_horizon dt) ],
 * the caller keeps passing U[B][nc][M], and every evaluation first forms the delayed rows as W(i dt) . (node values) on the
 * MFMA defect kernel: W(delay)[k][j] = Lagrange basis polynomial j of the LGL nodes at t_k - delay (the value of the
 * collocation polynomial -- PSOPT's "Legendre" interpolation), with t_k - delay CLAMPED to t0: PSOPT 5.0.0 is not part of the
 * reference tree, and this build takes the history of a delayed variable before t0 to be its value at t0.
 * VALS / H then hold partials with respect to the delayed inputs as they hold those of the controls (entries of the extended
 * node-variable vector); the total derivative with respect to the trajectory is (d . / d delayed) . W -- W stays an operator,
 * like the off-diagonal part of I (x) D; emi_lagr_grad_total_* applies it to the Lagrangian gradient.  emi_get_layout reports nc = nc_model; emi_get_delays the split.  Must follow
 * emi_set_model_source (a model change drops the delays).  Horizons 0 / 1 and 0: no delayed values, as the reference.    */
int emi_set_delays(emi_ctx_t ctx, int x_horizon, int u_horizon, double dt);
int emi_get_delays(emi_ctx_t ctx, int* x_horizon, int* u_horizon, int* n_delayed);
/* W(delay)[M][M] as above, on the host (no device needed)                                                                   */
int emi_delay_matrix(int M, const double* tau, const double* w, double t0, double tf, double delay, double* W);
/* recs: [nsets][np][EMI_PATH_REC]; nsets is 1 (shared) or B (per instance) */
int emi_set_path(emi_ctx_t ctx, int np, int nsets, const double* recs,
                 int px_state, int py_state);
/* xc, yc: [nsets][ntracks][M] disc centres at the node times               */
int emi_set_tracks(emi_ctx_t ctx, int ntracks, int nsets, const double* xc,
                   const double* yc);
/* The centres of the tracks from WAYPOINT TABLES kept on the device, for whatever mesh the context is on -- the device route to what
 * emi_track_centres per track plus emi_set_tracks do from the host, and what the mesh ladder calls per rung.
 * emi_set_track_waypoints: t, x, y host [nsets][ntracks][ld]; counts host [nsets][ntracks], the waypoints of each track, each in
 * 2 .. ld (NULL: ld everywhere; what lies behind a track's count is never read).  Times strictly ascending within a count, else
 * EMI_ERR_ARG naming set and track; EMI_ERR_ARG also for a count outside 2 .. ld and a NULL table.  The tables are kept as
 * doubles in every context and belong to no mesh, model or batch: they survive emi_set_mesh, emi_set_model* and emi_set_batch,
 * and only ntracks = 0 drops them.  Needs no mesh; touches neither the centres the context holds nor the record of
 * EMI_EVAL_KEEP_INVARIANT.  Synchronises.
 * emi_tracks_from_waypoints_dev: writes the centre arrays of the context (those of emi_set_tracks) at the context's node times.
 * dSetMap NULL (n = 0 or nsets): result set s from waypoint set s.  Otherwise n device ints in [0, nsets), result set i from
 * waypoint set dSetMap[i]: a permutation compacts, a repeated value copies; values in range are the caller's duty.  Afterwards
 * the context holds ntracks tracks in n (or nsets) sets, as after emi_set_tracks (also for EMI_EVAL_KEEP_INVARIANT); the batch
 * need not match yet -- the next evaluation checks that.  Per (set, track, node) the statements of emi_track_centres, every
 * operation rounded once, none fused: the bits are that function's; in an f32 context computed in double at the double node
 * times and stored with the conversion of emi_set_tracks.  Asynchronous on the context's stream, one writer per output, two
 * calls give the same bits.  EMI_ERR_STATE: no mesh, no waypoints.  EMI_ERR_ARG: n < 0, n other than 0 or nsets with a NULL map,
 * n = 0 with a map.
 * emi_get_tracks: synchronises and returns the centres the context holds, [sets][ntracks][M] doubles each; EMI_ERR_STATE where
 * it holds none (no mesh, or none set since emi_set_mesh).                                                                    */
int emi_set_track_waypoints(emi_ctx_t ctx, int ntracks, int nsets, int ld, const int* counts, const double* t, const double* x,
                            const double* y);
int emi_tracks_from_waypoints_dev(emi_ctx_t ctx, int n, const void* dSetMap);
int emi_get_tracks(emi_ctx_t ctx, double* xc, double* yc);
int emi_get_layout(emi_ctx_t ctx, emi_layout_t* out);

/* ---- Newton step of the NLP iteration (batch of one, f64 contexts) --------
 * KKT matrix of one instance, N = (ns+nc+ns)*M rows:
 *     [ Q    J^T ]   Q: node-block-diagonal, Qblk [nhess][M] packed lower
 *     [ J  -dc I ]      triangles (layout of emi_hess_*: Hessian blocks plus
 *                       whatever diagonal / path-row terms the caller adds)
 *                    J: D (x) [I 0] off the node diagonal, Jblk [ns*(ns+nc)][M]
 *                       on it (the defect entries of VALS, which hold D_kk)
 * Unknown order: variables v*M+k, then defect multipliers i*M+k.  fixed
 * [(ns+nc)*M]: 1 = the variable does not move (identity row/column, rhs 0).
 * Host pointers.  *info = 0 factorised, > 0 singular.
 * Option "kkt_method" (emi_set_option): 1 (default) factorises the Schur
 * complement J Q^-1 J^T + dc I with a Cholesky -- valid when every Q block is
 * positive definite, which also fixes the inertia of K by construction; a
 * matrix that is not takes method 0 automatically: K assembled in HBM and
 * LU-factorised.  Neither reports an inertia; see emi_kkt_lowrank.           */
int emi_kkt_factor(emi_ctx_t ctx, const double* Qblk, const double* Jblk,
                   const unsigned char* fixed, double dc, int* info);
/* Low-rank correction of the factorised matrix: K = K~ - sum_c delta_c u_c u_c^T,
 * u_c = vec[c][0..nv) placed on the variables of node[c] (what the caller added
 * to make the Q blocks positive definite).  K~^-1 U and the Cholesky factor of
 * C = Delta^-1 - U^T K~^-1 U stay on the device.  *exact = 1 iff C is positive
 * definite, i.e. iff K has the inertia of K~; emi_kkt_solve then returns
 * solutions of K (Woodbury), else of K~.  r = 0 clears the correction.  The
 * columns may come in any order (they are kept sorted by node) and for any
 * number of variables per node the factorisation took.                      */
int emi_kkt_lowrank(emi_ctx_t ctx, int r, const int* node, const double* vec,
                    const double* delta, int* exact);
/* The Newton steps of n scenarios at once: ctxs[b] are n DIFFERENT contexts on one
 * device with the same mesh size and model dimensions, each with its own mesh
 * (emi_set_mesh: tau and D may differ between them) (one scenario of a
 * Monte-Carlo batch each, BASELINE configs[3]); arguments per scenario as the
 * single entry points take them (host pointers).  Every launch of the
 * factorisation then carries the whole batch -- the 96-step dependency chain of a
 * 1024-node Cholesky is paid once per batch instead of once per scenario -- on
 * ctxs[0]'s stream; each context keeps its own factors, so emi_kkt_lowrank /
 * emi_kkt_solve / emi_kkt_solve_batch may follow in any grouping.  A scenario
 * the batch cannot take (a node block that is not positive definite, one
 * whose regularisation ladder is exhausted, or any scenario of a model with more
 * than 16 variables per node) is factorised through emi_kkt_factor inside the
 * call.  info[b] as emi_kkt_factor's.  What IPOPT does
 * once per scenario behind ePSOPT (reference src/ePSOPT/ePSOPT.cpp:62-66, 84).     */
int emi_kkt_factor_batch(int n, const emi_ctx_t* ctxs, const double* const* Qblk,
                         const double* const* Jblk, const unsigned char* const* fixed,
                         const double* dc, int* info);
/* one right-hand side [N] per scenario, in place (host pointers); low-rank
 * corrections of the scenarios that hold one are applied                          */
int emi_kkt_solve_batch(int n, const emi_ctx_t* ctxs, double* const* rhs);
/* 1 if the context holds a factorisation of the Schur path (what the batched and refined solves take), else 0 */
int emi_kkt_is_schur(emi_ctx_t ctx);
/* The Newton step WITH its iterative refinement on the device: x = K~^-1 b, then
 * up to max_steps rounds of  r = b - K x,  x += K~^-1 r  against the NOMINAL
 * matrix K -- the node blocks and dc_nominal the caller handed emi_kkt_factor
 * (the factorisation may hold a regularised matrix: emi_kkt_last_regularisation),
 * minus the low-rank term while emi_kkt_lowrank reported "exact".  A round stops
 * when the residual is at round-off or no longer halves; a correction that made
 * the residual worse is taken back.  Only residual norms cross to the host.  Out:
 * rel = final max|r| / max(1, max|b|), nsolve = solves with the factors used,
 * reverted = 1 if the last correction was taken back, status = 0 ok / 2 the first
 * solution is not finite.  Schur-path factorisations only (EMI_ERR_UNSUPPORTED
 * otherwise: refine around emi_kkt_solve).  What IPOPT's own iterative refinement
 * does behind ePSOPT (reference src/ePSOPT/ePSOPT.cpp:62-66).                     */
int emi_kkt_solve_refined(emi_ctx_t ctx, double* rhs, double dc_nominal, int max_steps,
                          double* rel, int* nsolve, int* reverted, int* status);
int emi_kkt_solve_refined_batch(int n, const emi_ctx_t* ctxs, double* const* rhs,
                                const double* dc_nominal, int max_steps, double* rel,
                                int* nsolve, int* reverted, int* status);
/* What the last emi_kkt_factor really factorised: [[Q + dw I_x, J^T], [J, -dc I]]
 * with dw on the diagonal of the free STATE variables.  dc >= the caller's and
 * dw >= 0; they exceed the nominal (dc, 0) when the Schur path had to climb its
 * regularisation ladder (csrc/emi_kkt.hip).  A caller that refines its step
 * against the nominal matrix reads them to know the step is inexact -- what
 * IPOPT's delta_w / delta_c tell its own iteration
 * (reference src/ePSOPT/ePSOPT.cpp:62-66: nlp_method "IPOPT").                */
int emi_kkt_last_regularisation(emi_ctx_t ctx, double* dc, double* dw);
/* emi_kkt_factor with Qblk, Jblk and fixed in DEVICE memory (copied on the context's stream: e.g. the dQ of
 * emi_kkt_blocks_dev and the first ns*nv rows of VALS); everything behind the copies is emi_kkt_factor.       */
int emi_kkt_factor_dev(emi_ctx_t ctx, const void* dQblk, const void* dJblk, const void* dFixed, double dc, int* info);

/* ---- the node blocks of the Newton step, assembled and made positive definite on the device (f64 contexts, ns+nc <= 16) ----
 * What an interior-point iteration puts in front of emi_kkt_factor, for the B instances of the context at once:
 *   Q[v][q] = H[v][q] + (v == q: Sigma[v] + (fixed[v] ? 0 : dw_shift)) + sum over path rows j, pairs a, b <= a of row j with
 *             {var_a, var_b} = {v, q}:  SigT[j] VALS[entry_a] VALS[entry_b]         (rows ascending, pairs in list order)
 * H[B][nhess][M], VALS[B][nvals][M], Sigma[B][ns+nc][M] (0 where fixed), SigT[B][np][M] (NULL when np == 0), fixed[B][ns+nc][M]
 * bytes.  Qexact (may be NULL) and Q receive the sum.  Then per block, on a working copy with identity rows / columns for fixed
 * variables and the scaling d_v = sqrt(max(|A_vv|, 1e-12 max|A|)): a Cholesky screen (pivot <= 1e-8 fails).  A block that
 * passes stays in Q as assembled, bit for bit.  A block that fails gets a Jacobi eigen-decomposition of the scaled block (to
 * off^2 < 1e-32 max(1, dia^2), at most 30 sweeps); with nl = max(|lambda|, 1e-9), Q~ = d o (V diag(nl) V^T) o d replaces the
 * entries of Q whose two variables are free, and every eigenvalue < -1e-9 is recorded: delta = nl - lambda, vec = d o v, so
 * that Q~ = Q + sum delta vec vec^T up to the floored (|lambda| <= 1e-9) ones -- the columns emi_kkt_lowrank takes.
 * The list of an instance is ordered by node, then by eigenvalue (ascending); count[b] is the TRUE number of recorded pairs,
 * of which the first min(count, max_mods) are written to node[B][max_mods] / delta[B][max_mods] / vec[B][max_mods][ns+nc]
 * (nothing is written behind them; max_mods 0: the three may be NULL).  worst[b] = max delta d_0^2 over the recorded pairs.
 * No atomics, every sum in a fixed order: two calls give the same bits.
 * emi_kkt_blocks_rows gives the (variable, VALS entry) pairs of every path row (CSR: row_ptr[np + 1]); np must be the
 * context's number of path rows.  Without it, a context whose rows all come from the record table takes (px, ns*nv + 2j),
 * (py, ns*nv + 2j + 1) as emi_jac_structure lays them out.
 * EMI_ERR_UNSUPPORTED: f32 context, or ns+nc > 16;  EMI_ERR_STATE: rows traced by the model (emi_set_model_source npath > 0)
 * and no list, or a list of another length;  EMI_ERR_ARG: a pair out of range.  The _dev form is asynchronous on the
 * context's stream; the _host form copies in, runs it, copies out and synchronises.  Option "blocks_generic" 1 (emi_set_option,
 * a test switch): the assembly kernel with the block size as a run-time value also where a compiled size (4, 8, 16) exists.  */
int emi_kkt_blocks_rows(emi_ctx_t ctx, int np, const int* row_ptr, const int* var, const int* entry);
int emi_kkt_blocks_dev(emi_ctx_t ctx, const void* dH, const void* dVALS, const void* dSigma, const void* dSigT,
                       const void* dFixed, double dw_shift, void* dQexact, void* dQ, int max_mods, void* dCount, void* dNode,
                       void* dDelta, void* dVec, void* dWorst);
int emi_kkt_blocks_host(emi_ctx_t ctx, const double* H, const double* VALS, const double* Sigma, const double* SigT,
                        const unsigned char* fixed, double dw_shift, double* Qexact, double* Q, int max_mods, int* count,
                        int* node, double* delta, double* vec, double* worst);
/* rhs [nrhs][N] (one right-hand side after the other) in, solutions out;
 * may be called repeatedly after one factor.                               */
int emi_kkt_solve(emi_ctx_t ctx, double* rhs, int nrhs);
/* The same with the right-hand sides in DEVICE memory, solved in place: no copies and no synchronisation, asynchronous on the
 * context's stream (a Woodbury correction from emi_kkt_lowrank is applied as in emi_kkt_solve).  Same statuses.               */
int emi_kkt_solve_dev(emi_ctx_t ctx, void* dRhs, int nrhs);

/* ---- the array arithmetic of an interior-point iteration, batched (f64 contexts without delays, ns+nc <= 16) ----------------
 * What ETOL::eMI355X::solve() runs on the host between two evaluations (host/emi_nlp.cpp, the ipm_* functions), over
 * [instance][node], device memory in and out.  The NLP of one instance: minimise COST s.t. defects RES[i][k] = 0, path rows
 * cl_j <= c_j <= cu_j written  c - s - e1 + e2 = 0  with a slack s in [cl, cu] and elastics e1, e2 > 0 weighted rho, and variable
 * bounds zl <= z <= zu.  All arrays node index fastest, B = the context's batch, nv = ns + nc:
 *   point        X[B][ns][M], U[B][nc][M], S, E1, E2 [B][np][M]
 *   multipliers  LamF[B][ns][M] (defects), Y[B][np][M] (rows), ZL, ZU [B][nv][M], VL, VU (slack bounds), W1, W2 (elastics) [B][np][M]
 *   step         DZLam[B][nv+ns][M] in the unknown order of emi_kkt_factor (variables, then defect multipliers): the right-hand
 *                side going into emi_kkt_solve_dev and the solution coming out; DS, DY, DE1, DE2, DVL, DVU, DW1, DW2 [B][np][M],
 *                DZL, DZU [B][nv][M]
 *   bounds       zl, zu [nsets][nv][M], nsets 1 or B (zl == zu fixes a variable, |bound| >= 1e19: absent: the certificate's
 *                convention); cl, cu, cscale: [np] HOST arrays in both forms, cscale NULL = 1.  The kernels read path values and
 *                their partials as cscale[j] RES and cscale[j] VALS and the row bounds as cscale[j] cl, cscale[j] cu; the caller
 *                forms G with LamC = cscale Y.
 *   par[B][4]    = {mu, rho, tau, nu} per instance (device)
 *   path-row partials: the (variable, VALS entry) list of emi_kkt_blocks_rows, without one the record table's default.
 * With g- = z - zl, g+ = zu - z (a term is absent with its bound), c = cscale RES[ns+j], lo = cscale cl, hi = cscale cu:
 * emi_ipm_reduce   sig_s = VL/(s-lo) + VU/(hi-s);  rhat_s = -Y - mu/(s-lo) + mu/(hi-s);  a1 = E1/W1, a2 = E2/W2;
 *                  SigT = 1/(1/sig_s + a1 + a2);   Rt = rowres + rhat_s/sig_s - a1 (Y - rho + mu/E1) - a2 (Y + rho - mu/E2)
 *                  with rowres = RowRes, or c - s - e1 + e2 when RowRes is NULL;   Sigma = ZL/g- + ZU/g+ (0 where fixed);
 *                  Rhs[v] = -(G - mu/g- + mu/g+) - sum over the partials of v: cscale VALS[e] SigT Rt (0 where fixed);
 *                  Rhs[nv+i] = -DefRes[i], or -RES[i] when DefRes is NULL.  Sigma and SigT are what emi_kkt_blocks_dev takes.
 * emi_ipm_expand   dz of fixed variables set to 0 in place;  DY = SigT (sum cscale VALS[e] dz[var] + Rt);  DS = (DY - rhat_s)/sig_s;
 *                  DE1 = a1 (DY + Y - rho + mu/E1);  DE2 = a2 (-DY - Y - rho + mu/E2);  DVL = mu/(s-lo) - VL - VL/(s-lo) DS;
 *                  DVU = mu/(hi-s) - VU + VU/(hi-s) DS;  DW1 = mu/E1 - W1 - W1/E1 DE1 (DW2 alike);  DZL = mu/g- - ZL - ZL/g- dz;
 *                  DZU = mu/g+ - ZU + ZU/g+ dz;   scal[B][4] = {apr, adu, dphi, mmax}: the fraction-to-the-boundary lengths for
 *                  tau (primal: z, s, e1, e2; dual: every bound multiplier; both <= 1), dphi = sum (costgrad - mu/g- + mu/g+) dz
 *                  + (-mu/(s-lo) + mu/(hi-s)) DS + (rho - mu/E1) DE1 + (rho - mu/E2) DE2,  mmax = max(|LamF + dlam| / rs, |Y + DY|);
 *                  rs[B][ns][M]: row weights of the merit function, NULL = 1.
 * emi_ipm_trial    trial = point + alpha[b] step  (alpha[B] device)
 * emi_ipm_merit    reset != 0 first: S[r] <- t = c - e1 + e2 where lo < t < hi and the barrier terms of t are below those of S[r]
 *                  plus nu |t - S[r]| (S in place).  out[B][2] = {phi, infeas}:  phi = COST - mu sum log(g-, g+, s-lo, hi-s, e1, e2)
 *                  + rho sum (e1 + e2),  infeas = sum |c - s - e1 + e2| + sum rs |RES[i]|.  A point outside a bound gives a
 *                  non-finite phi for THAT instance (the line search rejects it); no other instance is touched.
 * emi_ipm_accept   point <- trial;  LamF += a_pr dlam, Y += a_pr DY;  ZL, ZU, VL, VU, W1, W2 += a_du (their steps), each then
 *                  clamped to [mu / (1e10 gap), 1e10 mu / gap] with the gap at the new point.  a_pr, a_du [B] device; mask[B] bytes
 *                  (NULL: all): instances with mask 0 keep every bit.  Fixed variables keep ZL, ZU.
 * emi_ipm_error    out[B][3] = {kkt_error, viol, emax} of the barrier problem mu = par.mu:  ed = max |G - ZL + ZU|, |-Y - VL + VU|,
 *                  |rho - Y - W1|, |rho + Y - W2|;  ep = viol = max |RES[i]|, |c - s - e1 + e2|;  ec = max |gap multiplier - mu|;
 *                  sd = max(100, (sum |LamF| + sum |Y| + sumz) / (ns M + np M + cnt)) / 100,  sc = max(100, sumz / cnt) / 100 with
 *                  sumz the sum and cnt the number of positive bound multipliers (W1, W2 always counted);
 *                  kkt_error = max(ed / sd, ep, ec / sc);  emax = max(E1, E2).
 * Sums are added per thread, across the wave, across the workgroup and then over the workgroups of an instance in a fixed order:
 * two calls give the same bits.  The _dev forms are asynchronous on the context's stream; the _host forms take the same structs
 * holding HOST arrays of doubles, copy in, run the _dev form, copy out what it writes, and synchronise.
 * EMI_ERR_UNSUPPORTED: f32 context, delays set (emi_set_delays), ns+nc > 16;  EMI_ERR_ARG: a NULL argument that is not optional. */
typedef struct emi_ipm_point { void *X, *U, *S, *E1, *E2; } emi_ipm_point_t;
typedef struct emi_ipm_duals { void *LamF, *Y, *ZL, *ZU, *VL, *VU, *W1, *W2; } emi_ipm_duals_t;
typedef struct emi_ipm_step { void *DZLam, *DS, *DY, *DE1, *DE2, *DZL, *DZU, *DVL, *DVU, *DW1, *DW2; } emi_ipm_step_t;
typedef struct emi_ipm_elim { void *Sigma, *SigT, *SigS, *RhatS, *Rt; } emi_ipm_elim_t;    /* [B][nv][M], then [B][np][M] x 4 */
typedef struct emi_ipm_bounds { const void *zl, *zu; int nsets; const double *cl, *cu, *cscale; } emi_ipm_bounds_t;
int emi_ipm_reduce_dev(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dVALS,
                       const void* dG, const emi_ipm_bounds_t* bd, const void* dPar, const void* dDefRes, const void* dRowRes,
                       const emi_ipm_elim_t* out, void* dRhs);
int emi_ipm_expand_dev(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dVALS,
                       const emi_ipm_bounds_t* bd, const void* dPar, const emi_ipm_elim_t* el, const void* dRs,
                       const emi_ipm_step_t* st, void* dScal);
int emi_ipm_trial_dev(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_step_t* st, const void* dAlpha,
                      const emi_ipm_point_t* trial);
int emi_ipm_merit_dev(emi_ctx_t ctx, const emi_ipm_point_t* pt, const void* dRES, const void* dCOST, const emi_ipm_bounds_t* bd,
                      const void* dPar, const void* dRs, int reset, void* dOut);
int emi_ipm_accept_dev(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_point_t* trial, const emi_ipm_duals_t* du,
                       const emi_ipm_step_t* st, const emi_ipm_bounds_t* bd, const void* dPar, const void* dApr, const void* dAdu,
                       const void* dMask);
int emi_ipm_error_dev(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dG,
                      const emi_ipm_bounds_t* bd, const void* dPar, void* dOut);
int emi_ipm_reduce_host(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* VALS,
                        const double* G, const emi_ipm_bounds_t* bd, const double* par, const double* DefRes, const double* RowRes,
                        const emi_ipm_elim_t* out, double* Rhs);
int emi_ipm_expand_host(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* VALS,
                        const emi_ipm_bounds_t* bd, const double* par, const emi_ipm_elim_t* el, const double* rs,
                        const emi_ipm_step_t* st, double* scal);
int emi_ipm_trial_host(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_step_t* st, const double* alpha,
                       const emi_ipm_point_t* trial);
int emi_ipm_merit_host(emi_ctx_t ctx, const emi_ipm_point_t* pt, const double* RES, const double* COST, const emi_ipm_bounds_t* bd,
                       const double* par, const double* rs, int reset, double* out);
int emi_ipm_accept_host(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_point_t* trial, const emi_ipm_duals_t* du,
                        const emi_ipm_step_t* st, const emi_ipm_bounds_t* bd, const double* par, const double* a_pr,
                        const double* a_du, const unsigned char* mask);
int emi_ipm_error_host(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* G,
                       const emi_ipm_bounds_t* bd, const double* par, double* out);

/* ---- The Newton steps of a context's whole batch (a "shard"), device arrays in and out ------------------------------------
 *
 * The joint between the batched kernels above (emi_eval_dev ... emi_kkt_blocks_dev, emi_ipm_*_dev: [B][.][M] arrays of ONE
 * context) and the batched Newton-step machinery (emi_kkt_factor_batch ...: n contexts, host arrays).  The context owns one
 * Newton-step workspace per instance of its batch, created at the first call that needs it, freed with the context, told of
 * every emi_set_mesh, and apart from the workspace of emi_kkt_factor / _solve / _lowrank, whose results these calls never touch.
 * f64 contexts without delays, Schur method ("kkt_method" 1), ns + nc <= 16; otherwise EMI_ERR_UNSUPPORTED.
 * Memory: every instance holds its own Schur complement S, (ns M)^2 doubles -- 0.3 GB per instance at 1024 nodes of a 6-state
 * model, before the factor's block inverses; a failed allocation returns EMI_ERR_HIP with the message of the single call.
 *
 * Layouts are those of the neighbouring calls:
 *   dQ      [B][nhess][M]    the Q of emi_kkt_blocks_dev
 *   dVALS   [B][nvals][M]    emi_eval_dev's; the first ns (ns + nc) rows of an instance are its Jacobian node entries
 *   dFixed  [B][ns+nc][M]    bytes
 *   dRhs    [B][2 ns+nc][M]  the DZLam of emi_ipm_reduce_dev / emi_ipm_expand_dev, solved in place
 *   dCount [B], dNode / dDelta [B][max_mods], dVec [B][max_mods][ns+nc]   as emi_kkt_blocks_dev writes them
 *   mask    [B] host bytes, NULL = every instance.  An instance with mask 0 is not touched: its factors, its low-rank state and
 *           its slice of dRhs keep every bit.
 *   dc, info, exact, dc_nominal, rel, nsolve, reverted, status   [B] HOST arrays, read and written at unmasked instances only:
 *           these per-instance scalars are all that crosses.
 *
 * emi_kkt_factor_shard_dev          emi_kkt_factor_batch over the shard's workspaces: the same regularisation ladder round by round,
 *                                   the same kernels and rocBLAS calls, one synchronisation per round.  info[b] = 0 factorised,
 *                                   > 0 singular (raise dc[b], call again with a mask on those).  An instance the batch cannot take (a
 *                                   node block not positive definite, the ladder exhausted) goes through the single path and its LU
 *                                   inside the call.  The blocks reach the workspaces by one launch, not by copies per instance.
 * emi_kkt_lowrank_shard_dev         emi_kkt_lowrank per instance from the device lists (already ordered by node: no sort, no upload;
 *                                   the B counts are the one download).  count 0: exact[b] = 1, no correction.  count > max_mods or
 *                                   > 4096: exact[b] = 0, no correction (the modified step, untested).  Otherwise exact[b] = 1 and the
 *                                   Woodbury correction is active iff Delta^-1 - U^T K~^-1 U is positive definite.  max_mods == 0 reads
 *                                   no list and clears the correction of every unmasked instance (exact[b] = 1).
 * emi_kkt_solve_shard_dev           dRhs[b] <- K~_b^-1 dRhs[b] (K_b^-1 while the instance's correction is active).  Returns nothing per
 *                                   instance and does not synchronise: asynchronous on the context's stream, like emi_kkt_solve_dev.
 *                                   Instances that hold the LU go through the single solve.
 * emi_kkt_solve_refined_shard_dev   emi_kkt_solve_refined_batch, rule for rule, in place on dRhs; outputs as there.  Every unmasked
 *                                   instance must hold a factorisation of the Schur path (else EMI_ERR_UNSUPPORTED).
 * EMI_ERR_STATE: mesh, model or batch not set; solve or low-rank with an unmasked instance that holds no factorisation for the
 * context's present mesh.  EMI_ERR_ARG: NULL where not optional, negative dc.                                                     */
int emi_kkt_factor_shard_dev(emi_ctx_t ctx, const void* dQ, const void* dVALS, const void* dFixed, const double* dc,
                             const unsigned char* mask, int* info);
int emi_kkt_lowrank_shard_dev(emi_ctx_t ctx, int max_mods, const void* dCount, const void* dNode, const void* dDelta,
                              const void* dVec, const unsigned char* mask, int* exact);
int emi_kkt_solve_shard_dev(emi_ctx_t ctx, void* dRhs, const unsigned char* mask);
int emi_kkt_solve_refined_shard_dev(emi_ctx_t ctx, void* dRhs, const unsigned char* mask, const double* dc_nominal, int max_steps,
                                    double* rel, int* nsolve, int* reverted, int* status);

/* ---- Lock-step interior-point solve of a context's whole batch on ONE mesh ----------------------------------------------------
 *
 * B starting trajectories in, B solved ones out: the calls above (emi_eval_dev, emi_lagr_grad_dev, emi_hess_dev, emi_ipm_*_dev,
 * emi_kkt_blocks_dev, emi_kkt_*_shard_dev) chained inside the library, one round = one iteration of every instance that is
 * still active, with the per-instance control (convergence test, penalty escalation, barrier update, merit weight, Armijo
 * backtracking) as kernels of one thread per instance (csrc/emi_ipm_solve.hip, the rules in csrc/emi_ipm_control.hpp).  Per round
 * a few bytes per instance reach the host: who is active, the factorisation's info / exact / status, who is still searching.
 * The rules are those of ETOL::mi355x::solve_nlp (host/emi_nlp.cpp) without second-order correction, inertia search, stagnation
 * rule, variable and Jacobian-based scaling, warm-start multipliers, coupling rows and time limit.
 * Residual-based acceptance and the crawl rule are taken over behind opt.rules bit EMI_IPM_RULE_RESIDUAL: an instance whose first
 * trial point (length apr) fails the Armijo test, and whose KKT error at mu = 0 is at most 1e-2 or whose last crawl_limit accepted
 * steps were each shorter than crawl_frac apr, takes the full step (primal apr without the slack reset, multipliers with apr and
 * adu), is evaluated with derivatives, and keeps the step if the KKT error of the present barrier problem is finite and at most
 * 0.9 times what it was; otherwise its iterate is put back bit for bit and the backtracking goes on from apr / 2.  The attempt
 * is one evaluation; results[b].newton_steps / restored_steps count the steps kept / taken back.  With rules == 0 the launches and
 * every bit of every output are those of the driver without the rule, and none of the rule's arrays exists.
 *   dX[B][ns][M], dU[B][nc][M]   the start on entry (pushed into the bounds by the call), the final iterate on return
 *   dLamF[B][ns][M]              out: defect multipliers
 *   dLamC[B][np][M]              out: path-row multipliers in the caller's units (cscale Y), the Lagrangian of emi_hess_*: the
 *                                outputs go straight into emi_kkt_certificate_dev.  May be NULL without path rows.
 *   bd                           bounds as for emi_ipm_*: zl, zu [nsets][nv][M] (device in the _dev form), cl, cu, cscale host
 *   opt                          zero-initialised fields take solve_nlp's defaults: tol 1e-8, mu_init 0.1, bound_push and
 *                                bound_frac 1e-2, rho_init 10, acceptable_factor 100, max_iter 200, acceptable_iter 10,
 *                                max_futile_escalations 3; rules: bit set of EMI_IPM_RULE_* (0: none; an unknown bit is
 *                                EMI_ERR_ARG); with EMI_IPM_RULE_RESIDUAL crawl_limit <= 0 takes 3 and crawl_frac <= 0 takes 0.3 (a
 *                                crawl_limit beyond max_iter leaves the kkt_error <= 1e-2 branch only)
 *   results[B]                   host: status (EMI_IPM_*), iterations, evaluations, factorisations, steps of the convexified
 *                                matrix, and cost, KKT error at mu = 0, largest residual, largest elastic, mu, rho at the end;
 *                                full steps kept / taken back on the KKT residual (0 without EMI_IPM_RULE_RESIDUAL)
 * Path-row partials: the list of emi_kkt_blocks_rows, or the default.  An instance that has ended is masked out of every call
 * that takes a mask and keeps every bit of its iterate; the call returns when none is active.  Two identical calls give the
 * same bits.  The iterate's slacks, multipliers, step, elimination arrays, trial point, H, Q, eigenpair lists, G and the state
 * records are device arrays of the context, created at the first call, grown when mesh or batch grow, freed with the context;
 * with EMI_IPM_RULE_RESIDUAL also a kept iterate, a full-step point and a second RES / VALS / COST / G.
 * Returns EMI_OK when the run ended normally whatever the instances' statuses; EMI_ERR_UNSUPPORTED: f32 context, delays set,
 * ns + nc > 16, LU method;  EMI_ERR_STATE: mesh, model or batch not set;  EMI_ERR_ARG: a NULL argument that is not optional.
 * The _host form takes host arrays (zl, zu included), copies in, runs the _dev form, copies out and synchronises.            */
enum { EMI_IPM_CONVERGED = 0, EMI_IPM_ACCEPTABLE = 1, EMI_IPM_MAX_ITER = 2, EMI_IPM_LINE_SEARCH = 3, EMI_IPM_INFEASIBLE = 4,
       EMI_IPM_FACTOR = 5 /* still singular after the dual ladder, or the instance left the Schur path */, EMI_IPM_NOT_FINITE = 6 };
enum { EMI_IPM_RULE_RESIDUAL = 1 /* residual-based acceptance of the full step and the crawl rule */ };
typedef struct emi_ipm_options {
  double tol, mu_init, bound_push, bound_frac, rho_init, acceptable_factor;
  int max_iter, acceptable_iter, max_futile_escalations;
  int rules;
  int crawl_limit;
  double crawl_frac;
} emi_ipm_options_t;
typedef struct emi_ipm_result {
  int status, iterations, evaluations, factorisations, reflected_steps;
  double cost, kkt_error, constr_viol, emax, mu, rho;
  int newton_steps, restored_steps;
} emi_ipm_result_t;
int emi_ipm_solve_shard_dev(emi_ctx_t ctx, void* dX, void* dU, const emi_ipm_bounds_t* bd, const emi_ipm_options_t* opt,
                            void* dLamF, void* dLamC, emi_ipm_result_t* results);
int emi_ipm_solve_shard_host(emi_ctx_t ctx, double* X, double* U, const emi_ipm_bounds_t* bd, const emi_ipm_options_t* opt,
                             double* LamF, double* LamC, emi_ipm_result_t* results);
/* ---- Lock-step solve over a MESH LADDER: every instance on the same rung at the same time --------------------------------------
 *
 * B coarse starts in, B solved trajectories on the finest mesh and their multipliers out; between the rungs the trajectories are
 * interpolated by a kernel and never visit the host (csrc/emi_ipm_ladder.hip).
 *
 * emi_prolong_matrix (host, no device needed): P[Mf][Mc], row q = the Lagrange basis polynomials of the coarse LGL nodes
 * (tau_c, w_c) at tau_f[q], in the barycentric second form with the weights (-1)^j sqrt(w_j); where tau_f[q] == tau_c[j] exactly
 * the row is the unit vector e_j.  Any Mc >= 2, Mf >= 2.
 * emi_prolong_dev: Vf[r][q] = sum_j P[q][j] Vc[r][j] for R rows, from dPT[Mc][Mf] = P transposed (device).  Asynchronous on the
 * context's stream; needs no mesh, model or batch.  Fused multiply-adds in ascending j, one writer per output: a unit row of P
 * copies the coarse value (a -0 arrives as +0), a row's bits do not depend on R or on the other rows, two calls give the same
 * bits.  f64 contexts only (EMI_ERR_UNSUPPORTED).
 * emi_repair_guess_dev: ETOL::mi355x::repair_guess on dX[B][ns][M] for the context's record table (shared or per instance) on the
 * context's mesh: an interior node whose position (px, py) lies inside a keep-out (quadratic form below 1.025) is moved out
 * radially to 1.05, from a dead centre (form below 1e-12) along the minor axis; up to 50 sweeps over the table rows in row
 * order, until a sweep moves nothing.  End nodes are never touched; rows of kind EMI_PATH_TRACK take their centres from the
 * arrays of emi_set_tracks / emi_tracks_from_waypoints_dev (EMI_ERR_STATE without them); traced rows are skipped.  Single rounded operations, never fused: the
 * bits are the formulas' bits.  Asynchronous.  EMI_ERR_UNSUPPORTED: f32 context;  EMI_ERR_STATE: mesh, model or batch not set.
 *
 * emi_ipm_solve_ladder_dev: per rung r = 0 .. nrungs-1
 *   1. emi_lgl and emi_set_mesh(M_r, .., t0, tf);
 *   2. emi_set_path with the rung's recs where given (np, nsets, px, py as the context has them: a caller inflates its
 *      keep-outs per rung this way); after the call the context holds what the last rung set;
 *   2a. where the table now in force has rows of kind EMI_PATH_TRACK: emi_tracks_from_waypoints_dev (identity map), the centres of
 *      the moving discs at this rung's node times from the waypoint tables of emi_set_track_waypoints -- one launch, nothing goes
 *      up or down; after the call the context holds the centres of the last rung's mesh;
 *   3. from the second rung on, X and U prolonged from the previous rung's final iterate (emi_prolong_dev);
 *   4. emi_repair_guess_dev where the rung asks for it;
 *   5. emi_ipm_solve_shard_dev on this rung with the rung's bounds and options (its start pushes the prolonged point inside the
 *      bounds).
 * Multipliers are not carried: LamF = 0 at every start.  Every instance climbs whatever its status on a rung; results[r][b] says
 * what happened (a non-finite iterate ends EMI_IPM_NOT_FINITE on the next rung).  dX0 [B][ns][M_0] and dU0 [B][nc][M_0] are only
 * read; dX, dU, dLamF, dLamC are sized for the LAST rung.  The call is emi_ipm_solve_refine_dev's loop with a check on no rung: the
 * interpolation matrix and the iterates and multipliers of two consecutive rungs, sized for the largest, are device arrays of the
 * context (grown as needed, freed with it), every rung -- the last included -- is solved there, and one emi_shard_move_dev launch
 * after the last solve takes everybody to the caller's arrays; per rung pair Mc Mf doubles go up, nothing of a trajectory's size
 * comes down.  On return the context is on the last rung's mesh.  A ladder of one rung runs the launches of
 * emi_ipm_solve_shard_dev on a copy of the start.
 * EMI_ERR_UNSUPPORTED: whatever emi_ipm_solve_shard_dev refuses, and a record table (the context's or a rung's) with a row of
 * kind EMI_PATH_TRACK while the context holds NO waypoint tables: the centres of such rows are per mesh and without the tables
 * this call has no way to supply them (centres set with emi_set_tracks go with the first emi_set_mesh).  EMI_ERR_ARG: nrungs < 1,
 * a rung with M < 2, a NULL that is not optional, recs given while the context has no table; with track rows and waypoint
 * tables: a track row (of the context's table or of a rung's) that names a track outside 0 .. ntracks-1 of the waypoint tables,
 * and waypoint tables whose nsets is neither 1 nor B.  EMI_ERR_STATE: model or batch not set (whatever mesh the context is on
 * is replaced).  The _host form takes host arrays (every rung's zl, zu included) and
 * synchronises.                                                                                                                 */
typedef struct emi_ipm_rung {
  int M;                       /* LGL nodes of this rung */
  emi_ipm_bounds_t bd;         /* bounds at this M (zl, zu [nsets][nv][M]) */
  const double* recs;          /* host, shape of emi_set_path's table; NULL: keep the context's */
  emi_ipm_options_t opt;       /* zero fields: the defaults of emi_ipm_solve_shard_dev (warm mu_init / bound_push go here) */
  int repair;                  /* non-zero: emi_repair_guess_dev on the prolonged states before the solve */
} emi_ipm_rung_t;
int emi_prolong_matrix(int Mc, const double* tau_c, const double* w_c, int Mf, const double* tau_f, double* P);
int emi_prolong_dev(emi_ctx_t ctx, int Mc, int Mf, const void* dPT, const void* dVc, int R, void* dVf);
int emi_repair_guess_dev(emi_ctx_t ctx, void* dX);
int emi_ipm_solve_ladder_dev(emi_ctx_t ctx, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const void* dX0,
                             const void* dU0, void* dX, void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results);
int emi_ipm_solve_ladder_host(emi_ctx_t ctx, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const double* X0,
                              const double* U0, double* X, double* U, double* LamF, double* LamC, emi_ipm_result_t* results);
/* ---- Relative local ODE error of the context's batch on its collocation mesh: is the mesh fine enough? --------------------------
 *
 * The quantity PSOPT's mesh refinement compares with ode_tolerance (the reference's ePSOPT.cpp:69-71), for every instance of the
 * batch at once (csrc/emi_ode_error.hip, DESIGN.md sections 3 and 6).  Mesh tau_0 < .. < tau_{M-1}, weights w, h = (tf - t0) / 2.
 *   points          s_p, p = q (M-1) + k: the 5 Gauss-Legendre points q of the interval [tau_k, tau_k+1] (q-major: consecutive k
 *                   are consecutive in memory); a Gauss point never coincides with a node
 *   interpolation   E[p][j] = lam_j(s_p) / sum_i lam_i(s_p),  lam_j(s) = (-1)^j sqrt(w_j) / (s - tau_j)
 *   derivative      E'[p][j] = (E[p][j] sum_i lam_i / (s_p - tau_i) - lam_j / (s_p - tau_j)) / sum_i lam_i   (d/dtau of the interpolant)
 *   values          z~ = E z for all ns + nc variables of instance b; controls clipped to [ul_j, uu_j] where the caller gives
 *                   bounds;  x~' = E' x / h
 *   model           f = Model::f(params, z~, t0 + h (s_p + 1))
 *   interval error  eta[b][i][k] = (tau_k+1 - tau_k) / 2 * h * sum_q g_q |x~'_i - f_i|      (g: the Gauss weights, sum 2)
 *   state scale     W[b][i] = max_k max(|x_ik|, |(D x)_ik| / h)
 *   estimate        err[b] = max_{i,k} eta[b][i][k] / (W[b][i] + 1)
 * A trajectory that is not finite gives a non-finite err[b], for that instance only (the maxima carry a NaN; an interpolated
 * control that is not finite is not clipped).
 *
 * emi_ode_error_operator (host, no device needed): E, Ed [5 (M-1)][M] row-major and tq [5 (M-1)] = s_p in the point order above;
 * the operator is that of the rounded tq, formed in extended precision.  EMI_ERR_ARG: M < 2 or a NULL pointer.
 * emi_interp_dev: the product alone, dOut[r][c] = sum_j dV[r][j] dOP[c][j] for R rows of K values and N outputs, on the matrix
 * pipe; dOP [N][ldk] with ldk even and >= K, rows padded with zeros, on a 16-byte boundary; dOut rows ldo >= N long, columns
 * N .. ldo-1 are not written.  Needs no mesh, model or batch; R = 0 is a no-op; K >= 2, N >= 1.  One writer per output, sums
 * in ascending j: a row's bits depend on that row and dOP alone, two calls give the same bits.  Asynchronous.
 * emi_ode_error_dev: dX [B][ns][M], dU [B][nc][M] -> dErr [B] and, where dEta is not NULL, dEta [B][ns][M-1].  ul, uu: host [nc]
 * arrays (kept in a context buffer), a NULL pair means no clip.  Asynchronous on the context's stream (the first call on a mesh
 * builds the operator: 2 * 5 (M-1) M doubles go up once).  The operator, the point times and the workspace are device arrays of
 * the context (grown as needed, freed with it).  The context's mesh, tables and every other piece of state are as before the call.
 * EMI_ERR_UNSUPPORTED: f32 context; context with delays (f reads the delayed values).  EMI_ERR_STATE: points-only mesh; mesh,
 * model or batch not set.  Track and record tables play no part and are accepted as they are.  The _host form takes host arrays
 * and synchronises.                                                                                                             */
int emi_ode_error_operator(int M, const double* tau, const double* w, double* E, double* Ed, double* tq);
int emi_interp_dev(emi_ctx_t ctx, int K, int N, int ldk, const void* dOP, const void* dV, int R, int ldo, void* dOut);
int emi_ode_error_dev(emi_ctx_t ctx, const void* dX, const void* dU, const double* ul, const double* uu, void* dEta, void* dErr);
int emi_ode_error_host(emi_ctx_t ctx, const double* X, const double* U, const double* ul, const double* uu, double* Eta, double* Err);
/* ---- ... of a context WITH delays: the _total_ calls --------------------------------------------------------------------------
 *
 * Take a context with emi_set_delays(xh, uh, dt): ncf = nc - n_delayed free controls, then the delayed slots in the order of
 * emi_set_delays.  Everything of the definition above stays (the points s_p, E, E', the clip of the free controls, eta, W, err);
 * the model is evaluated on the extended node variables
 *   z~(s_p) = [ x~(s_p) | u~(s_p) clipped | delayed slots ]
 *   slot q = (source v, delay index i)  ->  z~_v at the time max(t_p - i dt, t0),  t_p = t0 + h (s_p + 1)
 * which is the clamp of emi_delay_matrix applied between the nodes.  The delayed copy of a control is the same clipped interpolant
 * at the earlier time: it is clipped with its source's bounds.  W[b][i] and err[b] are as before, from X and D x.
 *
 * emi_ode_error_delay_operator (host, no device needed): the operator of one delay, Edel [5 (M-1)][M] row-major.  Row p is the
 * Lagrange basis of the mesh at x_p, formed in double exactly as emi_delay_matrix forms it at a node: ts = t_p - delay,
 * ts = max(ts, t0), x_p = (ts - t0) / h - 1, with t_p from the rounded s_p of emi_ode_error_operator.  The row is formed in
 * extended precision, in barycentric form with the weights (-1)^j sqrt(w_j); where ts <= t0 it is e_0, where x_p == tau_j exactly
 * it is e_j.  EMI_ERR_ARG: M < 2, a NULL pointer, tf <= t0, delay < 0.
 * emi_ode_error_total_dev: dX [B][ns][M], dU [B][ncf][M] (the FREE controls) -> dErr [B] and, where dEta is not NULL, dEta
 * [B][ns][M-1].  ul, uu: host [ncf] arrays, a NULL pair means no clip.  On a context without delays this is emi_ode_error_dev: the
 * same launches, the same bits.  With delays the state rows go against the stacked operator [E | E' | D | Edel(dt) ..
 * Edel((xh-1) dt)] and the ncf control rows against [E | Edel(dt) .. Edel(uh dt)], both on emi_interp_dev's kernel; the stacks
 * are built once per (mesh, delays): max(xh - 1, uh) * 5 (M-1) * ldk doubles go up then.  Asynchronous on the context's stream;
 * operators and workspace are device arrays of the context (grown as needed, freed with it); the context's mesh, delays, tables
 * and every later pass's bits are as before the call.  EMI_ERR_UNSUPPORTED: f32 context; more than 65535 instances.
 * EMI_ERR_STATE: points-only mesh; mesh, model or batch not set.  EMI_ERR_ARG: a NULL that is not optional, half a pair of
 * bounds.  The _host form takes host arrays and synchronises.  emi_ode_error_dev / _host keep refusing a context with delays.     */
int emi_ode_error_delay_operator(int M, const double* tau, const double* w, double t0, double tf, double delay, double* Edel);
int emi_ode_error_total_dev(emi_ctx_t ctx, const void* dX, const void* dU, const double* ul, const double* uu, void* dEta, void* dErr);
int emi_ode_error_total_host(emi_ctx_t ctx, const double* X, const double* U, const double* ul, const double* uu, double* Eta, double* Err);
/* ---- Lock-step MESH REFINEMENT: the ladder, with the instances that meet the ODE tolerance retired rung by rung -----------------
 *
 * PSOPT's automatic mesh refinement (solve, estimate the ODE error, add nodes, solve again until ode_tolerance holds: the loop of
 * ETOL::eMI355X::solve, host/eMI355X.cpp) for a whole batch: B coarse starts in, every instance back on the mesh it retired on
 * (csrc/emi_ipm_ladder.hip).  An instance that is done leaves the batch: the rest are compacted into a
 * smaller batch of the same context and only those are solved on the next rung.  Nothing of a trajectory's size visits the host.
 *
 * emi_ipm_refine_decide (host, no device needed): the rule, for one instance after its solve on a rung r >= first_check.
 *   ok = status is EMI_IPM_CONVERGED or EMI_IPM_ACCEPTABLE;  met = err is finite and err <= ode_tol (a NaN or an infinite err: missed)
 *   ok and met                    retires on r,     EMI_REFINE_MET
 *   ok, missed, r the last rung   retires on r,     EMI_REFINE_NOT_MET
 *   ok, missed, not the last      climbs; its rung-r iterate and multipliers are its good solution (*verdict = EMI_REFINE_NOT_MET,
 *                                 what it would carry if the ladder ended here)
 *   not ok, has_good              retires with the good solution of rung r-1, EMI_REFINE_FELL_BACK: a refinement solve that fails
 *                                 does not take the converged coarser solution with it
 *   not ok, no good solution      retires on r with whatever the solve left, EMI_REFINE_FAILED
 * Returns 1 where the instance retires, 0 where it climbs; verdict may be NULL.
 * emi_prolong_rows_dev: emi_prolong_dev with the source row of output row r taken from a list, Vf[r] = P Vc[dRowMap[r]] (device
 * ints, any values in [0, rows of dVc): a permutation compacts, a repeated value copies).  The same fused multiply-adds in ascending
 * j: row r has the bits emi_prolong_dev gives for row dRowMap[r] alone; dRowMap NULL is the identity, the bits of emi_prolong_dev.
 * emi_shard_move_dev: the instances of a list moved between two sets of up to 4 arrays in one launch.  Array a holds rows[a] rows
 * per instance of src_ld[a] (source) / dst_ld[a] (destination) doubles; entry i of the list copies the first len values of every
 * row of instance dSrcIdx[i] of src[a] to instance dDstIdx[i] of dst[a] (device ints; a NULL list is 0, 1, .., n-1).  No
 * arithmetic: the copies are the source's bits; what the list does not name, and the columns from len on, keep every bit.  The
 * destination instances of a list must differ and no destination may overlap a source.  n = 0 is a no-op; a list beyond 65535 entries
 * goes out in more than one launch.  Both calls: asynchronous on the context's stream, no mesh, model or batch needed, f64 contexts
 * only (EMI_ERR_UNSUPPORTED); EMI_ERR_ARG: a count below 0, narrays outside 1 .. 4, rows < 0, len beyond a leading dimension, a NULL array.
 *
 * emi_ipm_solve_refine_dev: with live = every instance at the start, per rung r = 0 .. nrungs-1 while anybody is live
 *   1. emi_lgl and emi_set_mesh(M_r, .., t0, tf);
 *   2. emi_set_batch(n) for the n live instances and emi_set_path with their rows of the record table (the context's table is read
 *      back before its first compaction; a rung's recs, given for all B instances in the caller's numbering, replaces that copy);
 *   2a. where the table has rows of kind EMI_PATH_TRACK: emi_tracks_from_waypoints_dev for the live instances -- waypoint tables with
 *      one set per instance (nsets == B) are read through the live list as the set map, so the compaction of the centres happens
 *      in the launch; a shared set (nsets == 1) serves whoever is live;
 *   3. from the second rung on, X and U of the live instances prolonged from the previous rung's compact iterate: the row map of
 *      emi_prolong_rows_dev does the compaction in the same pass;
 *   4. a rung's bounds with nsets == B are given in the caller's numbering: the sets of the live instances are gathered
 *      (emi_shard_move_dev) once somebody has left;
 *   5. emi_repair_guess_dev where asked for, emi_ipm_solve_shard_dev on the compact batch;
 *   6. below rf->first_check every live instance climbs, as in the ladder call.  From first_check on: emi_ode_error_dev (clip rf->ul,
 *      rf->uu) on the compact iterate, n doubles come down, emi_ipm_refine_decide per instance, and the retirees' X, U, LamF, LamC
 *      go into the caller's arrays by emi_shard_move_dev (one launch for those that return this rung's iterate, one for those that
 *      fall back to the previous rung's); a few ints per live instance go up.
 * dX [B][ns][ldm], dU [B][nc][ldm], dLamF [B][ns][ldm], dLamC [B][np][ldm] with ldm >= the largest rung: instance b holds
 * M_{out[b].rung} values per row, the columns beyond keep the caller's bits.  results[r][b]: what emi_ipm_solve_shard_dev reported,
 * status -1 (all else zero) on a rung the instance did not solve.  err[r][b]: the estimate, NaN where none was taken.  out[b]: the
 * rung the returned trajectory is on, the verdict, the number of rungs the instance was solved on, the estimate on the returned
 * rung (NaN without one).  The starts dX0 [B][ns][M_0], dU0 [B][nc][M_0] are only read.  While nobody has retired the launches on the
 * trajectories are those of emi_ipm_solve_ladder_dev (into arrays of the context) and every bit of an iterate is that call's; an
 * instance solved in a compacted batch agrees with the same instance solved alone as two batch sizes agree in
 * emi_ipm_solve_shard_dev.  Two identical calls give the same bits.  On return, also after an error, the context has batch B again,
 * the full record table (that of the last rung which brought one) and, with track rows, the centres of all sets of the waypoint
 * tables on the mesh it is on; it is on the mesh of the last rung that was solved.  The
 * compact iterates and multipliers of two consecutive rungs, the gathered bounds and the lists are device arrays of the context.
 * Statuses: those of emi_ipm_solve_ladder_dev (track rows are taken with waypoint tables and refused without, as there), and EMI_ERR_ARG: rf NULL, ode_tol negative or NaN, first_check outside
 * 0 .. nrungs-1, one of ul / uu without the other, ldm below the largest rung, a rung whose bounds have nsets other than 1 or B, a
 * NULL err or out.  Instances are never masked instead of compacted.  The _host form takes host arrays (every rung's zl, zu included;
 * X, U, LamF, LamC go in and come out, so that the columns beyond an instance's mesh are the caller's) and synchronises.         */
enum { EMI_REFINE_MET = 0, EMI_REFINE_NOT_MET = 1, EMI_REFINE_FELL_BACK = 2, EMI_REFINE_FAILED = 3 };
typedef struct emi_ipm_refine {
  double ode_tol;          /* retire when err <= ode_tol; 0 retires nobody early, +inf everybody who solved at first_check */
  int first_check;         /* rungs below it are mesh-sequencing rungs: every live instance climbs, as in the ladder call */
  const double *ul, *uu;   /* host [nc], the clip of emi_ode_error_dev; a NULL pair: none */
} emi_ipm_refine_t;
typedef struct emi_ipm_refine_result { int rung, verdict, rungs_solved; double err; } emi_ipm_refine_result_t;
int emi_ipm_refine_decide(int status, double err, double ode_tol, int has_good, int is_last, int* verdict);
int emi_prolong_rows_dev(emi_ctx_t ctx, int Mc, int Mf, const void* dPT, const void* dVc, int R, const void* dRowMap, void* dVf);
int emi_shard_move_dev(emi_ctx_t ctx, int n, const void* dSrcIdx, const void* dDstIdx, int narrays, const int* rows,
                       const void* const* src, const int* src_ld, void* const* dst, const int* dst_ld, int len);
int emi_ipm_solve_refine_dev(emi_ctx_t ctx, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                             const void* dX0, const void* dU0, int ldm, void* dX, void* dU, void* dLamF, void* dLamC,
                             emi_ipm_result_t* results, double* err, emi_ipm_refine_result_t* out);
int emi_ipm_solve_refine_host(emi_ctx_t ctx, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                              const double* X0, const double* U0, int ldm, double* X, double* U, double* LamF, double* LamC,
                              emi_ipm_result_t* results, double* err, emi_ipm_refine_result_t* out);
/* ---- starts of a context's whole batch: the straight line, the bent line, the route planned past the static keep-outs ----------
 * What ETOL::mi355x::initial_guess does for the states of one problem, for every instance of the batch in one call, so that the
 * lock-step calls above can be given the starts solve() owes its robustness to without a Dijkstra per instance on the host and
 * without [B][ns][M] going up per attempt.  Controls are the caller's business.
 *
 * emi_plan_route (host, no device needed): the route of planned_path_guess (host/eMI355X.cpp) from (ends[0], ends[1]) to (ends[2],
 * ends[3]) past the np records recs[np][EMI_PATH_REC], on a grid of `grid` points per axis (0: 161; else 9 .. 161), resampled at
 * the M node abscissae tau (M >= 2) into xs[M], ys[M].  Cell (i, j) is the point (xl + i hx, yl + j hy) and has the number i grid + j.
 *   span = max(|x1 - x0|, |y1 - y0|); the box {xl, xu, yl, yu}: an axis of `box` that is not inside (-1e18, 1e18) (or box NULL) is
 *   [min - span, max + span] of the end points on that axis; hx = (xu - xl) / (grid - 1), hy likewise.
 *   Static records: ellipses and discs with a^2 > 0 and b^2 > 0; rows of kind EMI_PATH_TRACK are ignored.
 *   clear(cell) = min over static records of (sqrt(ex^2 / a^2 + ey^2 / b^2) - 1) sqrt(min(a^2, b^2)), (ex, ey) the cell's offset
 *   from the centre in the record's axes; cellcost = 1 + (room / max(clear, 1e-3 span))^2 with room = clearance span (1 where
 *   room is not positive); a cell is blocked at grow g in {0.25, 0.1, 0} where ex^2 / (a^2 G) + ey^2 / (b^2 G) < 1, G = (1 + g)^2,
 *   for some static record; the cells of the two end points are never blocked.
 *   *level: 0, 1, 2: the first of the three grows with a route; -1: none has one; -2: nothing to plan (no static record, a span
 *   that is not positive, or a box without extent).  xs, ys, cells are written, and *cost, *ncells are non-zero, only with a route.
 *   cells (NULL, or room for grid^2 numbers): the *ncells cells of the route from start to goal; *cost: its length, dist[goal].
 * planned_path_guess term by term, with four exceptions that make a parallel evaluation possible and reproducible:
 *   Distances are a fixed point, not Dijkstra's visiting order: dist[start] = 0, dist[c] = min over the 8 neighbours a of
 *     fl(dist[a] + w(a -> c)), w = fl(step cellcost[c]), step = hx, hy or sd = sqrt(hx hx + hy hy) (computed once).  Rounded addition
 *     is monotone and the weights are positive, so Dijkstra and a relaxation in any order from +inf reach the same bits: each value
 *     is the least left-folded cost of a path.
 *   The path is the backtrack from the goal: the predecessor of c is the first neighbour a, in the order di = -1 .. 1 outer,
 *     dj = -1 .. 1 inner, with fl(dist[a] + w(a -> c)) == dist[c].  (A backtrack of more than grid^2 cells ends with level -1.)
 *   sqrt(dx dx + dy dy) stands where the host function has hypot, floor(v + 0.5) where it has lround; single rounded operations,
 *     never fused.
 *   Distances are computed for all cells: no early exit at the goal.
 * Three in-place passes of (1/4, 1/2, 1/4) smoothing, the arc length and the resampling at 0.5 (tau_k + 1) arc are the host's;
 * the segment of a node is searched from the first one for every node (the same for ascending tau).
 * EMI_ERR_ARG: np < 0, recs NULL with np > 0, a NULL among ends, tau, xs, ys, level, a grid outside 9 .. 161 and not 0, M < 2, a NaN
 * clearance.
 *
 * emi_start_guess_dev writes dX[B][ns][M] on the context's mesh for its model, batch, record table (shared or per instance) and
 * position states px, py (emi_set_path); asynchronous on the context's stream (the end states go up from one page-locked buffer of
 * the context: a call issued while the copy of the previous one is still queued waits on the host for that copy, and no longer):
 *   1. every state i: a_i + (b_i - a_i) 0.5 (tau_k + 1) with a = xa, b = xb of the instance's set;
 *   2. EMI_START_PLANNED: rows px, py replaced by emi_plan_route's xs, ys (ends and box of the instance's set) where it has a route;
 *   3. EMI_START_BEND, and PLANNED instances without a route while bend != 0: rows px, py bent by half a sine wave,
 *      x - bend dy / len sin(pi/2 (tau_k + 1)), y + bend dx / len sin(..) with (dx, dy) the line's end-to-end vector, len its length,
 *      clipped to the box (no clip with box NULL; the sines are the host's, one table per call);
 *   4. emi_repair_guess_dev on the result where `repair` is set (track rows then need their centres, as there).
 * dLevel int[B] (NULL: not wanted): emi_plan_route's level per instance; -2 everywhere for the other kinds.  The device's bits are
 * emi_plan_route's.  The relaxation runs with one workgroup per instance over distances kept in a workspace of the context (161^2
 * doubles do not fit the LDS), grown as needed and freed with the context.
 * Statuses: EMI_ERR_UNSUPPORTED for an f32 context and for more than 65535 instances; EMI_ERR_STATE without mesh, model or batch;
 * EMI_ERR_ARG for a NULL ctx, st, dX, xa or xb, a grid outside 9 .. 161 and not 0, an nsets that is neither 1 nor B, an unknown kind,
 * a NaN in bend or clearance, px or py that is no state, a mesh of fewer than 2 nodes.  The _host form takes host arrays and synchronises. */
enum { EMI_START_LINE = 0, EMI_START_BEND = 1, EMI_START_PLANNED = 2 };
typedef struct emi_start {
  int kind;
  int nsets;            /* 1 or B: sets of xa, xb, box */
  const double* xa;     /* host [nsets][ns]: states at t0 */
  const double* xb;     /* host [nsets][ns]: states at tf */
  const double* box;    /* host [nsets][4] {xl, xu, yl, yu} of the position states px, py; NULL or a non-finite entry:
                           planned_path_guess's box of twice the span round the end points, and no clip of the bend */
  double bend;          /* BEND, and PLANNED where no route exists: sideways offset as a length (Prob::guess_bend) */
  double clearance;     /* PLANNED: Prob::guess_clearance (0: the shortest route) */
  int grid;             /* PLANNED: grid points per axis, 0 = 161; 9 .. 161 */
  int repair;           /* non-zero: emi_repair_guess_dev on the result */
} emi_start_t;
int emi_plan_route(int np, const double* recs, const double ends[4], const double box[4], double clearance, int grid, int M,
                   const double* tau, double* xs, double* ys, int* level, double* cost, int* cells, int* ncells);
int emi_start_guess_dev(emi_ctx_t ctx, const emi_start_t* st, void* dX, void* dLevel);
int emi_start_guess_host(emi_ctx_t ctx, const emi_start_t* st, double* X, int* level);
/* ---- Lock-step ladder RESTARTS: the instances an attempt did not solve are solved again from the next start ---------------------
 *
 * What ETOL::eMI355X::solve owes its robustness to (host/emi_mesh_driver.cpp: cold_start_with_retries, run_ladder,
 * restart_after_failed_target), for a whole batch: a climb that fails goes back to the coarsest mesh with the next start, and a rung
 * that fails ends the climb at once (csrc/emi_ipm_ladder.hip, csrc/emi_restart_book.hpp).
 *
 * emi_ipm_restart_decide (host, no device needed): 1 where an instance that ended an attempt with `verdict` (EMI_REFINE_*) goes to
 * the next attempt: bit `verdict` of retry_mask is set, a retry_mask of 0 standing for 1 << EMI_REFINE_FAILED; 0 for any other verdict.
 *
 * emi_ipm_solve_restart_dev: the attempts are numbered 0 .. A-1, A = (dX0 ? 1 : 0) + rs->nstarts, 1 <= A <= 8.  With dX0 given
 * attempt 0 starts from dX0 [B][ns][M_0], a user's guess; every other attempt starts from emi_start_guess_dev with the next entry
 * of rs->starts on rung 0's mesh (whose `repair` applies as there; the rung's `repair` flag applies as in the ladder call).  The
 * controls start from dU0 [B][nc][M_0] in every attempt; dX0 and dU0 are only read.
 *   Attempt 0 runs the rung loop of emi_ipm_solve_refine_dev (rf NULL: of emi_ipm_solve_ladder_dev) on all B instances.  After an
 *   attempt every instance whose verdict emi_ipm_restart_decide sends on is pending; with rf NULL the verdict is EMI_REFINE_MET where
 *   the solve on the rung the instance ended on is converged or acceptable, else EMI_REFINE_FAILED.  The next attempt runs the same
 *   loop on the pending instances only, a compact batch of the same context from rung 0 on: their rows of the record table go in
 *   through emi_set_path, their waypoint sets through the set map of emi_tracks_from_waypoints_dev, their bounds sets (nsets == B)
 *   and their rows of dU0 are gathered by emi_shard_move_dev, their xa, xb and box sets (a start with nsets == B, given in the
 *   CALLER's numbering) on the host; emi_start_guess_dev then writes the compact batch's states.  A record table that a rung brought
 *   is replaced by the one the context came with before rung 0 is solved again.
 *   The first attempt that gives an instance a verdict outside retry_mask writes its X, U, LamF, LamC into the caller's arrays
 *   [B][rows][ldm], on the mesh it retired on, as the refine call does; nothing later touches that instance.  An instance that is
 *   still pending after the last attempt keeps what attempt 0 left: out[b].attempt = 0, out[b].attempts = A.
 *   EMI_RESTART_DROP_FAILED: an instance whose solve on a rung is neither converged nor acceptable, and that has no good solution from
 *   an earlier rung of this attempt (emi_ipm_refine_decide's has_good), leaves the attempt on that rung with EMI_REFINE_FAILED -- also
 *   below rf->first_check and with rf NULL, where without the flag everybody climbs.  That is how the host driver's climb ends at a
 *   failed rung, and what makes a restart cheap: the failure is known after a cold start on the coarsest mesh.  Without the flag the
 *   rung loop's rules are exactly those of the ladder and refine calls.
 *   rs->patience[a] (NULL, or A entries; 0: the rung's own) replaces rungs[0].opt.max_iter in attempt a only: an early start does not
 *   get the full budget while other starts are unused (the host driver's warm_patience / target_patience).
 * results [A][nrungs][B], err [A][nrungs][B]: per attempt as in the refine call, status -1 and NaN where the instance was not
 * solved (with rf NULL no estimate is taken).  out[b]: the attempt whose trajectory the caller's arrays hold, the number of attempts
 * the instance was solved in, emi_plan_route's level in that attempt (-2 for the other kinds and for dX0), and the refine call's
 * out[b] of that attempt.  Nothing of a trajectory's size crosses to the host: per attempt a few ints per instance go up, statuses,
 * levels and estimates come down.  An attempt on all B instances runs the launches of the refine / ladder call, and every bit is that
 * call's; an instance solved in a compacted batch agrees with the same instance in a whole batch as two batch sizes agree in
 * emi_ipm_solve_shard_dev, so the number of instances a restart run solves is a count, not a guarantee.  Two identical calls give
 * the same bits.  On return, also after an error, the context is as the refine call leaves it: batch B, the full record table, the
 * centres of all sets, on the mesh of the last rung that was solved.  The workspaces are those of the ladder call (device arrays of
 * the context, grown as needed, freed with it).
 * Statuses: whatever emi_ipm_solve_refine_dev (rf NULL: emi_ipm_solve_ladder_dev; ldm and the bounds' nsets are checked as in the
 * refine call) and emi_start_guess_dev return, and EMI_ERR_ARG: rs NULL, A outside 1 .. 8, nstarts < 0, starts NULL with nstarts > 0,
 * a start whose nsets is neither 1 nor B, a negative patience entry, a retry_mask with bits beyond the four verdicts, an unknown
 * flag, a NULL err or out.  The _host form takes host arrays as emi_ipm_solve_refine_host does (X0 may be NULL) and synchronises. */
enum { EMI_RESTART_DROP_FAILED = 1 };
typedef struct emi_ipm_restart {
  int nstarts;                 /* entries of starts */
  const emi_start_t* starts;   /* [nstarts]; nsets 1 or B, sets in the CALLER's numbering */
  const int* patience;         /* NULL, or [attempts]: max_iter of rung 0 in that attempt (0: the rung's own) */
  int retry_mask;              /* bit v set: verdict v (EMI_REFINE_*) sends the instance to the next attempt; 0 takes 1 << EMI_REFINE_FAILED */
  int flags;                   /* EMI_RESTART_* */
} emi_ipm_restart_t;
typedef struct emi_ipm_restart_result {
  int attempt;                 /* the attempt whose trajectory the caller's arrays hold */
  int attempts;                /* attempts this instance was solved in */
  int level;                   /* emi_plan_route's level in that attempt (-2 for the other kinds and for dX0) */
  emi_ipm_refine_result_t refine;   /* rung, verdict, rungs_solved, err of that attempt */
} emi_ipm_restart_result_t;
int emi_ipm_restart_decide(int verdict, int retry_mask);
int emi_ipm_solve_restart_dev(emi_ctx_t ctx, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                              const emi_ipm_restart_t* rs, const void* dX0, const void* dU0, int ldm, void* dX, void* dU, void* dLamF,
                              void* dLamC, emi_ipm_result_t* results, double* err, emi_ipm_restart_result_t* out);
int emi_ipm_solve_restart_host(emi_ctx_t ctx, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const emi_ipm_refine_t* rf,
                               const emi_ipm_restart_t* rs, const double* X0, const double* U0, int ldm, double* X, double* U,
                               double* LamF, double* LamC, emi_ipm_result_t* results, double* err, emi_ipm_restart_result_t* out);
/* The components of emi_ipm_error's scaled KKT error, out[B][8] = {ed, sd, ep, sc, pmin, pmax, emax, ymax}: ed, ep, sd, sc and emax
 * as there; pmin / pmax the smallest and largest complementarity product (gap times multiplier); ymax = max |Y|.  For ANY
 * barrier parameter mu_t:  kkt_error(mu_t) = max(ed / sd, ep, max(0, pmax - mu_t, mu_t - pmin) / sc)  -- one launch serves the
 * test at mu = 0 and every firing of the barrier update.  par is read for rho only.  Same reduction order, same statuses.     */
/* The array part of solve_nlp's start(), as the lock-step solve runs it (device arrays; asynchronous on the context's stream):
 *   phase 0  X, U pushed inside their bounds by bound_push max(1, |bound|), at most bound_frac of the interval (a fixed variable is
 *            set to its bound); dFixed[B][nv][M] bytes = 1 where fixed; LamF = 0.          Reads pt (X, U), du (LamF), bd.
 *   phase 1  after the first evaluation: S = cscale RES[ns+j] pushed inside its row bounds, gap = c - S, E1 = max(gap, 0) + e,
 *            E2 = max(-gap, 0) + e with e = bound_push max(1, |gap|); Y = 0; ZL, ZU, VL, VU = 1 where the bound exists (0 at
 *            fixed variables); W1 = W2 = max(1e-8, rho).                                   Reads dRES, bd, dPar.
 *   phase 2  W1 = max(1e-8, rho - Y), W2 = max(1e-8, rho + Y) at the instances of dMask (bytes, NULL: all): the reset of the
 *            elastic multipliers after a penalty escalation.
 * Exact operations or single rounded ones, never fused: the arrays are the formulas' bits.  Statuses as the emi_ipm_* calls.  */
int emi_ipm_start_dev(emi_ctx_t ctx, int phase, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES,
                      const emi_ipm_bounds_t* bd, const void* dPar, double bound_push, double bound_frac, void* dFixed,
                      const void* dMask);
int emi_ipm_error_parts_dev(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const void* dRES, const void* dG,
                            const emi_ipm_bounds_t* bd, const void* dPar, void* dOut);
int emi_ipm_error_parts_host(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const double* RES, const double* G,
                             const emi_ipm_bounds_t* bd, const double* par, double* out);
/* The iterate of the instances of a mask copied between the live arrays (pt, du) and a kept set of the same shapes (kept_pt,
 * kept_du): restore == 0 live -> kept, otherwise kept -> live.  The iterate is X, U, S, E1, E2, LamF, Y, ZL, ZU, VL, VU, W1, W2;
 * dMask [B] bytes (device; NULL: every instance); an instance with mask 0 keeps every bit on both sides.  One launch, no
 * arithmetic: the copies are the source's bits.  The row arrays may be NULL without path rows.  Asynchronous on the context's
 * stream; the _host form takes host arrays (the mask included) and synchronises.  Statuses as the emi_ipm_* calls.            */
int emi_ipm_keep_dev(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const emi_ipm_point_t* kept_pt,
                     const emi_ipm_duals_t* kept_du, const void* dMask, int restore);
int emi_ipm_keep_host(emi_ctx_t ctx, const emi_ipm_point_t* pt, const emi_ipm_duals_t* du, const emi_ipm_point_t* kept_pt,
                      const emi_ipm_duals_t* kept_du, const unsigned char* mask, int restore);

/* What emi_eval_dev's default dispatch would do with a batch of B instances on this
 * context (mesh, model, options as set): the one definition of the launch policy,
 * for reports, tools and tests (csrc/emi_pass_plan.hpp: plan_pass, plan_piece; the
 * form fields are those of the kernel that is launched).                            */
typedef struct emi_pass_plan {
  int one_launch;      /* 1: the pass goes out as ONE launch (emi_pass_f64_kernel: MFMA-role + node-role workgroups) */
  int sw;              /* states per MFMA workgroup */
  int ksplit;          /* K slices per tile (> 1: combined in-kernel by ticket, in slice order) */
  int ring_stages;     /* operand ring stages of the MFMA role */
  int cpart, cx;       /* tile order: 0 plain, > 0 column partitions, < 0 grouped (-G instance groups per super-block); column tiles per block */
  int mfma_workgroups; /* workgroups of the MFMA role (tiles x K slices) */
  int store_mode;      /* node-role result stores: 0 plain, 1 sc1, 2 non-temporal, 3 nt sc1 */
  int block_order;     /* 1 MFMA workgroups first, 0 evenly interleaved, >= 100: MFMA workgroups at that % of the even density */
  int tiles16;         /* 16-instance x 128-node tiles of the (first) launch */
  int piece, tail;     /* > 0: the batch goes out in launches of `piece` instances and a last one of `tail` (0: none) */
  int k_tile;          /* depth of a K tile of the MFMA role: 8 or 16 */
  int column_tiles;    /* 64-column sub-tiles per MFMA workgroup: 1 or 2 */
  int k_halves;        /* 2: the K range of a tile in two halves inside a 512-thread workgroup */
} emi_pass_plan_t;
int emi_plan_pass(emi_ctx_t ctx, int B, emi_pass_plan_t* out);
/* ... and what the report has no field for: the resident workgroups per CU the (first) launch of that plan states ("sym_res": 2,
 * or 3, which only the forms that take De / Do straight from L2 are granted); *res = 0 where the pass does not go out as one launch. */
int emi_plan_pass_residency(emi_ctx_t ctx, int B, int* res);

/* COO pattern of VALS in per-instance NLP numbering:
 * rows/cols have nvals*M entries ordered like VALS; cost-gradient entries
 * carry row = -1.                                                          */
int emi_jac_structure(emi_ctx_t ctx, int* rows, int* cols);
/* No device and no context needed: which rows of VALS do not depend on (X, U) for a built-in model with np table rows
 * -- entries of the dynamics block and of the cost gradient that are 0, -h, D_kk or a quotient of parameters times h
 * (Quadrotor2D: 50 of its 56 + 2 np rows).  mask[r] = 1 for such a row, 0 otherwise (mask may be NULL); *nvals = the
 * number of rows.  These are the rows a pass with EMI_EVAL_KEEP_INVARIANT does not store.  EMI_ERR_ARG: not a built-in model. */
int emi_invariant_rows(int model, int np, unsigned char* mask, int* nvals);

/* ---- device memory helpers (for callers without their own allocator) ---- */
int emi_dev_alloc(emi_ctx_t ctx, size_t bytes, void** dptr);
int emi_dev_free(emi_ctx_t ctx, void* dptr);
int emi_h2d(emi_ctx_t ctx, void* dst, const void* src, size_t bytes);
int emi_d2h(emi_ctx_t ctx, void* dst, const void* src, size_t bytes);

/* ---- the hot path -------------------------------------------------------- */
/* Device-pointer form: every pointer is device memory of the layout above,
 * in the context's real type.  Asynchronous on the context's stream.
 *
 * EMI_EVAL_KEEP_INVARIANT (with a pass that writes the Jacobian): the caller asserts that dVALS is the buffer THIS context
 * last filled with a full Jacobian pass and that nobody else has written its invariant rows (emi_invariant_rows) since.
 * The pass then does not store those rows again -- they depend on the mesh, the model parameters and the cost sign only
 * (400 of the 976 bytes a quadrotor node-eval writes) -- and every other output is bit for bit what a full pass gives.
 * The context keeps its own record (buffer address, whole batch written, a generation bumped by emi_set_mesh, emi_set_model,
 * emi_set_model_source, emi_set_batch, emi_set_path, emi_set_tracks, emi_set_delays) and honours the flag only where address
 * and generation match; otherwise, and for run-time compiled models and launch forms without such a kernel, the pass
 * writes everything, which renews the record.  EMI_EVAL_NOJAC passes leave the record alone.  What the record cannot see
 * is the caller's side of the assertion: a buffer freed and allocated again at the same address, or overwritten by other
 * code, must not be passed with the flag.                                                                            */
int emi_eval_dev(emi_ctx_t ctx, const void* dX, const void* dU, void* dRES,
                 void* dVALS, void* dCOST, unsigned flags);
/* Host-buffer form (double in/out whatever the arithmetic type): copies in,
 * evaluates, copies out, synchronises.  Output pointers may be NULL.  (VALS is staged in a buffer of the context's own,
 * so this form keeps the invariant rows by itself from its second Jacobian pass on.)                                  */
int emi_eval_host(emi_ctx_t ctx, const double* X, const double* U, double* RES,
                  double* VALS, double* COST, unsigned flags);

/* Lagrangian Hessian node blocks: H[B][nhess][M], lower triangle row-major
 * of  sigma*sgn*h*w_k*L_zz - h*sum_i lamF_i,k f_i,zz + sum_j lamC_j,k c_j,zz */
int emi_hess_dev(emi_ctx_t ctx, const void* dX, const void* dU,
                 const void* dLamF, const void* dLamC, double sigma, void* dH);
int emi_hess_host(emi_ctx_t ctx, const double* X, const double* U,
                  const double* LamF, const double* LamC, double sigma,
                  double* H);

/* ---- the adjoint pass: Lagrangian gradient and KKT certificate (f64 contexts; with delays: the _total_ forms below) ----
 * The NLP of one instance: minimise COST subject to defect rows RES[i][k] = 0, path rows cl_j <= RES[ns+j][k] <= cu_j and
 * variable bounds zl[v][k] <= z[v][k] <= zu[v][k] (zl == zu fixes a variable; |bound| >= 1e19: absent).  Lagrangian
 * L = sigma COST + sum lamF.defect + sum lamC.c -- the one whose Hessian blocks emi_hess_* returns: lamC >= 0 goes with an
 * active upper bound, lamC <= 0 with an active lower one.
 *   G[B][ns+nc][M]:  G[v][k] = sigma VALS[costgrad v][k] + sum_i VALS[i*nv+v][k] lamF[i][k]
 *                            + (v < ns: sum_{j != k} D[j][k] lamF[v][j])  + sum over path rows and their partials VALS[.][k] lamC[r][k]
 *                    (partials indexed as emi_jac_structure does).  LamC may be NULL when np == 0.
 *   cert[B][6] = {stat, comp, defect, viol, gmax, lmax}, each a maximum over the instance; with G+ = max(G,0), G- = max(-G,0),
 *   lamC+ / lamC- likewise:
 *     stat    G+ where the variable has no lower bound, G- where it has no upper bound; fixed variables: 0
 *     comp    G+ max(z-zl,0), G- max(zu-z,0) on bounded sides (not for fixed variables); lamC+ max(cu-c,0), lamC- max(c-cl,0)
 *             on path rows; lamC+ / lamC- itself on a side without a bound
 *     defect  |RES| over the ns defect rows;   viol  max(zl-z, z-zu, cl-c, c-cu, 0)
 *     gmax    max |sigma costgrad|;  lmax  max(|lamF|, |lamC|)   (for relative figures)
 *   A maximum has no summation order and G is summed in a fixed order: both are bit-reproducible call to call.
 * zl, zu: [nsets][ns+nc][M], nsets 1 or B;  cl, cu: [np] HOST arrays in both forms.  The _dev forms are asynchronous on the
 * context's stream (device pointers; dG may be NULL: the gradient then stays in the context's workspace).  The _host form of
 * the certificate evaluates (EMI_EVAL_ALL) at (X, U) and then certifies; G may be NULL.
 * EMI_ERR_UNSUPPORTED: f32 context, or delays set (emi_set_delays: the _total_ forms below take those);  EMI_ERR_STATE: points-only mesh;  a NULL context on a
 * machine without a device: EMI_ERR_NO_DEVICE.                                                                              */
int emi_lagr_grad_dev(emi_ctx_t ctx, const void* dVALS, const void* dLamF, const void* dLamC, double sigma, void* dG);
int emi_lagr_grad_host(emi_ctx_t ctx, const double* VALS, const double* LamF, const double* LamC, double sigma, double* G);
int emi_kkt_certificate_dev(emi_ctx_t ctx, const void* dX, const void* dU, const void* dRES, const void* dVALS,
                            const void* dLamF, const void* dLamC, double sigma, const void* dZl, const void* dZu, int nsets,
                            const double* cl, const double* cu, void* dCert, void* dG);
int emi_kkt_certificate_host(emi_ctx_t ctx, const double* X, const double* U, const double* LamF, const double* LamC,
                             double sigma, const double* zl, const double* zu, int nsets, const double* cl, const double* cu,
                             double* cert, double* G);
/* The same for the TRAJECTORY of a context with delays (emi_set_delays).  ncf = nc - n_delayed free controls; the node variables
 * of the model are [x | u | delayed slots q = 0 .. n_delayed-1], slot q the copy of source variable src(q) (a state or a free
 * control) at delay index i(q), in the order of emi_set_delays.  With Gx[B][ns+nc][M] the formula above on those extended
 * variables (the D term on the state rows):
 *   Gdel[B][n_delayed][M]:  Gdel[q][k] = Gx[ns+ncf+q][k]      the adjoint of the delayed value: d Lagrangian / d (delayed input)
 *   G[B][ns+ncf][M]:        G[v][k] = Gx[v][k] + sum_{q: src(q) = v} sum_j Gdel[q][j] W(i(q) dt)[j][k]
 * -- a row vector times W: j runs over the ROWS of emi_delay_matrix's W.  Per class of sources (states, controls) one product on
 * the matrix pipe, K = the node ranges of the delay indices one after the other, last addition Gx[v] + product; one writer per
 * entry, fixed order, no atomics: bit-reproducible.  Gdel may be NULL.  A solver that carries the delayed values as variables
 * z_q tied to their sources by rows z_q - W z_src(q) = 0 with multipliers lamL (L = .. + sum lamL (z_q - W z_src)) has
 * Gdel = -lamL at a KKT point.
 * The certificate takes U, zl, zu and G on the FREE variables ([.][ns+ncf][M]; delayed values carry no bounds of their own) and
 * certifies the folded G; gmax runs over all ns+nc cost-gradient entries of VALS (a scale figure).  The _host form evaluates
 * first, so it forms the delayed values on the device.  An adjoint call may be the first use of a mesh: it builds W itself.
 * On a context WITHOUT delays these calls are the ones above, bit for bit (Gdel is not touched).  Statuses as above, except
 * that delays are supported.                                                                                                   */
int emi_lagr_grad_total_dev(emi_ctx_t ctx, const void* dVALS, const void* dLamF, const void* dLamC, double sigma, void* dG,
                            void* dGdel);
int emi_lagr_grad_total_host(emi_ctx_t ctx, const double* VALS, const double* LamF, const double* LamC, double sigma, double* G,
                             double* Gdel);
int emi_kkt_certificate_total_dev(emi_ctx_t ctx, const void* dX, const void* dU, const void* dRES, const void* dVALS,
                                  const void* dLamF, const void* dLamC, double sigma, const void* dZl, const void* dZu, int nsets,
                                  const double* cl, const double* cu, void* dCert, void* dG, void* dGdel);
int emi_kkt_certificate_total_host(emi_ctx_t ctx, const double* X, const double* U, const double* LamF, const double* LamC,
                                   double sigma, const double* zl, const double* zu, int nsets, const double* cl, const double* cu,
                                   double* cert, double* G, double* Gdel);

/* ---- measurement --------------------------------------------------------- */
/* HIP-event timers on the context's stream.                                 */
int emi_timer_start(emi_ctx_t ctx);
int emi_timer_stop(emi_ctx_t ctx, float* elapsed_ms); /* synchronises */
/* Per-kernel event brackets inside emi_eval_dev, recorded on the stream the
 * kernel is launched on.  level 1: every bracket (both kernels and the whole
 * overlapped pass: eight events per pass, ~25 us of dependency latency on a
 * 0.25 ms pass -- for diagnosis); 2: the defect (MFMA) kernel only; 3: the
 * node kernel only (two events per pass); 0: off.                            */
int emi_profile_enable(emi_ctx_t ctx, int level);
int emi_profile_read(emi_ctx_t ctx, float* node_ms, int* node_launches,
                     float* defect_ms, int* defect_launches,
                     float* fused_ms, int* fused_launches); /* syncs+resets */

/* ---- kernel selection ------------------------------------------------------ */
/* "overlap" (default 1): emi_eval with EMI_EVAL_ALL runs the even/odd MFMA defect
 * kernel (emi_symdefect.hip) and the streaming node kernel CONCURRENTLY on two
 * streams when the mesh allows it (f64, M % 128 == 0, centro-antisymmetric D,
 * 2- or 6-state model); 0 forces the general node-then-defect sequence.
 * "sym_ct": MFMA kernel variant.  0 (default) = chosen from the batch size;
 * 3 = LDS-DMA operand ring, one workgroup per CU; 5 / 6 / 7 / 8 = the ring with
 * SW = NS / 2 / 1 / 3 states per workgroup, 8-deep K tiles, several workgroups per
 * CU; 4 = as 0; 1 / 2 = register-staged, 64 / 128 columns (2 needs M % 256 == 0).
 * "node_store": cache policy of the node kernel's result stores on the overlapped
 * path: -1 (default) non-temporal once a pass writes more than the Infinity Cache
 * holds, 0 plain, 1 write-through, 2 non-temporal.
 * "sym_order" (default 1): workgroup -> tile order within an XCD (sym_ct 1..3).
 * "overlap_mode": how the two kernels share the chip.  0 (default) = by batch size;
 * 2 = two streams (fork / join through events); 3 = ONE launch, MFMA-role and
 * node-role workgroups in one grid with COST finished in-kernel (what 0 chooses at
 * every batch size, one instance included, where the model has a pass instantiation);
 * 1 = one stream, back to back.
 * "sym_ksplit": K slices per tile of the state-split ring: 0 (default) = chosen by the
 * default dispatch for small batches (4 slices while the MFMA role stays within 256
 * workgroups, 2 within 512: up to 16 / 80 instances at 1024 nodes), 1 = never,
 * 2 / 4 / 8 forced; partial sums through a slab, summed in slice order (bitwise
 * reproducible, not bitwise the unsplit sum).
 * "small_rows" (default 24): up to this many rows B*ns the skinny streaming defect
 * kernel takes a pass that cannot go as one launch (0: never).  "sym_combine": 1
 * (default) the workgroup that draws a tile's last ticket adds the slices
 * in-kernel, 0 a second launch does; bitwise the same result.
 * "sym_cpart": tile order of the state-split ring.  0 (default) = by mesh and batch
 * size; -1 = plain (the column tiles of an X tile are neighbours, X tiles dealt over
 * the XCDs); 1 / 2 / 4 / 8 = the column tiles cut into that many partitions, each
 * worked on by 8 / cpart XCDs, so that an XCD's share of De / Do stays in its L2.
 * "sym_gblk" / "sym_cx": the GROUPED tile order (csrc/emi_pass_work.hpp ring_tile_of): an XCD keeps a contiguous range of instance
 * groups -- the range whose node-role workgroups it also runs -- and walks it in super-blocks of sym_gblk 16-instance groups,
 * the column tiles in blocks of sym_cx (0: 2); X and U of a super-block then reach that XCD's L2 once for every consumer.
 * sym_gblk 0: off (unless the policy chooses it: inputs that do not stay in the Infinity Cache between passes).
 * "sym_nst": ring stages of the one-launch pass (3 default, 4).  "pass_order": the MFMA workgroups of an
 * XCD first in its share of the one-launch grid (1), interleaved with the node workgroups (0), interleaved
 * at value / 100 times the even MFMA density with the node workgroups at the tail (>= 100), or -1 (default)
 * by batch size: first for small batches (fewer than 128 tiles).
 * "kkt_*": process-wide switches of emi_kkt_factor ("kkt_block_trsv" 1 (default): single right-hand sides through the
 * library's block-inverse triangular solves instead of rocBLAS trsv; "kkt_primal_levels" 1 (default): primal regularisation levels behind the
 * dual ones before the LU fallback; "kkt_sticky_reg" 1 (default):
 * the Schur path starts at the dual regularisation level that worked last on this
 * mesh; "kkt_cholesky" 2 (default): the library's blocked Cholesky in two-level form from 1024 rows
 * (outer panels of "kkt_chol_outer" columns, default 768), 1: one level (any other value: EMI_ERR_ARG);
 * "kkt_chol_diag" 2 (default): the 64 x 64 diagonal block of a Cholesky step by one wave with matrix-pipe block updates, 1: column by column by 256 threads;
 * "kkt_chol_panel" 2 (default): the panel solve of a Cholesky step as 16 x 16 block products on the matrix pipe, 1: one row per thread, 0: rocblas_dtrsm;
 * "kkt_debug", "kkt_batched_max_nodes": diagnostics, see csrc/emi_kkt.hip).
 * "slice": > 0: batches above 2 * slice instances are evaluated in pieces of `slice` instances; 0 (default): a batch above
 * 2048 instances goes as one launch over its multiple of 256 instances plus one for the remainder.
 * "adj_fold_tile": tile shape of the fold product of emi_lagr_grad_total_*: 0 (default) by the number of workgroups the rows give
 * (as the operator term: 96 x 128 where that gives every CU a workgroup, else 48 x 64), 1 = 48 x 64, 2 = 96 x 128; the
 * summation order of an entry is the same either way.
 * "sym_ablate": diagnostics only, results invalid.                             */
int emi_set_option(emi_ctx_t ctx, const char* name, int value);
/* 1 if emi_eval(EMI_EVAL_ALL) currently takes the overlapped path             */
int emi_last_path(emi_ctx_t ctx, int* fused);
/* Diagnostics, no device needed: the tile order the state-split MFMA defect kernel would use for (ns states, B instances,
 * M nodes) with sym_ct (0 / 5..8) and sym_cpart as emi_set_option takes them.  out_tile[t] = column_tile + ncoltiles * group
 * for every tile slot t of the launch (out_cap entries at most); *ntiles_total = number of slots, *cpart / *cx = the plan.
 * Every value 0 .. ntiles_total-1 must occur exactly once (tests/test_abi.py).                                               */
int emi_debug_tile_order(int ns, int B, int M, int sym_ct, int sym_cpart, int* out_tile, int out_cap, int* ntiles_total,
                         int* cpart, int* cx);
/* ... the same with the grouped order's options "sym_gblk" / "sym_cx" (*cpart comes back negative, -gblk, when the plan takes it) */
int emi_debug_tile_order2(int ns, int B, int M, int sym_ct, int sym_cpart, int sym_gblk, int sym_cx, int* out_tile, int out_cap,
                          int* ntiles_total, int* cpart, int* cx);
/* Diagnostics, no device needed: De / Do of the M x M differentiation matrix D (exactly centro-antisymmetric, M a multiple of 128) in the
 * order the MFMA role of the one-launch pass loads them straight into registers (the "sym_dop" 2 form; a context builds the same copy
 * at emi_set_mesh).  out holds 2 (M/2)^2 doubles: pair (((ct*4 + w)*nkt + kt)*4 + q)*64 + lane, nkt = M/32, q = 2h + odd, lane = 16 kq + r16,
 * is {P[64 ct + 16 w + r16][16 kt + 8 h + 2 kq], its right neighbour}, P = De (odd = 0) or Do (odd = 1).                           */
int emi_debug_operator_fragments(int M, const double* D, double* out);
/* Diagnostics, no device needed: how the one-launch pass deals an XCD's nm MFMA-role and nn node-role blocks ("pass_order":
 * 0 evenly interleaved, 1 MFMA blocks first, >= 100 interleaved at order / 100 times the even MFMA density).  out_role[j] =
 * MFMA block index (>= 0) or -1 - node block index; every index of either role must occur exactly once.                      */
int emi_debug_pass_roles(int nm, int nn, int order, int* out_role, int out_cap);
/* Diagnostics, no device needed: the WORK TABLE of a launch of the one-launch pass (csrc/emi_pass_work.hpp): what every block of its
 * grid does, as the host builds it from the two maps above and as emi_pass_f64_kernel reads it.  The launch: B instances of ns states on
 * M nodes, sw states and ctc 64-column sub-tiles per MFMA workgroup, ksplit K slices per tile (made legal as a launch does), hs K
 * halves (1 or 2: a node workgroup then takes two chunks), the tile order by "sym_cpart" / "sym_gblk" / "sym_cx", the block order
 * "pass_order".  info[12] = {blocks of the grid, nm, nn, nm8, nn8, nbx, ntiles, ngrp, cpart, cx, K slices, state groups}; out (may be
 * NULL) takes five ints per block g while out_cap has room: role (0 idle, 1 MFMA, 2 node); MFMA: column tile, group, K slice, 0;
 * node: chunk and instance of the first 256 threads, then of the second 256 (-1, -1: none).  EMI_ERR_UNSUPPORTED where
 * plan_symdefect admits no such launch or it does not fit the fields of an entry.                                              */
int emi_debug_pass_work(int ns, int B, int M, int sw, int ctc, int ksplit, int hs, int sym_cpart, int sym_gblk, int sym_cx, int order,
                        int* out, int out_cap, int* info);
/* ... and of a context: work tables it has built and uploaded so far (a call whose launch was seen before uploads nothing) and,
 * where tables is not NULL, how many it holds now.                                                                             */
int emi_debug_pass_work_uploads(emi_ctx_t ctx, unsigned long long* uploads, int* tables);
/* name of the kernel that produced the defect rows in this context's last
 * emi_eval_dev (what a rocprofv3 kernel trace will show); "" before the first  */
const char* emi_last_defect_kernel(emi_ctx_t ctx);

/* ---- the one collective: gather of a batch's results over RCCL ---------------- */
/* SURVEY.md section 8e / north_star: instances shard over the GPUs of a node with no
 * communication while they are evaluated or solved; afterwards every rank hands its
 * block to the root: one group of point-to-point ncclSend/ncclRecv over xGMI.
 * (The reference has no distributed code; this replaces nothing, it is what lets a
 * caller of ETOL::eMI355X run a Monte-Carlo batch on 8 GPUs and end up with every
 * trajectory in one place.)  A communicator is its own handle, one per process/GPU.
 * The 128-byte id is made on one rank (emi_comm_unique_id) and carried to the others
 * by the launcher's means (a file, an environment variable, torch.distributed).     */
#define EMI_COMM_ID_BYTES 128
typedef struct emi_comm_s* emi_comm_t;
int emi_comm_unique_id(void* id /* EMI_COMM_ID_BYTES, out */);
int emi_comm_create(int device_id, int world, int rank, const void* id, emi_comm_t* out); /* collective */
/* every rank sends `bytes` bytes of device memory; on the root, drecv[world][bytes]
 * (device memory) receives them in rank order (the root's own block is copied).
 * hip_stream NULL: the communicator's own stream, synchronised before returning;
 * otherwise asynchronous on that stream.                                            */
int emi_comm_gather(emi_comm_t comm, const void* dsend, void* drecv, size_t bytes, int root, void* hip_stream);
int emi_comm_destroy(emi_comm_t comm);
const char* emi_comm_last_error(emi_comm_t comm); /* NULL: error of the last handle-less call of this thread */

#ifdef __cplusplus
}
#endif
#endif /* EMI355X_H_ */
