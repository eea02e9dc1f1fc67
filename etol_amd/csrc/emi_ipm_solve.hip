// emi_ipm_solve.hip -- lock-step interior-point solve of a context's whole batch on one mesh (emi_ipm_solve_shard_*): the driver
// and its per-instance control kernels.
//
// One ROUND is one iteration of every instance that is still active, on the context's stream, as batched calls over the
// [B][.][M] arrays (include/emi355x.h); the rules are those of solve_nlp's phases (host/emi_nlp.cpp), the scalar ones written
// once in emi_ipm_control.hpp:
//
//   1. evaluate and test   emi_eval_dev, LamC = cscale Y, emi_lagr_grad_dev, error components (emi_ipm_error_parts_kernel),
//                          emi_ipm_barrier_kernel: convergence, acceptable level, penalty escalation, iteration limit, barrier
//                          update.  3 B bytes come down (active, escalated, force_modified) and the B records {mu, rho, tau, nu}.
//                          Escalated instances get their elastic multipliers reset (emi_ipm_start_kernel, masked).
//   2. Newton system       emi_hess_dev, emi_ipm_reduce_dev, emi_kkt_blocks_dev (eigenpair lists stay on the device; B counts come
//                          down), a copy of the right-hand side, then per instance the dual ladder of solve_nlp around
//                          emi_kkt_factor_shard_dev / emi_kkt_lowrank_shard_dev / emi_kkt_solve_refined_shard_dev (8 steps), each
//                          call masked to the instances it is for: dc = 0, raised to 1e-8 mu^1/4 and then x100 while the matrix is
//                          singular or the first solution is not finite, 24 attempts.  An instance with force_modified set has
//                          its correction cleared (max_mods 0): it takes the step of the convexified matrix.  An instance whose
//                          workspace left the Schur path, or that is still singular after the ladder, ends with EMI_IPM_FACTOR.
//   3. line search         emi_ipm_expand_dev, emi_ipm_merit_dev at the point, emi_ipm_search_kernel (init): penalty weight nu,
//                          merit and slope at the point, alpha = apr.  Then at most 40 passes of emi_ipm_trial_dev, emi_eval_dev
//                          without the Jacobian, emi_ipm_merit_dev with the slack reset, emi_ipm_search_kernel (step): Armijo test,
//                          alpha halved; B bytes come down (still searching) and the passes stop when none is.  An instance that
//                          has accepted keeps its alpha, so the later passes recompute its trial point to the same bits.
//                          emi_ipm_accept_dev with the accepted bytes as its mask, a_pr = alpha, a_du = adu.
//
// With EMI_IPM_RULE_RESIDUAL (residual-based acceptance and the crawl rule), after the search kernel of pass 0
// emi_ipm_rescue_kernel (candidates) marks the instances whose first trial failed and that are near a solution (err0 <= 1e-2) or
// crawling; B bytes more come down in the same synchronisation.  Only if one is marked: error components of the present iterate
// (second `parts`), rescue (select: err_mu, apr into its own [B] array), emi_ipm_keep_kernel (iterate of the candidates -> kept set),
// emi_ipm_trial_dev with apr into the FULL-STEP point (the ordinary trial arrays hold slack-reset points the accepted instances
// still need), emi_ipm_accept_dev from it under the candidate mask, emi_eval_dev / LamC / emi_lagr_grad_dev / error components into
// the second output set, rescue (decide), B verdict bytes down, emi_ipm_keep_kernel back under the taken-back mask.  An instance
// whose step stands has stopped searching with `accepted` clear; one taken back has every bit of its iterate again and goes on
// from apr / 2.  After the loop rescue (crawl) counts the short accepted steps.  rules == 0 launches none of this.
//
// An instance that has ended is masked out of every call that takes a mask; the unmasked kernels recompute its arrays from an
// iterate nobody writes any more.  Nothing an instance computes depends on another instance, and every sum has a fixed order:
// two identical calls give the same bits, and an instance ends with the same bits whatever the others do after it.
//
// Taken over from solve_nlp: start(), the convergence test with its emax condition, penalty escalation with the reset of the
// elastic multipliers and the futile rule, the acceptable-level counter, the barrier update (several firings per round), tau,
// the dual ladder, the exact / reflected verdict, the nu rule, the Armijo test, the slack reset at trial points, force_modified,
// a failed line search ending in the acceptable check, max_iter; behind opt.rules, residual-based acceptance and the crawl rule.
// NOT taken over: second-order correction, the inertia search (dw shifts), stagnation / mu_restart, vscale and Jacobian-based
// defect weights, warm-start multipliers, coupling rows, the time limit.  Differences the batched round forces: emi_ipm_control.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "emi_ctx.hpp"
#include "emi_ipm_control.hpp"

namespace emi {
namespace {

constexpr int CTL_T = 64;

// flags [3][B] bytes: still running, escalated in this round, force_modified
__global__ __launch_bounds__(CTL_T) void emi_ipm_barrier_kernel(const double* parts, IpmCtlState* st, IpmCtlOptions o, double* par,
                                                                unsigned char* flags, int B) {
    const int b = blockIdx.x * CTL_T + threadIdx.x;
    if (b >= B) return;
    IpmCtlState s = st[b];
    ipm_ctl_barrier(parts + (size_t)b * IPM_NPARTS, s, o);
    st[b] = s;
    par[b * 4] = s.mu; par[b * 4 + 1] = s.rho; par[b * 4 + 2] = s.tau; par[b * 4 + 3] = s.nu;
    flags[b] = s.status == IPM_RUNNING;
    flags[B + b] = s.escalated != 0;
    flags[2 * B + b] = s.force_modified != 0;
}

// form 0: head of the line search (scal [B][4], mer [B][2] at the point; hflag bit 1: the factorisation failed);
// form 1: one backtracking pass (mer at the trial point; hflag bit 0: exact step of a matrix with modified blocks)
__global__ __launch_bounds__(CTL_T) void emi_ipm_search_kernel(int form, const double* scal, const double* mer, const int* hflag,
                                                               IpmCtlState* st, IpmCtlOptions o, double* par, double* alpha, double* adu,
                                                               unsigned char* accepted, unsigned char* searching, int B) {
    const int b = blockIdx.x * CTL_T + threadIdx.x;
    if (b >= B) return;
    IpmCtlState s = st[b];
    if (form == 0) {
        ipm_ctl_search_init(scal + (size_t)b * 4, mer + (size_t)b * 2, (hflag[b] >> 1) & 1, s);
        par[b * 4 + 3] = s.nu;
        if (s.searching) { adu[b] = s.adu; }
    } else {
        ipm_ctl_search_step(mer + (size_t)b * 2, hflag[b] & 1, s, o);
    }
    if (s.searching || s.accepted) alpha[b] = s.alpha;
    st[b] = s;
    accepted[b] = s.accepted != 0;
    searching[b] = s.searching != 0;
}

// residual-based acceptance and the crawl rule, one thread per instance (the rules: emi_ipm_control.hpp)
//   RESCUE_CANDIDATES  after the search kernel of pass 0: cand[b] = the rule is for this instance
//   RESCUE_SELECT      parts: error components of the present iterate.  err_mu, cand[b], apr[b] = scal[b][0] (the full-step trial)
//   RESCUE_DECIDE      parts: error components of the stepped iterate.  back[b] = the step is taken back; searching[b]
//   RESCUE_CRAWL       after the line-search loop: the crawl counter of the instances that accepted
enum { RESCUE_CANDIDATES, RESCUE_SELECT, RESCUE_DECIDE, RESCUE_CRAWL };
__global__ __launch_bounds__(CTL_T) void emi_ipm_rescue_kernel(int form, const double* parts, const double* scal, IpmCtlState* st,
                                                               IpmCtlRescue* rs, IpmCtlOptions o, double* apr, unsigned char* cand,
                                                               unsigned char* back, unsigned char* searching, int B) {
    const int b = blockIdx.x * CTL_T + threadIdx.x;
    if (b >= B) return;
    IpmCtlState s = st[b];
    IpmCtlRescue r = rs[b];
    if (form == RESCUE_CANDIDATES) {
        cand[b] = ipm_ctl_rescue_applies(s, r, o);
        return;
    }
    if (form == RESCUE_SELECT) {
        ipm_ctl_rescue_select(parts + (size_t)b * IPM_NPARTS, s, r, o);
        cand[b] = r.candidate != 0;
        apr[b] = scal[(size_t)b * 4];
    } else if (form == RESCUE_DECIDE) {
        const bool tried = r.candidate != 0;
        const bool stands = ipm_ctl_rescue_decide(parts + (size_t)b * IPM_NPARTS, s, r);
        back[b] = tried && !stands;
        searching[b] = s.searching != 0;
        st[b] = s;
    } else {
        ipm_ctl_rescue_crawl(scal + (size_t)b * 4, s, r, o);
    }
    rs[b] = r;
}

// the iterate of the masked instances copied between the live arrays and a kept set (a.restore: kept -> live).  Grid (chunks of
// 256 nodes, B): the mask byte first, a masked-out workgroup returns at once; every access is a run of consecutive doubles along
// the node axis, one writer per element
constexpr int KEEP_T = 256;
__device__ __forceinline__ void keep_rows(double* live, double* kept, int restore, size_t first, int rows, int M, int k) {
    for (int i = 0; i < rows; ++i) {
        const size_t e = (first + i) * M + k;
        if (restore) live[e] = kept[e];
        else kept[e] = live[e];
    }
}
__global__ __launch_bounds__(KEEP_T) void emi_ipm_keep_kernel(IpmKeepArgs a) {
    const int b = blockIdx.y;
    if (a.mask && !a.mask[b]) return;
    const int k = blockIdx.x * KEEP_T + threadIdx.x;
    if (k >= a.M) return;
    const int nv = a.ns + a.nc;
    keep_rows(a.live[0], a.kept[0], a.restore, (size_t)b * a.ns, a.ns, a.M, k);                     // X
    if (a.nc > 0) keep_rows(a.live[1], a.kept[1], a.restore, (size_t)b * a.nc, a.nc, a.M, k);       // U
    keep_rows(a.live[5], a.kept[5], a.restore, (size_t)b * a.ns, a.ns, a.M, k);                     // LamF
    keep_rows(a.live[7], a.kept[7], a.restore, (size_t)b * nv, nv, a.M, k);                         // ZL
    keep_rows(a.live[8], a.kept[8], a.restore, (size_t)b * nv, nv, a.M, k);                         // ZU
    if (a.np > 0) {
        constexpr int rows[8] = {2, 3, 4, 6, 9, 10, 11, 12};                                        // S E1 E2 Y VL VU W1 W2
        for (int q = 0; q < 8; ++q) keep_rows(a.live[rows[q]], a.kept[rows[q]], a.restore, (size_t)b * a.np, a.np, a.M, k);
    }
}

bool any(const std::vector<unsigned char>& m) { return std::find(m.begin(), m.end(), (unsigned char)1) != m.end(); }

}  // namespace

// the device arrays of the driver: the part of the iterate the caller does not hold, the step, the trial point, the evaluations,
// the Newton system, the per-instance records; and the pinned host twins of what crosses per round
struct IpmSolveWs {
    DeviceArray<double> S, E1, E2, Y, ZL, ZU, VL, VU, W1, W2;
    DeviceArray<double> DZLam, DS, DY, DE1, DE2, DZL, DZU, DVL, DVU, DW1, DW2, rhs_keep;
    DeviceArray<double> Sigma, SigT, SigS, RhatS, Rt;
    DeviceArray<double> tX, tU, tS, tE1, tE2;
    DeviceArray<double> RES, VALS, COST, REt, COSTt, G, H, Q, Qx, delta, vec, worst;
    DeviceArray<double> par, parts, scal, mer, mert, alpha, adu;
    DeviceArray<int> count, node, hflag;
    DeviceArray<unsigned char> fixed, flags, accepted, searching;
    DeviceArray<IpmCtlState> state;
    PinnedArray<IpmCtlState> h_state;
    PinnedArray<double> h_par, h_cost;
    PinnedArray<int> h_count, h_hflag;
    PinnedArray<unsigned char> h_flags, h_searching;
    // residual-based acceptance (reserved only when the rule is on): the kept iterate, the full-step point, the second output set
    DeviceArray<double> kX, kU, kS, kE1, kE2, kLamF, kY, kZL, kZU, kVL, kVU, kW1, kW2;
    DeviceArray<double> fX, fU, fS, fE1, fE2;
    DeviceArray<double> RES2, VALS2, COST2, G2, parts2, apr_full;
    DeviceArray<unsigned char> rflags;          // [2][B]: candidate, taken back
    DeviceArray<IpmCtlRescue> rescue;
    PinnedArray<IpmCtlRescue> h_rescue;
    PinnedArray<unsigned char> h_rflags;
};

hipError_t launch_ipm_keep(const IpmKeepArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.M <= 0) return hipSuccess;
    hipLaunchKernelGGL(emi_ipm_keep_kernel, dim3((a.M + KEEP_T - 1) / KEEP_T, a.B), dim3(KEEP_T), 0, s, a);
    return hipGetLastError();
}

void ipm_solve_destroy(IpmSolveWs* w) { delete w; }

#define S_HIP(call) HIP_TRY_AS(c, "emi_ipm_solve_shard_dev", call)
#define S_TRY EMI_TRY

int ipm_solve_shard(emi_ctx_t c, void* dX, void* dU, const emi_ipm_bounds_t* bd, const emi_ipm_options_t& given, void* dLamF, void* dLamC,
                    emi_ipm_result_t* results) {
    if (!c->ipm_solve) c->ipm_solve = new IpmSolveWs();
    IpmSolveWs& w = *c->ipm_solve;
    const int B = c->B, M = c->M, ns = c->ns, nc = c->nc, nv = ns + nc, np = emi_api::np_total(c);
    const size_t nX = (size_t)B * ns * M, nU = (size_t)B * nc * M, nVar = (size_t)B * nv * M, nRow = (size_t)B * np * M;
    const size_t nKkt = (size_t)B * (nv + ns) * M, nRes = (size_t)B * (ns + np) * M, nVals = (size_t)B * emi_api::nvals_of(c) * M, nH = (size_t)B * emi_api::nhess_of(c) * M;
    const size_t N1 = (size_t)(nv + ns) * M;                    // unknowns of one instance
    const int mm = std::min(4096, nv * M);                      // eigenpairs per instance the lists hold (solve_nlp's max_lowrank)
    const hipStream_t s = c->stream;

    // zero-initialised options take solve_nlp's defaults (NlpOptions)
    emi_ipm_options_t opt = given;
    if (!(opt.tol > 0)) opt.tol = 1e-8;
    if (!(opt.mu_init > 0)) opt.mu_init = 0.1;
    if (!(opt.bound_push > 0)) opt.bound_push = 1e-2;
    if (!(opt.bound_frac > 0)) opt.bound_frac = 1e-2;
    if (!(opt.rho_init > 0)) opt.rho_init = 10.0;
    if (!(opt.acceptable_factor > 0)) opt.acceptable_factor = 100.0;
    if (opt.max_iter <= 0) opt.max_iter = 200;
    if (opt.acceptable_iter <= 0) opt.acceptable_iter = 10;
    if (opt.max_futile_escalations <= 0) opt.max_futile_escalations = 3;
    const bool rescue = (opt.rules & EMI_IPM_RULE_RESIDUAL) != 0;
    if (rescue && opt.crawl_limit <= 0) opt.crawl_limit = 3;
    if (rescue && !(opt.crawl_frac > 0)) opt.crawl_frac = 0.3;
    const IpmCtlOptions ctl{opt.tol, opt.acceptable_factor, opt.max_iter, opt.acceptable_iter, opt.max_futile_escalations, np > 0 ? 1 : 0,
                            rescue ? EMI_IPM_RULE_RESIDUAL : 0, rescue ? opt.crawl_limit : 0, rescue ? opt.crawl_frac : 0.0};

    // ---- the arrays (a launch in flight may still use one that has to move) ---------------------------------------------------------
    S_HIP(hipStreamSynchronize(s));
    for (auto* a : {&w.S, &w.E1, &w.E2, &w.Y, &w.VL, &w.VU, &w.W1, &w.W2, &w.DS, &w.DY, &w.DE1, &w.DE2, &w.DVL, &w.DVU, &w.DW1, &w.DW2, &w.SigT,
                    &w.SigS, &w.RhatS, &w.Rt, &w.tS, &w.tE1, &w.tE2})
        S_HIP(a->reserve(nRow));
    for (auto* a : {&w.ZL, &w.ZU, &w.DZL, &w.DZU, &w.Sigma, &w.G}) S_HIP(a->reserve(nVar));
    for (auto* a : {&w.DZLam, &w.rhs_keep}) S_HIP(a->reserve(nKkt));
    for (auto* a : {&w.H, &w.Q, &w.Qx}) S_HIP(a->reserve(nH));
    for (auto* a : {&w.RES, &w.REt}) S_HIP(a->reserve(nRes));
    for (auto* a : {&w.COST, &w.COSTt, &w.worst, &w.alpha, &w.adu}) S_HIP(a->reserve((size_t)B));
    S_HIP(w.tX.reserve(nX)); S_HIP(w.tU.reserve(nU)); S_HIP(w.VALS.reserve(nVals));
    S_HIP(w.delta.reserve((size_t)B * mm)); S_HIP(w.vec.reserve((size_t)B * mm * nv)); S_HIP(w.node.reserve((size_t)B * mm));
    S_HIP(w.par.reserve((size_t)B * 4)); S_HIP(w.scal.reserve((size_t)B * 4)); S_HIP(w.parts.reserve((size_t)B * IPM_NPARTS));
    S_HIP(w.mer.reserve((size_t)B * 2)); S_HIP(w.mert.reserve((size_t)B * 2));
    S_HIP(w.count.reserve((size_t)B)); S_HIP(w.hflag.reserve((size_t)B));
    S_HIP(w.fixed.reserve(nVar)); S_HIP(w.flags.reserve((size_t)3 * B)); S_HIP(w.accepted.reserve((size_t)B)); S_HIP(w.searching.reserve((size_t)B));
    S_HIP(w.state.reserve((size_t)B));
    S_HIP(w.h_state.reserve((size_t)B)); S_HIP(w.h_par.reserve((size_t)B * 4)); S_HIP(w.h_cost.reserve((size_t)B));
    S_HIP(w.h_count.reserve((size_t)B)); S_HIP(w.h_hflag.reserve((size_t)B));
    S_HIP(w.h_flags.reserve((size_t)3 * B)); S_HIP(w.h_searching.reserve((size_t)B));
    if (rescue) {
        for (auto* a : {&w.kS, &w.kE1, &w.kE2, &w.kY, &w.kVL, &w.kVU, &w.kW1, &w.kW2, &w.fS, &w.fE1, &w.fE2}) S_HIP(a->reserve(nRow));
        for (auto* a : {&w.kZL, &w.kZU, &w.G2}) S_HIP(a->reserve(nVar));
        for (auto* a : {&w.kX, &w.kLamF, &w.fX}) S_HIP(a->reserve(nX));
        for (auto* a : {&w.kU, &w.fU}) S_HIP(a->reserve(nU));
        S_HIP(w.RES2.reserve(nRes)); S_HIP(w.VALS2.reserve(nVals)); S_HIP(w.COST2.reserve((size_t)B)); S_HIP(w.apr_full.reserve((size_t)B));
        S_HIP(w.parts2.reserve((size_t)B * IPM_NPARTS)); S_HIP(w.rflags.reserve((size_t)2 * B)); S_HIP(w.rescue.reserve((size_t)B));
        S_HIP(w.h_rescue.reserve((size_t)B)); S_HIP(w.h_rflags.reserve((size_t)2 * B));
    }

    emi_ipm_point_t pt{dX, dU, w.S.p, w.E1.p, w.E2.p}, tr{w.tX.p, w.tU.p, w.tS.p, w.tE1.p, w.tE2.p};
    emi_ipm_duals_t du{dLamF, w.Y.p, w.ZL.p, w.ZU.p, w.VL.p, w.VU.p, w.W1.p, w.W2.p};
    emi_ipm_step_t stp{w.DZLam.p, w.DS.p, w.DY.p, w.DE1.p, w.DE2.p, w.DZL.p, w.DZU.p, w.DVL.p, w.DVU.p, w.DW1.p, w.DW2.p};
    emi_ipm_elim_t el{w.Sigma.p, w.SigT.p, w.SigS.p, w.RhatS.p, w.Rt.p};
    const dim3 cgrid((B + CTL_T - 1) / CTL_T), cblock(CTL_T);
    // residual-based acceptance: the kept iterate and the full-step point (null arrays while the rule is off)
    const emi_ipm_point_t full{w.fX.p, w.fU.p, w.fS.p, w.fE1.p, w.fE2.p};
    IpmKeepArgs keep{};
    keep.B = B; keep.M = M; keep.ns = ns; keep.nc = nc; keep.np = np;
    {
        double* const live[13] = {(double*)dX, (double*)dU, w.S.p, w.E1.p, w.E2.p, (double*)dLamF, w.Y.p, w.ZL.p, w.ZU.p, w.VL.p, w.VU.p, w.W1.p, w.W2.p};
        double* const kept[13] = {w.kX.p, w.kU.p, w.kS.p, w.kE1.p, w.kE2.p, w.kLamF.p, w.kY.p, w.kZL.p, w.kZU.p, w.kVL.p, w.kVU.p, w.kW1.p, w.kW2.p};
        std::copy(live, live + 13, keep.live);
        std::copy(kept, kept + 13, keep.kept);
    }
    const auto rescue_launch = [&](int form, const double* parts) {
        hipLaunchKernelGGL(emi_ipm_rescue_kernel, cgrid, cblock, 0, s, form, parts, w.scal.p, w.state.p, w.rescue.p, ctl, w.apr_full.p, w.rflags.p,
                           w.rflags.p + B, w.searching.p, B);
        return hipGetLastError();
    };

    // ---- start(): state records, interior push; the rest follows the first evaluation ---------------------------------------------
    for (KktWorkspace* k : c->kkt_shard) kkt_forget_ladder(k);
    for (int b = 0; b < B; ++b) {
        ipm_ctl_start(w.h_state.p[b], opt.mu_init, opt.rho_init);
        double* p = w.h_par.p + (size_t)b * 4;
        p[0] = opt.mu_init; p[1] = opt.rho_init; p[2] = 0.0; p[3] = 1.0;
    }
    S_HIP(hipMemcpyAsync(w.state.p, w.h_state.p, (size_t)B * sizeof(IpmCtlState), hipMemcpyHostToDevice, s));
    S_HIP(hipMemcpyAsync(w.par.p, w.h_par.p, (size_t)B * 4 * sizeof(double), hipMemcpyHostToDevice, s));
    S_HIP(hipMemsetAsync(w.alpha.p, 0, (size_t)B * sizeof(double), s));
    S_HIP(hipMemsetAsync(w.adu.p, 0, (size_t)B * sizeof(double), s));
    if (rescue) {
        for (int b = 0; b < B; ++b) ipm_ctl_rescue_start(w.h_rescue.p[b]);
        S_HIP(hipMemcpyAsync(w.rescue.p, w.h_rescue.p, (size_t)B * sizeof(IpmCtlRescue), hipMemcpyHostToDevice, s));
    }
    S_TRY(emi_ipm_start_dev(c, 0, &pt, &du, nullptr, bd, w.par.p, opt.bound_push, opt.bound_frac, w.fixed.p, nullptr));

    std::vector<unsigned char> act(B, 1), fm(B, 0), todo(B), fresh(B), m_lists(B), m_clear(B), dirty(B), failed(B), search(B);
    std::vector<double> dc(B), rel(B);
    std::vector<int> info(B), exact(B), nsol(B), rev(B), sst(B), nfact(B, 0), nrefl(B, 0);

    for (int round = 0; round <= opt.max_iter + 1; ++round) {
        // ---- 1. evaluate and test -------------------------------------------------------------------------------------------------
        S_TRY(emi_eval_dev(c, dX, dU, w.RES.p, w.VALS.p, w.COST.p, EMI_EVAL_ALL));
        if (round == 0) S_TRY(emi_ipm_start_dev(c, 1, &pt, &du, w.RES.p, bd, w.par.p, opt.bound_push, opt.bound_frac, w.fixed.p, nullptr));
        if (np > 0) {           // path-row multipliers in the caller's units, for the gradient and the Hessian
            IpmArgs a{};
            a.Y = w.Y.p; a.LamC = (double*)dLamC;
            S_TRY(emi_api::ctx_ipm_launch(c, IPM_LAMC, bd, w.par.p, a));
        }
        S_TRY(emi_lagr_grad_dev(c, w.VALS.p, dLamF, dLamC, 1.0, w.G.p));
        S_TRY(emi_ipm_error_parts_dev(c, &pt, &du, w.RES.p, w.G.p, bd, w.par.p, w.parts.p));
        hipLaunchKernelGGL(emi_ipm_barrier_kernel, cgrid, cblock, 0, s, w.parts.p, w.state.p, ctl, w.par.p, w.flags.p, B);
        S_HIP(hipGetLastError());
        S_HIP(hipMemcpyAsync(w.h_flags.p, w.flags.p, (size_t)3 * B, hipMemcpyDeviceToHost, s));
        S_HIP(hipMemcpyAsync(w.h_par.p, w.par.p, (size_t)B * 4 * sizeof(double), hipMemcpyDeviceToHost, s));      // (mu, for raise_dc)
        S_HIP(hipStreamSynchronize(s));
        bool escalated = false;
        for (int b = 0; b < B; ++b) {
            act[b] = w.h_flags.p[b];
            fm[b] = w.h_flags.p[2 * B + b];
            escalated = escalated || (act[b] && w.h_flags.p[B + b]);
        }
        if (!any(act)) break;
        if (escalated && np > 0)        // reset_elastic_duals of the instances that raised their penalty weight
            S_TRY(emi_ipm_start_dev(c, 2, &pt, &du, nullptr, bd, w.par.p, opt.bound_push, opt.bound_frac, nullptr, w.flags.p + B));

        // ---- 2. Newton system -----------------------------------------------------------------------------------------------------
        S_TRY(emi_hess_dev(c, dX, dU, dLamF, dLamC, 1.0, w.H.p));
        S_TRY(emi_ipm_reduce_dev(c, &pt, &du, w.RES.p, w.VALS.p, w.G.p, bd, w.par.p, nullptr, nullptr, &el, w.DZLam.p));
        S_TRY(emi_kkt_blocks_dev(c, w.H.p, w.VALS.p, w.Sigma.p, w.SigT.p, w.fixed.p, 0.0, w.Qx.p, w.Q.p, mm, w.count.p, w.node.p, w.delta.p,
                                 w.vec.p, w.worst.p));
        S_HIP(hipMemcpyAsync(w.rhs_keep.p, w.DZLam.p, nKkt * sizeof(double), hipMemcpyDeviceToDevice, s));
        S_HIP(hipMemcpyAsync(w.h_count.p, w.count.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s));
        S_HIP(hipStreamSynchronize(s));
        std::fill(dc.begin(), dc.end(), 0.0);
        std::fill(exact.begin(), exact.end(), 0);
        std::fill(failed.begin(), failed.end(), 0);
        std::fill(dirty.begin(), dirty.end(), 0);
        todo = act;
        for (int attempt = 0; attempt < 24 && any(todo); ++attempt) {
            S_TRY(emi_kkt_factor_shard_dev(c, w.Q.p, w.VALS.p, w.fixed.p, dc.data(), todo.data(), info.data()));
            for (int b = 0; b < B; ++b) {
                fresh[b] = 0;
                if (!todo[b]) continue;
                ++nfact[b];
                if (info[b] > 0) dc[b] = ipm_ctl_raise_dc(dc[b], w.h_par.p[(size_t)b * 4]);     // singular: regularise the dual block
                else if (kkt_holds(c->kkt_shard[b], M, ns, nv) != 1) { failed[b] = 1; todo[b] = 0; }    // the instance left the Schur path
                else fresh[b] = 1;
                m_lists[b] = fresh[b] && !fm[b];
                m_clear[b] = fresh[b] && fm[b];
            }
            if (!any(fresh)) continue;
            if (any(m_lists))
                S_TRY(emi_kkt_lowrank_shard_dev(c, mm, w.count.p, w.node.p, w.delta.p, w.vec.p, m_lists.data(), exact.data()));
            if (any(m_clear)) S_TRY(emi_kkt_lowrank_shard_dev(c, 0, nullptr, nullptr, nullptr, nullptr, m_clear.data(), exact.data()));
            for (int b = 0; b < B; ++b)
                if (fresh[b] && dirty[b])
                    S_HIP(hipMemcpyAsync(w.DZLam.p + b * N1, w.rhs_keep.p + b * N1, N1 * sizeof(double), hipMemcpyDeviceToDevice, s));
            S_TRY(emi_kkt_solve_refined_shard_dev(c, w.DZLam.p, fresh.data(), dc.data(), 8, rel.data(), nsol.data(), rev.data(), sst.data()));
            for (int b = 0; b < B; ++b) {
                if (!fresh[b]) continue;
                if (sst[b] == 2) { dc[b] = ipm_ctl_raise_dc(dc[b], w.h_par.p[(size_t)b * 4]); dirty[b] = 1; }     // first solution not finite
                else todo[b] = 0;
            }
        }
        for (int b = 0; b < B; ++b) {
            if (todo[b]) failed[b] = 1;         // still singular after the dual ladder
            const bool exact_step = exact[b] == 1 && !fm[b];
            w.h_hflag.p[b] = (exact_step && w.h_count.p[b] > 0 ? 1 : 0) | (failed[b] ? 2 : 0);
            if (act[b] && !failed[b] && w.h_count.p[b] > 0 && !exact_step) ++nrefl[b];
            search[b] = act[b] && !failed[b];
        }
        S_HIP(hipMemcpyAsync(w.hflag.p, w.h_hflag.p, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));

        // ---- 3. line search -------------------------------------------------------------------------------------------------------
        S_TRY(emi_ipm_expand_dev(c, &pt, &du, w.VALS.p, bd, w.par.p, &el, nullptr, &stp, w.scal.p));
        S_TRY(emi_ipm_merit_dev(c, &pt, w.RES.p, w.COST.p, bd, w.par.p, nullptr, 0, w.mer.p));
        hipLaunchKernelGGL(emi_ipm_search_kernel, cgrid, cblock, 0, s, 0, w.scal.p, w.mer.p, w.hflag.p, w.state.p, ctl, w.par.p, w.alpha.p,
                           w.adu.p, w.accepted.p, w.searching.p, B);
        S_HIP(hipGetLastError());
        for (int pass = 0; pass < 40 && any(search); ++pass) {
            S_TRY(emi_ipm_trial_dev(c, &pt, &stp, w.alpha.p, &tr));
            S_TRY(emi_eval_dev(c, w.tX.p, w.tU.p, w.REt.p, nullptr, w.COSTt.p, EMI_EVAL_ALL | EMI_EVAL_NOJAC));
            S_TRY(emi_ipm_merit_dev(c, &tr, w.REt.p, w.COSTt.p, bd, w.par.p, nullptr, 1, w.mert.p));
            hipLaunchKernelGGL(emi_ipm_search_kernel, cgrid, cblock, 0, s, 1, w.scal.p, w.mert.p, w.hflag.p, w.state.p, ctl, w.par.p, w.alpha.p,
                               w.adu.p, w.accepted.p, w.searching.p, B);
            S_HIP(hipGetLastError());
            const bool ask = rescue && pass == 0;
            if (ask) {
                S_HIP(rescue_launch(RESCUE_CANDIDATES, nullptr));
                S_HIP(hipMemcpyAsync(w.h_rflags.p, w.rflags.p, (size_t)B, hipMemcpyDeviceToHost, s));
            }
            S_HIP(hipMemcpyAsync(w.h_searching.p, w.searching.p, (size_t)B, hipMemcpyDeviceToHost, s));
            S_HIP(hipStreamSynchronize(s));
            for (int b = 0; b < B; ++b) search[b] = w.h_searching.p[b];
            if (!ask || std::find(w.h_rflags.p, w.h_rflags.p + B, (unsigned char)1) == w.h_rflags.p + B) continue;
            // ---- residual-based acceptance: the full step of the candidates, judged by the KKT error of their barrier problem -------
            S_TRY(emi_ipm_error_parts_dev(c, &pt, &du, w.RES.p, w.G.p, bd, w.par.p, w.parts2.p));
            S_HIP(rescue_launch(RESCUE_SELECT, w.parts2.p));
            keep.mask = w.rflags.p; keep.restore = 0;
            S_HIP(launch_ipm_keep(keep, s));
            S_TRY(emi_ipm_trial_dev(c, &pt, &stp, w.apr_full.p, &full));
            S_TRY(emi_ipm_accept_dev(c, &pt, &full, &du, &stp, bd, w.par.p, w.apr_full.p, w.adu.p, w.rflags.p));
            S_TRY(emi_eval_dev(c, dX, dU, w.RES2.p, w.VALS2.p, w.COST2.p, EMI_EVAL_ALL));
            if (np > 0) {
                IpmArgs a{};
                a.Y = w.Y.p; a.LamC = (double*)dLamC;
                S_TRY(emi_api::ctx_ipm_launch(c, IPM_LAMC, bd, w.par.p, a));
            }
            S_TRY(emi_lagr_grad_dev(c, w.VALS2.p, dLamF, dLamC, 1.0, w.G2.p));
            S_TRY(emi_ipm_error_parts_dev(c, &pt, &du, w.RES2.p, w.G2.p, bd, w.par.p, w.parts2.p));
            S_HIP(rescue_launch(RESCUE_DECIDE, w.parts2.p));
            keep.mask = w.rflags.p + B; keep.restore = 1;
            S_HIP(launch_ipm_keep(keep, s));
            S_HIP(hipMemcpyAsync(w.h_rflags.p + B, w.rflags.p + B, (size_t)B, hipMemcpyDeviceToHost, s));
            S_HIP(hipStreamSynchronize(s));
            for (int b = 0; b < B; ++b)
                if (w.h_rflags.p[b] && !w.h_rflags.p[B + b]) search[b] = 0;       // the step stands: the iteration is over
        }
        if (rescue) S_HIP(rescue_launch(RESCUE_CRAWL, nullptr));
        S_TRY(emi_ipm_accept_dev(c, &pt, &tr, &du, &stp, bd, w.par.p, w.alpha.p, w.adu.p, w.accepted.p));
    }

    // ---- results --------------------------------------------------------------------------------------------------------------------
    S_HIP(hipMemcpyAsync(w.h_state.p, w.state.p, (size_t)B * sizeof(IpmCtlState), hipMemcpyDeviceToHost, s));
    S_HIP(hipMemcpyAsync(w.h_cost.p, w.COST.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (rescue) S_HIP(hipMemcpyAsync(w.h_rescue.p, w.rescue.p, (size_t)B * sizeof(IpmCtlRescue), hipMemcpyDeviceToHost, s));
    S_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        const IpmCtlState& t = w.h_state.p[b];
        emi_ipm_result_t& r = results[b];
        r.status = t.status == IPM_RUNNING ? EMI_IPM_MAX_ITER : t.status;
        r.iterations = t.iterations; r.evaluations = t.evaluations; r.factorisations = nfact[b]; r.reflected_steps = nrefl[b];
        r.cost = w.h_cost.p[b]; r.kkt_error = t.err0; r.constr_viol = t.viol; r.emax = t.emax; r.mu = t.mu; r.rho = t.rho;
        r.newton_steps = rescue ? w.h_rescue.p[b].newton_steps : 0;
        r.restored_steps = rescue ? w.h_rescue.p[b].restored_steps : 0;
    }
    return EMI_OK;
}

}  // namespace emi
