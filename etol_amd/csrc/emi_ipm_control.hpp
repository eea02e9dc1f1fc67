// emi_ipm_control.hpp -- the per-instance scalar rules of the lock-step interior-point driver (emi_ipm_solve.hip), written once.
//
// The driver runs one iteration of every instance of a batch per round; what decides how an instance goes on -- convergence,
// penalty escalation, barrier update, penalty weight of the merit function, Armijo test, step halving -- is a handful of scalar
// rules on a per-instance state record.  They are the rules of solve_nlp's phases (host/emi_nlp.cpp: test_and_update_barrier,
// line_search, futile_escalation, escalate_penalty, acceptable, armijo, raise_dc), as functions of plain structs: the control
// kernels call them with one thread per instance, and the host shim of the CPU test calls the same text (the pattern of
// pass_role_of in emi_pass_work.hpp).
//
// Where a rule differs from solve_nlp because the round is batched:
//   * a round that escalated the penalty runs NO barrier update.  solve_nlp resets the elastic multipliers in place and goes on
//     into its barrier loop with them; here the reset is an array kernel that runs after this scalar rule, so the loop would see
//     the error components of the multipliers before the reset.  The update follows in the next round.
//   * mu^1.5 is mu sqrt(mu) and mu^0.25 is sqrt(sqrt(mu)): correctly rounded on host and device alike, where pow is not.
//   * an error that is not finite ends the instance (EMI_IPM_NOT_FINITE); solve_nlp has no such exit.
//   * residual-based acceptance (EMI_IPM_RULE_RESIDUAL) is three steps around array kernels -- select, the full step and its
//     evaluation, decide -- with its own record per instance (IpmCtlRescue).  A stepped iterate with ANY component of its error
//     that is not finite is taken back (solve_nlp asks std::isfinite of the maximum, which drops a NaN); the attempt counts as one
//     evaluation and a kept step is evaluated again at the head of the next round, where solve_nlp goes on with the values it has.
// Every function is free of fused multiply-adds (contraction off), so the host and the device compute the same bits.
#pragma once

#include <math.h>

#include "emi355x.h"

#if defined(__HIPCC__)
#define EMI_CTL_HD __host__ __device__
#else
#define EMI_CTL_HD
#endif
#if defined(__clang__)
#define EMI_CTL_NO_FMA _Pragma("clang fp contract(off)")
#else
#define EMI_CTL_NO_FMA
#endif

namespace emi {

constexpr int IPM_RUNNING = -1;     // status of an instance that is still iterated on (never returned)

struct IpmCtlOptions {
    double tol, acceptable_factor;
    int max_iter, acceptable_iter, max_futile_escalations;
    int has_rows;                   // the problem has path rows (np > 0)
    // residual-based acceptance and the crawl rule (at the end: a record built from the fields above leaves them zero, the rule off)
    int rules;                      // EMI_IPM_RULE_* bits
    int crawl_limit;                // consecutive short steps before the crawl rule acts
    double crawl_frac;              // a step is short below this fraction of the longest admissible one
};

// the state record of one instance
struct IpmCtlState {
    double mu, rho, tau, nu;        // what the array kernels read as par[b] = {mu, rho, tau, nu}
    double emax_ref;                // futile rule: the largest elastic at the last escalation that helped
    double err0, viol, emax;        // of the last test: KKT error at mu = 0, largest residual, largest elastic
    double phi0, slope, alpha, adu; // line search: merit and slope at the point, the trial length, the dual length
    int n_acceptable, futile, iterations, status, force_modified;
    int escalated;                  // this round raised the penalty weight: the elastic multipliers are to be reset
    int searching, accepted, passes;
    int evaluations;
};

// components of the scaled KKT error (emi_ipm_error_parts_*): the error of ANY barrier parameter follows from them
enum { IPM_P_ED, IPM_P_SD, IPM_P_EP, IPM_P_SC, IPM_P_PMIN, IPM_P_PMAX, IPM_P_EMAX, IPM_P_YMAX, IPM_NPARTS };

EMI_CTL_HD inline double ipm_ctl_max(double a, double b) { return a > b ? a : b; }
EMI_CTL_HD inline double ipm_ctl_min(double a, double b) { return a < b ? a : b; }

EMI_CTL_HD inline double ipm_ctl_kkt(const double* p, double mu_t) {
    EMI_CTL_NO_FMA
    const double ec = ipm_ctl_max(0.0, ipm_ctl_max(p[IPM_P_PMAX] - mu_t, mu_t - p[IPM_P_PMIN]));
    return ipm_ctl_max(ipm_ctl_max(p[IPM_P_ED] / p[IPM_P_SD], p[IPM_P_EP]), ec / p[IPM_P_SC]);
}

EMI_CTL_HD inline void ipm_ctl_start(IpmCtlState& s, double mu_init, double rho_init) {
    s.mu = mu_init; s.rho = rho_init; s.tau = 0.0; s.nu = 1.0;
    s.emax_ref = 1e300;
    s.err0 = s.viol = s.emax = 0.0;
    s.phi0 = s.slope = s.alpha = s.adu = 0.0;
    s.n_acceptable = s.futile = s.iterations = 0;
    s.status = IPM_RUNNING;
    s.force_modified = s.escalated = s.searching = s.accepted = s.passes = 0;
    s.evaluations = 0;
}

EMI_CTL_HD inline bool ipm_ctl_acceptable(const IpmCtlState& s, const IpmCtlOptions& o) {
    EMI_CTL_NO_FMA
    return s.err0 <= o.acceptable_factor * o.tol && (!o.has_rows || s.emax <= 1e-6);
}

// beyond 1e5, max_futile_escalations tenfold raises in a row that have not halved the largest elastic end the solve
EMI_CTL_HD inline bool ipm_ctl_futile(IpmCtlState& s, const IpmCtlOptions& o, double emax_now) {
    EMI_CTL_NO_FMA
    if (s.rho < 1e5) return false;
    if (emax_now < 0.5 * s.emax_ref) { s.emax_ref = emax_now; s.futile = 0; return false; }
    return ++s.futile >= o.max_futile_escalations;
}

EMI_CTL_HD inline void ipm_ctl_escalate(IpmCtlState& s) {
    EMI_CTL_NO_FMA
    s.rho *= 10.0;
    s.mu = ipm_ctl_max(s.mu, 1e-2);
    s.escalated = 1;
}

// test_and_update_barrier on the error components of the iterate, at the head of a round (the full evaluation of the iterate
// is counted here).  Leaves status at IPM_RUNNING or sets how the instance ended.
EMI_CTL_HD inline void ipm_ctl_barrier(const double* p, IpmCtlState& s, const IpmCtlOptions& o) {
    EMI_CTL_NO_FMA
    s.escalated = 0;
    if (s.status != IPM_RUNNING) return;
    ++s.evaluations;
    const double err0 = ipm_ctl_kkt(p, 0.0), emax = p[IPM_P_EMAX];
    s.err0 = err0; s.viol = p[IPM_P_EP]; s.emax = emax;
    double all = err0;                  // (a maximum drops a NaN: every component is asked)
    for (int i = 0; i < IPM_NPARTS; ++i) all += p[i];
    if (!(all - all == 0.0)) { s.status = EMI_IPM_NOT_FINITE; return; }
    if (err0 <= o.tol) {
        if (emax <= ipm_ctl_max(o.tol, 1e-9) * 10.0 || !o.has_rows) { s.status = EMI_IPM_CONVERGED; return; }
        // a path row is still relaxed: the penalty was too small for it
        if (s.rho >= 1e12 || ipm_ctl_futile(s, o, emax)) { s.status = EMI_IPM_INFEASIBLE; return; }
        ipm_ctl_escalate(s);
    }
    if (ipm_ctl_acceptable(s, o)) {
        if (++s.n_acceptable >= o.acceptable_iter) { s.status = EMI_IPM_ACCEPTABLE; return; }
    } else {
        s.n_acceptable = 0;
    }
    if (s.iterations >= o.max_iter) { s.status = EMI_IPM_MAX_ITER; return; }
    // barrier update (may fire several times in a row)
    const double kappa_eps = 10.0, kappa_mu = 0.2;
    while (!s.escalated && s.mu > o.tol / 10.0 && ipm_ctl_kkt(p, s.mu) <= kappa_eps * s.mu) {
        // this barrier problem is solved.  A row multiplier at the penalty weight, or an elastic still far above mu / rho, means
        // the weight is too small for that row: raise it now instead of converging to a relaxed point first
        if (o.has_rows && (emax > ipm_ctl_max(1e-6, 100.0 * s.mu) || p[IPM_P_YMAX] > 0.9 * s.rho) && s.rho < 1e12) {
            if (ipm_ctl_futile(s, o, emax)) { s.status = EMI_IPM_INFEASIBLE; return; }
            ipm_ctl_escalate(s);
            s.nu = 1.0;
            break;
        }
        s.mu = ipm_ctl_max(o.tol / 10.0, ipm_ctl_min(kappa_mu * s.mu, s.mu * sqrt(s.mu)));
        s.nu = 1.0;     // a new barrier problem: the penalty weight is rebuilt from its multipliers, not inherited
    }
    s.tau = ipm_ctl_max(0.99, 1.0 - s.mu);
}

// dual regularisation of the next factorisation attempt of an instance whose matrix was singular (host side of the driver)
EMI_CTL_HD inline double ipm_ctl_raise_dc(double dc, double mu) {
    EMI_CTL_NO_FMA
    return dc == 0.0 ? 1e-8 * sqrt(sqrt(mu)) : dc * 100.0;
}

// head of the line search: scal = {apr, adu, dphi, mmax} of the expanded step, mer = {barrier function, infeasibility} at the
// point.  factor_failed: the Newton system of this instance could not be factorised (the instance ends here).
EMI_CTL_HD inline void ipm_ctl_search_init(const double* scal, const double* mer, int factor_failed, IpmCtlState& s) {
    EMI_CTL_NO_FMA
    s.searching = s.accepted = s.passes = 0;
    if (s.status != IPM_RUNNING) return;
    if (factor_failed) { s.status = EMI_IPM_FACTOR; return; }
    const double dphi = scal[2], mmax = scal[3], infeas0 = mer[1];
    // penalty weight of the l1 merit function: what the multipliers and the descent condition ask for; it may come down again,
    // at most halving per iteration
    double nu_want = ipm_ctl_max(1.0, ipm_ctl_min(1.1 * mmax, 1e8));
    if (infeas0 > 0) nu_want = ipm_ctl_max(nu_want, dphi / (0.9 * infeas0) + 1.0);
    s.nu = ipm_ctl_max(nu_want, 0.5 * s.nu);
    const double pen = s.nu * infeas0;
    s.phi0 = mer[0] + pen;
    s.slope = dphi - pen;
    s.alpha = scal[0];
    s.adu = scal[1];
    s.searching = 1;
}

EMI_CTL_HD inline bool ipm_ctl_armijo(double phi, double a, double phi0, double slope) {
    EMI_CTL_NO_FMA
    const double t1 = 1e-4 * a * ipm_ctl_min(slope, 0.0), t2 = 1e-13 * fabs(phi0);
    return phi - phi == 0.0 && phi <= phi0 + t1 + t2;
}

// one pass of the backtracking: mer = {barrier function, infeasibility} at the trial point of length s.alpha (slacks reset).
// exact_with_mods: the step is the exact Newton step of a matrix whose node blocks had to be modified -- if the search rejects
// it, the next round redoes the iteration with the step of the convexified matrix (force_modified).
EMI_CTL_HD inline void ipm_ctl_search_step(const double* mer, int exact_with_mods, IpmCtlState& s, const IpmCtlOptions& o) {
    EMI_CTL_NO_FMA
    if (s.status != IPM_RUNNING || !s.searching) return;
    ++s.evaluations;
    const double pen = s.nu * mer[1];
    const double phi = mer[0] + pen;
    if (ipm_ctl_armijo(phi, s.alpha, s.phi0, s.slope)) {
        s.accepted = 1;
        s.searching = 0;
        s.force_modified = 0;
        ++s.iterations;
        return;
    }
    if (++s.passes < 40) { s.alpha *= 0.5; return; }
    s.searching = 0;
    if (exact_with_mods && !s.force_modified) {
        // the exact Newton direction is not a descent direction the merit function accepts here
        s.force_modified = 1;
        ++s.iterations;
        return;
    }
    s.force_modified = 0;
    // a search that can go no further: the point is a solution only if it meets the acceptable level
    s.status = ipm_ctl_acceptable(s, o) ? EMI_IPM_ACCEPTABLE : EMI_IPM_LINE_SEARCH;
}

// ---- residual-based acceptance of the full step and the crawl rule (solve_nlp: residual_based_acceptance and the lines around
// its call in line_search) ---------------------------------------------------------------------------------------------------------
// what the rule keeps per instance, apart from IpmCtlState (whose layout the CPU test's shim fills field by field)
struct IpmCtlRescue {
    int crawl;                      // accepted steps in a row that were shorter than crawl_frac apr
    int candidate;                  // between select and decide: the full step of this instance is being tried
    int newton_steps, restored_steps;   // full steps kept / taken back
    double err_mu;                  // KKT error of the present barrier problem at the iterate the step starts from
};

EMI_CTL_HD inline void ipm_ctl_rescue_start(IpmCtlRescue& r) {
    r.crawl = r.candidate = r.newton_steps = r.restored_steps = 0;
    r.err_mu = 0.0;
}

// the first trial point (length apr) of this instance has just failed the Armijo test, and the rule is for it
EMI_CTL_HD inline bool ipm_ctl_rescue_applies(const IpmCtlState& s, const IpmCtlRescue& r, const IpmCtlOptions& o) {
    EMI_CTL_NO_FMA
    if (!(o.rules & EMI_IPM_RULE_RESIDUAL) || s.status != IPM_RUNNING || !s.searching || s.passes != 1) return false;
    return s.err0 <= 1e-2 || r.crawl >= o.crawl_limit;
}

// select, after the first backtracking pass: parts_now are the error components of the iterate with its present multipliers and
// penalty weight (the round head's predate the reset of the elastic multipliers an escalation brings)
EMI_CTL_HD inline void ipm_ctl_rescue_select(const double* parts_now, const IpmCtlState& s, IpmCtlRescue& r, const IpmCtlOptions& o) {
    EMI_CTL_NO_FMA
    r.candidate = ipm_ctl_rescue_applies(s, r, o) ? 1 : 0;
    if (r.candidate) r.err_mu = ipm_ctl_kkt(parts_now, s.mu);
}

// decide, from the error components of the stepped iterate: true = the step stands (the iteration is over, and the accept at the
// end of the line search must not touch the instance), false = the iterate is to be restored and the search goes on with the
// alpha the search step has already halved.  An instance that is no candidate is left as it is (false).
EMI_CTL_HD inline bool ipm_ctl_rescue_decide(const double* parts_tr, IpmCtlState& s, IpmCtlRescue& r) {
    EMI_CTL_NO_FMA
    if (!r.candidate) return false;
    r.candidate = 0;
    ++s.evaluations;
    const double err_tr = ipm_ctl_kkt(parts_tr, s.mu);
    double all = err_tr;                // (a maximum drops a NaN: every component is asked)
    for (int i = 0; i < IPM_NPARTS; ++i) all += parts_tr[i];
    if (all - all == 0.0 && err_tr <= 0.9 * r.err_mu) {
        s.searching = 0;
        s.accepted = 0;
        s.force_modified = 0;
        ++s.iterations;
        r.crawl = 0;
        ++r.newton_steps;
        return true;
    }
    ++r.restored_steps;
    return false;
}

// crawl update, once after the line-search loop: scal[0] is apr, s.alpha the accepted length
EMI_CTL_HD inline void ipm_ctl_rescue_crawl(const double* scal, const IpmCtlState& s, IpmCtlRescue& r, const IpmCtlOptions& o) {
    EMI_CTL_NO_FMA
    if (!(o.rules & EMI_IPM_RULE_RESIDUAL) || !s.accepted) return;
    r.crawl = s.alpha < o.crawl_frac * scal[0] ? r.crawl + 1 : 0;
}

}  // namespace emi
