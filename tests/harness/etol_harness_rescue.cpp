// etol_harness_rescue.cpp -- extern "C" shim for the tests of the lock-step driver's residual-based acceptance and crawl rule
// (EMI_IPM_RULE_RESIDUAL):
//   * the three rule functions of csrc/emi_ipm_control.hpp (select, decide, crawl update), the text emi_ipm_rescue_kernel runs, on
//     the host;
//   * solve_nlp on the CPU oracle with the dense host factorisation for one quadrotor instance under the device's rule set --
//     inertia search and stagnation rule off, the second-order correction by a switch, crawl_limit and crawl_frac as given: what
//     tests/golden/gen_lockstep_rescue_cases.py records.
// Linked into libetol_harness.so.  Test infrastructure.
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")     // the rules are compared bit for bit: no fused multiply-adds on a host that has them
#endif
#include <dlfcn.h>

#include <algorithm>
#include <string>
#include <vector>

#include "emi355x.h"
#include "emi_ipm_control.hpp"
#include "emi_nlp.hpp"

namespace mx = ETOL::mi355x;

namespace {

// the state record as tests/lockstep_ref.py passes it (SD, SI), the rescue record as tests/lockstep_rescue_ref.py does (RI, err_mu)
enum { D_MU, D_RHO, D_TAU, D_NU, D_EMAX_REF, D_ERR0, D_VIOL, D_EMAX, D_PHI0, D_SLOPE, D_ALPHA, D_ADU, ND };
enum { I_NACC, I_FUTILE, I_ITER, I_STATUS, I_FM, I_ESC, I_SEARCHING, I_ACCEPTED, I_PASSES, I_EVALS, NI };
enum { R_CRAWL, R_CANDIDATE, R_NEWTON, R_RESTORED, NR };

emi::IpmCtlState state_of(const double* d, const int* i) {
    emi::IpmCtlState s;
    s.mu = d[D_MU]; s.rho = d[D_RHO]; s.tau = d[D_TAU]; s.nu = d[D_NU]; s.emax_ref = d[D_EMAX_REF]; s.err0 = d[D_ERR0]; s.viol = d[D_VIOL];
    s.emax = d[D_EMAX]; s.phi0 = d[D_PHI0]; s.slope = d[D_SLOPE]; s.alpha = d[D_ALPHA]; s.adu = d[D_ADU];
    s.n_acceptable = i[I_NACC]; s.futile = i[I_FUTILE]; s.iterations = i[I_ITER]; s.status = i[I_STATUS]; s.force_modified = i[I_FM];
    s.escalated = i[I_ESC]; s.searching = i[I_SEARCHING]; s.accepted = i[I_ACCEPTED]; s.passes = i[I_PASSES]; s.evaluations = i[I_EVALS];
    return s;
}
void state_to(const emi::IpmCtlState& s, double* d, int* i) {
    d[D_MU] = s.mu; d[D_RHO] = s.rho; d[D_TAU] = s.tau; d[D_NU] = s.nu; d[D_EMAX_REF] = s.emax_ref; d[D_ERR0] = s.err0; d[D_VIOL] = s.viol;
    d[D_EMAX] = s.emax; d[D_PHI0] = s.phi0; d[D_SLOPE] = s.slope; d[D_ALPHA] = s.alpha; d[D_ADU] = s.adu;
    i[I_NACC] = s.n_acceptable; i[I_FUTILE] = s.futile; i[I_ITER] = s.iterations; i[I_STATUS] = s.status; i[I_FM] = s.force_modified;
    i[I_ESC] = s.escalated; i[I_SEARCHING] = s.searching; i[I_ACCEPTED] = s.accepted; i[I_PASSES] = s.passes; i[I_EVALS] = s.evaluations;
}
emi::IpmCtlRescue rescue_of(const int* ri, double err_mu) {
    emi::IpmCtlRescue r;
    r.crawl = ri[R_CRAWL]; r.candidate = ri[R_CANDIDATE]; r.newton_steps = ri[R_NEWTON]; r.restored_steps = ri[R_RESTORED]; r.err_mu = err_mu;
    return r;
}
void rescue_to(const emi::IpmCtlRescue& r, int* ri, double* err_mu) {
    ri[R_CRAWL] = r.crawl; ri[R_CANDIDATE] = r.candidate; ri[R_NEWTON] = r.newton_steps; ri[R_RESTORED] = r.restored_steps; *err_mu = r.err_mu;
}
// the rule's options: the fields the rule functions read; the rest as a record built without the rule has them
emi::IpmCtlOptions options_of(int rules, int crawl_limit, double crawl_frac) {
    emi::IpmCtlOptions o{1e-8, 100.0, 200, 10, 3, 1};
    o.rules = rules; o.crawl_limit = crawl_limit; o.crawl_frac = crawl_frac;
    return o;
}

typedef int (*orc_eval_t)(int, const double*, int, int, int, const double*, const double*, const double*, double, double, int, int,
                          const double*, int, int, int, int, const double*, const double*, const double*, const double*, double*, double*,
                          double*);
typedef int (*orc_hess_t)(int, const double*, int, int, int, const double*, double, double, int, int, const double*, int, int, int, int,
                          const double*, const double*, const double*, const double*, const double*, const double*, double, double*);

struct OracleQuadR : public mx::NlpEvaluator {
    orc_eval_t ev = nullptr;
    orc_hess_t hs = nullptr;
    std::vector<double> params, tau, w, D, recs;
    int M = 0, np = 0;
    double tf = 0;
    int eval(const double* X, const double* U, double* RES, double* VALS, double* COST, bool jac) override {
        return ev(EMI_MODEL_QUADROTOR2D, params.data(), 0, M, 1, tau.data(), w.data(), D.data(), 0.0, tf, np, 1, recs.data(), 0, 1, 0, 1, nullptr,
                  nullptr, X, U, RES, jac ? VALS : nullptr, COST);
    }
    int hess(const double* X, const double* U, const double* lamF, const double* lamC, double sigma, double* H) override {
        return hs(EMI_MODEL_QUADROTOR2D, params.data(), 0, M, 1, w.data(), 0.0, tf, np, 1, recs.data(), 0, 1, 0, 1, nullptr, nullptr, X, U, lamF,
                  lamC, sigma, H);
    }
};

}  // namespace

extern "C" {

int harness_rescue_sizes(int* nd, int* ni, int* nr) { *nd = ND; *ni = NI; *nr = NR; return EMI_IPM_RULE_RESIDUAL; }

// each returns what the function returns (select: the candidate flag); sd / si are written back by decide only (the others take
// the state const)
int harness_rescue_select(const double* parts, const double* sd, const int* si, int* ri, double* err_mu, int rules, int crawl_limit,
                          double crawl_frac) {
    const emi::IpmCtlState s = state_of(sd, si);
    emi::IpmCtlRescue r = rescue_of(ri, *err_mu);
    emi::ipm_ctl_rescue_select(parts, s, r, options_of(rules, crawl_limit, crawl_frac));
    rescue_to(r, ri, err_mu);
    return r.candidate;
}

int harness_rescue_decide(const double* parts, double* sd, int* si, int* ri, double* err_mu) {
    emi::IpmCtlState s = state_of(sd, si);
    emi::IpmCtlRescue r = rescue_of(ri, *err_mu);
    const bool stands = emi::ipm_ctl_rescue_decide(parts, s, r);
    state_to(s, sd, si);
    rescue_to(r, ri, err_mu);
    return stands ? 1 : 0;
}

void harness_rescue_crawl(const double* scal, const double* sd, const int* si, int* ri, double* err_mu, int rules, int crawl_limit,
                          double crawl_frac) {
    const emi::IpmCtlState s = state_of(sd, si);
    emi::IpmCtlRescue r = rescue_of(ri, *err_mu);
    emi::ipm_ctl_rescue_crawl(scal, s, r, options_of(rules, crawl_limit, crawl_frac));
    rescue_to(r, ri, err_mu);
}

// One quadrotor instance through solve_nlp as harness_lockstep_solve_oracle runs it, under the lock-step driver's rule set:
// inertia search and stagnation rule off, the second-order correction on only where soc != 0, crawl_limit / crawl_frac as given
// (a crawl_limit beyond max_iter leaves the err0 <= 1e-2 branch of the residual-based acceptance only).
// out_d = {cost, rho, kkt_error, constr_viol}, out_i = {ok, iterations, evaluations, newton_steps, restored_steps, locally
// infeasible, iteration limit}.  Returns 0 when solve_nlp ran (whatever it reports).
int harness_rescue_solve_oracle(const char* oracle_so, int M, double tf, const double* params, int np, const double* recs,
                                const double* cscale, const double* zl, const double* zu, const double* z0, double tol, int max_iter,
                                int crawl_limit, double crawl_frac, int soc, double* out_d, int* out_i) {
    void* h = dlopen(oracle_so, RTLD_NOW);
    if (!h) return 3;
    OracleQuadR oe;
    oe.ev = (orc_eval_t)dlsym(h, "orc_eval");
    oe.hs = (orc_hess_t)dlsym(h, "orc_hess");
    if (!oe.ev || !oe.hs) { dlclose(h); return 3; }
    oe.params.assign(params, params + 5);
    oe.M = M; oe.np = np; oe.tf = tf;
    oe.tau.resize(M); oe.w.resize(M); oe.D.resize((size_t)M * M);
    emi_lgl(M, oe.tau.data(), oe.w.data(), oe.D.data());
    oe.recs.assign(recs, recs + (size_t)np * EMI_PATH_REC);
    const int nz = 8 * M;
    mx::NlpProblem P;
    P.ns = 6; P.nc = 2; P.np = np; P.M = M; P.px = 0; P.py = 1;
    P.D = oe.D;
    P.zl.assign(zl, zl + nz); P.zu.assign(zu, zu + nz);
    P.cl.assign(np, -1000.0); P.cu.assign(np, 0.0);
    P.cscale.assign(cscale, cscale + np);
    P.ev = &oe;
    mx::NlpOptions opt;
    opt.tol = tol; opt.max_iter = max_iter;
    opt.max_shift_trials = 0; opt.stagnation_iters = 1 << 30;
    opt.second_order_correction = soc != 0;
    opt.crawl_limit = crawl_limit; opt.crawl_frac = crawl_frac;
    const mx::NlpResult r = mx::solve_nlp(P, opt, std::vector<double>(z0, z0 + nz));
    out_d[0] = r.cost; out_d[1] = r.rho; out_d[2] = r.kkt_error; out_d[3] = r.constr_viol;
    out_i[0] = r.ok ? 1 : 0; out_i[1] = r.iterations; out_i[2] = r.evaluations; out_i[3] = r.newton_steps; out_i[4] = r.restored_steps;
    out_i[5] = r.msg.find("locally infeasible") != std::string::npos ? 1 : 0;
    out_i[6] = r.msg.find("maximum number of iterations") != std::string::npos ? 1 : 0;
    dlclose(h);
    return 0;
}

}  // extern "C"
