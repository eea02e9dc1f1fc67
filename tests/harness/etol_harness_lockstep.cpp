// etol_harness_lockstep.cpp -- extern "C" shim for the tests of the lock-step interior-point driver (emi_ipm_solve_shard_*):
//   * the scalar control rules of csrc/emi_ipm_control.hpp, the text the control kernels run, on the host;
//   * solve_nlp on the CPU oracle with the dense host factorisation for one quadrotor instance given by its bounds, discs, row
//     scales and start: what tests/golden/gen_lockstep_cases.py records as the fixture.
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

// the state record as two flat arrays (tests/lockstep_ref.py: SD, SI)
enum { D_MU, D_RHO, D_TAU, D_NU, D_EMAX_REF, D_ERR0, D_VIOL, D_EMAX, D_PHI0, D_SLOPE, D_ALPHA, D_ADU, ND };
enum { I_NACC, I_FUTILE, I_ITER, I_STATUS, I_FM, I_ESC, I_SEARCHING, I_ACCEPTED, I_PASSES, I_EVALS, NI };

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
// od = {tol, acceptable_factor}, oi = {max_iter, acceptable_iter, max_futile_escalations, has_rows}
emi::IpmCtlOptions options_of(const double* od, const int* oi) { return emi::IpmCtlOptions{od[0], od[1], oi[0], oi[1], oi[2], oi[3]}; }

typedef int (*orc_eval_t)(int, const double*, int, int, int, const double*, const double*, const double*, double, double, int, int,
                          const double*, int, int, int, int, const double*, const double*, const double*, const double*, double*, double*,
                          double*);
typedef int (*orc_hess_t)(int, const double*, int, int, int, const double*, double, double, int, int, const double*, int, int, int, int,
                          const double*, const double*, const double*, const double*, const double*, const double*, double, double*);

struct OracleQuad : public mx::NlpEvaluator {
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

int harness_ctl_sizes(int* nd, int* ni, int* nparts) { *nd = ND; *ni = NI; *nparts = emi::IPM_NPARTS; return emi::IPM_RUNNING; }

void harness_ctl_start(double mu_init, double rho_init, double* sd, int* si) {
    emi::IpmCtlState s;
    emi::ipm_ctl_start(s, mu_init, rho_init);
    state_to(s, sd, si);
}

double harness_ctl_kkt(const double* parts, double mu_t) { return emi::ipm_ctl_kkt(parts, mu_t); }

double harness_ctl_raise_dc(double dc, double mu) { return emi::ipm_ctl_raise_dc(dc, mu); }

void harness_ctl_barrier(const double* parts, double* sd, int* si, const double* od, const int* oi) {
    emi::IpmCtlState s = state_of(sd, si);
    emi::ipm_ctl_barrier(parts, s, options_of(od, oi));
    state_to(s, sd, si);
}

void harness_ctl_search_init(const double* scal, const double* mer, int factor_failed, double* sd, int* si) {
    emi::IpmCtlState s = state_of(sd, si);
    emi::ipm_ctl_search_init(scal, mer, factor_failed, s);
    state_to(s, sd, si);
}

void harness_ctl_search_step(const double* mer, int exact_with_mods, double* sd, int* si, const double* od, const int* oi) {
    emi::IpmCtlState s = state_of(sd, si);
    emi::ipm_ctl_search_step(mer, exact_with_mods, s, options_of(od, oi));
    state_to(s, sd, si);
}

// One quadrotor instance through solve_nlp: oracle evaluator, dense host factorisation, default options but tol and max_iter.
// recs [np][8] path records, cscale [np], zl / zu / z0 [(6 + 2) M].  out_d = {cost, rho, kkt_error, constr_viol}, out_i = {ok,
// iterations, evaluations}; z (may be null) receives the solution.  Returns 0 when solve_nlp ran (whatever it reports).
int harness_lockstep_solve_oracle(const char* oracle_so, int M, double tf, const double* params, int np, const double* recs,
                                  const double* cscale, const double* zl, const double* zu, const double* z0, double tol, int max_iter,
                                  double* out_d, int* out_i, double* z) {
    void* h = dlopen(oracle_so, RTLD_NOW);
    if (!h) return 3;
    OracleQuad oe;
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
    const mx::NlpResult r = mx::solve_nlp(P, opt, std::vector<double>(z0, z0 + nz));
    out_d[0] = r.cost; out_d[1] = r.rho; out_d[2] = r.kkt_error; out_d[3] = r.constr_viol;
    out_i[0] = r.ok ? 1 : 0; out_i[1] = r.iterations; out_i[2] = r.evaluations;
    if (z && (int)r.z.size() == nz) std::copy(r.z.begin(), r.z.end(), z);
    dlclose(h);
    return 0;
}

}  // extern "C"
