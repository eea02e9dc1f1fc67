// etol_harness_ladder.cpp -- extern "C" shim for the tests of the mesh ladder over the lock-step solve (emi_ipm_solve_ladder_*):
//   * ETOL::mi355x::repair_guess (host/eMI355X.cpp) on plain arrays: what emi_repair_guess_kernel restates per node;
//   * solve_nlp on the CPU oracle with the dense host factorisation for one quadrotor instance on a mesh of any size, with the
//     rules solve_nlp can switch off switched off (inertia search, crawl rule, stagnation rule): what
//     tests/golden/gen_ladder_cases.py records per rung.
// Linked into libetol_harness.so.  Test infrastructure.
#include <dlfcn.h>

#include <algorithm>
#include <vector>

#include "ETOL/eMI355X.hpp"
#include "emi355x.h"
#include "emi_nlp.hpp"

namespace ETOL {
namespace mi355x {
void repair_guess(const Prob& P, double* xs, double* ys);
}
}  // namespace ETOL

namespace mx = ETOL::mi355x;

namespace {

typedef int (*orc_eval_t)(int, const double*, int, int, int, const double*, const double*, const double*, double, double, int, int,
                          const double*, int, int, int, int, const double*, const double*, const double*, const double*, double*, double*,
                          double*);
typedef int (*orc_hess_t)(int, const double*, int, int, int, const double*, double, double, int, int, const double*, int, int, int, int,
                          const double*, const double*, const double*, const double*, const double*, const double*, double, double*);

struct OracleQuadL : public mx::NlpEvaluator {
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

// xs, ys [M] in place; recs [np][8]; trkx, trky [ntracks][M] (may be null without track rows)
void harness_repair_guess(int M, int np, const double* recs, int ntracks, const double* trkx, const double* trky, double* xs, double* ys) {
    mx::Prob P;
    P.nodes = (size_t)M;
    P.npath = (size_t)np;
    P.npath_traced = 0;
    P.path_records.assign(recs, recs + (size_t)np * EMI_PATH_REC);
    P.ntracks = (size_t)ntracks;
    if (ntracks > 0) {
        P.track_x.assign(trkx, trkx + (size_t)ntracks * M);
        P.track_y.assign(trky, trky + (size_t)ntracks * M);
    }
    mx::repair_guess(P, xs, ys);
}

// As harness_lockstep_solve_oracle, with reduced != 0: inertia search, crawl rule and stagnation rule off (the rules of solve_nlp
// the lock-step driver leaves out, as far as NlpOptions can switch them off: the second-order correction and the residual-based
// acceptance have no switch).  out_d = {cost, rho, kkt_error, constr_viol}, out_i = {ok, iterations, evaluations}.
int harness_ladder_solve_oracle(const char* oracle_so, int M, double tf, const double* params, int np, const double* recs,
                                const double* cscale, const double* zl, const double* zu, const double* z0, double tol, int max_iter,
                                int reduced, double* out_d, int* out_i, double* z) {
    void* h = dlopen(oracle_so, RTLD_NOW);
    if (!h) return 3;
    OracleQuadL oe;
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
    if (reduced) { opt.max_shift_trials = 0; opt.crawl_limit = 1 << 30; opt.stagnation_iters = 1 << 30; }
    const mx::NlpResult r = mx::solve_nlp(P, opt, std::vector<double>(z0, z0 + nz));
    out_d[0] = r.cost; out_d[1] = r.rho; out_d[2] = r.kkt_error; out_d[3] = r.constr_viol;
    out_i[0] = r.ok ? 1 : 0; out_i[1] = r.iterations; out_i[2] = r.evaluations;
    if (z && (int)r.z.size() == nz) std::copy(r.z.begin(), r.z.end(), z);
    dlclose(h);
    return 0;
}

}  // extern "C"
