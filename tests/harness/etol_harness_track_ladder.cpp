// etol_harness_track_ladder.cpp -- extern "C" shim for the tests of the mesh ladder with moving-disc rows (emi_ipm_solve_ladder_*
// over waypoint tables, emi_set_track_waypoints): harness_ladder_solve_oracle of etol_harness_ladder.cpp with a track table.
// solve_nlp on the CPU oracle with the dense host factorisation for one quadrotor instance on a mesh of any size, the record table
// holding rows of kind EMI_PATH_TRACK whose centres at this rung's nodes the caller supplies; they reach the oracle the way
// etol_harness.cpp's OracleEval passes a Prob's tracks.  What tests/golden/gen_track_ladder_cases.py records per rung.
// Linked into libetol_harness.so.  Test infrastructure.
#include <dlfcn.h>

#include <algorithm>
#include <vector>

#include "ETOL/eMI355X.hpp"
#include "emi355x.h"
#include "emi_nlp.hpp"

namespace mx = ETOL::mi355x;

namespace {

typedef int (*orc_eval_t)(int, const double*, int, int, int, const double*, const double*, const double*, double, double, int, int,
                          const double*, int, int, int, int, const double*, const double*, const double*, const double*, double*, double*,
                          double*);
typedef int (*orc_hess_t)(int, const double*, int, int, int, const double*, double, double, int, int, const double*, int, int, int, int,
                          const double*, const double*, const double*, const double*, const double*, const double*, double, double*);

struct OracleQuadT : public mx::NlpEvaluator {
    orc_eval_t ev = nullptr;
    orc_hess_t hs = nullptr;
    std::vector<double> params, tau, w, D, recs, trkx, trky;
    int M = 0, np = 0, ntracks = 0;
    double tf = 0;
    int eval(const double* X, const double* U, double* RES, double* VALS, double* COST, bool jac) override {
        return ev(EMI_MODEL_QUADROTOR2D, params.data(), 0, M, 1, tau.data(), w.data(), D.data(), 0.0, tf, np, 1, recs.data(), 0, 1, ntracks, 1,
                  trkx.data(), trky.data(), X, U, RES, jac ? VALS : nullptr, COST);
    }
    int hess(const double* X, const double* U, const double* lamF, const double* lamC, double sigma, double* H) override {
        return hs(EMI_MODEL_QUADROTOR2D, params.data(), 0, M, 1, w.data(), 0.0, tf, np, 1, recs.data(), 0, 1, ntracks, 1, trkx.data(),
                  trky.data(), X, U, lamF, lamC, sigma, H);
    }
};

}  // namespace

extern "C" {

// As harness_ladder_solve_oracle; trkx, trky [ntracks][M]: the centres of the tracks at the M nodes of this rung (a record of kind
// EMI_PATH_TRACK names its track in field 1).  out_d = {cost, rho, kkt_error, constr_viol}, out_i = {ok, iterations, evaluations}.
int harness_track_ladder_solve_oracle(const char* oracle_so, int M, double tf, const double* params, int np, const double* recs, int ntracks,
                                      const double* trkx, const double* trky, const double* cscale, const double* zl, const double* zu,
                                      const double* z0, double tol, int max_iter, int reduced, double* out_d, int* out_i, double* z) {
    if (ntracks < 0 || (ntracks > 0 && (!trkx || !trky))) return 2;
    for (int j = 0; j < np; ++j) {
        const double* r = recs + (size_t)j * EMI_PATH_REC;
        if ((int)r[0] == EMI_PATH_TRACK && !(r[1] >= 0 && r[1] < ntracks)) return 2;
    }
    void* h = dlopen(oracle_so, RTLD_NOW);
    if (!h) return 3;
    OracleQuadT oe;
    oe.ev = (orc_eval_t)dlsym(h, "orc_eval");
    oe.hs = (orc_hess_t)dlsym(h, "orc_hess");
    if (!oe.ev || !oe.hs) { dlclose(h); return 3; }
    oe.params.assign(params, params + 5);
    oe.M = M; oe.np = np; oe.tf = tf; oe.ntracks = ntracks;
    oe.tau.resize(M); oe.w.resize(M); oe.D.resize((size_t)M * M);
    emi_lgl(M, oe.tau.data(), oe.w.data(), oe.D.data());
    oe.recs.assign(recs, recs + (size_t)np * EMI_PATH_REC);
    if (ntracks > 0) {
        oe.trkx.assign(trkx, trkx + (size_t)ntracks * M);
        oe.trky.assign(trky, trky + (size_t)ntracks * M);
    }
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
