// etol_harness_delay_ode_error.cpp -- extern "C" shim over ETOL::eMI355X for the ODE-error tests of DELAYED problems: the delayed
// problem of etol_harness.cpp (configure_delay_demo: same functions and numbers, model 3 of oracle/emi_oracle.c, no keep-out) with
// odeError() on a given trajectory, on either setting of Alg::ode_error, and solved with the default Alg, reporting Sol::ode_error
// beside the mesh the solve ended on.  Linked into libetol_harness.so.  Test infrastructure.
#include <ETOL/eMI355X.hpp>

#include <dlfcn.h>

#include <algorithm>
#include <any>
#include <cmath>
#include <string>
#include <vector>

#include "emi355x.h"
#include "emi_nlp.hpp"
#include "emi_transcribe.hpp"

namespace mx = ETOL::mi355x;

namespace {

// the NLP iteration's evaluator on the CPU oracle (as in etol_harness.cpp; fixtures and solver-logic tests only, never the product path)
typedef int (*orc_eval_t)(int, const double*, int, int, int, const double*, const double*, const double*, double, double,
                          int, int, const double*, int, int, int, int, const double*, const double*, const double*,
                          const double*, double*, double*, double*);
typedef int (*orc_hess_t)(int, const double*, int, int, int, const double*, double, double, int, int, const double*, int,
                          int, int, int, const double*, const double*, const double*, const double*, const double*,
                          const double*, double, double*);
struct OracleEval : public mx::NlpEvaluator {
    const mx::Prob* P = nullptr;
    orc_eval_t ev = nullptr;
    orc_hess_t hs = nullptr;
    int eval(const double* X, const double* U, double* RES, double* VALS, double* COST, bool jac) override {
        return ev(P->model, P->model_params.data(), 0, (int)P->nodes, 1, P->tau.data(), P->w.data(), P->D.data(), P->t0,
                  P->tf, (int)P->npath, 1, P->path_records.data(), (int)P->px, (int)P->py, (int)P->ntracks, 1,
                  P->track_x.data(), P->track_y.data(), X, U, RES, jac ? VALS : nullptr, COST);
    }
    int hess(const double* X, const double* U, const double* lamF, const double* lamC, double sigma, double* H) override {
        return hs(P->model, P->model_params.data(), 0, (int)P->nodes, 1, P->w.data(), P->t0, P->tf, (int)P->npath, 1,
                  P->path_records.data(), (int)P->px, (int)P->py, (int)P->ntracks, 1, P->track_x.data(),
                  P->track_y.data(), X, U, lamF, lamC, sigma, H);
    }
};

struct Demo {           // owns the callbacks: the optimiser keeps raw f_t pointers
    ETOL::f_t obj, f0, f1;
};
std::string g_msg;

// x = [x0 x1 | x(t-dt) | x(t-2dt)], u = [u0 u1 | u(t-dt)]  (reference ePSOPT.cpp:225-248)
void configure(ETOL::TrajectoryOptimizer* t, Demo& d, int nsteps, double dt, int xh, int uh) {
    t->setNSteps(nsteps); t->setDt(dt); t->setNStates(2); t->setNControls(2);
    t->setXrhorizon(xh); t->setUrhorizon(uh);
    t->setX0({1, 2}); t->setXf({3, 1}); t->setXtol({0.01, 0.01});
    t->setXlower({-10, -10}); t->setXupper({10, 10}); t->setUlower({-5, -5}); t->setUupper({5, 5});
    t->setMaximize(false);
    const double p0 = 0.7, p1 = 0.3;
    auto V = [](const std::any& a) { return std::any_cast<mx::Var>(a); };
    d.obj = [=](F_ARGS) -> ETOL::scalar_t {
        return V(u.at(0)) * V(u.at(0)) + V(u.at(1)) * V(u.at(1)) + p1 * V(x.at(2)) * V(x.at(4)) + 0.05 * V(u.at(2)) * V(u.at(2));
    };
    d.f0 = [=](F_ARGS) -> ETOL::scalar_t { return -p0 * V(x.at(2)) + V(u.at(0)) + 0.1 * V(u.at(3)) * V(x.at(1)); };
    d.f1 = [=](F_ARGS) -> ETOL::scalar_t { return V(x.at(0)) * V(x.at(5)) - mx::sin(V(x.at(3))) + V(u.at(1)) * V(u.at(2)); };
    t->setObjective(&d.obj);
    t->setGradient({&d.f0, &d.f1});
}

// what a reference needs of the problem: nodes, ndelayed, t0, tf, delay_dt, lifted
void put_dims(const mx::Prob* P, double* dims6) {
    dims6[0] = (double)P->nodes; dims6[1] = (double)P->ndelayed; dims6[2] = P->t0; dims6[3] = P->tf; dims6[4] = P->delay_dt;
    dims6[5] = P->lifted ? 1.0 : 0.0;
}

}  // namespace

extern "C" {

const char* harness_doe_message(void) { return g_msg.c_str(); }

// odeError(z = [X (2 x M) | U (2 x M)]) of the delayed problem on nsteps + 1 nodes, Alg::ode_error = "device" (device_route != 0)
// or "host"; tau [M] of the mesh the class is on
int harness_doe_ode_error(int nsteps, double dt, int xh, int uh, int device_route, const double* z, double* err, double* dims6, double* tau) {
    ETOL::eMI355X solver;
    ETOL::TrajectoryOptimizer* t = &solver;
    Demo d;
    configure(t, d, nsteps, dt, xh, uh);
    t->setup();
    solver.getAlgorithm()->ode_error = device_route ? "device" : "host";
    const mx::Prob* P = solver.getProblem();
    const size_t M = P->nodes;
    if (M != (size_t)nsteps + 1) { g_msg = "unexpected mesh"; t->close(); return 2; }
    *err = solver.odeError(std::vector<double>(z, z + 4 * M));
    put_dims(P, dims6);
    for (size_t k = 0; k < M; ++k) tau[k] = P->tau[k];
    t->close();
    return 0;
}

// solve() with the default Alg (print_level as given) and, where refine != 0, Alg::refine_delayed with ode_tolerance = ode_tol,
// mr_max_nodes = max_nodes (<= 0: the default), nlp_tolerance = nlp_tol, nlp_iter_max 400 and the certificate.
// stats14: nodes, mesh_iterations, ode_error, cost, nlp_iterations_total, largest defect of evaluate() at the solution on the stated
// problem, nlp_runs, error_flag, certificate stationarity / complementarity / defect / computed, mean |multiplier| over lamF and
// lamC, acceptable_factor * nlp_tolerance.  X, U [2][cap_nodes]
int harness_doe_solve(int nsteps, double dt, int xh, int uh, int print_level, int refine, double ode_tol, int max_nodes, double nlp_tol,
                      double* stats14, double* dims6, double* X, double* U, double* tau, int cap_nodes) {
    ETOL::eMI355X solver;
    ETOL::TrajectoryOptimizer* t = &solver;
    Demo d;
    configure(t, d, nsteps, dt, xh, uh);
    t->setup();
    mx::Alg* a = solver.getAlgorithm();
    a->print_level = print_level;
    if (refine) {
        a->refine_delayed = true;
        a->ode_tolerance = ode_tol;
        if (max_nodes > 0) a->mr_max_nodes = max_nodes;
        a->nlp_tolerance = nlp_tol;
        a->nlp_iter_max = 400;
        a->certify = true;
    }
    t->solve();
    const mx::Sol* s = solver.getSolution();
    const mx::Prob* P = solver.getProblem();
    g_msg = s->error_msg;
    if (s->error_flag) { t->close(); return 1; }
    const size_t M = s->nodes;
    if ((int)M > cap_nodes || s->states.size() != 2 * M || s->controls.size() != 2 * M) { g_msg = "unexpected sizes"; t->close(); return 2; }
    std::vector<double> zz(4 * M), r, v;
    for (size_t q = 0; q < 2 * M; ++q) { X[q] = zz[q] = s->states[q]; U[q] = zz[2 * M + q] = s->controls[q]; }
    double c2 = 0, dm = 0;
    solver.evaluate(zz, &r, &v, &c2);
    for (size_t q = 0; q < 2 * M; ++q) dm = std::max(dm, std::fabs(r[q]));
    double msum = 0;
    for (double v : s->lamF) msum += std::fabs(v);
    for (double v : s->lamC) msum += std::fabs(v);
    const size_t nmult = s->lamF.size() + s->lamC.size();
    double* st = stats14;
    st[0] = (double)M; st[1] = (double)s->mesh_iterations; st[2] = s->ode_error; st[3] = s->cost;
    st[4] = (double)s->nlp_iterations_total; st[5] = dm; st[6] = (double)s->nlp_runs.size(); st[7] = (double)s->error_flag;
    st[8] = s->certificate.stationarity; st[9] = s->certificate.complementarity; st[10] = s->certificate.defect;
    st[11] = s->certificate.computed ? 1.0 : 0.0; st[12] = nmult ? msum / (double)nmult : 0.0;
    st[13] = mx::NlpOptions().acceptable_factor * a->nlp_tolerance;
    put_dims(P, dims6);
    for (size_t k = 0; k < M; ++k) tau[k] = P->tau[k];
    t->close();
    return 0;
}

// The same problem LIFTED and solved on the CPU oracle (model 3 of oracle/emi_oracle.c, dense host step) on an LGL mesh of `nodes`
// nodes over [0, tf] with the physical delay delay_dt: what tests/golden/gen_delay_refine_cases.py solves on every mesh the growth
// rule visits.  No device.  Z out: [X (2 x M) | U (2 x M) | delayed (6 x M)].
int harness_doe_solve_oracle(const char* oracle_so, int nodes, double tf, double delay_dt, double tol, double* cost, double* Z, int* iters) {
    void* h = dlopen(oracle_so, RTLD_NOW);
    if (!h) { g_msg = dlerror(); return 3; }
    OracleEval oe;
    oe.ev = (orc_eval_t)dlsym(h, "orc_eval");
    oe.hs = (orc_hess_t)dlsym(h, "orc_hess");
    if (!oe.ev || !oe.hs) { g_msg = "the oracle has no orc_eval / orc_hess"; dlclose(h); return 3; }
    mx::Prob P;
    P.nstates = 2; P.ncontrols = 2; P.xhorizon = 3; P.uhorizon = 1; P.ndelayed = 6; P.delay_dt = delay_dt; P.lifted = true;
    P.nodes = (size_t)nodes; P.t0 = 0; P.tf = tf;
    P.model = 3;
    P.model_params = {0.7, 0.3};
    P.tau.resize(P.nodes); P.w.resize(P.nodes); P.D.resize(P.nodes * P.nodes);
    emi_lgl((int)P.nodes, P.tau.data(), P.w.data(), P.D.data());
    P.npath = 0;
    P.px = 0; P.py = 1;
    P.state_lower = {-10, -10}; P.state_upper = {10, 10}; P.control_lower = {-5, -5}; P.control_upper = {5, 5};
    P.event_lower = {1, 2, 3 - 0.01, 1 - 0.01}; P.event_upper = {1, 2, 3 + 0.01, 1 + 0.01};
    oe.P = &P;
    mx::NlpProblem nlp = mx::make_nlp(P, &oe);
    mx::NlpOptions opt;
    opt.tol = tol; opt.print_level = 0; opt.max_iter = 400;
    mx::NlpResult r = mx::solve_nlp(nlp, opt, mx::initial_guess(P));
    *iters = r.iterations;
    g_msg = r.msg;
    if (!r.ok) { dlclose(h); return 1; }
    *cost = r.cost;
    std::copy(r.z.begin(), r.z.end(), Z);
    dlclose(h);
    return 0;
}

}  // extern "C"
