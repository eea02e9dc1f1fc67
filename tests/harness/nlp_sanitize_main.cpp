// nlp_sanitize_main.cpp -- stand-alone run of mi355x::solve_nlp (etol_amd/host/emi_nlp.cpp) under the host sanitizers
// (`make check-nlp`): no Python, no device.  The iteration keeps its state in member arrays and reads them through views
// of raw pointers; its second-order correction and its residual-based acceptance copy whole steps / iterates and take them
// back.  This program drives those paths on a point-mass problem (x' = u, min int |u|^2, one disc keep-out) and, for the
// strongly curved rows the corrections need, on the 6-state quadrotor with the same kind of keep-out, each of 17 LGL nodes,
// with the CPU oracle (oracle/emi_oracle.c) as evaluator and the dense host factorisation.
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "emi355x.h"
#include "emi_nlp.hpp"

extern "C" {
int orc_eval(int model, const double* params, int maximize, int M, int B, const double* tau, const double* w, const double* D, double t0,
             double tf, int np, int path_sets, const double* recs, int px, int py, int ntracks, int track_sets, const double* trkx,
             const double* trky, const double* X, const double* U, double* RES, double* VALS, double* COST);
int orc_hess(int model, const double* params, int maximize, int M, int B, const double* w, double t0, double tf, int np, int path_sets,
             const double* recs, int px, int py, int ntracks, int track_sets, const double* trkx, const double* trky, const double* X,
             const double* U, const double* LamF, const double* LamC, double sigma, double* H);
}

namespace mx = ETOL::mi355x;

namespace {

constexpr int M = 17;
constexpr double TF = 8.0;

// a model of the oracle with one disc keep-out on its first two states: value r^2 - |p - c|^2 <= 0 outside
struct OracleModel : public mx::NlpEvaluator {
    int model;
    double tf;
    std::vector<double> params, tau = std::vector<double>(M), w = std::vector<double>(M), D = std::vector<double>(M * M);
    double disc[8];
    OracleModel(int model_, double tf_, std::vector<double> params_, double cx, double cy, double r)
        : model(model_), tf(tf_), params(std::move(params_)), disc{1 /* disc */, cx, cy, r * r, 0, 0, 0, 0} {
        emi_lgl(M, tau.data(), w.data(), D.data());
    }
    int eval(const double* X, const double* U, double* RES, double* VALS, double* COST, bool jac) override {
        return orc_eval(model, params.data(), 0, M, 1, tau.data(), w.data(), D.data(), 0.0, tf, 1, 1, disc, 0, 1, 0, 1, nullptr, nullptr, X, U, RES,
                        jac ? VALS : nullptr, COST);
    }
    int hess(const double* X, const double* U, const double* lamF, const double* lamC, double sigma, double* H) override {
        return orc_hess(model, params.data(), 0, M, 1, w.data(), 0.0, tf, 1, 1, disc, 0, 1, 0, 1, nullptr, nullptr, X, U, lamF, lamC, sigma, H);
    }
};
struct PointMass : public OracleModel {
    PointMass() : OracleModel(0, TF, {}, 2.0, 0.0, 0.5) {}
};

// the quadrotor (x, z, theta and their rates; thrust, torque) from rest at (1, 1) to rest at (8, 6) in 2.5 s, the disc on the way;
// the start is the straight line at hover thrust, which crosses the disc
mx::NlpProblem quadrotor_problem(OracleModel& ev, std::vector<double>* z0) {
    const double lo[8] = {0, 0, -1.2, -6, -6, -4, 0, -1}, hi[8] = {10, 10, 1.2, 6, 6, 4, 25, 1};
    const double x0[6] = {1, 1, 0, 0, 0, 0}, xf[6] = {8, 6, 0, 0, 0, 0}, xtol[6] = {0.01, 0.01, 0.01, 0.05, 0.05, 0.05};
    mx::NlpProblem P;
    P.ns = 6; P.nc = 2; P.np = 1; P.M = M;
    P.D = ev.D;
    P.zl.resize(8 * M);
    P.zu.resize(8 * M);
    z0->assign(8 * M, 0.0);
    for (int v = 0; v < 8; ++v)
        for (int k = 0; k < M; ++k) { P.zl[v * M + k] = lo[v]; P.zu[v * M + k] = hi[v]; }
    for (int i = 0; i < 6; ++i) {
        P.zl[i * M] = P.zu[i * M] = x0[i];
        P.zl[i * M + M - 1] = xf[i] - xtol[i];
        P.zu[i * M + M - 1] = xf[i] + xtol[i];
    }
    for (int k = 0; k < M; ++k) {
        const double s = 0.5 * (ev.tau[k] + 1.0);
        (*z0)[k] = 1 + 7 * s;
        (*z0)[M + k] = 1 + 5 * s;
        (*z0)[6 * M + k] = 9.81;
    }
    P.cl = {-1e20};
    P.cu = {0.0};
    P.ev = &ev;
    return P;
}

// from (0, 0) to within 0.01 of (xe, ye); states in [-10, 10], controls in [-2, 2]
mx::NlpProblem problem(PointMass& ev, double xe, double ye) {
    mx::NlpProblem P;
    P.ns = 2; P.nc = 2; P.np = 1; P.M = M;
    P.D = ev.D;
    P.zl.assign(4 * M, -10.0);
    P.zu.assign(4 * M, 10.0);
    for (int k = 0; k < M; ++k) { P.zl[2 * M + k] = P.zl[3 * M + k] = -2.0; P.zu[2 * M + k] = P.zu[3 * M + k] = 2.0; }
    P.zl[0] = P.zu[0] = 0.0;
    P.zl[M] = P.zu[M] = 0.0;
    P.zl[M - 1] = xe - 0.01; P.zu[M - 1] = xe + 0.01;
    P.zl[2 * M - 1] = ye - 0.01; P.zu[2 * M - 1] = ye + 0.01;
    P.cl = {-1e20};
    P.cu = {0.0};
    P.cscale = {100.0};
    P.ev = &ev;
    return P;
}

// a start along the straight line to (xe, ye), lifted sideways by `bump` in the middle
std::vector<double> guess(const PointMass& ev, double xe, double ye, double bump) {
    std::vector<double> z(4 * M);
    for (int k = 0; k < M; ++k) {
        const double s = 0.5 * (ev.tau[k] + 1.0);
        z[k] = xe * s;
        z[M + k] = ye * s + bump * std::sin(3.141592653589793 * s);
        z[2 * M + k] = xe / TF;
        z[3 * M + k] = ye / TF;
    }
    return z;
}

int failures = 0;
// eager: a penalty weight that starts too small (0.1), and the residual-based acceptance tried at every rejected first trial
mx::NlpResult run(const char* name, const mx::NlpProblem& P, const std::vector<double>& z0, bool eager = false) {
    mx::NlpOptions opt;
    if (eager) { opt.rho_init = 0.1; opt.crawl_limit = 0; }
    opt.tol = 1e-9;
    opt.max_iter = 300;
    const mx::NlpResult r = mx::solve_nlp(P, opt, z0);
    std::printf("%-28s %s: %s; %d iterations, cost %.9f, soc_steps %d, newton_steps %d, restored_steps %d, rho %.0e\n", name,
                r.ok ? "ok" : "FAILED", r.msg.c_str(), r.iterations, r.cost, r.soc_steps, r.newton_steps, r.restored_steps, r.rho);
    if (!r.ok || r.z.size() != z0.size()) ++failures;
    return r;
}

}  // namespace

int main() {
    PointMass ev;
    const mx::NlpProblem plain = problem(ev, 4.0, 0.0);
    const mx::NlpResult a = run("plain", plain, guess(ev, 4.0, 0.0, 1.5));
    mx::NlpProblem scaled = plain;
    scaled.vscale = {10.0, 10.0, 2.0, 2.0};
    const mx::NlpResult b = run("vscale", scaled, guess(ev, 4.0, 0.0, 1.5));
    if (a.ok && b.ok && std::fabs(a.cost - b.cost) > 1e-6 * a.cost) { std::printf("scaled and unscaled optima differ\n"); ++failures; }
    // the straight line crosses the disc: elastic rows, rejected first trials with their second-order corrections (a step kept and
    // taken back), a full step tried on the KKT residual and taken back (the kept iterate restored), a penalty escalation
    const mx::NlpResult c = run("start through the disc", plain, guess(ev, 4.0, 0.0, 0.0), true);
    if (c.restored_steps == 0 || !(c.rho > 0.1)) { std::printf("the crossing start no longer restores an iterate and escalates the penalty weight\n"); ++failures; }
    // one coupling row: u_y = 0.6 u_x at every node, so the way to (4, 2.4) is a straight line past the disc
    mx::NlpProblem linked = problem(ev, 4.0, 2.4);
    mx::NlpLink L;
    L.dst = 3; L.src = 2;
    L.W.assign(M * M, 0.0);
    for (int k = 0; k < M; ++k) L.W[k * M + k] = 0.6;
    linked.links.push_back(L);
    const mx::NlpResult d = run("one coupling row", linked, guess(ev, 4.0, 2.4, 0.0));
    if (d.ok && d.lamL.size() != (size_t)M) ++failures;
    // the quadrotor through its disc: accepted second-order corrections and an accepted residual-based step
    OracleModel quad(1, 2.5, {1.0, 0.01, 9.81, 1.0, 1.0}, 4.0, 3.2, 0.8);
    std::vector<double> zq;
    const mx::NlpProblem qp = quadrotor_problem(quad, &zq);
    const mx::NlpResult e = run("quadrotor through the disc", qp, zq, true);
    if (e.soc_steps == 0 || e.newton_steps == 0) {
        std::printf("the quadrotor start no longer takes an accepted correction and an accepted residual-based step\n");
        ++failures;
    }
    std::printf(failures ? "%d FAILURES\n" : "all solves ok\n", failures);
    return failures ? 1 : 0;
}
