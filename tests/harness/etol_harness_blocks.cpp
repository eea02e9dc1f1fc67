// etol_harness_blocks.cpp -- extern "C" shim for the node-block tests: (1) the HOST routines of the Newton step's node blocks
// (mi355x::assemble_node_blocks + convexify_node_blocks, what solve_nlp runs per factorisation attempt) on given arrays, one
// instance at a time; (2) a solve of the quadrotor / fixed-wing test problems with Alg::node_blocks set, kept alive for its
// figures.  Linked into libetol_harness.so; the problems are the ones etol_harness_certify.cpp solves (same numbers).
// Test infrastructure.
#include <ETOL/eMI355X.hpp>

#include <array>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "emi_nlp.hpp"
#include "emi_transcribe.hpp"

namespace mx = ETOL::mi355x;

namespace {

struct Held {
    ETOL::eMI355X solver;
    ETOL::f_t obj, obs;
    std::vector<ETOL::f_t> grad;
    std::map<std::string, std::vector<double>> out;
    std::string msg;
};
std::unique_ptr<Held> g_held;

const std::vector<double> kQuad = {1.0, 0.01, 9.81, 1.0, 1.0};
const std::vector<double> kFw = {10.0, 0.8, 1.1, 1.8, 9.81, 120.0, 0.3, 4.5, 0.03, 0.05, 0.08, -0.6, 0.06, 25.0, 0.9, 1.0};

void set_model(Held& h, int model, int ns, const std::vector<double>& mp) {
    h.obj = [model, mp](F_ARGS) -> ETOL::scalar_t { return mx::objective(model, mp); };
    h.solver.setObjective(&h.obj);
    h.grad.resize(ns);
    std::vector<ETOL::f_t*> gp;
    for (int i = 0; i < ns; ++i) {
        h.grad[i] = [model, i, mp](F_ARGS) -> ETOL::scalar_t { return mx::derivative(model, i, mp); };
        gp.push_back(&h.grad[i]);
    }
    h.solver.setGradient(gp);
}

void quadrotor(Held& h, int nsteps, double dt, int ndiscs) {
    ETOL::TrajectoryOptimizer* t = &h.solver;
    t->setNSteps(nsteps); t->setDt(dt); t->setNStates(6); t->setNControls(2);
    t->setX0({1, 1, 0, 0, 0, 0}); t->setXf({8, 6, 0, 0, 0, 0}); t->setXtol({0.01, 0.01, 0.01, 0.05, 0.05, 0.05});
    t->setXlower({0, 0, -1.2, -6, -6, -4}); t->setXupper({10, 10, 1.2, 6, 6, 4});
    t->setUlower({0, -1.0}); t->setUupper({25, 1.0});
    t->setMaximize(false);
    const std::array<double, 3> all[20] = {{4.0, 3.2, 0.8}, {6.3, 4.4, 0.7}, {2.5, 1.2, 0.4}, {1.6, 3.4, 0.35}, {3.1, 5.2, 0.30},
                                           {5.2, 1.4, 0.35}, {7.4, 2.6, 0.30}, {8.6, 4.2, 0.25}, {5.0, 6.3, 0.35}, {2.2, 7.1, 0.30},
                                           {6.9, 7.4, 0.35}, {8.9, 7.9, 0.30}, {0.9, 5.6, 0.25}, {3.9, 8.4, 0.30}, {9.2, 1.3, 0.30},
                                           {7.0, 0.8, 0.25}, {4.6, 4.9, 0.20}, {2.9, 2.9, 0.20}, {5.6, 3.0, 0.20}, {7.6, 5.4, 0.20}};
    set_model(h, EMI_MODEL_QUADROTOR2D, 6, kQuad);
    if (ndiscs > 20) ndiscs = 20;
    if (ndiscs > 0) {
        std::vector<std::array<double, 3>> discs(all, all + ndiscs);
        for (int i = 0; i < ndiscs; ++i)
            t->addParams({std::pair<PARAM_PAIR>("disc_" + std::to_string(i), {ETOL::var_t::CONTINUOUS, -1000., 0., 0., nsteps * dt})});
        h.obs = [discs](F_ARGS) -> ETOL::scalar_t {
            return mx::disc_rows(discs, std::any_cast<mx::Symbol>(x.at(0)), std::any_cast<mx::Symbol>(x.at(1)));
        };
        t->setConstraints({&h.obs});
    }
}

void fixedwing(Held& h, int nsteps, double tf, double lateral) {
    ETOL::TrajectoryOptimizer* t = &h.solver;
    const std::vector<double>& p = kFw;
    const double CL = p[0] * p[4] / p[5], alpha = (CL - p[6]) / p[7], V = p[13], wt = alpha * V, tht = alpha;
    t->setNSteps(nsteps); t->setDt(tf / nsteps); t->setNStates(12); t->setNControls(4);
    t->setX0({0.0, 0.0, -100.0, 0.0, tht, 0.0, V, 0.0, wt, 0, 0, 0});
    t->setXf({V * tf, lateral, -100.0, 0.0, tht, 0.0, V, 0.0, wt, 0, 0, 0});
    t->setXtol({5.0, 0.5, 2.0, 0.05, 0.05, 0.1, 2.0, 1.0, 1.0, 0.2, 0.2, 0.2});
    t->setXlower({-50, -200, -200, -1.0, -0.6, -1.5, 10, -10, -10, -2, -2, -2});
    t->setXupper({2000, 200, -10, 1.0, 0.6, 1.5, 40, 10, 10, 2, 2, 2});
    t->setUlower({0, -0.5, -0.5, -0.5}); t->setUupper({60, 0.5, 0.5, 0.5});
    t->setMaximize(false);
    set_model(h, EMI_MODEL_FIXEDWING12, 12, kFw);
}

}  // namespace

extern "C" {

// The host loop of one instance: Q = H + (Sigma + dw_shift on free diagonals) + path-row terms (np rows, CSR list of
// (variable, VALS entry) pairs), Qexact = Q, then convexify_node_blocks.  Arrays in the layouts of include/emi355x.h, batch of
// one: H[nh][M], VALS[nvals][M], Sigma[nv][M], sig_t[np][M], fixed[nv][M].  Out: Qexact, Q [nh][M]; *count = recorded pairs,
// of which the first min(count, max_mods) go to node / delta / vec[.][nv]; *worst.  Returns 0, or 1 for nv > 16.
int harness_blocks_host(int nv, int M, int np, const int* row_ptr, const int* var, const int* entry, const double* H, const double* VALS,
                        const double* Sigma, const double* sig_t, const unsigned char* fixed, double dw_shift, double* Qexact, double* Q,
                        int max_mods, int* count, int* node, double* delta, double* vec, double* worst) {
    if (nv > 16) return 1;
    std::vector<std::vector<std::pair<int, int>>> rv((size_t)np);
    for (int j = 0; j < np; ++j)
        for (int a = row_ptr[j]; a < row_ptr[j + 1]; ++a) rv[j].push_back({var[a], entry[a]});
    const size_t nh = (size_t)nv * (nv + 1) / 2;
    mx::assemble_node_blocks(H, VALS, Sigma, sig_t, fixed, dw_shift, rv, nv, M, Q);
    if (Qexact) std::memcpy(Qexact, Q, nh * M * sizeof(double));
    std::vector<mx::BlockMod> mods;
    *worst = mx::convexify_node_blocks(Q, fixed, nv, M, &mods);
    *count = (int)mods.size();
    for (int c = 0; c < (int)mods.size() && c < max_mods; ++c) {
        node[c] = mods[c].node;
        delta[c] = mods[c].delta;
        for (int v = 0; v < nv; ++v) vec[(size_t)c * nv + v] = mods[c].v[v];
    }
    return 0;
}

// problem 1: quadrotor (nsteps, horizon, ndiscs = n);  2: fixed wing (nsteps, horizon, lateral = n).  Default Alg except:
// node_blocks "device" / "host" as given, nlp_tolerance tol (<= 0: the default), certify on, one mesh of nsteps + 1 nodes; the
// iteration budget is Alg's default (nlp_iter_max 200 per NLP solve).  Returns 0 solved, 1 not solved (harness_blk_message).  Figures through harness_blk_get.
int harness_blk_solve(int problem, int nsteps, double horizon, double n, int device_blocks, double tol) {
    g_held.reset(new Held());
    Held& h = *g_held;
    if (problem == 1) quadrotor(h, nsteps, horizon / nsteps, (int)n);
    else if (problem == 2) fixedwing(h, nsteps, horizon, n);
    else return 3;
    h.solver.setup();
    mx::Alg* a = h.solver.getAlgorithm();
    a->certify = true;
    a->mesh_refinement = "none";
    a->node_blocks = device_blocks ? "device" : "host";
    if (tol > 0) a->nlp_tolerance = tol;
    h.solver.solve();
    const mx::Sol* s = h.solver.getSolution();
    h.msg = s->error_msg;
    if (s->error_flag) return 1;
    auto& o = h.out;
    o["X"] = s->states; o["U"] = s->controls; o["lamF"] = s->lamF; o["lamC"] = s->lamC;
    const mx::Sol::Certificate& c = s->certificate;
    o["cert"] = {c.stationarity, c.complementarity, c.defect, c.violation, c.grad_max, c.lam_max, c.computed ? 1.0 : 0.0};
    o["on_device"] = {s->linear_solver.rfind("device", 0) == 0 ? 1.0 : 0.0, s->node_blocks == "device" ? 1.0 : 0.0};   // Newton step, node blocks
    o["stats"] = {s->cost, (double)s->nlp_iterations_total, (double)s->nlp_iterations, s->kkt_error, (double)s->mesh_iterations,
                  a->nlp_tolerance, mx::NlpOptions().acceptable_factor};
    std::vector<double>& runs = o["runs"];      // per NLP solve: nodes, iterations, seconds, t_blocks, t_factor, factorisations
    for (const auto& r : s->nlp_runs) {
        runs.push_back((double)r.nodes); runs.push_back(r.iterations); runs.push_back(r.seconds); runs.push_back(r.t_blocks);
        runs.push_back(r.t_factor); runs.push_back(r.factorisations);
    }
    return 0;
}

const char* harness_blk_message(void) { return g_held ? g_held->msg.c_str() : "no solve held"; }

// number of values of `name` (copied into out when cap suffices); -1: unknown name
int harness_blk_get(const char* name, double* out, int cap) {
    if (!g_held) return -1;
    auto it = g_held->out.find(name);
    if (it == g_held->out.end()) return -1;
    const int n = (int)it->second.size();
    if (out && cap >= n && n > 0) std::memcpy(out, it->second.data(), (size_t)n * sizeof(double));
    return n;
}

void harness_blk_release(void) {
    if (g_held) g_held->solver.close();
    g_held.reset();
}

}  // extern "C"
