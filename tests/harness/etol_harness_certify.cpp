// etol_harness_certify.cpp -- extern "C" shim over ETOL::eMI355X for the certificate tests: solves one of the test problems
// with the default Alg, keeps the solver alive and hands out the trajectory, the multipliers, Sol::certificate and everything
// of the transcribed problem an INDEPENDENT check needs (record table, track centres, bounds).  Linked into
// libetol_harness.so beside etol_harness.cpp; the problems are the ones that file solves (same numbers).  Test infrastructure.
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
    ETOL::f_t obj, obs, saa;
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

// the quadrotor problem of etol_harness.cpp (configure_quadrotor, built-in model): corner to corner past up to 20 discs
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

// the fixed-wing lateral offset of etol_harness.cpp (configure_fixedwing)
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

// the shipped problem (an XML configuration) with its keep-outs, as harness_solve_example1 sets it up (built-in rows)
void example1(Held& h, const char* xml) {
    ETOL::TrajectoryOptimizer* t = &h.solver;
    t->loadConfigs(xml);
    t->setMaximize(false);
    set_model(h, EMI_MODEL_POINTMASS2D, 2, {});
    const double tspan = t->getDt() * t->getNSteps();
    const std::vector<ETOL::border_t>* zones = t->getObstacles_Raw();
    size_t i = 0;
    for (const auto& z : *zones) {
        for (size_t j = 0; j < z.size(); ++j)
            t->addParams({std::pair<PARAM_PAIR>("side_" + std::to_string(i) + "_" + std::to_string(j) + "_0",
                                                {ETOL::var_t::CONTINUOUS, -1000., 0., 0., tspan})});
        ++i;
    }
    const std::list<ETOL::track_t>* tracks = t->getTracks();
    for (size_t k = 0; k < tracks->size(); ++k)
        t->addParams({std::pair<PARAM_PAIR>("ball_" + std::to_string(k) + "_0_0", {ETOL::var_t::CONTINUOUS, -1000., 0., 0., tspan})});
    h.obs = [zones](F_ARGS) -> ETOL::scalar_t {
        return mx::ellipse_rows(*zones, std::any_cast<mx::Symbol>(x.at(0)), std::any_cast<mx::Symbol>(x.at(1)));
    };
    h.saa = [tracks](F_ARGS) -> ETOL::scalar_t {
        return mx::track_rows(*tracks, std::any_cast<mx::Symbol>(x.at(0)), std::any_cast<mx::Symbol>(x.at(1)));
    };
    t->setConstraints({&h.obs, &h.saa});
}

void put_cert(std::vector<double>& v, const mx::Sol::Certificate& c) {
    v = {c.stationarity, c.complementarity, c.defect, c.violation, c.grad_max, c.lam_max, c.computed ? 1.0 : 0.0};
}

}  // namespace

extern "C" {

// problem 0: the shipped XML problem (xml);  1: quadrotor (nsteps, horizon, ndiscs = n);  2: fixed wing (nsteps, horizon, lateral = n).
// Default Alg except: certify as given, no mesh refinement for problems 1 / 2 (one mesh of nsteps + 1 nodes, reached through the
// mesh ladder), nlp_iter_max 400.  Returns 0 solved, 1 not solved (harness_cs_message).  The solver stays alive for harness_cs_*.
int harness_cs_solve(int problem, const char* xml, int nsteps, double horizon, double n, int certify) {
    g_held.reset(new Held());
    Held& h = *g_held;
    if (problem == 0) example1(h, xml);
    else if (problem == 1) quadrotor(h, nsteps, horizon / nsteps, (int)n);
    else if (problem == 2) fixedwing(h, nsteps, horizon, n);
    else return 3;
    h.solver.setup();
    mx::Alg* a = h.solver.getAlgorithm();
    a->certify = certify != 0;
    a->nlp_iter_max = 400;
    if (problem != 0) a->mesh_refinement = "none";
    h.solver.solve();
    const mx::Sol* s = h.solver.getSolution();
    const mx::Prob* P = h.solver.getProblem();
    h.msg = s->error_msg;
    if (s->error_flag) return 1;
    auto& o = h.out;
    o["X"] = s->states; o["U"] = s->controls; o["lamF"] = s->lamF; o["lamC"] = s->lamC;
    put_cert(o["cert"], s->certificate);
    o["recs"] = P->path_records; o["track_x"] = P->track_x; o["track_y"] = P->track_y;
    o["params"] = P->model_params; o["tau"] = P->tau;
    const mx::NlpProblem nlp = mx::make_nlp(*P, nullptr);
    o["zl"] = nlp.zl; o["zu"] = nlp.zu; o["cl"] = nlp.cl; o["cu"] = nlp.cu;
    o["dims"] = {(double)P->nstates, (double)P->ncontrols, (double)P->npath, (double)P->nodes, (double)P->ntracks, (double)P->px,
                 (double)P->py, (double)P->model, P->t0, P->tf, (double)P->npath_traced};
    o["stats"] = {s->cost, (double)s->nlp_iterations_total, (double)s->nlp_iterations, s->kkt_error, (double)s->mesh_iterations,
                  a->nlp_tolerance, mx::NlpOptions().acceptable_factor};
    std::vector<double>& runs = o["runs"];          // per NLP solve: nodes, iterations, seconds, host J^T lambda seconds
    for (const auto& r : s->nlp_runs) { runs.push_back((double)r.nodes); runs.push_back(r.iterations); runs.push_back(r.seconds); runs.push_back(r.t_jt); }
    return 0;
}

const char* harness_cs_message(void) { return g_held ? g_held->msg.c_str() : "no solve held"; }

// number of values of `name` (copied into out when cap suffices); -1: unknown name
int harness_cs_get(const char* name, double* out, int cap) {
    if (!g_held) return -1;
    auto it = g_held->out.find(name);
    if (it == g_held->out.end()) return -1;
    const int n = (int)it->second.size();
    if (out && cap >= n && n > 0) std::memcpy(out, it->second.data(), (size_t)n * sizeof(double));
    return n;
}

// ETOL::eMI355X::certify of any point on the held solver's mesh: z = [X | U]; cert7 = six figures + computed
int harness_cs_certify(const double* z, int nz, const double* lamF, int nf, const double* lamC, int nc, double* cert7) {
    if (!g_held) return 1;
    std::vector<double> c;
    put_cert(c, g_held->solver.certify(std::vector<double>(z, z + nz), std::vector<double>(lamF, lamF + nf),
                                       std::vector<double>(lamC, lamC + nc)));
    std::memcpy(cert7, c.data(), 7 * sizeof(double));
    return 0;
}

void harness_cs_release(void) {
    if (g_held) g_held->solver.close();
    g_held.reset();
}

}  // extern "C"
