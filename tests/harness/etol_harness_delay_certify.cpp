// etol_harness_delay_certify.cpp -- extern "C" shim over ETOL::eMI355X for the certificate tests of DELAYED problems: solves the
// delayed problem of etol_harness.cpp (configure_delay_demo: same functions and numbers, model 3 of oracle/emi_oracle.c) as
// harness_solve_delay_demo does, keeps the solver alive and hands out the trajectory, the multipliers (Sol::lamL included),
// Sol::adjDelayed, Sol::certificate and the bounds an INDEPENDENT check needs.  Linked into libetol_harness.so.  Test infrastructure.
#include <ETOL/eMI355X.hpp>

#include <any>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "emi_nlp.hpp"
#include "emi_transcribe.hpp"

namespace mx = ETOL::mi355x;

namespace {

struct HeldDelay {
    ETOL::eMI355X solver;
    ETOL::f_t obj, f0, f1, obs;
    std::map<std::string, std::vector<double>> out;
    std::string msg;
};
std::unique_ptr<HeldDelay> g_dc;

// x = [x0 x1 | x(t-dt) | x(t-2dt)], u = [u0 u1 | u(t-dt)]  (reference ePSOPT.cpp:225-248)
void configure(HeldDelay& d, int nsteps, double dt, int xh, int uh, double disc_r) {
    ETOL::TrajectoryOptimizer* t = &d.solver;
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
    d.obs = [disc_r](F_ARGS) -> ETOL::scalar_t {
        return mx::disc_rows({{2.0, 1.5, disc_r}}, std::any_cast<mx::Symbol>(x.at(0)), std::any_cast<mx::Symbol>(x.at(1)));
    };
    if (disc_r > 0) {
        t->addParams({std::pair<PARAM_PAIR>("disc_0", {ETOL::var_t::CONTINUOUS, -1000., 0., 0., nsteps * dt})});
        t->setConstraints({&d.obs});
    }
}

void put_cert(std::vector<double>& v, const mx::Sol::Certificate& c) {
    v = {c.stationarity, c.complementarity, c.defect, c.violation, c.grad_max, c.lam_max, c.computed ? 1.0 : 0.0};
}

}  // namespace

extern "C" {

// Alg as harness_solve_delay_demo sets it (nlp_tolerance = tol, nlp_iter_max 400), certify as given.  0 solved, 1 not solved
// (harness_dc_message).  The solver stays alive for harness_dc_get / harness_dc_certify.
int harness_dc_solve(int nsteps, double dt, int xh, int uh, double disc_r, double tol, int certify) {
    g_dc.reset(new HeldDelay());
    HeldDelay& h = *g_dc;
    configure(h, nsteps, dt, xh, uh, disc_r);
    h.solver.setup();
    mx::Alg* a = h.solver.getAlgorithm();
    a->nlp_tolerance = tol;
    a->nlp_iter_max = 400;
    a->certify = certify != 0;
    h.solver.solve();
    const mx::Sol* s = h.solver.getSolution();
    const mx::Prob* P = h.solver.getProblem();
    h.msg = s->error_msg;
    if (s->error_flag) return 1;
    auto& o = h.out;
    o["X"] = s->states; o["U"] = s->controls; o["lamF"] = s->lamF; o["lamC"] = s->lamC; o["lamL"] = s->lamL; o["adjDelayed"] = s->adjDelayed;
    put_cert(o["cert"], s->certificate);
    o["recs"] = P->path_records; o["tau"] = P->tau;
    const mx::NlpProblem nlp = mx::make_nlp(*P, nullptr);          // the stated problem (not lifted): bounds on [x | u]
    o["zl"] = nlp.zl; o["zu"] = nlp.zu; o["cl"] = nlp.cl; o["cu"] = nlp.cu;
    o["dims"] = {(double)P->nstates, (double)P->ncontrols, (double)P->npath, (double)P->nodes, (double)P->ndelayed, (double)P->xhorizon,
                 (double)P->uhorizon, P->delay_dt, P->t0, P->tf, P->lifted ? 1.0 : 0.0};
    o["stats"] = {s->cost, (double)s->nlp_iterations_total, (double)s->nlp_iterations, s->kkt_error, a->nlp_tolerance,
                  mx::NlpOptions().acceptable_factor};
    return 0;
}

const char* harness_dc_message(void) { return g_dc ? g_dc->msg.c_str() : "no solve held"; }

// number of values of `name` (copied into out when cap suffices); -1: unknown name
int harness_dc_get(const char* name, double* out, int cap) {
    if (!g_dc) return -1;
    auto it = g_dc->out.find(name);
    if (it == g_dc->out.end()) return -1;
    const int n = (int)it->second.size();
    if (out && cap >= n && n > 0) std::memcpy(out, it->second.data(), (size_t)n * sizeof(double));
    return n;
}

// ETOL::eMI355X::certify of any point on the held solver's mesh: z = [X | U]; cert7 = six figures + computed; adj [ndelayed][nodes]
int harness_dc_certify(const double* z, int nz, const double* lamF, int nf, const double* lamC, int nc, double* cert7, double* adj, int adj_cap) {
    if (!g_dc) return 1;
    std::vector<double> c, g;
    put_cert(c, g_dc->solver.certify(std::vector<double>(z, z + nz), std::vector<double>(lamF, lamF + nf),
                                     std::vector<double>(lamC, lamC + nc), &g));
    std::memcpy(cert7, c.data(), 7 * sizeof(double));
    if (adj && adj_cap >= (int)g.size() && !g.empty()) std::memcpy(adj, g.data(), g.size() * sizeof(double));
    return 0;
}

void harness_dc_release(void) {
    if (g_dc) g_dc->solver.close();
    g_dc.reset();
}

}  // extern "C"
