// mesh_driver_main.cpp -- the decision tree of mi355x::MeshDriver (etol_amd/host/emi_mesh_driver.cpp) under a scripted solver and
// the host sanitizers (`make check-mesh-driver`): no Python, no device.  The host interface is a script: every NLP call returns the
// next scripted (ok, iterations, msg, rho) with z = the guess it was given and records what it was asked -- mesh, barrier settings,
// limits, which start the default guess is; every mesh change and ODE-error call is logged.  The problem is a point mass from (0, 0)
// to (8, 0) with a disc of radius 1 at (4, 0) between them, so that planned_path_guess finds a route (npath = 1, span = 8).
// The expected sequences are read from the code of solve() as it was before the strategy became an object.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include <unistd.h>

#include "emi355x.h"
#include "emi_mesh_driver.hpp"
#include "emi_transcribe.hpp"

namespace mx = ETOL::mi355x;

namespace {

struct Step { bool ok; int iterations; double rho; };
struct Call {
    size_t nodes;
    double mu_init;
    int max_iter;
    double tol, bound_push, rho_init, bend;
    bool planned, guess_empty;
    double disc_rsq;
    double lam0_err;        // multiplier guesses given: max |lamF0 - w|, |lamC0 - 2 w| over the mesh; -1: none given
};
struct Event { char kind; size_t nodes; double disc_rsq; };      // 'm' set_mesh, 'c' reconfigure, 's' solve, 'e' ode_error

struct ScriptHost : public mx::MeshHost {
    mx::Prob& P;
    std::function<Step(int, size_t)> script;        // (index of the call, nodes) -> what the solve returns
    std::vector<double> errors;                     // ODE errors, in call order
    std::vector<Call> calls;
    std::vector<Event> events;
    size_t ode_calls = 0;
    explicit ScriptHost(mx::Prob& p) : P(p) {}
    void set_mesh(size_t nodes) override {          // as eMI355X::setMesh (no tracks here)
        P.nodes = nodes;
        P.tau.resize(nodes); P.w.resize(nodes); P.D.resize(nodes * nodes);
        emi_lgl((int)nodes, P.tau.data(), P.w.data(), P.D.data());
        events.push_back({'m', nodes, P.path_records[3]});
    }
    void reconfigure() override { events.push_back({'c', P.nodes, P.path_records[3]}); }
    mx::NlpResult solve_nlp(mx::NlpProblem& nlp, const mx::NlpOptions& o, const std::vector<double>& z0) override {
        const Step s = script((int)calls.size(), P.nodes);
        const size_t M = P.nodes;
        double lam0_err = -1;
        if (nlp.lamF0.size() == 2 * M && nlp.lamC0.size() == M) {
            lam0_err = 0;
            for (size_t k = 0; k < M; ++k)
                lam0_err = std::max({lam0_err, std::fabs(nlp.lamF0[k] - P.w[k]), std::fabs(nlp.lamF0[M + k] - P.w[k]), std::fabs(nlp.lamC0[k] - 2 * P.w[k])});
        }
        calls.push_back({P.nodes, o.mu_init, o.max_iter, o.tol, o.bound_push, o.rho_init, P.guess_bend, P.guess_planned, P.guess_states.empty(),
                         P.path_records[3], lam0_err});
        events.push_back({'s', P.nodes, P.path_records[3]});
        mx::NlpResult r;
        r.ok = s.ok;
        r.iterations = s.iterations;
        r.msg = s.ok ? "converged" : "scripted failure";
        r.rho = s.rho;
        r.z = z0;
        // multipliers whose costate samples lambda_k / w_k are constant (1 on the defect rows, 2 on the path row): what the covector mapping
        // of Alg::warm_multipliers carries to the next mesh is then that mesh's weights times the same constants
        r.lamF.resize(2 * M);
        r.lamC.resize(M);
        for (size_t k = 0; k < M; ++k) { r.lamF[k] = r.lamF[M + k] = P.w[k]; r.lamC[k] = 2 * P.w[k]; }
        if ((size_t)nlp.M != P.nodes || z0.size() != 4 * P.nodes) { std::printf("solve_nlp: problem and guess are not of the current mesh\n"); std::exit(1); }
        return r;
    }
    double ode_error(const std::vector<double>& z) override {
        events.push_back({'e', P.nodes, P.path_records[3]});
        if (z.size() != 4 * P.nodes || ode_calls >= errors.size()) { std::printf("ode_error: unexpected call\n"); std::exit(1); }
        return errors[ode_calls++];
    }
};

mx::Prob problem(size_t nodes) {
    mx::Prob P;
    P.nstates = 2; P.ncontrols = 2; P.nodes = nodes; P.t0 = 0; P.tf = 8;
    P.model = EMI_MODEL_POINTMASS2D;
    P.tau.resize(nodes); P.w.resize(nodes); P.D.resize(nodes * nodes);
    emi_lgl((int)nodes, P.tau.data(), P.w.data(), P.D.data());
    P.path_records = {(double)EMI_PATH_DISC, 4.0, 0.0, 1.0, 0, 0, 0, 0};
    P.npath = 1;
    P.px = 0; P.py = 1;
    P.state_lower = {-10, -10}; P.state_upper = {10, 10}; P.control_lower = {-2, -2}; P.control_upper = {2, 2};
    P.event_lower = {0, 0, 8 - 0.01, -0.01}; P.event_upper = {0, 0, 8 + 0.01, 0.01};
    P.path_lower = {-1000.0}; P.path_upper = {0.0};
    return P;
}

// stdout of the run, taken at file-descriptor level
struct Capture {
    int keep;
    FILE* f;
    Capture() : f(std::tmpfile()) { std::fflush(stdout); keep = dup(1); dup2(fileno(f), 1); }
    std::string end() {
        std::fflush(stdout);
        dup2(keep, 1);
        close(keep);
        std::string s;
        std::rewind(f);
        char buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
        std::fclose(f);
        return s;
    }
};

int failures = 0;
const char* current = "";
void expect(bool ok, const std::string& what) {
    if (ok) return;
    std::printf("case %s: %s\n", current, what.c_str());
    ++failures;
}

struct Outcome {
    mx::NlpResult r;
    mx::Sol sol;
    std::vector<Call> calls;
    std::vector<Event> events;
    std::string text;
    size_t nodes_after;
};

// one run of the driver as eMI355X::solve() makes it (options from Alg, KeepGuess round it); case 11 in every case: the working
// storage of the strategy on the Prob is what it was before
Outcome run(const char* name, const mx::Alg& alg, size_t nodes, std::function<Step(int, size_t)> script, std::vector<double> errors = {}) {
    current = name;
    mx::Prob P = problem(nodes);
    const mx::Prob before = P;
    ScriptHost host(P);
    host.script = std::move(script);
    host.errors = std::move(errors);
    mx::NlpOptions opt;
    opt.tol = alg.nlp_tolerance;
    opt.max_iter = alg.nlp_iter_max;
    opt.print_level = alg.print_level;
    Outcome out;
    Capture cap;
    {
        mx::KeepGuess keep(P);
        out.r = mx::MeshDriver(P, alg, out.sol, host, opt).run();
    }
    out.text = cap.end();
    out.calls = host.calls;
    out.events = host.events;
    out.nodes_after = P.nodes;
    expect(P.guess_states == before.guess_states && P.guess_controls == before.guess_controls && P.guess_lamF == before.guess_lamF &&
               P.guess_lamC == before.guess_lamC, "the guess vectors of the Prob are not what they were before the run");
    expect(P.guess_bend == before.guess_bend && P.guess_planned == before.guess_planned, "guess_bend / guess_planned are not what they were before the run");
    expect(P.path_records == before.path_records, "path_records are not what they were before the run");
    expect(out.sol.nlp_runs.size() == out.calls.size(), "Sol::nlp_runs does not hold one entry per NLP call");
    for (size_t i = 0; i < out.sol.nlp_runs.size() && i < out.calls.size(); ++i)
        expect(out.sol.nlp_runs[i].nodes == out.calls[i].nodes, "Sol::nlp_runs[" + std::to_string(i) + "] is not of the mesh of call " + std::to_string(i));
    return out;
}

mx::Alg defaults() {
    mx::Alg a;
    a.mesh_refinement = "none";
    a.print_level = 5;
    return a;
}

// what a recorded call must be
struct Want {
    size_t nodes;
    bool cold;              // cold barrier settings (mu_init 0.1, push 1e-2) or the warm ones of Alg
    int max_iter;
    double tol, rho_init, bend;
    bool planned, guess_empty;
};
void expect_calls(const Outcome& o, const mx::Alg& a, const std::vector<Want>& want) {
    expect(o.calls.size() == want.size(), "expected " + std::to_string(want.size()) + " NLP calls, got " + std::to_string(o.calls.size()));
    for (size_t i = 0; i < want.size() && i < o.calls.size(); ++i) {
        const Call& c = o.calls[i];
        const Want& w = want[i];
        const double mu = w.cold ? 0.1 : a.warm_mu_init, push = w.cold ? 1e-2 : a.warm_bound_push;
        char buf[400];
        std::snprintf(buf, sizeof buf, "call %zu: got nodes %zu mu %.3g max_iter %d tol %.3g push %.3g rho_init %.3g bend %+.3f planned %d empty %d; "
                      "want nodes %zu mu %.3g max_iter %d tol %.3g push %.3g rho_init %.3g bend %+.3f planned %d empty %d", i, c.nodes, c.mu_init,
                      c.max_iter, c.tol, c.bound_push, c.rho_init, c.bend, (int)c.planned, (int)c.guess_empty, w.nodes, mu, w.max_iter, w.tol, push,
                      w.rho_init, w.bend, (int)w.planned, (int)w.guess_empty);
        expect(c.nodes == w.nodes && c.mu_init == mu && c.max_iter == w.max_iter && c.tol == w.tol && c.bound_push == push && c.rho_init == w.rho_init &&
                   c.bend == w.bend && c.planned == w.planned && c.guess_empty == w.guess_empty, buf);
    }
}
std::string mesh_changes(const Outcome& o) {
    std::string s;
    for (const Event& e : o.events)
        if (e.kind == 'm') s += (s.empty() ? "" : " ") + std::to_string(e.nodes);
    return s;
}
std::string runs(const Outcome& o) {
    std::string s;
    for (const auto& u : o.sol.nlp_runs) s += (s.empty() ? "" : " ") + std::to_string(u.nodes) + (u.converged ? "" : "!");
    return s;
}
bool has(const Outcome& o, const char* what) { return o.text.find(what) != std::string::npos; }
std::function<Step(int, size_t)> sequence(std::vector<Step> steps, Step then) {
    return [steps, then](int i, size_t) { return i < (int)steps.size() ? steps[i] : then; };
}

const Step OK{true, 20, 10.0}, FAIL{false, 40, 10.0};

}  // namespace

int main() {
    const double span = 8.0;
    // 1: every solve converges -- planned route on 33 (cold), 65 (warm, rung patience, rung tolerance), 129 (warm, target patience)
    {
        const mx::Alg a = defaults();
        const double rt = std::max(a.nlp_tolerance, a.rung_tolerance);
        const Outcome o = run("1 all converge", a, 129, sequence({}, OK));
        expect_calls(o, a, {{33, true, 200, rt, 10.0, 0.0, true, true},
                            {65, false, 100, rt, 10.0, 0.0, false, false},
                            {129, false, std::min(200, a.target_patience), a.nlp_tolerance, 10.0, 0.0, false, false}});
        expect(mesh_changes(o) == "33 65 129", "mesh changes " + mesh_changes(o));
        expect(o.sol.mesh_iterations == 3 && o.r.ok && o.nodes_after == 129, "three mesh iterations, solved on 129 nodes");
        expect(span == mx::boundary_span(problem(129)), "boundary_span of the problem is 8");
    }
    // 2: the second rung fails once -- the ladder again from the straight line; the penalty weight of the warm rungs carries the largest
    // seen within one climb and starts again with the next
    {
        const mx::Alg a = defaults();
        const double rt = std::max(a.nlp_tolerance, a.rung_tolerance);
        const Outcome o = run("2 second rung fails once", a, 129, sequence({{true, 20, 50.0}, {false, 40, 20.0}, {true, 20, 30.0}, {true, 20, 5.0}}, OK));
        expect_calls(o, a, {{33, true, 200, rt, 10.0, 0.0, true, true},
                            {65, false, 100, rt, 50.0, 0.0, false, false},
                            {33, true, 200, rt, 10.0, 0.0, false, true},
                            {65, false, 100, rt, 30.0, 0.0, false, false},
                            {129, false, 200, a.nlp_tolerance, 30.0, 0.0, false, false}});
        expect(runs(o) == "33 65! 33 65 129", "runs " + runs(o));
        expect(has(o, "mesh sequencing: a rung failed (scripted failure), ladder restarted from the line bent by +0.000\n"), "the restart line is missing");
        expect(o.sol.mesh_iterations == 5 && o.r.ok, "five mesh iterations, solved");
    }
    // 3: the first rung never converges -- its cold start goes through the bends (no planned retry: it began from the plan), no second
    // climb; then the cold start on the requested mesh with all its retries
    {
        const mx::Alg a = defaults();
        const double rt = std::max(a.nlp_tolerance, a.rung_tolerance), t = a.nlp_tolerance;
        const Outcome o = run("3 first rung never converges", a, 129, sequence({}, FAIL));
        expect_calls(o, a, {{33, true, 200, rt, 10.0, 0.0, true, true},
                            {33, true, 200, rt, 10.0, 0.15 * span, false, true},
                            {33, true, 200, rt, 10.0, -0.15 * span, false, true},
                            {33, true, 200, rt, 10.0, 0.35 * span, false, true},
                            {33, true, 200, rt, 10.0, -0.35 * span, false, true},
                            {129, true, 200, t, 10.0, 0.0, false, true},
                            {129, true, 200, t, 10.0, 0.15 * span, false, true},
                            {129, true, 200, t, 10.0, -0.15 * span, false, true},
                            {129, true, 200, t, 10.0, 0.35 * span, false, true},
                            {129, true, 200, t, 10.0, -0.35 * span, false, true},
                            {129, true, 200, t, 10.0, 0.0, true, true}});
        expect(mesh_changes(o) == "33 129", "mesh changes " + mesh_changes(o));
        expect(!o.r.ok && o.sol.mesh_iterations == 2, "not solved, two mesh iterations");
        expect(!has(o, "cold start on ") && !has(o, "ladder restarted"), "no sequenced warm start happened: no fall-back line, no restart");
    }
    // 4: the warm start on the requested mesh fails, using all its iterations -- the ladder again from start 1, no cold start on 129
    {
        const mx::Alg a = defaults();
        const double rt = std::max(a.nlp_tolerance, a.rung_tolerance), t = a.nlp_tolerance;
        const Outcome o = run("4 warm start on the target fails", a, 129, sequence({OK, OK, {false, 200, 10.0}}, OK));
        expect_calls(o, a, {{33, true, 200, rt, 10.0, 0.0, true, true}, {65, false, 100, rt, 10.0, 0.0, false, false}, {129, false, 200, t, 10.0, 0.0, false, false},
                            {33, true, 200, rt, 10.0, 0.0, false, true}, {65, false, 100, rt, 10.0, 0.0, false, false}, {129, false, 200, t, 10.0, 0.0, false, false}});
        expect(runs(o) == "33 65 129! 33 65 129", "runs " + runs(o));
        expect(has(o, "mesh sequencing: warm start on 129 nodes failed (scripted failure), ladder restarted from the line bent by +0.000\n"), "the restart line is missing");
        expect(!has(o, "cold start on "), "a cold start on the requested mesh");
        expect(o.r.ok && o.sol.mesh_iterations == 6, "solved in six mesh iterations");
    }
    // 5: the requested mesh always fails -- one climb per start (planned, line, four bends: start ca needs ca - 2 < guess_retries), the
    // target patience for as long as another start is left, then exactly one cold start with its retries on 129
    {
        mx::Alg a = defaults();
        a.target_patience = 50;
        const double rt = std::max(a.nlp_tolerance, a.rung_tolerance), t = a.nlp_tolerance;
        const Outcome o = run("5 every start used up", a, 129, [](int, size_t nodes) { return nodes == 129 ? FAIL : OK; });
        std::vector<Want> want;
        const double bends[6] = {0.0, 0.0, 0.15 * span, -0.15 * span, 0.35 * span, -0.35 * span};
        for (int ca = 0; ca < 6; ++ca) {
            want.push_back({33, true, 200, rt, 10.0, bends[ca], ca == 0, true});
            want.push_back({65, false, 100, rt, 10.0, 0.0, false, false});
            want.push_back({129, false, ca < 5 ? 50 : 200, t, 10.0, 0.0, false, false});
        }
        for (int q = 0; q < 6; ++q) want.push_back({129, true, 200, t, 10.0, q >= 1 && q <= 4 ? bends[q + 1] : 0.0, q == 5, true});
        expect_calls(o, a, want);
        expect(has(o, "mesh sequencing: warm start on 129 nodes failed (scripted failure), ladder restarted from the line bent by -2.800\n"), "the last restart line is missing");
        expect(has(o, "mesh sequencing: warm start failed (scripted failure), cold start on 129 nodes\n"), "the fall-back line is missing");
        expect(!o.r.ok && o.sol.mesh_iterations == 19, "not solved; 12 rungs, 6 warm starts and the cold start");
        a.guess_retries = 2;            // the planned route, the line and two bends; the cold start: the line, two bends, the planned route
        const Outcome o2 = run("5 every start used up, guess_retries 2", a, 129, [](int, size_t nodes) { return nodes == 129 ? FAIL : OK; });
        expect(runs(o2) == "33 65 129! 33 65 129! 33 65 129! 33 65 129! 129! 129! 129! 129!", "runs " + runs(o2));
        expect(o2.calls.size() == 16 && o2.calls[8].max_iter == 50 && o2.calls[11].max_iter == 200, "the last warm start on the target runs without the target patience");
    }
    // 6: the iteration budget of the solve() is crossed during the second run -- nothing is asked of the solver after that
    {
        mx::Alg a = defaults();
        a.nlp_iter_budget = 150;
        const Outcome o = run("6 budget", a, 129, sequence({{true, 100, 10.0}, {false, 50, 10.0}}, OK));
        expect(o.calls.size() == 2 && o.calls[0].max_iter == 150 && o.calls[1].max_iter == 50, "two calls, with what was left of the budget as their limit");
        expect(o.sol.nlp_runs.size() == 2 && o.sol.nlp_iterations_total == 150, "nlp_runs holds the two runs that happened");
        expect(!o.r.ok && o.r.msg.rfind("iteration budget exhausted (", 0) == 0, "message: " + o.r.msg);
        expect(o.sol.mesh_iterations == 4, "mesh iterations " + std::to_string(o.sol.mesh_iterations));
    }
    // 7: a warm start still running after warm_patience iterations runs again with a 10 x larger barrier parameter and its full limit
    {
        mx::Alg a = defaults();
        a.warm_patience = 30;
        const double rt = std::max(a.nlp_tolerance, a.rung_tolerance);
        const Outcome o = run("7 warm patience", a, 129, sequence({OK, {false, 30, 10.0}}, OK));
        expect(o.calls.size() == 4, "four calls");
        if (o.calls.size() == 4) {
            expect(o.calls[1].nodes == 65 && o.calls[1].max_iter == 30 && o.calls[1].mu_init == a.warm_mu_init, "the rung first runs warm_patience iterations");
            expect(o.calls[2].nodes == 65 && o.calls[2].max_iter == 100 && o.calls[2].mu_init == 10.0 * a.warm_mu_init && o.calls[2].tol == rt &&
                       o.calls[2].bound_push == a.warm_bound_push && !o.calls[2].guess_empty, "... then again with mu_init x 10 and its full limit");
            expect(o.calls[3].nodes == 129 && o.calls[3].max_iter == 30, "the target's warm start begins with warm_patience iterations too");
        }
        expect(has(o, "warm start still running after 30 iterations: again from the same guess with barrier parameter 1.0e-04\n"), "the line of the repeat is missing");
        expect(o.r.ok && o.sol.mesh_iterations == 3, "solved in three mesh iterations");
    }
    // 8: a refinement solve that fails leaves the converged coarser solution
    {
        mx::Alg a = defaults();
        a.mesh_refinement = "automatic";
        const Outcome o = run("8 refinement falls back", a, 41, sequence({OK, FAIL}, OK), {1e-2});
        expect_calls(o, a, {{41, true, 200, a.nlp_tolerance, 10.0, 0.0, false, true}, {61, true, 200, a.nlp_tolerance, 10.0, 0.0, false, false}});
        expect(mesh_changes(o) == "61 41", "mesh changes " + mesh_changes(o));
        expect(o.r.ok && o.r.z.size() == 4 * 41 && o.nodes_after == 41 && o.sol.ode_error == 1e-2 && o.sol.mesh_iterations == 2, "the 41-node result with its error");
        expect(has(o, "mesh iteration 1 failed (scripted failure): keeping the 41-node solution\n"), "the fall-back line is missing");
    }
    // 9: refinement stops when the tolerance is met; mr_max_nodes caps the new mesh
    {
        mx::Alg a = defaults();
        a.mesh_refinement = "automatic";
        const Outcome o = run("9 refinement stops", a, 41, sequence({}, OK), {1e-2, 1e-5});
        expect(mesh_changes(o) == "61" && o.calls.size() == 2 && o.r.ok && o.nodes_after == 61 && o.sol.ode_error == 1e-5 && o.sol.mesh_iterations == 2, "stops on 61 nodes");
        a.mr_max_nodes = 50;
        const Outcome o2 = run("9 refinement stops, capped", a, 41, sequence({}, OK), {1e-2, 1e-5});
        expect(mesh_changes(o2) == "50" && o2.nodes_after == 50, "mesh changes " + mesh_changes(o2));
        const Outcome o3 = run("9 refinement stops at the cap", a, 41, sequence({}, OK), {1e-2, 1e-2});
        expect(mesh_changes(o3) == "50" && o3.calls.size() == 2 && o3.sol.ode_error == 1e-2, "no mesh beyond mr_max_nodes");
    }
    // 10: inflated keep-outs on the rungs, the true ones at the interpolation to the requested mesh and on it, also after a failed climb
    {
        mx::Alg a = defaults();
        a.inflate_keepouts = true;
        auto grown = [&](size_t m) { const double r0 = std::sqrt(1.0) + 0.5 * span * 1.5707963267948966 / (double)(m - 1); return r0 * r0; };
        const Outcome o = run("10 inflated keep-outs", a, 129, sequence({OK, FAIL}, OK));
        expect(runs(o) == "33 65! 33 65 129", "runs " + runs(o));
        for (const Call& c : o.calls) expect(c.disc_rsq == (c.nodes == 129 ? 1.0 : grown(c.nodes)), "squared radius on " + std::to_string(c.nodes) + " nodes");
        std::string seen;
        for (const Event& e : o.events) {
            seen += e.kind;
            if (e.kind == 'm' && e.nodes == 129) expect(e.disc_rsq == 1.0, "the interpolation to 129 nodes sees the true radius");
            if (e.kind == 'c') expect(e.nodes == 65 && e.disc_rsq == grown(65), "the 65-node rung is configured with its inflated radius");
        }
        expect(seen == "msmcsmsmcsms", "events " + seen);
        expect(grown(33) > grown(65) && grown(65) > 1.0, "the inflation shrinks with the mesh");
    }
    // multipliers are carried to the next mesh only with Alg::warm_multipliers, by the covector mapping
    {
        mx::Alg a = defaults();
        const Outcome o = run("warm multipliers off", a, 129, sequence({}, OK));
        for (const Call& c : o.calls) expect(c.lam0_err == -1, "no multiplier guess without Alg::warm_multipliers");
        a.warm_multipliers = true;
        const Outcome o2 = run("warm multipliers", a, 129, sequence({}, OK));
        expect(o2.calls.size() == 3 && o2.calls[0].lam0_err == -1, "the cold start has no multiplier guess");
        for (size_t i = 1; i < o2.calls.size(); ++i)
            expect(o2.calls[i].lam0_err >= 0 && o2.calls[i].lam0_err < 1e-12, "call " + std::to_string(i) + ": constant costates arrive as the new mesh's weights");
    }
    std::printf(failures ? "%d FAILURES\n" : "mesh driver: ok\n", failures);
    return failures ? 1 : 0;
}
