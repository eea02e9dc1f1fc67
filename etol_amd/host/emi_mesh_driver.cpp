// emi_mesh_driver.cpp -- the mesh strategy of eMI355X::solve() as one object with named phases (emi_mesh_driver.hpp).
#include "emi_mesh_driver.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "emi_transcribe.hpp"

namespace ETOL {
namespace mi355x {

namespace {
[[noreturn]] void die(const char* msg) {
    fprintf(stderr, "eMI355X: %s\n", msg);
    exit(EXIT_FAILURE);
}
// sideways offsets of the straight-line guess, as fractions of the span: the starts after the line (and the planned route)
const double kBends[4] = {0.15, -0.15, 0.35, -0.35};

// Barycentric Lagrange interpolation from the LGL nodes (tau, w) to the points t2.  For LGL
// nodes the barycentric weights are (-1)^j sqrt(w_j) up to a common factor, because
// w_j = 2 / (N (N+1) P_N(tau_j)^2) and the Lagrange weights are proportional to 1 / P_N(tau_j).
void interp_lgl(const std::vector<double>& tau, const std::vector<double>& w, const double* v, size_t M,
                const std::vector<double>& t2, double* out) {
    for (size_t q = 0; q < t2.size(); ++q) {
        double num = 0, den = 0;
        bool hit = false;
        for (size_t j = 0; j < M; ++j) {
            const double d = t2[q] - tau[j];
            if (d == 0.0) { out[q] = v[j]; hit = true; break; }
            const double lam = ((j & 1) ? -1.0 : 1.0) * std::sqrt(w[j]) / d;
            num += lam * v[j];
            den += lam;
        }
        if (!hit) out[q] = num / den;
    }
}
}  // namespace

double boundary_span(const Prob& P) {
    const size_t ns = P.nstates;
    if (P.event_lower.size() != 2 * ns) return 0;
    const double dx = 0.5 * (P.event_lower[ns + P.px] + P.event_upper[ns + P.px]) - 0.5 * (P.event_lower[P.px] + P.event_upper[P.px]);
    const double dy = 0.5 * (P.event_lower[ns + P.py] + P.event_upper[ns + P.py]) - 0.5 * (P.event_lower[P.py] + P.event_upper[P.py]);
    return std::sqrt(dx * dx + dy * dy);
}

MeshDriver::MeshDriver(Prob& P, const Alg& alg, Sol& sol, MeshHost& host, const NlpOptions& opt)
    : P_(P), alg_(alg), sol_(sol), host_(host), ns_(P.nstates), nc_(P.ncontrols), opt_(opt), warm_(opt), target_(P.nodes),
      true_records_(P.path_records), span_(boundary_span(P)) {
    if (alg.scaling == "automatic") scale_by_bounds_ = true;
    else if (alg.scaling != "none") die("Alg::scaling must be \"automatic\" or \"none\"");
    if (alg.defect_scaling == "jacobian-based") jacobian_defect_scaling_ = true;
    else if (alg.defect_scaling != "state-based") die("Alg::defect_scaling must be \"state-based\" or \"jacobian-based\"");
    // started from an interpolated solution: stay close to it
    warm_.mu_init = alg.warm_mu_init;                    // (1e-3 .. 1e-5 measured, profiles/r01_notes.md)
    warm_.bound_push = warm_.bound_frac = alg.warm_bound_push;
    warm_.mu_restart = alg.mu_restart;
}

NlpResult MeshDriver::run() {
    P_.guess_clearance = alg_.plan_clearance;
    sol_.mesh_iterations = 0;
    sol_.nlp_iterations_total = 0;
    sol_.nlp_runs.clear();
    sol_.certificate = Sol::Certificate();
    sol_.lamF.clear();
    sol_.lamC.clear();
    sol_.ode_error = 0;
    // Mesh sequencing: a fine global mesh is reached through coarse ones (33, 65, 129, ... nodes), each
    // solve started from the interpolated previous solution.  An interior-point iteration from a cold
    // straight-line guess needs hundreds of Newton steps on a 1000-node mesh; from the interpolant of the
    // next-coarser solution it needs a few dozen, and the coarse solves cost next to nothing.
    // (PSOPT's own remedy is the same idea driven by the error estimate: start coarse, refine.)
    if (alg_.mesh_sequencing && P_.nodes > 80 && P_.guess_states.empty() && !P_.lifted) {
        plan_ladder();
        sequenced_ = run_ladder();
    }
    refine_loop();
    return r_;
}

// ---------------------------------------------------------------------------------------------
// one NLP solve
// ---------------------------------------------------------------------------------------------
void MeshDriver::solve_on_current_mesh(const NlpOptions& o) {
    NlpProblem nlp = make_nlp(P_, nullptr);
    if (scale_by_bounds_) nlp.vscale = bound_scales(P_);
    nlp.jacobian_defect_scaling = jacobian_defect_scaling_;
    if (P_.guess_lamF.size() == ns_ * P_.nodes) nlp.lamF0 = P_.guess_lamF;
    if (P_.guess_lamC.size() == P_.npath * P_.nodes) nlp.lamC0 = P_.guess_lamC;
    NlpOptions ob = o;
    if (alg_.nlp_iter_budget > 0) {           // what is left of the solve()'s iteration budget
        const int left = alg_.nlp_iter_budget - sol_.nlp_iterations_total;
        if (left <= 0) {
            r_ = NlpResult();
            r_.msg = "iteration budget exhausted (" + std::to_string(sol_.nlp_iterations_total) + " iterations over all meshes and restarts)";
            return;
        }
        ob.max_iter = std::min(ob.max_iter, left);
    }
    const auto t_run = std::chrono::steady_clock::now();
    r_ = host_.solve_nlp(nlp, ob, initial_guess(P_));
    sol_.nlp_iterations_total += r_.iterations;
    sol_.node_blocks = r_.n_factor_terms > 0 ? "device" : "host";
    sol_.nlp_runs.push_back({P_.nodes, r_.iterations, r_.ok, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_run).count(),
                             r_.t_eval, r_.t_hess, r_.t_factor, r_.t_solve, r_.t_lowrank, r_.t_blocks, r_.t_jt, r_.t_matvec, r_.n_factor, r_.n_solve});
    if (!r_.ok && alg_.nlp_iter_budget > 0 && sol_.nlp_iterations_total >= alg_.nlp_iter_budget)
        r_.msg = "iteration budget exhausted (" + std::to_string(sol_.nlp_iterations_total) + " iterations over all meshes and restarts); last: " + r_.msg;
}

// A warm start that wanders (no failure, just hundreds of regularised steps along a flat valley; Monte-Carlo scenario 10 of
// profiles/r02_notes.md section 12) is cut off after Alg::warm_patience iterations and repeated from the same interpolated
// guess with a 10 x larger barrier parameter
void MeshDriver::warm_start(const NlpOptions& o) {
    if (alg_.warm_patience <= 0 || alg_.warm_patience >= o.max_iter) { solve_on_current_mesh(o); return; }
    NlpOptions first = o;
    first.max_iter = alg_.warm_patience;
    solve_on_current_mesh(first);
    if (r_.ok || r_.iterations < first.max_iter) return;                  // converged, or ended for another reason
    if (alg_.print_level >= 5)
        printf("warm start still running after %d iterations: again from the same guess with barrier parameter %.1e\n",
               first.max_iter, 10.0 * o.mu_init);
    NlpOptions again = o;
    again.mu_init = 10.0 * o.mu_init;
    solve_on_current_mesh(again);
}

// A cold start that ends locally infeasible (the path rows stay violated whatever the penalty weight: the iterate
// sits on the wrong side of a keep-out) is repeated from the straight line bent to either side, by 15 % and 35 %
// of its length.  IPOPT's restoration phase does this job for ePSOPT; here it is a search over homotopy classes,
// decided by the first start that converges.  Only for the default guess: a user's guess is taken as given.
void MeshDriver::cold_start_with_retries(const NlpOptions& o) {
    solve_on_current_mesh(o);
    if (r_.ok || P_.npath == 0 || !P_.guess_states.empty() || alg_.guess_retries <= 0) return;
    const bool outer_planned = P_.guess_planned;          // (a ladder climb that starts from the planned route: the bends follow without it)
    P_.guess_planned = false;
    for (int t = 0; t < 4 && t < alg_.guess_retries && !r_.ok && span_ > 0; ++t) {
        P_.guess_bend = kBends[t] * span_;
        if (alg_.print_level >= 5) printf("cold start failed (%s): retrying from the line bent by %+.3f\n", r_.msg.c_str(), P_.guess_bend);
        solve_on_current_mesh(o);
    }
    P_.guess_bend = 0;
    // ... and last from a route planned through the free space of the static keep-outs (planned_path_guess), unless this cold start
    // already began from it (a ladder climb's second start, Alg::plan_second_start).
    if (!r_.ok && span_ > 0 && !outer_planned) {
        P_.guess_planned = true;
        if (alg_.print_level >= 5) printf("cold start failed (%s): retrying from a path planned through the free space\n", r_.msg.c_str());
        solve_on_current_mesh(o);
    }
    P_.guess_planned = outer_planned;
}

// ---------------------------------------------------------------------------------------------
// meshes
// ---------------------------------------------------------------------------------------------
void MeshDriver::clear_guess() {
    for (std::vector<double>* g : {&P_.guess_states, &P_.guess_controls, &P_.guess_lamF, &P_.guess_lamC}) g->clear();
}

// the solution on the current mesh, interpolated to Mnew LGL nodes, becomes the guess there
void MeshDriver::remesh_with_guess(size_t Mnew) {
    const std::vector<double> tau = P_.tau, w = P_.w;
    const size_t M = P_.nodes, ns = ns_, nc = nc_;
    host_.set_mesh(Mnew);
    P_.guess_states.assign(ns * Mnew, 0.0);
    P_.guess_controls.assign(nc * Mnew, 0.0);
    for (size_t i = 0; i < ns; ++i) interp_lgl(tau, w, &r_.z[i * M], M, P_.tau, &P_.guess_states[i * Mnew]);
    // the interpolant may cut through a keep-out between two old nodes
    repair_guess(P_, &P_.guess_states[P_.px * Mnew], &P_.guess_states[P_.py * Mnew]);
    for (size_t j = 0; j < nc; ++j) {
        interp_lgl(tau, w, &r_.z[(ns + j) * M], M, P_.tau, &P_.guess_controls[j * Mnew]);
        for (size_t k = 0; k < Mnew; ++k)
            P_.guess_controls[j * Mnew + k] =
                std::min(std::max(P_.guess_controls[j * Mnew + k], P_.control_lower[j]), P_.control_upper[j]);
    }
    // Multipliers are NOT carried to the next mesh by default: measured over 32 Monte-Carlo scenarios at 257 nodes the
    // costate-mapped warm start needed 112 iterations on average against 103 from zero multipliers (interior-point
    // warm starts want centred pairs, which interpolated multipliers are not).  Alg::warm_multipliers enables it:
    // lambda_k / w_k samples the costate (covector mapping of pseudospectral methods), which is what
    // interpolates between meshes; the row multipliers of the keep-outs likewise
    P_.guess_lamF.clear();
    P_.guess_lamC.clear();
    if (alg_.warm_multipliers && r_.lamF.size() == ns * M && r_.lamC.size() == P_.npath * M) {
        std::vector<double> tmp(M);
        auto carry = [&](const std::vector<double>& lam, size_t rows, std::vector<double>& guess) {
            guess.assign(rows * Mnew, 0.0);
            for (size_t i = 0; i < rows; ++i) {
                for (size_t k = 0; k < M; ++k) tmp[k] = lam[i * M + k] / w[k];
                interp_lgl(tau, w, tmp.data(), M, P_.tau, &guess[i * Mnew]);
                for (size_t k = 0; k < Mnew; ++k) guess[i * Mnew + k] *= P_.w[k];
            }
        };
        carry(r_.lamF, ns, P_.guess_lamF);
        carry(r_.lamC, P_.npath, P_.guess_lamC);
    }
}

// Constraints hold at the nodes only, so a coarse mesh can step over a thin keep-out ("tunnelling") and leave
// the finer meshes a start on the wrong side of it.  On the ladder the keep-outs of the record table are
// therefore inflated by half the largest node spacing of the straight line between the boundary positions
// (LGL nodes are (pi/2) / (m-1) of the span apart at mid-horizon); the requested mesh gets the true sizes back.
void MeshDriver::inflate_records(size_t m) {
    P_.path_records = true_records_;
    if (!alg_.inflate_keepouts || !(span_ > 0)) return;
    const double delta = 0.5 * span_ * 1.5707963267948966 / (double)(m - 1);
    for (size_t j = 0; j < P_.npath - P_.npath_traced; ++j) {
        double* rec = &P_.path_records[j * EMI_PATH_REC];
        const int kind = (int)rec[0];
        auto grow = [&](double& sq) { const double r0 = std::sqrt(std::max(sq, 0.0)) + delta; sq = r0 * r0; };
        if (kind == EMI_PATH_ELLIPSE) { grow(rec[5]); grow(rec[6]); }
        else if (kind == EMI_PATH_DISC) grow(rec[3]);
        else grow(rec[2]);
    }
}

// ---------------------------------------------------------------------------------------------
// the ladder
// ---------------------------------------------------------------------------------------------
// start k of a climb: 0 the straight line, then (Alg::plan_second_start, if there is one) the planned route, then the bends
// (Alg::plan_first_start: the planned route FIRST and the straight line second)
MeshDriver::Start MeshDriver::start(int k) const {
    const int b = k - 1 - (has_plan_ ? 1 : 0);
    return {has_plan_ && k == (alg_.plan_first_start ? 0 : 1), (b >= 0 && b < 4) ? kBends[b] : 0.0};
}

// the ladder can be climbed once more: from a start no climb has used yet (the climb is deterministic: none is worth repeating)
// that Alg::guess_retries still allows
bool MeshDriver::ladder_has_unused_start() const {
    return !ladder_.empty() && ladder_tries_ > 1 && !first_rung_failed_ && next_start_ < starts() &&
           next_start_ - (has_plan_ ? 2 : 1) < alg_.guess_retries;
}

void MeshDriver::plan_ladder() {
    const size_t lr = (size_t)std::max(2, alg_.ladder_ratio);
    for (size_t m = 33; m < target_; m = lr * m - (lr - 1)) ladder_.push_back(m);
    // Alg::plan_second_start: the route planned through the free space as the second start of a climb, before the bends.  (The SHORTEST
    // route, which hugs the keep-outs, made things worse in that place: 138.7 against 129.7 iterations per scenario on the 64-scenario
    // set, scenario 960 lost; charged for narrow places it takes that set to 127.0, the 256-scenario set from 135.2 to 125.5, scenario
    // 960 from 870 to 235 iterations and scenario 17 from 685 to 313: profiles/r04_notes.md section 24.)
    if (alg_.plan_second_start) {
        std::vector<double> px(P_.nodes), py(P_.nodes);
        has_plan_ = P_.npath > 0 && span_ > 0 && alg_.guess_retries > 0 && planned_path_guess(P_, px.data(), py.data(), alg_.plan_clearance);
    }
    ladder_tries_ = (P_.npath > 0 && span_ > 0) ? 1 + (has_plan_ ? 1 : 0) + std::min(4, std::max(0, alg_.guess_retries)) : 1;
}

// the ladder from its coarsest mesh with the given start: true if every rung converged (the guess on the requested mesh is then set)
bool MeshDriver::climb(const Start& s) {
    clear_guess();
    warm_.rho_init = opt_.rho_init;
    bool ok = true;
    for (size_t li = 0; li < ladder_.size() && ok; ++li) {
        inflate_records(ladder_[li]);
        if (li == 0) host_.set_mesh(ladder_[0]);
        else host_.reconfigure();
        NlpOptions o = li == 0 ? opt_ : warm_;
        o.tol = std::max(opt_.tol, alg_.rung_tolerance);          // intermediate meshes only feed the next guess
        if (li > 0 && alg_.rung_patience > 0) o.max_iter = std::min(o.max_iter, alg_.rung_patience);
        if (li == 0) {
            P_.guess_bend = s.bend * span_;
            P_.guess_planned = s.planned;
            cold_start_with_retries(o);
            P_.guess_bend = 0;
            P_.guess_planned = false;
        } else {
            warm_start(o);
        }
        ++sol_.mesh_iterations;
        if (alg_.print_level >= 5)
            printf("mesh sequencing: %zu nodes, %d iterations, cost %.10e (%s)\n", P_.nodes, r_.iterations, r_.cost,
                   r_.msg.c_str());
        ok = r_.ok;
        warm_.rho_init = std::max(warm_.rho_init, r_.rho);     // a penalty weight found too small stays raised
        if (ok) {
            if (li + 1 == ladder_.size()) P_.path_records = true_records_;       // the guess repair below sees the true sizes
            remesh_with_guess(li + 1 < ladder_.size() ? ladder_[li + 1] : target_);
        } else if (li == 0) {
            first_rung_failed_ = true;                   // the cold start already went through its own bends
        }
    }
    P_.path_records = true_records_;
    return ok;
}

// A rung that fails after the coarsest one converged (the interpolant runs into a corner the coarse mesh did not
// see) sends the whole ladder back to its start with the next start: a cold start on 33 nodes costs a quarter of a
// second, whereas the fallback -- cold starts on the requested mesh -- spent 4 x 400 iterations of a 513-node problem
// on one Monte-Carlo scenario (36 of its 41 s, profiles/r02_notes.md).  False: no climb got through, and the requested
// mesh is set up for a cold start.
bool MeshDriver::run_ladder() {
    bool chain_ok = false;
    for (int ca = 0; ca < ladder_tries_ && !chain_ok && !first_rung_failed_; ++ca) {
        const Start s = start(ca);
        if (ca > 0 && alg_.print_level >= 5) {
            if (s.planned) printf("mesh sequencing: a rung failed (%s), ladder restarted from the route planned through the free space\n", r_.msg.c_str());
            else printf("mesh sequencing: a rung failed (%s), ladder restarted from the line bent by %+.3f\n", r_.msg.c_str(), s.bend * span_);
        }
        chain_ok = climb(s);
        next_start_ = ca + 1;
    }
    if (!chain_ok) {
        host_.set_mesh(target_);
        clear_guess();
    }
    return chain_ok;
}

// ---------------------------------------------------------------------------------------------
// the requested mesh and beyond
// ---------------------------------------------------------------------------------------------
// The warm start on the requested mesh, while the ladder still has a start it has not used: at most Alg::target_patience iterations
// (converged ones take 11 at the median, 24 at the 90th percentile, 212 at most over 256 Monte-Carlo scenarios; the one that fails used
// all 400 of nlp_iter_max -- 20 s of a 1024-node problem -- before the next start got its turn: scenario 558, r04_notes.md section 26)
void MeshDriver::target_warm() {
    NlpOptions w = warm_;
    if (alg_.target_patience > 0 && ladder_has_unused_start()) w.max_iter = std::min(w.max_iter, alg_.target_patience);
    warm_start(w);
    ++sol_.mesh_iterations;
}

// The ladder led into a corner (typically an interpolant cutting through a keep-out the coarse meshes did not see): the ladder again
// from the first start it has not been climbed with yet (a Monte-Carlo scenario whose climb from the +15 % bend ended in a failed
// warm start used to climb from +15 % AGAIN, to the same failure, 117 iterations later), and when the starts are used up, a cold
// start on the requested mesh from the default guess.
void MeshDriver::restart_after_failed_target() {
    while (ladder_has_unused_start() && !r_.ok) {
        const Start s = start(next_start_++);
        if (alg_.print_level >= 5) {
            if (s.planned) printf("mesh sequencing: warm start on %zu nodes failed (%s), ladder restarted from the planned route\n", target_, r_.msg.c_str());
            else printf("mesh sequencing: warm start on %zu nodes failed (%s), ladder restarted from the line bent by %+.3f\n", target_, r_.msg.c_str(), s.bend * span_);
        }
        if (climb(s)) target_warm();
    }
    if (r_.ok) return;
    if (P_.nodes != target_) host_.set_mesh(target_);
    if (alg_.print_level >= 5) printf("mesh sequencing: warm start failed (%s), cold start on %zu nodes\n", r_.msg.c_str(), P_.nodes);
    clear_guess();
    cold_start_with_retries(opt_);
    ++sol_.mesh_iterations;
}

// PSOPT's mesh refinement ("automatic", ePSOPT.cpp:69-71): solve, estimate the ODE error,
// add nodes and re-solve from the interpolated solution until the tolerance is met.
void MeshDriver::refine_loop() {
    // a lifted problem (delays) is refined only where Alg::refine_delayed asks for it: the host takes the estimate of the STATED
    // problem (the delayed values between the nodes are those of the interpolants), the next mesh starts from the interpolated
    // states and free controls, and initial_guess forms the delayed values on it as W . guess, as it does for a cold start
    const bool refine = alg_.mesh_refinement == "automatic" && (!P_.lifted || alg_.refine_delayed);
    // the dense step of a lifted problem takes up to 4000 KKT rows, (2 ns + nc + 2 ndelayed) per node
    const size_t dense_cap = P_.lifted ? 4000 / (2 * ns_ + nc_ + 2 * P_.ndelayed) : (size_t)-1;
    for (int mr = 0;; ++mr) {
        if (mr == 0 && sequenced_) {
            target_warm();
            if (!r_.ok) restart_after_failed_target();
        } else {
            if (mr == 0) cold_start_with_retries(opt_);
            else solve_on_current_mesh(opt_);
            ++sol_.mesh_iterations;
        }
        if (!r_.ok && mr > 0 && r_good_.ok) {
            // a refinement solve that fails does not take the converged coarser solution with it
            if (alg_.print_level >= 5) printf("mesh iteration %d failed (%s): keeping the %zu-node solution\n", mr, r_.msg.c_str(), M_good_);
            host_.set_mesh(M_good_);
            r_ = r_good_;
            break;
        }
        if (!r_.ok || !refine) break;
        sol_.ode_error = host_.ode_error(r_.z);
        if (alg_.print_level >= 5)
            printf("mesh iteration %d: %zu nodes, cost %.10e, relative ODE error %.3e\n", mr, P_.nodes, r_.cost,
                   sol_.ode_error);
        if (sol_.ode_error <= alg_.ode_tolerance || mr + 1 >= alg_.mr_max_iterations) break;
        size_t Mnew = std::min((size_t)alg_.mr_max_nodes, P_.nodes + std::max<size_t>(4, (P_.nodes - 1) / 2));
        if (Mnew > dense_cap) {
            Mnew = dense_cap;
            if (Mnew <= P_.nodes && alg_.print_level >= 1)
                printf("mesh refinement stops on %zu nodes with a relative ODE error of %.3e: the dense Newton step of a problem with delays takes up to "
                       "4000 KKT rows, %zu nodes\n", P_.nodes, sol_.ode_error, dense_cap);
        }
        if (Mnew <= P_.nodes) break;
        // refined meshes start from the interpolated solution but with the cold-start barrier settings: the
        // interpolant may cut through keep-outs between the old nodes, and the elastic rows need room to move
        r_good_ = r_;
        M_good_ = P_.nodes;
        remesh_with_guess(Mnew);
    }
}

}  // namespace mi355x
}  // namespace ETOL
