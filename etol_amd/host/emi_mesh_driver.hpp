// emi_mesh_driver.hpp -- the mesh strategy of eMI355X::solve(): how a cold problem gets onto a fine mesh.
//
// One solve() is one MeshDriver object.  It owns the decisions -- the sequencing ladder 33 -> 65 -> ..., the order of the
// starts of a climb (planned route, straight line, four bends), rung / target / warm patience, the restart of the ladder
// after a failed rung or a failed warm start on the requested mesh, the cold-start retries, the iteration budget of the
// solve(), inflated keep-outs on the rungs, PSOPT-style refinement with fall-back to the last converged mesh -- and asks a
// MeshHost for the four things that need the device.  eMI355X implements the host on its device context; a test
// implements it with a script or with the CPU oracle, so every branch of the strategy runs without a GPU.
//
// Known and untouched here (the driver moves the strategy, it does not change it): a problem with delays is solved
// lifted, for which sequencing and refinement are silently off (eMI355X::solve takes the ODE-error estimate of such a
// solve itself, of the stated problem once the lifted form has ended); planned_path_guess ignores keep-in rows.
#ifndef ETOL_MI355X_EMI_MESH_DRIVER_HPP_
#define ETOL_MI355X_EMI_MESH_DRIVER_HPP_

#include <utility>
#include <vector>

#include <ETOL/eMI355X.hpp>

#include "emi_nlp.hpp"

namespace ETOL {
namespace mi355x {

// What the strategy needs of whoever holds the problem's functions (eMI355X: the device context).
struct MeshHost {
    virtual ~MeshHost() {}
    // the problem on an LGL mesh of `nodes` nodes: Prob::nodes / tau / w / D and the track tables, and the evaluator on them
    virtual void set_mesh(size_t nodes) = 0;
    // Prob::path_records changed (inflated keep-outs of a rung): the evaluator takes the table again
    virtual void reconfigure() = 0;
    // ONE NLP solve on the current mesh from z0.  nlp comes from make_nlp(P, nullptr) with scalings and multiplier guesses
    // set; the host puts in its evaluator and chooses the Newton-step backend for the duration of this call.
    virtual NlpResult solve_nlp(NlpProblem& nlp, const NlpOptions& opt, const std::vector<double>& z0) = 0;
    // relative local ODE error of the trajectory z on the current mesh (the refinement criterion)
    virtual double ode_error(const std::vector<double>& z) = 0;
};

// The guess vectors of the problem are working storage of the driver; the caller's own guess (ePSOPT.cpp:47-56) is put
// back when the guard goes, so that a second solve() starts from it again.
struct KeepGuess {
    Prob& P;
    std::vector<double> gs, gc, lf, lc;
    explicit KeepGuess(Prob& p) : P(p), gs(p.guess_states), gc(p.guess_controls), lf(p.guess_lamF), lc(p.guess_lamC) {}
    ~KeepGuess() { P.guess_states = gs; P.guess_controls = gc; P.guess_lamF = lf; P.guess_lamC = lc; }
};

// distance between the boundary positions (states px, py at t0 and tf, mid-points of their event bounds): the length the
// bends of the straight-line guess and the inflation of the keep-outs are fractions of; 0 without event bounds
double boundary_span(const Prob& P);

class MeshDriver {
 public:
    // opt: the cold-start options of one NLP solve (tolerance, iteration limit, print level, ... from Alg)
    MeshDriver(Prob& P, const Alg& alg, Sol& sol, MeshHost& host, const NlpOptions& opt);
    // every mesh, rung and restart of one solve(); returns the NLP result on the mesh Prob is left on.  Sol receives the
    // bookkeeping of the run (mesh_iterations, nlp_iterations_total, nlp_runs, node_blocks, ode_error), not the answer.
    NlpResult run();

 private:
    struct Start { bool planned; double bend; };        // bend: fraction of the span

    // one NLP solve, into r_
    void solve_on_current_mesh(const NlpOptions& o);
    void warm_start(const NlpOptions& o);
    void cold_start_with_retries(const NlpOptions& o);
    // meshes
    void remesh_with_guess(size_t Mnew);
    void inflate_records(size_t m);
    void clear_guess();
    // the ladder
    Start start(int k) const;
    int starts() const { return 1 + (has_plan_ ? 1 : 0) + 4; }
    bool ladder_has_unused_start() const;
    void plan_ladder();
    bool climb(const Start& s);
    bool run_ladder();
    // the requested mesh and beyond
    void target_warm();
    void restart_after_failed_target();
    void refine_loop();

    Prob& P_;
    const Alg& alg_;
    Sol& sol_;
    MeshHost& host_;
    const size_t ns_, nc_;
    NlpOptions opt_, warm_;             // cold start; started from an interpolated solution (warm_.rho_init follows a climb)
    bool scale_by_bounds_ = false, jacobian_defect_scaling_ = false;       // Alg::scaling / defect_scaling, parsed once
    NlpResult r_;                       // result of the last NLP solve
    const size_t target_;               // the requested mesh
    std::vector<size_t> ladder_;        // rungs below it (empty: no sequencing)
    const std::vector<double> true_records_;
    const double span_;
    int ladder_tries_ = 1;              // climbs the first pass over the ladder may take (1: no second start)
    int next_start_ = 1;                // index of the first start no climb has used yet
    bool has_plan_ = false;             // Alg::plan_second_start, and the static keep-outs leave a route that planned_path_guess finds
    bool first_rung_failed_ = false;    // the coarsest rung went through its own bends and failed: no other start is worth a climb
    bool sequenced_ = false;            // the requested mesh is started from the ladder's solution
    NlpResult r_good_;                  // last converged solution of the refinement and its mesh
    size_t M_good_ = 0;
};

}  // namespace mi355x
}  // namespace ETOL
#endif
