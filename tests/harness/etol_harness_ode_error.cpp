// etol_harness_ode_error.cpp -- extern "C" shim for the tests of Alg::ode_error = "device": ETOL::eMI355X::odeError of a given
// trajectory of the quadrotor problem through emi_ode_error_dev.  Linked into libetol_harness.so; the problem is the one
// harness_ode_error_quadrotor (etol_harness.cpp) sets up (same numbers, built-in model).  Test infrastructure.
#include <ETOL/eMI355X.hpp>

#include <array>
#include <chrono>
#include <string>
#include <vector>

#include "emi_transcribe.hpp"

namespace mx = ETOL::mi355x;

namespace {

struct Quad {
    ETOL::eMI355X solver;
    ETOL::f_t obj, obs;
    std::vector<ETOL::f_t> grad;
};

void quadrotor(Quad& h, int nsteps, double dt, int ndiscs) {
    ETOL::TrajectoryOptimizer* t = &h.solver;
    const std::vector<double> mp = {1.0, 0.01, 9.81, 1.0, 1.0};
    t->setNSteps(nsteps); t->setDt(dt); t->setNStates(6); t->setNControls(2);
    t->setX0({1, 1, 0, 0, 0, 0}); t->setXf({8, 6, 0, 0, 0, 0}); t->setXtol({0.01, 0.01, 0.01, 0.05, 0.05, 0.05});
    t->setXlower({0, 0, -1.2, -6, -6, -4}); t->setXupper({10, 10, 1.2, 6, 6, 4});
    t->setUlower({0, -1.0}); t->setUupper({25, 1.0});
    t->setMaximize(false);
    const std::array<double, 3> all[3] = {{4.0, 3.2, 0.8}, {6.3, 4.4, 0.7}, {2.5, 1.2, 0.4}};
    h.obj = [mp](F_ARGS) -> ETOL::scalar_t { return mx::objective(EMI_MODEL_QUADROTOR2D, mp); };
    t->setObjective(&h.obj);
    h.grad.resize(6);
    std::vector<ETOL::f_t*> gp;
    for (int i = 0; i < 6; ++i) {
        h.grad[i] = [i, mp](F_ARGS) -> ETOL::scalar_t { return mx::derivative(EMI_MODEL_QUADROTOR2D, i, mp); };
        gp.push_back(&h.grad[i]);
    }
    t->setGradient(gp);
    if (ndiscs > 3) ndiscs = 3;
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

}  // namespace

// as harness_ode_error_quadrotor, with Alg::ode_error = "device" (up to 3 discs; the estimate does not read them)
extern "C" int harness_ode_error_quadrotor_dev(int nsteps, double dt, int ndiscs, const double* X, const double* U, double* err) {
    Quad q;
    quadrotor(q, nsteps, dt, ndiscs);
    q.solver.setup();
    q.solver.getAlgorithm()->ode_error = "device";
    const size_t M = nsteps + 1;
    std::vector<double> z(8 * M);
    std::copy(X, X + 6 * M, z.begin());
    std::copy(U, U + 2 * M, z.begin() + 6 * M);
    *err = q.solver.odeError(z);
    q.solver.close();
    return 0;
}

// wall seconds of one odeError call (after a first, untimed one), the mean over reps calls on one solver, by either route
// (tools/ode_error_times.py); device_route 0: Alg::ode_error = "host", 1: "device"
extern "C" int harness_ode_error_quadrotor_seconds(int nsteps, double dt, int device_route, int reps, const double* X, const double* U,
                                                   double* err, double* seconds) {
    Quad q;
    quadrotor(q, nsteps, dt, 0);
    q.solver.setup();
    q.solver.getAlgorithm()->ode_error = device_route ? "device" : "host";
    const size_t M = nsteps + 1;
    std::vector<double> z(8 * M);
    std::copy(X, X + 6 * M, z.begin());
    std::copy(U, U + 2 * M, z.begin() + 6 * M);
    *err = q.solver.odeError(z);
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; ++r) *err = q.solver.odeError(z);
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (reps > 0 ? reps : 1);
    q.solver.close();
    return 0;
}
