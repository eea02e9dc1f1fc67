// etol_harness_param_table.cpp -- test shim of the per-instance parameter table (emi_set_model_params_batch): the text of a TRACED
// quadrotor whose mass, inertia, gravity and cost weights are entries of the model's parameter block (IN_PARAM inputs of the trace,
// P.p[i] in the generated struct) instead of constants.  Host-only: what tests/test_gpu_param_table.py hands emi_set_model_source.
#include <string>
#include <vector>

#include "emi_trace.hpp"

namespace mx = ETOL::mi355x;

namespace {
std::string g_text;
}

// x = (px, pz, theta, vx, vz, omega), u = (T, tau), p = {mass, inertia, gravity, w_thrust, w_torque}: the equations of
// EMI_MODEL_QUADROTOR2D (etol_amd/csrc/emi_models.hpp), first and second derivatives by the trace
extern "C" const char* harness_param_table_traced_quad_source(void) {
    mx::Trace& tr = mx::Trace::active();
    tr.clear();
    auto par = [&](int i) { mx::Var v; v.kind = mx::Var::EXPR; v.node = tr.input(mx::Trace::IN_PARAM, i); return v; };
    std::vector<mx::Var> x, u;
    for (size_t i = 0; i < 6; ++i) x.push_back(mx::Var(mx::Var::STATE, i));
    for (size_t j = 0; j < 2; ++j) u.push_back(mx::Var(mx::Var::CONTROL, j));
    const mx::Var m = par(0), I = par(1), g = par(2), wT = par(3), wq = par(4);
    std::vector<mx::Var> f(6);
    f[0] = x[3];
    f[1] = x[4];
    f[2] = x[5];
    f[3] = -(u[0] / m) * mx::sin(x[2]);
    f[4] = (u[0] / m) * mx::cos(x[2]) - g;
    f[5] = u[1] / I;
    const mx::Var L = wT * u[0] * u[0] + wq * u[1] * u[1];
    std::vector<int> fn;
    for (const mx::Var& fi : f) fn.push_back(fi.node);
    g_text = tr.generate_model("TracedModel", 6, 2, fn, L.node);
    return g_text.c_str();
}
