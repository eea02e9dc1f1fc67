// emi_kernels_tab.hip -- the TABLED instantiations of the model-templated streaming kernels (emi_node_kernels.hpp) for the built-in
// models, and their launchers: what a context with a per-instance parameter table (emi_set_model_params_batch) runs in place of
// emi_nodes_kernel, emi_hess_kernel and emi_ode_resid_kernel.  The workgroup of instance b reads row b of the table once, by scalar
// loads, where the untabled forms read the set in their argument block; everything behind that read is the same body.
//
// A translation unit of its own: the untabled instantiations of emi_kernels.hip and the pass kernels stay what they were, and the
// two compile side by side.  A context with a table takes the sequential route (emi_pass_plan.hpp), so the node kernel exists here
// with the defect rows and plain stores only: both pack widths, values only / Jacobian / Jacobian without the invariant rows.
#include <hip/hip_runtime.h>
#include "emi_kernels.hpp"
#include "emi_models.hpp"
#include "emi_node_kernels.hpp"

namespace emi {

template <typename T, class Model>
static hipError_t launch_nodes_tab_model(const NodeArgs<T>& a, const T* tab, bool jac, hipStream_t s) {
    const int M = a.M;
    const bool vec2 = (M % 2 == 0);
    const int per_block = EMI_NODE_THREADS * (vec2 ? 2 : 1);
    dim3 grid((M + per_block - 1) / per_block, a.B), block(EMI_NODE_THREADS);
    const bool keep = jac && a.keep;
    const Tabled<NodeArgs<T>, T> t{a, tab};
    if (vec2) {
        if (keep)     hipLaunchKernelGGL((emi_nodes_tab_kernel<T, Model, 2, true, true, true>), grid, block, 0, s, t);
        else if (jac) hipLaunchKernelGGL((emi_nodes_tab_kernel<T, Model, 2, true, true>), grid, block, 0, s, t);
        else          hipLaunchKernelGGL((emi_nodes_tab_kernel<T, Model, 2, false, true>), grid, block, 0, s, t);
    } else {
        if (keep)     hipLaunchKernelGGL((emi_nodes_tab_kernel<T, Model, 1, true, true, true>), grid, block, 0, s, t);
        else if (jac) hipLaunchKernelGGL((emi_nodes_tab_kernel<T, Model, 1, true, true>), grid, block, 0, s, t);
        else          hipLaunchKernelGGL((emi_nodes_tab_kernel<T, Model, 1, false, true>), grid, block, 0, s, t);
    }
    return hipGetLastError();
}

// node kernel with the defect rows (-h f), one table row per instance of the launch; the caller launches launch_cost_finish behind it
template <typename T>
hipError_t launch_nodes_tab(int model, const NodeArgs<T>& a, const T* tab, bool jac, hipStream_t s) {
    if (!tab) return hipErrorInvalidValue;
    switch (model) {
        case 0: return launch_nodes_tab_model<T, PointMass2D<T>>(a, tab, jac, s);
        case 1: return launch_nodes_tab_model<T, Quadrotor2D<T>>(a, tab, jac, s);
        case 2: return launch_nodes_tab_model<T, FixedWing12<T>>(a, tab, jac, s);
    }
    return hipErrorInvalidValue;
}
template hipError_t launch_nodes_tab<double>(int, const NodeArgs<double>&, const double*, bool, hipStream_t);
template hipError_t launch_nodes_tab<float>(int, const NodeArgs<float>&, const float*, bool, hipStream_t);

template <typename T>
hipError_t launch_hess_tab(int model, const HessArgs<T>& a, const T* tab, hipStream_t s) {
    if (!tab) return hipErrorInvalidValue;
    dim3 grid((a.M + EMI_NODE_THREADS - 1) / EMI_NODE_THREADS, a.B), block(EMI_NODE_THREADS);
    const Tabled<HessArgs<T>, T> t{a, tab};
    switch (model) {
        case 0: hipLaunchKernelGGL((emi_hess_kernel<T, PointMass2D<T>, true>), grid, block, 0, s, t); break;
        case 1: hipLaunchKernelGGL((emi_hess_kernel<T, Quadrotor2D<T>, true>), grid, block, 0, s, t); break;
        case 2: hipLaunchKernelGGL((emi_hess_kernel<T, FixedWing12<T>, true>), grid, block, 0, s, t); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_hess_tab<double>(int, const HessArgs<double>&, const double*, hipStream_t);
template hipError_t launch_hess_tab<float>(int, const HessArgs<float>&, const float*, hipStream_t);

hipError_t launch_ode_resid_tab(int model, const OdeResidArgs<double>& a, const double* tab, hipStream_t s) {
    if (!tab) return hipErrorInvalidValue;
    dim3 grid((a.M - 1 + EMI_NODE_THREADS - 1) / EMI_NODE_THREADS, a.B), block(EMI_NODE_THREADS);
    const Tabled<OdeResidArgs<double>, double> t{a, tab};
    switch (model) {
        case 0: hipLaunchKernelGGL((emi_ode_resid_kernel<double, PointMass2D<double>, true>), grid, block, 0, s, t); break;
        case 1: hipLaunchKernelGGL((emi_ode_resid_kernel<double, Quadrotor2D<double>, true>), grid, block, 0, s, t); break;
        case 2: hipLaunchKernelGGL((emi_ode_resid_kernel<double, FixedWing12<double>, true>), grid, block, 0, s, t); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace emi
