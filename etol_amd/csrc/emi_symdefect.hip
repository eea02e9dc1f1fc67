// emi_symdefect.hip -- K4 in its fast form: the defect rows  D.X - h f  in one gfx950 kernel (fp64).
//
//   * D.X on v_mfma_f64_16x16x4_f64, with the flops HALVED by the centro-antisymmetry of the LGL
//     differentiation matrix, D[N-i][N-j] = -D[i][j]:
//          e_j = x_j + x_{N-j},  o_j = x_j - x_{N-j}                        (j < M/2)
//          a_i = sum_j De[i][j] e_j,   b_i = sum_j Do[i][j] o_j             (i < M/2)
//          (D x)_i = a_i + b_i,        (D x)_{N-i} = -a_i + b_i
//     De = (D[i][j] + D[i][N-j])/2, Do = (D[i][j] - D[i][N-j])/2 are built once on the host.
//   * Epilogue: accumulator rows are ordered state-major inside a workgroup (row = state*16 +
//     instance), so one lane holds all NS components of D.X for its (instance, node) pairs: it
//     evaluates f there and writes  defect = D.X - h f  directly.  The MFMA work therefore depends
//     only on X and U and runs BESIDE the streaming node work (emi_kernels.hip), the matrix pipe
//     under the ~1 KB/node of HBM stores.  By default the two go out as ONE launch at every batch
//     size (emi_pass_f64_kernel, emi_symdefect_kernels.hpp): MFMA-role and node-role workgroups in
//     one grid, dealt to the XCDs in the block order of the plan, K slices combined and COST finished
//     in-kernel by ticket.  Which instantiation a launch takes is the form table of emi_pass_plan.hpp
//     (EMI_PASS_FORMS), walked by launch_pass_planned below; the policy that picks it is plan_pass
//     there.  The stand-alone kernels of this file -- the one-workgroup-per-CU ring, the register-staged
//     forms and the state-split ring, concurrent with the node kernel on a second HIP stream or back to
//     back on one -- remain behind "overlap_mode" 1 / 2 and for passes without a Jacobian.
//     (Round 1 measured two single-kernel fusions against the two-stream form and both lost: node work
//     inside the K loop, and roles that all followed one schedule, so that the chip alternated between
//     all-MFMA and all-store phases; profiles/r01_notes.md has the numbers.  The one-launch pass of
//     round 3 gives each role its own workgroups and register budget: profiles/r03_notes.md.)
//
// Workgroup = 256 threads = 4 waves; tile = 16 instances x 64*CT half-indices i (nodes i and N-i);
// each wave owns NS x CT x 2 accumulator tiles (96*CT registers for 6 states), one workgroup per CU.  LDS: two buffers (register prefetch of the next K tile) of E,O [NS*16][18], De,Do
// [64*CT][18] doubles; rows padded to 18 doubles: 16-byte aligned for ds_write_b128, conflict-free for the
// ds_read_b64 fragment reads.  blockIdx -> tile map is XCD-aware: workgroups that share a De/Do
// panel share blockIdx % 8, i.e. one XCD's L2.
//
// Requires M % (128*CT) == 0 and an exactly centro-antisymmetric D (emi_lgl guarantees it; emi_set_mesh
// checks); every other shape takes the general defect kernel of emi_kernels.hip.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "emi_kernels.hpp"
#include "emi_models.hpp"
#include "emi_symdefect_kernels.hpp"

namespace emi {

template <class Model>
static hipError_t launch_symdefect_ring_model(const SymDefectArgs& a, hipStream_t s, bool set_attr) {
    constexpr int NS = Model::NS;
    const int mtiles = (a.B + FUSED_TI - 1) / FUSED_TI, ntiles = (a.M / 2) / 64;
    const size_t lds = (size_t)3 * (2 * NS * FUSED_TI + 2 * 64) * 16 * sizeof(double);
    if (set_attr) {
        hipError_t e = hipFuncSetAttribute((const void*)emi_symdefect_ring_f64_kernel<Model>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 grid(mtiles * ntiles), block(256);
    hipLaunchKernelGGL((emi_symdefect_ring_f64_kernel<Model>), grid, block, lds, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
template <class Model, int CT>
static hipError_t launch_symdefect_model(const SymDefectArgs& a, hipStream_t s, bool set_attr) {
    constexpr int NS = Model::NS, TN = 64 * CT;
    const int mtiles = (a.B + FUSED_TI - 1) / FUSED_TI, ntiles = (a.M / 2) / TN;
    // two LDS buffers of E, O, De, Do tiles: 92 KB (CT=1) / 129 KB (CT=2) for the 6-state model,
    // i.e. one workgroup per CU, which leaves the streaming node kernel's waves room beside it
    const size_t lds = (size_t)2 * (2 * NS * FUSED_TI + 2 * TN) * (FUSED_BK + 2) * sizeof(double);
    if (set_attr) {
        hipError_t e = hipFuncSetAttribute((const void*)emi_symdefect_f64_kernel<Model, CT>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    dim3 grid(mtiles * ntiles), block(256);
    hipLaunchKernelGGL((emi_symdefect_f64_kernel<Model, CT>), grid, block, lds, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// second ring form: SW states per workgroup, 8-deep stages, 16-byte fragment reads, two (or more) workgroups per CU,
// optionally split-K (partial sums through a slab, combined in slice order by a second launch)
template <class Model, int SW>
static hipError_t launch_ring2_model(const SymDefectArgs& a, hipStream_t s) {
    constexpr int NS = Model::NS;
    const int mtiles = (a.B + FUSED_TI - 1) / FUSED_TI, ntiles = (a.M / 2) / 64;
    const size_t lds = (size_t)3 * ((2 * SW * FUSED_TI + 2 * 64 + 63) / 64 * 64) * 8 * sizeof(double);
    static bool attr_done = false;          // per instantiation; a repeated call is harmless
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)emi_symdefect_ring2_f64_kernel<Model, SW>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_done = true;
    }
    const int tiles = mtiles * ntiles * (NS / SW), ks = a.ksplit > 1 ? a.ksplit : 1;
    hipLaunchKernelGGL((emi_symdefect_ring2_f64_kernel<Model, SW>), dim3(tiles * ks), dim3(256), lds, s, a);
    if (ks > 1 && a.tile_ticket == nullptr) hipLaunchKernelGGL((emi_symdefect_combine_kernel<Model, SW>), dim3(tiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <class Model>
static hipError_t launch_ring2_planned(const SymDefectArgs& a, hipStream_t s, const SymPlan& p) {
    constexpr int NS = Model::NS;
    if (p.sw == NS) return launch_ring2_model<Model, NS>(a, s);
    if constexpr (NS > 2 && NS % 2 == 0) {
        if (p.sw == 2) return launch_ring2_model<Model, 2>(a, s);
    }
    if constexpr (NS > 3 && NS % 3 == 0) {
        if (p.sw == 3) return launch_ring2_model<Model, 3>(a, s);
    }
    return launch_ring2_model<Model, 1>(a, s);
}

// ---------------------------------------------------------------------------------------------
// the pass as one launch (emi_pass_f64_kernel): MFMA-role and node-role workgroups interleaved per XCD
template <class Model, int SW, int NST, int BK = 8, int CT = 1, int HS = 1, bool DOP = false>
static hipError_t launch_pass_model(const SymDefectArgs& sa, const NodeArgs<double>& na, hipStream_t s, int res, const PassWorkKey& key, const PassWork* work) {
    constexpr int NS = Model::NS;
    PassArgs a;
    a.s = sa;
    a.n = na;
    const int mtiles = (sa.B + FUSED_TI - 1) / FUSED_TI, ntiles = (sa.M / 2) / (64 * CT);
    const int nm = mtiles * ntiles * (NS / SW) * (sa.ksplit > 1 ? sa.ksplit : 1);
    a.nbx = (na.M + 2 * EMI_NODE_THREADS - 1) / (2 * EMI_NODE_THREADS);
    const int nn = a.nbx * na.B;
    a.nm = nm;
    a.nn = nn;
    a.nm8 = (nm + 7) / 8;
    a.nn8 = ((nn + HS - 1) / HS + 7) / 8;          // node-role WORKGROUPS per XCD: one takes HS chunks
    // the work table the blocks read was built for exactly this grid and these counts, or the launch is an error
    if (!work || key.nm != nm || key.nn != nn || key.nm8 != a.nm8 || key.nn8 != a.nn8 || key.nbx != a.nbx || key.hs != HS || key.nsg != NS / SW ||
        key.ntiles != ntiles || key.ks != (sa.ksplit > 1 ? sa.ksplit : 1) || key.order != sa.mfma_first || key.cpart != sa.cpart || key.cx != sa.cx)
        return hipErrorInvalidValue;
    a.work = work;
    // a ring stage: forward and mirrored x rows, De and Do rows, in whole DMA instructions -- DOP: the x rows only (whole instructions as they are)
    const size_t lds = DOP ? (size_t)NST * (2 * SW * FUSED_TI) * BK * sizeof(double)
                           : (size_t)HS * NST * ((2 * SW * FUSED_TI + 2 * 64 * CT + 63) / 64 * 64) * BK * sizeof(double);
    if (DOP && (!sa.Dfrag || sa.ksplit > 1)) return hipErrorInvalidValue;
    const int st = (na.store_mode >= 0 && na.store_mode <= 3) ? na.store_mode : 0;   // result stores: plain / sc1 (write-through) / non-temporal / nt sc1
    // The KEEP instantiations (na.keep: the node role leaves the model-invariant VALS rows alone) exist for the forms the default
    // dispatch chooses: three ring stages, undivided K range.  The forms only an option reaches write everything, which is always right.
    constexpr bool HAS_KEEP = NST == 3 && HS == 1;
    const bool keep = HAS_KEEP && na.keep;
    // Three resident workgroups per CU (SymPlan::res, "sym_res"): the same kernel with a register allocation that admits a third wave per
    // SIMD, held for the direct-operator forms only (a staged form's LDS never admits a third workgroup); anything else states two.
    const bool res3 = DOP && res == 3;
    auto pick = [&](auto keep_c, auto res_c) {
        constexpr bool K = decltype(keep_c)::value;
        constexpr int R = decltype(res_c)::value;
        return st == 2 ? emi_pass_f64_kernel<Model, SW, 2, 2, NST, BK, CT, HS, K, DOP, R>
             : (st == 1 ? emi_pass_f64_kernel<Model, SW, 2, 1, NST, BK, CT, HS, K, DOP, R>
                        : (st == 3 ? emi_pass_f64_kernel<Model, SW, 2, 3, NST, BK, CT, HS, K, DOP, R> : emi_pass_f64_kernel<Model, SW, 2, 0, NST, BK, CT, HS, K, DOP, R>));
    };
    using res2_t = std::integral_constant<int, 2>;
    using res3_t = std::integral_constant<int, 3>;
    auto kern = pick(std::false_type{}, res2_t{});
    if constexpr (HAS_KEEP) {
        if (keep) kern = pick(std::true_type{}, res2_t{});
    }
    if constexpr (DOP) {
        if (res3) kern = pick(std::false_type{}, res3_t{});
        if constexpr (HAS_KEEP) {
            if (res3 && keep) kern = pick(std::true_type{}, res3_t{});
        }
    }
    static bool attr_done[2][2][4] = {};
    if (!attr_done[res3][keep][st]) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        attr_done[res3][keep][st] = true;
    }
    hipLaunchKernelGGL(kern, dim3(8 * (a.nm8 + a.nn8)), dim3(256 * HS), lds, s, a);
    return hipGetLastError();
}

// The form of the plan, by walking the form table (EMI_PASS_FORMS, emi_pass_plan.hpp): a row is instantiated here and nowhere else, for the
// models its SW class applies to.  plan_pass resolves every plan to a row; a plan that names none is an error, not another kernel.
template <class Model>
static hipError_t launch_pass_planned(const SymDefectArgs& sa, const NodeArgs<double>& na, hipStream_t s, const SymPlan& p, const PassWorkKey& key,
                                      const PassWork* work) {
    constexpr int NS = Model::NS;
#define EMI_PASS_FORM_LAUNCH(CLS, NST, BK, CT, HS, DOP, SLICES, STORES)                                                                   \
    if constexpr (pass_class_applies(CLS, NS)) {                                                                                          \
        if (p.sw == pass_class_sw(CLS, NS) && p.nst == NST && p.bk == BK && p.ct == CT && p.hs == HS && p.dop == DOP && (SLICES || p.ks == 1)) \
            return launch_pass_model<Model, pass_class_sw(CLS, NS), NST, BK, CT, HS, DOP>(sa, na, s, p.res, key, work);                  \
    }
    EMI_PASS_FORMS(EMI_PASS_FORM_LAUNCH)
#undef EMI_PASS_FORM_LAUNCH
    return hipErrorInvalidValue;
}

// the built-in models the pass kernels (and the even/odd MFMA defect kernels) are instantiated for
bool pass_model_supported(int model) { return model == EMI_MODEL_POINTMASS2D || model == EMI_MODEL_QUADROTOR2D; }

hipError_t launch_pass(int model, const SymDefectArgs& sa, const NodeArgs<double>& na, hipStream_t s, const SymPlan& p, const PassWorkKey& key,
                       const PassWork* work) {
    if (model == EMI_MODEL_POINTMASS2D) return launch_pass_planned<PointMass2D<double>>(sa, na, s, p, key, work);
    if (model == EMI_MODEL_QUADROTOR2D) return launch_pass_planned<Quadrotor2D<double>>(sa, na, s, p, key, work);
    return hipErrorInvalidValue;
}

bool fused_supported(int model, int M, int ct) {
    return pass_model_supported(model) && symdefect_shape_ok(M, ct);
}

hipError_t launch_symdefect(int model, const SymDefectArgs& a, hipStream_t s, bool set_attr, int ct, const SymPlan& plan) {
    if (!plan.ring1) {
        if (model == EMI_MODEL_POINTMASS2D) return launch_ring2_planned<PointMass2D<double>>(a, s, plan);
        if (model == EMI_MODEL_QUADROTOR2D) return launch_ring2_planned<Quadrotor2D<double>>(a, s, plan);
        return hipErrorInvalidValue;
    }
    if (ct == 0 || ct >= 4) {
        ct = 3;
        set_attr = true;    // cheap; the attribute bookkeeping of the caller is per requested ct
    }
    if (ct == 3) {   // LDS-DMA ring variant (column tiling as ct == 1)
        if (model == EMI_MODEL_POINTMASS2D) return launch_symdefect_ring_model<PointMass2D<double>>(a, s, set_attr);
        if (model == EMI_MODEL_QUADROTOR2D) return launch_symdefect_ring_model<Quadrotor2D<double>>(a, s, set_attr);
        return hipErrorInvalidValue;
    }
    if (model == EMI_MODEL_POINTMASS2D)
        return ct == 1 ? launch_symdefect_model<PointMass2D<double>, 1>(a, s, set_attr)
                       : launch_symdefect_model<PointMass2D<double>, 2>(a, s, set_attr);
    if (model == EMI_MODEL_QUADROTOR2D)
        return ct == 1 ? launch_symdefect_model<Quadrotor2D<double>, 1>(a, s, set_attr)
                       : launch_symdefect_model<Quadrotor2D<double>, 2>(a, s, set_attr);
    return hipErrorInvalidValue;
}

}  // namespace emi
