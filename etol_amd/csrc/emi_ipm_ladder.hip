// emi_ipm_ladder.hip -- the mesh ladder of a context's whole batch (emi_ipm_solve_ladder_*): prolongation between LGL meshes,
// the repair of a guess that lies inside keep-outs, and the driver that takes the B instances from rung to rung.
//
//   emi_prolong_matrix       host: P[Mf][Mc], row q = the Lagrange basis polynomials of the coarse nodes at tau_f[q] (barycentric
//                            second form, weights (-1)^j sqrt(w_j): interp_lgl of host/eMI355X.cpp as a matrix)
//   emi_prolong_kernel       Vf[r][q] = sum_j PT[j][q] Vc[r][j]: a thread owns one fine node and PROLONG_ROWS rows, reads PT[j][q]
//                            once per j (coalesced along q), the coarse values as wave-uniform loads, and accumulates with fma
//                            in ascending j.  One writer per output; a row's bits depend on nothing but the row and P.
//   emi_repair_guess_kernel  mi355x::repair_guess (host/eMI355X.cpp) with one thread per (instance, interior node): nodes do not
//                            interact, so the sweeps of a node are the host's sweeps of that node.  Contraction off.
//   ipm_solve_ladder         per rung: emi_lgl + emi_set_mesh, emi_set_path where the rung brings a table, prolongation of X and U
//                            from the previous rung's final iterate, the repair where asked for, emi_ipm_solve_shard_dev.  Nothing
//                            of a trajectory's size crosses to the host between rungs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "emi_ctx.hpp"

namespace emi {
namespace {

constexpr int PROLONG_T = 256;      // fine nodes per block
constexpr int PROLONG_ROWS = 4;     // rows per thread
constexpr int REPAIR_T = 256;

__global__ __launch_bounds__(PROLONG_T) void emi_prolong_kernel(const double* __restrict__ PT, const double* __restrict__ Vc,
                                                                double* __restrict__ Vf, int Mc, int Mf, int R) {
    const int q = blockIdx.x * PROLONG_T + threadIdx.x;
    if (q >= Mf) return;
    for (int r0 = blockIdx.y * PROLONG_ROWS; r0 < R; r0 += gridDim.y * PROLONG_ROWS) {
        const double* v[PROLONG_ROWS];
        double acc[PROLONG_ROWS];
#pragma unroll
        for (int i = 0; i < PROLONG_ROWS; ++i) {
            v[i] = Vc + (size_t)(r0 + i < R ? r0 + i : r0) * Mc;        // a row past the end reads the group's first (not stored)
            acc[i] = 0.0;
        }
        for (int j = 0; j < Mc; ++j) {
            const double p = PT[(size_t)j * Mf + q];
#pragma unroll
            for (int i = 0; i < PROLONG_ROWS; ++i) acc[i] = fma(p, v[i][j], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < PROLONG_ROWS; ++i)
            if (r0 + i < R) Vf[(size_t)(r0 + i) * Mf + q] = acc[i];
    }
}

__global__ __launch_bounds__(REPAIR_T) void emi_repair_guess_kernel(RepairArgs a) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * REPAIR_T + threadIdx.x, b = blockIdx.y;
    if (k < 1 || k + 1 >= a.M) return;                      // end nodes are never touched
    double* xp = a.X + ((size_t)b * a.ns + a.px) * a.M + k;
    double* yp = a.X + ((size_t)b * a.ns + a.py) * a.M + k;
    const double* recs = a.recs + (size_t)(a.path_sets > 1 ? b : 0) * a.np * EMI_PATH_REC;
    const int tset = a.track_sets > 1 ? b : 0;
    const double margin = 0.05;
    double x = *xp, y = *yp;
    bool any = false;
    for (int sweep = 0; sweep < 50; ++sweep) {
        bool moved = false;
        for (int j = 0; j < a.np; ++j) {
            const double* r = recs + (size_t)j * EMI_PATH_REC;
            const int kind = (int)r[0];
            double xc, yc, ct = 1, st = 0, asq, bsq;
            if (kind == EMI_PATH_ELLIPSE) { xc = r[1]; yc = r[2]; ct = r[3]; st = r[4]; asq = r[5]; bsq = r[6]; }
            else if (kind == EMI_PATH_DISC) { xc = r[1]; yc = r[2]; asq = bsq = r[3]; }
            else {
                const int t = (int)r[1];
                if (t < 0 || t >= a.ntracks) continue;
                const size_t off = ((size_t)tset * a.ntracks + t) * a.M + k;
                xc = a.trkx[off]; yc = a.trky[off]; asq = bsq = r[2];
            }
            if (!(asq > 0) || !(bsq > 0)) continue;
            const double dx = x - xc, dy = y - yc;
            double ex = ct * dx - st * dy, ey = st * dx + ct * dy;
            const double q = ex * ex / asq + ey * ey / bsq;
            if (q >= 1.0 + 0.5 * margin) continue;
            if (q < 1e-12) { ex = 0; ey = sqrt(bsq * (1.0 + margin)); }        // dead centre: minor axis
            else { const double g = sqrt((1.0 + margin) / q); ex *= g; ey *= g; }
            x = xc + ct * ex + st * ey;
            y = yc - st * ex + ct * ey;
            moved = true;
        }
        if (!moved) break;
        any = true;
    }
    if (any) { *xp = x; *yp = y; }
}

}  // namespace

hipError_t launch_prolong(const double* PT, const double* Vc, double* Vf, int Mc, int Mf, int R, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    const int groups = (R + PROLONG_ROWS - 1) / PROLONG_ROWS;
    const dim3 grid((Mf + PROLONG_T - 1) / PROLONG_T, groups < 65535 ? groups : 65535);
    hipLaunchKernelGGL(emi_prolong_kernel, grid, dim3(PROLONG_T), 0, s, PT, Vc, Vf, Mc, Mf, R);
    return hipGetLastError();
}

hipError_t launch_repair_guess(const RepairArgs& a, hipStream_t s) {
    if (a.np <= 0 || a.M <= 2 || a.B <= 0) return hipSuccess;
    if (a.B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(emi_repair_guess_kernel, dim3((a.M + REPAIR_T - 1) / REPAIR_T, a.B), dim3(REPAIR_T), 0, s, a);
    return hipGetLastError();
}

// the arrays of the ladder between its rungs: P transposed for the present pair of rungs, two sets of iterates (the rung being
// solved and the one before it), the multipliers of the rungs below the last
struct IpmLadderWs {
    DeviceArray<double> PT, X[2], U[2], LamF, LamC;
};

void ipm_ladder_destroy(IpmLadderWs* w) { delete w; }

#define L_HIP(call) HIP_TRY_AS(c, "emi_ipm_solve_ladder_dev", call)
#define L_TRY EMI_TRY

int ipm_solve_ladder(emi_ctx_t c, int nrungs, const emi_ipm_rung_t* rungs, double t0, double tf, const void* dX0, const void* dU0, void* dX,
                     void* dU, void* dLamF, void* dLamC, emi_ipm_result_t* results) {
    if (!c->ipm_ladder) c->ipm_ladder = new IpmLadderWs();
    IpmLadderWs& w = *c->ipm_ladder;
    const size_t B = (size_t)c->B, ns = (size_t)c->ns, nc = (size_t)c->nc, np = (size_t)emi_api::np_total(c);
    const hipStream_t s = c->stream;
    std::vector<double> tau, wt, D, tau_c, w_c, P, PT;
    const void *pX = nullptr, *pU = nullptr;        // the previous rung's final iterate
    for (int r = 0; r < nrungs; ++r) {
        const emi_ipm_rung_t& g = rungs[r];
        const int M = g.M, Mc = r > 0 ? rungs[r - 1].M : 0;
        const bool last = r + 1 == nrungs;
        tau.resize(M); wt.resize(M); D.resize((size_t)M * M);
        L_TRY(emi_lgl(M, tau.data(), wt.data(), D.data()));
        L_TRY(emi_set_mesh(c, M, tau.data(), wt.data(), D.data(), t0, tf));
        if (g.recs) L_TRY(emi_set_path(c, c->np, c->path_sets, g.recs, c->px, c->py));
        // where this rung's iterate lives: the caller's arrays on the last rung, else one of the two sets (not the previous rung's)
        void *cX = dX, *cU = dU, *cLF = dLamF, *cLC = dLamC;
        if (!last) {
            L_HIP(hipStreamSynchronize(s));             // a launch in flight may still use an array that has to move
            L_HIP(w.X[r & 1].reserve(B * ns * M)); L_HIP(w.U[r & 1].reserve(B * nc * M));
            L_HIP(w.LamF.reserve(B * ns * M)); L_HIP(w.LamC.reserve(B * np * M));
            cX = w.X[r & 1].p; cU = w.U[r & 1].p; cLF = w.LamF.p; cLC = w.LamC.p;
        }
        if (r == 0) {
            L_HIP(hipMemcpyAsync(cX, dX0, B * ns * M * sizeof(double), hipMemcpyDeviceToDevice, s));
            if (nc > 0) L_HIP(hipMemcpyAsync(cU, dU0, B * nc * M * sizeof(double), hipMemcpyDeviceToDevice, s));
        } else {
            P.resize((size_t)M * Mc); PT.resize((size_t)M * Mc);
            L_TRY(emi_prolong_matrix(Mc, tau_c.data(), w_c.data(), M, tau.data(), P.data()));
            for (int q = 0; q < M; ++q)
                for (int j = 0; j < Mc; ++j) PT[(size_t)j * M + q] = P[(size_t)q * Mc + j];
            L_HIP(hipStreamSynchronize(s));
            L_HIP(w.PT.reserve(PT.size()));
            L_HIP(hipMemcpyAsync(w.PT.p, PT.data(), PT.size() * sizeof(double), hipMemcpyHostToDevice, s));
            L_HIP(hipStreamSynchronize(s));             // (PT is rewritten for the next pair)
            L_TRY(emi_prolong_dev(c, Mc, M, w.PT.p, pX, c->B * c->ns, cX));
            if (nc > 0) L_TRY(emi_prolong_dev(c, Mc, M, w.PT.p, pU, c->B * c->nc, cU));
        }
        if (g.repair) L_TRY(emi_repair_guess_dev(c, cX));
        L_TRY(emi_ipm_solve_shard_dev(c, cX, cU, &g.bd, &g.opt, cLF, cLC, results + (size_t)r * B));
        pX = cX; pU = cU;
        tau_c.swap(tau); w_c.swap(wt);
    }
    return EMI_OK;
}

}  // namespace emi

extern "C" int emi_prolong_matrix(int Mc, const double* tau_c, const double* w_c, int Mf, const double* tau_f, double* P) {
#pragma clang fp contract(off)
    if (Mc < 2 || Mf < 2 || !tau_c || !w_c || !tau_f || !P) return EMI_ERR_ARG;
    for (int q = 0; q < Mf; ++q) {
        double* row = P + (size_t)q * Mc;
        int hit = -1;
        double den = 0.0;
        for (int j = 0; j < Mc; ++j) {
            const double dlt = tau_f[q] - tau_c[j];
            if (dlt == 0.0) { hit = j; break; }
            row[j] = ((j & 1) ? -1.0 : 1.0) * std::sqrt(w_c[j]) / dlt;
            den += row[j];
        }
        for (int j = 0; j < Mc; ++j) row[j] = hit >= 0 ? (j == hit ? 1.0 : 0.0) : row[j] / den;
    }
    return EMI_OK;
}
