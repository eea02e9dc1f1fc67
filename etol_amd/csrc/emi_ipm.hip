// emi_ipm.hip -- the array arithmetic of one interior-point iteration between two evaluator calls, over [instance][node] (fp64, gfx950).
//
// What solve_nlp runs on one core per iteration (host/emi_nlp.cpp: ipm_eliminate_rows, ipm_barrier_diagonal, ipm_fill_rt,
// ipm_build_rhs, ipm_expand_step, ipm_step_lengths, ipm_dphi_mmax, ipm_slack_reset, ipm_barrier_merit, ipm_update_duals,
// ipm_kkt_error), for a whole batch, device memory in and out:
//
//   emi_ipm_reduce_kernel   (s, e+, e-) of every path row eliminated, barrier diagonal, right-hand side of the reduced system
//   emi_ipm_expand_kernel   every eliminated step component from the solved step; step lengths, dphi and mmax as partials
//   emi_ipm_trial_kernel    trial point = point + alpha step
//   emi_ipm_merit_kernel    slack reset (optional), barrier function and l1 infeasibility as partials
//   emi_ipm_accept_kernel   point <- trial point, multipliers += step, clamped around mu / gap; masked instances untouched
//   emi_ipm_error_kernel    scale sums and the four maxima of the scaled KKT error as partials
//   emi_ipm_finish_kernel   the partials of the reducing kernels, added in chunk order, and what is formed from them
// and for the lock-step driver (emi_ipm_solve.hip):
//   emi_ipm_error_parts_kernel  the components of the KKT error, from which the error of any barrier parameter follows
//   emi_ipm_start_kernel    start(): interior push and fixed bytes; slacks, elastics and multipliers after the first evaluation; the
//                           reset of the elastic multipliers after a penalty escalation (masked)
//   emi_ipm_lamc_kernel     LamC = cscale Y
//
// One thread per (instance, node), 256 threads, grid (ceil(M / 256), B).  The loops run over variables and rows, so every access
// of a wave is a run of consecutive doubles along the node axis.  NOT "all loads of a thread before its stores": the number of
// path rows is a run-time value (20 at the measurement shape) and a row's eight outputs cannot wait in registers for the rows behind
// it without register arrays indexed at run time, i.e. scratch.  So a thread loads and stores once per loop step (a row: 8 - 12
// loads, then 4 - 8 stores), the arrays may alias as far as the compiler knows, and a thread exposes one memory round trip per row
// that only the other waves of the CU hide (at B = 1 and few nodes nothing does).  A value that a later loop
// needs again (sig_t r_t in the right-hand side, the zeroed dz in the row step) is read back from the array the thread itself wrote.  Per-instance sums and extrema: per-thread value, wave shuffles, LDS in wave order, one
// partial per workgroup, then the finishing kernel in chunk order: no atomics, two calls give the same bits.
//
// Conventions (include/emi355x.h): a variable is fixed where !(zu > zl); a bound is absent at |bound| >= 1e19; path values and
// their partials are read as cscale[j] RES and cscale[j] VALS, row bounds as cscale[j] bound (formed once on the host).
#include <hip/hip_runtime.h>

#include "emi_kernels.hpp"

namespace emi {
namespace {

constexpr double IPM_INF = 1e19;
constexpr int IPM_T = 256;
enum { R_SUM = 0, R_MIN = 1, R_MAX = 2 };

__device__ __forceinline__ double red2(double a, double b, int op) { return op == R_SUM ? a + b : op == R_MIN ? fmin(a, b) : fmax(a, b); }

// per-workgroup partial of N per-thread values: wave shuffles, then LDS in wave order; thread 0 writes part[0 .. N)
template <int N>
__device__ __forceinline__ void block_partials(double (&v)[N], const int (&op)[N], double* part) {
    __shared__ double lds[N * (IPM_T / 64)];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double x = v[i];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x = red2(x, __shfl_xor(x, m), op[i]);
        if (lane == 0) lds[i * (IPM_T / 64) + w] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            double x = lds[i * (IPM_T / 64)];
#pragma unroll
            for (int ww = 1; ww < IPM_T / 64; ++ww) x = red2(x, lds[i * (IPM_T / 64) + ww], op[i]);
            part[i] = x;
        }
    }
}

// where things of (instance b, node k) are
struct Idx {
    size_t M, k;
    int b, ns, nc, nv, np, set;
    __device__ Idx(const IpmArgs& a, int b_, int k_)
        : M((size_t)a.M), k((size_t)k_), b(b_), ns(a.ns), nc(a.nc), nv(a.ns + a.nc), np(a.np), set(a.nsets == 1 ? 0 : b_) {}
    __device__ size_t var(int v) const { return ((size_t)b * nv + v) * M + k; }
    __device__ size_t row(int j) const { return ((size_t)b * np + j) * M + k; }
    __device__ size_t bnd(int v) const { return ((size_t)set * nv + v) * M + k; }
    __device__ size_t kkt(int r) const { return ((size_t)b * (nv + ns) + r) * M + k; }
    __device__ size_t res(int r) const { return ((size_t)b * (ns + np) + r) * M + k; }
    __device__ size_t val(const IpmArgs& a, int e) const { return ((size_t)b * a.nvals + e) * M + k; }
    __device__ size_t st(int i) const { return ((size_t)b * ns + i) * M + k; }
    // variable v of a point given as (X, U)
    template <typename P> __device__ P* z(P* X, P* U, int v) const {
        return v < ns ? X + ((size_t)b * ns + v) * M + k : U + ((size_t)b * nc + (v - ns)) * M + k;
    }
};

// the row bounds of row j as the iteration sees them
struct RowB {
    bool hasL, hasU;
    double lo, hi, cs;
    __device__ RowB(const IpmArgs& a, int j)
        : hasL(a.crow[j] > -IPM_INF), hasU(a.crow[a.np + j] < IPM_INF), lo(a.crow[2 * a.np + j]), hi(a.crow[3 * a.np + j]), cs(a.crow[4 * a.np + j]) {}
};

// ---- reduce ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IPM_T) void emi_ipm_reduce_kernel(IpmArgs a) {
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    if (k >= a.M) return;
    const Idx ix(a, b, k);
    const int nv = ix.nv, ns = a.ns, np = a.np;
    const double mu = a.par[b * 4 + 0], rho = a.par[b * 4 + 1];
    for (int j = 0; j < np; ++j) {
        const RowB rb(a, j);
        const size_t r = ix.row(j);
        const double s = a.S[r], e1 = a.E1[r], e2 = a.E2[r], y = a.Y[r], vL = a.VL[r], vU = a.VU[r], w1 = a.W1[r], w2 = a.W2[r];
        const double rowres = a.RowRes ? a.RowRes[r] : rb.cs * a.RES[ix.res(ns + j)] - s - e1 + e2;
        double sg = 0, rh = -y;
        if (rb.hasL) { const double g = s - rb.lo; sg += vL / g; rh -= mu / g; }
        if (rb.hasU) { const double g = rb.hi - s; sg += vU / g; rh += mu / g; }
        const double a1 = e1 / w1, a2 = e2 / w2;
        const double sig_t = 1.0 / (1.0 / sg + a1 + a2);
        const double r_t = rowres + rh / sg - a1 * (y - rho + mu / e1) - a2 * (y + rho - mu / e2);
        a.SigS[r] = sg;
        a.RhatS[r] = rh;
        a.SigT[r] = sig_t;
        a.Rt[r] = r_t;
    }
    for (int v = 0; v < nv; ++v) {
        const double z = *ix.z(a.X, a.U, v), zl = a.zl[ix.bnd(v)], zu = a.zu[ix.bnd(v)];
        const double zL = a.ZL[ix.var(v)], zU = a.ZU[ix.var(v)], g = a.G[ix.var(v)];
        const bool free_v = zu > zl;
        double sg = 0.0, rr = g;
        if (free_v) {
            if (zl > -IPM_INF) { sg += zL / (z - zl); rr -= mu / (z - zl); }
            if (zu < IPM_INF) { sg += zU / (zu - z); rr += mu / (zu - z); }
        }
        double out = free_v ? -rr : 0.0;
        if (free_v)
            for (int t = a.vptr[v]; t < a.vptr[v + 1]; ++t) {       // the path rows of this variable, in row order
                const int j = a.vrow[t];
                const size_t r = ix.row(j);
                out -= a.crow[4 * np + j] * a.VALS[ix.val(a, a.vent[t])] * (a.SigT[r] * a.Rt[r]);
            }
        a.Sigma[ix.var(v)] = sg;
        a.Rhs[ix.kkt(v)] = out;
    }
    for (int i = 0; i < ns; ++i) a.Rhs[ix.kkt(nv + i)] = -(a.DefRes ? a.DefRes[ix.st(i)] : a.RES[ix.res(i)]);
}

// ---- expand ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IPM_T) void emi_ipm_expand_kernel(IpmArgs a) {
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    const bool act = k < a.M;
    const Idx ix(a, b, act ? k : 0);
    const int nv = ix.nv, ns = a.ns, np = a.np;
    const double mu = a.par[b * 4 + 0], rho = a.par[b * 4 + 1], tau = a.par[b * 4 + 2];
    double apr = 1.0, adu = 1.0, dphi = 0.0, mmax = 0.0;
    if (act) {
        for (int v = 0; v < nv; ++v) {
            const double z = *ix.z(a.X, a.U, v), zl = a.zl[ix.bnd(v)], zu = a.zu[ix.bnd(v)];
            const double zL = a.ZL[ix.var(v)], zU = a.ZU[ix.var(v)];
            const double gf = a.VALS[ix.val(a, a.nvals - nv + v)];          // cost gradient
            double dz = a.DZ[ix.kkt(v)];
            double dzL = 0.0, dzU = 0.0;
            if (zu > zl) {
                double g = gf;
                if (zl > -IPM_INF) {
                    const double gap = z - zl;
                    dzL = mu / gap - zL - zL / gap * dz;
                    g -= mu / gap;
                    if (dz < 0) apr = fmin(apr, -tau * gap / dz);
                }
                if (zu < IPM_INF) {
                    const double gap = zu - z;
                    dzU = mu / gap - zU + zU / gap * dz;
                    g += mu / gap;
                    if (dz > 0) apr = fmin(apr, tau * gap / dz);
                }
                if (dzL < 0) adu = fmin(adu, -tau * zL / dzL);
                if (dzU < 0) adu = fmin(adu, -tau * zU / dzU);
                dphi += g * dz;
            } else {
                dz = 0.0;
            }
            a.DZ[ix.kkt(v)] = dz;
            a.DZL[ix.var(v)] = dzL;
            a.DZU[ix.var(v)] = dzU;
        }
        for (int j = 0; j < np; ++j) {
            const RowB rb(a, j);
            const size_t r = ix.row(j);
            const double s = a.S[r], e1 = a.E1[r], e2 = a.E2[r], y = a.Y[r], vL = a.VL[r], vU = a.VU[r], w1 = a.W1[r], w2 = a.W2[r];
            const double sig_t = a.SigT[r], r_t = a.Rt[r], sig_s = a.SigS[r], rhat_s = a.RhatS[r];
            double jcdz = 0.0;
            for (int t = a.rptr[j]; t < a.rptr[j + 1]; ++t) jcdz += rb.cs * a.VALS[ix.val(a, a.rent[t])] * a.DZ[ix.kkt(a.rvar[t])];
            const double dy = sig_t * (jcdz + r_t);
            const double ds = (dy - rhat_s) / sig_s;
            const double de1 = e1 / w1 * (dy + y - rho + mu / e1);
            const double de2 = e2 / w2 * (-dy - y - rho + mu / e2);
            double dvL = 0.0, dvU = 0.0, g = 0.0;
            if (rb.hasL) {
                const double gap = s - rb.lo;
                dvL = mu / gap - vL - vL / gap * ds;
                g -= mu / gap;
                if (ds < 0) apr = fmin(apr, -tau * gap / ds);
            }
            if (rb.hasU) {
                const double gap = rb.hi - s;
                dvU = mu / gap - vU + vU / gap * ds;
                g += mu / gap;
                if (ds > 0) apr = fmin(apr, tau * gap / ds);
            }
            const double dw1 = mu / e1 - w1 - w1 / e1 * de1;
            const double dw2 = mu / e2 - w2 - w2 / e2 * de2;
            if (de1 < 0) apr = fmin(apr, -tau * e1 / de1);
            if (de2 < 0) apr = fmin(apr, -tau * e2 / de2);
            if (dvL < 0) adu = fmin(adu, -tau * vL / dvL);
            if (dvU < 0) adu = fmin(adu, -tau * vU / dvU);
            if (dw1 < 0) adu = fmin(adu, -tau * w1 / dw1);
            if (dw2 < 0) adu = fmin(adu, -tau * w2 / dw2);
            dphi += g * ds + (rho - mu / e1) * de1 + (rho - mu / e2) * de2;
            mmax = fmax(mmax, fabs(y + dy));
            a.DY[r] = dy; a.DS[r] = ds; a.DE1[r] = de1; a.DE2[r] = de2;
            a.DVL[r] = dvL; a.DVU[r] = dvU; a.DW1[r] = dw1; a.DW2[r] = dw2;
        }
        for (int i = 0; i < ns; ++i) {
            const double w = a.rs ? a.rs[ix.st(i)] : 1.0;
            mmax = fmax(mmax, fabs(a.LF[ix.st(i)] + a.DZ[ix.kkt(nv + i)]) / w);
        }
    }
    double v[4] = {apr, adu, dphi, mmax};
    constexpr int op[4] = {R_MIN, R_MIN, R_SUM, R_MAX};
    block_partials<4>(v, op, a.part + ((size_t)b * gridDim.x + blockIdx.x) * 4);
}

// ---- trial point ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IPM_T) void emi_ipm_trial_kernel(IpmArgs a) {
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    if (k >= a.M) return;
    const Idx ix(a, b, k);
    const double al = a.apr[b];
    for (int v = 0; v < ix.nv; ++v) *ix.z(a.tX, a.tU, v) = *ix.z(a.X, a.U, v) + al * a.DZ[ix.kkt(v)];
    for (int j = 0; j < a.np; ++j) {
        const size_t r = ix.row(j);
        const double s = a.S[r] + al * a.DS[r], e1 = a.E1[r] + al * a.DE1[r], e2 = a.E2[r] + al * a.DE2[r];
        a.tS[r] = s; a.tE1[r] = e1; a.tE2[r] = e2;
    }
}

// ---- merit ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IPM_T) void emi_ipm_merit_kernel(IpmArgs a) {
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    const bool act = k < a.M;
    const Idx ix(a, b, act ? k : 0);
    const int ns = a.ns, np = a.np;
    const double mu = a.par[b * 4 + 0], rho = a.par[b * 4 + 1], nu = a.par[b * 4 + 3];
    double phi = 0.0, viol = 0.0;
    if (act) {
        for (int v = 0; v < ix.nv; ++v) {
            const double z = *ix.z(a.X, a.U, v), zl = a.zl[ix.bnd(v)], zu = a.zu[ix.bnd(v)];
            if (!(zu > zl)) continue;
            if (zl > -IPM_INF) phi -= mu * log(z - zl);
            if (zu < IPM_INF) phi -= mu * log(zu - z);
        }
        for (int j = 0; j < np; ++j) {
            const RowB rb(a, j);
            const size_t r = ix.row(j);
            const double c = rb.cs * a.RES[ix.res(ns + j)], e1 = a.E1[r], e2 = a.E2[r];
            double s = a.S[r];
            if (a.reset) {
                const double target = c - e1 + e2;
                const double lo = rb.hasL ? rb.lo : -IPM_INF, hi = rb.hasU ? rb.hi : IPM_INF;
                if (target > lo && target < hi) {
                    double keep = nu * fabs(target - s), take = 0.0;
                    if (rb.hasL) { keep -= mu * log(s - lo); take -= mu * log(target - lo); }
                    if (rb.hasU) { keep -= mu * log(hi - s); take -= mu * log(hi - target); }
                    if (take < keep) {
                        s = target;
                        a.S[r] = s;
                    }
                }
            }
            if (rb.hasL) phi -= mu * log(s - rb.lo);
            if (rb.hasU) phi -= mu * log(rb.hi - s);
            phi += rho * (e1 + e2) - mu * (log(e1) + log(e2));
            viol += fabs(c - s - e1 + e2);
        }
        for (int i = 0; i < ns; ++i) viol += (a.rs ? a.rs[ix.st(i)] : 1.0) * fabs(a.RES[ix.res(i)]);
    }
    double v[2] = {phi, viol};
    constexpr int op[2] = {R_SUM, R_SUM};
    block_partials<2>(v, op, a.part + ((size_t)b * gridDim.x + blockIdx.x) * 2);
}

// ---- accept -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double clampm(double m, double g, double mu) {
    const double ks = 1e10;
    return fmax(fmin(m, ks * mu / g), mu / (ks * g));
}

__global__ __launch_bounds__(IPM_T) void emi_ipm_accept_kernel(IpmArgs a) {
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    if (k >= a.M) return;
    if (a.mask && !a.mask[b]) return;
    const Idx ix(a, b, k);
    const int ns = a.ns, np = a.np;
    const double mu = a.par[b * 4 + 0], apr = a.apr[b], adu = a.adu[b];
    for (int v = 0; v < ix.nv; ++v) {
        const double z = *ix.z(a.tX, a.tU, v), zl = a.zl[ix.bnd(v)], zu = a.zu[ix.bnd(v)];
        double zL = a.ZL[ix.var(v)], zU = a.ZU[ix.var(v)];
        const double dzL = a.DZL[ix.var(v)], dzU = a.DZU[ix.var(v)];
        *ix.z(a.X, a.U, v) = z;
        if (!(zu > zl)) continue;
        zL += adu * dzL;
        zU += adu * dzU;
        if (zl > -IPM_INF) zL = clampm(zL, z - zl, mu);
        if (zu < IPM_INF) zU = clampm(zU, zu - z, mu);
        a.ZL[ix.var(v)] = zL;
        a.ZU[ix.var(v)] = zU;
    }
    for (int i = 0; i < ns; ++i) a.LF[ix.st(i)] += apr * a.DZ[ix.kkt(ix.nv + i)];
    for (int j = 0; j < np; ++j) {
        const RowB rb(a, j);
        const size_t r = ix.row(j);
        const double s = a.tS[r], e1 = a.tE1[r], e2 = a.tE2[r];
        const double y = a.Y[r] + apr * a.DY[r];
        double vL = a.VL[r] + adu * a.DVL[r], vU = a.VU[r] + adu * a.DVU[r];
        double w1 = a.W1[r] + adu * a.DW1[r], w2 = a.W2[r] + adu * a.DW2[r];
        if (rb.hasL) vL = clampm(vL, s - rb.lo, mu);
        if (rb.hasU) vU = clampm(vU, rb.hi - s, mu);
        w1 = clampm(w1, e1, mu);
        w2 = clampm(w2, e2, mu);
        a.S[r] = s; a.E1[r] = e1; a.E2[r] = e2;
        a.Y[r] = y; a.VL[r] = vL; a.VU[r] = vU; a.W1[r] = w1; a.W2[r] = w2;
    }
}

// ---- KKT error ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IPM_T) void emi_ipm_error_kernel(IpmArgs a) {
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    const bool act = k < a.M;
    const Idx ix(a, b, act ? k : 0);
    const int ns = a.ns, np = a.np;
    const double mu = a.par[b * 4 + 0], rho = a.par[b * 4 + 1];
    double sumz = 0, summ = 0, cnt = 0, ed = 0, ep = 0, ec = 0, emax = 0;
    if (act) {
        for (int v = 0; v < ix.nv; ++v) {
            const double z = *ix.z(a.X, a.U, v), zl = a.zl[ix.bnd(v)], zu = a.zu[ix.bnd(v)];
            const double zL = a.ZL[ix.var(v)], zU = a.ZU[ix.var(v)], g = a.G[ix.var(v)];
            sumz += zL + zU;
            cnt += (zL > 0) + (zU > 0);
            if (!(zu > zl)) continue;
            ed = fmax(ed, fabs(g - zL + zU));
            if (zl > -IPM_INF) ec = fmax(ec, fabs((z - zl) * zL - mu));
            if (zu < IPM_INF) ec = fmax(ec, fabs((zu - z) * zU - mu));
        }
        for (int j = 0; j < np; ++j) {
            const RowB rb(a, j);
            const size_t r = ix.row(j);
            const double s = a.S[r], e1 = a.E1[r], e2 = a.E2[r], y = a.Y[r], vL = a.VL[r], vU = a.VU[r], w1 = a.W1[r], w2 = a.W2[r];
            const double c = rb.cs * a.RES[ix.res(ns + j)];
            sumz += vL + vU + w1 + w2;
            cnt += (vL > 0) + (vU > 0) + 2;
            summ += fabs(y);
            ed = fmax(ed, fabs(-y - vL + vU));
            ed = fmax(ed, fabs(rho - y - w1));
            ed = fmax(ed, fabs(rho + y - w2));
            ep = fmax(ep, fabs(c - s - e1 + e2));
            emax = fmax(emax, fmax(e1, e2));
            if (rb.hasL) ec = fmax(ec, fabs((s - rb.lo) * vL - mu));
            if (rb.hasU) ec = fmax(ec, fabs((rb.hi - s) * vU - mu));
            ec = fmax(ec, fabs(e1 * w1 - mu));
            ec = fmax(ec, fabs(e2 * w2 - mu));
        }
        for (int i = 0; i < ns; ++i) {
            summ += fabs(a.LF[ix.st(i)]);
            ep = fmax(ep, fabs(a.RES[ix.res(i)]));
        }
    }
    double v[7] = {sumz, summ, cnt, ed, ep, ec, emax};
    constexpr int op[7] = {R_SUM, R_SUM, R_SUM, R_MAX, R_MAX, R_MAX, R_MAX};
    block_partials<7>(v, op, a.part + ((size_t)b * gridDim.x + blockIdx.x) * 7);
}

// ---- components of the KKT error: what emi_ipm_error_kernel folds into one number for par.mu, kept apart -----------------------------
// The sums and the maxima ed, ep, emax are those of emi_ipm_error_kernel term for term; instead of ec = max |product - mu| the
// smallest and the largest product, from which ec follows for any mu (rounding is monotonic: the same bits as the maximum of the
// rounded differences); and max |Y|, which the barrier update asks for.
__global__ __launch_bounds__(IPM_T) void emi_ipm_error_parts_kernel(IpmArgs a) {
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    const bool act = k < a.M;
    const Idx ix(a, b, act ? k : 0);
    const int ns = a.ns, np = a.np;
    const double rho = a.par[b * 4 + 1];
    double sumz = 0, summ = 0, cnt = 0, ed = 0, ep = 0, pmin = 1e300, pmax = -1e300, emax = 0, ymax = 0;
    if (act) {
        for (int v = 0; v < ix.nv; ++v) {
            const double z = *ix.z(a.X, a.U, v), zl = a.zl[ix.bnd(v)], zu = a.zu[ix.bnd(v)];
            const double zL = a.ZL[ix.var(v)], zU = a.ZU[ix.var(v)], g = a.G[ix.var(v)];
            sumz += zL + zU;
            cnt += (zL > 0) + (zU > 0);
            if (!(zu > zl)) continue;
            ed = fmax(ed, fabs(g - zL + zU));
            if (zl > -IPM_INF) { const double p = (z - zl) * zL; pmin = fmin(pmin, p); pmax = fmax(pmax, p); }
            if (zu < IPM_INF) { const double p = (zu - z) * zU; pmin = fmin(pmin, p); pmax = fmax(pmax, p); }
        }
        for (int j = 0; j < np; ++j) {
            const RowB rb(a, j);
            const size_t r = ix.row(j);
            const double s = a.S[r], e1 = a.E1[r], e2 = a.E2[r], y = a.Y[r], vL = a.VL[r], vU = a.VU[r], w1 = a.W1[r], w2 = a.W2[r];
            const double c = rb.cs * a.RES[ix.res(ns + j)];
            sumz += vL + vU + w1 + w2;
            cnt += (vL > 0) + (vU > 0) + 2;
            summ += fabs(y);
            ed = fmax(ed, fabs(-y - vL + vU));
            ed = fmax(ed, fabs(rho - y - w1));
            ed = fmax(ed, fabs(rho + y - w2));
            ep = fmax(ep, fabs(c - s - e1 + e2));
            emax = fmax(emax, fmax(e1, e2));
            ymax = fmax(ymax, fabs(y));
            if (rb.hasL) { const double p = (s - rb.lo) * vL; pmin = fmin(pmin, p); pmax = fmax(pmax, p); }
            if (rb.hasU) { const double p = (rb.hi - s) * vU; pmin = fmin(pmin, p); pmax = fmax(pmax, p); }
            const double p1 = e1 * w1, p2 = e2 * w2;
            pmin = fmin(pmin, fmin(p1, p2));
            pmax = fmax(pmax, fmax(p1, p2));
        }
        for (int i = 0; i < ns; ++i) {
            summ += fabs(a.LF[ix.st(i)]);
            ep = fmax(ep, fabs(a.RES[ix.res(i)]));
        }
    }
    double v[9] = {sumz, summ, cnt, ed, ep, pmin, pmax, emax, ymax};
    constexpr int op[9] = {R_SUM, R_SUM, R_SUM, R_MAX, R_MAX, R_MIN, R_MAX, R_MAX, R_MAX};
    block_partials<9>(v, op, a.part + ((size_t)b * gridDim.x + blockIdx.x) * 9);
}

// ---- the start of a lock-step solve (solve_nlp's start()) and the small array steps of its rounds -------------------------------------
// Every operation below is an exact one or a single rounded one with contraction off: the arrays are, bit for bit, what the
// formulas give in any IEEE arithmetic.
__device__ __forceinline__ double pushed_inside(double v, double l, double u, bool hasL, bool hasU, double push, double frac) {
#pragma clang fp contract(off)
    double pl = hasL ? push * fmax(1.0, fabs(l)) : 0.0, pu = hasU ? push * fmax(1.0, fabs(u)) : 0.0;
    if (hasL && hasU) { pl = fmin(pl, frac * (u - l)); pu = fmin(pu, frac * (u - l)); }
    if (hasL) v = fmax(v, l + pl);
    if (hasU) v = fmin(v, u - pu);
    return v;
}

__global__ __launch_bounds__(IPM_T) void emi_ipm_start_kernel(IpmArgs a, int phase) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    if (k >= a.M) return;
    const Idx ix(a, b, k);
    const int ns = a.ns, np = a.np;
    if (phase == IPM_START_PUSH) {
        for (int v = 0; v < ix.nv; ++v) {
            const double zl = a.zl[ix.bnd(v)], zu = a.zu[ix.bnd(v)];
            double* z = ix.z(a.X, a.U, v);
            const bool fx = !(zu > zl);
            a.fixedb[ix.var(v)] = fx ? 1 : 0;
            *z = fx ? zl : pushed_inside(*z, zl, zu, zl > -IPM_INF, zu < IPM_INF, a.push, a.frac);
        }
        for (int i = 0; i < ns; ++i) a.LF[ix.st(i)] = 0.0;
        return;
    }
    const double rho = a.par[b * 4 + 1];
    if (phase == IPM_RESET_W) {
        if (a.mask && !a.mask[b]) return;
        for (int j = 0; j < np; ++j) {
            const size_t r = ix.row(j);
            const double y = a.Y[r];
            a.W1[r] = fmax(1e-8, rho - y);
            a.W2[r] = fmax(1e-8, rho + y);
        }
        return;
    }
    for (int v = 0; v < ix.nv; ++v) {           // IPM_START_ROWS
        const double zl = a.zl[ix.bnd(v)], zu = a.zu[ix.bnd(v)];
        const bool fr = zu > zl;
        a.ZL[ix.var(v)] = fr && zl > -IPM_INF ? 1.0 : 0.0;
        a.ZU[ix.var(v)] = fr && zu < IPM_INF ? 1.0 : 0.0;
    }
    for (int j = 0; j < np; ++j) {
        const RowB rb(a, j);
        const size_t r = ix.row(j);
        const double c0 = rb.cs * a.RES[ix.res(ns + j)];
        const double s = pushed_inside(c0, rb.lo, rb.hi, rb.hasL, rb.hasU, a.push, a.frac);
        const double gap = c0 - s, ee = a.push * fmax(1.0, fabs(gap));
        a.S[r] = s;
        a.E1[r] = fmax(gap, 0.0) + ee;          // the residual c - s - e1 + e2 starts at exactly 0
        a.E2[r] = fmax(-gap, 0.0) + ee;
        a.Y[r] = 0.0;
        a.VL[r] = rb.hasL ? 1.0 : 0.0;
        a.VU[r] = rb.hasU ? 1.0 : 0.0;
        a.W1[r] = fmax(1e-8, rho);
        a.W2[r] = fmax(1e-8, rho);
    }
}

// path-row multipliers in the caller's units
__global__ __launch_bounds__(IPM_T) void emi_ipm_lamc_kernel(IpmArgs a) {
    const int k = blockIdx.x * IPM_T + threadIdx.x, b = blockIdx.y;
    if (k >= a.M) return;
    const Idx ix(a, b, k);
    for (int j = 0; j < a.np; ++j) a.LamC[ix.row(j)] = a.crow[4 * a.np + j] * a.Y[ix.row(j)];
}

// ---- the partials of an instance in chunk order -------------------------------------------------------------------------------------
// what: 0 expand -> out[b][4] = {apr, adu, dphi, mmax};  1 merit -> out[b][2] = {COST + phi, infeas};
//       2 error -> out[b][3] = {kkt_error, viol, emax};  3 error parts -> out[b][8] = {ed, sd, ep, sc, pmin, pmax, emax, ymax}
__global__ __launch_bounds__(IPM_T) void emi_ipm_finish_kernel(const double* part, const double* cost, double* out, int B, int nchunk, int what,
                                                              int me_mc) {
    const int b = blockIdx.x * IPM_T + threadIdx.x;
    if (b >= B) return;
    if (what == 0) {
        const double* p = part + (size_t)b * nchunk * 4;
        double apr = p[0], adu = p[1], dphi = p[2], mmax = p[3];
        for (int c = 1; c < nchunk; ++c) {
            apr = fmin(apr, p[c * 4]); adu = fmin(adu, p[c * 4 + 1]); dphi += p[c * 4 + 2]; mmax = fmax(mmax, p[c * 4 + 3]);
        }
        out[b * 4] = apr; out[b * 4 + 1] = adu; out[b * 4 + 2] = dphi; out[b * 4 + 3] = mmax;
    } else if (what == 1) {
        const double* p = part + (size_t)b * nchunk * 2;
        double phi = cost[b], viol = 0.0;
        for (int c = 0; c < nchunk; ++c) { phi += p[c * 2]; viol += p[c * 2 + 1]; }
        out[b * 2] = phi; out[b * 2 + 1] = viol;
    } else if (what == 3) {
        const double* p = part + (size_t)b * nchunk * 9;
        double sumz = 0, summ = 0, cnt = 0, ed = 0, ep = 0, pmin = 1e300, pmax = -1e300, emax = 0, ymax = 0;
        for (int c = 0; c < nchunk; ++c) {
            sumz += p[c * 9]; summ += p[c * 9 + 1]; cnt += p[c * 9 + 2];
            ed = fmax(ed, p[c * 9 + 3]); ep = fmax(ep, p[c * 9 + 4]); pmin = fmin(pmin, p[c * 9 + 5]); pmax = fmax(pmax, p[c * 9 + 6]);
            emax = fmax(emax, p[c * 9 + 7]); ymax = fmax(ymax, p[c * 9 + 8]);
        }
        const double smax = 100.0;
        double* o = out + (size_t)b * 8;
        o[0] = ed; o[1] = fmax(smax, (summ + sumz) / fmax(1.0, (double)me_mc + cnt)) / smax; o[2] = ep;
        o[3] = fmax(smax, sumz / fmax(1.0, cnt)) / smax; o[4] = pmin; o[5] = pmax; o[6] = emax; o[7] = ymax;
    } else {
        const double* p = part + (size_t)b * nchunk * 7;
        double sumz = 0, summ = 0, cnt = 0, ed = 0, ep = 0, ec = 0, emax = 0;
        for (int c = 0; c < nchunk; ++c) {
            sumz += p[c * 7]; summ += p[c * 7 + 1]; cnt += p[c * 7 + 2];
            ed = fmax(ed, p[c * 7 + 3]); ep = fmax(ep, p[c * 7 + 4]); ec = fmax(ec, p[c * 7 + 5]); emax = fmax(emax, p[c * 7 + 6]);
        }
        const double smax = 100.0;
        const double sd = fmax(smax, (summ + sumz) / fmax(1.0, (double)me_mc + cnt)) / smax;
        const double sc = fmax(smax, sumz / fmax(1.0, cnt)) / smax;
        out[b * 3] = fmax(fmax(ed / sd, ep), ec / sc); out[b * 3 + 1] = ep; out[b * 3 + 2] = emax;
    }
}

}  // namespace

int ipm_chunks(int M) { return (M + IPM_T - 1) / IPM_T; }

hipError_t launch_ipm(int what, const IpmArgs& a, hipStream_t s) {
    const int nchunk = ipm_chunks(a.M);
    const dim3 grid(nchunk, a.B), fgrid((a.B + IPM_T - 1) / IPM_T);
    switch (what) {
        case IPM_REDUCE: hipLaunchKernelGGL(emi_ipm_reduce_kernel, grid, dim3(IPM_T), 0, s, a); break;
        case IPM_EXPAND:
            hipLaunchKernelGGL(emi_ipm_expand_kernel, grid, dim3(IPM_T), 0, s, a);
            hipLaunchKernelGGL(emi_ipm_finish_kernel, fgrid, dim3(IPM_T), 0, s, a.part, nullptr, a.out, a.B, nchunk, 0, 0);
            break;
        case IPM_TRIAL: hipLaunchKernelGGL(emi_ipm_trial_kernel, grid, dim3(IPM_T), 0, s, a); break;
        case IPM_MERIT:
            hipLaunchKernelGGL(emi_ipm_merit_kernel, grid, dim3(IPM_T), 0, s, a);
            hipLaunchKernelGGL(emi_ipm_finish_kernel, fgrid, dim3(IPM_T), 0, s, a.part, a.COST, a.out, a.B, nchunk, 1, 0);
            break;
        case IPM_ACCEPT: hipLaunchKernelGGL(emi_ipm_accept_kernel, grid, dim3(IPM_T), 0, s, a); break;
        case IPM_ERROR:
            hipLaunchKernelGGL(emi_ipm_error_kernel, grid, dim3(IPM_T), 0, s, a);
            hipLaunchKernelGGL(emi_ipm_finish_kernel, fgrid, dim3(IPM_T), 0, s, a.part, nullptr, a.out, a.B, nchunk, 2, (a.ns + a.np) * a.M);
            break;
        case IPM_ERROR_PARTS:
            hipLaunchKernelGGL(emi_ipm_error_parts_kernel, grid, dim3(IPM_T), 0, s, a);
            hipLaunchKernelGGL(emi_ipm_finish_kernel, fgrid, dim3(IPM_T), 0, s, a.part, nullptr, a.out, a.B, nchunk, 3, (a.ns + a.np) * a.M);
            break;
        case IPM_START_PUSH: case IPM_START_ROWS: case IPM_RESET_W: hipLaunchKernelGGL(emi_ipm_start_kernel, grid, dim3(IPM_T), 0, s, a, what); break;
        case IPM_LAMC: hipLaunchKernelGGL(emi_ipm_lamc_kernel, grid, dim3(IPM_T), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace emi
