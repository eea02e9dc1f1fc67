// etol_harness_ipm.cpp -- extern "C" shim for the interior-point arithmetic tests: the HOST functions solve_nlp runs between two
// evaluator calls (mi355x::ipm_*, host/emi_nlp.hpp) on given arrays, one instance at a time, driven the way solve_nlp drives them
// (path values and partials scaled by cscale first, the Lagrangian gradient handed over as gradf with jtl = 0, dz of fixed
// variables zeroed before the expansion).  Linked into libetol_harness.so.  Test infrastructure.
#include <chrono>
#include <cmath>
#include <utility>
#include <vector>

#include "emi_nlp.hpp"

namespace mx = ETOL::mi355x;

namespace {

struct Problem {
    int nv = 0, ns = 0, np = 0, M = 0, nvals = 0;
    std::vector<double> zl, zu, cl, cu, cs, cls, cus;
    std::vector<std::vector<std::pair<int, int>>> rows;
    mx::IpmDims dims() const {
        mx::IpmDims d;
        d.nv = nv; d.ns = ns; d.np = np; d.M = M; d.ml = 0;
        d.zl = zl.data(); d.zu = zu.data(); d.cl = cl.data(); d.cu = cu.data(); d.cls = cls.data(); d.cus = cus.data();
        d.row_vars = &rows;
        return d;
    }
};
Problem g_p;

// slots of the array table (tests/test_ipm_cpu.py: SLOTS)
enum { Z, S, E1, E2, LAM, Y, ZL, ZU, VL, VU, W1, W2, RES, VALS, G, DEFRES, ROWRES, RS, SIGMA, SIGT, SIGS, RHATS, RT, RHS, DZLAM, DS, DY, DE1,
       DE2, DZL, DZU, DVL, DVU, DW1, DW2, OUT, NSLOTS };

}  // namespace

extern "C" {

// bounds of one instance: zl, zu [nv*M], cl, cu, cscale [np] (cscale may be null = 1), rows as a CSR list of (variable, VALS entry)
void harness_ipm_problem(int nv, int ns, int np, int M, int nvals, const double* zl, const double* zu, const double* cl, const double* cu,
                         const double* cscale, const int* row_ptr, const int* var, const int* entry) {
    Problem& p = g_p;
    p.nv = nv; p.ns = ns; p.np = np; p.M = M; p.nvals = nvals;
    p.zl.assign(zl, zl + (size_t)nv * M); p.zu.assign(zu, zu + (size_t)nv * M);
    p.cl.assign(cl, cl + np); p.cu.assign(cu, cu + np);
    p.cs.assign(np, 1.0);
    for (int j = 0; j < np && cscale; ++j) p.cs[j] = cscale[j];
    p.cls.resize(np); p.cus.resize(np);
    for (int j = 0; j < np; ++j) {          // as solve_nlp forms them
        p.cls[j] = p.cl[j] > -1e19 ? p.cs[j] * p.cl[j] : p.cl[j];
        p.cus[j] = p.cu[j] < 1e19 ? p.cs[j] * p.cu[j] : p.cu[j];
    }
    p.rows.assign((size_t)np, {});
    for (int j = 0; j < np; ++j)
        for (int t = row_ptr[j]; t < row_ptr[j + 1]; ++t) p.rows[j].push_back({var[t], entry[t]});
}

// what: 0 reduce, 1 expand (+ step lengths, dphi, mmax into OUT[4]), 2 merit (reset optional; OUT[2]), 3 multipliers after a step
// (the point given is the new one), 4 kkt_error (OUT[3]).  a: the array table; sc = {mu, rho, tau, nu, cost, a_pr, a_du}.
// reps > 1: the ipm_* calls of `what` are repeated that often on the same arrays (the preparation above them is not) and *seconds
// receives the wall time of the repetitions alone: the host figure of tools/ipm_times.py
int harness_ipm_timed(int what, double** a, const double* sc, int reset, int reps, double* seconds) {
    const Problem& p = g_p;
    const int M = p.M, nv = p.nv, ns = p.ns, np = p.np, nz = nv * M, md = ns * M, mc = np * M;
    const mx::IpmDims P = p.dims();
    const double mu = sc[0], rho = sc[1], tau = sc[2], nu = sc[3], cost = sc[4];
    // the evaluator's values as the iteration holds them: path rows and their partials times cscale
    std::vector<double> res, vals;
    if (a[RES]) {
        res.assign(a[RES], a[RES] + md + mc);
        for (int j = 0; j < np; ++j)
            if (p.cs[j] != 1.0)
                for (int k = 0; k < M; ++k) res[(size_t)md + j * M + k] *= p.cs[j];
    }
    if (a[VALS]) {
        vals.assign(a[VALS], a[VALS] + (size_t)p.nvals * M);
        for (int j = 0; j < np; ++j)
            if (p.cs[j] != 1.0)
                for (const auto& ve : p.rows[j])
                    for (int k = 0; k < M; ++k) vals[(size_t)ve.second * M + k] *= p.cs[j];
    }
    const mx::IpmPoint x{a[Z], a[S], a[E1], a[E2]};
    const mx::IpmDuals d{a[LAM], a[Y], a[ZL], a[ZU], a[VL], a[VU], a[W1], a[W2]};
    const mx::IpmRes e{res.data(), nullptr};
    const mx::IpmElim el{a[SIGS], a[RHATS], a[SIGT], a[RT]};
    const mx::IpmStep st{a[DZLAM], a[DZLAM] ? a[DZLAM] + nz : nullptr, a[DS], a[DY], a[DE1], a[DE2], a[DZL], a[DZU], a[DVL], a[DVU], a[DW1], a[DW2]};
    std::vector<double> ones(md, 1.0), zeros(nz, 0.0);
    const double* rs = a[RS] ? a[RS] : ones.data();
    int rc = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < reps && rc == 0; ++it) switch (what) {
        case 0: {
            mx::ipm_eliminate_rows(P, x, d, e, mu, rho, el);
            if (a[ROWRES]) mx::ipm_fill_rt(P, x, d, a[ROWRES], mu, rho, el);
            mx::ipm_barrier_diagonal(P, x, d, a[SIGMA]);
            mx::ipm_build_rhs(P, x, a[G], zeros.data(), vals.data(), el, a[DEFRES] ? a[DEFRES] : res.data(), mu, a[RHS]);
            break;
        }
        case 1: {
            for (int q = 0; q < nz; ++q)
                if (!(p.zu[q] > p.zl[q])) a[DZLAM][q] = 0.0;
            mx::ipm_expand_step(P, x, d, vals.data(), el, mu, rho, st);
            mx::ipm_step_lengths(P, x, d, st, tau, &a[OUT][0], &a[OUT][1]);
            mx::ipm_dphi_mmax(P, x, d, vals.data() + (size_t)(p.nvals - nv) * M, st, rs, mu, rho, &a[OUT][2], &a[OUT][3]);
            break;
        }
        case 2: {
            if (reset) mx::ipm_slack_reset(P, res.data() + md, a[E1], a[E2], mu, nu, a[S]);
            a[OUT][0] = mx::ipm_barrier_merit(P, x, e, cost, rs, mu, 0.0, rho, &a[OUT][1]);
            break;
        }
        case 3: {
            const mx::IpmDualsRW dw{a[LAM], a[Y], a[ZL], a[ZU], a[VL], a[VU], a[W1], a[W2]};
            mx::ipm_update_duals(P, x, dw, st, sc[5], sc[6], mu);
            break;
        }
        case 4: {
            a[OUT][0] = mx::ipm_kkt_error(P, x, d, a[G], zeros.data(), e, mu, rho, &a[OUT][1], &a[OUT][2]);
            break;
        }
        default: rc = 1;
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int harness_ipm(int what, double** a, const double* sc, int reset) { return harness_ipm_timed(what, a, sc, reset, 1, nullptr); }

int harness_ipm_nslots(void) { return NSLOTS; }

}  // extern "C"
