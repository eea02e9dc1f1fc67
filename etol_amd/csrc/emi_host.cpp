// emi_host.cpp -- host-only parts of the C ABI: mesh construction and the
// per-problem constants the kernels consume.  No device code here.
//
// Legendre-Gauss-Lobatto transcription: PSOPT 5.0.0's collocation_method =
// "Legendre" (reference src/ePSOPT/ePSOPT.cpp:68) places the nodes at the
// zeros of (1-tau^2) P'_N(tau), N = nodes-1 (ePSOPT.cpp:44-45), which include
// the end points that ePSOPT::events reads (ePSOPT.cpp:281-291).  PSOPT's
// sources are not part of the reference tree, so the construction below is the
// textbook one, written from the defining formulas.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "emi355x.h"
#include "emi_plan_route.hpp"

namespace {

// P_N(x) and P_{N-1}(x) by the three-term recurrence, in extended precision.
inline void legendre_pair(int N, long double x, long double* pn, long double* pnm1) {
    long double p0 = 1.0L, p1 = x;
    if (N == 0) { *pn = 1.0L; *pnm1 = 0.0L; return; }
    for (int n = 1; n < N; ++n) {
        const long double p2 = ((2 * n + 1) * x * p1 - n * p0) / (n + 1);
        p0 = p1;
        p1 = p2;
    }
    *pn = p1;
    *pnm1 = p0;
}

}  // namespace

extern "C" {

int emi_abi_version(void) { return EMI_ABI_VERSION; }

const char* emi_status_string(int status) {
    switch (status) {
        case EMI_OK: return "ok";
        case EMI_ERR_ARG: return "invalid argument";
        case EMI_ERR_STATE: return "call out of order";
        case EMI_ERR_HIP: return "HIP runtime error";
        case EMI_ERR_NO_DEVICE: return "no gfx950 device";
        case EMI_ERR_UNSUPPORTED: return "unsupported in this build";
        case EMI_ERR_COMM: return "RCCL error";
    }
    return "unknown status";
}

int emi_lgl(int M, double* tau, double* w, double* D) {
    if (M < 2 || !tau || !w) return EMI_ERR_ARG;
    const int N = M - 1;
    const long double pi = 3.14159265358979323846264338327950288L;
    std::vector<long double> x(M), pN(M);
    x[0] = -1.0L;
    x[N] = 1.0L;
    // interior zeros of P'_N by Newton on q(x) = (1-x^2) P'_N = N (P_{N-1} - x P_N),
    // q'(x) = -N (N+1) P_N  (Legendre's equation), from Chebyshev-Lobatto guesses
    for (int k = 1; k <= N / 2; ++k) {
        long double xk = -cosl(pi * k / N);
        for (int it = 0; it < 100; ++it) {
            long double pn, pnm1;
            legendre_pair(N, xk, &pn, &pnm1);
            const long double dx = (xk * pn - pnm1) / ((N + 1) * pn);
            xk -= dx;
            if (fabsl(dx) <= 4.0L * 1.0842021724855044e-19L * fmaxl(1.0L, fabsl(xk))) break;
        }
        x[k] = xk;
        x[N - k] = -xk;  // the node set is symmetric about 0
    }
    if (N % 2 == 0) x[N / 2] = 0.0L;
    for (int k = 0; k < M; ++k) {
        long double pn, pnm1;
        legendre_pair(N, x[k], &pn, &pnm1);
        pN[k] = pn;
        tau[k] = (double)x[k];
        w[k] = (double)(2.0L / ((long double)N * (N + 1) * pn * pn));
    }
    if (D) {
        // D_ij = P_N(x_i) / (P_N(x_j) (x_i - x_j)), i != j;  the diagonal is the
        // negative row sum so that D.1 = 0 holds to rounding (the closed-form
        // diagonal already loses 1e-6 at N = 255).
        for (int i = 0; i < M; ++i) {
            long double rs = 0.0L;
            for (int j = 0; j < M; ++j) {
                if (i == j) continue;
                const long double d = pN[i] / (pN[j] * (x[i] - x[j]));
                D[(size_t)i * M + j] = (double)d;
                rs += (long double)D[(size_t)i * M + j];
            }
            D[(size_t)i * M + i] = (double)(-rs);
        }
        // The node set is symmetric, so D is centro-antisymmetric: D[N-i][N-j] = -D[i][j].
        // The off-diagonal entries satisfy this bit for bit; make the summed diagonal do so
        // too (the kernels split D.X into even and odd halves when it holds exactly).
        for (int i = 0; i < M / 2; ++i) D[(size_t)(N - i) * M + (N - i)] = -D[(size_t)i * M + i];
        if (M % 2 == 1) D[(size_t)(N / 2) * M + N / 2] = 0.0;
    }
    return EMI_OK;
}

int emi_model_dims(int model, int* ns, int* nc, int* nparams) {
    int s, c, p;
    switch (model) {
        case EMI_MODEL_POINTMASS2D: s = 2; c = 2; p = 0; break;
        case EMI_MODEL_QUADROTOR2D: s = 6; c = 2; p = 5; break;
        case EMI_MODEL_FIXEDWING12: s = 12; c = 4; p = 16; break;
        default: return EMI_ERR_ARG;
    }
    if (ns) *ns = s;
    if (nc) *nc = c;
    if (nparams) *nparams = p;
    return EMI_OK;
}

// Interpolation operator E and its tau-derivative E' of the barycentric interpolant through the nodes (tau, w) at the five
// Gauss-Legendre points of every mesh interval; point p = q (M-1) + k is Gauss point q of [tau_k, tau_k+1] (include/emi355x.h).
// tq[p] is rounded to double first and the operator is that of the rounded abscissa, formed in extended precision:
//   lam_j = (-1)^j sqrt(w_j) / (s - tau_j),  E_j = lam_j / sum lam,  E'_j = (E_j sum_i lam_i / (s - tau_i) - lam_j / (s - tau_j)) / sum lam
static const long double gx[5] = {-0.906179845938663992797626878299392965L, -0.538469310105683091036314420700208805L, 0.0L,
                                  0.538469310105683091036314420700208805L, 0.906179845938663992797626878299392965L};

int emi_ode_error_operator(int M, const double* tau, const double* w, double* E, double* Ed, double* tq) {
    if (M < 2 || !tau || !w || !E || !Ed || !tq) return EMI_ERR_ARG;
    const int nq = M - 1;
    std::vector<long double> sw(M), lam(M);
    for (int j = 0; j < M; ++j) sw[j] = ((j & 1) ? -1.0L : 1.0L) * sqrtl((long double)w[j]);
    for (int q = 0; q < 5; ++q)
        for (int k = 0; k < nq; ++k) {
            const int p = q * nq + k;
            tq[p] = (double)((long double)tau[k] + 0.5L * ((long double)tau[k + 1] - (long double)tau[k]) * (gx[q] + 1.0L));
            const long double s = tq[p];
            long double S = 0.0L, T = 0.0L;
            for (int j = 0; j < M; ++j) {
                lam[j] = sw[j] / (s - (long double)tau[j]);
                S += lam[j];
                T += lam[j] / (s - (long double)tau[j]);
            }
            for (int j = 0; j < M; ++j) {
                const long double e = lam[j] / S;
                E[(size_t)p * M + j] = (double)e;
                Ed[(size_t)p * M + j] = (double)((e * T - lam[j] / (s - (long double)tau[j])) / S);
            }
        }
    return EMI_OK;
}

// The operator of one delay between the nodes: row p of Edel is the Lagrange basis of the mesh at the node coordinate of
// max(t_p - delay, t0), t_p = t0 + h (s_p + 1) the time of point p of emi_ode_error_operator (the same rounded s_p).  The shifted
// abscissa is formed in double exactly as emi_delay_matrix forms it at a node (one clamp for both), the row in extended precision
// in barycentric form; a time at or before t0 gives e_0, an abscissa that is a node exactly gives that node's unit row.
int emi_ode_error_delay_operator(int M, const double* tau, const double* w, double t0, double tf, double delay, double* Edel) {
    if (M < 2 || !tau || !w || !Edel || !(tf > t0) || !(delay >= 0)) return EMI_ERR_ARG;
    const int nq = M - 1;
    const double hh = (tf - t0) / 2.0;
    std::vector<long double> sw(M), lam(M);
    for (int j = 0; j < M; ++j) sw[j] = ((j & 1) ? -1.0L : 1.0L) * sqrtl((long double)w[j]);
    for (int q = 0; q < 5; ++q)
        for (int k = 0; k < nq; ++k) {
            const double sp = (double)((long double)tau[k] + 0.5L * ((long double)tau[k + 1] - (long double)tau[k]) * (gx[q] + 1.0L));
            const double tp = t0 + hh * (sp + 1.0);
            double ts = tp - delay;
            if (ts < t0) ts = t0;
            const double x = (ts - t0) / hh - 1.0;
            double* row = Edel + (size_t)(q * nq + k) * M;
            int hit = -1;
            for (int j = 0; j < M; ++j)
                if (x == tau[j]) hit = j;
            if (ts <= t0) hit = 0;
            if (hit >= 0) {
                for (int j = 0; j < M; ++j) row[j] = j == hit ? 1.0 : 0.0;
                continue;
            }
            long double S = 0.0L;
            for (int j = 0; j < M; ++j) {
                lam[j] = sw[j] / ((long double)x - (long double)tau[j]);
                S += lam[j];
            }
            for (int j = 0; j < M; ++j) row[j] = (double)(lam[j] / S);
        }
    return EMI_OK;
}

// One polygon edge a->b as an ellipse keep-out record.  The reference evaluates
// these constants inside the node loop (etol_psopt_example1.cpp:163-176); they
// depend only on the XML, so they are computed once here -- same operations,
// same order: centre (midpoint in x, point on the edge's line in y), squared
// half-length, rotation angle, b^2 = 0.2 a^2.  A vertical edge divides by zero
// exactly as the reference does (:169).
int emi_edge_ellipse(double xa, double ya, double xb, double yb, double* rec8) {
    if (!rec8) return EMI_ERR_ARG;
    const double xc = (xb + xa) / 2.;
    const double m = (yb - ya) / (xb - xa);
    const double yc = ya + m * (xc - xa);
    const double radsq = std::pow(xc - xa, 2.0) + std::pow(yc - ya, 2.0);
    const double tt = -1.0 * std::atan2(yc - ya, xc - xa);
    rec8[0] = (double)EMI_PATH_ELLIPSE;
    rec8[1] = xc;
    rec8[2] = yc;
    rec8[3] = std::cos(tt);
    rec8[4] = std::sin(tt);
    rec8[5] = radsq;
    rec8[6] = .2 * radsq;
    rec8[7] = 0.0;
    return EMI_OK;
}

// Waypoint table -> disc centre at each node time.  Bracket rule of the
// reference's linear_interpolation (TrajectoryOptimizer.hpp:239-258): before
// the table use segment 0, after it the last segment, inside it the LAST
// segment whose closed interval contains t.
int emi_track_centres(int nway, const double* t, const double* x, const double* y, int M,
                      const double* node_t, double* xc, double* yc) {
    if (nway < 2 || !t || !x || !y || M < 1 || !node_t || !xc || !yc) return EMI_ERR_ARG;
    for (int k = 0; k < M; ++k) {
        const double tv = node_t[k];
        int j = 0;
        if (tv > t[nway - 1]) {
            j = nway - 2;
        } else if (tv >= t[0]) {
            for (int s = 0; s + 1 < nway; ++s)
                if (tv >= t[s] && tv <= t[s + 1]) j = s;
        }
        const double dt = t[j + 1] - t[j];
        xc[k] = (tv - t[j]) * (x[j + 1] - x[j]) / dt + x[j];
        yc[k] = (tv - t[j]) * (y[j + 1] - y[j]) / dt + y[j];
    }
    return EMI_OK;
}

// Prolongation between two LGL meshes (the mesh ladder, emi_ipm_ladder.hip): P[Mf][Mc], row q = the Lagrange basis
// polynomials of the coarse nodes at tau_f[q], barycentric second form with the weights (-1)^j sqrt(w_j) (interp_lgl of
// host/eMI355X.cpp as a matrix).  No product feeds a sum here: there is nothing a compiler could contract.
int emi_prolong_matrix(int Mc, const double* tau_c, const double* w_c, int Mf, const double* tau_f, double* P) {
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

// The route of planned_path_guess past the static records, as the header specifies it (arithmetic: emi_plan_route.hpp, shared with
// the kernels of emi_start_guess_dev).  The distances here come from Dijkstra over all cells; the device relaxes to the same fixed point.
int emi_plan_route(int np, const double* recs, const double ends[4], const double box[4], double clearance, int grid, int M,
                   const double* tau, double* xs, double* ys, int* level, double* cost, int* cells, int* ncells) {
    namespace P = emi_plan;
    const int N = grid == 0 ? P::GRID_DEFAULT : grid;
    if (np < 0 || (np > 0 && !recs) || !ends || !tau || !xs || !ys || !level || M < 2 || N < P::GRID_MIN || N > P::GRID_MAX ||
        clearance != clearance)
        return EMI_ERR_ARG;
    if (cost) *cost = 0.0;
    if (ncells) *ncells = 0;
    const P::Geom g = P::geom(ends, box, clearance, N);
    if (g.level == -2 || P::count_static(np, recs) == 0) { *level = -2; return EMI_OK; }
    const size_t n2 = (size_t)N * N;
    std::vector<double> cellcost(n2), dist(n2), px(n2), py(n2), arc(n2);
    std::vector<unsigned char> bits(n2);
    std::vector<int> path(n2);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) P::cell_eval(g, np, recs, i, j, &cellcost[(size_t)i * N + j], &bits[(size_t)i * N + j]);
    *level = -1;
    for (int lv = 0; lv < P::LEVELS; ++lv) {
        std::fill(dist.begin(), dist.end(), P::UNREACHED);
        typedef std::pair<double, int> QE;
        std::priority_queue<QE, std::vector<QE>, std::greater<QE>> pq;
        dist[g.start] = 0.0;
        pq.push({0.0, g.start});
        while (!pq.empty()) {
            const QE e = pq.top();
            pq.pop();
            if (e.first > dist[e.second]) continue;
            const int i = e.second / N, j = e.second % N;
            for (int di = -1; di <= 1; ++di)
                for (int dj = -1; dj <= 1; ++dj) {
                    const int a = i + di, b = j + dj;
                    if ((!di && !dj) || a < 0 || b < 0 || a >= N || b >= N || P::is_blocked(g, bits.data(), a * N + b, lv)) continue;
                    const double w = P::step_of(g, di, dj) * cellcost[(size_t)a * N + b];
                    const double d = e.first + w;
                    if (d < dist[(size_t)a * N + b]) { dist[(size_t)a * N + b] = d; pq.push({d, a * N + b}); }
                }
        }
        if (!(dist[g.goal] < P::UNREACHED)) continue;       // no route with the keep-outs grown this much: try them smaller
        const int L = P::trace(g, dist.data(), cellcost.data(), path.data(), px.data(), py.data(), arc.data());
        if (L == 0) return EMI_OK;                          // (level -1)
        for (int k = 0; k < M; ++k) P::resample(L, px.data(), py.data(), arc.data(), tau[k], &xs[k], &ys[k]);
        *level = lv;
        if (cost) *cost = dist[g.goal];
        if (ncells) *ncells = L;
        if (cells) std::copy(path.begin(), path.begin() + L, cells);
        return EMI_OK;
    }
    return EMI_OK;
}

// What becomes of an instance of the lock-step mesh refinement after its solve on a rung: 1 where it retires, 0 where it
// climbs, and the verdict (the table in emi355x.h).
int emi_ipm_refine_decide(int status, double err, double ode_tol, int has_good, int is_last, int* verdict) {
    const bool ok = status == EMI_IPM_CONVERGED || status == EMI_IPM_ACCEPTABLE;
    const bool met = std::isfinite(err) && err <= ode_tol;
    const int v = ok ? (met ? EMI_REFINE_MET : EMI_REFINE_NOT_MET) : (has_good ? EMI_REFINE_FELL_BACK : EMI_REFINE_FAILED);
    if (verdict) *verdict = v;
    return !(ok && !met && !is_last);
}

// Whether an instance that ended an attempt of emi_ipm_solve_restart_* with this verdict is solved again from the next start.
int emi_ipm_restart_decide(int verdict, int retry_mask) {
    if (verdict < EMI_REFINE_MET || verdict > EMI_REFINE_FAILED) return 0;
    const int mask = retry_mask ? retry_mask : 1 << EMI_REFINE_FAILED;
    return (mask >> verdict) & 1;
}

}  // extern "C"
