// emi_nlp.cpp -- primal-dual interior-point iteration for the transcribed VGP.
// See emi_nlp.hpp for what this stands in for in the reference (IPOPT behind
// PSOPT, src/ePSOPT/ePSOPT.cpp:62-66,84).  Written from the published
// algorithm (Waechter & Biegler 2006: barrier subproblems, fraction-to-the-
// boundary rule, second-order correction, acceptable-level termination), with
// an l1 merit function instead of a filter, and with the inertia of the KKT
// matrix fixed by construction instead of by trial factorisations: the node
// blocks of the Hessian are made positive definite (quasi-definite matrix for
// the backend: Cholesky of a Schur complement on the device) and the exact
// matrix comes back, together with an exact inertia verdict, through a
// low-rank correction.
//
// NLP in per-instance numbering (DESIGN.md "NLP layout"):
//   variables   z (states then controls, index v*M+k), slacks s for the path rows
//   equalities  defect_(i,k)(z) = 0,   c_(j,k)(z) - s_(j,k) = 0
//   bounds      zl <= z <= zu (zl==zu removes the variable), cl_j <= s_(j,k) <= cu_j
// The boundary conditions of ePSOPT::events (ePSOPT.cpp:137-141, 281-291) act
// directly on node variables, so they arrive here as variable bounds.
#include "emi_nlp.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ETOL {
namespace mi355x {

// ---------------------------------------------------------------------------------------------
// Bunch-Kaufman LDL^T, lower triangle, unblocked
// ---------------------------------------------------------------------------------------------
bool ldlt_factor(LdltFactor& F) {
    const int n = F.n;
    double* A = F.a.data();
    F.ipiv.assign(n, 0);
    F.npos = F.nneg = F.nzero = 0;
    const double alpha = (1.0 + std::sqrt(17.0)) / 8.0;
    auto at = [&](int i, int j) -> double& { return A[(size_t)i * n + j]; };
    bool ok = true;
    int k = 0;
    while (k < n) {
        int kstep = 1, kp = k;
        const double absakk = std::fabs(at(k, k));
        int imax = k;
        double colmax = 0.0;
        for (int i = k + 1; i < n; ++i)
            if (std::fabs(at(i, k)) > colmax) { colmax = std::fabs(at(i, k)); imax = i; }
        if (std::max(absakk, colmax) == 0.0) {
            ok = false;
            F.ipiv[k] = k;
            ++F.nzero;
            ++k;
            continue;
        }
        if (absakk < alpha * colmax) {
            double rowmax = 0.0;
            for (int j = k; j < imax; ++j) rowmax = std::max(rowmax, std::fabs(at(imax, j)));
            for (int i = imax + 1; i < n; ++i) rowmax = std::max(rowmax, std::fabs(at(i, imax)));
            if (absakk >= alpha * colmax * (colmax / rowmax)) kp = k;
            else if (std::fabs(at(imax, imax)) >= alpha * rowmax) kp = imax;
            else { kp = imax; kstep = 2; }
        }
        const int kk = k + kstep - 1;
        if (kp != kk) {   // symmetric interchange of rows/columns kk and kp in the trailing block
            for (int i = kp + 1; i < n; ++i) std::swap(at(i, kk), at(i, kp));
            for (int j = kk + 1; j < kp; ++j) std::swap(at(j, kk), at(kp, j));
            std::swap(at(kk, kk), at(kp, kp));
            if (kstep == 2) std::swap(at(k + 1, k), at(kp, k));
        }
        if (kstep == 1) {
            const double piv = at(k, k);
            (piv > 0 ? F.npos : F.nneg)++;
            const double r = 1.0 / piv;
            for (int j = k + 1; j < n; ++j) {
                const double ajk = at(j, k) * r;
                if (ajk != 0.0)
                    for (int i = j; i < n; ++i) at(i, j) -= at(i, k) * ajk;
            }
            for (int i = k + 1; i < n; ++i) at(i, k) *= r;
            F.ipiv[k] = kp;
        } else {
            const double a11 = at(k, k), a21 = at(k + 1, k), a22 = at(k + 1, k + 1);
            const double det = a11 * a22 - a21 * a21, tr = a11 + a22;
            if (det < 0) { ++F.npos; ++F.nneg; }
            else if (det > 0) { (tr > 0 ? F.npos : F.nneg) += 2; }
            else { ++F.nzero; (tr > 0 ? F.npos : F.nneg)++; }
            if (k + 2 < n) {
                const double d11 = a22 / a21, d22 = a11 / a21;
                const double t = 1.0 / (d11 * d22 - 1.0), d21 = t / a21;
                for (int j = k + 2; j < n; ++j) {
                    const double wk = d21 * (d11 * at(j, k) - at(j, k + 1));
                    const double wk1 = d21 * (d22 * at(j, k + 1) - at(j, k));
                    for (int i = j; i < n; ++i) at(i, j) -= at(i, k) * wk + at(i, k + 1) * wk1;
                    at(j, k) = wk;
                    at(j, k + 1) = wk1;
                }
            }
            F.ipiv[k] = F.ipiv[k + 1] = -(kp + 1);
        }
        k += kstep;
    }
    return ok;
}

void ldlt_solve(const LdltFactor& F, double* b) {
    const int n = F.n;
    const double* A = F.a.data();
    auto at = [&](int i, int j) -> double { return A[(size_t)i * n + j]; };
    int k = 0;
    while (k < n) {   // L D y = P b
        if (F.ipiv[k] >= 0) {
            const int kp = F.ipiv[k];
            if (kp != k) std::swap(b[k], b[kp]);
            for (int i = k + 1; i < n; ++i) b[i] -= at(i, k) * b[k];
            b[k] /= at(k, k);
            ++k;
        } else {
            const int kp = -F.ipiv[k] - 1;
            if (kp != k + 1) std::swap(b[k + 1], b[kp]);
            for (int i = k + 2; i < n; ++i) b[i] -= at(i, k) * b[k] + at(i, k + 1) * b[k + 1];
            const double a21 = at(k + 1, k);
            const double akm1 = at(k, k) / a21, ak = at(k + 1, k + 1) / a21;
            const double den = akm1 * ak - 1.0;
            const double bkm1 = b[k] / a21, bk = b[k + 1] / a21;
            b[k] = (ak * bkm1 - bk) / den;
            b[k + 1] = (akm1 * bk - bkm1) / den;
            k += 2;
        }
    }
    k = n - 1;
    while (k >= 0) {   // L^T x = y, undo P
        if (F.ipiv[k] >= 0) {
            double s = b[k];
            for (int i = k + 1; i < n; ++i) s -= at(i, k) * b[i];
            b[k] = s;
            const int kp = F.ipiv[k];
            if (kp != k) std::swap(b[k], b[kp]);
            --k;
        } else {
            double s0 = b[k - 1], s1 = b[k];
            for (int i = k + 1; i < n; ++i) {
                s0 -= at(i, k - 1) * b[i];
                s1 -= at(i, k) * b[i];
            }
            b[k - 1] = s0;
            b[k] = s1;
            const int kp = -F.ipiv[k] - 1;
            if (kp != k) std::swap(b[k], b[kp]);
            k -= 2;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// interior point
// ---------------------------------------------------------------------------------------------
// Path rows are elastic:  sigma_j c_j(z) - s - e+ + e- = 0,  cl <= s <= cu,  e+- >= 0, with the
// exact penalty rho (e+ + e-) in the objective.  A strictly interior start then always exists
// (a straight-line guess usually crosses keep-outs, where a plain slack formulation jams against
// the slack bound), and for rho above the row multipliers the minimiser has e = 0, i.e. it is a
// KKT point of the original problem.  rho is raised and the iteration continued if some e stays
// positive at convergence.
namespace {

constexpr double INF_BOUND = 1e19;
}  // namespace

void assemble_node_blocks(const double* H, const double* VALS, const double* Sigma, const double* sig_t, const unsigned char* fixed,
                          double dw_shift, const std::vector<std::vector<std::pair<int, int>>>& rv, int nv, int M, double* Qblk) {
    const int nh = nv * (nv + 1) / 2, np = (int)rv.size();
    std::copy(H, H + (size_t)nh * M, Qblk);
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < M; ++k) {
            const int qq = v * M + k;
            Qblk[(size_t)(v * (v + 1) / 2 + v) * M + k] += Sigma[qq] + (fixed[qq] ? 0.0 : dw_shift);
        }
    // eliminated path rows: sum_j sig_j (grad c_j)(grad c_j)^T on the variables each row depends on
    for (int j = 0; j < np; ++j)
        for (size_t a = 0; a < rv[j].size(); ++a)
            for (size_t b = 0; b <= a; ++b) {
                const int va = rv[j][a].first, vb = rv[j][b].first;
                const int hi = std::max(va, vb), lo = std::min(va, vb);
                double* q = &Qblk[(size_t)(hi * (hi + 1) / 2 + lo) * M];
                const double* ga = &VALS[(size_t)rv[j][a].second * M];
                const double* gb = &VALS[(size_t)rv[j][b].second * M];
                const double* sg = &sig_t[(size_t)j * M];
                for (int k = 0; k < M; ++k) q[k] += sg[k] * ga[k] * gb[k];
            }
}

// Makes every node block of Q (packed lower triangles, Qblk[nh][M]) positive definite over its free
// variables: cyclic Jacobi eigen-decomposition of the (at most 16 x 16) block; if an eigenvalue is
// below eps * max|lambda|, the block is rebuilt from max(|lambda|, floor).  Returns the largest
// shift applied to an eigenvalue (0: nothing was modified).
double convexify_node_blocks(double* Qblk, const unsigned char* fixed, int nv, int M, std::vector<BlockMod>* mods) {
    constexpr int NMAX = 16;
    mods->clear();
    if (nv > NMAX) return 0.0;
    double worst = 0.0;
    double A[NMAX][NMAX], Vv[NMAX][NMAX], lam[NMAX], d[NMAX];
    // thresholds in the diagonally scaled block (unit diagonal): a block mixes barrier terms of 1e10 with
    // curvatures of 1e-2, and only after scaling is "zero" distinguishable from "negative"
    const double fl = 1e-9;
    for (int k = 0; k < M; ++k) {
        for (int v = 0; v < nv; ++v)
            for (int q = 0; q <= v; ++q) {
                const bool fx = fixed[v * M + k] || fixed[q * M + k];
                A[v][q] = A[q][v] = fx ? (v == q ? 1.0 : 0.0) : Qblk[(size_t)(v * (v + 1) / 2 + q) * M + k];
            }
        double amax = 0;
        for (int v = 0; v < nv; ++v) amax = std::max(amax, std::fabs(A[v][v]));
        for (int v = 0; v < nv; ++v)
            for (int q = 0; q < v; ++q) amax = std::max(amax, std::fabs(A[v][q]));
        if (amax == 0.0) amax = 1.0;
        for (int v = 0; v < nv; ++v) d[v] = std::sqrt(std::max(std::fabs(A[v][v]), 1e-12 * amax));
        for (int v = 0; v < nv; ++v)
            for (int q = 0; q < nv; ++q) A[v][q] /= d[v] * d[q];          // congruence: inertia unchanged
        // cheap screen: a block whose Cholesky runs through with comfortable pivots is left alone
        {
            double Lc[NMAX][NMAX];
            bool pd = true;
            for (int i = 0; i < nv && pd; ++i)
                for (int j = 0; j <= i; ++j) {
                    double sum = A[i][j];
                    for (int t = 0; t < j; ++t) sum -= Lc[i][t] * Lc[j][t];
                    if (i == j) {
                        if (!(sum > 10.0 * fl)) { pd = false; break; }
                        Lc[i][i] = std::sqrt(sum);
                    } else {
                        Lc[i][j] = sum / Lc[j][j];
                    }
                }
            if (pd) continue;
        }
        for (int i = 0; i < nv; ++i)
            for (int j = 0; j < nv; ++j) Vv[i][j] = i == j ? 1.0 : 0.0;
        for (int sweep = 0; sweep < 30; ++sweep) {
            double off = 0, dia = 0;
            for (int i = 0; i < nv; ++i) {
                dia += A[i][i] * A[i][i];
                for (int j = 0; j < i; ++j) off += A[i][j] * A[i][j];
            }
            if (off < 1e-32 * std::max(1.0, dia)) break;
            for (int p = 0; p < nv; ++p)
                for (int q = p + 1; q < nv; ++q) {
                    if (A[p][q] == 0.0) continue;
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                    for (int r = 0; r < nv; ++r) {
                        const double arp = A[r][p], arq = A[r][q];
                        A[r][p] = c * arp - sn * arq;
                        A[r][q] = sn * arp + c * arq;
                    }
                    for (int r = 0; r < nv; ++r) {
                        const double apr = A[p][r], aqr = A[q][r];
                        A[p][r] = c * apr - sn * aqr;
                        A[q][r] = sn * apr + c * aqr;
                    }
                    for (int r = 0; r < nv; ++r) {
                        const double vrp = Vv[r][p], vrq = Vv[r][q];
                        Vv[r][p] = c * vrp - sn * vrq;
                        Vv[r][q] = sn * vrp + c * vrq;
                    }
                }
        }
        for (int i = 0; i < nv; ++i) {
            lam[i] = A[i][i];
            const double nl = std::max(std::fabs(lam[i]), fl);
            // a (numerically) zero eigenvalue is floored without bookkeeping -- a perturbation of 1e-9 of
            // the diagonal; reflected, genuinely negative ones become columns of the low-rank correction
            if (lam[i] < -fl) {
                BlockMod m;
                m.node = k;
                m.delta = nl - lam[i];
                for (int r = 0; r < nv; ++r) m.v[r] = d[r] * Vv[r][i];
                mods->push_back(m);
                worst = std::max(worst, m.delta * d[0] * d[0]);
            }
            lam[i] = nl;
        }
        for (int v = 0; v < nv; ++v)
            for (int q = 0; q <= v; ++q) {
                if (fixed[v * M + k] || fixed[q * M + k]) continue;
                double sum = 0;
                for (int e = 0; e < nv; ++e) sum += Vv[v][e] * lam[e] * Vv[q][e];
                Qblk[(size_t)(v * (v + 1) / 2 + q) * M + k] = d[v] * d[q] * sum;
            }
    }
    return worst;
}

namespace {

// Host backend: the same matrix as etol_amd/csrc/emi_kkt.hip assembles, dense LDL^T (Bunch-Kaufman).
class DenseHostKkt : public KktBackend {
 public:
    explicit DenseHostKkt(const NlpProblem& P) : _P(P) {}
    int factor(const double* Qblk, const double* Jblk, const unsigned char* fx, double dc) override {
        const int M = _P.M, ns = _P.ns, nv = ns + _P.nc, nz = nv * M, md = ns * M, N = nz + md + (int)_P.links.size() * M;
        _F.n = N;
        _r = 0;
        _F.a.assign((size_t)N * N, 0.0);
        _fixed.assign(fx, fx + nz);
        double* a = _F.a.data();
        for (int k = 0; k < M; ++k)
            for (int v = 0; v < nv; ++v) {
                if (_fixed[v * M + k]) { a[(size_t)(v * M + k) * N + v * M + k] = 1.0; continue; }
                for (int q = 0; q <= v; ++q)
                    if (!_fixed[q * M + k]) a[(size_t)(v * M + k) * N + q * M + k] = Qblk[(size_t)(v * (v + 1) / 2 + q) * M + k];
            }
        for (int i = 0; i < ns; ++i)
            for (int k = 0; k < M; ++k) {
                double* row = a + (size_t)(nz + i * M + k) * N;
                for (int j = 0; j < M; ++j)
                    if (!_fixed[i * M + j]) row[i * M + j] = _P.D[(size_t)k * M + j];
                for (int v = 0; v < nv; ++v)
                    if (!_fixed[v * M + k]) row[v * M + k] = Jblk[(size_t)(i * nv + v) * M + k];
                row[nz + i * M + k] = -dc;
            }
        // coupling rows  z[dst][k] - sum_j W[k][j] z[src][j] = 0  (delayed values): constant entries, regularised like the defects
        for (size_t l = 0; l < _P.links.size(); ++l) {
            const NlpLink& L = _P.links[l];
            for (int k = 0; k < M; ++k) {
                double* row = a + (size_t)(nz + md + (int)l * M + k) * N;
                for (int j = 0; j < M; ++j)
                    if (!_fixed[L.src * M + j]) row[L.src * M + j] = -L.W[(size_t)k * M + j];
                if (!_fixed[L.dst * M + k]) row[L.dst * M + k] += 1.0;
                row[nz + md + (int)l * M + k] = -dc;
            }
        }
        _ok = ldlt_factor(_F) && _F.nzero == 0;
        return _ok ? 0 : 1;
    }
    int lowrank(int r, const int* node, const double* vec, const double* delta, bool* exact) override {
        _r = 0;
        *exact = r == 0;
        if (r == 0) return 0;
        if (!_ok) return -1;
        const int M = _P.M, nv = _P.ns + _P.nc, N = _F.n;
        _node.assign(node, node + r);
        _vec.assign(vec, vec + (size_t)r * nv);
        _Y.assign((size_t)N * r, 0.0);
        for (int c = 0; c < r; ++c) {
            double* y = &_Y[(size_t)c * N];
            for (int v = 0; v < nv; ++v) y[v * M + node[c]] = vec[(size_t)c * nv + v];
            for (size_t q = 0; q < _fixed.size(); ++q)
                if (_fixed[q]) y[q] = 0.0;
            ldlt_solve(_F, y);
        }
        // C = Delta^-1 - U^T Y, row-major lower triangle; right-looking Cholesky
        _C.assign((size_t)r * r, 0.0);
        for (int c = 0; c < r; ++c) {
            const double* y = &_Y[(size_t)c * N];
            for (int a = c; a < r; ++a) {
                double dot = 0;
                for (int v = 0; v < nv; ++v) dot += vec[(size_t)a * nv + v] * y[v * M + node[a]];
                _C[(size_t)a * r + c] = -dot;
            }
            _C[(size_t)c * r + c] += 1.0 / delta[c];
        }
        std::vector<double> colj(r);
        for (int j = 0; j < r; ++j) {
            const double djj = _C[(size_t)j * r + j];
            if (!(djj > 1e-14 * (1.0 / delta[j]))) return 0;          // not positive definite: K~ answers stay
            const double ljj = std::sqrt(djj);
            _C[(size_t)j * r + j] = ljj;
            for (int i = j + 1; i < r; ++i) {
                _C[(size_t)i * r + j] /= ljj;
                colj[i] = _C[(size_t)i * r + j];
            }
            for (int i = j + 1; i < r; ++i) {
                const double lij = colj[i];
                double* row = &_C[(size_t)i * r];
                for (int t = j + 1; t <= i; ++t) row[t] -= lij * colj[t];
            }
        }
        _r = r;
        *exact = true;
        return 0;
    }
    int solve(double* rhs, int nrhs) override {
        if (!_ok) return -1;
        const int M = _P.M, nv = _P.ns + _P.nc, N = _F.n;
        std::vector<double> t(_r);
        for (int c = 0; c < nrhs; ++c) {
            double* b = rhs + (size_t)c * N;
            for (size_t q = 0; q < _fixed.size(); ++q)
                if (_fixed[q]) b[q] = 0.0;
            ldlt_solve(_F, b);
            if (_r == 0) continue;
            // b <- b + Y C^-1 (U^T b)
            for (int a = 0; a < _r; ++a) {
                double dot = 0;
                for (int v = 0; v < nv; ++v) dot += _vec[(size_t)a * nv + v] * b[v * M + _node[a]];
                t[a] = dot;
            }
            for (int i = 0; i < _r; ++i) {
                double sum = t[i];
                for (int q = 0; q < i; ++q) sum -= _C[(size_t)i * _r + q] * t[q];
                t[i] = sum / _C[(size_t)i * _r + i];
            }
            for (int i = _r - 1; i >= 0; --i) {
                double sum = t[i];
                for (int q = i + 1; q < _r; ++q) sum -= _C[(size_t)q * _r + i] * t[q];
                t[i] = sum / _C[(size_t)i * _r + i];
            }
            for (int a = 0; a < _r; ++a) {
                const double* y = &_Y[(size_t)a * N];
                const double ta = t[a];
                for (int q = 0; q < N; ++q) b[q] += ta * y[q];
            }
        }
        return 0;
    }
    std::string last_error() const override { return "dense host factorisation"; }

 private:
    const NlpProblem& _P;
    LdltFactor _F;
    std::vector<unsigned char> _fixed;
    bool _ok = false;
    int _r = 0;                       // active low-rank correction (0: none)
    std::vector<int> _node;
    std::vector<double> _vec, _Y, _C;
};

}  // namespace

// ---- variable scaling (PSOPT's scaling = "automatic", reference src/ePSOPT/ePSOPT.cpp:63) ------------------------------
// PSOPT iterates on  z~_v = z_v / s_v  with s_v taken from the variable's bounds, and scales the defect rows of state i like
// state i ("state-based" defect scaling, its default).  With one scale per state / control (the same at every node) the scaled
// transcription has the SAME shape as the unscaled one:  (D x_i - h f_i) / s_i = D x~_i - h f_i / s_i,  so D, the node-diagonal
// Jacobian entries and the packed node blocks of the Hessian keep their layouts and only their values change:
//     defect rows / s_i;   f-partial (i, v) * s_v / s_i  (the entry (i, i) carries D_kk: factor 1);   path partials and the cost
//     gradient * s_v;   Hessian entry (v, q) * s_v s_q, evaluated with the multipliers lambda~_i / s_i.
// The evaluator and the KKT backend of the caller are used as they are (the backend reads D from its own context).
// The example's defect_scaling = "jacobian-based" (etol_psopt_example1.cpp:91: one scale per defect ROW) would break the
// D (x) I structure the Newton step is built on and is not offered.
class ScaledEvaluator : public NlpEvaluator {
 public:
    ScaledEvaluator(const NlpProblem& P, const std::vector<std::vector<std::pair<int, int>>>& rv, int npart)
        : in_(P.ev), s_(P.vscale), rv_(rv), ns_(P.ns), nc_(P.nc), M_(P.M), npart_(npart), z_((size_t)(P.ns + P.nc) * P.M),
          lam_((size_t)P.ns * P.M) {}
    int eval(const double* X, const double* U, double* RES, double* VALS, double* COST, bool jac) override {
        unscale(X, U);
        const int rc = in_->eval(z_.data(), z_.data() + (size_t)ns_ * M_, RES, VALS, COST, jac);
        if (rc != 0) return rc;
        const int nv = ns_ + nc_;
        for (int i = 0; i < ns_; ++i) {
            const double inv = 1.0 / s_[i];
            for (int k = 0; k < M_; ++k) RES[(size_t)i * M_ + k] *= inv;
        }
        if (jac && VALS) {
            for (int i = 0; i < ns_; ++i)
                for (int v = 0; v < nv; ++v) {
                    if (v == i) continue;
                    const double f = s_[v] / s_[i];
                    double* e = VALS + (size_t)(i * nv + v) * M_;
                    for (int k = 0; k < M_; ++k) e[k] *= f;
                }
            for (const auto& row : rv_)
                for (const auto& ve : row) {
                    double* e = VALS + (size_t)ve.second * M_;
                    for (int k = 0; k < M_; ++k) e[k] *= s_[ve.first];
                }
            for (int v = 0; v < nv; ++v) {
                double* e = VALS + (size_t)(ns_ * nv + npart_ + v) * M_;
                for (int k = 0; k < M_; ++k) e[k] *= s_[v];
            }
        }
        return 0;
    }
    int hess(const double* X, const double* U, const double* lamF, const double* lamC, double sigma, double* H) override {
        unscale(X, U);
        for (int i = 0; i < ns_; ++i)
            for (int k = 0; k < M_; ++k) lam_[(size_t)i * M_ + k] = lamF[(size_t)i * M_ + k] / s_[i];
        const int rc = in_->hess(z_.data(), z_.data() + (size_t)ns_ * M_, lam_.data(), lamC, sigma, H);
        if (rc != 0) return rc;
        const int nv = ns_ + nc_;
        for (int hi = 0; hi < nv; ++hi)
            for (int lo = 0; lo <= hi; ++lo) {
                const double f = s_[hi] * s_[lo];
                if (f == 1.0) continue;
                double* e = H + (size_t)(hi * (hi + 1) / 2 + lo) * M_;
                for (int k = 0; k < M_; ++k) e[k] *= f;
            }
        return 0;
    }
    std::string last_error() const override { return in_->last_error(); }

 private:
    void unscale(const double* X, const double* U) {
        for (int v = 0; v < ns_; ++v)
            for (int k = 0; k < M_; ++k) z_[(size_t)v * M_ + k] = X[(size_t)v * M_ + k] * s_[v];
        for (int j = 0; j < nc_; ++j)
            for (int k = 0; k < M_; ++k) z_[(size_t)(ns_ + j) * M_ + k] = U[(size_t)j * M_ + k] * s_[ns_ + j];
    }
    NlpEvaluator* in_;
    std::vector<double> s_;
    std::vector<std::vector<std::pair<int, int>>> rv_;
    int ns_, nc_, M_, npart_;
    std::vector<double> z_, lam_;
};

// ---- the array arithmetic of one iteration (emi_nlp.hpp: IpmDims and what follows it) -----------------------------------------
namespace {

// the bound tests and scaled row bounds of solve_nlp, on an IpmDims
struct IpmB {
    const IpmDims& P;
    bool free_var(int q) const { return P.zu[q] > P.zl[q]; }
    bool hasL(int q) const { return P.zl[q] > -INF_BOUND; }
    bool hasU(int q) const { return P.zu[q] < INF_BOUND; }
    bool shasL(int r) const { return P.cl[r / P.M] > -INF_BOUND; }
    bool shasU(int r) const { return P.cu[r / P.M] < INF_BOUND; }
    double cL(int r) const { return P.cls[r / P.M]; }
    double cU(int r) const { return P.cus[r / P.M]; }
    int nz() const { return P.nv * P.M; }
    int md() const { return P.ns * P.M; }
    int mc() const { return P.np * P.M; }
    int me() const { return P.ns * P.M + P.ml; }
};
inline double ipm_eqr(const IpmDims& P, const IpmRes& e, int r) { const int md = P.ns * P.M; return r < md ? e.RES[r] : e.LNK[r - md]; }
inline double ipm_row_res(const IpmDims& P, const IpmRes& e, const double* s, const double* e1, const double* e2, int r) {
    return e.RES[(size_t)P.ns * P.M + r] - s[r] - e1[r] + e2[r];
}

}  // namespace

void ipm_eliminate_rows(const IpmDims& P, const IpmPoint& x, const IpmDuals& d, const IpmRes& e, double mu, double rho, const IpmElim& out) {
    const IpmB b{P};
    const int mc = b.mc();
    for (int r = 0; r < mc; ++r) {
        double sg = 0, rh = -d.y[r];
        if (b.shasL(r)) { const double g = x.s[r] - b.cL(r); sg += d.vL[r] / g; rh -= mu / g; }
        if (b.shasU(r)) { const double g = b.cU(r) - x.s[r]; sg += d.vU[r] / g; rh += mu / g; }
        out.sig_s[r] = sg;
        out.rhat_s[r] = rh;
        const double a1 = x.e1[r] / d.w1[r], a2 = x.e2[r] / d.w2[r];
        out.sig_t[r] = 1.0 / (1.0 / sg + a1 + a2);
        out.r_t[r] = ipm_row_res(P, e, x.s, x.e1, x.e2, r) + rh / sg - a1 * (d.y[r] - rho + mu / x.e1[r]) -
                     a2 * (d.y[r] + rho - mu / x.e2[r]);
    }
}

void ipm_barrier_diagonal(const IpmDims& P, const IpmPoint& x, const IpmDuals& d, double* Sigma) {
    const IpmB b{P};
    const int nz = b.nz();
    for (int qq = 0; qq < nz; ++qq) {
        double sg = 0.0;
        if (b.free_var(qq)) {
            if (b.hasL(qq)) sg += d.zL[qq] / (x.z[qq] - P.zl[qq]);
            if (b.hasU(qq)) sg += d.zU[qq] / (P.zu[qq] - x.z[qq]);
        }
        Sigma[qq] = sg;
    }
}

void ipm_fill_rt(const IpmDims& P, const IpmPoint& x, const IpmDuals& d, const double* rowres, double mu, double rho, const IpmElim& el) {
    const int mc = P.np * P.M;
    for (int r = 0; r < mc; ++r) {
        const double a1 = x.e1[r] / d.w1[r], a2 = x.e2[r] / d.w2[r];
        el.r_t[r] = rowres[r] + el.rhat_s[r] / el.sig_s[r] - a1 * (d.y[r] - rho + mu / x.e1[r]) -
                    a2 * (d.y[r] + rho - mu / x.e2[r]);
    }
}

void ipm_build_rhs(const IpmDims& P, const IpmPoint& x, const double* gradf, const double* jtl, const double* VALS, const IpmElim& el,
                   const double* eqres, double mu, double* out) {
    const IpmB b{P};
    const int nz = b.nz(), me = b.me(), M = P.M, np = P.np;
    const double* V = VALS;
    const auto& rv = *P.row_vars;
    std::fill(out, out + (size_t)nz + me, 0.0);
    for (int q = 0; q < nz; ++q) {
        if (!b.free_var(q)) continue;
        double r = gradf[q] + jtl[q];
        if (b.hasL(q)) r -= mu / (x.z[q] - P.zl[q]);
        if (b.hasU(q)) r += mu / (P.zu[q] - x.z[q]);
        out[q] = -r;
    }
    for (int j = 0; j < np; ++j)
        for (int k = 0; k < M; ++k) {
            const double t = el.sig_t[j * M + k] * el.r_t[j * M + k];
            for (const auto& ve : rv[j])
                if (b.free_var(ve.first * M + k)) out[ve.first * M + k] -= V[(size_t)ve.second * M + k] * t;
        }
    for (int r = 0; r < me; ++r) out[nz + r] = -eqres[r];
}

void ipm_expand_step(const IpmDims& P, const IpmPoint& x, const IpmDuals& d, const double* VALS, const IpmElim& el, double mu, double rho,
                     const IpmStep& st) {
    const IpmB b{P};
    const int nz = b.nz(), M = P.M, np = P.np;
    const double* V = VALS;
    const auto& rv = *P.row_vars;
    for (int j = 0; j < np; ++j)
        for (int k = 0; k < M; ++k) {
            const int r = j * M + k;
            double jcdz = 0.0;
            for (const auto& ve : rv[j]) jcdz += V[(size_t)ve.second * M + k] * st.dz[ve.first * M + k];
            st.dy[r] = el.sig_t[r] * (jcdz + el.r_t[r]);
            st.ds[r] = (st.dy[r] - el.rhat_s[r]) / el.sig_s[r];
            st.de1[r] = x.e1[r] / d.w1[r] * (st.dy[r] + d.y[r] - rho + mu / x.e1[r]);
            st.de2[r] = x.e2[r] / d.w2[r] * (-st.dy[r] - d.y[r] - rho + mu / x.e2[r]);
            st.dvL[r] = st.dvU[r] = 0;
            if (b.shasL(r)) { const double g = x.s[r] - b.cL(r); st.dvL[r] = mu / g - d.vL[r] - d.vL[r] / g * st.ds[r]; }
            if (b.shasU(r)) { const double g = b.cU(r) - x.s[r]; st.dvU[r] = mu / g - d.vU[r] + d.vU[r] / g * st.ds[r]; }
            st.dw1[r] = mu / x.e1[r] - d.w1[r] - d.w1[r] / x.e1[r] * st.de1[r];
            st.dw2[r] = mu / x.e2[r] - d.w2[r] - d.w2[r] / x.e2[r] * st.de2[r];
        }
    for (int q = 0; q < nz; ++q) {
        st.dzL[q] = st.dzU[q] = 0;
        if (!b.free_var(q)) continue;
        if (b.hasL(q)) { const double g = x.z[q] - P.zl[q]; st.dzL[q] = mu / g - d.zL[q] - d.zL[q] / g * st.dz[q]; }
        if (b.hasU(q)) { const double g = P.zu[q] - x.z[q]; st.dzU[q] = mu / g - d.zU[q] + d.zU[q] / g * st.dz[q]; }
    }
}

void ipm_step_lengths(const IpmDims& P, const IpmPoint& x, const IpmDuals& d, const IpmStep& st, double tau, double* apr_out, double* adu_out) {
    const IpmB b{P};
    const int nz = b.nz(), mc = b.mc();
    double apr = 1.0, adu = 1.0;
    for (int q = 0; q < nz; ++q) {
        if (!b.free_var(q)) continue;
        if (b.hasL(q) && st.dz[q] < 0) apr = std::min(apr, -tau * (x.z[q] - P.zl[q]) / st.dz[q]);
        if (b.hasU(q) && st.dz[q] > 0) apr = std::min(apr, tau * (P.zu[q] - x.z[q]) / st.dz[q]);
        if (st.dzL[q] < 0) adu = std::min(adu, -tau * d.zL[q] / st.dzL[q]);
        if (st.dzU[q] < 0) adu = std::min(adu, -tau * d.zU[q] / st.dzU[q]);
    }
    for (int r = 0; r < mc; ++r) {
        if (b.shasL(r) && st.ds[r] < 0) apr = std::min(apr, -tau * (x.s[r] - b.cL(r)) / st.ds[r]);
        if (b.shasU(r) && st.ds[r] > 0) apr = std::min(apr, tau * (b.cU(r) - x.s[r]) / st.ds[r]);
        if (st.de1[r] < 0) apr = std::min(apr, -tau * x.e1[r] / st.de1[r]);
        if (st.de2[r] < 0) apr = std::min(apr, -tau * x.e2[r] / st.de2[r]);
        if (st.dvL[r] < 0) adu = std::min(adu, -tau * d.vL[r] / st.dvL[r]);
        if (st.dvU[r] < 0) adu = std::min(adu, -tau * d.vU[r] / st.dvU[r]);
        if (st.dw1[r] < 0) adu = std::min(adu, -tau * d.w1[r] / st.dw1[r]);
        if (st.dw2[r] < 0) adu = std::min(adu, -tau * d.w2[r] / st.dw2[r]);
    }
    *apr_out = apr;
    *adu_out = adu;
}

void ipm_dphi_mmax(const IpmDims& P, const IpmPoint& x, const IpmDuals& d, const double* gradf, const IpmStep& st, const double* rs,
                   double mu, double rho, double* dphi_out, double* mmax_out) {
    const IpmB b{P};
    const int nz = b.nz(), mc = b.mc(), me = b.me();
    double dphi = 0;
    for (int q = 0; q < nz; ++q) {
        if (!b.free_var(q)) continue;
        double g = gradf[q];
        if (b.hasL(q)) g -= mu / (x.z[q] - P.zl[q]);
        if (b.hasU(q)) g += mu / (P.zu[q] - x.z[q]);
        dphi += g * st.dz[q];
    }
    for (int r = 0; r < mc; ++r) {
        double g = 0;
        if (b.shasL(r)) g -= mu / (x.s[r] - b.cL(r));
        if (b.shasU(r)) g += mu / (b.cU(r) - x.s[r]);
        dphi += g * st.ds[r] + (rho - mu / x.e1[r]) * st.de1[r] + (rho - mu / x.e2[r]) * st.de2[r];
    }
    double mmax = 0;
    for (int r = 0; r < me; ++r) mmax = std::max(mmax, std::fabs(d.lam[r] + st.dlam[r]) / rs[r]);
    for (int r = 0; r < mc; ++r) mmax = std::max(mmax, std::fabs(d.y[r] + st.dy[r]));
    *dphi_out = dphi;
    *mmax_out = mmax;
}

double ipm_barrier_merit(const IpmDims& P, const IpmPoint& x, const IpmRes& e, double cost, const double* rs, double mu_t, double nu_t,
                         double rho, double* infeas) {
    const IpmB b{P};
    const int nz = b.nz(), mc = b.mc(), me = b.me();
    double phi = cost, viol = 0;
    for (int q = 0; q < nz; ++q) {
        if (!b.free_var(q)) continue;
        if (b.hasL(q)) phi -= mu_t * std::log(x.z[q] - P.zl[q]);
        if (b.hasU(q)) phi -= mu_t * std::log(P.zu[q] - x.z[q]);
    }
    for (int r = 0; r < mc; ++r) {
        if (b.shasL(r)) phi -= mu_t * std::log(x.s[r] - b.cL(r));
        if (b.shasU(r)) phi -= mu_t * std::log(b.cU(r) - x.s[r]);
        phi += rho * (x.e1[r] + x.e2[r]) - mu_t * (std::log(x.e1[r]) + std::log(x.e2[r]));
        viol += std::fabs(ipm_row_res(P, e, x.s, x.e1, x.e2, r));
    }
    for (int r = 0; r < me; ++r) viol += rs[r] * std::fabs(ipm_eqr(P, e, r));
    if (infeas) *infeas = viol;
    return phi + nu_t * viol;
}

void ipm_slack_reset(const IpmDims& P, const double* c, const double* e1, const double* e2, double mu, double nu, double* s) {
    const IpmB b{P};
    const int mc = b.mc();
    for (int r = 0; r < mc; ++r) {
        const double target = c[r] - e1[r] + e2[r];
        const double lo = b.shasL(r) ? b.cL(r) : -INF_BOUND, hi = b.shasU(r) ? b.cU(r) : INF_BOUND;
        if (!(target > lo) || !(target < hi)) continue;
        double keep = nu * std::fabs(target - s[r]), take = 0.0;
        if (b.shasL(r)) { keep -= mu * std::log(s[r] - lo); take -= mu * std::log(target - lo); }
        if (b.shasU(r)) { keep -= mu * std::log(hi - s[r]); take -= mu * std::log(hi - target); }
        if (take < keep) s[r] = target;
    }
}

void ipm_update_duals(const IpmDims& P, const IpmPoint& x, const IpmDualsRW& d, const IpmStep& st, double a_pr, double a_du, double mu) {
    const IpmB b{P};
    const int nz = b.nz(), mc = b.mc(), me = b.me();
    const double kappa_sigma = 1e10;
    auto clampm = [&](double m, double g) { return std::max(std::min(m, kappa_sigma * mu / g), mu / (kappa_sigma * g)); };
    for (int r = 0; r < me; ++r) d.lam[r] += a_pr * st.dlam[r];
    for (int r = 0; r < mc; ++r) {
        d.y[r] += a_pr * st.dy[r];
        d.vL[r] += a_du * st.dvL[r];
        d.vU[r] += a_du * st.dvU[r];
        d.w1[r] += a_du * st.dw1[r];
        d.w2[r] += a_du * st.dw2[r];
        if (b.shasL(r)) d.vL[r] = clampm(d.vL[r], x.s[r] - b.cL(r));
        if (b.shasU(r)) d.vU[r] = clampm(d.vU[r], b.cU(r) - x.s[r]);
        d.w1[r] = clampm(d.w1[r], x.e1[r]);
        d.w2[r] = clampm(d.w2[r], x.e2[r]);
    }
    for (int q = 0; q < nz; ++q) {
        if (!b.free_var(q)) continue;
        d.zL[q] += a_du * st.dzL[q];
        d.zU[q] += a_du * st.dzU[q];
        if (b.hasL(q)) d.zL[q] = clampm(d.zL[q], x.z[q] - P.zl[q]);
        if (b.hasU(q)) d.zU[q] = clampm(d.zU[q], P.zu[q] - x.z[q]);
    }
}

double ipm_kkt_error(const IpmDims& P, const IpmPoint& x, const IpmDuals& d, const double* gradf, const double* jtl, const IpmRes& e,
                     double mu_t, double rho, double* viol_out, double* emax_out) {
    const IpmB b{P};
    const int nz = b.nz(), mc = b.mc(), me = b.me();
    double sumz = 0, summ = 0;
    int cntz = 0;
    for (int q = 0; q < nz; ++q) { sumz += d.zL[q] + d.zU[q]; cntz += (d.zL[q] > 0) + (d.zU[q] > 0); }
    for (int r = 0; r < mc; ++r) {
        sumz += d.vL[r] + d.vU[r] + d.w1[r] + d.w2[r];
        cntz += (d.vL[r] > 0) + (d.vU[r] > 0) + 2;
        summ += std::fabs(d.y[r]);
    }
    for (int r = 0; r < me; ++r) summ += std::fabs(d.lam[r]);
    const double smax = 100.0;
    const double sd = std::max(smax, (summ + sumz) / std::max(1, me + mc + cntz)) / smax;
    const double sc = std::max(smax, sumz / std::max(1, cntz)) / smax;
    double ed = 0, ep = 0, ec = 0, emax = 0;
    for (int q = 0; q < nz; ++q)
        if (b.free_var(q)) ed = std::max(ed, std::fabs(gradf[q] + jtl[q] - d.zL[q] + d.zU[q]));
    for (int r = 0; r < mc; ++r) {
        ed = std::max(ed, std::fabs(-d.y[r] - d.vL[r] + d.vU[r]));
        ed = std::max(ed, std::fabs(rho - d.y[r] - d.w1[r]));
        ed = std::max(ed, std::fabs(rho + d.y[r] - d.w2[r]));
    }
    for (int r = 0; r < me; ++r) ep = std::max(ep, std::fabs(ipm_eqr(P, e, r)));
    for (int r = 0; r < mc; ++r) {
        ep = std::max(ep, std::fabs(ipm_row_res(P, e, x.s, x.e1, x.e2, r)));
        emax = std::max(emax, std::max(x.e1[r], x.e2[r]));
    }
    for (int q = 0; q < nz; ++q) {
        if (!b.free_var(q)) continue;
        if (b.hasL(q)) ec = std::max(ec, std::fabs((x.z[q] - P.zl[q]) * d.zL[q] - mu_t));
        if (b.hasU(q)) ec = std::max(ec, std::fabs((P.zu[q] - x.z[q]) * d.zU[q] - mu_t));
    }
    for (int r = 0; r < mc; ++r) {
        if (b.shasL(r)) ec = std::max(ec, std::fabs((x.s[r] - b.cL(r)) * d.vL[r] - mu_t));
        if (b.shasU(r)) ec = std::max(ec, std::fabs((b.cU(r) - x.s[r]) * d.vU[r] - mu_t));
        ec = std::max(ec, std::fabs(x.e1[r] * d.w1[r] - mu_t));
        ec = std::max(ec, std::fabs(x.e2[r] * d.w2[r] - mu_t));
    }
    if (viol_out) *viol_out = ep;
    if (emax_out) *emax_out = emax;
    return std::max(std::max(ed / sd, ep), ec / sc);
}

// ---- the iteration: its state as an object, its phases as members ("Phases of the iteration") -------------
namespace {

using Clock = std::chrono::steady_clock;
using RowVars = std::vector<std::vector<std::pair<int, int>>>;
inline double secs_since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }
// v pushed into the interior of [l, u] (a side that is not there: hasL / hasU false)
inline double pushed_inside(double v, double l, double u, bool hasL, bool hasU, const NlpOptions& opt) {
    double pl = hasL ? opt.bound_push * std::max(1.0, std::fabs(l)) : 0, pu = hasU ? opt.bound_push * std::max(1.0, std::fabs(u)) : 0;
    if (hasL && hasU) { pl = std::min(pl, opt.bound_frac * (u - l)); pu = std::min(pu, opt.bound_frac * (u - l)); }
    if (hasL) v = std::max(v, l + pl);
    if (hasU) v = std::min(v, u - pu);
    return v;
}
inline bool all_finite(const double* v, size_t n) {
    bool fin = true;
    for (size_t r = 0; r < n && fin; ++r) fin = std::isfinite(v[r]);
    return fin;
}

struct Iterate {
    std::vector<double> z, s, e1, e2;             // primal: variables, row slacks, elastics
    std::vector<double> lam, y;                   // equality multipliers (defects then coupling rows, path rows)
    std::vector<double> zL, zU, vL, vU, w1, w2;   // bound multipliers (0 where the bound is infinite)
};
struct Eval {
    std::vector<double> RES, VALS;
    std::vector<double> LNK;          // residuals of the coupling rows (NlpProblem::links), [link][M]
    double cost = 0;
};
// an iterate with everything evaluated at it: what the residual-based acceptance keeps and takes back as a whole
struct Point : Iterate {
    Eval E;
    std::vector<double> gradf, jtl;   // cost gradient and J^T (lam, y)
};
// a Newton step with the r_t of the eliminated rows it was expanded from and its fraction-to-the-boundary lengths: what the
// second-order correction keeps and takes back as a whole
struct Step {
    std::vector<double> dz, dlam, ds, dy, de1, de2, dzL, dzU, dvL, dvU, dw1, dw2, r_t;
    double apr = 1.0, adu = 1.0;
};

// One solve.  The driver (solve_nlp) calls start(), then per iteration test_and_update_barrier(), newton_system() and
// line_search() for as long as each says `go`, then finish().  Every Ipm* view of a member array is built where it is used
// (here(), duals(), elim(), ...): none is kept across an assignment to the array it points into.
class IpmSolve {
 public:
    enum class Next { go, finish, abort };    // next phase / leave the loop and finish() / return result() as it stands

    IpmSolve(const NlpProblem& prob, const NlpOptions& options, RowVars row_vars, int n_partials)
        : P(prob), opt(options), rv(std::move(row_vars)), ns(P.ns), np(P.np), M(P.M), nv(P.ns + P.nc), nz(nv * M), md(ns * M),
          mc(np * M), nl((int)P.links.size()), ml(nl * M), me(md + ml), npart(n_partials), NN((size_t)nz + me), host_kkt(P),
          kkt(P.kkt ? P.kkt : &host_kkt), backend_blocks(opt.device_node_blocks && P.kkt != nullptr) {
        const size_t nh = (size_t)nv * (nv + 1) / 2, nvals = (size_t)ns * nv + npart + nv;
        // path rows are iterated on in scaled form  sigma_j * c_j  (same KKT points, better balanced against the defects)
        sig.assign(np, 1.0);
        if ((int)P.cscale.size() == np)
            for (int j = 0; j < np; ++j) sig[j] = P.cscale[j] > 0 ? P.cscale[j] : 1.0;
        for (int j = 0; j < np; ++j) {      // the row bounds the iteration works with: sig_j * bound where there is one
            cls.push_back(P.cl[j] > -INF_BOUND ? sig[j] * P.cl[j] : P.cl[j]);
            cus.push_back(P.cu[j] < INF_BOUND ? sig[j] * P.cu[j] : P.cu[j]);
        }
        PD.nv = nv; PD.ns = ns; PD.np = np; PD.M = M; PD.ml = ml; PD.row_vars = &rv;
        PD.zl = P.zl.data(); PD.zu = P.zu.data(); PD.cl = P.cl.data(); PD.cu = P.cu.data(); PD.cls = cls.data(); PD.cus = cus.data();
        fixed_mask.resize(nz);
        for (int q = 0; q < nz; ++q) fixed_mask[q] = B.free_var(q) ? 0 : 1;
        rs.assign(me, 1.0);
        it.E.RES.resize((size_t)(ns + np) * M);
        it.E.VALS.resize(nvals * M);
        Et.RES.resize(it.E.RES.size());
        H.resize(nh * M);
        Qblk.resize(nh * M);
        for (auto* v : {&it.gradf, &it.jtl, &zt, &Sigma, &step.dz, &step.dzL, &step.dzU}) v->resize(nz);
        for (auto* v : {&st, &e1t, &e2t, &y_unscaled, &sig_t, &sig_s, &rhat_s, &step.ds, &step.dy, &step.de1, &step.de2, &step.dvL, &step.dvU,
                        &step.dw1, &step.dw2, &step.r_t, &soc_row})
            v->resize(mc);
        for (auto* v : {&step.dlam, &eqres, &soc_def}) v->resize(me);
        for (auto* v : {&rhs_full, &rhs_keep, &resid, &x_prev, &soc_rhs}) v->resize(NN);
    }
    IpmSolve(const IpmSolve&) = delete;
    IpmSolve& operator=(const IpmSolve&) = delete;

    const NlpResult& result() const { return R; }

    // interior push of z0, first evaluation, slacks and elastics, multipliers, merit row weights, first J^T lambda
    bool start(const std::vector<double>& z0) {
        it.z = z0;
        for (int q = 0; q < nz; ++q)        // push the start into the interior of the bounds
            it.z[q] = fixed_mask[q] ? P.zl[q] : pushed_inside(it.z[q], P.zl[q], P.zu[q], B.hasL(q), B.hasU(q), opt);
        if (!evaluate(it.z, it.E, true)) return evaluator_failed(), false;
        rho = opt.rho_init > 0 ? opt.rho_init : 10.0;
        for (auto* v : {&it.s, &it.e1, &it.e2, &it.y, &it.vL, &it.vU}) v->assign(mc, 0.0);
        for (int r = 0; r < mc; ++r) {
            const double c0 = it.E.RES[(size_t)md + r];
            it.s[r] = pushed_inside(c0, B.cL(r), B.cU(r), B.shasL(r), B.shasU(r), opt);
            const double gap = c0 - it.s[r], ee = opt.bound_push * std::max(1.0, std::fabs(gap));
            it.e1[r] = std::max(gap, 0.0) + ee;     // residual c - s - e1 + e2 starts at exactly 0
            it.e2[r] = std::max(-gap, 0.0) + ee;
        }
        it.lam.assign(me, 0.0);
        if ((int)P.lamF0.size() == md) std::copy(P.lamF0.begin(), P.lamF0.end(), it.lam.begin());
        // row weights of the merit function (jacobian_defect_scaling): 1 / max(1, inf-norm of the defect row of the Jacobian at the start)
        if (P.jacobian_defect_scaling) {
            const double* V0 = it.E.VALS.data();
            for (int k = 0; k < M; ++k) {
                double dmax = 0;
                for (int j = 0; j < M; ++j)
                    if (j != k) dmax = std::max(dmax, std::fabs(P.D[(size_t)k * M + j]));
                for (int i = 0; i < ns; ++i) {
                    double nrm = dmax;
                    for (int v = 0; v < nv; ++v) nrm = std::max(nrm, std::fabs(V0[(size_t)(i * nv + v) * M + k]));
                    rs[i * M + k] = 1.0 / std::max(1.0, nrm);
                }
            }
        }
        if ((int)P.lamC0.size() == mc)      // iterated on in scaled form; inside the penalty box
            for (int r = 0; r < mc; ++r) it.y[r] = std::min(std::max(P.lamC0[r] / sig[r / M], -0.9 * rho), 0.9 * rho);
        it.zL.assign(nz, 0.0); it.zU.assign(nz, 0.0);
        it.w1.assign(mc, rho); it.w2.assign(mc, rho);
        reset_elastic_duals();
        for (int q = 0; q < nz; ++q) if (!fixed_mask[q]) { if (B.hasL(q)) it.zL[q] = 1.0; if (B.hasU(q)) it.zU[q] = 1.0; }
        for (int r = 0; r < mc; ++r) { if (B.shasL(r)) it.vL[r] = 1.0; if (B.shasU(r)) it.vU[r] = 1.0; }
        mu = opt.mu_init, nu = 1.0;
        grad_and_jt();
        return true;
    }

    // convergence, acceptable-level, locally-infeasible, iteration and time tests; stagnation rule; barrier loop with penalty escalation
    Next test_and_update_barrier(int iter) {
        R.iterations = iter;
        double viol = 0;
        err0 = kkt_error(0.0, &viol, &emax);
        R.kkt_error = err0;
        R.constr_viol = viol;
        if (opt.print_level >= 5)
            printf("iter %3d  cost %.10e  inf_pr %.2e  kkt %.2e  mu %.1e  dw %.1e  nu %.1e  emax %.1e  rho %.0e  r %d%s\n", iter,
                   it.E.cost, viol, err0, mu, dw_used, nu, emax, rho, n_mods, exact_step ? " exact" : "");
        if (err0 <= opt.tol) {
            if (emax <= std::max(opt.tol, 1e-9) * 10.0 || mc == 0) { R.ok = true; R.msg = "converged"; return Next::finish; }
            // a path row is still relaxed: the penalty was too small for it
            if (rho >= 1e12 || futile_escalation(emax)) { R.msg = "converged to a point that violates the path rows (locally infeasible)"; return Next::finish; }
            escalate_penalty();
        }
        // stagnation at round-off above the tolerance (large meshes): accept like IPOPT's acceptable level
        if (acceptable()) {
            if (++n_acceptable >= opt.acceptable_iter) { R.ok = true; R.msg = "converged to acceptable level"; return Next::finish; }
        } else {
            n_acceptable = 0;
        }
        // reflected steps that have not reduced the KKT residual of the barrier problem by 10 % over `stagnation_iters` iterations: switch the inertia search
        // on (measured, profiles/r01_notes.md: 4 costs the keep-out Monte-Carlo sets half their throughput in trial factorisations, 12 keeps it and still rescues the fixed wing)
        const double err_mu_now = kkt_error(mu, nullptr, nullptr);
        if (last_step_reflected && err_mu_now > 0.9 * stagn_ref) {
            if (++stagn >= opt.stagnation_iters) {
                search_on = true;
                if (opt.mu_restart > 1.0 && !mu_restarted && mu < 1e-4) {
                    mu_restarted = true;
                    mu = std::min(1e-3, mu * opt.mu_restart);
                    nu = 1.0;
                    stagn = 0;
                    stagn_ref = 1e300;
                    if (opt.print_level >= 5) printf("stagnation at a small barrier parameter: raised to %.1e\n", mu);
                }
            }
        } else {
            stagn = 0;
            stagn_ref = err_mu_now;
        }
        if (iter >= opt.max_iter) { R.msg = "maximum number of iterations exceeded"; return Next::finish; }
        if (secs_since(tstart) > opt.max_cpu_time) { R.msg = "time limit exceeded"; return Next::finish; }
        // barrier update (may fire several times in a row)
        const double kappa_eps = 10.0, kappa_mu = 0.2, theta_mu = 1.5;     // (kappa_sigma: ipm_update_duals)
        while (mu > opt.tol / 10.0 && kkt_error(mu, nullptr, nullptr) <= kappa_eps * mu) {
            // this barrier problem is solved.  A row multiplier at the penalty weight (or, equivalently, an elastic still far above mu / rho)
            // means the weight is too small for that row: raise it now instead of converging to a relaxed point first
            double ymax = 0;
            for (int r = 0; r < mc; ++r) ymax = std::max(ymax, std::fabs(it.y[r]));
            if (mc > 0 && (emax > std::max(1e-6, 100.0 * mu) || ymax > 0.9 * rho) && rho < 1e12) {
                if (futile_escalation(emax)) { R.msg = "the path rows stay violated while the penalty weight grows (locally infeasible)"; return Next::finish; }
                escalate_penalty();
                nu = 1.0;
                break;
            }
            mu = std::max(opt.tol / 10.0, std::min(kappa_mu * mu, std::pow(mu, theta_mu)));
            nu = 1.0;    // a new barrier problem: the penalty weight is rebuilt from its multipliers, not inherited
        }
        tau = std::max(0.99, 1.0 - mu);
        return Next::go;
    }

    // Hessian, row elimination, attempt loop (node blocks, factorisation, low-rank verdict, inertia search), refined solve -> rhs_full
    Next newton_system() {
        // exact Lagrangian Hessian blocks from the device
        for (int r = 0; r < mc; ++r) y_unscaled[r] = sig[r / M] * it.y[r];
        const auto th0 = Clock::now();
        const int hess_rc = P.ev->hess(it.z.data(), it.z.data() + (size_t)ns * M, it.lam.data(), np ? y_unscaled.data() : nullptr, 1.0, H.data());
        R.t_hess += secs_since(th0);
        if (hess_rc != 0) { R.msg = "Hessian evaluation failed: " + P.ev->last_error(); return Next::finish; }
        // eliminate (s, e+, e-) of every path row:  dy = sig_t (J_c dz + r_t)
        ipm_eliminate_rows(PD, here(), duals(), res_of(it.E), mu, rho, elim());
        // factor with inertia correction
        bool factored = false;
        double dw = 0.0, dc = 0.0;
        double dw_shift = 0.0;      // primal regularisation delta_w I of the inertia search (below)
        int shift_trials = 0;
        for (int attempt = 0; attempt < 24; ++attempt) {
            const int info = factor_node_blocks(dc, dw_shift, &dw);
            if (info < 0) { R.msg = "KKT factorisation failed: " + kkt->last_error(); return Next::abort; }
            if (info > 0) { raise_dc(dc); continue; }   // exactly singular: the defect Jacobian lost rank; regularise the dual block
            if (!lowrank_verdict()) return Next::abort;
            // Inertia search (IPOPT's delta_w): the unmodified K has the wrong inertia.  The step of the reflected blocks is the cheap answer and
            // usually a good one; where it stagnates (search_on, set by the stagnation rule) look for the smallest shift K + delta_w I_z whose inertia
            // is right instead -- the verdict for every trial comes from the same low-rank test, at the price of a factorisation each
            // (experiments, profiles/r01_notes.md: max_shift_trials = 0 switches the search off).
            if (search_on && !exact_step && !force_modified && n_mods > 0 && r_mod == n_mods && shift_trials < opt.max_shift_trials) {
                if (dw_shift == 0.0) dw_shift = dw_last_ok == 0.0 ? 1e-4 : std::max(1e-20, dw_last_ok / 3.0);
                else dw_shift *= (dw_last_ok == 0.0 ? 100.0 : 8.0);
                ++shift_trials;
                continue;
            }
            if (exact_step && dw_shift > 0.0) dw_last_ok = dw_shift;
            for (int r = 0; r < me; ++r) eqres[r] = ipm_eqr(PD, res_of(it.E), r);
            build_rhs(rhs_full.data(), eqres.data());
            std::copy(rhs_full.begin(), rhs_full.begin() + NN, rhs_keep.begin());
            const auto ts0 = Clock::now();
            // a backend that refines on its own (the device: residuals and corrections never leave HBM) ...
            double rel_dev = 0.0;
            int ns_dev = 0, rev_dev = 0;
            const int rr = kkt->solve_refined(rhs_full.data(), dc, 8, &rel_dev, &ns_dev, &rev_dev);
            if (rr == 0 || rr == 2) {
                R.t_solve += secs_since(ts0);
                R.n_solve += ns_dev;
                if (rr == 2 || !all_finite(rhs_full.data(), NN)) { raise_dc(dc); continue; }
                const BackendShift sh = backend_shift(dc);
                R.n_refine_reverted += rev_dev;
                step_used_with(sh, rel_dev);
            } else {
                if (rr < 0) { R.msg = "KKT solve failed: " + kkt->last_error(); return Next::abort; }
                // ... otherwise: solve, then refine against the host's own matrix-vector product
                const int sst = kkt->solve(rhs_full.data(), 1);
                R.t_solve += secs_since(ts0);
                ++R.n_solve;
                if (sst != 0) { R.msg = "KKT solve failed: " + kkt->last_error(); return Next::abort; }
                if (!all_finite(rhs_full.data(), NN)) { raise_dc(dc); continue; }
                refine_on_host(dc);
            }
            if (exact_step) dw = dw_shift;     // the log shows delta_w of an exact step, else the largest reflected shift
            factored = true;
            break;
        }
        if (!factored) { R.msg = "KKT matrix could not be factorised (still singular after dual regularisation)"; return Next::finish; }
        dw_used = dw;
        last_step_reflected = !exact_step;
        if (exact_step && dw_shift == 0.0) search_on = false;      // the plain Newton matrix is fine again
        return Next::go;
    }

    // step expansion and lengths, merit slope and penalty weight, backtracking with the two rescues of its first trial, take_step
    Next line_search() {
        // the step in the eliminated quantities
        set_step_from(rhs_full);
        // l1 merit: directional derivative of the barrier function and the penalty weight
        double dphi = 0, mmax = 0;
        MeritRef ref;
        ipm_dphi_mmax(PD, here(), duals(), it.gradf.data(), step_view(), rs.data(), mu, rho, &dphi, &mmax);
        const double phi0_base = barrier_merit(here(), it.E, 0.0, &ref.infeas0);
        // penalty weight of the l1 merit function: what the current multipliers and the descent condition ask for.  It may come down again
        // (at most halving per iteration): the multipliers of the first, far-from-feasible iterations are orders of magnitude above those near
        // the solution, and a weight frozen at that level rejects every step whose constraint curvature shows at all.
        double nu_want = std::max(1.0, std::min(1.1 * mmax, 1e8));
        if (ref.infeas0 > 0) nu_want = std::max(nu_want, dphi / (0.9 * ref.infeas0) + 1.0);
        nu = std::max(nu_want, 0.5 * nu);
        ref.phi0 = phi0_base + nu * ref.infeas0;
        ref.slope = dphi - nu * ref.infeas0;
        // backtracking
        double alpha = step.apr;
        bool accepted = false, newton_accepted = false;
        for (int ls = 0; ls < 40; ++ls) {
            if (!evaluate_trial(alpha)) return Next::abort;
            if (armijo(barrier_merit(trial(), Et, nu, nullptr), alpha, ref)) { accepted = true; break; }
            if (ls == 0) {
                if (opt.second_order_correction) {
                    const Tried soc = second_order_correction(ref, &alpha);
                    if (soc == Tried::failed) return Next::abort;
                    if (soc == Tried::taken) { accepted = true; break; }
                }
                // Close to a solution the merit function stops resolving progress: the full Newton step changes it by less than constraint
                // curvature and round-off move it, and the backtracking then crawls with steps of 1e-6 for a hundred iterations.  There -- and
                // wherever the line search has just cut three steps in a row below 30 % of the longest admissible step (`crawl`: the same effect
                // further out, with a penalty weight the far-from-feasible start left behind; crawl_limit = 1000 switches the rule off) -- the
                // KKT residual itself is the better judge.
                if (err0 <= 1e-2 || crawl >= opt.crawl_limit) {
                    const Tried full = residual_based_acceptance();
                    if (full == Tried::failed) return Next::abort;
                    if (full == Tried::taken) { newton_accepted = true; break; }
                }
            }
            alpha *= 0.5;
        }
        if (opt.print_level >= 6)
            printf("          apr %.3e  alpha %.3e  adu %.3e  dphi %.3e  infeas1 %.3e  slope %.3e\n", step.apr, alpha, step.adu, dphi, ref.infeas0, ref.slope);
        if (newton_accepted) { crawl = 0; force_modified = false; return Next::go; }       // the iterate is already updated and re-evaluated
        if (!accepted && exact_step && n_mods > 0 && !force_modified) {
            // the exact Newton direction is not a descent direction the merit function accepts at this point:
            // redo the iteration with the step of the convexified matrix (a descent direction by construction)
            force_modified = true;
            return Next::go;
        }
        force_modified = false;
        if (!accepted) {
            R.msg = "line search failed";
            // IPOPT's rule for a search that can go no further: the point is a solution only if it meets the acceptable level (the same
            // acceptable_factor as the iteration-count rule); otherwise the failure is reported, with kkt_error / constr_viol for the caller to judge
            if (acceptable()) { R.ok = true; R.msg = "converged to acceptable level (line search at round-off)"; }
            return Next::finish;
        }
        // accept
        crawl = alpha < opt.crawl_frac * step.apr ? crawl + 1 : 0;
        if (!take_step(alpha, step.adu)) return Next::abort;
        return Next::go;
    }

    NlpResult finish() {
        R.cost = it.E.cost;
        R.rho = rho;
        R.t_total = secs_since(tstart);
        if (opt.print_level >= 5)
            printf("time: total %.2f s = evaluator %.2f + KKT factor %.2f (%d factorisations) + KKT solves %.2f (%d calls) + low-rank/refinement (host) %.2f + rest"
                   " (of the host part: J^T lambda %.2f, refinement matvecs %.2f, node blocks %.2f; Hessian calls %.2f)\n",
                   R.t_total, R.t_eval, R.t_factor, R.n_factor, R.t_solve, R.n_solve, R.t_lowrank, R.t_jt, R.t_matvec, R.t_blocks, R.t_hess);
        R.z = it.z;
        R.lamF.assign(it.lam.begin(), it.lam.begin() + md);
        R.lamL.assign(it.lam.begin() + md, it.lam.end());
        R.lamC.resize(mc);
        for (int r = 0; r < mc; ++r) R.lamC[r] = sig[r / M] * it.y[r];
        return std::move(R);
    }

 private:
    enum class Tried { rejected, taken, failed };       // of a trial the line search makes: failed = the evaluator did (R.msg set)
    struct MeritRef { double phi0 = 0, slope = 0, infeas0 = 0; };    // merit, its slope and the infeasibility at the current point
    struct BackendShift { bool shifted; double dc, dw; };           // what the backend factorised beyond the nominal matrix

    // ---- views, built where they are used -----------------------------------------------------------------------------------
    IpmPoint here() const { return IpmPoint{it.z.data(), it.s.data(), it.e1.data(), it.e2.data()}; }
    IpmPoint trial() const { return IpmPoint{zt.data(), st.data(), e1t.data(), e2t.data()}; }
    IpmDuals duals() const { return IpmDuals{it.lam.data(), it.y.data(), it.zL.data(), it.zU.data(), it.vL.data(), it.vU.data(), it.w1.data(), it.w2.data()}; }
    static IpmRes res_of(const Eval& e) { return IpmRes{e.RES.data(), e.LNK.data()}; }
    IpmElim elim() { return IpmElim{sig_s.data(), rhat_s.data(), sig_t.data(), step.r_t.data()}; }
    IpmStep step_view() {
        return IpmStep{step.dz.data(), step.dlam.data(), step.ds.data(), step.dy.data(), step.de1.data(), step.de2.data(), step.dzL.data(),
                       step.dzU.data(), step.dvL.data(), step.dvU.data(), step.dw1.data(), step.dw2.data()};
    }

    void evaluator_failed() { R.msg = "evaluator failed: " + P.ev->last_error(); }
    bool evaluate(const std::vector<double>& z, Eval& e, bool jac) {
        ++R.evaluations;
        const auto te = Clock::now();
        const int est = P.ev->eval(z.data(), z.data() + (size_t)ns * M, e.RES.data(), jac ? e.VALS.data() : nullptr, &e.cost, jac);
        R.t_eval += secs_since(te);
        if (est != 0) return false;
        e.LNK.resize(ml);
        for (int l = 0; l < nl; ++l) {
            const NlpLink& L = P.links[l];
            const double* src = &z[(size_t)L.src * M];
            for (int k = 0; k < M; ++k) {
                const double* Wk = &L.W[(size_t)k * M];
                double acc = 0;
                for (int j = 0; j < M; ++j) acc += Wk[j] * src[j];
                e.LNK[(size_t)l * M + k] = z[(size_t)L.dst * M + k] - acc;
            }
        }
        for (int j = 0; j < np; ++j) {
            if (sig[j] == 1.0) continue;
            for (int k = 0; k < M; ++k) {
                e.RES[(size_t)(ns + j) * M + k] *= sig[j];
                if (jac) {
                    e.VALS[(size_t)(ns * nv + 2 * j) * M + k] *= sig[j];
                    e.VALS[(size_t)(ns * nv + 2 * j + 1) * M + k] *= sig[j];
                }
            }
        }
        return true;
    }
    // cost gradient and J^T (lam, y) at the iterate
    void grad_and_jt() {
        const auto tj = Clock::now();
        const double* V = it.E.VALS.data();
        std::vector<double>&gradf = it.gradf, &jtl = it.jtl;
        for (int v = 0; v < nv; ++v)
            for (int k = 0; k < M; ++k) gradf[v * M + k] = V[(size_t)(ns * nv + npart + v) * M + k];
        std::fill(jtl.begin(), jtl.end(), 0.0);
        // J_d^T lam: off-diagonal D part, then the node blocks (which hold D_kk)
        for (int i = 0; i < ns; ++i)
            for (int k = 0; k < M; ++k) {
                const double l = it.lam[i * M + k];
                if (l == 0.0) continue;
                const double* Dk = &P.D[(size_t)k * M];
                double* col = &jtl[(size_t)i * M];
                for (int j = 0; j < M; ++j) col[j] += Dk[j] * l;
                col[k] -= Dk[k] * l;
                for (int v = 0; v < nv; ++v) jtl[v * M + k] += V[(size_t)(i * nv + v) * M + k] * l;
            }
        for (int j = 0; j < np; ++j)
            for (int k = 0; k < M; ++k) {
                const double yy = it.y[j * M + k];
                for (const auto& ve : rv[j]) jtl[ve.first * M + k] += V[(size_t)ve.second * M + k] * yy;
            }
        for (int l = 0; l < nl; ++l) {          // coupling rows: + nu on the coupled variable, - W^T nu on its source
            const NlpLink& L = P.links[l];
            double* col = &jtl[(size_t)L.src * M];
            for (int k = 0; k < M; ++k) {
                const double nu_k = it.lam[md + l * M + k];
                if (nu_k == 0.0) continue;
                jtl[(size_t)L.dst * M + k] += nu_k;
                const double* Wk = &L.W[(size_t)k * M];
                for (int j = 0; j < M; ++j) col[j] -= Wk[j] * nu_k;
            }
        }
        R.t_jt += secs_since(tj);
    }
    double kkt_error(double mu_t, double* viol_out, double* emax_out) const {
        return ipm_kkt_error(PD, here(), duals(), it.gradf.data(), it.jtl.data(), res_of(it.E), mu_t, rho, viol_out, emax_out);
    }
    double barrier_merit(const IpmPoint& x, const Eval& e, double nu_t, double* infeas) const {
        return ipm_barrier_merit(PD, x, res_of(e), e.cost, rs.data(), mu, nu_t, rho, infeas);
    }
    bool acceptable() const { return err0 <= opt.acceptable_factor * opt.tol && (mc == 0 || emax <= 1e-6); }

    void reset_elastic_duals() {
        for (int r = 0; r < mc; ++r) { it.w1[r] = std::max(1e-8, rho - it.y[r]); it.w2[r] = std::max(1e-8, rho + it.y[r]); }
    }
    void escalate_penalty() { rho *= 10.0; mu = std::max(mu, 1e-2); reset_elastic_duals(); }
    // Raising the penalty weight is the answer to a relaxed path row only while it helps: beyond 1e5, `max_futile_escalations` tenfold raises in
    // a row that have not halved the largest elastic variable end the solve (a keep-out that cannot be cleared from this side)
    bool futile_escalation(double emax_now) {
        if (rho < 1e5) return false;         // weights a multiplier of a scaled row can plausibly need: keep raising
        if (emax_now < 0.5 * emax_ref) { emax_ref = emax_now; futile = 0; return false; }
        return ++futile >= opt.max_futile_escalations;
    }

    // ---- pieces of the Newton system -----------------------------------------------------------------------------------------
    void raise_dc(double& dc) const { dc = dc == 0.0 ? 1e-8 * std::pow(mu, 0.25) : dc * 100.0; }
    // r_t of the eliminated path rows for given row residuals  c - s - e1 + e2
    void fill_rt(const std::vector<double>& rowres) { ipm_fill_rt(PD, here(), duals(), rowres.data(), mu, rho, elim()); }
    // right-hand side of the reduced KKT system in full indexing (fixed variables: 0), for equality residuals eqr
    void build_rhs(double* out, const double* eqr) {
        ipm_build_rhs(PD, here(), it.gradf.data(), it.jtl.data(), it.E.VALS.data(), elim(), eqr, mu, out);
    }
    // One factorisation attempt.  The backend's factorisation (the device: Cholesky of a Schur complement) reports no inertia,
    // so the matrix handed to it has its inertia by construction: every node block  Q_k = H_k + Sigma_k + sum_j sig_t g_j g_j^T
    // is made positive definite (negative eigenvalues reflected, Q~_k = Q_k + sum delta v v^T), which makes K~ quasi-definite:
    // exactly nz positive and md negative eigenvalues.  With U = [v; 0] (r columns, one per modified eigenpair) the true matrix is
    // K = K~ - U Delta U^T and  inertia(K) = (nz - r, md, 0) + inertia(C),  C = Delta^-1 - U^T K~^-1 U  (r x r; both Schur
    // complements of [[K~, U], [U^T, Delta^-1]]).  So r extra solves with the same factors decide EXACTLY whether the unmodified
    // K has the right inertia (lowrank_verdict); if it has, the Woodbury identity turns the solve with K~ into the exact Newton
    // step (quadratic convergence is kept); if not, the step of K~ is the inertia-corrected one.  Y = K~^-1 U and the factor of
    // C live with the backend (KktBackend::lowrank): on the device for eMI355X.
    // Returns KktBackend::factor's codes; *dw = the largest reflected eigenvalue shift.
    int factor_node_blocks(double dc, double dw_shift, double* dw) {
        const double* V = it.E.VALS.data();
        const auto tb0 = Clock::now();
        ipm_barrier_diagonal(PD, here(), duals(), Sigma.data());     // (0 where fixed)
        int info = KktBackend::NOT_OFFERED;
        if (backend_blocks) {       // assembly, convexification and factorisation by the backend, from the terms
            Qexact.resize(Qblk.size());
            KktBackend::BlockResult br;
            br.Qexact = Qexact.data(); br.Q = Qblk.data(); br.max_mods = max_lowrank;
            br.node = &lr_node; br.delta = &lr_delta; br.vec = &lr_vec;
            info = kkt->factor_terms({H.data(), V, Sigma.data(), sig_t.data(), fixed_mask.data(), dw_shift, &rv}, dc, &br);
            if (info == KktBackend::NOT_OFFERED) {
                backend_blocks = false;
            } else {
                n_mods = br.count;
                ++R.n_factor_terms;
                *dw = br.worst;
                R.t_blocks += br.t_blocks;
                R.t_factor += br.t_factor;
            }
        }
        if (!backend_blocks) {
            assemble_node_blocks(H.data(), V, Sigma.data(), sig_t.data(), fixed_mask.data(), dw_shift, rv, nv, M, Qblk.data());
            Qexact = Qblk;
            *dw = convexify_node_blocks(Qblk.data(), fixed_mask.data(), nv, M, &mods);
            n_mods = (int)mods.size();
            R.t_blocks += secs_since(tb0);
            const auto tf0 = Clock::now();
            info = kkt->factor(Qblk.data(), V, fixed_mask.data(), dc);
            R.t_factor += secs_since(tf0);
        }
        ++R.n_factor;
        return info;
    }
    // the low-rank correction (kept by the backend, next to its factors) and the inertia verdict: sets exact_step
    bool lowrank_verdict() {
        r_mod = n_mods <= max_lowrank ? n_mods : 0;
        lr_node.resize(r_mod);
        lr_delta.resize(r_mod);
        lr_vec.resize((size_t)r_mod * nv);
        for (int c = 0; c < r_mod && !backend_blocks; ++c) {        // (the backend filled the three itself)
            lr_node[c] = mods[c].node;
            lr_delta[c] = mods[c].delta;
            for (int v = 0; v < nv; ++v) lr_vec[(size_t)c * nv + v] = mods[c].v[v];
        }
        const auto tl0 = Clock::now();
        bool lr_exact = false;
        if (force_modified) r_mod = 0;      // the exact step failed the line search here: take the convexified one
        if (kkt->lowrank(r_mod, lr_node.data(), lr_vec.data(), lr_delta.data(), &lr_exact) != 0) {
            R.msg = "KKT low-rank correction failed: " + kkt->last_error();
            return false;
        }
        R.t_lowrank += secs_since(tl0);
        exact_step = !force_modified && lr_exact && r_mod == n_mods;
        return true;
    }
    // The backend may have factorised a MORE regularised matrix than it was given (applied_regularisation: the Schur path's ladder):
    // counted, and reported with the residual the step is finally used with (an inexact Newton step: the line search still decides)
    BackendShift backend_shift(double dc) {
        BackendShift sh{false, dc, 0.0};
        kkt->applied_regularisation(&sh.dc, &sh.dw);
        sh.shifted = sh.dw > 0.0 || sh.dc > std::max(dc, 1e-9) * 1.0001;
        if (sh.shifted) ++R.n_backend_shifted;
        return sh;
    }
    void step_used_with(const BackendShift& sh, double rel) {
        R.worst_step_residual = std::max(R.worst_step_residual, rel);
        if (opt.print_level >= 5 && sh.shifted && rel > 1e-6)
            printf("          backend factorised with dc %.1e dw %.1e; step used with relative residual %.2e\n", sh.dc, sh.dw, rel);
    }
    // y = [[Q, J^T], [J, -dc I]] x  with the node blocks Qb (fixed variables: identity rows/columns)
    void kkt_matvec(const double* Qb, const double* x, double* y, double dcv) {
        const double* V = it.E.VALS.data();
        const unsigned char* fixed = fixed_mask.data();
        std::fill(y, y + NN, 0.0);
        for (int k = 0; k < M; ++k)
            for (int v = 0; v < nv; ++v) {
                if (fixed[v * M + k]) continue;
                double acc = 0;
                for (int q = 0; q < nv; ++q) {
                    if (fixed[q * M + k]) continue;
                    const int hi = std::max(v, q), lo = std::min(v, q);
                    acc += Qb[(size_t)(hi * (hi + 1) / 2 + lo) * M + k] * x[q * M + k];
                }
                y[v * M + k] = acc;
            }
        // D part: plain dot / axpy over whole rows of D (vectorisable), with x of fixed variables taken as 0
        // and the node-diagonal term (which lives in the node blocks V) taken out again
        xfree.assign(x, x + nz);
        for (int q = 0; q < nz; ++q)
            if (fixed[q]) xfree[q] = 0.0;
        for (int i = 0; i < ns; ++i) {
            const double* xi = &xfree[(size_t)i * M];
            double* yi = &y[(size_t)i * M];
            for (int k = 0; k < M; ++k) {
                const int Rr = nz + i * M + k;
                const double* Dk = &P.D[(size_t)k * M];
                const double xr = x[Rr];
                double acc = 0;
#pragma omp simd reduction(+ : acc)
                for (int j = 0; j < M; ++j) acc += Dk[j] * xi[j];
#pragma omp simd
                for (int j = 0; j < M; ++j) yi[j] += Dk[j] * xr;
                acc -= Dk[k] * xi[k];
                yi[k] -= Dk[k] * xr;
                for (int v = 0; v < nv; ++v) {
                    if (fixed[v * M + k]) continue;
                    const double jv = V[(size_t)(i * nv + v) * M + k];
                    acc += jv * x[v * M + k];
                    y[v * M + k] += jv * xr;
                }
                y[Rr] = acc - dcv * xr;
            }
        }
        for (int l = 0; l < nl; ++l) {          // coupling rows
            const NlpLink& L = P.links[l];
            const double* xs = &xfree[(size_t)L.src * M];
            double* ys = &y[(size_t)L.src * M];
            for (int k = 0; k < M; ++k) {
                const int Rr = nz + md + l * M + k;
                const double* Wk = &L.W[(size_t)k * M];
                const double xr = x[Rr];
                double acc = xfree[(size_t)L.dst * M + k];
                // (the fused operation, spelt out: vectorised in order, the compiler would round the product first)
                for (int j = 0; j < M; ++j) acc = std::fma(-Wk[j], xs[j], acc);
                for (int j = 0; j < M; ++j) ys[j] -= Wk[j] * xr;
                y[(size_t)L.dst * M + k] += xr;
                y[Rr] = acc - dcv * xr;
            }
        }
        for (int q = 0; q < nz; ++q)
            if (fixed[q]) y[q] = x[q];
    }
    // The host twin of KktBackend::solve_refined, around solve(): iterative refinement of rhs_full against the matrix the step
    // belongs to (K if exact, K~ otherwise): the factorisation of a 1000-node KKT matrix leaves residuals that would stall the Newton
    // iteration some orders above the requested tolerance.  Where the backend regularised beyond the nominal matrix this is a
    // stationary iteration with (K + E)^-1 that need not contract, so a correction that makes the residual worse is taken back.
    void refine_on_host(double dc) {
        const std::vector<double>& Qm = exact_step ? Qexact : Qblk;
        const BackendShift sh = backend_shift(dc);
        double bmax = 0;
        for (size_t r = 0; r < NN; ++r) bmax = std::max(bmax, std::fabs(rhs_keep[r]));
        double prev = 1e300, rlast = 0.0;
        bool have_prev = false;
        for (int ir = 0; ir < 8; ++ir) {      // (8 since the backend may have regularised the factorised matrix: linear convergence)
            { const auto tm = Clock::now(); kkt_matvec(Qm.data(), rhs_full.data(), resid.data(), dc); R.t_matvec += secs_since(tm); }
            double rmax = 0;
            for (size_t r = 0; r < NN; ++r) { resid[r] = rhs_keep[r] - resid[r]; rmax = std::max(rmax, std::fabs(resid[r])); }
            if (have_prev && !(rmax < prev)) {          // the last correction did harm: undo it and stop
                for (size_t r = 0; r < NN; ++r) rhs_full[r] = x_prev[r];
                ++R.n_refine_reverted;
                rlast = prev;
                break;
            }
            rlast = rmax;
            if (!(rmax > 1e-14 * std::max(1.0, bmax)) || !(rmax < 0.5 * prev)) break;
            prev = rmax;
            { const auto ts = Clock::now(); const int rc = kkt->solve(resid.data(), 1); R.t_solve += secs_since(ts); ++R.n_solve; if (rc != 0) break; }
            if (!all_finite(resid.data(), NN)) break;
            x_prev.assign(rhs_full.begin(), rhs_full.begin() + NN);
            have_prev = true;
            for (size_t r = 0; r < NN; ++r) rhs_full[r] += resid[r];
        }
        step_used_with(sh, rlast / std::max(1.0, bmax));
    }

    // ---- pieces of the line search -------------------------------------------------------------------------------------------
    // the whole step from a solution of the reduced system: everything that was eliminated (uses r_t), and its lengths
    void set_step_from(const std::vector<double>& sol) {
        for (int q = 0; q < nz; ++q) step.dz[q] = fixed_mask[q] ? 0.0 : sol[q];
        for (int r = 0; r < me; ++r) step.dlam[r] = sol[nz + r];
        ipm_expand_step(PD, here(), duals(), it.E.VALS.data(), elim(), mu, rho, step_view());
        ipm_step_lengths(PD, here(), duals(), step_view(), tau, &step.apr, &step.adu);      // fraction to the boundary
    }
    // the primal trial point for step length a
    void form_trial(double a) {
        for (int q = 0; q < nz; ++q) zt[q] = it.z[q] + a * step.dz[q];
        for (int r = 0; r < mc; ++r) {
            st[r] = it.s[r] + a * step.ds[r];
            e1t[r] = it.e1[r] + a * step.de1[r];
            e2t[r] = it.e2[r] + a * step.de2[r];
        }
    }
    // ... evaluated without derivatives, and with the slack reset: a row's slack may jump to the value that closes its residual whenever
    // that lowers the merit function (the keep-out rows are strongly curved: a step along one otherwise shows as a residual c - s)
    bool evaluate_trial(double a) {
        form_trial(a);
        if (!evaluate(zt, Et, false)) return evaluator_failed(), false;
        ipm_slack_reset(PD, Et.RES.data() + md, e1t.data(), e2t.data(), mu, nu, st.data());
        return true;
    }
    static bool armijo(double phi, double a, const MeritRef& m) {
        return std::isfinite(phi) && phi <= m.phi0 + 1e-4 * a * std::min(m.slope, 0.0) + 1e-13 * std::fabs(m.phi0);
    }
    // the iterate after a step of length a_pr (primal: zt, st, e1t, e2t hold the trial point) / a_du (bound
    // multipliers), re-evaluated with derivatives
    bool take_step(double a_pr, double a_du) {
        it.z = zt;
        it.s = st;
        it.e1 = e1t;
        it.e2 = e2t;
        ipm_update_duals(PD, here(),
                         IpmDualsRW{it.lam.data(), it.y.data(), it.zL.data(), it.zU.data(), it.vL.data(), it.vU.data(), it.w1.data(), it.w2.data()},
                         step_view(), a_pr, a_du, mu);
        if (!evaluate(it.z, it.E, true)) return evaluator_failed(), false;
        grad_and_jt();
        return true;
    }
    // Second-order correction (as in IPOPT's line search): the first trial point (length *alpha, in zt .. Et) was rejected and is less
    // feasible than the current one -- the curvature of the constraints, not the direction, is to blame (Maratos effect; without this
    // the l1 merit function lets the iteration crawl along the strongly curved defect / keep-out rows with steps of 2^-8).  Re-solve
    // with the SAME factorisation for the constraint values seen at the trial point.  Taken: the corrected step is in `step`, its
    // trial point in zt .. Et and its length in *alpha; rejected: `step` is what it was.
    Tried second_order_correction(const MeritRef& ref, double* alpha) {
        double infeas_t = 0;
        barrier_merit(trial(), Et, 0.0, &infeas_t);
        if (!(std::isfinite(infeas_t) && infeas_t >= ref.infeas0)) return Tried::rejected;
        const Step keep = step;
        // the residuals to correct for: a * (those of the step before) + those at its trial point, from the current point's on
        for (int r = 0; r < me; ++r) soc_def[r] = ipm_eqr(PD, res_of(it.E), r);
        for (int r = 0; r < mc; ++r) soc_row[r] = ipm_row_res(PD, res_of(it.E), it.s.data(), it.e1.data(), it.e2.data(), r);
        double a = *alpha, infeas_old = infeas_t;
        for (int pc = 0; pc < 4; ++pc) {
            for (int r = 0; r < me; ++r) soc_def[r] *= a;       // (scaled, then added to: the product is rounded, not fused into the sum)
            for (int r = 0; r < me; ++r) soc_def[r] += ipm_eqr(PD, res_of(Et), r);
            for (int r = 0; r < mc; ++r) soc_row[r] = a * soc_row[r] + ipm_row_res(PD, res_of(Et), st.data(), e1t.data(), e2t.data(), r);
            fill_rt(soc_row);
            build_rhs(soc_rhs.data(), soc_def.data());
            if (kkt->solve(soc_rhs.data(), 1) != 0) break;
            if (!all_finite(soc_rhs.data(), NN)) break;
            set_step_from(soc_rhs);
            const double asoc = step.apr;
            if (!evaluate_trial(asoc)) return Tried::failed;
            double infeas_s = 0;
            if (armijo(barrier_merit(trial(), Et, nu, &infeas_s), asoc, ref)) {
                *alpha = asoc;
                ++R.soc_steps;
                return Tried::taken;
            }
            if (!std::isfinite(infeas_s) || infeas_s > 0.99 * infeas_old) break;
            infeas_old = infeas_s;
            a = asoc;
        }
        step = keep;
        return Tried::rejected;
    }
    // Residual-based acceptance: take the full step if it reduces the KKT residual of the current barrier problem, else take
    // the iterate back as it was (and backtrack)
    Tried residual_based_acceptance() {
        const double err_mu = kkt_error(mu, nullptr, nullptr);
        it_keep = it;
        form_trial(step.apr);
        if (!take_step(step.apr, step.adu)) return Tried::failed;
        const double err_tr = kkt_error(mu, nullptr, nullptr);
        if (std::isfinite(err_tr) && err_tr <= 0.9 * err_mu) {
            ++R.newton_steps;
            return Tried::taken;
        }
        it = it_keep;
        ++R.restored_steps;
        return Tried::rejected;
    }

    // ---- the problem ---------------------------------------------------------------------------------------------------------
    const NlpProblem& P;
    const NlpOptions& opt;
    const RowVars rv;                   // (variable, VALS entry) pairs of every path row
    const int ns, np, M, nv, nz, md, mc;
    const int nl, ml, me;               // coupling rows behind the defects: me equality multipliers
    const int npart;
    const size_t NN;                    // unknowns of the reduced system
    const Clock::time_point tstart = Clock::now();
    std::vector<double> sig, cls, cus;  // row scales; scaled row bounds
    IpmDims PD;                         // the same problem as the ipm_* functions take it
    const IpmB B{PD};
    std::vector<unsigned char> fixed_mask;
    std::vector<double> rs;             // row weights of the merit function
    // ---- the iterate and the scalars of the barrier / penalty / inertia-search / stagnation / crawl rules -----------------------
    Point it, it_keep;
    Eval Et;                            // trial point: values ...
    std::vector<double> zt, st, e1t, e2t;   // ... and primal variables
    double mu = 0, nu = 1.0, rho = 0;
    double err0 = 0, emax = 0, tau = 0;     // of this iteration: KKT error at mu = 0, largest elastic, fraction to the boundary
    double dw_used = 0.0;               // delta_w of the last exact step, or the largest reflected eigenvalue shift (log only)
    double dw_last_ok = 0.0;            // last nonzero delta_w that gave the right inertia
    int n_acceptable = 0, futile = 0, stagn = 0, crawl = 0;
    bool force_modified = false, search_on = false, last_step_reflected = false, mu_restarted = false;
    double emax_ref = 1e300, stagn_ref = 1e300;
    // ---- Newton-step linear algebra: the caller's backend (eMI355X: the device) or the dense host one -----------------------------
    DenseHostKkt host_kkt;
    KktBackend* const kkt;
    bool backend_blocks;                // until the backend says NOT_OFFERED
    static constexpr int max_lowrank = 4096;        // more modified eigenpairs than this: take the modified step untested
    std::vector<double> H, Qblk, Qexact, Sigma, y_unscaled;
    std::vector<double> sig_t, sig_s, rhat_s;       // row elimination (r_t: with the step)
    std::vector<BlockMod> mods;
    int n_mods = 0;                     // modified eigenpairs of the last factorisation (the true number, also beyond max_lowrank)
    int r_mod = 0;                      // ... of which the low-rank correction holds
    bool exact_step = false;
    std::vector<int> lr_node;
    std::vector<double> lr_vec, lr_delta;
    std::vector<double> rhs_full, rhs_keep, eqres, resid, x_prev, xfree;
    // ---- the step, and the right-hand sides of its second-order correction -------------------------------------------------------
    Step step;
    std::vector<double> soc_def, soc_row, soc_rhs;
    NlpResult R;
};

// Iterate on the scaled variables (ScaledEvaluator above), answer in the caller's
NlpResult solve_scaled(const NlpProblem& P, const NlpOptions& opt, const std::vector<double>& z0, const RowVars& rv, int npart) {
    NlpResult R;
    const int ns = P.ns, M = P.M, nv = ns + P.nc, nz = nv * M, md = ns * M;
    if ((int)P.vscale.size() != nv || (int)z0.size() != nz || (int)P.zl.size() != nz || (int)P.zu.size() != nz || !P.ev) {
        R.msg = "solve_nlp: inconsistent problem sizes (vscale)";
        return R;
    }
    for (double sv : P.vscale)
        if (!(sv > 0) || !std::isfinite(sv)) { R.msg = "solve_nlp: vscale must be positive"; return R; }
    for (const NlpLink& L : P.links)        // (d - W z) / s keeps W only if both ends carry the same scale
        if (P.vscale[L.dst] != P.vscale[L.src]) { R.msg = "solve_nlp: a coupled variable must be scaled like its source"; return R; }
    NlpProblem Q = P;
    Q.vscale.clear();
    Q.row_vars = rv;
    ScaledEvaluator sev(P, rv, npart);
    Q.ev = &sev;
    std::vector<double> zs(z0);
    for (int v = 0; v < nv; ++v)
        for (int k = 0; k < M; ++k) {
            const size_t q = (size_t)v * M + k;
            const double inv = 1.0 / P.vscale[v];
            zs[q] *= inv;
            if (Q.zl[q] > -INF_BOUND) Q.zl[q] *= inv;
            if (Q.zu[q] < INF_BOUND) Q.zu[q] *= inv;
            if (P.zl[q] == P.zu[q]) Q.zu[q] = Q.zl[q];
        }
    if ((int)Q.lamF0.size() == md)
        for (int i = 0; i < ns; ++i)
            for (int k = 0; k < M; ++k) Q.lamF0[(size_t)i * M + k] *= P.vscale[i];
    NlpResult S = solve_nlp(Q, opt, zs);
    for (int v = 0; v < nv && (int)S.z.size() == nz; ++v)
        for (int k = 0; k < M; ++k) S.z[(size_t)v * M + k] *= P.vscale[v];
    for (int i = 0; i < ns && (int)S.lamF.size() == md; ++i)
        for (int k = 0; k < M; ++k) S.lamF[(size_t)i * M + k] /= P.vscale[i];
    for (size_t l = 0; l < P.links.size() && S.lamL.size() == P.links.size() * M; ++l)      // row (d - W z) / s: multiplier / s
        for (int k = 0; k < M; ++k) S.lamL[l * M + k] /= P.vscale[P.links[l].dst];
    return S;
}

}  // namespace

NlpResult solve_nlp(const NlpProblem& P, const NlpOptions& opt, const std::vector<double>& z0) {
    NlpResult R;
    const int ns = P.ns, np = P.np, M = P.M, nv = ns + P.nc, nz = nv * M;
    for (const NlpLink& L : P.links)
        if (L.dst < 0 || L.dst >= nv || L.src < 0 || L.src >= nv || L.dst == L.src || (int)L.W.size() != M * M) {
            R.msg = "solve_nlp: a coupling row names variables outside the problem or has no M x M operator";
            return R;
        }
    if (!P.links.empty() && P.kkt) { R.msg = "solve_nlp: coupling rows (delayed values) are solved with the dense host backend only"; return R; }
    // (variable, VALS entry) pairs of every path row
    RowVars rv = P.row_vars;
    if (rv.empty())
        for (int j = 0; j < np; ++j) rv.push_back({{P.px, ns * nv + 2 * j}, {P.py, ns * nv + 2 * j + 1}});
    if ((int)rv.size() != np) { R.msg = "solve_nlp: row_vars has the wrong length"; return R; }
    int npart = 0;
    for (const auto& r : rv) npart += (int)r.size();
    if (!P.vscale.empty()) return solve_scaled(P, opt, z0, rv, npart);
    if (!P.ev || (int)P.zl.size() != nz || (int)P.zu.size() != nz || (int)P.D.size() != M * M ||
        (int)P.cl.size() != np || (int)P.cu.size() != np || (int)z0.size() != nz) {
        R.msg = "solve_nlp: inconsistent problem sizes";
        return R;
    }
    if (!P.cscale.empty() && (int)P.cscale.size() != np) { R.msg = "solve_nlp: cscale has the wrong length"; return R; }
    for (int j = 0; j < np; ++j)
        if (!(P.cl[j] > -INF_BOUND) && !(P.cu[j] < INF_BOUND)) { R.msg = "solve_nlp: path row without any bound"; return R; }
    IpmSolve S(P, opt, std::move(rv), npart);
    if (!S.start(z0)) return S.result();
    for (int iter = 0;; ++iter) {
        IpmSolve::Next next = S.test_and_update_barrier(iter);
        if (next == IpmSolve::Next::go) next = S.newton_system();
        if (next == IpmSolve::Next::go) next = S.line_search();
        if (next == IpmSolve::Next::abort) return S.result();
        if (next == IpmSolve::Next::finish) break;
    }
    return S.finish();
}

}  // namespace mi355x
}  // namespace ETOL
