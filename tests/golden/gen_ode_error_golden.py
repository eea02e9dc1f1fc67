"""Generates tests/golden/ode_error_operators.npz: the fixture of emi_ode_error_operator's test.

For every M of tests/ode_error_ref.py (OPERATOR_SIZES): the LGL nodes at 50 digits (gen_prolong_golden.lgl_nodes), the barycentric
weights as the plain products 1 / prod_{k != j} (x_j - x_k) -- no Legendre identity, no square roots of quadrature weights --, the
five Gauss-Legendre points of every interval [x_k, x_k+1] from the 50-digit zeros of P_5, point p = q (M - 1) + k, and there the
Lagrange basis polynomials and their derivatives, rounded to double: E_<M>, Ed_<M> [5 (M-1)][M], tq_<M> [5 (M-1)].  No GPU, no
library needed:

    python tests/golden/gen_ode_error_golden.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from gen_prolong_golden import lgl_nodes  # noqa: E402

mp.mp.dps = 50
SIZES = (2, 3, 9, 41, 65)       # tests/ode_error_ref.py: OPERATOR_SIZES


def gauss5():
    r = mp.sqrt(mp.mpf(10) / 7)
    a, b = mp.sqrt(5 - 2 * r) / 3, mp.sqrt(5 + 2 * r) / 3
    return [-b, -a, mp.mpf(0), a, b]


def operators(M):
    x = lgl_nodes(M)
    beta = []
    for j in range(M):
        p = mp.mpf(1)
        for k in range(M):
            if k != j:
                p *= x[j] - x[k]
        beta.append(1 / p)
    g = gauss5()
    nq = M - 1
    E, Ed, tq = np.zeros((5 * nq, M)), np.zeros((5 * nq, M)), np.zeros(5 * nq)
    for q in range(5):
        for k in range(nq):
            s = x[k] + (x[k + 1] - x[k]) * (g[q] + 1) / 2
            lam = [beta[j] / (s - x[j]) for j in range(M)]
            S = mp.fsum(lam)
            T = mp.fsum(lam[j] / (s - x[j]) for j in range(M))
            p = q * nq + k
            tq[p] = float(s)
            E[p] = [float(v / S) for v in lam]
            Ed[p] = [float((lam[j] / S * T - lam[j] / (s - x[j])) / S) for j in range(M)]
    return E, Ed, tq


def main():
    out = {}
    for M in SIZES:
        E, Ed, tq = operators(M)
        out[f"E_{M}"], out[f"Ed_{M}"], out[f"tq_{M}"] = E, Ed, tq
        print(f"M {M}: row sums of E within {np.abs(E.sum(1) - 1).max():.2e}, of E' within {np.abs(Ed.sum(1)).max():.2e}, "
              f"Lebesgue constant {np.abs(E).sum(1).max():.3f}")
    path = os.path.join(ROOT, "tests", "golden", "ode_error_operators.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
