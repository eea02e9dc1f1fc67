"""Generates tests/golden/prolong_matrices.npz: the fixture of emi_prolong_matrix's test.

For every pair (Mc, Mf) of tests/ladder_ref.py: the LGL nodes of both meshes at 50 digits (mpmath; Newton on (1 - t^2) P'_N), the
barycentric weights of the coarse nodes as the plain products 1 / prod_{k != j} (x_j - x_k) -- no Legendre identity --, and the
Lagrange basis polynomials of the coarse nodes at the fine nodes, rounded to double: P_<Mc>_<Mf> [Mf][Mc].  A fine node that
coincides with a coarse one (both ends; the middle when both counts are odd) gives a unit row.  No GPU, no library needed:

    python tests/golden/gen_prolong_golden.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

mp.mp.dps = 50
PAIRS = ((2, 3), (5, 9), (21, 41), (33, 65), (40, 41), (129, 257))      # tests/ladder_ref.py: PAIRS
_nodes = {}


def lgl_nodes(M):
    if M in _nodes:
        return _nodes[M]
    N = M - 1
    x = [mp.mpf(-1)] + [None] * (N - 1) + [mp.mpf(1)]
    for k in range(1, N):
        g = -mp.cos(mp.pi * k / N)
        for _ in range(100):
            pn, pn1 = mp.legendre(N, g), mp.legendre(N - 1, g)
            step = (g * pn - pn1) / ((N + 1) * pn)
            g -= step
            if abs(step) < mp.mpf(10) ** (-45):
                break
        x[k] = g
    if N % 2 == 0:
        x[N // 2] = mp.mpf(0)
    for k in range(1, N):           # the node set is symmetric: make it exactly so
        if k < N - k:
            x[N - k] = -x[k]
    _nodes[M] = x
    return x


def basis(Mc, Mf):
    xc, xf = lgl_nodes(Mc), lgl_nodes(Mf)
    lam = []
    for j in range(Mc):
        p = mp.mpf(1)
        for k in range(Mc):
            if k != j:
                p *= xc[j] - xc[k]
        lam.append(1 / p)
    P = np.zeros((Mf, Mc))
    for q, t in enumerate(xf):
        hit = [j for j in range(Mc) if abs(t - xc[j]) < mp.mpf(10) ** (-40)]
        if hit:
            P[q, hit[0]] = 1.0
            continue
        terms = [lam[j] / (t - xc[j]) for j in range(Mc)]
        den = mp.fsum(terms)
        P[q] = [float(v / den) for v in terms]
    return P


def main():
    out = {}
    for mc, mf in PAIRS:
        out[f"P_{mc}_{mf}"] = basis(mc, mf)
        print(f"({mc}, {mf}): row sums within {np.abs(out[f'P_{mc}_{mf}'].sum(1) - 1).max():.2e}, Lebesgue constant "
              f"{np.abs(out[f'P_{mc}_{mf}']).sum(1).max():.3f}")
    path = os.path.join(ROOT, "tests", "golden", "prolong_matrices.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
