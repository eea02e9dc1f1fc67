"""numpy float64 statement of the adjoint pass of a problem WITH delays (include/emi355x.h, emi_lagr_grad_total_* /
emi_kkt_certificate_total_*), built on adjoint_ref.lagr_grad: the gradient on the extended node variables, then the adjoints
of the delayed values folded onto their sources through the interpolation operators,

    Gdel[b][q][k] = Gx[b][ns+ncf+q][k]
    G[b][v][k]    = Gx[b][v][k] + sum_{q: src(q) = v} sum_j Gdel[b][q][j] W_i(q)[j][k]            v < ns + ncf

(a row vector times W: j runs over the rows of W).  Test infrastructure: the reference the GPU tests compare the kernels with,
itself checked against central differences of the oracle's Lagrangian in tests/test_delay_adjoint_cpu.py."""
import numpy as np

import adjoint_ref as A
import oracle_lib as O


def slots(ns, ncf, xh, uh):
    """(source variable, delay index i) of every delayed slot, in the order of emi_set_delays:
    x(t - dt) of every state, .., x(t - (xh-1) dt), then u(t - dt) of every free control, .., u(t - uh dt)"""
    out = [(st, i) for i in range(1, xh) for st in range(ns)]
    out += [(ns + c, i) for i in range(1, uh + 1) for c in range(ncf)]
    return out


def copies(ns, ncf, xh, uh):
    """number of delayed copies of every free variable [ns+ncf]"""
    n = np.zeros(ns + ncf, dtype=int)
    for src, _ in slots(ns, ncf, xh, uh):
        n[src] += 1
    return n


def table_pattern(ns, nc, np_, px=0, py=1):
    """(kind, row, variable) of every VALS entry of a model whose path rows all come from the record table (the layout of
    include/emi355x.h); what adjoint_ref.entry_pattern reads from emi_jac_structure on a device"""
    nv = ns + nc
    pat = [(0, i, v) for i in range(ns) for v in range(nv)]
    for j in range(np_):
        pat += [(1, j, px), (1, j, py)]
    return pat + [(2, -1, v) for v in range(nv)]


def fold(Gx, W, ns, ncf, xh, uh, absolute=False):
    """Gx [B][ns+nc][M] on the extended variables, W [nd][M][M] with W[i-1] = W(i dt)  ->  (G [B][ns+ncf][M], Gdel [B][nd_slots][M])"""
    f = np.abs if absolute else (lambda a: a)
    Gx = np.asarray(Gx, dtype=np.float64)
    nf = ns + ncf
    G, Gdel = Gx[:, :nf].copy(), Gx[:, nf:].copy()
    for q, (src, i) in enumerate(slots(ns, ncf, xh, uh)):
        G[:, src] += f(Gdel[:, q]) @ f(np.asarray(W[i - 1]))        # sum_j Gdel[q][j] W[j][k]
    return G, Gdel


def lagr_grad_total(VALS, lamF, lamC, sigma, D, pattern, ns, nc, ncf, xh, uh, W, absolute=False):
    Gx = A.lagr_grad(VALS, lamF, lamC, sigma, D, pattern, ns, nc, absolute=absolute)
    return fold(Gx, W, ns, ncf, xh, uh, absolute=absolute)


def bound(T, Tdel, M, nv, np_, ncopies):
    """Nested dot product: an entry of Gdel is a sum of nv + np + 2 products and (state rows) M more; an entry of G adds M products
    per delayed copy, each factor carrying that error, and one more addition: 2 (M (1 + copies) + nv + np + 4) eps T elementwise,
    device and numpy together, whatever the summation order.  T / Tdel: the same sums over absolute values."""
    c = np.asarray(ncopies, dtype=np.float64).reshape(1, -1, 1)
    return 2.0 * (M * (1.0 + c) + nv + np_ + 4) * A.EPS * T, 2.0 * (M + nv + np_ + 4) * A.EPS * Tdel


def fold_weight(Gdel, W, ns, ncf, xh, uh):
    """[B][ns+ncf][M]: max(1, |W|max) sum_j |Gdel[q][j]| over the copies q of a variable -- what a relative difference between two
    statements of W costs an entry of G"""
    Gdel = np.asarray(Gdel)
    out = np.zeros((Gdel.shape[0], ns + ncf, Gdel.shape[2]))
    for q, (src, i) in enumerate(slots(ns, ncf, xh, uh)):
        out[:, src] += (max(1.0, np.abs(W[i - 1]).max()) * np.abs(Gdel[:, q]).sum(axis=1))[:, None]
    return out


def slot_weight(Gdel, W, ns, ncf, xh, uh):
    """[B][n_delayed][M]: the same figure for the slots themselves, max(1, |W_i(q)|max) sum_j |Gdel[q][j]| -- two statements of W give
    the node functions different delayed inputs, which the adjoint of a delayed value sees through their second derivatives"""
    Gdel = np.asarray(Gdel)
    out = np.zeros_like(Gdel)
    for q, (src, i) in enumerate(slots(ns, ncf, xh, uh)):
        out[:, q] = (max(1.0, np.abs(W[i - 1]).max()) * np.abs(Gdel[:, q]).sum(axis=1))[:, None]
    return out


def extended(X, U, W, ns, ncf, xh, uh):
    """[U | delayed values], the delayed values as W(i dt) . (node values)"""
    z = np.concatenate([X, U], axis=1)
    parts = [U] + [np.einsum("kj,bj->bk", W[i - 1], z[:, src])[:, None] for src, i in slots(ns, ncf, xh, uh)]
    return np.concatenate(parts, axis=1)


def oracle_delay_matrices(M, tau, t0, tf, dt, xh, uh):
    return np.array([O.delay_matrix(M, tau, t0, tf, (d + 1) * dt) for d in range(max(xh - 1, uh))])


def oracle_lagrangian(model, params, mesh, t0, tf, X, U, W, ns, ncf, xh, uh, lamF, lamC, sigma, recs=None, maximize=False):
    """[B]: sigma COST + sum lamF . defect + sum lamC . c from the CPU oracle at (X, U), the delayed values formed with W"""
    M = X.shape[-1]
    RES, _, COST = O.evaluate(model, params, M, mesh, t0, tf, X, extended(X, U, W, ns, ncf, xh, uh), recs, maximize=maximize)
    L = sigma * COST + (lamF * RES[:, :ns]).sum(axis=(1, 2))
    if RES.shape[1] > ns:
        L = L + (np.asarray(lamC) * RES[:, ns:]).sum(axis=(1, 2))
    return L


def directional_check(model, params, mesh, t0, tf, X, U, W, ns, ncf, xh, uh, lamF, lamC, sigma, G, dX, dU, recs=None, maximize=False,
                      h=1e-5):
    """(central difference of the oracle Lagrangian along (dX, dU), <G, (dX, dU)>), summed over the instances"""
    Lp = oracle_lagrangian(model, params, mesh, t0, tf, X + h * dX, U + h * dU, W, ns, ncf, xh, uh, lamF, lamC, sigma, recs, maximize)
    Lm = oracle_lagrangian(model, params, mesh, t0, tf, X - h * dX, U - h * dU, W, ns, ncf, xh, uh, lamF, lamC, sigma, recs, maximize)
    fd = float(((Lp - Lm) / (2.0 * h)).sum())
    an = float((G * np.concatenate([dX, dU], axis=1)).sum())
    return fd, an
