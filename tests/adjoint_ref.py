"""numpy float64 statement of the adjoint pass (include/emi355x.h, emi_lagr_grad_* / emi_kkt_certificate_*): the Lagrangian
gradient from VALS, the multipliers, the operator D and the library's published COO pattern (emi_jac_structure), and the six
certificate maxima.  Test infrastructure: the reference the GPU tests compare the kernels with."""
import numpy as np

EPS = np.finfo(np.float64).eps
INF_BOUND = 1e19
FIELDS = ("stat", "comp", "defect", "viol", "gmax", "lmax")


def entry_pattern(rows, cols, ns, nc, np_, M):
    """(kind, row index, variable) of every VALS entry from the COO pattern of emi_jac_structure (rows / cols have nvals * M
    entries ordered like VALS).  kind 0: defect row i, 1: path row j, 2: cost gradient.  The pattern must be node-diagonal."""
    rows = np.asarray(rows).reshape(-1, M)
    cols = np.asarray(cols).reshape(-1, M)
    k = np.arange(M)
    out = []
    for r, c in zip(rows, cols):
        v = int(c[0]) // M
        assert np.array_equal(c, v * M + k)
        if r[0] < 0:
            assert np.all(r == -1)
            out.append((2, -1, v))
        elif r[0] < ns * M:
            i = int(r[0]) // M
            assert np.array_equal(r, i * M + k)
            out.append((0, i, v))
        else:
            j = (int(r[0]) - ns * M - 2 * ns) // M
            assert 0 <= j < np_ and np.array_equal(r, ns * M + 2 * ns + j * M + k)
            out.append((1, j, v))
    assert len(out) == rows.shape[0]
    return out


def lagr_grad(VALS, lamF, lamC, sigma, D, pattern, ns, nc, absolute=False):
    """G[B][ns+nc][M]; absolute=True: the same sums over absolute values (T of the forward-error bound)."""
    VALS, lamF = np.asarray(VALS, dtype=np.float64), np.asarray(lamF, dtype=np.float64)
    f = np.abs if absolute else (lambda a: a)
    B, _, M = VALS.shape
    G = np.zeros((B, ns + nc, M))
    for e, (kind, r, v) in enumerate(pattern):
        if kind == 2:
            G[:, v] += f(sigma * VALS[:, e])
        elif kind == 0:
            G[:, v] += f(VALS[:, e]) * f(lamF[:, r])
        else:
            G[:, v] += f(VALS[:, e]) * f(np.asarray(lamC)[:, r])
    Doff = np.array(D, dtype=np.float64)
    np.fill_diagonal(Doff, 0.0)
    G[:, :ns] += (f(lamF).reshape(B * ns, M) @ f(Doff)).reshape(B, ns, M)      # sum_j D[j][k] lamF[v][j]
    return G


def bound(T, M, nv, np_):
    """dot-product forward error of G for any summation order: 2 (M + nv + np + 2) eps T, elementwise"""
    return 2.0 * (M + nv + np_ + 2) * EPS * T


def certificate(G, RES, X, U, VALS, lamF, lamC, sigma, zl, zu, cl, cu):
    """[B][6] = stat, comp, defect, viol, gmax, lmax (each a maximum over the instance); zl / zu: [1 or B][nv][M]"""
    G, RES, X, U, lamF = (np.asarray(a, dtype=np.float64) for a in (G, RES, X, U, lamF))
    B, ns, M = X.shape
    nv = G.shape[1]
    np_ = RES.shape[1] - ns
    z = np.concatenate([X, U], axis=1)
    zl = np.broadcast_to(np.asarray(zl, dtype=np.float64).reshape(-1, nv, M), (B, nv, M))
    zu = np.broadcast_to(np.asarray(zu, dtype=np.float64).reshape(-1, nv, M), (B, nv, M))
    gp, gm = np.maximum(G, 0.0), np.maximum(-G, 0.0)
    has_lo, has_up = np.abs(zl) < INF_BOUND, np.abs(zu) < INF_BOUND
    fixed = has_lo & has_up & (zl == zu)
    zero = np.zeros_like(G)
    mx = lambda a: a.reshape(B, -1).max(axis=1) if a.size else np.zeros(B)
    with np.errstate(invalid="ignore", over="ignore"):
        stat = np.maximum(np.where(~fixed & ~has_lo, gp, zero), np.where(~fixed & ~has_up, gm, zero))
        comp = np.maximum(np.where(~fixed & has_lo, gp * np.maximum(z - zl, 0.0), zero),
                          np.where(~fixed & has_up, gm * np.maximum(zu - z, 0.0), zero))
        viol = np.maximum(np.where(has_lo, zl - z, zero), np.where(has_up, z - zu, zero))
    out = np.zeros((B, 6))
    out[:, 0], out[:, 1], out[:, 3] = mx(stat), mx(comp), np.maximum(mx(viol), 0.0)
    out[:, 2] = mx(np.abs(RES[:, :ns]))
    out[:, 4] = mx(np.abs(sigma * np.asarray(VALS)[:, -nv:]))
    out[:, 5] = mx(np.abs(lamF))
    if np_:
        c, l = RES[:, ns:], np.asarray(lamC, dtype=np.float64)
        cl, cu = (np.asarray(a, dtype=np.float64).reshape(1, np_, 1) for a in (cl, cu))
        lp, lm = np.maximum(l, 0.0), np.maximum(-l, 0.0)
        c_lo, c_up = np.abs(cl) < INF_BOUND, np.abs(cu) < INF_BOUND
        with np.errstate(invalid="ignore", over="ignore"):
            cc = np.maximum(np.where(c_up, lp * np.maximum(cu - c, 0.0), lp), np.where(c_lo, lm * np.maximum(c - cl, 0.0), lm))
            cv = np.maximum(np.where(c_lo, cl - c, 0.0), np.where(c_up, c - cu, 0.0))
        out[:, 1] = np.maximum(out[:, 1], mx(cc))
        out[:, 3] = np.maximum(out[:, 3], mx(cv))
        out[:, 5] = np.maximum(out[:, 5], mx(np.abs(l)))
    return out
