"""Reference of the relative local ODE error (include/emi355x.h, emi_ode_error_*): a numpy restatement of the definition in long
double (the reference) and in float64 (held to the same bound as the kernels), the inputs the CPU and GPU tests share, and the bound.

The restatement builds its own operator from (tau, w) at the library's points tq -- it never reads the library's E, E' --, and takes
f and its Jacobian at the points from the CPU oracle on a points-only mesh (the traced demo model: from the long-double numpy
restatement of tests/test_gpu_traced.py), in float64 at the float64-rounded interpolated values.

The bound (derived, nothing measured).  u = 2^-53, p = q (M-1) + k:
    |eta - eta_ref|_ik <= (M + 16) u S_ik,
    S_ik = (tau_k+1 - tau_k)/2 h sum_q g_q ( sum_j |E'_pj| |x_ij| / h + |f_i| + sum_v |df_i/dz_v| sum_j |E_pj| |z_vj| )
any order of M rounded multiply-adds gives (M + 1) u on sum |terms|; the error of the interpolated values goes through f to first
order (a clip and an absolute value are 1-Lipschitz); fewer than 15 further roundings act on quantities of that size.
    |err - err_ref| <= max_ik bound_ik / (W_i + 1) + err_ref max_i dW_i / (W_i + 1),   dW_i = (M + 1) u max_k sum_j |D_kj| |x_ij| / h.
The product kernel alone: (K + 1) u sum_j |OP_cj| |v_j|, no margin."""
import functools
import os

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
OPERATOR_FIXTURE = os.path.join(HERE, "golden", "ode_error_operators.npz")
OPERATOR_SIZES = (2, 3, 9, 41, 65)      # tests/golden/gen_ode_error_golden.py: SIZES
# elementwise gates of emi_ode_error_operator against the mpmath operators, in units of 2^-53 sum_j |E*_pj| and 2^-53 sum_j |E'*_pj|:
# the largest ratio measured over OPERATOR_SIZES rounded up to the next power of two (tests/test_ode_error_cpu.py prints the
# figures).  Measured: E 1.0 / 0.8 / 7.3 / 66.8 / 332.4, E' 0.0 / 0.7 / 4.5 / 36.6 / 213.1 at M = 2 / 3 / 9 / 41 / 65.  What they cover:
# the nodes of emi_lgl are rounded doubles and the operator is that of the rounded point; near the ends of a mesh, where nodes lie
# ~ 1 / M^2 apart, a rounding of a node or of a point moves s - tau_j by a relative ~ M^2 eps.
E_GATE = 512.0
ED_GATE = 256.0
U53 = 2.0 ** -53
LD = np.longdouble

MODELS = ("pointmass", "quadrotor", "fixedwing", "traced")
SHAPES = ((1, 2), (3, 3), (5, 9), (2, 41), (17, 130), (3, 257))
PRODUCT_SHAPES = ((2, 5), (3, 1), (47, 63), (128, 64), (130, 645))      # (K, N)
PRODUCT_ROWS = (1, 7, 97, 513)

_FW_S = np.array([100, 100, 50, 0.4, 0.3, 3.0, 5, 2, 2, 0.5, 0.5, 0.5])
_FW_O = np.array([0, 0, -100, 0, 0, 0, 25, 0, 0, 0, 0, 0.0])
# model -> library model id (None: the traced demo model), parameters, (t0, tf), state range, control bounds
SPEC = {
    "pointmass": dict(model=0, params=[], t=(0.0, 16.0), xlo=[0.0, 0.0], xhi=[7.0, 7.0], ul=[-0.5, -0.5], uu=[0.5, 0.5]),
    "quadrotor": dict(model=1, params=[1.0, 0.01, 9.81, 1.0, 1.0], t=(0.5, 9.0), xlo=[0, 0, -np.pi / 4, -2, -2, -1.0],
                      xhi=[10, 10, np.pi / 4, 2, 2, 1.0], ul=[0.0, -1.0], uu=[25.0, 1.0]),
    "fixedwing": dict(model=2, params=[10.0, 0.8, 1.1, 1.8, 9.81, 120.0, 0.3, 4.5, 0.03, 0.05, 0.08, -0.6, 0.06, 25.0, 0.9, 1.0],
                      t=(0.0, 20.0), xlo=list(_FW_O - _FW_S), xhi=list(_FW_O + _FW_S), ul=[10.0, -0.3, -0.3, -0.3], uu=[50.0, 0.3, 0.3, 0.3]),
    "traced": dict(model=None, params=[], t=(0.25, 3.0), xlo=[0.2, 0.2], xhi=[1.2, 1.2], ul=[0.2], uu=[1.2]),
}


def gauss5():
    return np.polynomial.legendre.leggauss(5)


def operator_fixture():
    z = np.load(OPERATOR_FIXTURE)
    return {M: (z[f"E_{M}"], z[f"Ed_{M}"], z[f"tq_{M}"]) for M in OPERATOR_SIZES}


def operators(tau, w, tq, dtype=LD):
    """(E, E') [P][M] of the definition at the points tq, in dtype"""
    tau, w, tq = (np.asarray(a).astype(dtype) for a in (tau, w, tq))
    sgn = np.where(np.arange(len(tau)) % 2 == 1, dtype(-1), dtype(1))
    d = tq[:, None] - tau[None, :]
    lam = sgn * np.sqrt(w) / d
    S = lam.sum(1, keepdims=True)
    T = (lam / d).sum(1, keepdims=True)
    E = lam / S
    return E, (E * T - lam / d) / S


def library_points(M, mesh):
    import etol_amd as E
    return E.Evaluator.ode_error_operator(M, mesh)[2]


# ---- f and its Jacobian at points (float64) ----------------------------------------------------------------------------------------
def model_fun(name):
    """-> fun(Zx [B][ns][P], Zu [B][nc][P], pts [P] in tau, t0, tf) -> F [B][ns][P], J [B][ns][nv][P]"""
    sp = SPEC[name]
    if sp["model"] is None:
        from test_gpu_traced import _custom_reference

        def fun(Zx, Zu, pts, t0, tf):
            P, h = len(pts), (tf - t0) / 2
            RES, J, _, _ = _custom_reference(Zx, Zu, t0 + h * (pts + 1), np.zeros((P, P)), np.zeros(P), h)
            return -RES / h, J
        return fun

    def fun(Zx, Zu, pts, t0, tf):
        P, h = len(pts), (tf - t0) / 2
        B, ns = Zx.shape[:2]
        nv = ns + Zu.shape[1]
        RES, VALS, _ = O.evaluate(sp["model"], sp["params"], P, (pts, np.zeros(P), np.zeros((P, P))), t0, tf, Zx, Zu)
        return -RES[:, :ns] / h, -VALS[:, :ns * nv].reshape(B, ns, nv, P) / h
    return fun


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def overshoot_instance(B):
    """the instance of a batch whose controls are a step between the bounds"""
    return 2 if B >= 3 else 0


@functools.lru_cache(maxsize=None)
def case(name, B, M, poly=False):
    """One batch: instance b % 3 = 0 smooth, 1 rough (node noise), 2 smooth states under controls that step from just below the upper
    to just above the lower bound, so that the interpolant overshoots both (batches of fewer than three instances: instance 0;
    two nodes: a line cannot overshoot, the first node's control lies outside instead).  poly (point mass): x a polynomial of degree
    min(M - 1, 4) in time and u its exact derivative: eta is 0 up to rounding."""
    sp = SPEC[name]
    tau, w, D = O.lgl(M)
    t0, tf = sp["t"]
    h = (tf - t0) / 2
    xlo, xhi, ul, uu = (np.array(sp[k], dtype=np.float64) for k in ("xlo", "xhi", "ul", "uu"))
    ns, nc = len(xlo), len(ul)
    rng = np.random.default_rng(1000 * M + 10 * B + MODELS.index(name))
    lo, hi = np.concatenate([xlo, ul]), np.concatenate([xhi, uu])
    mid, half = (0.5 * (lo + hi))[:, None], (0.5 * (hi - lo))[:, None]
    Z = np.empty((B, ns + nc, M))
    v = np.arange(ns + nc)[:, None]
    for b in range(B):
        Z[b] = mid + 0.6 * half * np.sin((1 + 0.37 * v) * tau[None, :] + 0.5 * b + v)
        if b % 3 == 1:
            Z[b] += 0.3 * half * rng.uniform(-1, 1, (ns + nc, M))
        if b == overshoot_instance(B) or b % 3 == 2:
            step = np.where(np.arange(M) <= (M - 1) // 2, uu[:, None] - 0.02 * (uu - ul)[:, None], ul[:, None] + 0.02 * (uu - ul)[:, None])
            if M == 2:
                step = np.stack([uu + 0.1 * (uu - ul), 0.5 * (ul + uu)], 1)
            Z[b, ns:] = step
    if poly:
        assert name == "pointmass"
        deg = min(M - 1, 4)
        for b in range(B):
            for i in range(ns):
                c = rng.uniform(-1, 1, deg + 1) * 0.1
                c[0] += 3.0
                p = np.polynomial.Polynomial(c)
                Z[b, i] = p(tau)
                Z[b, ns + i] = p.deriv()(tau) / h       # |u| <= 0.1 * (1 + 2 + 3 + 4) / 8 < 0.5: inside the bounds
    c = dict(name=name, B=B, M=M, t0=t0, tf=tf, tau=tau, w=w, D=D, ns=ns, nc=nc, ul=ul, uu=uu,
             X=np.ascontiguousarray(Z[:, :ns]), U=np.ascontiguousarray(Z[:, ns:]))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def estimate(c, tq, dtype=LD, clip=True, X=None, U=None):
    """The definition on the batch of `c` in dtype -> dict eta [B][ns][M-1], err [B], W [B][ns], and the bound's parts: S [B][ns][M-1],
    dW [B][ns], clipped [B] (points where a control's interpolant lies outside its bounds)."""
    tau, w, D, M, ns, nc = c["tau"], c["w"], c["D"], c["M"], c["ns"], c["nc"]
    X = c["X"] if X is None else X
    U = c["U"] if U is None else U
    B, nq = X.shape[0], M - 1
    E, Ed = operators(tau, w, tq, dtype)
    h = (dtype(c["tf"]) - dtype(c["t0"])) / dtype(2)
    Z = np.concatenate([X, U], 1).astype(dtype)
    Zq = Z @ E.T                                            # [B][nv][P]
    raw = Zq[:, ns:].copy()
    clipped = np.zeros(B, dtype=int)
    if clip:
        lo, hi = c["ul"].astype(dtype)[None, :, None], c["uu"].astype(dtype)[None, :, None]
        clipped = ((raw < lo) | (raw > hi)).sum((1, 2))
        Zq[:, ns:] = np.minimum(np.maximum(raw, lo), hi)
    dXq = (Z[:, :ns] @ Ed.T) / h
    F, J = model_fun(c["name"])(np.ascontiguousarray(Zq[:, :ns].astype(np.float64)), np.ascontiguousarray(Zq[:, ns:].astype(np.float64)),
                                np.asarray(tq, dtype=np.float64), c["t0"], c["tf"])
    g = gauss5()[1].astype(dtype)
    half = (dtype(0.5) * np.diff(tau.astype(dtype))) * h                      # [M-1]
    resid = np.abs(dXq - F.astype(dtype)).reshape(B, ns, 5, nq)
    eta = half * (g[None, None, :, None] * resid).sum(2)
    DX = X.astype(dtype) @ D.astype(dtype).T
    W = np.maximum(np.abs(X.astype(dtype)).max(2), np.abs(DX).max(2) / h)
    err = (eta / (W[:, :, None] + 1)).max((1, 2))
    # the bound's scale, in float64
    aE, aEd, aZ, hf = np.abs(E).astype(np.float64), np.abs(Ed).astype(np.float64), np.abs(Z).astype(np.float64), float(h)
    mag = (aZ[:, :ns] @ aEd.T) / hf + np.abs(F) + np.einsum("bivp,bvp->bip", np.abs(J), aZ @ aE.T)
    S = (0.5 * np.diff(tau) * hf) * (gauss5()[1][None, None, :, None] * mag.reshape(B, ns, 5, nq)).sum(2)
    dW = (M + 1) * U53 * (np.abs(X) @ np.abs(D).T).max(2) / hf
    return dict(eta=eta, err=err, W=W, S=S, dW=dW, clipped=clipped)


@functools.lru_cache(maxsize=None)
def reference(name, B, M, poly=False):
    """the long-double estimate of case(name, B, M) at the library's points, computed once"""
    c = case(name, B, M, poly)
    tq = library_points(M, (c["tau"], c["w"]))
    r = estimate(c, tq)
    r["tq"] = tq
    return r


def eta_bound(ref, M):
    return (M + 16) * U53 * ref["S"]


def err_bound(ref, M):
    W = ref["W"].astype(np.float64)
    return (eta_bound(ref, M) / (W[:, :, None] + 1)).max((1, 2)) + ref["err"].astype(np.float64) * (ref["dW"] / (W + 1)).max(1)


def ratios(got_eta, got_err, ref, M):
    """largest |eta - eta_ref| / bound and |err - err_ref| / bound (a zero bound with a zero difference counts 0)"""
    de = np.abs(np.asarray(got_eta).astype(LD) - ref["eta"]).astype(np.float64)
    dr = np.abs(np.asarray(got_err).astype(LD) - ref["err"]).astype(np.float64)
    be, br = eta_bound(ref, M), err_bound(ref, M)
    with np.errstate(divide="ignore", invalid="ignore"):
        re = np.where(de == 0, 0.0, de / be)
        rr = np.where(dr == 0, 0.0, dr / br)
    return float(re.max()) if re.size else 0.0, float(rr.max())
