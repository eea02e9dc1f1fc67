"""Reference of the relative local ODE error of a context WITH delays (include/emi355x.h, emi_ode_error_total_*): the definition
restated in numpy, in long double (the reference) and in float64 (held to the same bound as the kernels), the inputs the CPU and GPU
tests share, and the bound.

The restatement builds its own E, E' and Edel(i dt) with ode_error_ref.operators from (tau, w) at the library's points tq -- it never
reads the library's operators.  The shifted abscissae are formed in float64 by the rule of the definition,
    t_p = t0 + h (tq_p + 1),  ts = max(t_p - delay, t0),  x_p = (ts - t0) / h - 1,    delay = i * dt,
a row with ts <= t0 is e_0 and one with x_p == tau_j is e_j.  f and its Jacobian at the points come from the CPU oracle on a
points-only mesh with the EXTENDED controls [free controls | delayed slots] as its inputs, in float64 at the float64-rounded values.

The bound (derived, nothing measured) is that of ode_error_ref.py with v running over the extended variables, each with the operator
that forms it in S_ik:
    |eta - eta_ref|_ik <= (M + 16) u S_ik,
    S_ik = (tau_k+1 - tau_k)/2 h sum_q g_q ( sum_j |E'_pj| |x_ij| / h + |f_i| + sum_v |df_i/dz_v| sum_j |OP(v)_pj| |z_src(v),j| ),
OP(v) = E for the states and the free controls, Edel(i dt) for a slot (src, i): a delayed value is one more dot product of M terms
with its own rounding, which reaches f to first order (a clip is 1-Lipschitz).  The (M + 16) u constant and the bound on err are
unchanged: W and D x do not see the delays."""
import functools

import numpy as np

import ode_error_ref as R
import oracle_lib as O
from delay_adjoint_ref import slots

LD = np.longdouble
U53 = R.U53

# name -> oracle / library model id (the demo is oracle model 3; on the device it is the traced model of tests/test_gpu_delay_adjoint.py),
# parameters, the split, (t0, tf), state range, bounds of the FREE controls
SPEC = {
    "demo": dict(model=3, params=[0.7, 0.3], ns=2, ncf=2, xh=3, uh=1, t=(0.5, 6.5), xlo=[0.5, 1.5], xhi=[1.5, 2.5], ul=[-0.3, 0.1], uu=[0.3, 0.3]),
    # the built-in quadrotor with its second control slot declared the delayed copy of the first: one free control
    "quad": dict(model=1, params=[1.0, 0.01, 9.81, 1.0, 1.0], ns=6, ncf=1, xh=0, uh=1, t=(0.5, 9.0), xlo=[0, 0, -np.pi / 4, -2, -2, -1.0],
                 xhi=[10, 10, np.pi / 4, 2, 2, 1.0], ul=[0.0], uu=[25.0]),
}
# (name, B, M, dt / (tf - t0)).  0.2 of the horizon: delays of one and two steps clamp the points of the first 0.2 / 0.4 of the horizon
# and no others (at M = 2: one and two of the five points).  258 nodes: 257 intervals, a second workgroup with one live thread.
# 1.3: every delayed value is the initial one.
CASES = [("demo", 1, 2, 0.2), ("demo", 3, 3, 0.2), ("demo", 5, 9, 0.2), ("demo", 2, 41, 0.2), ("demo", 17, 130, 0.2), ("demo", 3, 258, 0.2),
         ("demo", 3, 9, 1.3), ("quad", 3, 9, 0.15), ("quad", 2, 130, 0.15)]


def case_id(c):
    return f"{c[0]}_{c[1]}x{c[2]}_dt{c[3]}"


def oracle_fun(model, params):
    """-> fun(Zx [B][ns][P], Zu [B][nc][P], pts [P] in tau, t0, tf) -> F [B][ns][P], J [B][ns][ns+nc][P]: the oracle on a points-only mesh"""
    def fun(Zx, Zu, pts, t0, tf):
        P, h = len(pts), (tf - t0) / 2
        B, ns = Zx.shape[:2]
        nv = ns + Zu.shape[1]
        RES, VALS, _ = O.evaluate(model, params, P, (pts, np.zeros(P), np.zeros((P, P))), t0, tf, Zx, Zu)
        return -RES[:, :ns] / h, -VALS[:, :ns * nv].reshape(B, ns, nv, P) / h
    return fun


@functools.lru_cache(maxsize=None)
def case(name, B, M, dtf):
    """One batch, as ode_error_ref.case: instance b % 3 = 0 smooth, 1 rough (node noise), 2 smooth states under free controls that step
    from just below the upper to just above the lower bound, so that the interpolant -- and its delayed copy -- overshoots both (fewer
    than three instances: instance 0; two nodes: the first node's control lies outside instead).  Where the delay exceeds the horizon
    the delayed copy is the first node's control everywhere: that node's control lies outside its bounds there too."""
    sp = SPEC[name]
    tau, w, D = O.lgl(M)
    t0, tf = sp["t"]
    xlo, xhi, ul, uu = (np.array(sp[k], dtype=np.float64) for k in ("xlo", "xhi", "ul", "uu"))
    ns, ncf = sp["ns"], sp["ncf"]
    rng = np.random.default_rng(5000 * M + 10 * B + len(name))
    lo, hi = np.concatenate([xlo, ul]), np.concatenate([xhi, uu])
    mid, half = (0.5 * (lo + hi))[:, None], (0.5 * (hi - lo))[:, None]
    Z = np.empty((B, ns + ncf, M))
    v = np.arange(ns + ncf)[:, None]
    for b in range(B):
        Z[b] = mid + 0.6 * half * np.sin((1 + 0.37 * v) * tau[None, :] + 0.5 * b + v)
        if b % 3 == 1:
            Z[b] += 0.3 * half * rng.uniform(-1, 1, (ns + ncf, M))
        if b == R.overshoot_instance(B) or b % 3 == 2:
            step = np.where(np.arange(M) <= (M - 1) // 2, uu[:, None] - 0.02 * (uu - ul)[:, None], ul[:, None] + 0.02 * (uu - ul)[:, None])
            if M == 2:
                step = np.stack([uu + 0.1 * (uu - ul), 0.5 * (ul + uu)], 1)
            elif dtf >= 1.0:
                step[:, 0] = uu + 0.1 * (uu - ul)
            Z[b, ns:] = step
    nd = len(slots(ns, ncf, sp["xh"], sp["uh"]))
    c = dict(name=name, B=B, M=M, t0=t0, tf=tf, dt=dtf * (tf - t0), tau=tau, w=w, D=D, ns=ns, ncf=ncf, nc=ncf + nd, xh=sp["xh"], uh=sp["uh"],
             model=sp["model"], params=sp["params"], ul=ul, uu=uu, X=np.ascontiguousarray(Z[:, :ns]), U=np.ascontiguousarray(Z[:, ns:]))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def shifted_points(tq, t0, tf, delay):
    """(x_p, ts <= t0) in float64, operation for operation the rule of the definition"""
    tq = np.asarray(tq, dtype=np.float64)
    h = (tf - t0) / 2.0
    tp = t0 + h * (tq + 1.0)
    ts = tp - delay
    ts = np.where(ts < t0, t0, ts)
    return (ts - t0) / h - 1.0, ts <= t0


def delay_operator(tau, w, tq, t0, tf, delay, dtype=LD):
    """Edel(delay) [P][M] of the definition in dtype: the barycentric rows at the shifted abscissae, unit rows where the definition says so"""
    tau = np.asarray(tau, dtype=np.float64)
    x, before = shifted_points(tq, t0, tf, delay)
    hit = np.full(len(x), -1)
    for j in range(len(tau)):
        hit[x == tau[j]] = j
    hit[before] = 0
    free = hit < 0
    out = np.zeros((len(x), len(tau)), dtype=dtype)
    if free.any():
        out[free] = R.operators(tau, w, x[free], dtype)[0]
    out[~free, hit[~free]] = 1
    return out


def estimate(c, tq, dtype=LD, clip=True, X=None, U=None):
    """The definition on the batch of `c` in dtype -> dict eta [B][ns][M-1], err [B], W [B][ns], the bound's parts S [B][ns][M-1] and
    dW [B][ns], clipped [B] (points where a FREE control's interpolant lies outside its bounds) and clipped_delayed [B] (points where a
    delayed control copy does)."""
    tau, w, D, M, ns, ncf = c["tau"], c["w"], c["D"], c["M"], c["ns"], c["ncf"]
    X = c["X"] if X is None else X
    U = c["U"] if U is None else U
    B, nq = X.shape[0], M - 1
    sl = slots(ns, ncf, c["xh"], c["uh"])
    E, Ed = R.operators(tau, w, tq, dtype)
    nd = max(max(c["xh"] - 1, 0), c["uh"])
    Edel = [delay_operator(tau, w, tq, c["t0"], c["tf"], (i + 1) * c["dt"], dtype) for i in range(nd)]
    h = (dtype(c["tf"]) - dtype(c["t0"])) / dtype(2)
    Z = np.concatenate([X, U], 1).astype(dtype)
    lo, hi = c["ul"].astype(dtype)[None, :, None], c["uu"].astype(dtype)[None, :, None]
    Zq = Z @ E.T                                            # [B][ns+ncf][P]
    clipped, clipped_delayed = np.zeros(B, dtype=int), np.zeros(B, dtype=int)
    if clip:
        raw = Zq[:, ns:].copy()
        clipped = ((raw < lo) | (raw > hi)).sum((1, 2))
        Zq[:, ns:] = np.minimum(np.maximum(raw, lo), hi)
    ext, ops = [Zq], [E] * (ns + ncf)                        # the extended variables and the operator that forms each
    for src, i in sl:
        v = Z[:, src] @ Edel[i - 1].T                       # [B][P]
        if clip and src >= ns:
            l, u = lo[:, src - ns], hi[:, src - ns]
            clipped_delayed += ((v < l) | (v > u)).sum(1)
            v = np.minimum(np.maximum(v, l), u)
        ext.append(v[:, None])
        ops.append(Edel[i - 1])
    Zx = np.concatenate(ext, 1)                             # [B][ns+nc][P]
    src_of = list(range(ns + ncf)) + [s for s, _ in sl]
    dXq = (Z[:, :ns] @ Ed.T) / h
    F, J = oracle_fun(c["model"], c["params"])(np.ascontiguousarray(Zx[:, :ns].astype(np.float64)), np.ascontiguousarray(Zx[:, ns:].astype(np.float64)),
                                               np.asarray(tq, dtype=np.float64), c["t0"], c["tf"])
    g = R.gauss5()[1].astype(dtype)
    half = (dtype(0.5) * np.diff(tau.astype(dtype))) * h
    resid = np.abs(dXq - F.astype(dtype)).reshape(B, ns, 5, nq)
    eta = half * (g[None, None, :, None] * resid).sum(2)
    DX = X.astype(dtype) @ D.astype(dtype).T
    W = np.maximum(np.abs(X.astype(dtype)).max(2), np.abs(DX).max(2) / h)
    err = (eta / (W[:, :, None] + 1)).max((1, 2))
    # the bound's scale, in float64
    aZ, hf = np.abs(Z).astype(np.float64), float(h)
    amp = np.stack([aZ[:, s] @ np.abs(ops[v]).astype(np.float64).T for v, s in enumerate(src_of)], 1)       # [B][ns+nc][P]
    mag = (aZ[:, :ns] @ np.abs(Ed).astype(np.float64).T) / hf + np.abs(F) + np.einsum("bivp,bvp->bip", np.abs(J), amp)
    S = (0.5 * np.diff(tau) * hf) * (R.gauss5()[1][None, None, :, None] * mag.reshape(B, ns, 5, nq)).sum(2)
    dW = (M + 1) * U53 * (np.abs(X) @ np.abs(D).T).max(2) / hf
    return dict(eta=eta, err=err, W=W, S=S, dW=dW, clipped=clipped, clipped_delayed=clipped_delayed)


@functools.lru_cache(maxsize=None)
def reference(name, B, M, dtf):
    """the long-double estimate of case(name, B, M, dtf) at the library's points, computed once"""
    c = case(name, B, M, dtf)
    tq = R.library_points(M, (c["tau"], c["w"]))
    r = estimate(c, tq)
    r["tq"] = tq
    return r
