"""numpy restatement of the array arithmetic of one interior-point iteration (host/emi_nlp.cpp: the ipm_* functions;
csrc/emi_ipm.hip: the batched kernels), evaluated in np.longdouble, with a running error bound beside every value.

Every quantity is a T(v, m, d): value v, m = the sum of the absolute values of the terms v is made of (inputs: |v|), and d = the
number of floating-point operations that may have rounded on the way: the c of the bound  |computed - v| <= c eps m.  The rules
(first-order error analysis, eps = 2^-52 per operation, i.e. twice the unit round-off):
    x + y, x - y:  m = mx + my,        c = max(cx, cy) + 1        (the terms of a sum add up; one more rounding)
    x * y:         m = mx my,          c = cx + cy + 1            (relative errors of the factors add)
    x / y:         m = mx my / y^2,    c = cx + cy + 1            (my / |y| >= 1 is the amplification of the divisor's error)
    log x:         m = |log x| + mx / |x|,  c = cx + 2            (one log counts as 2)
    where(..):     the chosen branch;  an exact 0 or a negation costs nothing.
So c is "operations on the longest path plus the terms summed" wherever the expression is a chain, and the sum over both
branches of a product otherwise; the c of every output is written next to its formula below (for the branch with both bounds
present) and computed by the same rules at run time -- the run-time figure is what the tests use.

Sums over an instance (dphi, phi, infeas, the scale sums of kkt_error) are returned with n = the number of terms and S = the sum
of the absolute values of the terms: any summation order stays within (n - 1) eps S.  Extrema have no summation error: apr, adu,
mmax and emax are within 4 eps RELATIVE of the reference's (their candidates are at most three correctly rounded operations from
exact inputs and do not cancel).  viol and the three parts of kkt_error are maxima of residuals, i.e. of cancelling sums: there
the bound is 4 eps of the sum of the absolute values of the extremal candidate's terms (_ext explains why nothing tighter can
hold).  The candidates and the terms of the sums are formed from the element-wise outputs the code under test produced (its step,
its reset slacks): each stage is checked on its inputs.

Case generator: seeded, strictly interior iterates on the shapes of the built-in models."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
INF = 1e19

# (nv, ns, np) -> built-in model
MODEL_OF = {(4, 2): 0, (8, 6): 1, (16, 12): 2}
DISCS = [[4.0, 3.2, 0.64], [6.3, 4.4, 0.49], [2.5, 1.2, 0.16]]


class T:
    __slots__ = ("v", "m", "d")
    __array_ufunc__ = None          # numpy arrays on the left of an operator defer to T

    def __init__(self, v, m=None, d=None):
        self.v = np.asarray(v, dtype=LD)
        self.m = np.abs(self.v) if m is None else np.asarray(m, dtype=LD)
        self.d = np.zeros(self.v.shape, dtype=np.int64) if d is None else np.asarray(d, dtype=np.int64)

    @staticmethod
    def of(x):
        return x if isinstance(x, T) else T(x)

    def __neg__(self):
        return T(-self.v, self.m, self.d)

    def __add__(self, o):
        o = T.of(o)
        return T(self.v + o.v, self.m + o.m, np.maximum(self.d, o.d) + 1)

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-T.of(o))

    def __rsub__(self, o):
        return T.of(o) + (-self)

    def __mul__(self, o):
        o = T.of(o)
        return T(self.v * o.v, self.m * o.m, self.d + o.d + 1)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = T.of(o)
        with np.errstate(invalid="ignore", divide="ignore"):        # (a branch that where() does not take may divide by 0)
            return T(self.v / o.v, self.m * o.m / (o.v * o.v), self.d + o.d + 1)

    def __rtruediv__(self, o):
        return T.of(o) / self

    def log(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            lv = np.log(self.v)
            return T(lv, np.abs(lv) + self.m / np.abs(self.v), self.d + 2)

    def abs(self):
        return T(np.abs(self.v), self.m, self.d)

    def bound(self):
        """c eps m"""
        return np.asarray(self.d * EPS * self.m, dtype=np.float64)

    def f64(self):
        return np.asarray(self.v, dtype=np.float64)

    def __getitem__(self, i):
        return T(self.v[i], self.m[i], self.d[i])


def where(cond, a, b=0.0):
    a, b = T.of(a), T.of(b)
    shp = np.broadcast(cond, a.v, b.v).shape
    bc = lambda x: np.broadcast_to(x, shp)
    return T(np.where(cond, bc(a.v), bc(b.v)), np.where(cond, bc(a.m), bc(b.m)), np.where(cond, bc(a.d), bc(b.d)))


def add0(acc, cond, x):
    """`acc += x` under a condition, where acc may still be the exact 0 it started as"""
    s = acc + x
    first = (acc.m == 0) & (acc.d == 0)
    s = where(first, x, s)           # 0 + x is exact
    return where(cond, s, acc)


# ---- what a case holds -----------------------------------------------------------------------------------------------------
POINT = ("X", "U", "S", "E1", "E2")
DUALS = ("LamF", "Y", "ZL", "ZU", "VL", "VU", "W1", "W2")
STEP = ("DZLam", "DS", "DY", "DE1", "DE2", "DZL", "DZU", "DVL", "DVU", "DW1", "DW2")
ELIM = ("Sigma", "SigT", "SigS", "RhatS", "Rt")


def default_rows(ns, nv, npth):
    return [[(0, ns * nv + 2 * j), (1, ns * nv + 2 * j + 1)] for j in range(npth)]


def row_bounds(c):
    """hasL, hasU [np] and the scaled bounds lo, hi, cs [np] as the host forms them (one double multiplication)"""
    cl, cu = np.asarray(c["cl"], dtype=np.float64), np.asarray(c["cu"], dtype=np.float64)
    cs = np.ones(c["np"]) if c.get("cscale") is None else np.asarray(c["cscale"], dtype=np.float64)
    hasL, hasU = cl > -INF, cu < INF
    return hasL, hasU, np.where(hasL, cs * cl, cl), np.where(hasU, cs * cu, cu), cs


def _r(a):          # [np] -> broadcast over [B][np][M]
    return np.asarray(a)[None, :, None]


def _var_parts(c, pt):
    """z, the two gaps, and which sides of which variables count"""
    z = T(np.concatenate([pt["X"], pt["U"]], axis=1))
    zl, zu = np.broadcast_to(c["zl"], z.v.shape), np.broadcast_to(c["zu"], z.v.shape)
    free = zu > zl
    return z, z - zl, zu - z, free, free & (zl > -INF), free & (zu < INF)


def _par(c, i):
    return T(c["par"][:, i][:, None, None])


def _row_parts(c, pt):
    hasL, hasU, lo, hi, cs = row_bounds(c)
    s = T(pt["S"])
    return _r(hasL), _r(hasU), s - _r(lo), _r(hi) - s, _r(cs)


# ---- reduce ------------------------------------------------------------------------------------------------------------------
def reduce_ref(c):
    """-> dict of T: SigS, RhatS, SigT, Rt [B][np][M], Sigma [B][nv][M], Rhs [B][nv+ns][M]"""
    ns, nv, npth = c["ns"], c["nv"], c["np"]
    mu, rho = _par(c, 0), _par(c, 1)
    out = {}
    if npth:
        hasL, hasU, gL, gU, cs = _row_parts(c, c)
        s, e1, e2, y = T(c["S"]), T(c["E1"]), T(c["E2"]), T(c["Y"])
        vL, vU, w1, w2 = T(c["VL"]), T(c["VU"]), T(c["W1"]), T(c["W2"])
        cval = T(cs) * T(c["RES"][:, ns:])                                   # c = 1
        rowres = T(c["RowRes"]) if c.get("RowRes") is not None else cval - s - e1 + e2      # c = 4
        zero = T(np.zeros(s.v.shape))
        sg = add0(add0(zero, hasL, vL / gL), hasU, vU / gU)                  # sig_s: c = 3  (gap, quotient, sum)
        rh = add0(add0(-y, hasL, -(mu / gL)), hasU, mu / gU)                 # rhat_s: c = 4
        a1, a2 = e1 / w1, e2 / w2
        out["SigS"], out["RhatS"] = sg, rh
        out["SigT"] = 1.0 / (1.0 / sg + a1 + a2)                             # c = 7
        out["Rt"] = rowres + rh / sg - a1 * (y - rho + mu / e1) - a2 * (y + rho - mu / e2)      # c = 11
    z, gm, gp, free, fL, fU = _var_parts(c, c)
    zL, zU, G = T(c["ZL"]), T(c["ZU"]), T(c["G"])
    zero = T(np.zeros(z.v.shape))
    out["Sigma"] = add0(add0(zero, fL, zL / gm), fU, zU / gp)                # c = 3
    rr = add0(add0(G, fL, -(mu / gm)), fU, mu / gp)                          # c = 4
    rhs = -rr
    if npth:
        t = out["SigT"] * out["Rt"]                                          # c = 19
        acc = [rhs[:, v] for v in range(nv)]
        for j, row in enumerate(c["rows"]):                                  # one product and one subtraction per partial
            for v, e in row:
                acc[v] = acc[v] - (T(cs[0, j, 0]) * T(c["VALS"][:, e])) * t[:, j]
        rhs = T(np.stack([a.v for a in acc], 1), np.stack([a.m for a in acc], 1), np.stack([a.d for a in acc], 1))
    rhs = where(free, rhs, 0.0)
    dres = -T(c["DefRes"] if c.get("DefRes") is not None else c["RES"][:, :ns])     # exact
    out["Rhs"] = T(np.concatenate([rhs.v, dres.v], 1), np.concatenate([rhs.m, dres.m], 1), np.concatenate([rhs.d, dres.d], 1))
    return out


# ---- expand --------------------------------------------------------------------------------------------------------------------
def expand_ref(c, el, dzlam):
    """el: the reduction's outputs as doubles (SigT, Rt, SigS, RhatS); dzlam: the solved step [B][nv+ns][M] -> dict of T: the step
    arrays (DZLam exact: the input with the fixed variables zeroed)"""
    ns, nv, npth = c["ns"], c["nv"], c["np"]
    mu, rho = _par(c, 0), _par(c, 1)
    z, gm, gp, free, fL, fU = _var_parts(c, c)
    dzv = np.where(free, dzlam[:, :nv], 0.0)
    dz = T(dzv)
    zL, zU = T(c["ZL"]), T(c["ZU"])
    out = {"DZLam": T(np.concatenate([dzv, dzlam[:, nv:]], 1))}
    out["DZL"] = where(fL, mu / gm - zL - zL / gm * dz, 0.0)                 # c = 5
    out["DZU"] = where(fU, mu / gp - zU + zU / gp * dz, 0.0)
    if npth:
        hasL, hasU, gL, gU, cs = _row_parts(c, c)
        e1, e2, y = T(c["E1"]), T(c["E2"]), T(c["Y"])
        vL, vU, w1, w2 = T(c["VL"]), T(c["VU"]), T(c["W1"]), T(c["W2"])
        jc = []
        for j, row in enumerate(c["rows"]):
            a = None
            for v, e in row:                                                 # two products and one sum per partial
                term = (T(cs[0, j, 0]) * T(c["VALS"][:, e])) * dz[:, v]
                a = term if a is None else a + term
            jc.append(a)
        jcdz = T(np.stack([a.v for a in jc], 1), np.stack([a.m for a in jc], 1), np.stack([a.d for a in jc], 1))
        dy = T(el["SigT"]) * (jcdz + T(el["Rt"]))                            # c = 2 + (2 + partials)
        ds = (dy - T(el["RhatS"])) / T(el["SigS"])                           # c(dy) + 2
        de1 = e1 / w1 * (dy + y - rho + mu / e1)                             # c(dy) + 5
        de2 = e2 / w2 * (-dy - y - rho + mu / e2)
        out.update(DY=dy, DS=ds, DE1=de1, DE2=de2)
        out["DVL"] = where(hasL, mu / gL - vL - vL / gL * ds, 0.0)           # c(ds) + 4
        out["DVU"] = where(hasU, mu / gU - vU + vU / gU * ds, 0.0)
        out["DW1"] = mu / e1 - w1 - w1 / e1 * de1                            # c(de1) + 3
        out["DW2"] = mu / e2 - w2 - w2 / e2 * de2
    return out


def _ext(cands, kind, start, cancels=False):
    """extremum of the candidates (list of (T, mask)) with the value `start` always among them -> (value, tolerance).
    The tolerance is 4 eps |extremum|: the candidates of apr, adu, mmax and emax are at most three correctly rounded operations
    (a gap or a sum of two inputs, a product, a quotient) from exact inputs, none of which cancels, so each is relatively accurate
    to 1.5 eps and so is their extremum.  cancels=True is for candidates that ARE a cancelling sum of several inputs (a residual
    c - s - e1 + e2, a stationarity or complementarity residual): their rounding error is relative to the terms, not to the
    result, and no implementation can do better, so there the tolerance is 4 eps m with m the sum of the absolute values of the
    terms of the candidates within 1e-6 of the extremum."""
    vs, ms = [np.array([start], dtype=LD)], [np.array([abs(start)], dtype=LD)]
    for t, mask in cands:
        mask = np.broadcast_to(mask, t.v.shape)
        vs.append(t.v[mask]); ms.append(t.m[mask])
    v, m = np.concatenate(vs), np.concatenate(ms)
    ext = v.min() if kind == "min" else v.max()
    near = np.abs(v - ext) <= 1e-6 * np.abs(ext) + 1e-300
    return float(ext), float(4 * EPS * (m[near].max() if cancels else abs(ext)))


def _sum(classes):
    """classes: name -> list of (T, mask): -> dict value, n, S (sum of |terms|), share (per class, of S)"""
    tot, S, n, per = LD(0), LD(0), 0, {}
    for name, items in classes.items():
        a = LD(0)
        for t, mask in items:
            mask = np.broadcast_to(mask, t.v.shape)
            tot += t.v[mask].sum(dtype=LD); a += np.abs(t.v[mask]).sum(dtype=LD); n += int(mask.sum())
        per[name] = a
        S += a
    return dict(value=float(tot), n=n, S=float(S), share={k: float(v / S) if S > 0 else 0.0 for k, v in per.items()},
                tol=float(max(n - 1, 0) * EPS * S))


def expand_scalars_ref(c, st):
    """st: the step arrays as doubles (dz of fixed variables zero) -> per instance: apr, adu (value, tol), dphi (sum dict), mmax"""
    ns, nv, npth, B = c["ns"], c["nv"], c["np"], c["B"]
    res = []
    for b in range(B):
        cb = instance(c, b)
        sb = {k: v[b:b + 1] for k, v in st.items()}
        mu, rho, tau = _par(cb, 0), _par(cb, 1), _par(cb, 2)
        z, gm, gp, free, fL, fU = _var_parts(cb, cb)
        dz, dzL, dzU = T(sb["DZLam"][:, :nv]), T(sb["DZL"]), T(sb["DZU"])
        zL, zU = T(cb["ZL"]), T(cb["ZU"])
        pr = [(-tau * gm / dz, fL & (dz.v < 0)), (tau * gp / dz, fU & (dz.v > 0))]                # c = 3
        du = [(-tau * zL / dzL, free & (dzL.v < 0)), (-tau * zU / dzU, free & (dzU.v < 0))]      # c = 2
        gf = T(cb["VALS"][:, c["nvals"] - nv:])
        g = add0(add0(gf, fL, -(mu / gm)), fU, mu / gp)
        cls = {"variables": [(g * dz, free)]}
        mm = [((T(cb["LamF"]) + T(sb["DZLam"][:, nv:])).abs() / T(cb["rs"] if cb.get("rs") is not None else np.ones((1, ns, c["M"]))), True)]
        if npth:
            hasL, hasU, gL, gU, cs = _row_parts(cb, cb)
            e1, e2, y = T(cb["E1"]), T(cb["E2"]), T(cb["Y"])
            vL, vU, w1, w2 = T(cb["VL"]), T(cb["VU"]), T(cb["W1"]), T(cb["W2"])
            ds, de1, de2, dy = T(sb["DS"]), T(sb["DE1"]), T(sb["DE2"]), T(sb["DY"])
            dvL, dvU, dw1, dw2 = T(sb["DVL"]), T(sb["DVU"]), T(sb["DW1"]), T(sb["DW2"])
            pr += [(-tau * gL / ds, hasL & (ds.v < 0)), (tau * gU / ds, hasU & (ds.v > 0)), (-tau * e1 / de1, de1.v < 0), (-tau * e2 / de2, de2.v < 0)]
            du += [(-tau * vL / dvL, dvL.v < 0), (-tau * vU / dvU, dvU.v < 0), (-tau * w1 / dw1, dw1.v < 0), (-tau * w2 / dw2, dw2.v < 0)]
            zero = T(np.zeros(ds.v.shape))
            gs = add0(add0(zero, hasL, -(mu / gL)), hasU, mu / gU)
            cls["slacks"] = [(gs * ds, True)]
            cls["elastics"] = [((rho - mu / e1) * de1, True), ((rho - mu / e2) * de2, True)]
            mm.append(((y + dy).abs(), True))
        res.append(dict(apr=_ext(pr, "min", 1.0), adu=_ext(du, "min", 1.0), dphi=_sum(cls), mmax=_ext(mm, "max", 0.0)))
    return res


# ---- trial, merit, accept, error ---------------------------------------------------------------------------------------------------
def trial_ref(c, st, alpha):
    """point + alpha step -> dict of T (c = 2 each)"""
    nv, ns = c["nv"], c["ns"]
    al = T(np.asarray(alpha)[:, None, None])
    out = {"X": T(c["X"]) + al * T(st["DZLam"][:, :ns]), "U": T(c["U"]) + al * T(st["DZLam"][:, ns:nv])}
    for k, d in (("S", "DS"), ("E1", "DE1"), ("E2", "DE2")):
        if c["np"]:
            out[k] = T(c[k]) + al * T(st[d])
    return out


def reset_ref(c, pt):
    """the slack reset at the point pt -> (jump [B][np][M] bool, margin: keep - take as T, target [B][np][M] as T)"""
    ns = c["ns"]
    mu, nu = _par(c, 0), _par(c, 3)
    hasL, hasU, lo, hi, cs = row_bounds(c)
    s, e1, e2 = T(pt["S"]), T(pt["E1"]), T(pt["E2"])
    target = T(_r(cs)) * T(pt["RES"][:, ns:]) - e1 + e2                      # c = 3
    lo_e, hi_e = _r(np.where(hasL, lo, -INF)), _r(np.where(hasU, hi, INF))
    inside = (target.v > lo_e) & (target.v < hi_e)
    keep, take = nu * (target - s).abs(), T(np.zeros(s.v.shape))
    tv = where(inside, target, s)           # (keeps the logs of rows that cannot jump finite)
    keep = add0(keep, _r(hasL), -(mu * (s - lo_e).log())); take = add0(take, _r(hasL), -(mu * (tv - lo_e).log()))
    keep = add0(keep, _r(hasU), -(mu * (hi_e - s).log())); take = add0(take, _r(hasU), -(mu * (hi_e - tv).log()))
    margin = keep - take
    return inside & (margin.v > 0), margin, target, inside


def merit_ref(c, pt):
    """pt: X U S E1 E2 RES COST as doubles (S after the reset) -> per instance: phi, infeas (sum dicts)"""
    res = []
    ns, npth = c["ns"], c["np"]
    for b in range(c["B"]):
        cb = instance(c, b)
        pb = {k: np.asarray(v)[b:b + 1] for k, v in pt.items()}
        mu, rho = _par(cb, 0), _par(cb, 1)
        z, gm, gp, free, fL, fU = _var_parts(cb, pb)
        phi = {"cost": [(T(pb["COST"].reshape(1, 1, 1)), True)], "variables": [(-(mu * gm.log()), fL), (-(mu * gp.log()), fU)]}
        rs = T(cb["rs"] if cb.get("rs") is not None else np.ones((1, ns, c["M"])))
        inf = {"defects": [(rs * T(pb["RES"][:, :ns]).abs(), True)]}
        if npth:
            hasL, hasU, gL, gU, cs = _row_parts(cb, pb)
            s, e1, e2 = T(pb["S"]), T(pb["E1"]), T(pb["E2"])
            phi["slacks"] = [(-(mu * gL.log()), hasL), (-(mu * gU.log()), hasU)]
            phi["elastics"] = [(rho * e1, True), (rho * e2, True), (-(mu * e1.log()), True), (-(mu * e2.log()), True)]
            inf["rows"] = [((T(cs) * T(pb["RES"][:, ns:]) - s - e1 + e2).abs(), True)]
        res.append(dict(phi=_sum(phi), infeas=_sum(inf)))
    return res


def accept_ref(c, trial, st, a_pr, a_du):
    """-> dict of T: the multipliers after the step (clamped); fixed variables keep ZL, ZU.  c = 2 for the update, the clamp bounds
    within 3 operations of the inputs"""
    nv, ns, npth = c["nv"], c["ns"], c["np"]
    mu = _par(c, 0)
    ap, ad = T(np.asarray(a_pr)[:, None, None]), T(np.asarray(a_du)[:, None, None])
    ks = 1e10

    def clamp(m, g, cond):
        hi, lo = ks * mu / g, mu / (ks * g)
        cl = where(m.v > hi.v, hi, where(m.v < lo.v, lo, m))
        return where(cond, cl, m)

    z, gm, gp, free, fL, fU = _var_parts(c, trial)
    out = {"LamF": T(c["LamF"]) + ap * T(st["DZLam"][:, nv:])}
    out["ZL"] = where(free, clamp(T(c["ZL"]) + ad * T(st["DZL"]), gm, fL), T(c["ZL"]))
    out["ZU"] = where(free, clamp(T(c["ZU"]) + ad * T(st["DZU"]), gp, fU), T(c["ZU"]))
    if npth:
        hasL, hasU, gL, gU, cs = _row_parts(c, trial)
        out["Y"] = T(c["Y"]) + ap * T(st["DY"])
        out["VL"] = clamp(T(c["VL"]) + ad * T(st["DVL"]), gL, hasL)
        out["VU"] = clamp(T(c["VU"]) + ad * T(st["DVU"]), gU, hasU)
        out["W1"] = clamp(T(c["W1"]) + ad * T(st["DW1"]), T(trial["E1"]), True)
        out["W2"] = clamp(T(c["W2"]) + ad * T(st["DW2"]), T(trial["E2"]), True)
    return out


def error_ref(c):
    """-> per instance: dict kkt (value, tol), viol, emax (value, tol), sumz, summ (sum dicts), cnt"""
    res = []
    ns, nv, npth, M = c["ns"], c["nv"], c["np"], c["M"]
    for b in range(c["B"]):
        cb = instance(c, b)
        mu, rho = _par(cb, 0), _par(cb, 1)
        z, gm, gp, free, fL, fU = _var_parts(cb, cb)
        zL, zU, G, lam = T(cb["ZL"]), T(cb["ZU"]), T(cb["G"]), T(cb["LamF"])
        sz = {"variables": [(zL, True), (zU, True)]}
        sm = {"defects": [(lam.abs(), True)]}
        cnt = int((zL.v > 0).sum() + (zU.v > 0).sum())
        ed = [((G - zL + zU).abs(), free)]                                                    # c = 2
        ep = [(T(cb["RES"][:, :ns]).abs(), True)]
        ec = [((gm * zL - mu).abs(), fL), ((gp * zU - mu).abs(), fU)]                         # c = 3
        em = []
        if npth:
            hasL, hasU, gL, gU, cs = _row_parts(cb, cb)
            s, e1, e2, y = T(cb["S"]), T(cb["E1"]), T(cb["E2"]), T(cb["Y"])
            vL, vU, w1, w2 = T(cb["VL"]), T(cb["VU"]), T(cb["W1"]), T(cb["W2"])
            sz["slacks"] = [(vL, True), (vU, True)]
            sz["elastics"] = [(w1, True), (w2, True)]
            sm["rows"] = [(y.abs(), True)]
            cnt += int((vL.v > 0).sum() + (vU.v > 0).sum()) + 2 * npth * M
            ed += [((-y - vL + vU).abs(), True), ((rho - y - w1).abs(), True), ((rho + y - w2).abs(), True)]
            ep.append(((T(cs) * T(cb["RES"][:, ns:]) - s - e1 + e2).abs(), True))             # c = 4
            ec += [((gL * vL - mu).abs(), hasL), ((gU * vU - mu).abs(), hasU), ((e1 * w1 - mu).abs(), True), ((e2 * w2 - mu).abs(), True)]
            em = [(e1, True), (e2, True)]
        sumz, summ = _sum(sz), _sum(sm)
        sd = max(100.0, (summ["value"] + sumz["value"]) / max(1, ns * M + npth * M + cnt)) / 100.0
        sc = max(100.0, sumz["value"] / max(1, cnt)) / 100.0
        # the scale sums' own summation error, relative, as it passes through the divisions (0 while the scale is the constant 1)
        rel_d = (summ["tol"] + sumz["tol"]) / (summ["value"] + sumz["value"]) if sd > 1.0 else 0.0
        rel_c = sumz["tol"] / sumz["value"] if sc > 1.0 else 0.0
        # ed, ep (= viol) and ec are maxima of RESIDUALS: G - zL + zU, c - s - e1 + e2, gap * multiplier - mu cancel their terms (that
        # is what a residual near a KKT point does), so their error is 4 eps of the terms, not of the value (see _ext)
        (edv, edt), (epv, ept), (ecv, ect) = _ext(ed, "max", 0.0, True), _ext(ep, "max", 0.0, True), _ext(ec, "max", 0.0, True)
        parts = [(edv / sd, edt / sd + (rel_d + 2 * EPS) * edv / sd), (epv, ept), (ecv / sc, ect / sc + (rel_c + 2 * EPS) * ecv / sc)]
        kkt = max(p[0] for p in parts)
        ktol = max(p[1] for p in parts if p[0] >= kkt * (1 - 1e-6))
        res.append(dict(kkt=(kkt, ktol), viol=(epv, ept), emax=_ext(em, "max", 0.0), sumz=sumz, summ=summ, cnt=cnt, sd=sd, sc=sc))
    return res


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def instance(c, b):
    """the case restricted to instance b (arrays keep a leading axis of 1)"""
    out = dict(c)
    out["B"] = 1
    for k, v in c.items():
        if isinstance(v, np.ndarray) and k not in ("cl", "cu", "cscale", "zl", "zu") and v.ndim >= 1 and v.shape[0] == c["B"]:
            out[k] = v[b:b + 1]
    for k in ("zl", "zu"):
        out[k] = c[k][b:b + 1] if c[k].shape[0] == c["B"] and c["nsets"] == c["B"] else c[k][:1]
    return out


def make_case(nv, ns, npth, M, B, nsets, seed, cscale=False, rs=False, soc=False, rows=None):
    rng = np.random.default_rng(seed)
    nc = nv - ns
    nvals = ns * nv + 2 * npth + nv
    c = dict(nv=nv, ns=ns, nc=nc, np=npth, M=M, B=B, nsets=nsets, nvals=nvals, model=MODEL_OF[(nv, ns)], seed=seed,
             rows=rows if rows is not None else default_rows(ns, nv, npth), custom_rows=rows is not None)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s)
    # variable bounds: kinds by variable -- both, lower only, upper only, none; states fixed at both end nodes (controls: free)
    zl, zu = np.empty((nsets, nv, M)), np.empty((nsets, nv, M))
    for v in range(nv):
        kind = v % 4
        lo, hi = u(-3, -1, nsets, M), u(1, 3, nsets, M)
        zl[:, v] = lo if kind in (0, 1) else -1e20
        zu[:, v] = hi if kind in (0, 2) else 1e20
    zl_b, zu_b = np.broadcast_to(zl, (B, nv, M)) if nsets == 1 else zl, np.broadcast_to(zu, (B, nv, M)) if nsets == 1 else zu
    t = u(0.1, 0.9, B, nv, M)
    z = np.where((zl_b > -INF) & (zu_b < INF), zl_b + t * (zu_b - zl_b),
                 np.where(zl_b > -INF, zl_b + 0.1 + 2 * t, np.where(zu_b < INF, zu_b - 0.1 - 2 * t, 4 * t - 2)))
    fx = np.zeros((nsets, nv, M), dtype=bool)
    fx[:, :ns, 0] = True                    # initial state
    fx[:, 0, M - 1] = True                  # one final state everywhere ...
    fx[nsets - 1, :ns, M - 1] = True        # ... and the whole final state in the last set
    val = u(-1, 1, nsets, nv, M)
    zl, zu = np.where(fx, val, zl), np.where(fx, val, zu)
    z = np.where(np.broadcast_to(fx, (B, nv, M)) if nsets == 1 else fx, np.broadcast_to(val, (B, nv, M)) if nsets == 1 else val, z)
    c.update(zl=zl, zu=zu, X=np.ascontiguousarray(z[:, :ns]), U=np.ascontiguousarray(z[:, ns:]))
    free = np.broadcast_to(zu > zl, (B, nv, M))
    hl, hu = np.broadcast_to(zl > -INF, (B, nv, M)), np.broadcast_to(zu < INF, (B, nv, M))
    c["ZL"], c["ZU"] = np.where(free & hl, u(0.1, 2, B, nv, M), 0.0), np.where(free & hu, u(0.1, 2, B, nv, M), 0.0)
    # path rows: lower only, upper only, both
    cl = np.array([[-0.5, -1e20, -1.0][j % 3] for j in range(npth)])
    cu = np.array([[1e20, 0.7, 1.5][j % 3] for j in range(npth)])
    c.update(cl=cl, cu=cu, cscale=np.array([0.5, 2.0, 3.0])[:npth] if cscale and npth else None)
    hasL, hasU, lo, hi, cs = row_bounds(c)
    t = u(0.1, 0.9, B, npth, M)
    lo3, hi3 = _r(lo), _r(hi)
    c["S"] = np.where(_r(hasL & hasU), lo3 + t * (hi3 - lo3), np.where(_r(hasL), lo3 + 0.1 + 2 * t, hi3 - 0.1 - 2 * t)) if npth else np.zeros((B, 0, M))
    c["E1"], c["E2"] = u(0.05, 1, B, npth, M), u(0.05, 1, B, npth, M)
    c["VL"], c["VU"] = np.where(_r(hasL), u(0.1, 2, B, npth, M), 0.0), np.where(_r(hasU), u(0.1, 2, B, npth, M), 0.0)
    c["W1"], c["W2"] = u(1, 12, B, npth, M), u(1, 12, B, npth, M)
    c["Y"], c["LamF"] = rng.standard_normal((B, npth, M)) * 2, rng.standard_normal((B, ns, M)) * 3
    # values "from the evaluator": defects, path values near their slacks (so that resets go both ways), partials, gradient, cost
    RES = rng.standard_normal((B, ns + npth, M)) * 0.3
    if npth:
        RES[:, ns:] = (c["S"] + c["E1"] - c["E2"] + rng.standard_normal((B, npth, M)) * 0.4) / _r(cs)
    c.update(RES=RES, VALS=rng.standard_normal((B, nvals, M)), G=rng.standard_normal((B, nv, M)) * 2, COST=rng.standard_normal(B) * 10)
    par = np.empty((B, 4))
    par[:, 0], par[:, 1], par[:, 2], par[:, 3] = u(0.2, 1.0, B), u(2, 6, B), u(0.9, 0.995, B), u(1, 10, B)
    c["par"] = par
    c["rs"] = u(0.2, 1.0, B, ns, M) if rs else None
    c["DefRes"] = rng.standard_normal((B, ns, M)) * 0.2 if soc else None
    c["RowRes"] = rng.standard_normal((B, npth, M)) * 0.2 if soc and npth else None
    c["DZLam"] = rng.standard_normal((B, nv + ns, M)) * 0.5          # "the solved step"
    c["alpha"], c["a_pr"], c["a_du"] = u(0.05, 0.5, B), u(0.2, 1.0, B), u(0.2, 1.0, B)
    return c


SHAPES = [(4, 2, 0), (4, 2, 3), (8, 6, 3), (16, 12, 0)]


def case_list():
    """(nv, ns, np, M, B, nsets, flag): every shape at M 5 / 33 / 257 with B and nsets dealt round, then the special cases"""
    keys = []
    i = 0
    for (nv, ns, npth) in SHAPES:
        for M in (5, 33, 257):
            B = (1, 3)[i % 2]
            nsets = B if (i // 2) % 2 else 1
            keys.append((nv, ns, npth, M, B, nsets, "plain"))
            i += 1
    keys += [(8, 6, 3, 33, 3, 3, "cscale"), (8, 6, 3, 33, 3, 1, "rs"), (4, 2, 3, 33, 3, 1, "soc"), (8, 6, 3, 33, 1, 1, "rows3"),
             (4, 2, 3, 257, 3, 3, "plain"), (16, 12, 0, 257, 1, 1, "plain")]
    return list(dict.fromkeys(keys))


_CACHE = {}


def get_case(key):
    if key not in _CACHE:
        nv, ns, npth, M, B, nsets, flag = key
        rows = None
        if flag == "rows3":         # three partials in the first row: its third on variable 2, through the VALS entry of df_0/dz_2
            rows = default_rows(ns, nv, npth)
            rows[0] = rows[0] + [(2, 2)]
        seed = 7000 + 131 * nv + 17 * npth + M + 1000 * B + nsets + sum(map(ord, flag))
        _CACHE[key] = make_case(nv, ns, npth, M, B, nsets, seed, cscale=flag == "cscale", rs=flag == "rs", soc=flag == "soc", rows=rows)
        _CACHE[key]["flag"] = flag
    return _CACHE[key]


def case_id(key):
    return "nv%d-np%d-M%d-B%d-sets%d-%s" % (key[0], key[2], key[3], key[4], key[5], key[6])


# ---- checks shared by the CPU test (host functions) and the GPU test (kernels) -------------------------------------------------------
def check_elementwise(name, got, ref, log=None):
    """|got - ref| <= c eps m everywhere; returns the worst ratio"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.v.shape, (name, got.shape, ref.v.shape)
    assert np.isfinite(got).all(), f"{name}: not finite (poison left?)"
    err = np.abs(np.asarray(got, dtype=LD) - ref.v)
    bound = ref.bound()
    exact = bound == 0
    assert (err[exact] == 0).all(), f"{name}: an exact value differs"
    ratio = float((err[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    if log:
        log(f"  {name:6s} max err / bound {ratio:.3f}  (c up to {int(ref.d.max())})")
    assert ratio <= 1.0, f"{name}: error {ratio:.3g} x its bound c eps sum|terms|"
    return ratio


def check_scalar(name, got, value, tol):
    assert np.isfinite(got), (name, got)
    assert abs(LD(got) - LD(value)) <= tol, f"{name}: {got!r} against {value!r}, tolerance {tol:.3g}"


def run_checks(c, be, log=None):
    """Every call of a backend `be` (the host functions through the shim, or the kernels) on the case, each stage against the
    reference on that stage's inputs.  be.reduce(c) -> dict; be.expand(c, el, dzlam) -> (step dict, scal [B][4]);
    be.trial(c, st, alpha) -> point dict or None; be.merit(c, pt, reset) -> (S after, out [B][2]);
    be.accept(c, trial, st, a_pr, a_du) -> dict of multipliers (and the point, if the backend moves it); be.error(c) -> out [B][3].
    Returns figures: the class shares of every sum, the reset rows exempted."""
    log = log or (lambda s: None)
    nv, ns, npth, B, M = c["nv"], c["ns"], c["np"], c["B"], c["M"]
    fig = dict(shares=[], reset_rows=0, reset_exempt=0, jumped=0)
    free = np.broadcast_to(c["zu"] > c["zl"], (B, nv, M))
    # reduce
    red = be.reduce(c)
    ref = reduce_ref(c)
    for k in ("Sigma", "Rhs") + (("SigS", "RhatS", "SigT", "Rt") if npth else ()):
        check_elementwise(k, red[k], ref[k], log)
    assert (red["Sigma"][~free] == 0).all() and (red["Rhs"][:, :nv][~free] == 0).all()
    # expand
    st, scal = be.expand(c, red, c["DZLam"].copy())
    ref = expand_ref(c, red, c["DZLam"])
    for k in ("DZLam", "DZL", "DZU") + (("DY", "DS", "DE1", "DE2", "DVL", "DVU", "DW1", "DW2") if npth else ()):
        check_elementwise(k, st[k], ref[k], log)
    assert (st["DZLam"][:, :nv][~free] == 0).all() and (st["DZL"][~free] == 0).all() and (st["DZU"][~free] == 0).all()
    sref = expand_scalars_ref(c, st)
    z = np.concatenate([c["X"], c["U"]], 1)
    hasL, hasU, lo, hi, cs = row_bounds(c)
    for b in range(B):
        r = sref[b]
        apr, adu, dphi, mmax = (float(x) for x in scal[b])
        check_scalar("apr", apr, *r["apr"]); check_scalar("adu", adu, *r["adu"]); check_scalar("mmax", mmax, *r["mmax"])
        check_scalar("dphi", dphi, r["dphi"]["value"], r["dphi"]["tol"])
        fig["shares"].append(("dphi", r["dphi"]["share"]))
        assert 0 < apr <= 1 and 0 < adu <= 1
        # the step to the boundary stays strictly inside; every multiplier stays positive
        zt = z[b] + apr * st["DZLam"][b, :nv]
        fb = free[b]
        assert (zt[fb] > np.broadcast_to(c["zl"], (B, nv, M))[b][fb]).all() and (zt[fb] < np.broadcast_to(c["zu"], (B, nv, M))[b][fb]).all()
        assert ((c["ZL"][b] + adu * st["DZL"][b])[fb & (c["ZL"][b] > 0)] > 0).all() and ((c["ZU"][b] + adu * st["DZU"][b])[fb & (c["ZU"][b] > 0)] > 0).all()
        if npth:
            s1 = c["S"][b] + apr * st["DS"][b]
            assert (s1 > np.where(hasL, lo, -np.inf)[:, None]).all() and (s1 < np.where(hasU, hi, np.inf)[:, None]).all()
            assert (c["E1"][b] + apr * st["DE1"][b] > 0).all() and (c["E2"][b] + apr * st["DE2"][b] > 0).all()
            for m, dm in (("VL", "DVL"), ("VU", "DVU"), ("W1", "DW1"), ("W2", "DW2")):
                assert ((c[m][b] + adu * st[dm][b])[c[m][b] > 0] > 0).all(), m
    # trial point
    alpha = c["alpha"] * scal[:, 0]
    tref = trial_ref(c, st, alpha)
    trial = be.trial(c, st, alpha)
    if trial is None:
        trial = {k: v.f64() for k, v in tref.items()}
    for k in tref:
        check_elementwise("t" + k, trial[k], tref[k], log)
    for k in POINT:
        trial.setdefault(k, np.zeros((B, 0, M)))
    # merit at the trial point (the evaluator's values there: the case's)
    pt = dict(trial, RES=c["RES"], COST=c["COST"])
    _, out = be.merit(c, pt, False)
    for b, r in enumerate(merit_ref(c, pt)):
        check_scalar("phi", float(out[b, 0]), r["phi"]["value"], r["phi"]["tol"])
        check_scalar("infeas", float(out[b, 1]), r["infeas"]["value"], r["infeas"]["tol"])
        fig["shares"] += [("phi", r["phi"]["share"]), ("infeas", r["infeas"]["share"])]
    if npth:
        S1, out = be.merit(c, pt, True)
        jump, margin, target, inside = reset_ref(c, pt)
        moved = S1 != pt["S"]
        close = np.abs(margin.v) <= margin.bound()
        fig["reset_rows"], fig["reset_exempt"], fig["jumped"] = int(moved.size), int(close.sum()), int(jump.sum())
        assert (moved == jump)[~close].all(), "the set of rows that jump differs from the reference's"
        assert (~moved | inside).all()
        if moved.any():
            check_elementwise("Sreset", S1[moved], target[moved], log)
        pt1 = dict(pt, S=S1)
        for b, r in enumerate(merit_ref(c, pt1)):
            check_scalar("phi (reset)", float(out[b, 0]), r["phi"]["value"], r["phi"]["tol"])
            check_scalar("infeas (reset)", float(out[b, 1]), r["infeas"]["value"], r["infeas"]["tol"])
    # accept
    a_pr, a_du = alpha, c["a_du"] * scal[:, 1]
    new = be.accept(c, trial, st, a_pr, a_du)
    aref = accept_ref(c, trial, st, a_pr, a_du)
    for k, r in aref.items():
        check_elementwise("a" + k, new[k], r, log)
        if k not in ("LamF", "Y"):
            assert (new[k][c[k] > 0] > 0).all(), k
    assert np.array_equal(new["ZL"][~free], c["ZL"][~free]) and np.array_equal(new["ZU"][~free], c["ZU"][~free])
    for k in POINT:
        if k in new:
            assert np.array_equal(new[k], trial[k]), k
    # kkt error
    out = be.error(c)
    for b, r in enumerate(error_ref(c)):
        check_scalar("kkt_error", float(out[b, 0]), *r["kkt"]); check_scalar("viol", float(out[b, 1]), *r["viol"]); check_scalar("emax", float(out[b, 2]), *r["emax"])
        fig["shares"] += [("sumz", r["sumz"]["share"]), ("summ", r["summ"]["share"])]
    return fig
