"""Reference side of the lock-step interior-point driver's tests (emi_ipm_solve_shard_*).  TEST INFRASTRUCTURE: numpy + the harness.

  * the scalar control rules of etol_amd/csrc/emi_ipm_control.hpp restated in Python floats (IEEE doubles, one rounding per
    operation, math.sqrt correctly rounded): barrier(), search_init(), search_step(), raise_dc(), kkt();
  * the components of the scaled KKT error in numpy, with bounds from the number format (error_parts_ref);
  * start()'s formulas in numpy (start_ref): exact operations or single rounded ones, so the kernel's bits are these;
  * the cases of the fixture tests/golden/lockstep_cases.json: the 41-node quadrotor of indep_nlp.quad_problem with nine
    (two discs, start) combinations per final time.
"""
import ctypes as C
import json
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "lockstep_cases.json")
EPS = np.finfo(np.float64).eps
INF = 1e19
RUNNING = -1
CONVERGED, ACCEPTABLE, MAX_ITER, LINE_SEARCH, INFEASIBLE, FACTOR, NOT_FINITE = range(7)

# the state record as the harness passes it (tests/harness/etol_harness_lockstep.cpp)
SD = ("mu", "rho", "tau", "nu", "emax_ref", "err0", "viol", "emax", "phi0", "slope", "alpha", "adu")
SI = ("n_acceptable", "futile", "iterations", "status", "force_modified", "escalated", "searching", "accepted", "passes", "evaluations")
PARTS = ("ed", "sd", "ep", "sc", "pmin", "pmax", "emax", "ymax")
DEFAULTS = dict(tol=1e-8, acceptable_factor=100.0, max_iter=200, acceptable_iter=10, max_futile_escalations=3, has_rows=1)


# ---- the control rules ------------------------------------------------------------------------------------------------------------
def start(mu_init=0.1, rho_init=10.0):
    s = {k: 0.0 for k in SD}
    s.update({k: 0 for k in SI})
    s.update(mu=mu_init, rho=rho_init, nu=1.0, emax_ref=1e300, status=RUNNING)
    return s


def _max(a, b):
    return a if a > b else b        # (a NaN in `a` is dropped, one in `b` is kept: the comparison the header writes)


def kkt(p, mu_t):
    ec = _max(0.0, _max(p["pmax"] - mu_t, mu_t - p["pmin"]))
    return _max(_max(p["ed"] / p["sd"], p["ep"]), ec / p["sc"])


def _acceptable(s, o):
    return s["err0"] <= o["acceptable_factor"] * o["tol"] and (not o["has_rows"] or s["emax"] <= 1e-6)


def _futile(s, o, emax):
    if s["rho"] < 1e5:
        return False
    if emax < 0.5 * s["emax_ref"]:
        s["emax_ref"], s["futile"] = emax, 0
        return False
    s["futile"] += 1
    return s["futile"] >= o["max_futile_escalations"]


def _escalate(s):
    s["rho"] *= 10.0
    s["mu"] = max(s["mu"], 1e-2)
    s["escalated"] = 1


def barrier(p, s, o):
    """solve_nlp's test_and_update_barrier on the error components p (dict of PARTS); s in place"""
    s["escalated"] = 0
    if s["status"] != RUNNING:
        return
    s["evaluations"] += 1
    err0, emax = kkt(p, 0.0), p["emax"]
    s.update(err0=err0, viol=p["ep"], emax=emax)
    if not (math.isfinite(err0) and all(math.isfinite(p[k]) for k in PARTS)):
        s["status"] = NOT_FINITE
        return
    if err0 <= o["tol"]:
        if emax <= max(o["tol"], 1e-9) * 10.0 or not o["has_rows"]:
            s["status"] = CONVERGED
            return
        if s["rho"] >= 1e12 or _futile(s, o, emax):
            s["status"] = INFEASIBLE
            return
        _escalate(s)
    if _acceptable(s, o):
        s["n_acceptable"] += 1
        if s["n_acceptable"] >= o["acceptable_iter"]:
            s["status"] = ACCEPTABLE
            return
    else:
        s["n_acceptable"] = 0
    if s["iterations"] >= o["max_iter"]:
        s["status"] = MAX_ITER
        return
    while not s["escalated"] and s["mu"] > o["tol"] / 10.0 and kkt(p, s["mu"]) <= 10.0 * s["mu"]:
        if o["has_rows"] and (emax > max(1e-6, 100.0 * s["mu"]) or p["ymax"] > 0.9 * s["rho"]) and s["rho"] < 1e12:
            if _futile(s, o, emax):
                s["status"] = INFEASIBLE
                return
            _escalate(s)
            s["nu"] = 1.0
            break
        s["mu"] = max(o["tol"] / 10.0, min(0.2 * s["mu"], s["mu"] * math.sqrt(s["mu"])))
        s["nu"] = 1.0
    s["tau"] = max(0.99, 1.0 - s["mu"])


def raise_dc(dc, mu):
    return 1e-8 * math.sqrt(math.sqrt(mu)) if dc == 0.0 else dc * 100.0


def search_init(scal, mer, factor_failed, s):
    s["searching"] = s["accepted"] = s["passes"] = 0
    if s["status"] != RUNNING:
        return
    if factor_failed:
        s["status"] = FACTOR
        return
    apr, adu, dphi, mmax = (float(v) for v in scal)
    phi_b, infeas0 = float(mer[0]), float(mer[1])
    nu_want = max(1.0, min(1.1 * mmax, 1e8))
    if infeas0 > 0:
        nu_want = max(nu_want, dphi / (0.9 * infeas0) + 1.0)
    s["nu"] = max(nu_want, 0.5 * s["nu"])
    pen = s["nu"] * infeas0
    s.update(phi0=phi_b + pen, slope=dphi - pen, alpha=apr, adu=adu, searching=1)


def search_step(mer, exact_with_mods, s, o):
    if s["status"] != RUNNING or not s["searching"]:
        return
    s["evaluations"] += 1
    phi = float(mer[0]) + s["nu"] * float(mer[1])
    if math.isfinite(phi) and phi <= s["phi0"] + 1e-4 * s["alpha"] * min(s["slope"], 0.0) + 1e-13 * abs(s["phi0"]):
        s.update(accepted=1, searching=0, force_modified=0)
        s["iterations"] += 1
        return
    s["passes"] += 1
    if s["passes"] < 40:
        s["alpha"] *= 0.5
        return
    s["searching"] = 0
    if exact_with_mods and not s["force_modified"]:
        s["force_modified"] = 1
        s["iterations"] += 1
        return
    s["force_modified"] = 0
    s["status"] = ACCEPTABLE if _acceptable(s, o) else LINE_SEARCH


# ---- the same rules through the harness (the text the kernels run) --------------------------------------------------------------------
D_ = C.POINTER(C.c_double)
I_ = C.POINTER(C.c_int)


def load_harness():
    h = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    h.harness_ctl_sizes.argtypes = [I_, I_, I_]
    h.harness_ctl_start.argtypes = [C.c_double, C.c_double, D_, I_]
    h.harness_ctl_start.restype = None
    h.harness_ctl_kkt.argtypes, h.harness_ctl_kkt.restype = [D_, C.c_double], C.c_double
    h.harness_ctl_raise_dc.argtypes, h.harness_ctl_raise_dc.restype = [C.c_double, C.c_double], C.c_double
    h.harness_ctl_barrier.argtypes, h.harness_ctl_barrier.restype = [D_, D_, I_, D_, I_], None
    h.harness_ctl_search_init.argtypes, h.harness_ctl_search_init.restype = [D_, D_, C.c_int, D_, I_], None
    h.harness_ctl_search_step.argtypes, h.harness_ctl_search_step.restype = [D_, C.c_int, D_, I_, D_, I_], None
    h.harness_lockstep_solve_oracle.argtypes = [C.c_char_p, C.c_int, C.c_double, D_, C.c_int, D_, D_, D_, D_, D_, C.c_double, C.c_int, D_, I_, D_]
    nd, ni, npar = C.c_int(), C.c_int(), C.c_int()
    assert h.harness_ctl_sizes(C.byref(nd), C.byref(ni), C.byref(npar)) == RUNNING
    assert (nd.value, ni.value, npar.value) == (len(SD), len(SI), len(PARTS))
    return h


class HostRules:
    """the functions of emi_ipm_control.hpp behind the signatures of the Python restatement"""

    def __init__(self, h):
        self.h = h

    @staticmethod
    def _pack(s):
        return np.array([s[k] for k in SD], dtype=np.float64), np.array([s[k] for k in SI], dtype=np.int32)

    @staticmethod
    def _unpack(s, d, i):
        s.update({k: float(v) for k, v in zip(SD, d)})
        s.update({k: int(v) for k, v in zip(SI, i)})

    @staticmethod
    def _opt(o):
        return (np.array([o["tol"], o["acceptable_factor"]], dtype=np.float64),
                np.array([o["max_iter"], o["acceptable_iter"], o["max_futile_escalations"], o["has_rows"]], dtype=np.int32))

    def start(self, mu_init=0.1, rho_init=10.0):
        d, i = np.zeros(len(SD)), np.zeros(len(SI), dtype=np.int32)
        self.h.harness_ctl_start(mu_init, rho_init, d.ctypes.data_as(D_), i.ctypes.data_as(I_))
        s = {}
        self._unpack(s, d, i)
        return s

    def kkt(self, p, mu_t):
        a = np.array([p[k] for k in PARTS], dtype=np.float64)
        return self.h.harness_ctl_kkt(a.ctypes.data_as(D_), mu_t)

    def raise_dc(self, dc, mu):
        return self.h.harness_ctl_raise_dc(dc, mu)

    def barrier(self, p, s, o):
        a = np.array([p[k] for k in PARTS], dtype=np.float64)
        d, i = self._pack(s)
        od, oi = self._opt(o)
        self.h.harness_ctl_barrier(a.ctypes.data_as(D_), d.ctypes.data_as(D_), i.ctypes.data_as(I_), od.ctypes.data_as(D_), oi.ctypes.data_as(I_))
        self._unpack(s, d, i)

    def search_init(self, scal, mer, factor_failed, s):
        sc, me = np.array(scal, dtype=np.float64), np.array(mer, dtype=np.float64)
        d, i = self._pack(s)
        self.h.harness_ctl_search_init(sc.ctypes.data_as(D_), me.ctypes.data_as(D_), int(factor_failed), d.ctypes.data_as(D_), i.ctypes.data_as(I_))
        self._unpack(s, d, i)

    def search_step(self, mer, exact_with_mods, s, o):
        me = np.array(mer, dtype=np.float64)
        d, i = self._pack(s)
        od, oi = self._opt(o)
        self.h.harness_ctl_search_step(me.ctypes.data_as(D_), int(exact_with_mods), d.ctypes.data_as(D_), i.ctypes.data_as(I_),
                                       od.ctypes.data_as(D_), oi.ctypes.data_as(I_))
        self._unpack(s, d, i)


# ---- components of the KKT error in numpy ------------------------------------------------------------------------------------------
def error_parts_ref(c):
    """per instance of an ipm_ref case: (parts, tol), dicts keyed by PARTS.  Bounds from the format: a maximum of |residual| of up to
    four rounded operations (a product may be fused into the sum that follows it) is within 4 eps of the largest sum of its terms'
    magnitudes; a product of a rounded gap is within 4 eps of itself; emax and ymax are exact; the scale sums of n terms are within
    n eps of the sum of the magnitudes, passed through the divisions."""
    ns, nv, npth, M = c["ns"], c["nv"], c["np"], c["M"]
    out = []
    for b in range(c["B"]):
        st = b if c["nsets"] == c["B"] and c["B"] > 1 else 0
        z = np.concatenate([c["X"][b], c["U"][b]], 0)
        zl, zu = c["zl"][st], c["zu"][st]
        free = zu > zl
        hasL, hasU = free & (zl > -INF), free & (zu < INF)
        zL, zU, G, lam = c["ZL"][b], c["ZU"][b], c["G"][b], c["LamF"][b]
        rho = c["par"][b, 1]
        sumz, summ, cnt = zL.sum() + zU.sum(), np.abs(lam).sum(), int((zL > 0).sum() + (zU > 0).sum())
        nterms = 2 * zL.size + lam.size
        ed = np.abs(G - zL + zU)[free].max(initial=0.0)
        edm = (np.abs(G) + np.abs(zL) + np.abs(zU))[free].max(initial=0.0)
        RES = c["RES"][b]
        ep = np.abs(RES[:ns]).max(initial=0.0)
        epm = 0.0
        prods = [((z - zl) * zL)[hasL], ((zu - z) * zU)[hasU]]
        emax = ymax = 0.0
        if npth:
            cs = np.ones(npth) if c.get("cscale") is None else np.asarray(c["cscale"], dtype=float)
            s, e1, e2, y = c["S"][b], c["E1"][b], c["E2"][b], c["Y"][b]
            vL, vU, w1, w2 = c["VL"][b], c["VU"][b], c["W1"][b], c["W2"][b]
            rL, rU = c["cl"] > -INF, c["cu"] < INF
            lo, hi = np.where(rL, cs * c["cl"], c["cl"])[:, None], np.where(rU, cs * c["cu"], c["cu"])[:, None]
            sumz += (vL + vU + w1 + w2).sum()
            summ += np.abs(y).sum()
            cnt += int((vL > 0).sum() + (vU > 0).sum()) + 2 * npth * M
            nterms += 5 * y.size
            ed = max(ed, np.abs(-y - vL + vU).max(), np.abs(rho - y - w1).max(), np.abs(rho + y - w2).max())
            edm = max(edm, (np.abs(y) + vL + vU).max(), (rho + np.abs(y) + w1).max(), (rho + np.abs(y) + w2).max())
            cv = cs[:, None] * RES[ns:]
            ep = max(ep, np.abs(cv - s - e1 + e2).max())
            epm = (np.abs(cv) + np.abs(s) + e1 + e2).max()
            emax, ymax = max(e1.max(), e2.max()), np.abs(y).max()
            prods += [((s - lo) * vL)[rL], ((hi - s) * vU)[rU], (e1 * w1).ravel(), (e2 * w2).ravel()]
        prods = np.concatenate([p.ravel() for p in prods])
        pmin, pmax = (prods.min(), prods.max()) if prods.size else (1e300, -1e300)
        sd = max(100.0, (summ + sumz) / max(1, ns * M + npth * M + cnt)) / 100.0
        sc = max(100.0, sumz / max(1, cnt)) / 100.0
        rel = (nterms + 4) * EPS          # every term of the scale sums is a magnitude: relative error of a sum of n terms
        parts = dict(ed=float(ed), sd=float(sd), ep=float(ep), sc=float(sc), pmin=float(pmin), pmax=float(pmax), emax=float(emax), ymax=float(ymax))
        tol = dict(ed=4 * EPS * edm, sd=rel * sd, ep=4 * EPS * epm, sc=rel * sc, pmin=4 * EPS * abs(pmin), pmax=4 * EPS * abs(pmax), emax=0.0,
                   ymax=0.0)
        out.append((parts, tol))
    return out


# ---- start() in numpy ----------------------------------------------------------------------------------------------------------------
def pushed_inside(v, l, u, hasL, hasU, push=1e-2, frac=1e-2):
    with np.errstate(invalid="ignore", over="ignore"):
        pl = np.where(hasL, push * np.maximum(1.0, np.abs(l)), 0.0)
        pu = np.where(hasU, push * np.maximum(1.0, np.abs(u)), 0.0)
        both = hasL & hasU
        pl = np.where(both, np.minimum(pl, frac * (u - l)), pl)
        pu = np.where(both, np.minimum(pu, frac * (u - l)), pu)
        v = np.where(hasL, np.maximum(v, l + pl), v)
        v = np.where(hasU, np.minimum(v, u - pu), v)
    return v


def start_point_ref(z, zl, zu, push=1e-2, frac=1e-2):
    """z, zl, zu [B][nv][M] -> (pushed z, fixed bytes)"""
    fixed = ~(zu > zl)
    zp = pushed_inside(z, zl, zu, zl > -INF, zu < INF, push, frac)
    return np.where(fixed, zl, zp), fixed.astype(np.uint8)


def start_rows_ref(cpath, zl, zu, cl, cu, cscale, rho, push=1e-2, frac=1e-2):
    """cpath [B][np][M] path values of the first evaluation (caller's units) -> dict S E1 E2 Y VL VU W1 W2 ZL ZU"""
    cs = np.asarray(cscale, dtype=float)[None, :, None]
    rL, rU = (cl > -INF)[None, :, None], (cu < INF)[None, :, None]
    lo = np.where(cl > -INF, cscale * cl, cl)[None, :, None]
    hi = np.where(cu < INF, cscale * cu, cu)[None, :, None]
    c0 = cs * cpath
    rL, rU = np.broadcast_to(rL, c0.shape), np.broadcast_to(rU, c0.shape)
    s = pushed_inside(c0, np.broadcast_to(lo, c0.shape), np.broadcast_to(hi, c0.shape), rL, rU, push, frac)
    gap = c0 - s
    ee = push * np.maximum(1.0, np.abs(gap))
    free = zu > zl
    one = np.ones_like(c0)
    return dict(S=s, E1=np.maximum(gap, 0.0) + ee, E2=np.maximum(-gap, 0.0) + ee, Y=0.0 * one, VL=np.where(rL, 1.0, 0.0), VU=np.where(rU, 1.0, 0.0),
                W1=np.maximum(1e-8, rho) * one, W2=np.maximum(1e-8, rho) * one,
                ZL=np.where(free & (zl > -INF), 1.0, 0.0), ZU=np.where(free & (zu < INF), 1.0, 0.0))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
M_NODES = 41
TFS = (4.0, 2.5)
FIRST_DISCS = ((4.0, 3.2, 0.8), (4.3, 3.0, 0.7), (3.8, 3.5, 0.9))
BUMPS = (0.0, 1.5, -1.5)
QUAD_PARAMS = [1.0, 0.01, 9.81, 1.0, 1.0]
CL, CU = np.array([-1000.0, -1000.0]), np.array([0.0, 0.0])
# the rows are iterated on unscaled: the bounds struct holds ONE set of row scales and the discs differ per instance
CSCALE = np.ones(2)
NO_PATH_DISC = (1.0, 1.0, 0.5)       # on the fixed start state: no feasible path


def discs_of(first):
    cx, cy, r = first
    return (first, (cx + 2.3, cy + 1.2, r - 0.1))


def records(discs):
    recs = np.zeros((len(discs), 8))
    for j, (x, y, r) in enumerate(discs):
        recs[j, :4] = [1, x, y, r * r]          # PATH_DISC
    return recs


def quad(tf, discs=None):
    """indep_nlp.quad_problem at another final time / with other discs"""
    import indep_nlp as N
    P = N.quad_problem()
    return N.Nlp(1, QUAD_PARAMS, M_NODES, 0.0, tf, records(discs) if discs is not None else P.recs, None, x0=[1, 1, 0, 0, 0, 0],
                 xf=[8, 6, 0, 0, 0, 0], xtol=[0.01, 0.01, 0.01, 0.05, 0.05, 0.05], xlo=[0, 0, -1.2, -6, -6, -4], xup=[10, 10, 1.2, 6, 6, 4],
                 ulo=[0, -1], uup=[25, 1])


def instances(tf):
    """the nine instances of a final time, in instance order (bump outer, disc inner): list of dict discs, bump, z0"""
    import indep_nlp as N
    P = quad(tf)
    z0s = N.starts(P, BUMPS)
    return [dict(discs=discs_of(first), bump=bump, z0=z0) for bump, z0 in zip(BUMPS, z0s) for first in FIRST_DISCS]


def fixture():
    return json.load(open(FIXTURE))
