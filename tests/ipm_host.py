"""The host functions of the interior-point arithmetic (mi355x::ipm_*) behind the interface tests/ipm_ref.run_checks drives,
through tests/harness/etol_harness_ipm.cpp.  Shared by tests/test_ipm_cpu.py and tools/ipm_times.py."""
import ctypes as C
import os

import numpy as np

import ipm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ = C.POINTER(C.c_double)
I_ = C.POINTER(C.c_int)
SLOTS = ("Z", "S", "E1", "E2", "LamF", "Y", "ZL", "ZU", "VL", "VU", "W1", "W2", "RES", "VALS", "G", "DefRes", "RowRes", "rs", "Sigma", "SigT",
         "SigS", "RhatS", "Rt", "Rhs", "DZLam", "DS", "DY", "DE1", "DE2", "DZL", "DZU", "DVL", "DVU", "DW1", "DW2", "OUT")




def load_harness():
    h = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    h.harness_ipm_problem.restype = None
    h.harness_ipm_problem.argtypes = [C.c_int] * 5 + [D_] * 5 + [I_] * 3
    h.harness_ipm.restype = C.c_int
    h.harness_ipm.argtypes = [C.c_int, C.POINTER(D_), D_, C.c_int]
    h.harness_ipm_timed.restype = C.c_int
    h.harness_ipm_timed.argtypes = [C.c_int, C.POINTER(D_), D_, C.c_int, C.c_int, D_]
    assert h.harness_ipm_nslots() == len(SLOTS)
    return h


class HostBackend:
    """the host functions, instance by instance"""

    def __init__(self, h, reps=1):
        self.h, self.reps, self.seconds = h, reps, 0.0

    def _problem(self, c, b):
        ptr, var, ent = [0], [], []
        for row in c["rows"]:
            var += [v for v, _ in row]; ent += [e for _, e in row]; ptr.append(len(var))
        ia = lambda a: np.asarray(a + [0], dtype=np.int32)
        ptr, var, ent = ia(ptr)[:-1], ia(var), ia(ent)
        s = b if c["nsets"] == c["B"] and c["B"] > 1 else 0
        zl, zu = np.ascontiguousarray(c["zl"][s]), np.ascontiguousarray(c["zu"][s])
        cl, cu = np.ascontiguousarray(np.append(c["cl"], 0.0)), np.ascontiguousarray(np.append(c["cu"], 0.0))
        cs = np.ascontiguousarray(c["cscale"]) if c.get("cscale") is not None else None
        dp = lambda a: a.ctypes.data_as(D_)
        ip = lambda a: a.ctypes.data_as(I_)
        self.h.harness_ipm_problem(c["nv"], c["ns"], c["np"], c["M"], c["nvals"], dp(zl), dp(zu), dp(cl), dp(cu), dp(cs) if cs is not None else None,
                                   ip(ptr), ip(var), ip(ent))

    def _call(self, what, c, b, arrays, scal=(), reset=0):
        """arrays: slot name -> numpy array of instance b (contiguous, written in place)"""
        self._problem(c, b)
        tab = (D_ * len(SLOTS))()
        for i, n in enumerate(SLOTS):
            a = arrays.get(n)
            tab[i] = a.ctypes.data_as(D_) if a is not None and a.size else None
        sc = np.zeros(7)
        sc[:4] = c["par"][b]
        for i, v in scal:
            sc[i] = v
        if self.reps > 1:           # timed repetitions of the ipm_* calls alone (tools/ipm_times.py)
            sec = C.c_double()
            assert self.h.harness_ipm_timed(what, tab, sc.ctypes.data_as(D_), reset, self.reps, C.byref(sec)) == 0
            self.seconds += sec.value
        else:
            assert self.h.harness_ipm(what, tab, sc.ctypes.data_as(D_), reset) == 0

    @staticmethod
    def _inst(c, b, names, src=None):
        src = src or c
        out = {}
        for n in names:
            if n == "Z":
                out[n] = np.ascontiguousarray(np.concatenate([src["X"][b], src["U"][b]], 0))
            elif src.get(n) is not None:
                out[n] = np.ascontiguousarray(src[n][b]).copy()
        return out

    def reduce(self, c):
        names = ("Sigma", "SigT", "SigS", "RhatS", "Rt", "Rhs")
        shp = dict(Sigma=c["nv"], Rhs=c["nv"] + c["ns"])
        res = {n: np.full((c["B"], shp.get(n, c["np"]), c["M"]), np.nan) for n in names}
        for b in range(c["B"]):
            a = self._inst(c, b, SLOTS[:18])
            a.update({n: res[n][b] for n in names})
            self._call(0, c, b, a)
        return res

    def expand(self, c, el, dzlam):
        names = R.STEP[1:]
        st = {n: np.full((c["B"], c["nv"] if n in ("DZL", "DZU") else c["np"], c["M"]), np.nan) for n in names}
        st["DZLam"] = dzlam
        scal = np.full((c["B"], 4), np.nan)
        for b in range(c["B"]):
            a = self._inst(c, b, SLOTS[:18])
            a.update({n: np.ascontiguousarray(el[n][b]) for n in ("SigT", "SigS", "RhatS", "Rt")})
            a.update({n: st[n][b] for n in R.STEP})
            a["OUT"] = scal[b]
            self._call(1, c, b, a)
        return st, scal

    def trial(self, c, st, alpha):
        return None         # (a plain loop inside solve_nlp: no function of its own)

    def merit(self, c, pt, reset):
        S = pt["S"].copy()
        out = np.full((c["B"], 2), np.nan)
        for b in range(c["B"]):
            a = self._inst(c, b, ("Z", "E1", "E2", "RES"), pt)
            a.update(S=S[b], OUT=out[b])
            if c.get("rs") is not None:
                a["rs"] = np.ascontiguousarray(c["rs"][b])
            self._call(2, c, b, a, scal=[(4, pt["COST"][b])], reset=int(reset))
        return S, out

    def accept(self, c, trial, st, a_pr, a_du):
        new = {n: c[n].copy() for n in R.DUALS}
        for b in range(c["B"]):
            a = self._inst(c, b, ("Z", "S", "E1", "E2"), trial)
            a.update({n: new[n][b] for n in R.DUALS})
            a.update({n: np.ascontiguousarray(st[n][b]) for n in R.STEP})
            self._call(3, c, b, a, scal=[(5, a_pr[b]), (6, a_du[b])])
        return new

    def error(self, c):
        out = np.full((c["B"], 3), np.nan)
        for b in range(c["B"]):
            a = self._inst(c, b, SLOTS[:15])
            a["OUT"] = out[b]
            self._call(4, c, b, a)
        return out
