"""Reference side of the tests of the lock-step driver's residual-based acceptance and crawl rule (EMI_IPM_RULE_RESIDUAL).
TEST INFRASTRUCTURE: numpy + the harness.

  * the three rule functions of etol_amd/csrc/emi_ipm_control.hpp restated in Python floats, on the state dict of
    tests/lockstep_ref.py and a rescue dict {crawl, candidate, newton_steps, restored_steps, err_mu}: select(), decide(), crawl();
  * the same functions through the harness (tests/harness/etol_harness_rescue.cpp): the text emi_ipm_rescue_kernel runs;
  * the cases of the fixture tests/golden/lockstep_rescue_cases.json: the blocked instance (NO_PATH_DISC on the fixed start
    state) and the nine regular instances of tests/lockstep_ref.py per final time, under the device's rule set.
"""
import ctypes as C
import json
import math
import os

import numpy as np

import lockstep_ref as LR

ROOT = LR.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "lockstep_rescue_cases.json")
RULE_RESIDUAL = 1
RI = ("crawl", "candidate", "newton_steps", "restored_steps")
OPTIONS = dict(rules=RULE_RESIDUAL, crawl_limit=3, crawl_frac=0.3)
MAX_ITER = 200
RULE_OFF_CRAWL_LIMIT = 1 << 30      # solve_nlp has no switch for the err0 <= 1e-2 branch: beyond max_iter only that branch is left


def rescue_start():
    return dict(crawl=0, candidate=0, newton_steps=0, restored_steps=0, err_mu=0.0)


# ---- the rules ---------------------------------------------------------------------------------------------------------------------
def applies(s, r, o):
    if not (o["rules"] & RULE_RESIDUAL) or s["status"] != LR.RUNNING or not s["searching"] or s["passes"] != 1:
        return False
    return s["err0"] <= 1e-2 or r["crawl"] >= o["crawl_limit"]


def select(parts, s, r, o):
    """parts: dict of LR.PARTS at the present iterate; r in place"""
    r["candidate"] = 1 if applies(s, r, o) else 0
    if r["candidate"]:
        r["err_mu"] = LR.kkt(parts, s["mu"])
    return r["candidate"]


def decide(parts, s, r):
    """parts: dict of LR.PARTS at the stepped iterate; s, r in place; True = the step stands"""
    if not r["candidate"]:
        return False
    r["candidate"] = 0
    s["evaluations"] += 1
    err_tr = LR.kkt(parts, s["mu"])
    finite = math.isfinite(err_tr) and all(math.isfinite(parts[k]) for k in LR.PARTS)
    if finite and err_tr <= 0.9 * r["err_mu"]:
        s.update(searching=0, accepted=0, force_modified=0)
        s["iterations"] += 1
        r["crawl"] = 0
        r["newton_steps"] += 1
        return True
    r["restored_steps"] += 1
    return False


def crawl(scal, s, r, o):
    if not (o["rules"] & RULE_RESIDUAL) or not s["accepted"]:
        return
    r["crawl"] = r["crawl"] + 1 if s["alpha"] < o["crawl_frac"] * float(scal[0]) else 0


# ---- the same rules through the harness -----------------------------------------------------------------------------------------------
def load_harness():
    h = LR.load_harness()
    D_, I_ = LR.D_, LR.I_
    h.harness_rescue_sizes.argtypes = [I_, I_, I_]
    h.harness_rescue_select.argtypes = [D_, D_, I_, I_, D_, C.c_int, C.c_int, C.c_double]
    h.harness_rescue_decide.argtypes = [D_, D_, I_, I_, D_]
    h.harness_rescue_crawl.argtypes, h.harness_rescue_crawl.restype = [D_, D_, I_, I_, D_, C.c_int, C.c_int, C.c_double], None
    h.harness_rescue_solve_oracle.argtypes = [C.c_char_p, C.c_int, C.c_double, D_, C.c_int, D_, D_, D_, D_, D_, C.c_double, C.c_int, C.c_int,
                                              C.c_double, C.c_int, D_, I_]
    nd, ni, nr = C.c_int(), C.c_int(), C.c_int()
    assert h.harness_rescue_sizes(C.byref(nd), C.byref(ni), C.byref(nr)) == RULE_RESIDUAL
    assert (nd.value, ni.value, nr.value) == (len(LR.SD), len(LR.SI), len(RI))
    return h


class HostRescue:
    """the functions of emi_ipm_control.hpp behind the signatures of the Python restatement"""

    def __init__(self, h):
        self.h = h

    @staticmethod
    def _parts(p):
        return np.array([p[k] for k in LR.PARTS], dtype=np.float64)

    @staticmethod
    def _pack(r):
        return np.array([r[k] for k in RI], dtype=np.int32), np.array([r["err_mu"]], dtype=np.float64)

    @staticmethod
    def _unpack(r, ri, em):
        r.update({k: int(v) for k, v in zip(RI, ri)})
        r["err_mu"] = float(em[0])

    def select(self, parts, s, r, o):
        a, (d, i), (ri, em) = self._parts(parts), LR.HostRules._pack(s), self._pack(r)
        out = self.h.harness_rescue_select(a.ctypes.data_as(LR.D_), d.ctypes.data_as(LR.D_), i.ctypes.data_as(LR.I_), ri.ctypes.data_as(LR.I_),
                                           em.ctypes.data_as(LR.D_), o["rules"], o["crawl_limit"], o["crawl_frac"])
        self._unpack(r, ri, em)
        return out

    def decide(self, parts, s, r):
        a, (d, i), (ri, em) = self._parts(parts), LR.HostRules._pack(s), self._pack(r)
        out = self.h.harness_rescue_decide(a.ctypes.data_as(LR.D_), d.ctypes.data_as(LR.D_), i.ctypes.data_as(LR.I_), ri.ctypes.data_as(LR.I_),
                                           em.ctypes.data_as(LR.D_))
        LR.HostRules._unpack(s, d, i)
        self._unpack(r, ri, em)
        return bool(out)

    def crawl(self, scal, s, r, o):
        sc, (d, i), (ri, em) = np.array(scal, dtype=np.float64), LR.HostRules._pack(s), self._pack(r)
        self.h.harness_rescue_crawl(sc.ctypes.data_as(LR.D_), d.ctypes.data_as(LR.D_), i.ctypes.data_as(LR.I_), ri.ctypes.data_as(LR.I_),
                                    em.ctypes.data_as(LR.D_), o["rules"], o["crawl_limit"], o["crawl_frac"])
        self._unpack(r, ri, em)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def blocked_instance(tf):
    """NO_PATH_DISC on the fixed start state, from the straight-line start of the first regular instance"""
    return dict(discs=LR.discs_of(LR.NO_PATH_DISC), bump=0.0, z0=LR.instances(tf)[0]["z0"])


def solve_oracle(h, tf, inst, crawl_limit, crawl_frac=0.3, soc=False, tol=1e-8, max_iter=MAX_ITER):
    """solve_nlp on the CPU oracle under the device's rule set -> dict of what the fixture records"""
    P = LR.quad(tf, inst["discs"])
    recs = np.ascontiguousarray(LR.records(inst["discs"]))
    dp = lambda a: a.ctypes.data_as(LR.D_)
    prm, cs = np.array(LR.QUAD_PARAMS), np.ascontiguousarray(LR.CSCALE)
    zl, zu, z0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (P.lo, P.up, inst["z0"]))
    out_d, out_i = np.zeros(4), np.zeros(7, dtype=np.int32)
    rc = h.harness_rescue_solve_oracle(os.path.join(ROOT, "oracle", "liboracle.so").encode(), P.M, tf, dp(prm), recs.shape[0], dp(recs), dp(cs),
                                       dp(zl), dp(zu), dp(z0), tol, max_iter, int(crawl_limit), float(crawl_frac), int(soc), dp(out_d),
                                       out_i.ctypes.data_as(LR.I_))
    assert rc == 0, rc
    status = "converged" if out_i[0] else "locally infeasible" if out_i[5] else "max_iter" if out_i[6] else "other"
    return dict(status=status, iterations=int(out_i[1]), evaluations=int(out_i[2]), newton_steps=int(out_i[3]), restored_steps=int(out_i[4]),
                cost=float(out_d[0]), rho=float(out_d[1]), kkt_error=float(out_d[2]), constr_viol=float(out_d[3]))


def fixture():
    return json.load(open(FIXTURE))
