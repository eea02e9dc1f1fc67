"""Reference side of the tests of the per-instance parameter table (emi_set_model_params_batch).  TEST INFRASTRUCTURE: numpy + the
harness.

  * the lock-step cases of the fixture tests/golden/param_table_cases.json: instances 0, 4, 8 of lockstep_ref.instances(4.0) --
    their discs, their starts unchanged -- each with its own row of quadrotor parameters {mass, inertia, gravity, w_thrust,
    w_torque};
  * solve_oracle: solve_nlp on the CPU oracle through harness_rescue_solve_oracle, which takes the parameter set, under the
    device's rule set with the crawl rule out of reach;
  * rows_for: seeded parameter rows around a model's nominal set, for the evaluation tests.
"""
import json
import os

import numpy as np

import lockstep_ref as LR
import lockstep_rescue_ref as RR

ROOT = LR.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "param_table_cases.json")
TF = 4.0
INSTANCES = (0, 4, 8)
ROWS = ((0.8, 0.008, 9.81, 1.0, 1.0), (1.0, 0.01, 9.81, 1.0, 1.0), (1.25, 0.02, 9.81, 2.0, 0.5))
TOL, MAX_ITER = 1e-8, RR.MAX_ITER


def cases():
    """the three (instance, row) pairs: list of dict instance, row, inst (discs, bump, z0), params"""
    insts = LR.instances(TF)
    return [dict(instance=i, row=r, inst=insts[i], params=list(ROWS[r])) for r, i in enumerate(INSTANCES)]


def solve_oracle(h, inst, params, tf=TF, tol=TOL, max_iter=MAX_ITER):
    """lockstep_rescue_ref.solve_oracle with another parameter set: device rule set, crawl rule out of reach -> what the fixture records"""
    P = LR.quad(tf, inst["discs"])
    recs = np.ascontiguousarray(LR.records(inst["discs"]))
    dp = lambda a: a.ctypes.data_as(LR.D_)
    prm, cs = np.array(params, dtype=np.float64), np.ascontiguousarray(LR.CSCALE)
    zl, zu, z0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (P.lo, P.up, inst["z0"]))
    out_d, out_i = np.zeros(4), np.zeros(7, dtype=np.int32)
    rc = h.harness_rescue_solve_oracle(os.path.join(ROOT, "oracle", "liboracle.so").encode(), P.M, tf, dp(prm), recs.shape[0], dp(recs), dp(cs),
                                       dp(zl), dp(zu), dp(z0), tol, max_iter, int(RR.RULE_OFF_CRAWL_LIMIT), float(RR.OPTIONS["crawl_frac"]), 0,
                                       dp(out_d), out_i.ctypes.data_as(LR.I_))
    assert rc == 0, rc
    status = "converged" if out_i[0] else "locally infeasible" if out_i[5] else "max_iter" if out_i[6] else "other"
    return dict(status=status, iterations=int(out_i[1]), evaluations=int(out_i[2]), cost=float(out_d[0]))


def fixture():
    return json.load(open(FIXTURE))


def rows_for(base, B, seed=7):
    """B distinct parameter rows: every entry of the nominal set scaled by a seeded factor in [0.8, 1.25] (none changes sign or
    vanishes); row 0 is the nominal set itself.  [B][len(base)]"""
    base = np.asarray(base, dtype=np.float64)
    rng = np.random.default_rng(seed)
    rows = base[None, :] * rng.uniform(0.8, 1.25, (B, base.size))
    rows[0] = base
    return np.ascontiguousarray(rows)
