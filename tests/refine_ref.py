"""Reference side of the tests of the lock-step mesh refinement (emi_ipm_solve_refine_*, emi_prolong_rows_dev, emi_shard_move_dev,
emi_ipm_refine_decide).  TEST INFRASTRUCTURE: numpy + the harness.

  * the cases: the 2 x 9 quadrotor instances of tests/ladder_ref.py (started on 21 nodes) over the ladder (21, 41, 61, 91), with one
    ODE tolerance per final time, checked from the second rung on;
  * the rule restated (walk): what becomes of one instance given what it did on every rung -- through the library's
    emi_ipm_refine_decide, the one function the driver calls too;
  * the ODE error of a returned trajectory in float64 (ode_err: tests/ode_error_ref.py's estimate at the library's points), with the
    bound derived there;
  * the fixture tests/golden/refine_cases.json (tests/golden/gen_refine_cases.py): the CPU climb of every instance over the whole
    ladder -- per rung ok, iterations, cost, err -- and the rule's rung and verdict.
"""
import json
import os

import numpy as np

import ladder_ref as LD
import lockstep_ref as LR
import ode_error_ref as OE

ROOT = LR.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "refine_cases.json")
LADDER = (21, 41, 61, 91)
FIRST_CHECK = 1
# one tolerance per final time: every recorded err that decides something lies outside [tol / BAND, BAND tol]
TOLS = {4.0: 5.5e-4, 2.5: 6.6e-4}
BAND = 1.2
# per final time: how many instances retire on which rung
SPLIT = {4.0: {1: 6, 3: 3}, 2.5: {1: 5, 3: 4}}
MET, NOT_MET, FELL_BACK, FAILED = range(4)
UL, UU = np.array([0.0, -1.0]), np.array([25.0, 1.0])       # the controls' bounds of ladder_ref.quad_at: the clip of the estimate


def fixture():
    return json.load(open(FIXTURE))


def decide(status, err, tol, has_good, is_last):
    """(retires, verdict) from the library's emi_ipm_refine_decide"""
    import etol_amd as E
    return E.Evaluator.refine_decide(status, err, tol, has_good, is_last)


def walk(oks, errs, tol, first_check=FIRST_CHECK, rule=decide):
    """One instance up the ladder: oks[r] / errs[r] = whether its solve on rung r ended converged or acceptable, and its estimate
    there.  -> (rung of the returned trajectory, verdict, rungs solved, the decisions [(rung, err, retired)] that were taken)"""
    has_good, taken = False, []
    for r in range(len(oks)):
        if r < first_check:
            continue
        retires, verdict = rule(LR.CONVERGED if oks[r] else LR.MAX_ITER, errs[r], tol, has_good, r + 1 == len(oks))
        taken.append((r, errs[r], retires))
        if retires:
            return (r - 1 if verdict == FELL_BACK else r), verdict, r + 1, taken
        has_good = True
    raise AssertionError("the last rung retires everybody")


def ode_case(tf, M):
    """what ode_error_ref.estimate wants to know of the quadrotor on M LGL nodes over [0, tf]"""
    import etol_amd as E
    tau, w, D = E.lgl(M)
    return dict(name="quadrotor", M=M, t0=0.0, tf=float(tf), tau=tau, w=w, D=D, ns=6, nc=2, ul=UL, uu=UU)


def ode_err(tf, M, X, U, dtype=np.float64):
    """estimate of X [B][6][M], U [B][2][M] at the library's points -> the dict of ode_error_ref.estimate (err [B], bound parts)"""
    assert OE.SPEC["quadrotor"]["params"] == LR.QUAD_PARAMS
    c = ode_case(tf, M)
    tq = OE.library_points(M, (c["tau"], c["w"]))
    return OE.estimate(c, tq, dtype=dtype, X=np.ascontiguousarray(X), U=np.ascontiguousarray(U))


def band_violations(fx):
    """the decisions of the fixture whose err lies inside [tol / BAND, BAND tol]: [(tf, b, rung, err)]"""
    bad = []
    for tf, rows in fx["cases"].items():
        tol = fx["tolerances"][tf]
        for b, row in enumerate(rows):
            oks, errs = [g["ok"] for g in row["rungs"]], [g["err"] for g in row["rungs"]]
            for r, e, _ in walk(oks, errs, tol, fx["first_check"])[3]:
                if oks[r] and tol / BAND <= e <= BAND * tol:
                    bad.append((tf, b, r, e))
    return bad
