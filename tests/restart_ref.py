"""Reference side of the restart that matters (tests/test_gpu_restart.py, tests/golden/restart_cases.json): quadrotor instances whose
straight line runs into a wall of discs.  TEST INFRASTRUCTURE: numpy + the harness, nothing of the package.

  * the instances: six discs each, their centres on a line across the straight line (1, 1) -> (8, 6).  Two thin walls, which a
    trajectory started on the line gets past, and two thick ones that reach the edge of the state box on one side and leave a gap on the
    other: the line start converges on 21 nodes (the keep-outs act at the nodes only) and on 41 nodes runs out of iterations
    with the constraints still violated by more than 1e-3, while the route planned past the keep-outs is solved on both rungs;
  * the problem on M nodes (quad_at), the two starts (the line of tests/plan_ref.py; the planned route of its restatement of
    emi_plan_route, on the default grid), the solve on the CPU oracle with the reduced rule set (harness_ladder_solve_oracle) and the
    climb over the ladder that ends at a rung that fails, as tests/golden/gen_ladder_cases.py climbs;
  * the fixture tests/golden/restart_cases.json (tests/golden/gen_restart_cases.py).
"""
import json
import os

import numpy as np

import ladder_ref as LD
import lockstep_ref as LR
import plan_ref as PR

ROOT = LR.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "restart_cases.json")
TF = 4.0
LADDER = (21, 41)
TOL, MAX_ITER = 1e-8, 100
XA, XB = [1.0, 1.0, 0, 0, 0, 0], [8.0, 6.0, 0, 0, 0, 0]
BOX = [0.0, 10.0, 0.0, 10.0]                        # the position states' bounds: the planner's box
CLEARANCE = 0.01
STARTS = ("line", "planned")                        # the order of the attempts
NOT_SOLVED = 1e-3                                   # what "not solved" asks of constr_viol beyond the iteration limit


def wall(ks, r, spacing, shift=0.0, along=0.5):
    """discs of radius r, centres k spacing + shift (k in ks) to the left of the point `along` the straight line"""
    a, b = np.array(XA[:2]), np.array(XB[:2])
    d = (b - a) / np.hypot(*(b - a))
    n = np.array([-d[1], d[0]])
    mid = a + (b - a) * along
    return [tuple(float(v) for v in mid + (k * spacing + shift) * n) + (float(r),) for k in ks]


# (name, discs): thin walls first and last, the two thick walls between them
WALLS = (("thin", wall(range(-4, 2), 0.55, 0.9)), ("thick", wall(range(-4, 2), 0.9, 1.2, 0.3)),
         ("thick, nearer the start", wall(range(-4, 2), 0.9, 1.2, 0.3, 0.35)), ("thin, shifted", wall(range(-4, 2), 0.55, 0.9, 0.2)))
NDISCS = 6


def quad_at(M, discs):
    return LD.quad_at(TF, M, discs)


def start(M, discs, kind):
    """(z0 [8 M], level): the states of the line or, where the planner has a route, of the planned route; hover thrust"""
    import indep_nlp as N
    P = quad_at(M, discs)
    z = N.starts(P, [0.0])[0].reshape(8, M).copy()
    X = PR.line(np.array([XA]), np.array([XB]), P.tau)[0]
    level = -2
    if kind == "planned":
        xs, ys, level, _, _ = PR.plan_route(LR.records(discs), np.array(XA[:2] + XB[:2]), P.tau, np.array(BOX), CLEARANCE, 0)
        if level >= 0:
            X[0], X[1] = xs, ys
    z[:6] = X
    return np.clip(z.reshape(-1), P.lo, P.up), int(level)


def cpu_solve(h, M, discs, z0):
    """solve_nlp on the CPU oracle, reduced rule set -> (row, z)"""
    P = quad_at(M, discs)
    recs = np.ascontiguousarray(LR.records(discs))
    dp = lambda a: a.ctypes.data_as(LD.D_)
    prm, cs = np.array(LR.QUAD_PARAMS), np.ones(len(discs))
    zl, zu, z0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (P.lo, P.up, z0))
    out_d, out_i, z = np.zeros(4), np.zeros(3, dtype=np.int32), np.zeros(P.n)
    rc = h.harness_ladder_solve_oracle(os.path.join(ROOT, "oracle", "liboracle.so").encode(), M, TF, dp(prm), recs.shape[0], dp(recs), dp(cs),
                                       dp(zl), dp(zu), dp(z0), TOL, MAX_ITER, 1, dp(out_d), out_i.ctypes.data_as(LD.I_), dp(z))
    assert rc == 0, rc
    return dict(M=M, ok=bool(out_i[0]), iterations=int(out_i[1]), cost=float(out_d[0]), kkt_error=float(out_d[2]), constr_viol=float(out_d[3])), z


def cpu_climb(h, discs, kind):
    """the instance up the ladder from one start; a rung that fails ends the climb -> (rows, level)"""
    import oracle_lib as O
    z, level = start(LADDER[0], discs, kind)
    rows, prev = [], None
    for M in LADDER:
        if prev is not None:
            (tc, wc, _), tf_ = O.lgl(prev), O.lgl(M)[0]
            P = quad_at(M, discs)
            z = np.clip((z.reshape(8, prev) @ LD.bary_matrix(tc, wc, tf_).T).reshape(-1), P.lo, P.up)
        row, z = cpu_solve(h, M, discs, z)
        rows.append(row)
        prev = M
        if not row["ok"]:
            break
    return rows, level


def solved(rows):
    return len(rows) == len(LADDER) and all(r["ok"] for r in rows)


def fixture():
    return json.load(open(FIXTURE))
