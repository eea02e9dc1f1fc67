"""Reference side of the tests of moving-disc rows in the lock-step ladder and refinement (emi_set_track_waypoints,
emi_tracks_from_waypoints_dev, emi_get_tracks; rows of kind EMI_PATH_TRACK in emi_ipm_solve_ladder_* / emi_ipm_solve_refine_*).
TEST INFRASTRUCTURE: numpy + the harness.

  * the instances: those of tests/ladder_ref.py with their FIRST disc turned into a track row of the same radius, either at rest
    (static_instances: every waypoint at the disc's centre, so the centre arithmetic returns the centre exactly and the optima are
    those of tests/golden/ladder_cases.json and refine_cases.json) or moving (moving_instances: the first three tf = 4.0 instances,
    the centre crossing the straight line between the boundary positions; fixture tests/golden/track_ladder_cases.json,
    tests/golden/gen_track_ladder_cases.py);
  * the host route to the centres (host_centres: emi_track_centres per track at the node times t0 + h (tau_k + 1)), which the device
    route must reproduce bit for bit;
  * the record tables, the waypoint tables as emi_set_track_waypoints takes them, and the new harness call.
"""
import ctypes as C
import json
import os

import numpy as np

import ladder_ref as LD
import lockstep_ref as LR

ROOT = LR.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "track_ladder_cases.json")
TF = 4.0
LADDER = LD.LADDER
N_MOVING = 3
# the time of the middle waypoint: a node time of neither rung (no LGL node of 21 or 41 points on [0, 4] lies within 1e-3 of it;
# gen_track_ladder_cases.py asserts that)
T_MID = 1.7
# how far the centre travels across the line between the boundary positions, in units of the disc's diameter, the sign saying
# towards which side (positive: to the left of START -> END).  Not the one diameter first tried: the third instance passes its
# first disc at a distance, and the disc stayed inactive there for every displacement between -3 and +3 diameters (the fixture's
# `note`, tests/golden/gen_track_ladder_cases.py)
DISPLACEMENT = -5.0
START, END = (1.0, 1.0), (8.0, 6.0)
D_ = C.POINTER(C.c_double)
I_ = C.POINTER(C.c_int)


def track_records(discs):
    """lockstep_ref.records with the first disc as a row of kind EMI_PATH_TRACK (track 0, same radius)"""
    recs = LR.records(discs)
    recs[0] = 0.0
    recs[0, :3] = [2, 0, discs[0][2] ** 2]
    return recs


def static_waypoints(discs, tf=TF):
    """(t, x, y) [1 track][3]: a track that does not move from the first disc's centre"""
    cx, cy, _ = discs[0]
    return np.array([[0.0, T_MID, tf]]), np.full((1, 3), cx), np.full((1, 3), cy)


def moving_waypoints(discs, tf=TF, displacement=DISPLACEMENT):
    """(t, x, y) [1 track][3]: the centre crosses the line START -> END at right angles, through the first disc's own centre at
    T_MID, by displacement x the disc's diameter over [0, tf]"""
    cx, cy, r = discs[0]
    d = np.array(END) - np.array(START)
    n = np.array([-d[1], d[0]]) / np.hypot(*d)
    half = displacement * r
    a, b = np.array([cx, cy]) - half * n, np.array([cx, cy]) + half * n
    return np.array([[0.0, T_MID, tf]]), np.array([[a[0], cx, b[0]]]), np.array([[a[1], cy, b[1]]])


def static_instances(tf):
    """ladder_ref.instances(tf) with a track at rest for the first disc: list of dict discs, bump, z0, recs, way"""
    return [dict(i, recs=track_records(i["discs"]), way=static_waypoints(i["discs"], tf)) for i in LD.instances(tf)]


def moving_instances(displacement=DISPLACEMENT):
    return [dict(i, recs=track_records(i["discs"]), way=moving_waypoints(i["discs"], TF, displacement))
            for i in LD.instances(TF)[:N_MOVING]]


def node_times(M, t0, tf):
    """the node times as emi_set_mesh forms them: t0 + h (tau_k + 1)"""
    import etol_amd as E
    return t0 + (tf - t0) / 2.0 * (E.lgl(M)[0] + 1.0)


def host_centres(ways, M, t0=0.0, tf=TF, counts=None):
    """ways: list over sets of (t, x, y) [ntracks][ld] -> (xc, yc) [sets][ntracks][M] from emi_track_centres per track (the route
    the device call replaces); counts [sets][ntracks]: the waypoints of each track (None: all ld)"""
    import etol_amd as E
    nt = node_times(M, t0, tf)
    xc = np.empty((len(ways), ways[0][0].shape[0], M))
    yc = np.empty_like(xc)
    for s, (t, x, y) in enumerate(ways):
        for k in range(t.shape[0]):
            n = t.shape[1] if counts is None else int(counts[s][k])
            xc[s, k], yc[s, k] = E.track_centres(t[k, :n], x[k, :n], y[k, :n], nt)
    return xc, yc


def stacked(ways):
    """list over sets of (t, x, y) [ntracks][ld] -> t, x, y [sets][ntracks][ld]"""
    return tuple(np.ascontiguousarray(np.stack([w[q] for w in ways])) for q in range(3))


def load_harness():
    h = LD.load_harness()
    h.harness_track_ladder_solve_oracle.argtypes = [C.c_char_p, C.c_int, C.c_double, D_, C.c_int, D_, C.c_int, D_, D_, D_, D_, D_, D_, C.c_double,
                                                    C.c_int, C.c_int, D_, I_, D_]
    return h


def cpu_solve(h, tf, M, inst, z0, reduced=1, tol=1e-8, max_iter=200):
    """solve_nlp on the CPU oracle for one instance with its track on M nodes from z0 -> (row of the fixture, z)"""
    P = LD.quad_at(tf, M, inst["discs"])
    recs = np.ascontiguousarray(inst["recs"])
    xc, yc = host_centres([inst["way"]], M, 0.0, tf)
    tx, ty = np.ascontiguousarray(xc[0]), np.ascontiguousarray(yc[0])
    dp = lambda a: a.ctypes.data_as(D_)
    prm, cs = np.array(LR.QUAD_PARAMS), np.ascontiguousarray(LR.CSCALE)
    zl, zu, z0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (P.lo, P.up, z0))
    out_d, out_i, z = np.zeros(4), np.zeros(3, dtype=np.int32), np.zeros(P.n)
    rc = h.harness_track_ladder_solve_oracle(os.path.join(ROOT, "oracle", "liboracle.so").encode(), M, tf, dp(prm), recs.shape[0], dp(recs),
                                             tx.shape[0], dp(tx), dp(ty), dp(cs), dp(zl), dp(zu), dp(z0), tol, max_iter, int(reduced), dp(out_d),
                                             out_i.ctypes.data_as(I_), dp(z))
    assert rc == 0, rc
    return dict(M=M, ok=bool(out_i[0]), iterations=int(out_i[1]), cost=float(out_d[0]), kkt_error=float(out_d[2])), z


def cpu_climb(h, tf, inst, ladder=LADDER, reduced=1):
    """the instance up the ladder on the CPU, as tests/golden/gen_ladder_cases.py climbs: numpy barycentric prolongation and a clip
    into the bounds between the rungs -> (rows per rung, the final z)"""
    import etol_amd as E
    rows, z, prev = [], inst["z0"], None
    for M in ladder:
        if prev is not None:
            (tc, wc, _), tf_ = E.lgl(prev), E.lgl(M)[0]
            P = LD.quad_at(tf, M, inst["discs"])
            z = np.clip((z.reshape(8, prev) @ LD.bary_matrix(tc, wc, tf_).T).reshape(-1), P.lo, P.up)
        row, z = cpu_solve(h, tf, M, inst, z, reduced)
        rows.append(row)
        prev = M
    return rows, z


def fixture():
    return json.load(open(FIXTURE))
