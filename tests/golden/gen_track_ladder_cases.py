"""Generates tests/golden/track_ladder_cases.json: the fixture of the tests of the mesh ladder with moving-disc rows
(emi_ipm_solve_ladder_* with rows of kind EMI_PATH_TRACK over waypoint tables, tests/test_gpu_track_ladder.py).

The first three tf = 4.0 instances of tests/ladder_ref.py, each with its first disc replaced by a track row of the same radius
(tests/track_ladder_ref.py: moving_instances).  The track has three waypoints -- at t0, at T_MID (a node time of neither rung) and
at tf -- and its centre crosses the straight line between the boundary positions at right angles, through the disc's own centre
at T_MID, by DISPLACEMENT x the disc's diameter.  Every instance climbs (21, 41) on the CPU under the rule set of
tests/golden/gen_ladder_cases.py: the project's own solve_nlp -- oracle evaluator with the host centres of the rung
(emi_track_centres), dense host factorisation, tol 1e-8 -- with inertia search, crawl rule and stagnation rule off, through
tests/harness/etol_harness_track_ladder.cpp; between the rungs the numpy barycentric prolongation and a clip into the bounds.
Recorded per rung: ok, iterations, cost, KKT error.

Asserted, naming the offending instance: every instance converges on both rungs, and the moving disc is ACTIVE on the final
trajectory -- the row r^2 - |p - c(t)|^2 <= 0 comes within 1e-6 r^2 of its bound 0 at some node.  An instance that fails either is
a reason to change DISPLACEMENT (and say so in the fixture's `note`), not the criteria.  No GPU needed:

    python tests/golden/gen_track_ladder_cases.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ladder_ref as LD  # noqa: E402
import lockstep_ref as LR  # noqa: E402
import oracle_lib as O  # noqa: E402
import track_ladder_ref as TR  # noqa: E402

# why DISPLACEMENT is not 1
NOTE = ("displacement -5 disc diameters instead of 1: with 1 (and with 0.25, 0.5, 2, 3, -0.5, -1, -1.5, -2, -3) the third instance's "
        "trajectory keeps clear of its first disc (smallest slack 0.07 .. 0.51 against r^2 = 0.81, cost 400.8566 whatever the disc does), "
        "so the moving row was not active there; at -4 it just touches (cost 400.8653), at -5 every instance's cost moves")


def main():
    import __graft_entry__ as g
    g.build(quiet=True)
    h = TR.load_harness()
    tf = TR.TF
    for M in TR.LADDER:
        gap = np.abs(TR.node_times(M, 0.0, tf) - TR.T_MID).min()
        assert gap > 1e-3, f"T_MID {TR.T_MID} lies {gap:.1e} from a node time of the {M}-node rung"
    plain = LD.ladder_fixture()["cases"][str(tf)]
    out = dict(ladder=list(TR.LADDER), tf=tf, tol=1e-8, rules="solve_nlp with max_shift_trials 0, crawl and stagnation rules off",
               t_mid=TR.T_MID, displacement=TR.DISPLACEMENT, note=NOTE, cases=[])
    for b, inst in enumerate(TR.moving_instances()):
        rungs, z = TR.cpu_climb(h, tf, inst)
        M = TR.LADDER[-1]
        assert all(r["ok"] for r in rungs), f"instance {b} does not converge on every rung: {rungs}"
        X, U = z[:6 * M].reshape(1, 6, M), z[6 * M:].reshape(1, 2, M)
        RES = O.evaluate(1, LR.QUAD_PARAMS, M, O.lgl(M), 0.0, tf, X, U, recs=inst["recs"], tracks=TR.host_centres([inst["way"]], M, 0.0, tf))[0]
        rsq = inst["discs"][0][2] ** 2
        slack = float(-RES[0, 6].max())
        assert slack < 1e-6 * rsq, f"instance {b}: the moving disc is not active (smallest slack {slack:.3e}, r^2 {rsq:.3f})"
        t, x, y = inst["way"]
        out["cases"].append(dict(discs=[list(d) for d in inst["discs"]], bump=inst["bump"], waypoints=dict(t=t[0].tolist(), x=x[0].tolist(),
                                                                                                         y=y[0].tolist()),
                                 rungs=rungs, track_slack=slack))
        print(f"instance {b}: " + "; ".join(f"M {r['M']} ok {r['ok']} it {r['iterations']} cost {r['cost']:.6f} kkt {r['kkt_error']:.1e}" for r in rungs) +
              f"; slack of the track row {slack:.2e}; with the disc at rest the cost was {plain[b]['rungs'][-1]['cost']:.6f}")
    json.dump(out, open(TR.FIXTURE, "w"), indent=1)
    print("wrote", TR.FIXTURE)


if __name__ == "__main__":
    main()
