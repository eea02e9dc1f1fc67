"""Generates tests/golden/refine_cases.json: the fixture of the mesh refinement's tests (emi_ipm_solve_refine_*).

Every instance of tests/ladder_ref.py (the 2 x 9 quadrotor instances of tests/lockstep_ref.py, started on 21 nodes) taken up the whole
ladder (21, 41, 61, 91) on the CPU, as tests/golden/gen_ladder_cases.py does it: the project's own solve_nlp on the oracle with the
reduced rule set (harness_ladder_solve_oracle), the numpy barycentric prolongation of tests/ladder_ref.py and a clip into the bounds
between the rungs.  After every rung the relative local ODE error of the solution in float64 (tests/ode_error_ref.py: estimate, at
the library's points, controls clipped to their bounds).  Recorded per instance and rung: ok, iterations, cost, err; per instance
the rung and the verdict the rule (emi_ipm_refine_decide through tests/refine_ref.py: walk) gives with the tolerance of its final
time, checked from the second rung on; per final time the split over the retiring rungs.

The tolerances are chosen so that every err that decides something lies outside [tol / 1.2, 1.2 tol]: the lock-step solve reaches
the same optima to ~1e-6, not the same bits, and an err inside the band could fall on either side.  The generator asserts that; a
rebuild that moves a value into the band has to move the tolerance in tests/refine_ref.py and say so under "note".  No GPU needed:

    python tests/golden/gen_refine_cases.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import gen_ladder_cases as GL  # noqa: E402
import ladder_ref as LD  # noqa: E402
import lockstep_ref as LR  # noqa: E402
import refine_ref as RR  # noqa: E402


def climb(h, tf, inst):
    import etol_amd as E
    rows, z, prev = [], inst["z0"], None
    for M in RR.LADDER:
        if prev is not None:
            (tc, wc, _), tf_ = E.lgl(prev), E.lgl(M)[0]
            P = LD.quad_at(tf, M, inst["discs"])
            z = np.clip((z.reshape(8, prev) @ LD.bary_matrix(tc, wc, tf_).T).reshape(-1), P.lo, P.up)
        row, z, _ = GL.solve(h, tf, M, inst["discs"], z, reduced=1)
        Z = z.reshape(1, 8, M)
        row["err"] = float(RR.ode_err(tf, M, Z[:, :6], Z[:, 6:])["err"][0])
        rows.append(row)
        prev = M
    return rows


def main():
    import __graft_entry__ as g
    g.build(quiet=True)
    h = LD.load_harness()
    out = dict(ladder=list(RR.LADDER), tol=1e-8, first_check=RR.FIRST_CHECK, band=RR.BAND, tolerances={str(tf): t for tf, t in RR.TOLS.items()},
               rules="solve_nlp with max_shift_trials 0, crawl and stagnation rules off", note="", cases={}, split={})
    for tf in LR.TFS:
        rows, split = [], {}
        for b, inst in enumerate(LD.instances(tf)):
            rungs = climb(h, tf, inst)
            rung, verdict, solved, _ = RR.walk([r["ok"] for r in rungs], [r["err"] for r in rungs], RR.TOLS[tf])
            split[str(rung)] = split.get(str(rung), 0) + 1
            rows.append(dict(discs=[list(d) for d in inst["discs"]], bump=inst["bump"], rungs=rungs, rung=rung, verdict=verdict, rungs_solved=solved))
            print(f"tf {tf} instance {b}: " + "; ".join(f"M {r['M']} ok {r['ok']} it {r['iterations']} cost {r['cost']:.6f} err {r['err']:.3e}" for r in rungs) +
                  f" -> rung {rung} verdict {verdict}")
        out["cases"][str(tf)] = rows
        out["split"][str(tf)] = split
        assert {int(k): v for k, v in split.items()} == RR.SPLIT[tf], (tf, split)
    bad = RR.band_violations(out)
    assert not bad, f"decisions inside the band: move the tolerance (tests/refine_ref.py: TOLS) and say so under note: {bad}"
    json.dump(out, open(RR.FIXTURE, "w"), indent=1)
    print("wrote", RR.FIXTURE)


if __name__ == "__main__":
    main()
