"""Generates tests/golden/ladder_cases.json: the fixture of the mesh ladder's tests (emi_ipm_solve_ladder_*).

Every instance of tests/ladder_ref.py (the 2 x 9 quadrotor instances of tests/lockstep_ref.py, started on 21 nodes) taken up the
ladder (21, 41) on the CPU: the project's own solve_nlp -- oracle evaluator, dense host factorisation, tol 1e-8, default options
except that the rules the lock-step driver leaves out are switched off as far as NlpOptions can (inertia search, crawl rule,
stagnation rule; the second-order correction and the residual-based acceptance have no switch) -- through
tests/harness/etol_harness_ladder.cpp; between the rungs the numpy barycentric prolongation of tests/ladder_ref.py and a clip into
the bounds.  Recorded per rung and instance: whether it converged, iterations, evaluations, cost, final rho.  No GPU needed:

    python tests/golden/gen_ladder_cases.py
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


def solve(h, tf, M, discs, z0, reduced, tol=1e-8, max_iter=200):
    P = LD.quad_at(tf, M, discs)
    recs = np.ascontiguousarray(LR.records(discs))
    dp = lambda a: a.ctypes.data_as(LD.D_)
    prm, cs = np.array(LR.QUAD_PARAMS), np.ascontiguousarray(LR.CSCALE)
    zl, zu, z0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (P.lo, P.up, z0))
    out_d, out_i, z = np.zeros(4), np.zeros(3, dtype=np.int32), np.zeros(P.n)
    rc = h.harness_ladder_solve_oracle(os.path.join(ROOT, "oracle", "liboracle.so").encode(), M, tf, dp(prm), recs.shape[0], dp(recs), dp(cs),
                                       dp(zl), dp(zu), dp(z0), tol, max_iter, int(reduced), dp(out_d), out_i.ctypes.data_as(LD.I_), dp(z))
    assert rc == 0, rc
    row = dict(M=M, ok=bool(out_i[0]), iterations=int(out_i[1]), evaluations=int(out_i[2]), cost=float(out_d[0]), rho=float(out_d[1]),
               kkt_error=float(out_d[2]), constr_viol=float(out_d[3]))
    return row, z, P


def climb(h, tf, inst, reduced):
    import etol_amd as E
    rows, z, prev = [], inst["z0"], None
    for M in LD.LADDER:
        if prev is not None:
            (tc, wc, _), tf_ = E.lgl(prev), E.lgl(M)[0]
            Pm = LD.bary_matrix(tc, wc, tf_)
            P = LD.quad_at(tf, M, inst["discs"])
            z = np.clip((z.reshape(8, prev) @ Pm.T).reshape(-1), P.lo, P.up)
        row, z, _ = solve(h, tf, M, inst["discs"], z, reduced)
        rows.append(row)
        prev = M
    return rows


def main():
    import __graft_entry__ as g
    g.build(quiet=True)
    h = LD.load_harness()
    lock = LR.fixture()["cases"]
    out = dict(ladder=list(LD.LADDER), tol=1e-8, rules="solve_nlp with max_shift_trials 0, crawl and stagnation rules off", replaced=[], cases={})
    for tf in LR.TFS:
        rows = []
        for b, inst in enumerate(LD.instances(tf)):
            rungs = climb(h, tf, inst, reduced=1)
            full = climb(h, tf, inst, reduced=0)
            rel = abs(rungs[-1]["cost"] - lock[str(tf)][b]["cost"]) / abs(lock[str(tf)][b]["cost"])
            rows.append(dict(discs=[list(d) for d in inst["discs"]], bump=inst["bump"], rungs=rungs,
                             full_rules_iterations=[r["iterations"] for r in full]))
            print(f"tf {tf} instance {b}: " + "; ".join(f"M {r['M']} ok {r['ok']} it {r['iterations']} cost {r['cost']:.6f}" for r in rungs) +
                  f"; full rules it {[r['iterations'] for r in full]} ok {[r['ok'] for r in full]}; cost against the one-mesh fixture {rel:.1e}")
        out["cases"][str(tf)] = rows
    json.dump(out, open(LD.LADDER_FIXTURE, "w"), indent=1)
    print("wrote", LD.LADDER_FIXTURE)


if __name__ == "__main__":
    main()
