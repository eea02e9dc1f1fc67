"""Generates tests/golden/lockstep_cases.json: the fixture of the lock-step interior-point driver's tests.

Every instance of tests/lockstep_ref.py (41-node quadrotor, two discs, nine (discs, start) combinations per final time) solved
with the project's own solve_nlp -- oracle evaluator, dense host factorisation, default options, tol 1e-8 -- through
tests/harness/etol_harness_lockstep.cpp.  Recorded per instance: cost, iterations, evaluations, final rho, and whether it
converged.  No GPU needed:

    python tests/golden/gen_lockstep_cases.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lockstep_ref as LR  # noqa: E402


def solve(h, tf, inst, tol=1e-8, max_iter=200):
    P = LR.quad(tf, inst["discs"])
    recs = np.ascontiguousarray(LR.records(inst["discs"]))
    dp = lambda a: a.ctypes.data_as(LR.D_)
    prm, cs = np.array(LR.QUAD_PARAMS), np.ascontiguousarray(LR.CSCALE)
    zl, zu, z0 = (np.ascontiguousarray(a, dtype=np.float64) for a in (P.lo, P.up, inst["z0"]))
    out_d, out_i, z = np.zeros(4), np.zeros(3, dtype=np.int32), np.zeros(P.n)
    rc = h.harness_lockstep_solve_oracle(os.path.join(ROOT, "oracle", "liboracle.so").encode(), P.M, tf, dp(prm), recs.shape[0], dp(recs), dp(cs),
                                         dp(zl), dp(zu), dp(z0), tol, max_iter, dp(out_d), out_i.ctypes.data_as(LR.I_), dp(z))
    assert rc == 0, rc
    return dict(discs=[list(d) for d in inst["discs"]], bump=inst["bump"], ok=bool(out_i[0]), iterations=int(out_i[1]),
                evaluations=int(out_i[2]), cost=float(out_d[0]), rho=float(out_d[1]), kkt_error=float(out_d[2]), constr_viol=float(out_d[3]))


def main():
    import __graft_entry__ as g
    g.build(quiet=True)
    h = LR.load_harness()
    out = dict(M=LR.M_NODES, tol=1e-8, cscale=LR.CSCALE.tolist(), cases={})
    for tf in LR.TFS:
        rows = [solve(h, tf, inst) for inst in LR.instances(tf)]
        out["cases"][str(tf)] = rows
        for r in rows:
            print(f"tf {tf}: bump {r['bump']:5.1f} disc {r['discs'][0]}: ok {r['ok']} cost {r['cost']:.6f} iterations {r['iterations']} "
                  f"evaluations {r['evaluations']} rho {r['rho']:g}")
    json.dump(out, open(LR.FIXTURE, "w"), indent=1)
    print("wrote", LR.FIXTURE)


if __name__ == "__main__":
    main()
