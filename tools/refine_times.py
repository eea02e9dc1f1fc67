#!/usr/bin/env python3
"""Wall time of the lock-step mesh refinement of a whole batch (emi_ipm_solve_refine_dev: instances retire as they meet the ODE
tolerance, the rest are compacted) beside the route without it to the same answer: emi_ipm_solve_ladder_dev to the last rung for
everybody, then emi_ode_error_dev.  Same instances, same GPU.  Nothing is gated and nothing is predicted; one JSON line goes to
profiles/refine_times.jsonl.

  python tools/refine_times.py [--batch 64] [--ladder 33,65,129,257] [--first-check 1] [--ode-tol 1e-4] [--rounds 3] [--max-iter 60]
                               [--obstacles 20] [--rules 0]

Problem, instances and rung settings: those of tools/ladder_times.py (quadrotor, `--obstacles` random disc keep-outs per instance,
straight-line starts, warm settings above the first rung, keep-outs inflated per rung below the last, repair on).  After a warm-up
call of either form, `rounds` rounds alternate between the two; each figure is the wall time of the synchronised call(s).  Reported
beside the times: instances retired per rung, verdict counts, instances solved per rung, what the fixed ladder's ODE errors say of
its answers, and the bytes that cross the host per call for the decisions (n doubles down per checked rung; the row map, the live
list for per-instance bounds and the two scatter lists up)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import etol_amd as E
from etol_amd import workloads as W
import ladder_times as LA
import lockstep_times as LT

VERDICT = ("met", "not_met", "fell_back", "failed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ladder", default="33,65,129,257")
    ap.add_argument("--first-check", type=int, default=1)
    ap.add_argument("--ode-tol", type=float, default=1e-4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--obstacles", type=int, default=20)
    ap.add_argument("--rules", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_times.jsonl"))
    a = ap.parse_args()
    ladder = [int(m) for m in a.ladder.split(",")]
    B, ML, nobs = a.batch, ladder[-1], a.obstacles
    _, _, recs = W.quadrotor_batch(3, B, ML, nobs)
    assert (recs[..., 0] == 1).all()          # EMI_PATH_DISC
    ev = LT.context(ML, recs)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(ev.device)
    cl, cu = np.full(nobs, -1000.0), np.zeros(nobs)
    rungs = []
    for g, M in enumerate(ladder):
        zl, zu, X1, U1 = LT.problem(M, E.lgl(M)[0])
        if g == 0:
            X0d, U0d = up(np.repeat(X1[None], B, 0)), up(np.repeat(U1[None], B, 0))
        opt = dict(tol=1e-8, max_iter=a.max_iter, rules=a.rules)
        if g > 0:
            opt.update(mu_init=LA.WARM_MU, bound_push=LA.WARM_PUSH, bound_frac=LA.WARM_PUSH)
        rungs.append(dict(M=M, bounds=dict(zl=up(zl), zu=up(zu), cl=cl, cu=cu), options=opt, repair=1,
                          recs=LA.inflated(recs, M) if M != ML else recs))

    def refine():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ev.ipm_solve_refine(rungs, 0.0, LT.TF, X0d, U0d, a.ode_tol, a.first_check, LT.ULO, LT.UUP)
        ev.synchronize()
        return time.perf_counter() - t0, out

    def fixed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X, U, _, _, res = ev.ipm_solve_ladder(rungs, 0.0, LT.TF, X0d, U0d)
        err = ev.ode_error(X, U, LT.ULO, LT.UUP, eta=False)[0].cpu().numpy()
        ev.synchronize()
        return time.perf_counter() - t0, res, err

    refine(), fixed()
    sec = dict(refine=[], fixed=[])
    for _ in range(a.rounds):
        tr, (_, _, _, _, res, err, summ) = refine()
        tf_, fres, ferr = fixed()
        sec["refine"].append(tr)
        sec["fixed"].append(tf_)
    nr = len(ladder)
    solved = [sum(q["status"] != -1 for q in rows) for rows in res]
    ok = lambda q: q["status"] in (0, 1)
    # bytes for the decisions: n doubles down per checked rung; up: the row map of the next rung and the lists of the retirees
    down = 8 * sum(solved[r] for r in range(a.first_check, nr))
    retired = [sum(q["rung"] == r or (q["verdict"] == 2 and q["rung"] == r - 1) for q in summ) for r in range(nr)]
    upb = 4 * (sum(solved[1:]) + 2 * len(summ))
    rec = dict(B=B, ladder=ladder, obstacles=nobs, max_iter=a.max_iter, rounds=a.rounds, rules=a.rules, ode_tol=a.ode_tol, first_check=a.first_check,
               seconds_refine=sec["refine"], seconds_ladder_then_ode_error=sec["fixed"],
               median_seconds_refine=statistics.median(sec["refine"]), median_seconds_ladder_then_ode_error=statistics.median(sec["fixed"]),
               instances_solved_per_rung=solved, returned_on_rung=[sum(q["rung"] == r for q in summ) for r in range(nr)],
               verdicts={VERDICT[v]: sum(q["verdict"] == v for q in summ) for v in range(4)},
               iterations_per_rung=[sum(q["iterations"] for q in rows if q["status"] != -1) for rows in res],
               iterations_per_rung_fixed_ladder=[sum(q["iterations"] for q in rows) for rows in fres],
               fixed_ladder_last_rung=dict(solved=sum(ok(q) for q in fres[-1]), solved_and_within_tol=int(sum(ok(q) and e <= a.ode_tol for q, e in zip(fres[-1], ferr))),
                                           not_solved=sum(not ok(q) for q in fres[-1])),
               decision_bytes_down=down, decision_bytes_up=upb, trajectory_bytes_across_host=0)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    ev.close()


if __name__ == "__main__":
    main()
