#!/usr/bin/env python3
"""Ladder restarts of a whole batch (emi_ipm_solve_restart_dev: the instances an attempt did not solve are solved again, compacted,
from the next start) beside the two single-start ladder calls it replaces.  Same instances, same GPU, same session.  Nothing is gated
and nothing is predicted; one JSON line goes to profiles/restart_times.jsonl.

  python tools/restart_times.py [--batch 64] [--ladder 33,65,129,257] [--obstacles 20] [--max-iter 60]

Problem, instances and rung settings: those of tools/start_times.py (quadrotor, `--obstacles` random disc keep-outs per instance,
(1, 1) -> (8, 6) in the box [0, 10]^2, warm settings above the first rung, keep-outs inflated per rung below the last, repair on).
  line, planned   emi_ipm_solve_ladder_dev on all B instances from the straight line and from the planned route (repaired on the first
                  rung's mesh and table), as tools/start_times.py runs them
  restart         emi_ipm_solve_restart_dev without a check (rf NULL), the starts in the host driver's order (host/emi_mesh_driver.cpp):
                  planned route, line, then the line bent by +0.15, -0.15, +0.35 and -0.35 of the span; EMI_RESTART_DROP_FAILED; once
                  with the residual rule (EMI_IPM_RULE_RESIDUAL) on every rung and once with the rules of the two ladder calls; and,
                  with those rules, once without the flag (everybody climbs to the last rung, as in the ladder calls, and only who
                  fails there is solved again)
Per run: how many instances end converged (and converged or acceptable) on the last rung, the wall time of the synchronised call, the
instances solved per attempt and the rounds per attempt (a rung's rounds are the iterations of its slowest instance: the batch moves
in lock step).  For the restart runs also the status of every instance in the attempt that owns its output."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import etol_amd as E
from etol_amd import _lib as L
from etol_amd import workloads as W
import ladder_times as LdT
import lockstep_times as LT
import start_times as ST

BENDS = (0.15, -0.15, 0.35, -0.35)          # kBends of host/emi_mesh_driver.cpp, fractions of the span


def rounds(rows):
    """lock-step rounds of one rung's solve: the iterations of the slowest instance that was solved there"""
    return max([q["iterations"] for q in rows if q["status"] != -1], default=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ladder", default="33,65,129,257")
    ap.add_argument("--obstacles", type=int, default=20)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restart_times.jsonl"))
    a = ap.parse_args()
    ladder = [int(m) for m in a.ladder.split(",")]
    B, ML, nobs = a.batch, ladder[-1], a.obstacles
    _, _, recs = W.quadrotor_batch(3, B, ML, nobs)
    ev = LT.context(ML, recs)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(ev.device)
    cl, cu = np.full(nobs, -1000.0), np.zeros(nobs)

    def rungs_with(rules):
        rungs = []
        for g, M in enumerate(ladder):
            zl, zu, _, _ = LT.problem(M, E.lgl(M)[0])
            opt = dict(tol=1e-8, max_iter=a.max_iter, rules=rules)
            if g > 0:
                opt.update(mu_init=LdT.WARM_MU, bound_push=LdT.WARM_PUSH, bound_frac=LdT.WARM_PUSH)
            rungs.append(dict(M=M, bounds=dict(zl=up(zl), zu=up(zu), cl=cl, cu=cu), options=opt, repair=1,
                              recs=LdT.inflated(recs, M) if M != ML else recs))
        return rungs

    _, _, X1, U1 = LT.problem(ladder[0], E.lgl(ladder[0])[0])
    X0d, U0d = up(np.repeat(X1[None], B, 0)), up(np.repeat(U1[None], B, 0))
    plain = rungs_with(0)
    ok = lambda q, upto: 0 <= q["status"] <= upto

    def climb(X0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.ipm_solve_ladder(plain, 0.0, LT.TF, X0, U0d)[4]
        ev.synchronize()
        return dict(seconds=time.perf_counter() - t0, converged=sum(ok(q, 0) for q in res[-1]), converged_or_acceptable=sum(ok(q, 1) for q in res[-1]),
                    instances_per_attempt=[B], rounds_per_attempt=[sum(rounds(r) for r in res)],
                    solved=[bool(ok(q, 0)) for q in res[-1]])

    climb(X0d)                                  # warm
    line = climb(X0d)
    ev.set_mesh(ladder[0], 0.0, LT.TF)
    ev.set_path(plain[0]["recs"], 0, 1)
    Xp, _ = ev.start_guess(E.START_PLANNED, LT.X0, LT.XF, box=ST.BOX, clearance=ST.CLEARANCE, repair=1)
    ev.synchronize()
    planned = climb(Xp)
    either = sum(x or y for x, y in zip(line.pop("solved"), planned.pop("solved")))

    span = float(max(abs(LT.XF[0] - LT.X0[0]), abs(LT.XF[1] - LT.X0[1])))
    common = dict(xa=LT.X0, xb=LT.XF, box=ST.BOX)
    starts = [dict(kind=E.START_PLANNED, bend=BENDS[0] * span, clearance=ST.CLEARANCE, repair=1, **common), dict(kind=E.START_LINE, **common)]
    starts += [dict(kind=E.START_BEND, bend=f * span, **common) for f in BENDS]

    def restart(rules, flags=L.RESTART_DROP_FAILED):
        rungs = rungs_with(rules)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, _, _, res, _, summ = ev.ipm_solve_restart(rungs, 0.0, LT.TF, starts, U0d, flags=flags)
        ev.synchronize()
        sec = time.perf_counter() - t0
        last = len(ladder) - 1
        final = [res[q["attempt"]][q["rung"]][b] for b, q in enumerate(summ)]
        return dict(rules=rules, flags=flags, seconds=sec, converged=sum(q["rung"] == last and ok(f, 0) for q, f in zip(summ, final)),
                    converged_or_acceptable=sum(q["rung"] == last and ok(f, 1) for q, f in zip(summ, final)),
                    instances_per_attempt=[sum(q["status"] != -1 for q in block[0]) for block in res],
                    rounds_per_attempt=[sum(rounds(r) for r in block) for block in res],
                    solved_in_attempt=[sum(q["attempt"] == k and q["verdict"] == 0 for q in summ) for k in range(len(res))],
                    levels={str(l): sum(q["level"] == l for q in summ) for l in (0, 1, 2, -1, -2)},
                    per_instance=[dict(attempt=q["attempt"], attempts=q["attempts"], rung=q["rung"], status=LT.STATUS[f["status"]]) for q, f in zip(summ, final)])

    rec = dict(B=B, ladder=ladder, obstacles=nobs, max_iter=a.max_iter, starts=["planned", "line"] + [f"bend {f:+.2f}" for f in BENDS], span=span,
               line=line, planned=planned, line_or_planned_converged=either, restart_residual_rule=restart(L.IPM_RULE_RESIDUAL), restart_plain_rules=restart(0),
               restart_plain_rules_no_drop=restart(0, 0))
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    ev.close()


if __name__ == "__main__":
    main()
