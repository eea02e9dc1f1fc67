#!/usr/bin/env python3
"""Wall time of the lock-step solve of a whole batch over a mesh ladder (emi_ipm_solve_ladder_dev) beside the single cold
emi_ipm_solve_shard_dev on the ladder's last mesh, same instances, same GPU.  Nothing is gated; one JSON line goes to
profiles/ladder_times.jsonl.

  python tools/ladder_times.py [--batch 64] [--ladder 33,65,129,257] [--rounds 3] [--max-iter 60] [--obstacles 20] [--rules 0]

Problem and instances: those of tools/lockstep_times.py (quadrotor, `--obstacles` random disc keep-outs per instance, straight-line
starts with hover thrust, on the ladder's first mesh for the ladder and on its last for the cold call).  The ladder runs as
solve() runs its own: default options on the first rung, the warm settings of the host solver (Alg::warm_mu_init 1e-5,
warm_bound_push 1e-4 as bound_push and bound_frac) on the rungs above it, the keep-outs inflated per rung below the last by half
the largest node spacing of the straight line (inflate_records of host/eMI355X.cpp), repair on; --rules is the value of emi_ipm_options_t.rules on every rung and in the cold call (1: residual-based acceptance and
the crawl rule).  After a warm-up call of either
form, `rounds` rounds alternate between the two; each figure is the wall time of the synchronised call.  The share of prolongation
and repair is measured apart: the same kernels on arrays of the ladder's shapes, by the context's event timer."""
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
import lockstep_times as LT

WARM_MU, WARM_PUSH = 1e-5, 1e-4


def inflated(recs, M):
    """disc records [B][np][8] with radii grown by half the largest node spacing of the straight line on M nodes"""
    span = float(np.hypot(*(LT.XF[:2] - LT.X0[:2])))
    delta = 0.5 * span * 1.5707963267948966 / (M - 1)
    out = recs.copy()
    out[..., 3] = (np.sqrt(np.maximum(out[..., 3], 0.0)) + delta) ** 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ladder", default="33,65,129,257")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--obstacles", type=int, default=20)
    ap.add_argument("--rules", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ladder_times.jsonl"))
    a = ap.parse_args()
    ladder = [int(m) for m in a.ladder.split(",")]
    B, ML, nobs = a.batch, ladder[-1], a.obstacles
    _, _, recs = W.quadrotor_batch(3, B, ML, nobs)
    assert (recs[..., 0] == 1).all()          # EMI_PATH_DISC
    ev = LT.context(ML, recs)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(ev.device)
    cl, cu = np.full(nobs, -1000.0), np.zeros(nobs)
    per = {}
    for M in ladder:
        zl, zu, X1, U1 = LT.problem(M, E.lgl(M)[0])
        per[M] = dict(zl=zl, zu=zu, X=np.repeat(X1[None], B, 0), U=np.repeat(U1[None], B, 0))
    rungs = []
    for g, M in enumerate(ladder):
        opt = dict(tol=1e-8, max_iter=a.max_iter, rules=a.rules)
        if g > 0:
            opt.update(mu_init=WARM_MU, bound_push=WARM_PUSH, bound_frac=WARM_PUSH)
        rungs.append(dict(M=M, bounds=dict(zl=up(per[M]["zl"]), zu=up(per[M]["zu"]), cl=cl, cu=cu), options=opt, repair=1,
                          recs=inflated(recs, M) if M != ML else recs))
    X0d, U0d = up(per[ladder[0]]["X"]), up(per[ladder[0]]["U"])

    def climb():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.ipm_solve_ladder(rungs, 0.0, LT.TF, X0d, U0d)[4]
        ev.synchronize()
        return time.perf_counter() - t0, res

    def cold():
        ev.set_mesh(ML, 0.0, LT.TF)
        ev.set_path(recs, 0, 1)
        return LT.solve(ev, per[ML]["X"], per[ML]["U"], per[ML]["zl"], per[ML]["zu"], nobs, dict(tol=1e-8, max_iter=a.max_iter, rules=a.rules))

    climb(), cold()
    sec = dict(ladder=[], cold=[])
    for _ in range(a.rounds):
        tl, rl = climb()
        tc, rc = cold()
        sec["ladder"].append(tl)
        sec["cold"].append(tc)
    # prolongation and repair by themselves, on the shapes of the ladder (event timer; median of 5)
    aside = 0.0
    for g in range(1, len(ladder)):
        mc, mf = ladder[g - 1], ladder[g]
        PT = up(ev.prolong_matrix(mc, mf).T)
        Xc, Uc = up(per[mc]["X"]), up(per[mc]["U"])
        ev.set_mesh(mf, 0.0, LT.TF)
        ev.set_path(rungs[g]["recs"], 0, 1)
        Xf, Uf = ev.prolong(PT, Xc), ev.prolong(PT, Uc)
        ms = []
        for _ in range(5):
            ev.timer_start()
            ev.prolong(PT, Xc, Xf)
            ev.prolong(PT, Uc, Uf)
            ev.repair_guess(Xf)
            ms.append(ev.timer_stop())
        aside += statistics.median(ms) * 1e-3
    status = lambda rows: {LT.STATUS[k]: sum(q["status"] == k for q in rows) for k in range(len(LT.STATUS))}
    rec = dict(B=B, ladder=ladder, obstacles=nobs, max_iter=a.max_iter, rounds=a.rounds, warm_mu_init=WARM_MU, warm_bound_push=WARM_PUSH,
               rules=a.rules, evaluations_per_rung=[sum(q["evaluations"] for q in rows) for rows in rl],
               newton_steps_per_rung=[sum(q["newton_steps"] for q in rows) for rows in rl],
               restored_steps_per_rung=[sum(q["restored_steps"] for q in rows) for rows in rl],
               evaluations_cold_last_mesh=sum(q["evaluations"] for q in rc),
               seconds_ladder=sec["ladder"], seconds_cold_last_mesh=sec["cold"],
               ms_per_instance_ladder=1e3 * statistics.median(sec["ladder"]) / B,
               ms_per_instance_cold_last_mesh=1e3 * statistics.median(sec["cold"]) / B,
               status_per_rung=[status(rows) for rows in rl], iterations_per_rung=[sum(q["iterations"] for q in rows) for rows in rl],
               status_cold_last_mesh=status(rc), iterations_cold_last_mesh=sum(q["iterations"] for q in rc),
               seconds_prolong_and_repair=aside, share_prolong_and_repair=aside / statistics.median(sec["ladder"]))
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    ev.close()


if __name__ == "__main__":
    main()
