#!/usr/bin/env python3
"""The planned starts of a whole batch on the device (emi_start_guess_dev, EMI_START_PLANNED): what the call costs beside the
route through the host, and what the starts do to the lock-step ladder.  Nothing is gated; one JSON line goes to
profiles/start_times.jsonl.

  python tools/start_times.py [--shapes 64x33,128x65] [--obstacles 20] [--calls 9] [--ladder 33,65,129,257] [--batch 64] [--max-iter 60]

(a) Call time.  Instances of tools/lockstep_times.py (quadrotor, `--obstacles` random disc keep-outs per instance, (1, 1) -> (8, 6) in
    the box [0, 10]^2), default grid of 161 points: the median of `--calls` PLANNED calls by the context's event timer (the upload of
    the few doubles per instance included), beside the host route in wall time: B calls of emi_plan_route one after the other, the
    rows put into the straight-line array, and that array [B][ns][M] sent up.
(b) Ladder outcome.  The ladder of tools/ladder_times.py (same rungs, same options) from straight-line starts and again from PLANNED
    starts with repair on the first rung's mesh and table: status counts per rung of both runs, and how many instances end
    converged on the last rung in the one, in the other and in either -- the last is what a driver that restarts the failed
    instances from the next start could reach."""
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
import ladder_times as LdT
import lockstep_times as LT

BOX = np.array([LT.XLO[0], LT.XUP[0], LT.XLO[1], LT.XUP[1]])
ENDS = np.array([LT.X0[0], LT.X0[1], LT.XF[0], LT.XF[1]])
CLEARANCE = 0.01


def call_times(B, M, nobs, calls):
    _, _, recs = W.quadrotor_batch(3, B, M, nobs)
    ev = LT.context(M, recs)
    X, level = ev.start_guess(E.START_PLANNED, LT.X0, LT.XF, box=BOX, clearance=CLEARANCE)      # warm: the workspace
    ev.synchronize()
    ms = []
    for _ in range(calls):
        ev.timer_start()
        ev.start_guess(E.START_PLANNED, LT.X0, LT.XF, box=BOX, clearance=CLEARANCE, X=X)
        ms.append(ev.timer_stop())
    line = LT.problem(M, ev.tau)[2]
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        Xh = np.repeat(line[None], B, 0)
        for b in range(B):
            xs, ys, lv, _, _ = E.plan_route(recs[b], ENDS, ev.tau, BOX, CLEARANCE)
            if lv >= 0:
                Xh[b, 0], Xh[b, 1] = xs, ys
        Xd = torch.from_numpy(Xh).to(ev.device)
        torch.cuda.synchronize()
        host.append(time.perf_counter() - t0)
    same = bool(np.array_equal(Xd.cpu().numpy().view(np.uint8), X.cpu().numpy().view(np.uint8)))
    lv = level.cpu().numpy()
    ev.close()
    return dict(B=B, M=M, ms_device_call=ms, ms_device_call_median=statistics.median(ms), ms_host_route=[1e3 * t for t in host],
                ms_host_route_median=1e3 * statistics.median(host), same_bits=same,
                levels={str(l): int((lv == l).sum()) for l in (0, 1, 2, -1, -2)})


def ladder_outcome(B, ladder, nobs, max_iter):
    ML = ladder[-1]
    _, _, recs = W.quadrotor_batch(3, B, ML, nobs)
    ev = LT.context(ML, recs)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(ev.device)
    cl, cu = np.full(nobs, -1000.0), np.zeros(nobs)
    rungs = []
    for g, M in enumerate(ladder):
        zl, zu, X1, U1 = LT.problem(M, E.lgl(M)[0])
        if g == 0:
            X0d, U0d = up(np.repeat(X1[None], B, 0)), up(np.repeat(U1[None], B, 0))
        opt = dict(tol=1e-8, max_iter=max_iter)
        if g > 0:
            opt.update(mu_init=LdT.WARM_MU, bound_push=LdT.WARM_PUSH, bound_frac=LdT.WARM_PUSH)
        rungs.append(dict(M=M, bounds=dict(zl=up(zl), zu=up(zu), cl=cl, cu=cu), options=opt, repair=1,
                          recs=LdT.inflated(recs, M) if M != ML else recs))

    def climb(X0):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.ipm_solve_ladder(rungs, 0.0, LT.TF, X0, U0d)[4]
        ev.synchronize()
        return time.perf_counter() - t0, res

    climb(X0d)                                  # warm
    t_line, r_line = climb(X0d)
    ev.set_mesh(ladder[0], 0.0, LT.TF)
    ev.set_path(rungs[0]["recs"], 0, 1)
    Xp, level = ev.start_guess(E.START_PLANNED, LT.X0, LT.XF, box=BOX, clearance=CLEARANCE, repair=1)
    ev.synchronize()
    t_plan, r_plan = climb(Xp)
    status = lambda rows: {LT.STATUS[k]: sum(q["status"] == k for q in rows) for k in range(len(LT.STATUS))}
    ok = lambda rows, upto: np.array([q["status"] <= upto for q in rows])
    lv = level.cpu().numpy()
    ev.close()
    out = dict(B=B, ladder=ladder, max_iter=max_iter, seconds_line=t_line, seconds_planned=t_plan,
               status_per_rung_line=[status(r) for r in r_line], status_per_rung_planned=[status(r) for r in r_plan],
               iterations_per_rung_line=[sum(q["iterations"] for q in r) for r in r_line],
               iterations_per_rung_planned=[sum(q["iterations"] for q in r) for r in r_plan],
               levels={str(l): int((lv == l).sum()) for l in (0, 1, 2, -1, -2)})
    for name, upto in (("converged", 0), ("converged_or_acceptable", 1)):
        a, b = ok(r_line[-1], upto), ok(r_plan[-1], upto)
        out[name + "_last_rung"] = dict(line=int(a.sum()), planned=int(b.sum()), either=int((a | b).sum()), both=int((a & b).sum()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x33,128x65")
    ap.add_argument("--obstacles", type=int, default=20)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--ladder", default="33,65,129,257")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "start_times.jsonl"))
    a = ap.parse_args()
    rec = dict(obstacles=a.obstacles, grid=161, clearance=CLEARANCE, calls=[])
    for shape in a.shapes.split(","):
        B, M = (int(x) for x in shape.split("x"))
        rec["calls"].append(call_times(B, M, a.obstacles, a.calls))
        print(json.dumps(rec["calls"][-1]), flush=True)
    rec["ladder"] = ladder_outcome(a.batch, [int(m) for m in a.ladder.split(",")], a.obstacles, a.max_iter)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
