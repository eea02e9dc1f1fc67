#!/usr/bin/env python3
"""Wall time of one lock-step interior-point solve of a whole batch (emi_ipm_solve_shard_dev, B instances in one call) beside the
same B instances solved one after the other by the same call on a B = 1 context, on the same GPU.  Nothing is gated; one JSON
line per shape goes to profiles/lockstep_times.jsonl.

  python tools/lockstep_times.py [--shapes 64x65,64x257] [--rounds 3] [--max-iter 60] [--obstacles 20] [--rules 0,1] [--batch-only]

Problem: the quadrotor (6 states, 2 controls) from (1, 1) at rest to (8, 6) at rest in 4 s, boxes as in tests/indep_nlp.py's
quad_problem, `--obstacles` disc keep-outs per instance from workloads.quadrotor_batch (config 3), straight-line starts with
hover thrust.  Random discs may cover a boundary state: such an instance has no feasible path and, without residual-based
acceptance and the crawl rule, runs to --max-iter.  --rules lists the variants to run, each a value of
emi_ipm_options_t.rules (0: none, 1: EMI_IPM_RULE_RESIDUAL with crawl_limit 3, crawl_frac 0.3); how many instances ended in each
status, and the full steps kept / taken back on the KKT residual, are recorded beside the times.  Per shape: a warm-up call of either form, then `rounds` rounds that alternate between the two
forms; each figure is the wall time of the call(s), synchronised."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import etol_amd as E
from etol_amd import workloads as W

NS, NC, TF = 6, 2, 4.0
X0, XF = np.array([1.0, 1, 0, 0, 0, 0]), np.array([8.0, 6, 0, 0, 0, 0])
XTOL = np.array([0.01, 0.01, 0.01, 0.05, 0.05, 0.05])
XLO, XUP = np.array([0.0, 0, -1.2, -6, -6, -4]), np.array([10.0, 10, 1.2, 6, 6, 4])
ULO, UUP = np.array([0.0, -1]), np.array([25.0, 1])
STATUS = ("converged", "acceptable", "max_iter", "line_search", "infeasible", "factor", "not_finite")


def problem(M, tau):
    zl = np.concatenate([np.repeat(XLO[:, None], M, 1), np.repeat(ULO[:, None], M, 1)])
    zu = np.concatenate([np.repeat(XUP[:, None], M, 1), np.repeat(UUP[:, None], M, 1)])
    zl[:NS, 0] = zu[:NS, 0] = X0
    zl[:NS, -1], zu[:NS, -1] = np.maximum(zl[:NS, -1], XF - XTOL), np.minimum(zu[:NS, -1], XF + XTOL)
    s = (tau + 1) / 2
    X = X0[:, None] + (XF - X0)[:, None] * s[None]
    U = np.stack([np.full(M, W.QUAD_PARAMS[0] * W.QUAD_PARAMS[2]), np.zeros(M)])
    return zl[None], zu[None], X, U


def context(M, recs):
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, TF)
    ev.set_model(1, W.QUAD_PARAMS)
    ev.set_batch(recs.shape[0])
    ev.set_path(recs, 0, 1)
    return ev


def solve(ev, X, U, zl, zu, nobs, opt):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
    Xd, Ud, bd = up(X), up(U), dict(zl=up(zl), zu=up(zu), cl=np.full(nobs, -1000.0), cu=np.zeros(nobs))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, res = ev.ipm_solve_shard(Xd, Ud, bd, opt)
    ev.synchronize()
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x65,64x257")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--obstacles", type=int, default=20)
    ap.add_argument("--rules", default="0")
    ap.add_argument("--batch-only", action="store_true", help="leave out the one-by-one form (its figures are recorded as empty)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_times.jsonl"))
    a = ap.parse_args()
    for shape, rules in ((s, int(r)) for s in a.shapes.split(",") for r in a.rules.split(",")):
        opt = dict(tol=1e-8, max_iter=a.max_iter, rules=rules)
        B, M = (int(x) for x in shape.split("x"))
        _, _, recs = W.quadrotor_batch(3, B, M, a.obstacles)
        ev = context(M, recs)
        zl, zu, X1, U1 = problem(M, ev.tau)
        X, U = np.repeat(X1[None], B, 0), np.repeat(U1[None], B, 0)
        ev1 = context(M, recs[:1])

        def batch():
            return solve(ev, X, U, zl, zu, a.obstacles, opt)

        def singles():
            total, res = 0.0, []
            if a.batch_only:
                return total, res
            for b in range(B):
                ev1.set_path(recs[b:b + 1], 0, 1)
                t, r = solve(ev1, X[b:b + 1], U[b:b + 1], zl, zu, a.obstacles, opt)
                total, res = total + t, res + r
            return total, res

        batch(), singles()              # warm: buffers, workspaces, rocBLAS kernels
        sec = dict(batch=[], singles=[])
        for _ in range(a.rounds):
            tb, rb = batch()
            ts, rs = singles()
            sec["batch"].append(tb)
            sec["singles"].append(ts)
        its = [q["iterations"] for q in rb]
        rec = dict(B=B, M=M, obstacles=a.obstacles, max_iter=a.max_iter, rounds=a.rounds, rules=rules,
                   newton_steps_sum=sum(q["newton_steps"] for q in rb), restored_steps_sum=sum(q["restored_steps"] for q in rb),
                   seconds_batch=sec["batch"], seconds_one_by_one=sec["singles"],
                   ms_per_instance_batch=1e3 * statistics.median(sec["batch"]) / B,
                   ms_per_instance_one_by_one=None if a.batch_only else 1e3 * statistics.median(sec["singles"]) / B,
                   iterations=dict(min=min(its), median=statistics.median(its), max=max(its), sum=sum(its)),
                   iterations_one_by_one_sum=sum(q["iterations"] for q in rs),
                   evaluations_sum=sum(q["evaluations"] for q in rb), factorisations_sum=sum(q["factorisations"] for q in rb),
                   status_batch={STATUS[k]: sum(q["status"] == k for q in rb) for k in range(len(STATUS))},
                   status_one_by_one={STATUS[k]: sum(q["status"] == k for q in rs) for k in range(len(STATUS))})
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        ev.close()
        ev1.close()


if __name__ == "__main__":
    main()
