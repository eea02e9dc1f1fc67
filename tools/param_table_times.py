#!/usr/bin/env python3
"""What a per-instance parameter table (emi_set_model_params_batch) costs an evaluation pass, in ONE process, alternating rounds.

  python tools/param_table_times.py [--window 0.3] [--rounds 5] [--out profiles/param_table_times.jsonl] [--batches 1024,128]

Shape: config 3 of bench.py -- the quadrotor at 1024 nodes with 20 keep-outs per instance (a per-instance record table) -- at
B = 1024 and B = 128.  Three contexts on the same inputs:
   (a) default     the default plan, no table (the one-launch pass);
   (b) sequential  option "overlap" 0, no table (node kernel, then defect kernel: the route a table takes);
   (c) table       a table of B distinct rows (every parameter of the nominal set scaled by a seeded factor in [0.8, 1.25]).
Per round, the three in turn: a timed region of `window` seconds of back-to-back emi_eval_dev calls between two HIP events on the
context's stream (the library's timer), ms per pass = elapsed / calls.  Reported: the median over the rounds, min and max (the
spread), c / b (the claim: within b's own round-to-round spread -- the tabled kernels read their row by scalar loads and are
otherwise the untabled ones) and c / a (the price of leaving the one-launch pass).  Before timing, instance 0 and B - 1 of (c) are
compared with a context that holds that row as its shared set under "overlap" 0: the bits must be equal."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import etol_amd as E
from etol_amd import workloads as W

M, NOBS = 1024, 20


def rows_for(B, seed=7):
    rng = np.random.default_rng(seed)
    rows = np.array(W.QUAD_PARAMS)[None, :] * rng.uniform(0.8, 1.25, (B, 5))
    rows[0] = W.QUAD_PARAMS
    return np.ascontiguousarray(rows)


def context(B, recs, params=W.QUAD_PARAMS, overlap0=False, table=None):
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, W.TF)
    ev.set_model(E.MODEL_QUADROTOR2D, params)
    ev.set_batch(B)
    ev.set_path(recs, 0, 1)
    if overlap0:
        ev.set_option("overlap", 0)
    if table is not None:
        ev.set_model_params(table)
    return ev


def region(ev, dX, dU, outs, calls):
    ev.timer_start()
    for _ in range(calls):
        ev.eval_dev(dX, dU, *outs)
    return ev.timer_stop() / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed region")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", default="1024,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_table_times.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("param_table_times.py needs the GPU: a time from anywhere else says nothing")
    lines = []
    for B in (int(b) for b in a.batches.split(",")):
        X, U, recs = W.quadrotor_batch(3, B, M, NOBS)
        rows = rows_for(B)
        ctx = dict(default=context(B, recs), sequential=context(B, recs, overlap0=True), table=context(B, recs, table=rows))
        dX, dU = (torch.from_numpy(np.ascontiguousarray(v)).to(ctx["default"].device) for v in (X, U))
        outs = {k: ev.alloc_outputs() for k, ev in ctx.items()}
        torch.cuda.synchronize()
        # what is timed computes what it should: instances 0 and B - 1 of the tabled context against the shared set of that row
        ctx["table"].eval_dev(dX, dU, *outs["table"])
        ctx["table"].synchronize()
        got = [t.cpu().numpy() for t in outs["table"]]
        for b in (0, B - 1):
            ref = context(B, recs, params=rows[b], overlap0=True)
            ro = ref.alloc_outputs()
            ref.eval_dev(dX, dU, *ro)
            ref.synchronize()
            for g, r in zip(got, ro):
                assert np.ascontiguousarray(g[b]).tobytes() == np.ascontiguousarray(r[b].cpu().numpy()).tobytes(), ("bits differ", B, b)
            ref.close()
        plans = {k: ev.plan() for k, ev in ctx.items()}
        kernels, calls = {}, {}
        for k, ev in ctx.items():           # warm-up, and the number of calls that fill the window
            for _ in range(20):
                ev.eval_dev(dX, dU, *outs[k])
            ev.synchronize()
            kernels[k] = ev.last_defect_kernel
            ms = region(ev, dX, dU, outs[k], 50)
            calls[k] = max(50, int(a.window * 1e3 / ms))
        ms = {k: [] for k in ctx}
        for _ in range(a.rounds):           # alternating: one region of each per round
            for k, ev in ctx.items():
                ms[k].append(region(ev, dX, dU, outs[k], calls[k]))
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = dict(shape=f"quadrotor M {M}, {NOBS} keep-outs per instance", B=B, M=M, rounds=a.rounds, window_s=a.window, calls_per_region=calls,
                    ms_per_pass={k: dict(median=med[k], min=min(v), max=max(v), rounds=v) for k, v in ms.items()},
                    spread_rel={k: (max(v) - min(v)) / med[k] for k, v in ms.items()},
                    table_over_sequential=med["table"] / med["sequential"], table_over_default=med["table"] / med["default"],
                    sequential_over_default=med["sequential"] / med["default"],
                    one_launch={k: p["one_launch"] for k, p in plans.items()}, defect_kernel=kernels,
                    node_evals_per_s={k: B * M / (med[k] * 1e-3) for k in med},
                    timing="HIP events on the context's stream around a region of back-to-back emi_eval_dev calls; median of alternating rounds",
                    bits="instances 0 and B - 1 of the tabled context equal the shared-set context of that row under overlap 0",
                    device=torch.cuda.get_device_name(0))
        print(json.dumps({k: line[k] for k in ("B", "table_over_sequential", "table_over_default", "spread_rel")} | {"median_ms": med}))
        lines.append(line)
        for ev in ctx.values():
            ev.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
