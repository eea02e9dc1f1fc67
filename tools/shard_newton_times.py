#!/usr/bin/env python3
"""Times of the Newton step of a context's whole batch (emi_kkt_factor_shard_dev, and factor + emi_kkt_lowrank_shard_dev +
emi_kkt_solve_refined_shard_dev) beside, in the same process, (a) B single emi_kkt_factor_dev + emi_kkt_solve_dev calls on one
B = 1 context and (b) emi_kkt_factor_batch over B contexts with host arrays.  Nothing is gated; one JSON line per shape goes to
profiles/shard_newton_times.jsonl.

  python tools/shard_newton_times.py [--shapes 64x65,64x129,16x257,8x1024] [--calls 5] [--rounds 3]

Per form and shape: the median of single calls by HIP events on the context's stream (emi_timer_*), in `rounds` rounds that
alternate between the forms.  Data: quadrotor (6 states, 2 controls), random positive definite node blocks and Jacobian entries
with diag D added, the initial state fixed, four distinct instances repeated over the batch, `--lowrank` reflected directions per
instance (0.05-scale: the verdict is "exact", the Woodbury term is applied in the refined solve).  NOT late-iteration data of a
solve: no regularisation level above the nominal one is climbed here."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import etol_amd as E
from etol_amd import _lib as L
from etol_amd import workloads as W

NS, NV, DCV = 6, 8, 1e-9


def problem(D, M, rng):
    nh = NV * (NV + 1) // 2
    A = rng.standard_normal((M, NV, NV))
    Qk = A @ A.transpose(0, 2, 1) + NV * np.eye(NV)
    Q = np.zeros((nh, M))
    for v in range(NV):
        for q in range(v + 1):
            Q[v * (v + 1) // 2 + q] = Qk[:, v, q]
    V = np.zeros((NS * NV + NV, M))
    V[:NS * NV] = rng.standard_normal((NS * NV, M))
    for i in range(NS):
        V[i * NV + i] += np.diag(D)
    F = np.zeros((NV, M), dtype=np.uint8)
    F[:NS, 0] = 1
    return Q, V, F


def context(M, B):
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, 4.0)
    ev.set_model(1, W.QUAD_PARAMS)
    ev.set_batch(B)
    return ev


def timed(ev, fn):
    ms = C.c_float()
    ev.synchronize()
    L.check(ev.lib.emi_timer_start(ev.ctx), ev.ctx, "emi_timer_start")
    fn()
    L.check(ev.lib.emi_timer_stop(ev.ctx, C.byref(ms)), ev.ctx, "emi_timer_stop")
    return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x65,64x129,16x257,8x1024")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lowrank", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shard_newton_times.jsonl"))
    a = ap.parse_args()
    lib = L.load()
    D_ = C.POINTER(C.c_double)
    dp = lambda x: x.ctypes.data_as(D_)
    ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int))
    for shape in a.shapes.split(","):
        B, M = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(100 * M + B)
        ev = context(M, B)
        probs = [problem(ev.D, M, rng) for _ in range(min(B, 4))]
        probs = [probs[b % len(probs)] for b in range(B)]
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ev.device)
        Q, V, F = (up(np.stack([p[k] for p in probs])) for k in range(3))
        r = min(a.lowrank, M - 1)
        node = np.tile(np.sort(rng.choice(np.arange(1, M), size=r, replace=False)).astype(np.int32), (B, 1))
        lists = (up(np.full(B, r, dtype=np.int32)), up(node), up(0.05 * (1 + rng.random((B, r)))), up(rng.standard_normal((B, r, NV))))
        rhs = up(rng.standard_normal((B, NV + NS, M)))
        x = torch.empty_like(rhs)
        dc = np.full(B, DCV)
        # (a) one B = 1 context, the instances one after the other; (b) B contexts, host arrays
        ev1 = context(M, 1)
        x1 = torch.empty_like(rhs[0]).reshape(-1)
        evs = [context(M, 1) for _ in range(B)]
        ctxs = (C.c_void_p * B)(*[e.ctx for e in evs])
        Qp = (D_ * B)(*[dp(p[0]) for p in probs])
        Jp = (D_ * B)(*[dp(p[1]) for p in probs])
        Fp = (C.POINTER(C.c_ubyte) * B)(*[p[2].ctypes.data_as(C.POINTER(C.c_ubyte)) for p in probs])
        info = np.zeros(B, dtype=np.int32)
        torch.cuda.synchronize()
        out = {}

        def shard_factor():
            assert not ev.kkt_factor_shard_dev(Q, V, F, dc).any()

        def shard_step():
            shard_factor()
            assert ev.kkt_lowrank_shard_dev(r, *lists).all()
            x.copy_(rhs)
            torch.cuda.synchronize()
            out["refined"] = ev.kkt_solve_refined_shard_dev(x, dc, max_steps=8)

        def singles():
            for b in range(B):
                assert ev1.kkt_factor_dev(Q[b], V[b], F[b].reshape(-1), DCV) == 0
                ev1.kkt_solve_dev(x1)

        def batch_factor():
            assert lib.emi_kkt_factor_batch(B, ctxs, Qp, Jp, Fp, dp(dc), ip(info)) == 0 and not info.any()

        forms = (("shard_factor", ev, shard_factor), ("shard_factor_lowrank_refined", ev, shard_step), ("single_factor_solve", ev1, singles),
                 ("batch_factor_host_arrays", evs[0], batch_factor))
        for _, _, fn in forms:          # warm: buffers, handles, rocBLAS kernels
            fn()
        ms = {name: [] for name, _, _ in forms}
        for _ in range(a.rounds):
            for name, e, fn in forms:
                ms[name] += [timed(e, fn) for _ in range(a.calls)]
        rec = dict(B=B, M=M, lowrank_columns=r, calls=a.calls, rounds=a.rounds,
                   ms_per_call={k: statistics.median(v) for k, v in ms.items()},
                   ms_per_instance={k: statistics.median(v) / B for k, v in ms.items()},
                   refined_solves=float(out["refined"]["nsolve"].mean()), refined_rel=float(out["refined"]["rel"].max()),
                   data="random positive definite node blocks (not late-iteration data)")
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        for e in [ev, ev1] + evs:
            e.close()


if __name__ == "__main__":
    main()
