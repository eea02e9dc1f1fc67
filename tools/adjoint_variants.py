#!/usr/bin/env python3
"""The adjoint pass (emi_lagr_grad_dev: csrc/emi_adjoint.hip) against a PyTorch formulation of the same G on the same GPU, in ONE
process, alternating rounds.

  python tools/adjoint_variants.py [--launches 100] [--rounds 3] [--out profiles/adjoint_times.jsonl] [--shapes c3,shard,b1_129,b1_1024]
  python tools/adjoint_variants.py --trace-only       # just launches the HIP path (for rocprofv3 --kernel-trace --stats, a run of its own)

The yardstick is NOT the code under test: torch.matmul for the operator term lamF . (D - diag D) plus broadcast multiply-adds over
VALS.  Per shape: median of `launches` single launches by HIP events (the library's on its context stream, torch.cuda.Event on
torch's), per round; the ratio torch / hip; the fraction of the HBM roof (8 TB/s) on algorithmic bytes VALS + lamF + lamC + G; the
fraction of the fp64 matrix peak (78.6 TF) on the operator's 2 B ns M^2 flops.  The two results are compared first."""
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

HBM_ROOF = 8.0e12
FP64_MATRIX_PEAK = 78.6e12
SHAPES = {"c3": (1024, 1024, 20), "shard": (128, 1024, 20), "b1_129": (1, 129, 20), "b1_1024": (1, 1024, 20)}     # B, M, keep-outs


def torch_lagr_grad(VALS, lamF, lamC, sigma, Doff, ns, nc, npth, px, py):
    """G[B][nv][M] of include/emi355x.h for a built-in model (table rows only)"""
    B, _, M = VALS.shape
    nv = ns + nc
    G = sigma * VALS[:, -nv:]
    G = G + (VALS[:, :ns * nv].view(B, ns, nv, M) * lamF[:, :, None, :]).sum(1)
    G[:, :ns] += torch.matmul(lamF, Doff)
    if npth:
        P = VALS[:, ns * nv:ns * nv + 2 * npth].view(B, npth, 2, M)
        G[:, px] += (P[:, :, 0] * lamC).sum(1)
        G[:, py] += (P[:, :, 1] * lamC).sum(1)
    return G


def setup(B, M, nobs):
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, W.TF)
    ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS)
    ev.set_batch(B)
    X, U, recs = W.quadrotor_batch(3, B, M, nobs)
    ev.set_path(recs, 0, 1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    X, U = dev(X), dev(U)
    RES, VALS, COST = ev.alloc_outputs()
    ev.eval_dev(X, U, RES, VALS, COST)
    ev.synchronize()
    g = torch.Generator(device="cpu").manual_seed(7)
    lamF = torch.randn((B, 6, M), dtype=torch.float64, generator=g).to(ev.device)
    lamC = torch.randn((B, nobs, M), dtype=torch.float64, generator=g).to(ev.device)
    Doff = torch.from_numpy(ev.D - np.diag(np.diag(ev.D))).to(ev.device)
    return ev, VALS, lamF, lamC, Doff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", default="c3,shard,b1_129,b1_1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjoint_times.jsonl"))
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adjoint_variants.py needs the GPU: a time from anywhere else says nothing")
    sigma, ns, nc = 0.7, 6, 2
    records = []
    for name in a.shapes.split(","):
        B, M, nobs = SHAPES[name]
        ev, VALS, lamF, lamC, Doff = setup(B, M, nobs)
        G = torch.empty((B, ns + nc, M), dtype=torch.float64, device=ev.device)
        hip = lambda: ev.lagr_grad_dev(VALS, lamF, lamC, sigma, G)
        if a.trace_only:
            for _ in range(a.warmup + a.launches):
                hip()
            ev.synchronize()
            ev.close()
            continue
        ref = lambda: torch_lagr_grad(VALS, lamF, lamC, sigma, Doff, ns, nc, nobs, 0, 1)
        hip()
        ev.synchronize()
        Gt = ref()
        torch.cuda.synchronize()
        scale = float(Gt.abs().max())
        diff = float((G - Gt).abs().max())
        assert diff <= 1e-11 * scale, (name, diff, scale)
        for _ in range(a.warmup):
            hip()
            ref()
        ev.synchronize()
        torch.cuda.synchronize()
        t_hip, t_torch = [], []
        for _ in range(a.rounds):
            for _ in range(a.launches):
                ev.timer_start()
                hip()
                t_hip.append(ev.timer_stop())
            for _ in range(a.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ref()
                e1.record()
                e1.synchronize()
                t_torch.append(e0.elapsed_time(e1))
        per_round = lambda t: [statistics.median(t[r * a.launches:(r + 1) * a.launches]) for r in range(a.rounds)]
        hip_ms, torch_ms = statistics.median(t_hip), statistics.median(t_torch)
        nvals = ns * (ns + nc) + 2 * nobs + ns + nc
        nbytes = 8 * B * M * (nvals + ns + nobs + ns + nc)
        flops = 2.0 * B * ns * M * M
        rec = dict(shape=name, B=B, M=M, ns=ns, np=nobs, launches=a.launches, rounds=a.rounds, hip_ms=hip_ms, torch_ms=torch_ms,
                   hip_ms_rounds=per_round(t_hip), torch_ms_rounds=per_round(t_torch), torch_over_hip=torch_ms / hip_ms,
                   algorithmic_bytes=nbytes, hbm_roof_frac=nbytes / (hip_ms * 1e-3) / HBM_ROOF, operator_flops=flops,
                   fp64_matrix_peak_frac=flops / (hip_ms * 1e-3) / FP64_MATRIX_PEAK, max_abs_diff_vs_torch=diff, max_abs_G=scale,
                   timing="HIP events, one launch per bracket, median", device=torch.cuda.get_device_name(0))
        print(json.dumps(rec))
        records.append(rec)
        ev.close()
        del VALS, lamF, lamC, Doff, G, Gt
        torch.cuda.empty_cache()
    if records:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in records:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
