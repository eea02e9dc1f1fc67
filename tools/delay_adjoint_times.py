#!/usr/bin/env python3
"""The adjoint pass of contexts with delays (emi_lagr_grad_total_dev: csrc/emi_adjoint.hip) against a PyTorch formulation of the
same G on the same GPU, in ONE process, alternating rounds.  Style and yardstick of tools/adjoint_variants.py.

  python tools/delay_adjoint_times.py [--launches 100] [--rounds 3] [--out profiles/delay_adjoint_times.jsonl] [--shapes ...]

Shapes: those of tests/test_gpu_delay_adjoint.py -- the traced delay demo (2 states, 2 free controls, state horizon 3, control
horizon 1, a disc row) and the built-in quadrotor with its second control declared the delayed copy of the first.  The yardstick
is NOT the code under test: broadcast multiply-adds over VALS and torch.matmul for lamF . (D - diag D) give Gx on the extended
variables, torch.matmul with W(i dt) folds the delayed slots onto their sources.  Per shape: median of `launches` single calls by
HIP events (the library's on its context stream, torch.cuda.Event on torch's), per round; the ratio torch / hip.  The two results
are compared first.  `fold_tile` is the tile shape option of the fold product ("adj_fold_tile": 0 by size, 1 = 48 x 64, 2 = 96 x 128)."""
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
from etol_amd import workloads as W

# name -> kind, M, B
SHAPES = {"demo_33x3": ("demo", 33, 3), "demo_47x2": ("demo", 47, 2), "demo_128x20": ("demo", 128, 20), "demo_256x40": ("demo", 256, 40),
          "quad_64x1": ("quad", 64, 1), "quad_512x1024": ("quad", 512, 1024)}
DISC = np.array([[1.0, 2.0, 1.5, 0.25, 0, 0, 0, 0]])


def demo_source():
    """text of the traced delayed model as eMI355X::setup generates it (the test shim's delayed problem)"""
    h = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    h.harness_last_message.restype = C.c_char_p
    z, res, vals = np.zeros(4 * 9), np.zeros(64 * 9), np.zeros(256 * 9)
    cost, nres, nvals = C.c_double(), C.c_int(), C.c_int()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert h.harness_delay_demo(8, C.c_double(0.5), 3, 1, 0, dp(z), dp(res), res.size, dp(vals), vals.size, C.byref(cost), C.byref(nres),
                                C.byref(nvals)) == 0
    return h.harness_last_message().decode()


def slots(ns, ncf, xh, uh):
    return [(st, i) for i in range(1, xh) for st in range(ns)] + [(ns + c, i) for i in range(1, uh + 1) for c in range(ncf)]


def torch_total(VALS, lamF, lamC, sigma, Doff, Wd, ns, nc, ncf, xh, uh, npth, px, py):
    """(G[B][ns+ncf][M], Gdel[B][nc-ncf][M]) of include/emi355x.h for a model with table rows only"""
    B, _, M = VALS.shape
    nv, nf = ns + nc, ns + ncf
    Gx = sigma * VALS[:, -nv:]
    Gx = Gx + (VALS[:, :ns * nv].view(B, ns, nv, M) * lamF[:, :, None, :]).sum(1)
    Gx[:, :ns] += torch.matmul(lamF, Doff)
    if npth:
        P = VALS[:, ns * nv:ns * nv + 2 * npth].view(B, npth, 2, M)
        Gx[:, px] += (P[:, :, 0] * lamC).sum(1)
        Gx[:, py] += (P[:, :, 1] * lamC).sum(1)
    G, Gdel = Gx[:, :nf].clone(), Gx[:, nf:]
    q = 0
    for i in range(1, xh):                                   # all states against W(i dt): one matmul per delay index
        G[:, :ns] += torch.matmul(Gdel[:, q:q + ns], Wd[i - 1])
        q += ns
    for i in range(1, uh + 1):
        G[:, ns:] += torch.matmul(Gdel[:, q:q + ncf], Wd[i - 1])
        q += ncf
    return G, Gdel


def setup(kind, M, B):
    ev = E.Evaluator(0)
    if kind == "demo":
        ns, ncf, xh, uh, dt, tf = 2, 2, 3, 1, 0.2, 6.0
        ev.set_mesh(M, 0.0, tf)
        ev.set_model_source("TracedModel", demo_source(), 2, 8)
        t = ev.node_t
        rng = np.random.default_rng(M + B)
        X = np.stack([1 + 0.5 * np.sin(0.7 * t + rng.uniform(0, 3, (B, 1))), 2 - 0.1 * t + 0.3 * np.cos(t + rng.uniform(0, 3, (B, 1)))], axis=1)
        U = np.stack([0.3 * np.cos(t + rng.uniform(0, 3, (B, 1))), 0.2 + 0.1 * np.sin(2 * t + rng.uniform(0, 3, (B, 1)))], axis=1)
        recs = DISC
    else:
        ns, ncf, xh, uh, dt, tf = 6, 1, 0, 1, 0.15, W.TF
        ev.set_mesh(M, 0.0, tf)
        ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS)
        X, U, recs = W.quadrotor_batch(9, B, M, 2)
        U, recs = U[:, :1], recs[:1]
    ev.set_delays(xh, uh, dt)
    ev.set_batch(B)
    ev.set_path(recs, 0, 1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    RES, VALS, COST = ev.alloc_outputs()
    ev.eval_dev(dev(X), dev(U), RES, VALS, COST)
    ev.synchronize()
    lay = ev.layout
    g = torch.Generator(device="cpu").manual_seed(7)
    lamF = torch.randn((B, ns, M), dtype=torch.float64, generator=g).to(ev.device)
    lamC = torch.randn((B, lay.np, M), dtype=torch.float64, generator=g).to(ev.device)
    Doff = torch.from_numpy(ev.D - np.diag(np.diag(ev.D))).to(ev.device)
    nd = max(xh - 1, uh)
    Wd = np.empty((nd, M, M))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for d in range(nd):
        assert ev.lib.emi_delay_matrix(M, dp(ev.tau), dp(ev.w), 0.0, tf, (d + 1) * dt, dp(Wd[d])) == 0
    return ev, VALS, lamF, lamC, Doff, dev(Wd), (ns, lay.nc, ncf, xh, uh, lay.np)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--fold-tile", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delay_adjoint_times.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("delay_adjoint_times.py needs the GPU: a time from anywhere else says nothing")
    sigma = 0.7
    records = []
    for name in a.shapes.split(","):
        kind, M, B = SHAPES[name]
        ev, VALS, lamF, lamC, Doff, Wd, (ns, nc, ncf, xh, uh, npth) = setup(kind, M, B)
        ev.set_option("adj_fold_tile", a.fold_tile)
        kw = dict(dtype=torch.float64, device=ev.device)
        G, Gdel = torch.empty((B, ns + ncf, M), **kw), torch.empty((B, nc - ncf, M), **kw)
        hip = lambda: ev.lagr_grad_total_dev(VALS, lamF, lamC, sigma, G, Gdel)
        ref = lambda: torch_total(VALS, lamF, lamC, sigma, Doff, Wd, ns, nc, ncf, xh, uh, npth, 0, 1)
        hip()
        ev.synchronize()
        Gt, Gdt = ref()
        torch.cuda.synchronize()
        scale = float(Gt.abs().max())
        diff = max(float((G - Gt).abs().max()), float((Gdel - Gdt).abs().max()))
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
        copies = len(slots(ns, ncf, xh, uh))
        rec = dict(shape=name, B=B, M=M, ns=ns, ncf=ncf, n_delayed=nc - ncf, x_horizon=xh, u_horizon=uh, np=npth, fold_tile=a.fold_tile,
                   launches=a.launches, rounds=a.rounds, hip_ms=hip_ms, torch_ms=torch_ms, hip_ms_rounds=per_round(t_hip),
                   torch_ms_rounds=per_round(t_torch), torch_over_hip=torch_ms / hip_ms, fold_flops=2.0 * B * copies * M * M,
                   max_abs_diff_vs_torch=diff, max_abs_G=scale, timing="HIP events, one call per bracket, median",
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(rec))
        records.append(rec)
        ev.close()
        del VALS, lamF, lamC, Doff, Wd, G, Gdel, Gt, Gdt
        torch.cuda.empty_cache()
    if records:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for rec in records:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
