#!/usr/bin/env python3
"""Times of the relative local ODE error of a batch on the device (emi_ode_error_dev) beside a PyTorch formulation of the same
quantity on the same GPU, and of ETOL::eMI355X::odeError per trajectory by either route.  Nothing is gated; JSON lines go to
profiles/ode_error_times.jsonl.

  python tools/ode_error_times.py [--shapes 64x65,64x257,128x1024] [--calls 100] [--rounds 3] [--nodes 41,257,1024]
  python tools/ode_error_times.py --only-calls 128x1024 --calls 30        nothing timed: the calls alone, for a profiler run of its own
  python tools/ode_error_times.py --from-stats DIR --shape 128x1024       the product kernel's share of the call and of the fp64 matrix
                                                                          peak from the kernel statistics a profiler run left in DIR

Device call: quadrotor, B instances of the seeded synthetic batch on M nodes, control bounds given; the median of `calls` single calls
by HIP events on the context's stream (emi_timer_*), `rounds` rounds alternating with the baseline.  Baseline: torch.matmul with E, E'
and D (the library's operator, uploaded once), the clip, emi_eval_dev (values only) on a second context with a points-only mesh of the
5 (M-1) points that shares torch's stream, then torch reductions; the median of `calls` single evaluations by torch events.  Per
trajectory: the mean wall time of odeError over 10 calls on one solver (tests/harness: harness_ode_error_quadrotor_seconds) with
Alg::ode_error "host" and "device", the first call of each left out."""
import argparse
import csv
import ctypes as C
import glob
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

T0, TF = 0.0, W.TF
UL, UU = np.array([0.0, -1.0]), np.array([25.0, 1.0])
PEAK_F64_MATRIX = 78.6e12
GW = np.polynomial.legendre.leggauss(5)[1]


def product_flops(B, M, ns=6, nc=2):
    npts = 5 * (M - 1)
    return 2.0 * B * M * (ns * (2 * npts + M) + nc * npts)


def contexts(B, M):
    ev = E.Evaluator(0)
    ev.set_mesh(M, T0, TF)
    ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS)
    ev.set_batch(B)
    Eo, Ed, tq = E.Evaluator.ode_error_operator(M)
    pts = E.Evaluator(0)                    # points-only mesh, on torch's stream
    pts.use_stream(torch.cuda.current_stream().cuda_stream)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    wq = np.zeros(len(tq))
    pts._ck(pts.lib.emi_set_mesh(pts.ctx, len(tq), dp(tq), dp(wq), None, T0, TF), "emi_set_mesh (points)")
    pts._changed()
    pts.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS)
    pts.set_batch(B)
    return ev, pts, Eo, Ed


def run_shape(B, M, calls, rounds, only_calls=False):
    X, U, _ = W.quadrotor_batch(5, B, M, 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    ev, pts, Eo, Ed = contexts(B, M)
    Xd, Ud = up(X), up(U)
    torch.cuda.synchronize()
    if only_calls:
        for _ in range(calls):
            ev.ode_error(Xd, Ud, UL, UU, eta=False)
        ev.synchronize()
        ev.close(); pts.close()
        return None
    h, nq, P = (TF - T0) / 2, M - 1, 5 * (M - 1)
    ET, EdT, DT = up(Eo.T), up(Ed.T), up(ev.D.T)
    lo, hi = up(UL)[None, :, None], up(UU)[None, :, None]
    half, g = up(0.5 * np.diff(ev.tau) * h), up(GW)[None, None, :, None]
    RES = torch.empty((B, 6, P), dtype=torch.float64, device="cuda")
    COST = torch.empty(B, dtype=torch.float64, device="cuda")

    def baseline():
        Xq = (Xd @ ET).contiguous()
        Uq = torch.minimum(torch.maximum(Ud @ ET, lo), hi).contiguous()
        dXq = (Xd @ EdT) / h
        DX = Xd @ DT
        pts.eval_dev(Xq, Uq, RES, None, COST, flags=E.EVAL_NODES | E.EVAL_NOJAC)
        resid = (dXq + RES / h).abs().reshape(B, 6, 5, nq)              # the defect rows of a points-only mesh hold -h f
        eta = half * (g * resid).sum(2)
        Wt = torch.maximum(Xd.abs().amax(2), DX.abs().amax(2) / h)
        return (eta / (Wt[:, :, None] + 1)).amax((1, 2))

    def time_device():
        ms = []
        for _ in range(calls):
            ev.timer_start()
            ev.ode_error(Xd, Ud, UL, UU, eta=False)
            ms.append(ev.timer_stop())
        return statistics.median(ms)

    def time_baseline():
        ms = []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            baseline()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    err = ev.ode_error(Xd, Ud, UL, UU, eta=False)[0]
    ev.synchronize()
    ref = baseline()
    torch.cuda.synchronize()
    agree = float(((err - ref).abs() / ref.abs()).max())
    for _ in range(5):                      # warm-up of both
        ev.ode_error(Xd, Ud, UL, UU, eta=False)
        baseline()
    torch.cuda.synchronize()
    dev, base = [], []
    for _ in range(rounds):
        dev.append(time_device())
        base.append(time_baseline())
    rec = dict(what="device call", model="quadrotor", B=B, M=M, calls=calls, rounds=rounds, ms_device=dev, ms_pytorch=base,
               ms_device_median=statistics.median(dev), ms_pytorch_median=statistics.median(base),
               ratio=statistics.median(base) / statistics.median(dev), product_gflop=product_flops(B, M) / 1e9,
               ms_product_at_matrix_peak=1e3 * product_flops(B, M) / PEAK_F64_MATRIX, largest_relative_difference_of_err=agree)
    ev.close(); pts.close()
    return rec


def per_trajectory(M, reps=10):
    H = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    D_ = C.POINTER(C.c_double)
    H.harness_ode_error_quadrotor_seconds.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, D_, D_, D_, D_]
    X, U, _ = W.quadrotor_batch(5, 1, M, 0)
    X, U = np.ascontiguousarray(X[0]), np.ascontiguousarray(np.clip(U[0], UL[:, None], UU[:, None]))
    out = {}
    for route, name in ((0, "host"), (1, "device")):
        err, sec = C.c_double(), C.c_double()
        assert H.harness_ode_error_quadrotor_seconds(M - 1, TF / (M - 1), route, reps, X.ctypes.data_as(D_), U.ctypes.data_as(D_), C.byref(err),
                                                     C.byref(sec)) == 0
        out[name] = dict(ms=1e3 * sec.value, err=err.value)
    return dict(what="odeError per trajectory", model="quadrotor", B=1, M=M, reps=reps, ms_host_route=out["host"]["ms"],
                ms_device_route=out["device"]["ms"], err_host_route=out["host"]["err"], err_device_route=out["device"]["err"])


def from_stats(directory, B, M):
    """kernel statistics of a profiler run of --only-calls: total time per kernel name"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    assert files, f"no kernel statistics under {directory}"
    ns_by = {}
    calls_by = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Name"]
        key = next((k for k in ("emi_interp_op_kernel", "emi_ode_resid_kernel", "emi_ode_finish_kernel", "emi_ode_copy_D_kernel") if k in name), None)
        if key:
            ns_by[key] = ns_by.get(key, 0.0) + float(row["TotalDurationNs"])
            calls_by[key] = calls_by.get(key, 0) + int(row["Calls"])
    total = sum(v for k, v in ns_by.items() if k != "emi_ode_copy_D_kernel")
    ncalls = calls_by["emi_ode_finish_kernel"]
    prod_ms = 1e-6 * ns_by["emi_interp_op_kernel"] / ncalls                 # both launches of a call (state rows, control rows)
    return dict(what="kernels of the call (profiler run of its own)", model="quadrotor", B=B, M=M, calls=ncalls,
                ms_per_call={k: 1e-6 * v / ncalls for k, v in ns_by.items() if k != "emi_ode_copy_D_kernel"},
                product_share_of_kernel_time=ns_by["emi_interp_op_kernel"] / total,
                product_tflops=product_flops(B, M) / (prod_ms * 1e-3) / 1e12,
                product_fraction_of_matrix_peak=product_flops(B, M) / (prod_ms * 1e-3) / PEAK_F64_MATRIX)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x65,64x257,128x1024")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nodes", default="41,257,1024")
    ap.add_argument("--only-calls", default="")
    ap.add_argument("--from-stats", default="")
    ap.add_argument("--shape", default="128x1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ode_error_times.jsonl"))
    a = ap.parse_args()
    shape = lambda s: tuple(int(v) for v in s.split("x"))
    if a.only_calls:
        run_shape(*shape(a.only_calls), a.calls, 0, only_calls=True)
        return
    recs = []
    if a.from_stats:
        recs.append(from_stats(a.from_stats, *shape(a.shape)))
    else:
        assert torch.cuda.is_available(), "needs the GPU"
        for s in a.shapes.split(","):
            recs.append(run_shape(*shape(s), a.calls, a.rounds))
        for m in (int(v) for v in a.nodes.split(",") if v):
            recs.append(per_trajectory(m))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for r in recs:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
