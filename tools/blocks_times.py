#!/usr/bin/env python3
"""Times of the node-block stage of the Newton step (emi_kkt_blocks_dev: csrc/emi_kkt_blocks.hip) beside the host loop it
replaces, and of solve() in both Alg::node_blocks modes.  Nothing is gated; records go to profiles/blocks_times.jsonl.

  python tools/blocks_times.py --part device   [--launches 100] [--rounds 3]
  python tools/blocks_times.py --part solve    [--rounds 2]
  python tools/blocks_times.py --part default  --label NAME [--harness PATH/libetol_harness.so]

device   the emi_kkt_blocks_dev call: median of `launches` single calls by HIP events on the context's stream, per round, at
         (quadrotor: 8 variables, 20 keep-outs, 1024 nodes) and (fixed wing: 16 variables, 129 nodes), batches of 1 and 64, once
         with the blocks of the LAST iteration of a solve of that problem (H, VALS at the returned point and multipliers; the
         barrier terms rebuilt from complementarity at the final barrier parameter: late_iteration below) and once with synthetic
         blocks that ALL fail the screen (tests/blocks_ref.py kind "indefinite").  Beside it, alternating with it in every round, the
         host loop (assemble_node_blocks + convexify_node_blocks through the test shim) on the same arrays on one core.
         One instance is generated and repeated over the batch.
solve    the 41-node quadrotor, the 49-node fixed wing (the problems of tests/test_gpu_solve_device_blocks.py) and the 1024-node
         quadrotor with 20 keep-outs through the test shim, Alg::node_blocks "host" and "device" alternating:
         wall seconds, iterations, factorisations and Sol::nlp_runs' t_blocks / t_factor summed over the meshes.
default  the default solve() of that problem (tests/harness: harness_solve_quadrotor) in THIS process, wall seconds; --harness
         points at the shim of another build of the library (the parent commit's, say) so that a job can alternate the two in
         separate processes; --label names the build in the record."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
UP = C.POINTER(C.c_ubyte)
HARNESS = os.path.join(ROOT, "tests", "harness", "libetol_harness.so")
# name -> nv, ns, model, np, M, and the solve whose last iteration gives the blocks: (problem, nsteps, horizon, n) of the test shim
SHAPES = {"quadrotor_1024": (8, 6, 1, 20, 1024, (1, 1023, 4.0, 20.0)), "fixedwing_129": (16, 12, 2, 0, 129, (2, 128, 12.0, 20.0))}


def write(out, recs):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        for r in recs:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


def late_iteration(h, problem, nsteps, horizon, n, model, rows):
    """The block terms of the LAST iteration of a solve, rebuilt from what the solve returns (tests/harness/etol_harness_certify.cpp):
    H from emi_hess_host and VALS from emi_eval_host at the returned trajectory and multipliers; the barrier diagonal of a
    variable and the weight of an eliminated path row from complementarity at the barrier parameter the iteration ends with,
    mu = nlp_tolerance / 10:  Sigma = mu / (z - zl)^2 + mu / (zu - z)^2,  sig_t = mu / (c - cl)^2 + mu / (cu - c)^2 (elastics at their
    floor); variables with zl == zu are fixed."""
    h.harness_cs_solve.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_double, C.c_int]
    h.harness_cs_get.argtypes = [C.c_char_p, DP, C.c_int]
    h.harness_cs_message.restype = C.c_char_p
    if h.harness_cs_solve(problem, b"", nsteps, horizon, n, 0) != 0:
        raise SystemExit(h.harness_cs_message().decode())

    def get(name):
        k = h.harness_cs_get(name.encode(), None, 0)
        x = np.zeros(max(k, 1))
        h.harness_cs_get(name.encode(), x.ctypes.data_as(DP), k)
        return x[:k]

    dims, stats = get("dims"), get("stats")
    ns, nc, npth, M = (int(v) for v in dims[:4])
    nv = ns + nc
    X, U = get("X").reshape(1, ns, M), get("U").reshape(1, nc, M)
    lamF, lamC = get("lamF").reshape(1, ns, M), get("lamC").reshape(1, npth, M)
    zl, zu, cl, cu = get("zl").reshape(nv, M), get("zu").reshape(nv, M), get("cl"), get("cu")
    recs, params = get("recs"), get("params")
    h.harness_cs_release()
    import etol_amd as E
    ev = E.Evaluator(0)
    ev.set_mesh(M, dims[8], dims[9])
    ev.set_model(model, params)
    ev.set_batch(1)
    if npth:
        ev.set_path(recs.reshape(npth, -1), int(dims[5]), int(dims[6]))
    RES, VALS, _ = ev.eval_host(X, U)
    H = ev.hess_host(X, U, lamF, lamC if npth else None, 1.0)
    ev.close()
    mu = stats[5] / 10.0
    z = np.concatenate([X[0], U[0]])
    fixed = (zl == zu).astype(np.uint8)
    side = lambda gap, has: np.where(has, mu / np.maximum(gap, 1e-12) ** 2, 0.0)
    Sigma = np.where(fixed != 0, 0.0, side(z - zl, zl > -1e19) + side(zu - z, zu < 1e19))
    c = RES[0, ns:]
    SigT = side(c - cl[:, None], (cl > -1e19)[:, None]) + side(cu[:, None] - c, (cu < 1e19)[:, None]) if npth else np.zeros((0, M))
    return dict(kind="late iteration", nv=nv, ns=ns, M=M, B=1, np=npth, rows=rows, dw=0.0, H=H, VALS=VALS, Sigma=Sigma[None], SigT=SigT[None],
                fixed=fixed[None])


def part_device(a):
    import blocks_ref as R
    import etol_amd as E
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    h = C.CDLL(HARNESS)
    h.harness_blocks_host.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, IP, DP, DP, DP, DP, UP, C.c_double, DP, DP, C.c_int, IP, IP, DP, DP, DP]
    recs = []
    for name, (nv, ns, model, npth, M, slv) in SHAPES.items():
        nh = nv * (nv + 1) // 2
        for data in ("late_iteration", "all_failing"):
            if data == "late_iteration":
                one = late_iteration(h, *slv, model, R.default_rows(ns, nv, npth))
                assert (one["nv"], one["M"], one["np"]) == (nv, M, npth)
            else:
                one = R.make_case("indefinite", nv, ns, M, 1, npth, 31 * M + nv, dw=1e-4, fixed_patterns=False)
            ptr, var, ent = R.rows_csr(one["rows"])
            for B in (1, 64):
                ev = E.Evaluator(0)
                ev.set_mesh(M, 0.0, 4.0)
                ev.set_model(model, {1: W.QUAD_PARAMS, 2: W.FW_PARAMS}[model])
                ev.set_batch(B)
                if npth:
                    _, _, recs_p = W.quadrotor_batch(3, 1, M, npth)
                    ev.set_path(recs_p[0], 0, 1)
                rep = lambda x: np.ascontiguousarray(np.repeat(x, B, axis=0))
                t = lambda x: torch.from_numpy(rep(x)).to(ev.device)
                H, V, Sg, fx = t(one["H"]), t(one["VALS"]), t(one["Sigma"]), t(one["fixed"])
                St = t(one["SigT"]) if npth else None
                kw = dict(device=ev.device)
                mm = 4096
                Q, Qx = torch.zeros((B, nh, M), dtype=torch.float64, **kw), torch.zeros((B, nh, M), dtype=torch.float64, **kw)
                count, node = torch.zeros((B,), dtype=torch.int32, **kw), torch.zeros((B, mm), dtype=torch.int32, **kw)
                delta, vec = torch.zeros((B, mm), dtype=torch.float64, **kw), torch.zeros((B, mm, nv), dtype=torch.float64, **kw)
                worst = torch.zeros((B,), dtype=torch.float64, **kw)
                torch.cuda.synchronize()
                call = lambda: ev.kkt_blocks_dev(H, V, Sg, St, fx, one["dw"], Q, mm, count, node, delta, vec, worst, Qexact=Qx)

                def host():     # the host loop over the B instances, one core
                    dp = lambda x: x.ctypes.data_as(DP)
                    Hh, Vh, Sh, Th, Fh = (np.ascontiguousarray(one[n][0]) for n in ("H", "VALS", "Sigma", "SigT", "fixed"))
                    q0, q1 = np.zeros((nh, M)), np.zeros((nh, M))
                    nd, dl, vc = np.zeros(mm, dtype=np.int32), np.zeros(mm), np.zeros((mm, nv))
                    cnt, wst = C.c_int(), C.c_double()
                    t0 = time.perf_counter()
                    for _ in range(B):
                        h.harness_blocks_host(nv, M, npth, ptr.ctypes.data_as(IP), var.ctypes.data_as(IP), ent.ctypes.data_as(IP), dp(Hh), dp(Vh),
                                              dp(Sh), dp(Th), Fh.ctypes.data_as(UP), one["dw"], dp(q0), dp(q1), mm, C.byref(cnt),
                                              nd.ctypes.data_as(IP), dp(dl), dp(vc), C.byref(wst))
                    return (time.perf_counter() - t0) * 1e3, cnt.value

                for _ in range(10):
                    call()
                ev.synchronize()
                t_dev, t_host = [], []
                for _ in range(a.rounds):
                    for _ in range(a.launches):
                        ev.timer_start()
                        call()
                        t_dev.append(ev.timer_stop())
                    ms, pairs_host = host()
                    t_host.append(ms)
                failing = int(torch.count_nonzero((Q != Qx).any(dim=1))) if B == 1 else None
                med = lambda x: [statistics.median(x[r * a.launches:(r + 1) * a.launches]) for r in range(a.rounds)]
                recs.append(dict(part="device", shape=name, data=data, nv=nv, np=npth, M=M, B=B, launches=a.launches, rounds=a.rounds,
                                 dev_ms=statistics.median(t_dev), dev_ms_rounds=med(t_dev), host_ms=statistics.median(t_host),
                                 host_ms_rounds=t_host, host_over_dev=statistics.median(t_host) / statistics.median(t_dev),
                                 pairs_per_instance=int(count[0]), pairs_per_instance_host=pairs_host, blocks_changed_per_instance=failing,
                                 blocks_per_instance=M,
                                 timing="device: HIP events, one call per bracket, median; host: wall time of the loop over B instances, one core",
                                 device=torch.cuda.get_device_name(0)))
                print(json.dumps(recs[-1]))
                ev.close()
    return recs


def part_solve(a):
    h = C.CDLL(HARNESS)
    h.harness_blk_solve.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double]
    h.harness_blk_get.argtypes = [C.c_char_p, DP, C.c_int]
    h.harness_blk_message.restype = C.c_char_p

    def get(name):
        n = h.harness_blk_get(name.encode(), None, 0)
        x = np.zeros(max(n, 1))
        h.harness_blk_get(name.encode(), x.ctypes.data_as(DP), n)
        return x[:n]

    # the two problems of tests/test_gpu_solve_device_blocks.py (their iteration counts in both modes belong in the profile), then
    # the 1024-node one
    problems = [("quadrotor_41_2_keepouts", 1, 40, 4.0, 2.0, 1e-8), ("fixedwing_49", 2, 48, 8.0, 10.0, 1e-8),
                ("quadrotor_1024_20_keepouts", 1, 1023, 4.0, 20.0, -1.0)]
    recs = []
    for rnd in range(a.rounds):
      for pname, prob, nsteps, horizon, n, tol in problems:
        for mode in (0, 1):
            t0 = time.perf_counter()
            rc = h.harness_blk_solve(prob, nsteps, horizon, n, mode, tol)
            wall = time.perf_counter() - t0
            if rc != 0:
                raise SystemExit(h.harness_blk_message().decode())
            runs, stats, on = get("runs").reshape(-1, 6), get("stats"), get("on_device")
            h.harness_blk_release()
            recs.append(dict(part="solve", problem=pname, nlp_tolerance=stats[5], node_blocks="device" if mode else "host", round=rnd,
                             wall_s=wall, cost=stats[0], iterations_total=int(stats[1]), kkt_error=stats[3], node_blocks_used_device=bool(on[1]),
                             meshes=[int(x) for x in runs[:, 0]], t_blocks_s=float(runs[:, 3].sum()), t_factor_s=float(runs[:, 4].sum()),
                             factorisations=int(runs[:, 5].sum()), t_blocks_last_mesh_s=float(runs[-1, 3]),
                             factorisations_last_mesh=int(runs[-1, 5]), device=torch.cuda.get_device_name(0)))
            print(json.dumps(recs[-1]))
    return recs


def part_default(a):
    h = C.CDLL(a.harness)
    n = 1023
    h.harness_solve_quadrotor.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, DP, IP, DP, DP, C.c_int, IP, IP, DP]
    h.harness_last_message.restype = C.c_char_p
    cap = 1100
    X, U = np.zeros(6 * cap), np.zeros(2 * cap)
    cost, M, it, mesh, oerr = C.c_double(), C.c_int(), C.c_int(), C.c_int(), C.c_double()
    recs = []
    for rep in range(a.rounds):
        t0 = time.perf_counter()
        rc = h.harness_solve_quadrotor(n, 4.0 / n, 20, 1e-8, 0, 0, 1e-4, C.byref(cost), C.byref(M), X.ctypes.data_as(DP), U.ctypes.data_as(DP), cap,
                                       C.byref(it), C.byref(mesh), C.byref(oerr))
        wall = time.perf_counter() - t0
        if rc != 0:
            raise SystemExit(h.harness_last_message().decode())
        recs.append(dict(part="default", build=a.label, problem="quadrotor_1024_20_keepouts", repeat=rep, wall_s=wall, cost=cost.value,
                         iterations_last_mesh=it.value, meshes=mesh.value, device=torch.cuda.get_device_name(0)))
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("device", "solve", "default"), required=True)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="this")
    ap.add_argument("--harness", default=HARNESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks_times.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blocks_times.py needs the GPU: a time from anywhere else says nothing")
    write(a.out, {"device": part_device, "solve": part_solve, "default": part_default}[a.part](a))


if __name__ == "__main__":
    main()
