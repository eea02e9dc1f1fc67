#!/usr/bin/env python3
"""Times of the batched interior-point arithmetic (emi_ipm_*: csrc/emi_ipm.hip) beside (a) the host functions it restates
(mi355x::ipm_*, through the test shim, one core) and (b) a PyTorch formulation of the same arithmetic on the same GPU.
Nothing is gated; records go to profiles/ipm_times.jsonl.

  python tools/ipm_times.py [--launches 100] [--rounds 3] [--shapes quadrotor_1024,fixedwing_129]

Per call and shape: the median of `launches` single calls by HIP events on the context's stream, in `rounds` rounds that alternate
with the two comparisons.  Shapes: quadrotor (8 variables, 20 path rows) at 1024 nodes, batches of 1, 64 and 1024; fixed wing
(16 variables) at 129 nodes, batches of 1 and 64.  One generated instance (tests/ipm_ref.py) is repeated over the batch.  The
host functions are timed INSIDE the shim (a C++ loop around the ipm_* calls alone, no marshalling) on one instance and scaled to the
batch (they are linear in it).  Beside every time: the algorithmic bytes
of the call from the layouts of include/emi355x.h (every array the call reads or writes, once) and the fraction of 8 TB/s they
amount to -- to set beside the 0.62 - 0.67 of the adjoint's node kernel at B = 1024."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

SHAPES = {"quadrotor_1024": (8, 6, 20, 1024, (1, 64, 1024)), "fixedwing_129": (16, 12, 0, 129, (1, 64))}
HBM = 8e12


def call_bytes(nv, ns, npth, nvals, M, B, nsets=1):
    """algorithmic bytes per call: doubles read + written, each array once"""
    row, var, st, kkt = npth * M * B, nv * M * B, ns * M * B, (nv + ns) * M * B
    bnd, res, vals = 2 * nsets * nv * M, (ns + npth) * M * B, nvals * M * B
    point, duals = var + 3 * row, st + 2 * var + 5 * row
    d = dict(reduce=point + duals + res + vals + var + bnd + (var + 4 * row + kkt),
             expand=point + duals + vals + bnd + 4 * row + 2 * kkt + (8 * row + 2 * var),
             trial=2 * point + var + 3 * row,
             merit=point + res + bnd + row,
             accept=3 * point + 2 * duals + (st + 2 * var + 5 * row) + bnd,
             error=point + duals + res + var + bnd)
    return {k: 8 * v for k, v in d.items()}


def torch_forms(c, t):
    """the six calls as tensor expressions (default rows: two partials per row, on variables 0 and 1); t: name -> device tensor"""
    ns, nv, npth = c["ns"], c["nv"], c["np"]
    INF = 1e19
    z = lambda p: torch.cat([p["X"], p["U"]], 1)
    mu, rho, tau, nu = (t["par"][:, i][:, None, None] for i in range(4))
    zl, zu = t["zl"], t["zu"]
    free, hL, hU = zu > zl, zl > -INF, zu < INF
    if npth:
        hasL, hasU = t["hasL"], t["hasU"]
        lo, hi, cs = t["lo"], t["hi"], t["cs"]
        e0 = ns * nv
        Vx, Vy = t["VALS"][:, e0:e0 + 2 * npth:2] * cs, t["VALS"][:, e0 + 1:e0 + 2 * npth:2] * cs

    def reduce():
        out = {}
        zz = z(t)
        gm, gp = zz - zl, zu - zz
        out["Sigma"] = torch.where(free & hL, t["ZL"] / gm, 0.0) + torch.where(free & hU, t["ZU"] / gp, 0.0)
        rhs = -(t["G"] - torch.where(hL, mu / gm, 0.0) + torch.where(hU, mu / gp, 0.0))
        if npth:
            s, e1, e2, y = t["S"], t["E1"], t["E2"], t["Y"]
            gL, gU = s - lo, hi - s
            sg = torch.where(hasL, t["VL"] / gL, 0.0) + torch.where(hasU, t["VU"] / gU, 0.0)
            rh = -y - torch.where(hasL, mu / gL, 0.0) + torch.where(hasU, mu / gU, 0.0)
            a1, a2 = e1 / t["W1"], e2 / t["W2"]
            out["SigS"], out["RhatS"] = sg, rh
            out["SigT"] = 1.0 / (1.0 / sg + a1 + a2)
            out["Rt"] = cs * t["RES"][:, ns:] - s - e1 + e2 + rh / sg - a1 * (y - rho + mu / e1) - a2 * (y + rho - mu / e2)
            w = out["SigT"] * out["Rt"]
            rhs = rhs.clone()
            rhs[:, 0] -= (Vx * w).sum(1)
            rhs[:, 1] -= (Vy * w).sum(1)
        out["Rhs"] = torch.cat([torch.where(free, rhs, 0.0), -t["RES"][:, :ns]], 1)
        return out

    def expand(el, dzlam):
        zz = z(t)
        gm, gp = zz - zl, zu - zz
        dz = torch.where(free, dzlam[:, :nv], 0.0)
        dzL = torch.where(free & hL, mu / gm - t["ZL"] - t["ZL"] / gm * dz, 0.0)
        dzU = torch.where(free & hU, mu / gp - t["ZU"] + t["ZU"] / gp * dz, 0.0)
        big = torch.full_like(dz, float("inf"))
        pr = [torch.where(free & hL & (dz < 0), -tau * gm / dz, big), torch.where(free & hU & (dz > 0), tau * gp / dz, big)]
        du = [torch.where(dzL < 0, -tau * t["ZL"] / dzL, big), torch.where(dzU < 0, -tau * t["ZU"] / dzU, big)]
        gf = t["VALS"][:, -nv:] - torch.where(hL, mu / gm, 0.0) + torch.where(hU, mu / gp, 0.0)
        dphi = torch.where(free, gf * dz, 0.0).sum((1, 2))
        mmax = (t["LamF"] + dzlam[:, nv:]).abs().amax((1, 2))
        if npth:
            s, e1, e2, y = t["S"], t["E1"], t["E2"], t["Y"]
            gL, gU = s - lo, hi - s
            dy = el["SigT"] * (Vx * dz[:, 0:1] + Vy * dz[:, 1:2] + el["Rt"])
            ds = (dy - el["RhatS"]) / el["SigS"]
            de1 = e1 / t["W1"] * (dy + y - rho + mu / e1)
            de2 = e2 / t["W2"] * (-dy - y - rho + mu / e2)
            dvL = torch.where(hasL, mu / gL - t["VL"] - t["VL"] / gL * ds, 0.0)
            dvU = torch.where(hasU, mu / gU - t["VU"] + t["VU"] / gU * ds, 0.0)
            dw1 = mu / e1 - t["W1"] - t["W1"] / e1 * de1
            dw2 = mu / e2 - t["W2"] - t["W2"] / e2 * de2
            bigr = torch.full_like(ds, float("inf"))
            pr += [torch.where(hasL & (ds < 0), -tau * gL / ds, bigr), torch.where(hasU & (ds > 0), tau * gU / ds, bigr),
                   torch.where(de1 < 0, -tau * e1 / de1, bigr), torch.where(de2 < 0, -tau * e2 / de2, bigr)]
            du += [torch.where(dvL < 0, -tau * t["VL"] / dvL, bigr), torch.where(dvU < 0, -tau * t["VU"] / dvU, bigr),
                   torch.where(dw1 < 0, -tau * t["W1"] / dw1, bigr), torch.where(dw2 < 0, -tau * t["W2"] / dw2, bigr)]
            g = -torch.where(hasL, mu / gL, 0.0) + torch.where(hasU, mu / gU, 0.0)
            dphi = dphi + (g * ds + (rho - mu / e1) * de1 + (rho - mu / e2) * de2).sum((1, 2))
            mmax = torch.maximum(mmax, (y + dy).abs().amax((1, 2)))
        apr = torch.stack([x.amin((1, 2)) for x in pr]).amin(0).clamp(max=1.0)
        adu = torch.stack([x.amin((1, 2)) for x in du]).amin(0).clamp(max=1.0)
        return torch.stack([apr, adu, dphi, mmax], 1)

    def trial(st, alpha):
        al = alpha[:, None, None]
        out = [z(t) + al * st["DZLam"][:, :nv]]
        if npth:
            out += [t["S"] + al * st["DS"], t["E1"] + al * st["DE1"], t["E2"] + al * st["DE2"]]
        return out

    def merit():
        zz = z(t)
        phi = t["COST"] - (mu * torch.where(free & hL, torch.log(zz - zl), 0.0)).sum((1, 2)) - (mu * torch.where(free & hU, torch.log(zu - zz), 0.0)).sum((1, 2))
        inf = t["RES"][:, :ns].abs().sum((1, 2))
        if npth:
            s, e1, e2 = t["S"], t["E1"], t["E2"]
            c_ = cs * t["RES"][:, ns:]
            target = c_ - e1 + e2
            keep = nu * (target - s).abs() - mu * torch.where(hasL, torch.log(s - lo), 0.0) - mu * torch.where(hasU, torch.log(hi - s), 0.0)
            take = -mu * torch.where(hasL, torch.log(target - lo), 0.0) - mu * torch.where(hasU, torch.log(hi - target), 0.0)
            s = torch.where((target > torch.where(hasL, lo, -INF)) & (target < torch.where(hasU, hi, INF)) & (take < keep), target, s)
            phi = phi - (mu * (torch.where(hasL, torch.log(s - lo), 0.0) + torch.where(hasU, torch.log(hi - s), 0.0) + torch.log(e1) + torch.log(e2))
                         - rho * (e1 + e2)).sum((1, 2))
            inf = inf + (c_ - s - e1 + e2).abs().sum((1, 2))
        return torch.stack([phi, inf], 1)

    def accept(st, a_pr, a_du):
        ap, ad = a_pr[:, None, None], a_du[:, None, None]
        zz = z(t)
        clamp = lambda m, g: torch.maximum(torch.minimum(m, 1e10 * mu / g), mu / (1e10 * g))
        out = [t["LamF"] + ap * st["DZLam"][:, nv:]]
        zL, zU = t["ZL"] + ad * st["DZL"], t["ZU"] + ad * st["DZU"]
        out += [torch.where(free & hL, clamp(zL, zz - zl), zL), torch.where(free & hU, clamp(zU, zu - zz), zU)]
        if npth:
            s = t["S"]
            vL, vU = t["VL"] + ad * st["DVL"], t["VU"] + ad * st["DVU"]
            out += [t["Y"] + ap * st["DY"], torch.where(hasL, clamp(vL, s - lo), vL), torch.where(hasU, clamp(vU, hi - s), vU),
                    clamp(t["W1"] + ad * st["DW1"], t["E1"]), clamp(t["W2"] + ad * st["DW2"], t["E2"])]
        return out

    def error():
        zz = z(t)
        zL, zU = t["ZL"], t["ZU"]
        sumz, cnt = (zL + zU).sum((1, 2)), ((zL > 0).sum((1, 2)) + (zU > 0).sum((1, 2))).double()
        summ = t["LamF"].abs().sum((1, 2))
        ed = torch.where(free, (t["G"] - zL + zU).abs(), 0.0).amax((1, 2))
        ep = t["RES"][:, :ns].abs().amax((1, 2))
        ec = torch.maximum(torch.where(free & hL, ((zz - zl) * zL - mu).abs(), 0.0).amax((1, 2)), torch.where(free & hU, ((zu - zz) * zU - mu).abs(), 0.0).amax((1, 2)))
        if npth:
            s, e1, e2, y, vL, vU, w1, w2 = (t[k] for k in ("S", "E1", "E2", "Y", "VL", "VU", "W1", "W2"))
            sumz = sumz + (vL + vU + w1 + w2).sum((1, 2))
            cnt = cnt + ((vL > 0).sum((1, 2)) + (vU > 0).sum((1, 2))).double() + 2 * npth * c["M"]
            summ = summ + y.abs().sum((1, 2))
            ed = torch.stack([ed, (-y - vL + vU).abs().amax((1, 2)), (rho - y - w1).abs().amax((1, 2)), (rho + y - w2).abs().amax((1, 2))]).amax(0)
            ep = torch.maximum(ep, (cs * t["RES"][:, ns:] - s - e1 + e2).abs().amax((1, 2)))
            ec = torch.stack([ec, torch.where(hasL, ((s - lo) * vL - mu).abs(), 0.0).amax((1, 2)), torch.where(hasU, ((hi - s) * vU - mu).abs(), 0.0).amax((1, 2)),
                              (e1 * w1 - mu).abs().amax((1, 2)), (e2 * w2 - mu).abs().amax((1, 2))]).amax(0)
        sd = torch.clamp((summ + sumz) / torch.clamp(cnt + (ns + npth) * c["M"], min=1.0), min=100.0) / 100.0
        sc = torch.clamp(sumz / torch.clamp(cnt, min=1.0), min=100.0) / 100.0
        return torch.stack([torch.stack([ed / sd, ep, ec / sc]).amax(0), ep], 1)

    return dict(reduce=reduce, expand=expand, trial=trial, merit=merit, accept=accept, error=error)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipm_times.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ipm_times.py needs the GPU: a time from anywhere else says nothing")
    import ipm_host
    import ipm_ref as R
    import etol_amd as E
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    h = ipm_host.load_harness()
    host = ipm_host.HostBackend(h)
    HOST_REPS = 20          # repetitions of the ipm_* calls inside the shim per timing: the time is taken in C++ around them alone
    timed = ipm_host.HostBackend(h, reps=HOST_REPS)
    recs = []
    for name in a.shapes.split(","):
        nv, ns, npth, M, batches = SHAPES[name]
        R.MODEL_OF.setdefault((nv, ns), {8: 1, 16: 2}[nv])
        one = R.make_case(nv, ns, npth, M, 1, 1, 99 + M)
        # what the later stages take, from the host functions once
        red = host.reduce(one)
        st1, scal1 = host.expand(one, red, one["DZLam"].copy())
        for B in batches:
            ev = E.Evaluator(0)
            ev.set_mesh(M, 0.0, 4.0)
            ev.set_model(one["model"], {1: W.QUAD_PARAMS, 2: W.FW_PARAMS}[one["model"]])
            ev.set_batch(B)
            if npth:
                recs_p = np.zeros((npth, L.PATH_REC)); recs_p[:, 0] = L.PATH_DISC; recs_p[:, 1:4] = [4.0, 3.2, 0.64]
                ev.set_path(recs_p, 0, 1)
            rep = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ev.device).repeat(B, *([1] * (x.ndim - 1))).contiguous()
            t = {k: rep(one[k]) for k in R.POINT + R.DUALS + ("RES", "VALS", "G", "COST", "par", "DZLam") if one[k].size}
            t["zl"], t["zu"] = (torch.from_numpy(one[k]).to(ev.device) for k in ("zl", "zu"))
            el = {k: rep(red[k]) for k in R.ELIM if red[k].size}
            st = {k: rep(st1[k]) for k in R.STEP if st1[k].size}
            alpha = rep(0.5 * scal1[:, 0])
            adu = rep(scal1[:, 1])
            if npth:
                hasL, hasU, lo, hi, cs = R.row_bounds(one)
                for k, v in (("hasL", hasL), ("hasU", hasU), ("lo", lo), ("hi", hi), ("cs", cs)):
                    t[k] = torch.from_numpy(np.ascontiguousarray(v)).to(ev.device)[None, :, None]
            pt = {k: t[k] for k in R.POINT if k in t}
            du = {k: t[k] for k in R.DUALS if k in t}
            bd = dict(zl=t["zl"], zu=t["zu"], cl=one["cl"], cu=one["cu"], cscale=None)
            kw = dict(dtype=torch.float64, device=ev.device)
            rhs, scal, mer, err = torch.zeros((B, nv + ns, M), **kw), torch.zeros((B, 4), **kw), torch.zeros((B, 2), **kw), torch.zeros((B, 3), **kw)
            trial = {k: torch.zeros_like(v) for k, v in pt.items()}
            pt2, du2 = {k: v.clone() for k, v in pt.items()}, {k: v.clone() for k, v in du.items()}
            torch.cuda.synchronize()
            tf = torch_forms(one, t)
            calls = dict(
                reduce=(lambda: ev.ipm_reduce(pt, du, t["RES"], t["VALS"], t["G"], bd, t["par"], el, rhs), tf["reduce"], 0),
                expand=(lambda: ev.ipm_expand(pt, du, t["VALS"], bd, t["par"], el, st, scal), lambda: tf["expand"](el, st["DZLam"]), 1),
                trial=(lambda: ev.ipm_trial(pt, st, alpha, trial), lambda: tf["trial"](st, alpha), None),
                merit=(lambda: ev.ipm_merit(pt, t["RES"], t["COST"], bd, t["par"], mer, reset=True), tf["merit"], 2),
                accept=(lambda: ev.ipm_accept(pt2, pt, du2, st, bd, t["par"], alpha, adu), lambda: tf["accept"](st, alpha, adu), 3),
                error=(lambda: ev.ipm_error(pt, du, t["RES"], t["G"], bd, t["par"], err), tf["error"], 4))
            nb = call_bytes(nv, ns, npth, one["nvals"], M, B)
            for cname, (dev_call, torch_call, host_what) in calls.items():
                for _ in range(5):
                    dev_call(); torch_call()
                ev.synchronize(); torch.cuda.synchronize()
                t_dev, t_torch, t_host = [], [], []
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(a.rounds):
                    for _ in range(a.launches):
                        ev.timer_start(); dev_call(); t_dev.append(ev.timer_stop())
                    for _ in range(a.launches):
                        e0.record(); torch_call(); e1.record(); e1.synchronize(); t_torch.append(e0.elapsed_time(e1))
                    if host_what is not None:       # one instance, HOST_REPS repetitions timed inside the shim, scaled to the batch
                        timed.seconds = 0.0
                        {0: lambda: timed.reduce(one), 1: lambda: timed.expand(one, red, one["DZLam"].copy()),
                         2: lambda: timed.merit(one, dict(one), True), 3: lambda: timed.accept(one, one, st1, scal1[:, 0], scal1[:, 1]),
                         4: lambda: timed.error(one)}[host_what]()
                        t_host.append(timed.seconds / HOST_REPS * 1e3 * B)
                dev_ms = statistics.median(t_dev)
                recs.append(dict(call=cname, shape=name, nv=nv, np=npth, M=M, B=B, launches=a.launches, rounds=a.rounds, dev_ms=dev_ms,
                                 torch_ms=statistics.median(t_torch), host_ms=statistics.median(t_host) if t_host else None,
                                 host_note="the ipm_* functions alone, timed inside the shim over 20 repetitions on one instance, one core, times the batch",
                                 bytes=nb[cname], hbm_fraction=nb[cname] / (dev_ms * 1e-3) / HBM,
                                 timing="HIP events around one call, median", device=torch.cuda.get_device_name(0)))
                print(json.dumps(recs[-1]))
            ev.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
