#!/usr/bin/env python3
"""Does a change to the host side of the C ABI (csrc/emi_api*.hip) leave the library as it was?  Run in two trees -- the parent
commit's and the changed one, each with its own built library -- and compare what they write:

   python tools/api_identity.py plan    OUT.json   emi_plan_pass (all fields) and emi_last_path over a grid; launches no kernel
   python tools/api_identity.py results OUT.json   SHA-256 of what every launch form computes, the kernel name, launch counts
   python tools/api_identity.py times   OUT.json   ms per default-dispatch pass at B = 1, 16, 128, 1024 (quadrotor, 1024 nodes)
   python tools/api_identity.py lockstep OUT.json  SHA-256 of X, U, LamF, LamC and the result records of the lock-step solve (2 x 9
                                                   instances of tests/lockstep_ref.py on 41 nodes), of the ladder (21, 41) over
                                                   them, of the refinement of tests/refine_ref.py (bounds shared and per instance;
                                                   with err and out) and of the moving-disc ladder and refinement of
                                                   tests/track_ladder_ref.py, default options, each with the context the call left:
                                                   what a change behind an option that is off, or to the drivers, must keep
   ... plan / results / times OUT.json name=value ...   with these options set on every context first: a default that moved behind an
                                                   option is compared with the parent through the option value that restores the
                                                   parent's choice ("sym_res=2": two resident workgroups per CU in every band)
   python tools/api_identity.py compare PARENT.json BRANCH.json [OUT.json]     equal or not, case by case ("report_only": the cases
                                                   that differ in REPORT_ONLY fields alone, see there)

The library is the one of the tree the script lies in."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# every threshold of plan_pass / plan_piece (csrc/emi_pass_plan.hpp): 16-instance x 128-node tiles (last below, first above), then instances.
# tests/harness/pass_plan_main.cpp walks the same grid without a device (tests/test_pass_plan_cpu.py holds its case names to plan_cases()).
TILE_STEPS = [(32, 33), (48, 49), (127, 128), (143, 144), (207, 208), (383, 384), (767, 768), (1024, 1025)]
INSTANCES = [1, 16, 64, 2048, 2049, 4096, 16384]
FORCED = {"sym_ct": range(0, 9), "sym_ksplit": (0, 1, 2, 4, 8), "sym_bk": (0, 8, 16), "sym_ctc": (0, 1, 2), "sym_hs": (0, 1, 2),
          "sym_nst": (3, 4), "sym_cpart": (-1, 0, 1, 2, 4, 8), "sym_gblk": (0, 1, 2, 4, 8, 64), "pass_order": (-1, 0, 1, 100, 125, 150),
          "node_store": (-1, 0, 1, 2, 3), "overlap_mode": (0, 1, 2, 3), "slice": (0, 16, 256, 1024), "sym_dop": (0, 1, 2), "sym_cx": (0, 1, 2)}
DEFAULTS = {"sym_nst": 3, "sym_cpart": 0, "pass_order": -1, "node_store": -1}
BASE = {}       # options set on every context before anything else (name=value arguments)


def batches(M):
    per = M // 128
    out = set(INSTANCES)
    for lo, _ in TILE_STEPS:
        out.update((16 * (lo // per), 16 * (lo // per) + 1))      # the last batch within `lo` tiles and the first beyond
    return sorted((b for b in out if b >= 1), reverse=True)        # (descending: the context's buffers are sized once)


# the models of the plan grid by their number of states: which forms exist goes by it (the 2-state model's SW = 2 is all its states)
PLAN_MODELS = {2: "pointmass2", 6: "quadrotor6", 12: "fixedwing12"}
PLAN_MESHES = (128, 256, 1024)


def plan_cases(ns_axis=tuple(PLAN_MODELS)):
    """the grid as (case name, ns, M, option, value, B), in the order plan_grid walks it"""
    for ns in ns_axis:
        for M in PLAN_MESHES:
            for opt, value in [(None, None)] + [(o, v) for o, vs in FORCED.items() for v in vs]:
                for B in batches(M):
                    yield f"{PLAN_MODELS[ns]} M={M} {opt}={value} B={B}", ns, M, opt, value, B


def plan_grid():
    import etol_amd as E
    from etol_amd import workloads as W
    models = {"pointmass2": (E.MODEL_POINTMASS2D, ()), "quadrotor6": (E.MODEL_QUADROTOR2D, W.QUAD_PARAMS),
              "fixedwing12": (E.MODEL_FIXEDWING12, W.FW_PARAMS)}
    out = {}
    for mname, (model, params) in ((PLAN_MODELS[ns], models[PLAN_MODELS[ns]]) for ns in PLAN_MODELS):
        for M in PLAN_MESHES:
            ev = E.Evaluator(0)
            ev.set_mesh(M, 0.0, 2.0)
            ev.set_model(model, params)
            for k, v in BASE.items():
                ev.set_option(k, v)
            for opt, value in [(None, None)] + [(o, v) for o, vs in FORCED.items() for v in vs]:
                if opt:
                    ev.set_option(opt, value)
                for B in batches(M):
                    ev.set_batch(B)
                    out[f"{mname} M={M} {opt}={value} B={B}"] = dict(ev.plan(B), last_path=int(ev.uses_fused_kernel))
                if opt:
                    ev.set_option(opt, DEFAULTS.get(opt, 0))
            ev.close()
    return out


def sha(a):
    import numpy as np
    import torch
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def traced_quadrotor():
    import ctypes as C
    lib = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    lib.harness_traced_model_source.restype = C.c_char_p
    return lib.harness_traced_model_source(0).decode()


Q = dict(model="quad", M=1024)
CASES = {
    # fp64, the one-launch pass
    "pass K slices": dict(Q, B=16), "pass unsplit": dict(Q, B=256), "pass 16-deep K tiles": dict(Q, B=128),
    "pass 128-column tiles": dict(Q, B=64, opts=dict(sym_ct=6, sym_ksplit=1, sym_ctc=2)),
    "pass halved K": dict(Q, B=64, opts=dict(sym_ksplit=1, sym_hs=2)),
    "pass pointmass": dict(model="pm", M=256, B=16), "pass one instance": dict(Q, B=1),
    # (all the states of the 2-state model in one workgroup, in the range where two states of a larger model take 16-deep K tiles)
    "pass pointmass 1024": dict(model="pm", M=1024, B=1024),
    # fp64, two kernels
    **{f"two kernels mode {m} combine {sc} cost_in_kernel {ck}": dict(Q, B=32, opts=dict(overlap_mode=m, sym_ct=7, sym_ksplit=2, sym_combine=sc,
                                                                                         cost_in_kernel=ck))
       for m in (1, 2) for sc in (0, 1) for ck in (0, 1)},
    "two kernels ring": dict(Q, B=256, opts=dict(overlap_mode=2, sym_ct=3)),
    "skinny": dict(Q, B=2, opts=dict(overlap_mode=2)),
    "sliced large batch": dict(model="quad", M=128, B=2320, paths=True), "slice option": dict(Q, B=64, opts=dict(slice=16), paths=True),
    "delays": dict(model="quad", M=128, B=8, delays=(0, 1, 0.1)),
    "run-time compiled": dict(model="rtc", M=1024, B=16), "run-time compiled two kernels": dict(model="rtc", M=1024, B=16, opts=dict(overlap_mode=2)),
    "sequential": dict(Q, B=16, opts=dict(overlap=0)), "sequential 33 nodes": dict(model="quad", M=33, B=3),
    "defect only": dict(Q, B=16, flags=2), "nodes only": dict(Q, B=16, flags=1), "no Jacobian": dict(Q, B=16, flags=7),
    # fp32
    "f32 ring": dict(model="fw", M=1024, B=16, f32=True), "f32 register-staged": dict(model="fw", M=1024, B=16, f32=True, opts=dict(f32_ring=0)),
    "f32 one launch": dict(model="fw", M=512, B=64, f32=True, opts=dict(overlap_mode=3, f32_ring=0), atomics=True),
    "f32 two streams": dict(model="fw", M=512, B=64, f32=True, opts=dict(overlap_mode=2), atomics=True),
}


def run_case(c):
    import numpy as np
    import torch
    import etol_amd as E
    import oracle_lib as O
    from etol_amd import workloads as W
    f32, M, B, flags = c.get("f32", False), c["M"], c["B"], c.get("flags", 3)
    ev = E.Evaluator(0, f32=f32)
    ev.set_mesh(M, 0.0, 20.0 if c["model"] == "fw" else 2.0)
    if c["model"] == "rtc":
        ev.set_model_source("TracedModel", traced_quadrotor(), 6, 2)
    else:
        ev.set_model(*{"quad": (E.MODEL_QUADROTOR2D, W.QUAD_PARAMS), "pm": (E.MODEL_POINTMASS2D, ()), "fw": (E.MODEL_FIXEDWING12, W.FW_PARAMS)}[c["model"]])
    if c.get("delays"):
        ev.set_delays(*c["delays"])
    ev.set_batch(B)
    gen = min(B, 16)
    recs = None
    if c["model"] == "fw":
        X, U = W.fixedwing_batch(4, gen, M)
    elif c["model"] == "pm":
        X, U = W.pointmass_batch(1, gen, M)
    else:
        X, U, recs = W.quadrotor_batch(2, gen, M, 3 if c.get("paths") else 0)
    rep = lambda a: np.concatenate([a] * (B // gen) + [a[:B % gen]])
    X, U = rep(X), rep(U)[:, :ev.layout.nc - ev.n_delayed]
    if f32:
        X, U = (a.astype(np.float32).astype(np.float64) for a in (X, U))
    if c.get("paths"):
        recs = rep(recs)
        recs[:, :, 1] += 0.001 * np.arange(B)[:, None]           # a table per instance: a piece must read its own
        ev.set_path(recs, 0, 1)
    for k, v in {**BASE, **c.get("opts", {})}.items():
        ev.set_option(k, v)
    lay = ev.layout
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32 if f32 else np.float64)).cuda()
    dX, dU = dev(X), dev(U)
    out = dict(last_path=int(ev.uses_fused_kernel))

    def evaluate(tag):
        outs = ev.alloc_outputs()
        for t in outs:
            t.zero_()
        torch.cuda.synchronize()
        ev.eval_dev(dX, dU, outs[0], outs[1] if flags & 1 else None, outs[2] if flags & 1 else None, flags)
        ev.synchronize()
        out[tag] = dict(RES=sha(outs[0]), VALS=sha(outs[1]), COST=sha(outs[2]), kernel=ev.last_defect_kernel)
        return outs

    outs = evaluate("eval_dev")
    if c.get("atomics"):                    # float atomics from two roles: does one library agree with itself?  And with the oracle?
        out["repeats"] = []
        for _ in range(3):
            evaluate("eval_dev_again")
            out["repeats"].append(out["eval_dev_again"]["RES"])
        sub = slice(0, 4)
        rRES, rVALS, rCOST = O.evaluate(E.MODEL_FIXEDWING12, W.FW_PARAMS, M, (ev.tau, ev.w, ev.D), 0.0, 20.0, X[sub], U[sub])
        got = [o.cpu().numpy().astype(np.float64) for o in outs]
        scale = np.einsum("kj,bij->bik", np.abs(ev.D), np.abs(X[sub])) + np.abs(rRES) + 1.0
        errs = dict(RES=float((np.abs(got[0][sub] - rRES) / scale).max()),
                    VALS=float(max(np.abs(got[1][sub][:, e] - rVALS[:, e]).max() / (np.abs(rVALS[:, e]).max() + 1.0) for e in range(rVALS.shape[1]))),
                    COST=float(np.abs(got[2][sub] - rCOST).max() / np.abs(rCOST).max()))
        # the bounds of tests/test_gpu_parity.py::test_f32_pass_as_one_launch_matches_the_sequential_pair_and_the_oracle at M <= 512
        out["oracle"] = dict(errs, bound=2e-6, within=all(v < 2e-6 for v in errs.values()))
    ev.profile(1)
    evaluate("eval_dev_profiled")
    counts = ev.profile_read()
    out["launch_counts"] = {k: v for k, v in counts.items() if not k.endswith("_ms")}
    ev.profile(0)
    if flags != 3:
        ev.close()
        return out
    rng = np.random.default_rng(7)
    lamF, lamC = rng.standard_normal((B, lay.ns, M)), rng.standard_normal((B, lay.np, M))
    H = torch.zeros((B, lay.nhess, M), dtype=ev.dtype, device="cuda")
    ev.hess_dev(dX, dU, dev(lamF), dev(lamC) if lay.np else None, 0.7, H)
    ev.synchronize()
    out["hess_dev"] = sha(H)
    small = slice(0, min(B, 32))           # the host forms on a batch of their own (they stage through the context's buffers)
    if B > 32:
        ev.set_batch(32)
        if c.get("paths"):
            ev.set_path(recs[small], 0, 1)
    hX, hU, hF, hC = X[small], U[small], lamF[small], lamC[small] if lay.np else None
    hRES, hVALS, hCOST = ev.eval_host(hX, hU)
    out["eval_host"] = dict(RES=sha(hRES), VALS=sha(hVALS), COST=sha(hCOST), kernel=ev.last_defect_kernel)
    out["hess_host"] = sha(ev.hess_host(hX, hU, hF, hC, 0.7))
    if not f32:
        nf = lay.ns + lay.nc - ev.n_delayed
        z = np.concatenate([hX, hU], axis=1)
        zl, zu = z - 0.5 * rng.random(z.shape), z + 0.5 * rng.random(z.shape)
        cl, cu = -np.ones(lay.np), np.ones(lay.np)
        total = ev.n_delayed > 0
        if B > 32:
            ev.set_batch(B)
            if c.get("paths"):
                ev.set_path(recs, 0, 1)
        G = torch.zeros((B, nf, M), dtype=torch.float64, device="cuda")
        cert = torch.zeros((B, 6), dtype=torch.float64, device="cuda")
        dzl, dzu = dev(np.concatenate([X, U], axis=1) - 0.25), dev(np.concatenate([X, U], axis=1) + 0.25)
        args = (outs[1], dev(lamF), dev(lamC) if lay.np else None, 0.7)
        if total:
            Gdel = torch.zeros((B, ev.n_delayed, M), dtype=torch.float64, device="cuda")
            ev.lagr_grad_total_dev(*args, G, Gdel)
            ev.synchronize()
            out["lagr_grad_total_dev"] = dict(G=sha(G), Gdel=sha(Gdel))
            ev.kkt_certificate_total_dev(dX, dU, outs[0], *args, dzl, dzu, cl, cu, cert, G, Gdel)
            ev.synchronize()
            out["kkt_certificate_total_dev"] = dict(cert=sha(cert), G=sha(G), Gdel=sha(Gdel))
        else:
            ev.lagr_grad_dev(*args, G)
            ev.synchronize()
            out["lagr_grad_dev"] = sha(G)
            ev.kkt_certificate_dev(dX, dU, outs[0], *args, dzl, dzu, cl, cu, cert, G)
            ev.synchronize()
            out["kkt_certificate_dev"] = dict(cert=sha(cert), G=sha(G))
        if B > 32:
            ev.set_batch(32)
            if c.get("paths"):
                ev.set_path(recs[small], 0, 1)
        if total:
            out["lagr_grad_total_host"] = [sha(a) for a in ev.lagr_grad_total_host(hVALS, hF, hC, 0.7)]
            out["kkt_certificate_total_host"] = [sha(a) for a in ev.kkt_certificate_total_host(hX, hU, hF, hC, zl, zu, cl, cu, 0.7)]
        else:
            out["lagr_grad_host"] = sha(ev.lagr_grad_host(hVALS, hF, hC, 0.7))
            out["kkt_certificate_host"] = [sha(a) for a in ev.kkt_certificate_host(hX, hU, hF, hC, zl, zu, cl, cu, 0.7)]
    ev.close()
    return out


def times():
    import torch
    import etol_amd as E
    from etol_amd import workloads as W
    out = {}
    for B in (1, 16, 128, 1024):
        ev = E.Evaluator(0)
        ev.set_mesh(1024, 0.0, 2.0)
        ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS)
        ev.set_batch(B)
        for k, v in BASE.items():
            ev.set_option(k, v)
        X, U, _ = W.quadrotor_batch(2, min(B, 16), 1024, 0)
        dX, dU = (torch.from_numpy(a).cuda().repeat((B + 15) // 16, 1, 1)[:B].contiguous() for a in (X, U))
        outs = ev.alloc_outputs()
        import ctypes as C
        p = [C.c_void_p(t.data_ptr()) for t in (dX, dU, *outs)]
        call = lambda: ev.lib.emi_eval_dev(ev.ctx, *p, 3)
        for _ in range(2000):
            call()
        ev.synchronize()
        n, ms = 2000, 0.0
        while ms < 1100.0:                  # enough passes to fill a second
            n = int(n * max(1.5, 1300.0 / ms)) if ms else n
            ev.timer_start()
            for _ in range(n):
                call()
            ms = ev.timer_stop()
        out[str(B)] = dict(passes=n, ms_per_pass=ms / n, kernel=ev.last_defect_kernel)
        ev.close()
    return out


def lockstep():
    import numpy as np
    import torch
    import etol_amd as E
    import ladder_ref as LD
    import lockstep_ref as LR
    import refine_ref as RR
    import track_ladder_ref as TR
    fields = ("status", "iterations", "evaluations", "factorisations", "reflected_steps", "cost", "kkt_error", "constr_viol", "emax", "mu", "rho")
    rows = lambda res: [[q[k] for k in fields] for q in res]
    out = {}

    def context(ev, tracks):
        """the context a call left: mesh and batch, and what its table (and centres) make of one fixed trajectory"""
        lay = ev.layout
        rng = np.random.default_rng(7)
        kw = dict(dtype=torch.float64, device=ev.device)
        X, U = (torch.from_numpy(rng.standard_normal((lay.B, r, lay.M))).to(ev.device) for r in (lay.ns, lay.nc))
        RES, VALS, COST = torch.zeros((lay.B, lay.ns + lay.np, lay.M), **kw), torch.zeros((lay.B, lay.nvals, lay.M), **kw), torch.zeros(lay.B, **kw)
        torch.cuda.synchronize()
        ev.eval_dev(X, U, RES, VALS, COST)
        ev.synchronize()
        d = dict(M=lay.M, B=lay.B, np=lay.np, t0=lay.t0, tf=lay.tf, RES=sha(RES), VALS=sha(VALS), COST=sha(COST))
        if tracks:
            d["tracks"] = [sha(a) for a in ev.get_tracks()]
        return d

    def run(name, tf, insts, ladder, refine=None, replicate=False, tracks=False):
        """refine: None (the one-mesh solve or the ladder), or (ode_tol, first_check)"""
        B = len(insts)
        ev = E.Evaluator(0)
        ev.set_mesh(ladder[0], 0.0, tf)
        ev.set_model(1, LR.QUAD_PARAMS)
        ev.set_batch(B)
        ev.set_path(np.stack([i["recs"] if tracks else LR.records(i["discs"]) for i in insts]), 0, 1)
        if tracks:
            ev.set_track_waypoints(*TR.stacked([i["way"] for i in insts]))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
        z0 = np.stack([i["z0"] for i in insts]).reshape(B, 8, ladder[0])
        X, U = up(z0[:, :6]), up(z0[:, 6:])
        bounds = []
        for M in ladder:
            P = LD.quad_at(tf, M, LR.discs_of(LR.FIRST_DISCS[0]))
            rep = B if replicate else 1
            bounds.append(dict(zl=up(np.repeat(P.lo.reshape(1, 8, M), rep, 0)), zu=up(np.repeat(P.up.reshape(1, 8, M), rep, 0)), cl=LR.CL, cu=LR.CU,
                               cscale=LR.CSCALE))
        rungs = [dict(M=M, bounds=b, options=dict(tol=1e-8), repair=0) for M, b in zip(ladder, bounds)]
        torch.cuda.synchronize()
        extra = {}
        if refine:
            X, U, LamF, LamC, res, err, summ = ev.ipm_solve_refine(rungs, 0.0, tf, X, U, refine[0], refine[1], RR.UL, RR.UU)
            extra = dict(err=sha(err), out=[[q["rung"], q["verdict"], q["rungs_solved"], repr(q["err"])] for q in summ])
        elif len(ladder) == 1:
            LamF, LamC, res = ev.ipm_solve_shard(X, U, bounds[0], dict(tol=1e-8, max_iter=200))
            res = [res]
        else:
            X, U, LamF, LamC, res = ev.ipm_solve_ladder(rungs, 0.0, tf, X, U)
        ev.synchronize()
        out[name] = dict(X=sha(X), U=sha(U), LamF=sha(LamF), LamC=sha(LamC), results=[rows(r) for r in res], **extra)
        if len(ladder) > 1:
            out[name]["context"] = context(ev, tracks)
        ev.close()

    for tf in LR.TFS:
        run(f"one mesh tf={tf}", tf, LR.instances(tf), (LR.M_NODES,))
        run(f"ladder tf={tf}", tf, LD.instances(tf), tuple(LD.LADDER))
        # the refinement of tests/refine_ref.py, bounds shared and per instance
        run(f"refine tf={tf}", tf, LD.instances(tf), RR.LADDER, refine=(RR.TOLS[tf], RR.FIRST_CHECK))
        run(f"refine, bounds per instance tf={tf}", tf, LD.instances(tf), RR.LADDER, refine=(RR.TOLS[tf], RR.FIRST_CHECK), replicate=True)
    # moving discs (tests/track_ladder_ref.py): the two-rung ladder, the refinement over it checked from the first rung on, and the
    # refinement of the tracks at rest over the four rungs, which compacts the centres through the set map
    tf = TR.TF
    run("track ladder", tf, TR.moving_instances(), tuple(LD.LADDER), tracks=True)
    run("track refine", tf, TR.moving_instances(), tuple(LD.LADDER), refine=(RR.TOLS[tf], 0), tracks=True)
    run("track refine, four rungs", tf, TR.static_instances(tf), RR.LADDER, refine=(RR.TOLS[tf], RR.FIRST_CHECK), tracks=True)
    return out


# what may differ between two trees where one of them REPORTED a feature of the MFMA role that it has no kernel for and launched the
# plain form (SW = all the states, or 3): the depth of a K tile, the K halves, the ring stages, the column sub-tiles (and with them
# the workgroup count) and the kernel's name -- never what is launched or computed
REPORT_ONLY = ("k_tile", "k_halves", "ring_stages", "column_tiles", "mfma_workgroups", "kernel")


def report_only(name, a, b):
    """a and b differ in REPORT_ONLY fields alone; for a plan, in a case whose SW is all the states of its model, or 3"""
    def strip(d):
        return {k: strip(v) for k, v in d.items() if k not in REPORT_ONLY} if isinstance(d, dict) else d
    if not (isinstance(a, dict) and isinstance(b, dict)) or strip(a) != strip(b):
        return False
    if "sw" in a:
        ns = {v: k for k, v in PLAN_MODELS.items()}[name.split()[0]]
        return a["sw"] == b["sw"] and a["sw"] in (ns, 3)
    return True


def compare(pa, br):
    report = dict(equal=[], different=[], self_disagreeing=[], report_only=[])
    for name in sorted(set(pa) | set(br)):
        a, b = pa.get(name), br.get(name)
        unstable = isinstance(a, dict) and "repeats" in a and len(set(a["repeats"]) | {a["eval_dev"]["RES"]}) > 1
        if unstable:        # the parent does not reproduce its own bits here: the oracle decides, at the existing test's bounds
            strip = lambda d: {k: v for k, v in d.items() if k in ("last_path", "launch_counts", "oracle")}
            ok = a["oracle"]["within"] and b["oracle"]["within"] and strip(a)["launch_counts"] == strip(b)["launch_counts"]
            report["self_disagreeing"].append(dict(case=name, parent=a, branch=b, both_within_oracle_bound=ok))
            if not ok:
                report["different"].append(name)
        elif a == b:
            report["equal"].append(name)
        elif report_only(name, a, b):
            report["report_only"].append(name)
        else:
            report["different"].append(name)
    report["verdict"] = "identical" if not report["different"] else "DIFFERENT"
    return report


def changes(pa, br):
    """the cases that are not equal, by what changed in them ({field: [parent, branch]}, nested fields by their path); the case names of
    a plan grid ("model M=.. option=value B=..") gathered by model, mesh and batch sizes"""
    def leaves(d, at=""):
        return {k: v for key, val in d.items() for k, v in leaves(val, f"{at}{key}.").items()} if isinstance(d, dict) else {at[:-1]: d}
    kinds = {}
    for name in sorted(set(pa) | set(br)):
        a, b = leaves(pa.get(name, {})), leaves(br.get(name, {}))
        if a != b:
            changed = json.dumps({k: [a.get(k), b.get(k)] for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)})
            kind = kinds.setdefault(changed, dict(changed=json.loads(changed), n=0, cases={}))
            kind["n"] += 1
            if name.count(" ") == 3 and " B=" in name:
                model, M, opt, B = name.split()
                kind["cases"].setdefault(f"{model} {M}", {}).setdefault(opt, []).append(int(B[2:]))
            else:
                kind["cases"][name] = 1
    for kind in kinds.values():         # options with the same batches together: {model M=..: [{B: [...], options: [...]}]}
        for group, opts in kind["cases"].items():
            if isinstance(opts, dict):
                same = {}
                for opt, bs in opts.items():
                    same.setdefault(tuple(bs), []).append(opt)
                kind["cases"][group] = [dict(B=sorted(bs), options=o) for bs, o in same.items()]
    return list(kinds.values())


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "compare":
        pa, br = (json.load(open(f)) for f in sys.argv[2:4])
        rep = compare(pa, br)
        print(json.dumps({k: (v if k == "verdict" or k == "self_disagreeing" else len(v)) for k, v in rep.items()} | {"different": rep["different"][:20]}))
        if len(sys.argv) > 4:
            sha = lambda d: hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()
            text = json.dumps(dict(rep, equal=len(rep["equal"]), report_only=len(rep["report_only"]), sha256=dict(parent=sha(pa), branch=sha(br)),
                           changes=changes(pa, br)), indent=1)
            for flat in (r"\[\s+([^][{}]*?)\s+\]", r"\{\s+([^{}]*?)\s+\}"):       # lists of numbers and names, then flat objects, on one line each
                text = re.sub(flat, lambda m: m.group(0)[0] + " ".join(m.group(1).split()) + m.group(0)[-1], text)
            open(sys.argv[4], "w").write(text + "\n")
        sys.exit(0 if rep["verdict"] == "identical" else 1)
    BASE.update({k: int(v) for k, v in (arg.split("=") for arg in sys.argv[3:])})
    res = plan_grid() if mode == "plan" else times() if mode == "times" else lockstep() if mode == "lockstep" else {name: run_case(c) for name, c in CASES.items()}
    json.dump(res, open(sys.argv[2], "w"), indent=1 if mode != "plan" else None, sort_keys=True)
    print(mode, len(res), "entries ->", sys.argv[2], hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest()[:16])
