"""Residual-based acceptance and the crawl rule in the lock-step solve (opt.rules = EMI_IPM_RULE_RESIDUAL), and emi_ipm_keep_dev /
_host.  -m gpu

Cases: tests/lockstep_ref.py (41-node quadrotor, B <= 9) and its blocked instance; fixtures tests/golden/lockstep_cases.json and
tests/golden/lockstep_rescue_cases.json (solve_nlp on the CPU oracle under the device's rule set, tests/lockstep_rescue_ref.py).
The solve criterion, the tolerances and the 1.5 x margin of device counts over solve_nlp's are those of tests/test_gpu_lockstep.py."""
import ctypes as C

import numpy as np
import pytest

import ladder_ref as LD
import lockstep_ref as LR
import lockstep_rescue_ref as RR
import test_gpu_lockstep as TL

pytestmark = pytest.mark.gpu

TOL, TOL_FINE = TL.TOL, TL.TOL_FINE
NS, NP, M = TL.NS, TL.NP, TL.M
RULE = dict(rules=RR.RULE_RESIDUAL, crawl_limit=RR.OPTIONS["crawl_limit"], crawl_frac=RR.OPTIONS["crawl_frac"])
POINT = ("X", "U", "S", "E1", "E2")
DUALS = ("LamF", "Y", "ZL", "ZU", "VL", "VU", "W1", "W2")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- emi_ipm_keep_dev / _host -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npth", (0, 3))
@pytest.mark.parametrize("Mn", (33, 300))
def test_keep_copies_the_masked_instances_and_nothing_else(built, Mn, npth):
    import torch
    from test_gpu_ipm import make_ev as ipm_ev
    nv, ns, nc, B = 8, 6, 2, 3
    ev = ipm_ev(dict(nv=nv, ns=ns, nc=nc, np=npth, M=Mn, B=B, nsets=1, model=1, nvals=ns * nv + 2 * npth + nv))
    rng = np.random.default_rng(100 * Mn + npth)
    rows = lambda n: ns if n in ("X", "LamF") else nc if n == "U" else nv if n in ("ZL", "ZU") else npth
    names = [n for n in POINT + DUALS if rows(n) > 0]
    src = {n: rng.standard_normal((B, rows(n), Mn)) for n in names}
    up = lambda a: torch.from_numpy(a.copy()).to(ev.device)
    group = lambda keys, d: {n: d[n] for n in keys if n in d}
    for restore in (False, True):
        for mask in ([1, 0, 1], [0, 0, 0], [1, 1, 1], None):
            sel = [True] * B if mask is None else [bool(m) for m in mask]
            hm = None if mask is None else np.array(mask, dtype=np.uint8)
            # the source side holds the data, the destination NaN
            a_dev = {n: up(src[n]) for n in names}
            b_dev = {n: up(np.full_like(src[n], np.nan)) for n in names}
            a_host = {n: src[n].copy() for n in names}
            b_host = {n: np.full_like(src[n], np.nan) for n in names}
            live_d, kept_d = (b_dev, a_dev) if restore else (a_dev, b_dev)
            live_h, kept_h = (b_host, a_host) if restore else (a_host, b_host)
            torch.cuda.synchronize()
            ev.ipm_keep(group(POINT, live_d), group(DUALS, live_d), group(POINT, kept_d), group(DUALS, kept_d),
                        mask=None if hm is None else up(hm), restore=restore)
            ev.synchronize()
            ev.ipm_keep(group(POINT, live_h), group(DUALS, live_h), group(POINT, kept_h), group(DUALS, kept_h), mask=hm, restore=restore, dev=False)
            for n in names:
                a, b = a_dev[n].cpu().numpy(), b_dev[n].cpu().numpy()
                assert np.array_equal(bits(a), bits(src[n])), (n, "the source side is only read")
                for i in range(B):
                    want = src[n][i] if sel[i] else np.full_like(src[n][i], np.nan)
                    assert np.array_equal(bits(b[i]), bits(want)), (Mn, npth, restore, mask, n, i)
                assert np.array_equal(bits(b), bits(b_host[n])) and np.array_equal(bits(a), bits(a_host[n])), (n, "host form")
    # statuses
    import etol_amd as E
    from etol_amd import _lib as L
    lib = E.load()
    assert lib.emi_ipm_keep_dev(None, None, None, None, None, None, 0) == 1 and lib.emi_ipm_keep_dev(ev.ctx, None, None, None, None, None, 0) == 1
    assert lib.emi_ipm_keep_host(None, None, None, None, None, None, 0) == 1
    ev.close()
    f = ipm_ev(dict(nv=nv, ns=ns, nc=nc, np=0, M=33, B=B, nsets=1, model=1, nvals=ns * nv + nv), f32=True)
    pt, du = L.IpmPoint(), L.IpmDuals()
    assert lib.emi_ipm_keep_dev(f.ctx, C.byref(pt), C.byref(du), C.byref(pt), C.byref(du), None, 0) == 5        # EMI_ERR_UNSUPPORTED
    f.close()


# ---- the rule in the solve ------------------------------------------------------------------------------------------------------------
def three(tf):
    """the blocked instance between two regular ones (tests/test_gpu_lockstep.py::test_an_instance_without_a_feasible_path_ends_alone)"""
    insts = LR.instances(tf)
    return [insts[1], RR.blocked_instance(tf), insts[5]], (1, None, 5)


def show(tag, res):
    for b, q in enumerate(res):
        print(f"{tag} instance {b}: status {q['status']} iterations {q['iterations']} evaluations {q['evaluations']} newton {q['newton_steps']} "
              f"restored {q['restored_steps']} kkt {q['kkt_error']:.2e} viol {q['constr_viol']:.2e} emax {q['emax']:.2e} rho {q['rho']:g} "
              f"cost {q['cost']:.6f}")


@pytest.fixture(scope="module")
def three_runs(built):
    out, evs = {}, []
    for tf in LR.TFS:
        insts, src = three(tf)
        ev = TL.make_ev(tf, insts)
        evs.append(ev)
        out[tf] = dict(insts=insts, src=src, ev=ev, first=TL.solve(ev, tf, insts, dict(tol=TOL, max_iter=200, **RULE)))
    yield out
    for ev in evs:
        ev.close()


@pytest.mark.parametrize("tf", LR.TFS)
def test_the_blocked_instance_gets_its_verdict_before_the_limit(three_runs, tf):
    """Without the rule the instance crawls to max_iter (200 iterations, about 1900 evaluations on the CPU)."""
    a = three_runs[tf]
    ev, insts, r = a["ev"], a["insts"], a["first"]
    fine = TL.solve(ev, tf, insts, dict(tol=TOL_FINE, max_iter=80))
    show(f"tf {tf}", r["res"])
    want = RR.fixture()["cases"][str(tf)]["blocked"]["rule_on"]
    rows = LR.fixture()["cases"][str(tf)]
    bad = r["res"][1]
    print(f"tf {tf} blocked: fixture iterations {want['iterations']} evaluations {want['evaluations']} newton {want['newton_steps']} "
          f"restored {want['restored_steps']}")
    assert bad["status"] in (LR.INFEASIBLE, LR.LINE_SEARCH), bad
    assert bad["rho"] >= 1e5 and (bad["constr_viol"] > 1e-3 or bad["emax"] > 1e-3), bad
    assert bad["iterations"] <= 1.5 * want["iterations"] and bad["evaluations"] <= 1.5 * want["evaluations"], (bad, want)
    assert bad["newton_steps"] >= 1 and bad["restored_steps"] >= 1, bad
    for b in (0, 2):
        assert r["res"][b]["status"] in (LR.CONVERGED, LR.ACCEPTABLE)
        TL.meets_the_solve_criterion(tf, insts[b], rows[a["src"][b]], r["X"][b], r["U"][b], r["res"][b]["cost"], fine["X"][b], fine["U"][b],
                                     f"tf {tf} beside the blocked instance: {b}")


def test_two_calls_the_iteration_limit_and_the_host_form(three_runs):
    tf = LR.TFS[0]
    a = three_runs[tf]
    ev, insts, first = a["ev"], a["insts"], a["first"]
    opt = dict(tol=TOL, max_iter=200, **RULE)
    second = TL.solve(ev, tf, insts, opt)
    assert TL.same_bits(first, second) and first["res"] == second["res"]
    its = [q["iterations"] for q in first["res"]]
    n = min(its)
    third = TL.solve(ev, tf, insts, dict(opt, max_iter=n))
    for b in range(len(insts)):
        if its[b] == n:
            assert TL.same_bits(first, third, (b, b)) and third["res"][b] == first["res"][b], b
        else:
            assert third["res"][b]["status"] == LR.MAX_ITER and third["res"][b]["iterations"] == n, third["res"][b]
    host = TL.solve(ev, tf, insts, opt, dev=False)
    assert TL.same_bits(first, host) and first["res"] == host["res"]


def test_batch_a_with_the_rule_on(built):
    import torch
    tf = LR.TFS[0]
    insts, rows = LR.instances(tf), LR.fixture()["cases"][str(tf)]
    ev = TL.make_ev(tf, insts)
    r = TL.solve(ev, tf, insts, dict(tol=TOL, max_iter=200, **RULE))
    fine = TL.solve(ev, tf, insts, dict(tol=TOL_FINE, max_iter=80, **RULE))
    res, B = r["res"], len(insts)
    show(f"tf {tf}", res)
    assert all(q["status"] in (LR.CONVERGED, LR.ACCEPTABLE) for q in res), [q["status"] for q in res]
    kw = dict(dtype=torch.float64, device=ev.device)
    RES, VALS, COST = torch.zeros((B, NS + NP, M), **kw), torch.zeros((B, ev.layout.nvals, M), **kw), torch.zeros(B, **kw)
    torch.cuda.synchronize()
    ev.eval_dev(r["tX"], r["tU"], RES, VALS, COST)
    ev.synchronize()
    cost = COST.cpu().numpy()
    for b in range(B):
        assert cost[b] == res[b]["cost"]                        # the same evaluation: the same bits
        TL.meets_the_solve_criterion(tf, insts[b], rows[b], r["X"][b], r["U"][b], res[b]["cost"], fine["X"][b], fine["U"][b], f"tf {tf} instance {b}")
    ev.close()
    mine, theirs = sum(q["iterations"] for q in res), sum(q["iterations"] for q in rows)
    print(f"tf {tf}: {mine} iterations over the batch with the rule, fixture {theirs}")
    assert mine <= 1.5 * theirs


def test_options(built):
    import torch
    import etol_amd as E
    from etol_amd import _lib as L
    tf = LR.TFS[0]
    insts, _ = three(tf)
    ev = TL.make_ev(tf, insts)
    # an unknown bit
    Xh, Uh, zlh, zuh = TL.host_arrays(tf, insts)
    X, U, zl, zu = (torch.from_numpy(a.copy()).to(ev.device) for a in (Xh, Uh, zlh, zuh))
    LF, LC = (torch.zeros((3, n, M), dtype=torch.float64, device=ev.device) for n in (NS, NP))
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    bd = L.IpmBounds()
    bd.zl, bd.zu, bd.nsets = p(zl), p(zu), 1
    bd.cl, bd.cu = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (LR.CL, LR.CU))
    opt, res = L.IpmOptions(), (L.IpmResult * 3)()
    opt.max_iter = 3
    for rules, want in ((2, 1), (3, 1), (1 << 30, 1), (-1, 1), (1, 0), (0, 0)):
        opt.rules = rules
        assert E.load().emi_ipm_solve_shard_dev(ev.ctx, p(X), p(U), C.byref(bd), C.byref(opt), p(LF), p(LC), res) == want, rules
    ev.synchronize()
    # a crawl limit out of reach leaves the err0 <= 1e-2 branch, which the blocked instance never reaches in 40 iterations
    off = TL.solve(ev, tf, insts, dict(tol=TOL, max_iter=40))
    far = TL.solve(ev, tf, insts, dict(tol=TOL, max_iter=40, rules=RR.RULE_RESIDUAL, crawl_limit=1000000))
    ev.close()
    show("rule off", off["res"])
    show("crawl_limit 1000000", far["res"])
    assert TL.same_bits(off, far, (1, 1))
    drop = lambda q: {k: v for k, v in q.items() if k not in ("newton_steps", "restored_steps")}
    assert drop(off["res"][1]) == drop(far["res"][1]) and off["res"][1]["status"] == LR.MAX_ITER
    assert all(q["newton_steps"] == 0 == q["restored_steps"] for q in off["res"])


@pytest.mark.parametrize("tf", LR.TFS)
def test_the_ladder_takes_the_rule_per_rung(built, tf):
    import test_gpu_ladder as TG
    insts = LD.instances(tf)
    ev = TG.fresh_ev(tf, insts)
    r = TG.climb(ev, tf, insts, LD.LADDER, dict(tol=TOL, **RULE))
    ev.close()
    for g, Mg in enumerate(LD.LADDER):
        show(f"tf {tf} rung {Mg}", r["res"][g])
    for g in range(len(LD.LADDER)):
        assert all(q["status"] == LR.CONVERGED for q in r["res"][g]), (g, [q["status"] for q in r["res"][g]])
