"""emi_ipm_solve_shard_dev / _host: the lock-step interior-point solve of a context's whole batch on one mesh.  -m gpu

Cases and fixture: tests/lockstep_ref.py, tests/golden/lockstep_cases.json (the project's own solve_nlp on the CPU oracle with the
dense host factorisation).  The solve criterion is the project's existing one (tests/test_gpu_solve.py): relative cost within 1e-6
of the fixture's AND the trajectory within 1e-6 of the KKT point the independent Newton polish (tests/indep_nlp.py) reaches from
it, with kkt_ok.  The polish finds its active set with a threshold of 1e-7 on the bound and row slacks, which a point solved to 1e-8
does not resolve (a weakly active bound keeps a slack of mu / multiplier ~ 1e-6 there: from solve_nlp's own 1e-8 solutions of these
cases the polish drops such bounds and walks to another point).  tests/test_gpu_solve.py therefore solves to 1e-10 where it polishes,
and so does this file: the polish starts from the SAME instance solved by the same call with tol 1e-10, and the 1e-8 trajectory under
test must lie within 1e-6 of the KKT point reached (no less than asked: the point under test is held to a polished KKT point with
kkt_ok).  The iteration counts may differ from the fixture's -- a Schur complement with 1e-9 dual regularisation and steps
refined to 1e-10 instead of a dense LDL^T, and the rules the driver leaves out -- but their sum over a batch stays within 1.5 x."""
import ctypes as C

import numpy as np
import pytest

import lockstep_ref as LR

pytestmark = pytest.mark.gpu

TOL = 1e-8
TOL_FINE = 1e-10        # where the polish starts (module docstring)
NV, NS, NC, NP, M = 8, 6, 2, 2, LR.M_NODES


def make_ev(tf, insts, f32=False):
    import etol_amd as E
    ev = E.Evaluator(0, f32=f32)
    ev.set_mesh(M, 0.0, tf)
    ev.set_model(1, LR.QUAD_PARAMS)
    ev.set_batch(len(insts))
    ev.set_path(np.stack([LR.records(i["discs"]) for i in insts]), 0, 1)
    return ev


def host_arrays(tf, insts):
    P = LR.quad(tf)
    z0 = np.stack([i["z0"] for i in insts]).reshape(len(insts), NV, M)
    return (np.ascontiguousarray(z0[:, :NS]), np.ascontiguousarray(z0[:, NS:]), np.ascontiguousarray(P.lo.reshape(1, NV, M)),
            np.ascontiguousarray(P.up.reshape(1, NV, M)))


def solve(ev, tf, insts, options, dev=True):
    """one call on fresh copies of the starts -> dict X U LamF LamC (numpy) and res (list of dicts)"""
    import torch
    X, U, zl, zu = host_arrays(tf, insts)
    if dev:
        up = lambda a: torch.from_numpy(a.copy()).to(ev.device)
        X, U, zl, zu = up(X), up(U), up(zl), up(zu)
        torch.cuda.synchronize()
    bd = dict(zl=zl, zu=zu, cl=LR.CL, cu=LR.CU, cscale=LR.CSCALE)
    LamF, LamC, res = ev.ipm_solve_shard(X, U, bd, options, dev=dev)
    keep = dict(tX=X, tU=U, tLamF=LamF, tLamC=LamC, tzl=zl, tzu=zu)
    if dev:
        ev.synchronize()
        X, U, LamF, LamC = (t.cpu().numpy() for t in (X, U, LamF, LamC))
    return dict(X=X, U=U, LamF=LamF, LamC=LamC, res=res, **keep)


def same_bits(a, b, instances=None):
    for k in ("X", "U", "LamF", "LamC"):
        x, y = (a[k], b[k]) if instances is None else (a[k][instances[0]], b[k][instances[1]])
        if not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            return False
    return True


def meets_the_solve_criterion(tf, inst, row, X, U, cost, Xfine, Ufine, tag):
    """(X, U, cost): the solution under test; (Xfine, Ufine): the same instance solved to 1e-10, where the polish starts"""
    import indep_nlp as N
    P = LR.quad(tf, inst["discs"])
    z, lamF, lamC, k = N.polish(P, np.concatenate([Xfine.ravel(), Ufine.ravel()]))
    assert N.kkt_ok(k), (tag, k)
    Xs, Us = P.split(z)[0][0], P.split(z)[1][0]
    ex, eu = np.abs(X - Xs).max() / np.abs(Xs).max(), np.abs(U - Us).max() / np.abs(Us).max()
    print(f"{tag}: cost {cost:.9f} fixture {row['cost']:.9f} polished {P.cost(z):.9f}; rel err states {ex:.2e} controls {eu:.2e}")
    assert abs(cost - row["cost"]) < 1e-6 * abs(row["cost"]), (tag, cost, row["cost"])
    assert ex < 1e-6 and eu < 1e-6, (tag, ex, eu)


@pytest.fixture(scope="module")
def batch_a(built):
    """batch A of both final times, solved once: tf -> (instances, fixture rows, first call's outcome); the contexts stay open"""
    out, evs = {}, []
    fx = LR.fixture()["cases"]
    for tf in LR.TFS:
        insts = LR.instances(tf)
        ev = make_ev(tf, insts)
        evs.append(ev)
        out[tf] = dict(insts=insts, rows=fx[str(tf)], ev=ev, first=solve(ev, tf, insts, dict(tol=TOL, max_iter=200)),
                       fine=solve(ev, tf, insts, dict(tol=TOL_FINE, max_iter=80)))
    yield out
    for ev in evs:
        ev.close()


@pytest.mark.parametrize("tf", LR.TFS)
def test_batch_a_converges_to_the_fixtures_optima(batch_a, tf):
    import torch
    a = batch_a[tf]
    r, res, ev = a["first"], a["first"]["res"], a["ev"]
    B = len(res)
    for b in range(B):
        print(f"tf {tf} instance {b}: status {res[b]['status']} iterations {res[b]['iterations']} (fixture {a['rows'][b]['iterations']}) "
              f"evaluations {res[b]['evaluations']} factorisations {res[b]['factorisations']} reflected {res[b]['reflected_steps']} "
              f"kkt {res[b]['kkt_error']:.2e} viol {res[b]['constr_viol']:.2e} emax {res[b]['emax']:.2e} rho {res[b]['rho']:g} cost {res[b]['cost']:.6f}")
    print(f"tf {tf} solved to {TOL_FINE:g}: status / iterations", [(q["status"], q["iterations"]) for q in a["fine"]["res"]])
    status = [q["status"] for q in res]
    assert all(s in (LR.CONVERGED, LR.ACCEPTABLE) for s in status) and status.count(LR.ACCEPTABLE) <= 1, status
    assert all(q["kkt_error"] <= TOL for q in res if q["status"] == LR.CONVERGED)
    # the returned arrays go straight into the certificate
    kw = dict(dtype=torch.float64, device=ev.device)
    RES, VALS, COST = torch.zeros((B, NS + NP, M), **kw), torch.zeros((B, ev.layout.nvals, M), **kw), torch.zeros(B, **kw)
    cert = torch.zeros((B, 6), **kw)
    torch.cuda.synchronize()
    ev.eval_dev(r["tX"], r["tU"], RES, VALS, COST)
    ev.kkt_certificate_dev(r["tX"], r["tU"], RES, VALS, r["tLamF"], r["tLamC"], 1.0, r["tzl"], r["tzu"], LR.CL, LR.CU, cert)
    ev.synchronize()
    cert, cost = cert.cpu().numpy(), COST.cpu().numpy()
    for b in range(B):
        print(f"  certificate {b}: stat {cert[b, 0]:.2e} comp {cert[b, 1]:.2e} defect {cert[b, 2]:.2e} viol {cert[b, 3]:.2e}")
        assert cert[b, 2] <= TOL and cert[b, 3] <= TOL
        assert cost[b] == res[b]["cost"]                    # the same evaluation: the same bits
        meets_the_solve_criterion(tf, a["insts"][b], a["rows"][b], r["X"][b], r["U"][b], res[b]["cost"], a["fine"]["X"][b], a["fine"]["U"][b],
                                  f"tf {tf} instance {b}")
    mine, theirs = sum(q["iterations"] for q in res), sum(q["iterations"] for q in a["rows"])
    print(f"tf {tf}: {mine} iterations over the batch, fixture {theirs}")
    assert mine <= 1.5 * theirs


@pytest.mark.parametrize("tf", LR.TFS)
def test_two_calls_give_the_same_bits_and_nothing_touches_a_finished_instance(batch_a, tf):
    a = batch_a[tf]
    first, ev, insts = a["first"], a["ev"], a["insts"]
    second = solve(ev, tf, insts, dict(tol=TOL, max_iter=200))
    assert same_bits(first, second) and first["res"] == second["res"]
    its = [q["iterations"] for q in first["res"]]
    n = min(its)
    third = solve(ev, tf, insts, dict(tol=TOL, max_iter=n))
    done = [b for b, i in enumerate(its) if i == n]
    for b in range(len(insts)):
        if b in done:
            assert same_bits(first, third, (b, b)) and third["res"][b] == first["res"][b], b
        else:
            assert third["res"][b]["status"] == LR.MAX_ITER and third["res"][b]["iterations"] == n, third["res"][b]


def test_a_batch_of_one_agrees_with_the_batch_of_nine(batch_a):
    tf = LR.TFS[0]
    a = batch_a[tf]
    for b in (0, 4, 8):
        ev = make_ev(tf, [a["insts"][b]])
        one = solve(ev, tf, [a["insts"][b]], dict(tol=TOL, max_iter=200))
        ev.close()
        assert one["res"][0]["status"] in (LR.CONVERGED, LR.ACCEPTABLE)
        dx = np.abs(one["X"][0] - a["first"]["X"][b]).max() / np.abs(one["X"][0]).max()
        du = np.abs(one["U"][0] - a["first"]["U"][b]).max() / np.abs(one["U"][0]).max()
        print(f"instance {b}: alone {one['res'][0]['iterations']} iterations, in the batch {a['first']['res'][b]['iterations']}; {dx:.2e} {du:.2e}")
        assert dx < 1e-6 and du < 1e-6


def test_an_instance_without_a_feasible_path_ends_alone(batch_a):
    tf = LR.TFS[0]
    a = batch_a[tf]
    blocked = dict(discs=LR.discs_of(LR.NO_PATH_DISC), bump=0.0, z0=a["insts"][0]["z0"])
    insts = [a["insts"][1], blocked, a["insts"][5]]
    ev = make_ev(tf, insts)
    r = solve(ev, tf, insts, dict(tol=TOL, max_iter=40))
    fine = solve(ev, tf, insts, dict(tol=TOL_FINE, max_iter=40))
    ev.close()
    for b, q in enumerate(r["res"]):
        print(f"instance {b}: status {q['status']} iterations {q['iterations']} evaluations {q['evaluations']} kkt {q['kkt_error']:.2e} "
              f"viol {q['constr_viol']:.2e} emax {q['emax']:.2e} rho {q['rho']:g}")
    bad = r["res"][1]
    assert bad["status"] not in (LR.CONVERGED, LR.ACCEPTABLE) and (bad["constr_viol"] > 1e-3 or bad["emax"] > 1e-3)
    for b, src in ((0, 1), (2, 5)):
        assert r["res"][b]["status"] in (LR.CONVERGED, LR.ACCEPTABLE)
        meets_the_solve_criterion(tf, insts[b], a["rows"][src], r["X"][b], r["U"][b], r["res"][b]["cost"], fine["X"][b], fine["U"][b],
                                  f"beside the blocked instance: {b}")


def test_status_codes_and_the_host_form(batch_a):
    import torch
    import etol_amd as E
    from etol_amd import _lib as L
    tf = LR.TFS[0]
    insts = batch_a[tf]["insts"][:2]
    lib = E.load()
    Xh, Uh, zlh, zuh = host_arrays(tf, insts)

    def call(ev, drop=None, host=False):
        if host:
            X, U, zl, zu = (a.copy() for a in (Xh, Uh, zlh, zuh))
            LF, LC = np.zeros((2, NS, M)), np.zeros((2, NP, M))
            p = lambda a: C.c_void_p(a.ctypes.data)
        else:
            X, U, zl, zu = (torch.from_numpy(a.copy()).to(ev.device) for a in (Xh, Uh, zlh, zuh))
            LF, LC = (torch.zeros((2, n, M), dtype=torch.float64, device=ev.device) for n in (NS, NP))
            torch.cuda.synchronize()
            p = lambda t: C.c_void_p(t.data_ptr())
        bd = L.IpmBounds()
        bd.zl, bd.zu, bd.nsets = p(zl), p(zu), 1
        bd.cl, bd.cu = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (LR.CL, LR.CU))
        opt, res = L.IpmOptions(), (L.IpmResult * 2)()
        opt.max_iter = 3
        args = dict(X=p(X), U=p(U), bd=C.byref(bd), opt=C.byref(opt), LF=p(LF), LC=p(LC), res=res)
        if drop:
            args[drop] = None
        fn = lib.emi_ipm_solve_shard_host if host else lib.emi_ipm_solve_shard_dev
        st = fn(ev.ctx if ev is not None else None, *(args[k] for k in ("X", "U", "bd", "opt", "LF", "LC", "res")))
        if not host and ev is not None:
            ev.synchronize()
        return st, (X, U, LF, LC), [{n: getattr(q, n) for n, _ in L.IpmResult._fields_} for q in res]

    ev = make_ev(tf, insts, f32=True)
    assert call(ev)[0] == 5                                     # EMI_ERR_UNSUPPORTED: f32 context
    ev.close()
    ev = make_ev(tf, insts)
    ev.set_delays(0, 1, 0.1)
    assert call(ev)[0] == 5                                     # delays set
    ev.close()
    ev = E.Evaluator(0)
    assert call(ev)[0] == 2                                     # EMI_ERR_STATE: no mesh, model or batch
    ev.close()
    ev = make_ev(tf, insts)
    ev.set_option("kkt_method", 0)
    assert call(ev)[0] == 5                                     # the LU method
    ev.set_option("kkt_method", 1)
    for drop in ("X", "U", "bd", "opt", "LF", "LC", "res"):
        assert call(ev, drop)[0] == 1, drop                     # EMI_ERR_ARG: NULL where not optional
    assert call(None, host=True)[0] == 1 and lib.emi_ipm_solve_shard_dev(None, None, None, None, None, None, None, None) == 1
    st, dev, rd = call(ev)
    st2, host, rh = call(ev, host=True)
    assert st == 0 and st2 == 0 and rd == rh and all(q["status"] == LR.MAX_ITER and q["iterations"] == 3 for q in rd), (rd, rh)
    for t, h in zip(dev, host):
        assert np.array_equal(t.cpu().numpy().view(np.uint8), h.view(np.uint8))
    ev.close()


def test_error_components_and_the_start_on_the_device(built):
    """the three-instance set-up of tests/test_gpu_kkt_shard.py::test_one_iteration_of_a_shard_on_the_device: emi_ipm_error_parts_dev
    against numpy within the bounds of lockstep_ref.error_parts_ref, emi_ipm_error_dev's kkt_error reproduced from the components
    within 4 eps (pmax + mu) / sc; then emi_ipm_start_dev against start()'s formulas: equal bits"""
    import torch
    import ipm_ref as R
    from etol_amd import workloads as W
    from test_gpu_ipm import DevBackend
    from test_gpu_ipm import make_ev as ipm_ev
    nv, ns, nc, npth, Mn, B = 8, 6, 2, 3, 33, 3
    c = dict(nv=nv, ns=ns, nc=nc, np=npth, M=Mn, B=B, nsets=B, model=1, nvals=ns * nv + 2 * npth + nv, rows=R.default_rows(ns, nv, npth),
             cscale=None, rs=None, DefRes=None, RowRes=None)
    ev = ipm_ev(c)
    rng = np.random.default_rng(5)
    X, U, _ = W.quadrotor_batch(7, B, Mn, 0)
    RES0, VALS0, _ = ev.eval_host(X, U)
    z = np.concatenate([X, U], 1)
    zl, zu = z - (1.0 + np.abs(z)), z + (1.0 + np.abs(z))
    zl[:, nv - 1], zu[:, 3] = -1e20, 1e20
    zl[:, :ns, 0] = zu[:, :ns, 0] = z[:, :ns, 0]
    cl, cu = np.full(npth, -1e20), np.zeros(npth)
    cpath = RES0[:, ns:]
    Sl = np.minimum(cpath, -0.01)
    gap = cpath - Sl
    ee = 0.01 * np.maximum(1.0, np.abs(gap))
    rho = 10.0
    c.update(X=X, U=U, S=Sl, E1=np.maximum(gap, 0) + ee, E2=np.maximum(-gap, 0) + ee, zl=zl, zu=zu, cl=cl, cu=cu,
             LamF=0.1 * rng.standard_normal((B, ns, Mn)), Y=0.05 * rng.standard_normal((B, npth, Mn)),
             ZL=np.where((zu > zl) & (zl > -R.INF), 1.0, 0.0), ZU=np.where((zu > zl) & (zu < R.INF), 1.0, 0.0),
             VL=np.zeros((B, npth, Mn)), VU=np.ones((B, npth, Mn)),
             par=np.array([[0.1, rho, 0.99, 1.0], [0.05, rho, 0.99, 1.0], [0.2, rho, 0.99, 1.0]]), RES=RES0)
    c["W1"], c["W2"] = rho - c["Y"], rho + c["Y"]
    c["G"] = ev.lagr_grad_host(VALS0, c["LamF"], c["Y"])
    be = DevBackend(ev)
    pt, du, bd, par = be.group(R.POINT, c), be.group(R.DUALS, c), be.bounds(c), be.up(c["par"])
    RESd, Gd = be.up(c["RES"]), be.up(c["G"])
    parts = torch.full((B, 8), float("nan"), dtype=torch.float64, device=ev.device)
    err = torch.full((B, 3), float("nan"), dtype=torch.float64, device=ev.device)
    torch.cuda.synchronize()
    ev.ipm_error_parts(pt, du, RESd, Gd, bd, par, parts)
    ev.ipm_error(pt, du, RESd, Gd, bd, par, err)
    ev.synchronize()
    parts, err = parts.cpu().numpy(), err.cpu().numpy()
    ref = LR.error_parts_ref(c)
    for b in range(B):
        want, tol = ref[b]
        for i, k in enumerate(LR.PARTS):
            print(f"instance {b} {k}: {parts[b, i]:.16e} numpy {want[k]:.16e} (bound {tol[k]:.1e})")
            assert abs(parts[b, i] - want[k]) <= tol[k], (b, k)
        p = dict(zip(LR.PARTS, parts[b]))
        mu = c["par"][b, 0]
        again = LR.kkt(p, mu)
        print(f"instance {b}: kkt_error {err[b, 0]:.16e}, from the components {again:.16e}")
        assert abs(again - err[b, 0]) <= 4 * LR.EPS * (p["pmax"] + mu) / p["sc"]
        assert err[b, 1] == p["ep"] and err[b, 2] == p["emax"]
    # the start kernel: interior push and fixed bytes, then slacks, elastics and multipliers from the path values; W reset under a mask
    far = z + rng.standard_normal(z.shape) * (1.0 + np.abs(z)) * 1.5          # inside and outside the bounds
    far[:, :nv - 1, 5] = zl[:, :nv - 1, 5]                                   # on a bound
    Xd, Ud = be.up(far[:, :ns]), be.up(far[:, ns:])
    poison = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=ev.device)
    d2 = {n: poison(B, ns if n == "LamF" else nv if n in ("ZL", "ZU") else npth, Mn) for n in R.DUALS}
    p2 = dict(X=Xd, U=Ud, S=poison(B, npth, Mn), E1=poison(B, npth, Mn), E2=poison(B, npth, Mn))
    fixed = torch.full((B, nv, Mn), 7, dtype=torch.uint8, device=ev.device)
    torch.cuda.synchronize()
    ev.ipm_start(0, p2, d2, bd, fixed=fixed)
    # (a second set of row bounds with both sides present, through the same kernel)
    cases = [(bd, cl, cu)]
    cl2, cu2 = np.array([-1000.0, -1e20, -0.5]), np.array([0.0, 0.3, 1e20])
    cases.append((dict(bd, cl=cl2, cu=cu2, cscale=np.array([1.0, 2.5, 0.5])), cl2, cu2))
    ev.synchronize()
    zp, fx = LR.start_point_ref(far, zl, zu)
    got = np.concatenate([Xd.cpu().numpy(), Ud.cpu().numpy()], 1)
    assert np.array_equal(got.view(np.uint8), zp.view(np.uint8)) and np.array_equal(fixed.cpu().numpy(), fx)
    assert np.array_equal(d2["LamF"].cpu().numpy(), np.zeros((B, ns, Mn)))
    assert ((got > zl) & (got < zu))[zu > zl].all() and (got != far).any() and (got == far).any()
    for bnd, l, u in cases:
        ev.ipm_start(1, p2, d2, bnd, RES=RESd, par=par, fixed=fixed)
        ev.synchronize()
        cs = bnd.get("cscale") if bnd.get("cscale") is not None else np.ones(npth)
        want = LR.start_rows_ref(cpath, zl, zu, l, u, cs, rho)
        for k, w in want.items():
            g = (p2[k] if k in p2 else d2[k]).cpu().numpy()
            assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), k
    Y = be.up(c["Y"])
    d3 = dict(d2, Y=Y)
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device=ev.device)
    before = d2["W1"].cpu().numpy().copy()
    torch.cuda.synchronize()
    ev.ipm_start(2, p2, d3, bd, par=par, mask=mask)
    ev.synchronize()
    W1, W2 = d2["W1"].cpu().numpy(), d2["W2"].cpu().numpy()
    for b in range(B):
        if b == 1:
            assert np.array_equal(W1[b].view(np.uint8), before[b].view(np.uint8))
        else:
            assert np.array_equal(W1[b], np.maximum(1e-8, rho - c["Y"][b])) and np.array_equal(W2[b], np.maximum(1e-8, rho + c["Y"][b]))
    ev.close()
