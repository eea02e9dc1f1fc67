"""emi_ipm_* (reduce, expand, trial, merit, accept, error; _dev and _host forms) and emi_kkt_solve_dev: the array arithmetic of an
interior-point iteration as batched kernels, against the numpy reference (tests/ipm_ref.py, np.longdouble).  -m gpu

Cases, bounds and checks are the ones tests/test_ipm_cpu.py validates on the host functions (ipm_ref.case_list / run_checks):
element-wise outputs within c eps sum|terms| (c by the rules at the top of ipm_ref.py), sums within (n - 1) eps sum|terms|,
apr / adu / mmax / emax within 4 eps relative, viol and the parts of kkt_error (maxima of cancelling residuals) within 4 eps of
their terms, kkt_error with the scale sums' summation error passed through its divisions; steps to the boundary stay strictly inside, multipliers stay positive, fixed variables stay out of everything.
Every output buffer is poisoned with NaN before a call."""
import ctypes as C

import numpy as np
import pytest

import ipm_ref as R

pytestmark = pytest.mark.gpu

KEYS = R.case_list()


def make_ev(c, f32=False):
    import etol_amd as E
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    ev = E.Evaluator(0, f32=f32)
    ev.set_mesh(c["M"], 0.0, 4.0)
    ev.set_model(c["model"], {0: [], 1: W.QUAD_PARAMS, 2: W.FW_PARAMS}[c["model"]])
    ev.set_batch(c["B"])
    if c["np"]:
        recs = np.zeros((c["np"], L.PATH_REC))
        recs[:, 0] = L.PATH_DISC
        recs[:, 1:4] = R.DISCS[:c["np"]]
        ev.set_path(recs, 0, 1)
    lay = ev.layout
    assert (lay.ns + lay.nc, lay.ns, lay.np, lay.nvals) == (c["nv"], c["ns"], c["np"], c["nvals"])
    if c.get("custom_rows"):
        ev.kkt_blocks_rows(c["rows"])
    return ev


class DevBackend:
    """the kernels through Evaluator.ipm_*: dev=True on torch tensors (asynchronous, downloaded after a synchronise), dev=False the
    _host forms on numpy arrays"""

    def __init__(self, ev, dev=True):
        self.ev, self.dev = ev, dev

    def up(self, a):
        import torch
        if a is None or a.size == 0:
            return None
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.copy()).to(self.ev.device) if self.dev else a.copy()

    def poison(self, *shape):
        return self.up(np.full(shape, np.nan)) if int(np.prod(shape)) else None

    def down(self, t, shape=None):
        if t is None:
            return np.zeros(shape)
        return t.cpu().numpy() if self.dev else t

    def run(self, name, *args, **kw):
        import torch
        if self.dev:
            torch.cuda.synchronize()        # the uploads went over torch's stream
        getattr(self.ev, "ipm_" + name)(*args, dev=self.dev, **kw)
        if self.dev:
            self.ev.synchronize()

    def group(self, names, src):
        return {n: self.up(src[n]) for n in names if src.get(n) is not None}

    def bounds(self, c):
        return dict(zl=self.up(c["zl"]), zu=self.up(c["zu"]), cl=c["cl"], cu=c["cu"], cscale=c.get("cscale"))

    def reduce(self, c):
        B, nv, ns, npth, M = c["B"], c["nv"], c["ns"], c["np"], c["M"]
        el = dict(Sigma=self.poison(B, nv, M), **{n: self.poison(B, npth, M) for n in ("SigT", "SigS", "RhatS", "Rt")})
        rhs = self.poison(B, nv + ns, M)
        self.run("reduce", self.group(R.POINT, c), self.group(R.DUALS, c), self.up(c["RES"]), self.up(c["VALS"]), self.up(c["G"]), self.bounds(c),
                 self.up(c["par"]), el, rhs, DefRes=self.up(c.get("DefRes")), RowRes=self.up(c.get("RowRes")))
        out = {n: self.down(el[n], (B, npth, M)) for n in el}
        out["Rhs"] = self.down(rhs)
        return out

    def expand(self, c, el, dzlam):
        B, nv, npth, M = c["B"], c["nv"], c["np"], c["M"]
        st = {n: self.poison(B, nv if n in ("DZL", "DZU") else npth, M) for n in R.STEP[1:]}
        st["DZLam"] = self.up(dzlam)
        scal = self.poison(B, 4)
        self.run("expand", self.group(R.POINT, c), self.group(R.DUALS, c), self.up(c["VALS"]), self.bounds(c), self.up(c["par"]),
                 self.group(R.ELIM, el), st, scal, rs=self.up(c.get("rs")))
        return {n: self.down(st[n], (B, npth, M)) for n in st}, self.down(scal)

    def trial(self, c, st, alpha):
        B, ns, nc, npth, M = c["B"], c["ns"], c["nc"], c["np"], c["M"]
        tr = dict(X=self.poison(B, ns, M), U=self.poison(B, nc, M), **{n: self.poison(B, npth, M) for n in ("S", "E1", "E2")})
        self.run("trial", self.group(R.POINT, c), self.group(R.STEP, st), self.up(alpha), tr)
        return {n: self.down(tr[n]) for n in tr if tr[n] is not None}

    def merit(self, c, pt, reset):
        B = c["B"]
        p = self.group(R.POINT, pt)
        out = self.poison(B, 2)
        self.run("merit", p, self.up(pt["RES"]), self.up(pt["COST"]), self.bounds(c), self.up(c["par"]), out, rs=self.up(c.get("rs")), reset=reset)
        return self.down(p.get("S"), pt["S"].shape), self.down(out)

    def accept(self, c, trial, st, a_pr, a_du, mask=None):
        p, d = self.group(R.POINT, c), self.group(R.DUALS, c)
        self.run("accept", p, self.group(R.POINT, trial), d, self.group(R.STEP, st), self.bounds(c), self.up(c["par"]), self.up(a_pr), self.up(a_du),
                 mask=self.up(mask))
        out = {n: self.down(d[n], c[n].shape) for n in d}
        out.update({n: self.down(p[n], c[n].shape) for n in p})
        return out

    def error(self, c):
        out = self.poison(c["B"], 3)
        self.run("error", self.group(R.POINT, c), self.group(R.DUALS, c), self.up(c["RES"]), self.up(c["G"]), self.bounds(c), self.up(c["par"]), out)
        return self.down(out)


@pytest.mark.parametrize("key", KEYS, ids=R.case_id)
def test_kernels_against_the_reference(built, key):
    c = R.get_case(key)
    ev = make_ev(c)
    fig = R.run_checks(c, DevBackend(ev), log=print)
    assert c["np"] == 0 or fig["jumped"] > 0
    ev.close()


def all_outputs(c, be, mask=None):
    """every output of every call on the case's own inputs, as one dict of numpy arrays"""
    out = {}
    red = be.reduce(c)
    out.update({"red." + k: v for k, v in red.items()})
    st, scal = be.expand(c, red, c["DZLam"].copy())
    out.update({"st." + k: v for k, v in st.items()})
    out["scal"] = scal
    alpha = c["alpha"] * scal[:, 0]
    tr = be.trial(c, st, alpha)
    out.update({"tr." + k: v for k, v in tr.items()})
    for k in R.POINT:
        tr.setdefault(k, np.zeros((c["B"], 0, c["M"])))
    pt = dict(tr, RES=c["RES"], COST=c["COST"])
    S1, m1 = be.merit(c, pt, True)
    out["merit.S"], out["merit"] = S1, m1
    out["merit0"] = be.merit(c, pt, False)[1]
    new = be.accept(c, tr, st, alpha, c["a_du"] * scal[:, 1], mask=mask)
    out.update({"acc." + k: v for k, v in new.items()})
    out["error"] = be.error(c)
    return out, tr, st, scal


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("key", [k for k in KEYS if k[3] == 257 and k[4] == 3 and k[2] == 3] + [k for k in KEYS if k[6] in ("cscale", "soc")],
                         ids=R.case_id)
def test_two_calls_and_both_forms_give_the_same_bits(built, key):
    c = R.get_case(key)
    ev = make_ev(c)
    first = all_outputs(c, DevBackend(ev))[0]
    same_bits(first, all_outputs(c, DevBackend(ev))[0])
    same_bits(first, all_outputs(c, DevBackend(ev, dev=False))[0])
    ev.close()


def test_masked_instances_keep_every_bit(built):
    c = R.get_case(next(k for k in KEYS if k[4] == 3 and k[2] == 3 and k[3] == 33 and k[6] == "plain"))
    ev = make_ev(c)
    be = DevBackend(ev)
    full, tr, st, scal = all_outputs(c, be)
    mask = np.array([1, 0, 1], dtype=np.uint8)
    new = be.accept(c, tr, st, c["alpha"] * scal[:, 0], c["a_du"] * scal[:, 1], mask=mask)
    for k, v in new.items():
        assert np.array_equal(v[1].view(np.uint8), c[k][1].view(np.uint8)), k               # untouched
        assert np.array_equal(v[[0, 2]].view(np.uint8), full["acc." + k][[0, 2]].view(np.uint8)), k
        assert not np.array_equal(v[0], c[k][0]) or v[0].size == 0, k
    ev.close()


def test_a_trial_point_outside_a_bound_costs_that_instance_alone(built):
    c = R.get_case(next(k for k in KEYS if k[4] == 3 and k[2] == 3 and k[3] == 257))
    ev = make_ev(c)
    be = DevBackend(ev)
    pt = {k: c[k] for k in R.POINT}
    pt.update(RES=c["RES"], COST=c["COST"])
    good = be.merit(c, pt, False)[1]
    assert np.isfinite(good).all()
    bad = dict(pt, U=c["U"].copy(), E1=c["E1"].copy())
    zu = np.broadcast_to(c["zu"], (c["B"], c["nv"], c["M"]))
    v = next(v for v in range(c["ns"], c["nv"]) if zu[1, v, 200] < R.INF)
    bad["U"][1, v - c["ns"], 200] = zu[1, v, 200] + 0.5         # beyond an upper bound: log of a negative gap
    out = be.merit(c, bad, False)[1]
    assert not np.isfinite(out[1, 0]) and np.isfinite(out[1, 1])
    assert np.array_equal(out[[0, 2]].view(np.uint8), good[[0, 2]].view(np.uint8))
    bad["E1"][1, 0, 3] = -0.25                                   # ... and with the slack reset in front
    S1, out = be.merit(c, bad, True)
    assert not np.isfinite(out[1, 0])
    Sg, outg = be.merit(c, pt, True)
    assert np.array_equal(out[[0, 2]].view(np.uint8), outg[[0, 2]].view(np.uint8)) and np.array_equal(S1[[0, 2]], Sg[[0, 2]])
    ev.close()


def test_status_codes(built):
    import etol_amd as E
    from etol_amd import _lib as L
    c = R.get_case(next(k for k in KEYS if k[:3] == (4, 2, 3) and k[3] == 33))
    ev = make_ev(c, f32=True)
    with pytest.raises(E.EmiError, match="EMI_ERR_UNSUPPORTED.*f64"):
        DevBackend(ev, dev=False).error(c)
    ev.close()
    ev = make_ev(c)
    ev.set_delays(0, 1, 0.1)
    with pytest.raises(E.EmiError, match="EMI_ERR_UNSUPPORTED.*delays"):
        DevBackend(ev, dev=False).error(c)
    ev.close()
    ev = make_ev(c)
    lib = E.load()
    for form in ("dev", "host"):
        for name, nargs in (("reduce", 11), ("expand", 9), ("trial", 4), ("accept", 9), ("error", 7)):
            assert getattr(lib, f"emi_ipm_{name}_{form}")(ev.ctx, *([None] * nargs)) == 1, (name, form)          # EMI_ERR_ARG
            assert getattr(lib, f"emi_ipm_{name}_{form}")(None, *([None] * nargs)) == 1
        assert getattr(lib, f"emi_ipm_merit_{form}")(ev.ctx, None, None, None, None, None, None, 0, None) == 1
    be = DevBackend(ev)
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG"):            # a group with a missing array
        p = be.group(R.POINT, c)
        del p["E2"]
        ev.ipm_error(p, be.group(R.DUALS, c), be.up(c["RES"]), be.up(c["G"]), be.bounds(c), be.up(c["par"]), be.poison(c["B"], 3))
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG.*bounds"):    # nsets neither 1 nor the batch
        bd = be.bounds(c)
        bd["zl"] = be.up(np.concatenate([c["zl"]] * 2)); bd["zu"] = be.up(np.concatenate([c["zu"]] * 2))
        ev.ipm_error(be.group(R.POINT, c), be.group(R.DUALS, c), be.up(c["RES"]), be.up(c["G"]), bd, be.up(c["par"]), be.poison(c["B"], 3))
    assert lib.emi_kkt_solve_dev(ev.ctx, None, 1) == 1
    import torch
    x = torch.zeros((c["nv"] + c["ns"]) * c["M"], dtype=torch.float64, device=ev.device)
    with pytest.raises(E.EmiError, match="EMI_ERR_STATE.*factor"):
        ev.kkt_solve_dev(x)
    ev.close()


def test_one_iteration_on_the_device(built):
    """quadrotor, 33 nodes, 3 discs, one instance, an interior start: evaluation, Lagrangian gradient, reduction, node blocks,
    factorisation, solve, expansion, trial point, evaluation there, merit, acceptance and KKT error, all on device arrays; between
    the stages only scalars (info of the factorisation) reach the host.  Every stage is then checked on ITS downloaded inputs."""
    import torch
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    from test_gpu_kkt import dense_kkt
    nv, ns, nc, npth, M, B = 8, 6, 2, 3, 33, 1
    nh = nv * (nv + 1) // 2
    c = dict(nv=nv, ns=ns, nc=nc, np=npth, M=M, B=B, nsets=1, model=1, nvals=ns * nv + 2 * npth + nv, rows=R.default_rows(ns, nv, npth),
             cscale=None, rs=None, DefRes=None, RowRes=None)
    ev = make_ev(c)
    rng = np.random.default_rng(5)
    X, U, _ = W.quadrotor_batch(7, B, M, 0)
    RES0, _, _ = ev.eval_host(X, U)
    # the start as solve_nlp makes it: bounds around the point, the initial state fixed, slacks pushed inside, elastics closing the rows
    z = np.concatenate([X, U], 1)
    zl, zu = z - (1.0 + np.abs(z)), z + (1.0 + np.abs(z))
    zl[:, nv - 1], zu[:, 3] = -1e20, 1e20           # one side absent here and there
    zl[:, :ns, 0] = zu[:, :ns, 0] = z[:, :ns, 0]
    cl, cu = np.full(npth, -1e20), np.zeros(npth)
    cpath = RES0[:, ns:]
    S = np.minimum(cpath, -0.01)
    gap = cpath - S
    ee = 0.01 * np.maximum(1.0, np.abs(gap))
    rho = 10.0
    c.update(X=X, U=U, S=S, E1=np.maximum(gap, 0) + ee, E2=np.maximum(-gap, 0) + ee, zl=zl, zu=zu, cl=cl, cu=cu,
             LamF=0.1 * rng.standard_normal((B, ns, M)), Y=0.05 * rng.standard_normal((B, npth, M)),
             ZL=np.where((zu > zl) & (zl > -R.INF), 1.0, 0.0), ZU=np.where((zu > zl) & (zu < R.INF), 1.0, 0.0),
             VL=np.zeros((B, npth, M)), VU=np.ones((B, npth, M)), par=np.array([[0.1, rho, 0.99, 1.0]]))
    c["W1"], c["W2"] = rho - c["Y"], rho + c["Y"]
    fixed = np.ascontiguousarray((~(zu > zl)).astype(np.uint8))

    be = DevBackend(ev)
    kw = dict(dtype=torch.float64, device=ev.device)
    nan = lambda *s: torch.full(s, float("nan"), **kw)
    pt, du, bd, par = be.group(R.POINT, c), be.group(R.DUALS, c), be.bounds(c), be.up(c["par"])
    fx = be.up(fixed)
    RES, VALS, COST, G, H = nan(B, ns + npth, M), nan(B, c["nvals"], M), nan(B), nan(B, nv, M), nan(B, nh, M)
    el = dict(Sigma=nan(B, nv, M), **{n: nan(B, npth, M) for n in ("SigT", "SigS", "RhatS", "Rt")})
    step = {n: nan(B, nv if n in ("DZL", "DZU") else npth, M) for n in R.STEP[1:]}
    step["DZLam"] = nan(B, nv + ns, M)
    rhs_keep, Q = nan(B, nv + ns, M), nan(B, nh, M)
    count, worst = torch.zeros(B, dtype=torch.int32, device=ev.device), nan(B)
    scal, mer, err = nan(B, 4), nan(B, 2), nan(B, 3)
    trial = dict(X=nan(B, ns, M), U=nan(B, nc, M), **{n: nan(B, npth, M) for n in ("S", "E1", "E2")})
    RESt, COSTt = nan(B, ns + npth, M), nan(B)
    RES2, VALS2, COST2, G2 = nan(B, ns + npth, M), nan(B, c["nvals"], M), nan(B), nan(B, nv, M)
    torch.cuda.synchronize()
    # ---- the chain (one stream; the copies between its arrays are device-to-device on the same stream through torch's plumbing) ----
    ev.eval_dev(pt["X"], pt["U"], RES, VALS, COST)
    ev.lagr_grad_dev(VALS, du["LamF"], du["Y"], 1.0, G)                     # cscale = 1: LamC = Y
    ev.hess_dev(pt["X"], pt["U"], du["LamF"], du["Y"], 1.0, H)
    ev.ipm_reduce(pt, du, RES, VALS, G, bd, par, el, step["DZLam"])
    ev.kkt_blocks_dev(H, VALS, el["Sigma"], el["SigT"], fx, 0.0, Q, 0, count, None, None, None, worst)
    ev.synchronize()
    rhs_keep.copy_(step["DZLam"])                                           # (kept for the checks below)
    torch.cuda.synchronize()
    dc = 1e-9
    assert ev.kkt_factor_dev(Q[0], VALS[0], fx[0].reshape(-1), dc) == 0     # the one scalar that reaches the host
    ev.kkt_solve_dev(step["DZLam"][0].reshape(-1))
    ev.ipm_expand(pt, du, VALS, bd, par, el, step, scal)
    a_pr, a_du = _column(ev, scal, 0), _column(ev, scal, 1)                 # (device arrays: alpha = apr)
    ev.ipm_trial(pt, step, a_pr, trial)
    ev.synchronize()
    S_before = trial["S"].clone()                                           # (kept for the checks below)
    torch.cuda.synchronize()
    ev.eval_dev(trial["X"], trial["U"], RESt, None, COSTt, flags=L.EVAL_ALL | L.EVAL_NOJAC)
    ev.ipm_merit(trial, RESt, COSTt, bd, par, mer, reset=True)
    ev.ipm_accept(pt, trial, du, step, bd, par, a_pr, a_du)
    ev.eval_dev(pt["X"], pt["U"], RES2, VALS2, COST2)
    ev.lagr_grad_dev(VALS2, du["LamF"], du["Y"], 1.0, G2)
    ev.ipm_error(pt, du, RES2, G2, bd, par, err)
    ev.synchronize()
    # ---- every stage on its downloaded inputs ------------------------------------------------------------------------------------
    dn = lambda t: t.cpu().numpy()
    c.update(RES=dn(RES), VALS=dn(VALS), G=dn(G), COST=dn(COST))
    red = {n: dn(el[n]) for n in el}
    red["Rhs"] = dn(rhs_keep)
    ref = R.reduce_ref(c)
    for k in ("Sigma", "Rhs", "SigS", "RhatS", "SigT", "Rt"):
        R.check_elementwise(k, red[k], ref[k], print)
    # the solved step in the matrix numpy builds from the downloaded blocks
    lib = ev.lib
    dca, dwa = C.c_double(dc), C.c_double(0.0)
    assert lib.emi_kkt_last_regularisation(ev.ctx, C.byref(dca), C.byref(dwa)) == 0
    K = dense_kkt(ev.D, dn(Q)[0], c["VALS"][0, :ns * nv], fixed[0].reshape(-1), dca.value, M, ns, nv)
    free_x = np.nonzero(fixed[0, :ns].reshape(-1) == 0)[0]          # what the factorisation itself added, if anything
    K[free_x, free_x] += dwa.value
    st = {n: dn(step[n]) for n in step}
    x, b = st["DZLam"][0].reshape(-1), red["Rhs"][0].reshape(-1)
    assert np.abs(K @ x - b).max() < 1e-9 * (np.abs(K).max() * np.abs(x).max() + 1)
    assert np.array_equal(ev.kkt_solve(b), x), "emi_kkt_solve_dev and emi_kkt_solve differ"
    sref = R.expand_ref(c, red, st["DZLam"])
    for k in R.STEP:
        R.check_elementwise(k, st[k], sref[k], print)
    sc = dn(scal)
    r = R.expand_scalars_ref(c, st)[0]
    R.check_scalar("apr", sc[0, 0], *r["apr"]); R.check_scalar("adu", sc[0, 1], *r["adu"]); R.check_scalar("mmax", sc[0, 3], *r["mmax"])
    R.check_scalar("dphi", sc[0, 2], r["dphi"]["value"], r["dphi"]["tol"])
    tr = {n: dn(trial[n]) for n in trial}
    tref = R.trial_ref(c, st, sc[:, 0])
    S_reset = tr["S"]                       # the merit call reset the slacks in place
    ptm = dict(tr, S=dn(S_before), RES=dn(RESt), COST=dn(COSTt))
    for k in R.POINT:
        R.check_elementwise("t" + k, ptm[k], tref[k], print)
    jump, margin, target, inside = R.reset_ref(c, ptm)
    moved = S_reset != ptm["S"]
    close = np.abs(margin.v) <= margin.bound()
    assert (moved == jump)[~close].all()
    if moved.any():
        R.check_elementwise("Sreset", S_reset[moved], target[moved], print)
    m = R.merit_ref(c, dict(ptm, S=S_reset))[0]
    mo = dn(mer)
    R.check_scalar("phi", mo[0, 0], m["phi"]["value"], m["phi"]["tol"]); R.check_scalar("infeas", mo[0, 1], m["infeas"]["value"], m["infeas"]["tol"])
    new = {n: dn(du[n]) for n in du}
    aref = R.accept_ref(c, tr, st, sc[:, 0], sc[:, 1])
    for k, rr in aref.items():
        R.check_elementwise("a" + k, new[k], rr, print)
    for k in R.POINT:
        assert np.array_equal(dn(pt[k]), tr[k]), k
    c2 = dict(c, **new, **tr, RES=dn(RES2), G=dn(G2))
    e = R.error_ref(c2)[0]
    eo = dn(err)
    R.check_scalar("kkt_error", eo[0, 0], *e["kkt"]); R.check_scalar("viol", eo[0, 1], *e["viol"]); R.check_scalar("emax", eo[0, 2], *e["emax"])
    print(f"one iteration: apr {sc[0, 0]:.3f} adu {sc[0, 1]:.3f} dphi {sc[0, 2]:.3e} phi {mo[0, 0]:.6e} infeas {mo[0, 1]:.3e} kkt {eo[0, 0]:.3e}, "
          f"{int(moved.sum())} of {moved.size} slacks reset")
    ev.close()


def _column(ev, t, i):
    """column i of a [B][n] device tensor as a contiguous [B] tensor, ordered behind the context's stream"""
    import torch
    ev.synchronize()
    out = t[:, i].contiguous()
    torch.cuda.synchronize()
    return out
