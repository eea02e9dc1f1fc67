"""The relative local ODE error of a context WITH delays on the device (emi_ode_error_total_dev / _host, the residual kernel
emi_ode_resid_delay_kernel) against the long-double restatement of tests/ode_error_delay_ref.py, within the bound derived there; the
invariants the call promises (equal bits across calls, batch sizes and forms; a NaN stays in its instance; the context as before;
rebuilt after a change of the mesh or of the delays; the plain call's bits where there are no delays) and its statuses.  -m gpu

The demo model (2 states, 2 free controls, x(t - dt), x(t - 2 dt), u(t - dt)) is the traced model of tests/test_gpu_delay_adjoint.py, so
it takes the run-time compiled kernel; the quadrotor with its second control declared the delayed copy of the first takes the built-in
one."""
import ctypes as C

import numpy as np
import pytest

import ode_error_delay_ref as D
import ode_error_ref as R

pytestmark = pytest.mark.gpu
LD = np.longdouble
ARG, STATE, UNSUPPORTED = 1, 2, 5
DISC = np.array([[1.0, 2.0, 1.5, 0.25, 0, 0, 0, 0]])      # EMI_PATH_DISC: the passes of the context test need a record table


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _configure(ev, c, B=None):
    if c["name"] == "demo":
        import test_gpu_delay_adjoint as TD
        ev.set_model_source("TracedModel", TD.demo_source(), 2, 8)
    else:
        ev.set_model(c["model"], c["params"])
    ev.set_delays(c["xh"], c["uh"], c["dt"])
    assert ev.layout.nc == c["nc"] and ev.n_delayed == c["nc"] - c["ncf"]
    ev.set_batch(c["B"] if B is None else B)


def _evaluator(c, B=None):
    """a context on the case's mesh, model, delays and batch"""
    import etol_amd as E
    ev = E.Evaluator(0)
    ev.set_mesh(c["M"], c["t0"], c["tf"], mesh=(c["tau"], c["w"], c["D"]))
    _configure(ev, c, B)
    return ev


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()


def _ode(ev, *args, plain=False, **kw):
    """ev.ode_error_total between two device-wide synchronisations: the context has a stream of its own, torch another"""
    import torch
    torch.cuda.synchronize()
    out = (ev.ode_error if plain else ev.ode_error_total)(*args, **kw)
    torch.cuda.synchronize()
    return out


# ---- 1. within the bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_total_call_within_the_bound(built, case):
    name, B, M, dtf = case
    c, ref = D.case(*case), D.reference(*case)
    b = R.overshoot_instance(B)
    assert ref["clipped"][b] >= 1 and ref["clipped_delayed"][b] >= 1       # the clip is active on a free control and on a delayed copy
    ev = _evaluator(c)
    err, eta = _ode(ev, _dev(c["X"]), _dev(c["U"]), c["ul"], c["uu"])
    err, eta = err.cpu().numpy(), eta.cpu().numpy()
    assert np.isfinite(err).all() and np.isfinite(eta).all() and (eta >= 0).all()
    re, rr = R.ratios(eta, err, ref, M)
    print(f"{D.case_id(case)}: |eta - ref| {re:.3f}, |err - ref| {rr:.3f} of the bound; err {err.max():.3e}")
    assert re <= 1.0 and rr <= 1.0, (case, re, rr)
    # without bounds nothing is clipped, the delayed copies neither: the estimate of the overshooting instance is another one
    free = D.estimate(c, ref["tq"], clip=False)
    err0, eta0 = _ode(ev, _dev(c["X"]), _dev(c["U"]))
    re0, rr0 = R.ratios(eta0.cpu().numpy(), err0.cpu().numpy(), free, M)
    print(f"{D.case_id(case)}: no clip: |eta - ref| {re0:.3f}, |err - ref| {rr0:.3f} of the bound")
    assert re0 <= 1.0 and rr0 <= 1.0, (case, re0, rr0)
    ev.close()


# ---- 2. invariants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("demo", 5, 9, 0.2), ("demo", 17, 130, 0.2), ("demo", 3, 258, 0.2), ("quad", 3, 9, 0.15)], ids=D.case_id)
def test_invariants(built, case):
    import torch
    name, B, M, dtf = case
    c = D.case(*case)
    ev = _evaluator(c)
    X, U, ul, uu = _dev(c["X"]), _dev(c["U"]), c["ul"], c["uu"]
    err, eta = _ode(ev, X, U, ul, uu)
    err_only, none = _ode(ev, X, U, ul, uu, eta=False)                      # dEta = NULL
    assert none is None and _same(err, err_only)
    err2, eta2 = _ode(ev, X, U, ul, uu)
    assert _same(err, err2) and _same(eta, eta2)
    herr, heta = _ode(ev, c["X"], c["U"], ul, uu, dev=False)                # the host form
    assert _same(err, herr) and _same(eta, heta)
    herr_only, _ = _ode(ev, c["X"], c["U"], ul, uu, eta=False, dev=False)
    assert _same(err, herr_only)
    # a NaN in one instance's X, an infinity in another's U: those estimates are not finite, the others keep their bits
    bad = sorted({B // 2, B - 1})
    Xn, Un = c["X"].copy(), c["U"].copy()
    Xn[bad[0], c["ns"] - 1, M // 2] = np.nan
    if len(bad) > 1:
        Un[bad[1], 0, 0] = np.inf
    errn, etan = _ode(ev, _dev(Xn), _dev(Un), ul, uu)
    errn = errn.cpu().numpy()
    for b in range(B):
        if b in bad:
            assert not np.isfinite(errn[b]), (b, errn[b])
        else:
            assert _same(errn[b:b + 1], err[b:b + 1]) and _same(etan[b], eta[b]), b
    # instance b alone
    ev.set_batch(1)
    for b in sorted({0, B // 2, B - 1}):
        e1, t1 = _ode(ev, X[b:b + 1].contiguous(), U[b:b + 1].contiguous(), ul, uu)
        assert _same(e1, err[b:b + 1]) and _same(t1[0], eta[b]), b
    torch.cuda.synchronize()
    ev.close()


# ---- 3. the context is as before the call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("demo", 5, 9, 0.2), ("quad", 2, 130, 0.15)], ids=D.case_id)
def test_context_untouched(built, case):
    """an evaluation pass (EMI_EVAL_ALL) and the adjoint pass of the delayed context give the same bits before and after the call"""
    import torch
    import etol_amd as E
    c = D.case(*case)
    ev = _evaluator(c)
    ev.set_path(DISC, 0, 1)
    lay = ev.layout
    X, U = _dev(c["X"]), _dev(c["U"])
    rng = np.random.default_rng(4)
    lamF, lamC = _dev(rng.standard_normal((lay.B, lay.ns, lay.M))), _dev(rng.standard_normal((lay.B, lay.np, lay.M)))
    nf, nd = c["ns"] + c["ncf"], c["nc"] - c["ncf"]

    def passes():
        out = ev.alloc_outputs()
        for t in out:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        ev.eval_dev(X, U, *out, flags=E.EVAL_ALL)
        G = torch.full((lay.B, nf, lay.M), float("nan"), dtype=torch.float64, device="cuda")
        Gdel = torch.full((lay.B, nd, lay.M), float("nan"), dtype=torch.float64, device="cuda")
        ev.lagr_grad_total_dev(out[1], lamF, lamC, 0.7, G, Gdel)
        ev.synchronize()
        torch.cuda.synchronize()
        return out + (G, Gdel)

    before = passes()
    assert all(np.isfinite(t.cpu().numpy()).all() for t in before)
    err, _ = _ode(ev, X, U, c["ul"], c["uu"])
    after = passes()
    for a, b in zip(before, after):
        assert _same(a, b)
    fresh = E._lib.Layout()                                                     # mesh, batch, delays and tables as they were
    assert ev.lib.emi_get_layout(ev.ctx, C.byref(fresh)) == 0
    assert (fresh.M, fresh.B, fresh.np, fresh.ns, fresh.nc, fresh.t0, fresh.tf) == (lay.M, lay.B, lay.np, lay.ns, lay.nc, lay.t0, lay.tf)
    xh, uh, n = C.c_int(), C.c_int(), C.c_int()
    assert ev.lib.emi_get_delays(ev.ctx, C.byref(xh), C.byref(uh), C.byref(n)) == 0
    assert (xh.value, uh.value, n.value) == (c["xh"], c["uh"], nd)
    ref = D.reference(*case)                                                    # (the record table played no part)
    assert (np.abs(err.cpu().numpy().astype(LD) - ref["err"]) <= R.err_bound(ref, c["M"])).all()
    ev.close()


# ---- 4. a change of the mesh or of the delays rebuilds the operators ---------------------------------------------------------------
def test_mesh_and_delay_changes_rebuild_the_operators(built):
    def fresh_bits(c):
        f = _evaluator(c)
        out = _ode(f, _dev(c["X"]), _dev(c["U"]), c["ul"], c["uu"])
        f.close()
        return out

    first = D.case("demo", 5, 9, 0.2)
    ev = _evaluator(first)
    _ode(ev, _dev(first["X"]), _dev(first["U"]), first["ul"], first["uu"])
    for case in (("demo", 2, 41, 0.2), ("demo", 3, 3, 0.2), ("demo", 5, 9, 0.2)):       # larger mesh, smaller, back
        c = D.case(*case)
        ev.set_mesh(c["M"], c["t0"], c["tf"], mesh=(c["tau"], c["w"], c["D"]))
        ev.set_batch(c["B"])
        got, want = _ode(ev, _dev(c["X"]), _dev(c["U"]), c["ul"], c["uu"]), fresh_bits(c)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), case
    for dt in (0.37 * 6.0, 9.0, 0.2 * 6.0):                                          # another delay, one beyond the horizon, back
        c = dict(D.case("demo", 5, 9, 0.2), dt=dt)
        ev.set_delays(c["xh"], c["uh"], dt)
        got, want = _ode(ev, _dev(c["X"]), _dev(c["U"]), c["ul"], c["uu"]), fresh_bits(c)
        assert _same(got[0], want[0]) and _same(got[1], want[1]), dt
    ref = D.reference("demo", 5, 9, 0.2)
    re, rr = R.ratios(got[1].cpu().numpy(), got[0].cpu().numpy(), ref, 9)
    assert re <= 1.0 and rr <= 1.0
    ev.close()


# ---- 5. without delays: the plain call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,M", [("quadrotor", 5, 9), ("traced", 3, 257), ("fixedwing", 3, 3)])
def test_without_delays_the_total_calls_are_the_plain_calls(built, name, B, M):
    import test_gpu_ode_error as T
    c = R.case(name, B, M)
    ev = T._evaluator(c)
    assert ev.n_delayed == 0
    X, U = _dev(c["X"]), _dev(c["U"])
    for bounds in ((c["ul"], c["uu"]), (None, None)):
        plain = _ode(ev, X, U, *bounds, plain=True)
        total = _ode(ev, X, U, *bounds)
        assert _same(plain[0], total[0]) and _same(plain[1], total[1])
        hplain = _ode(ev, c["X"], c["U"], *bounds, dev=False, plain=True)
        htotal = _ode(ev, c["X"], c["U"], *bounds, dev=False)
        assert _same(hplain[0], htotal[0]) and _same(hplain[1], htotal[1]) and _same(plain[0], htotal[0])
    ev.close()


# ---- 6. statuses ------------------------------------------------------------------------------------------------------------------
def test_statuses(built):
    import torch
    import etol_amd as E
    c = D.case("quad", 3, 9, 0.15)
    X, U = _dev(c["X"]), _dev(c["U"])
    err = torch.zeros(3, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    dev = lambda ev: ev.lib.emi_ode_error_total_dev(ev.ctx, p(X), p(U), None, None, None, p(err))
    herr = np.zeros(3)
    host = lambda ev: ev.lib.emi_ode_error_total_host(ev.ctx, C.c_void_p(c["X"].ctypes.data), C.c_void_p(c["U"].ctypes.data), None, None, None,
                                                      C.c_void_p(herr.ctypes.data))
    # no mesh, model or batch
    ev = E.Evaluator(0)
    assert dev(ev) == STATE and host(ev) == STATE
    ev.set_mesh(9, c["t0"], c["tf"])
    assert dev(ev) == STATE
    ev.set_model(c["model"], c["params"])
    ev.set_delays(c["xh"], c["uh"], c["dt"])
    assert dev(ev) == STATE
    ev.set_batch(3)
    assert dev(ev) == 0 and host(ev) == 0
    # arguments
    ul = c["ul"].ctypes.data_as(E._lib._D)
    call = ev.lib.emi_ode_error_total_dev
    assert call(ev.ctx, None, p(U), None, None, None, p(err)) == ARG
    assert call(ev.ctx, p(X), None, None, None, None, p(err)) == ARG
    assert call(ev.ctx, p(X), p(U), None, None, None, None) == ARG
    assert call(ev.ctx, p(X), p(U), ul, None, None, p(err)) == ARG              # half a pair of bounds
    assert call(ev.ctx, p(X), p(U), None, ul, None, p(err)) == ARG
    assert call(None, p(X), p(U), None, None, None, p(err)) == ARG
    hcall = ev.lib.emi_ode_error_total_host
    hX, hU, hE = (C.c_void_p(a.ctypes.data) for a in (c["X"], c["U"], herr))
    assert hcall(ev.ctx, None, hU, None, None, None, hE) == ARG and hcall(ev.ctx, hX, None, None, None, None, hE) == ARG
    assert hcall(ev.ctx, hX, hU, None, None, None, None) == ARG and hcall(ev.ctx, hX, hU, ul, None, None, hE) == ARG
    assert hcall(None, hX, hU, None, None, None, hE) == ARG
    # the plain calls keep refusing the context, and say who takes it
    assert ev.lib.emi_ode_error_dev(ev.ctx, p(X), p(U), None, None, None, p(err)) == UNSUPPORTED
    msg = ev.lib.emi_last_error(ev.ctx).decode()
    assert "delays" in msg and "emi_ode_error_total" in msg
    assert ev.lib.emi_ode_error_host(ev.ctx, hX, hU, None, None, None, hE) == UNSUPPORTED
    # points-only mesh
    tau, w, _ = E.lgl(9)
    dp = lambda a: a.ctypes.data_as(E._lib._D)
    assert ev.lib.emi_set_mesh(ev.ctx, 9, dp(tau), dp(w), None, c["t0"], c["tf"]) == 0
    assert dev(ev) == STATE and host(ev) == STATE
    assert "points-only" in ev.lib.emi_last_error(ev.ctx).decode()
    ev.set_mesh(9, c["t0"], c["tf"])
    assert dev(ev) == 0
    # more than 65535 instances: refused before any array is read
    ev.set_batch(65536)
    assert dev(ev) == UNSUPPORTED and host(ev) == UNSUPPORTED
    assert "65535" in ev.lib.emi_last_error(ev.ctx).decode()
    ev.close()
    # fp32 context
    f32 = E.Evaluator(0, f32=True)
    f32.set_mesh(9, c["t0"], c["tf"])
    f32.set_model(c["model"], c["params"])
    f32.set_batch(3)
    assert dev(f32) == UNSUPPORTED and host(f32) == UNSUPPORTED
    f32.close()
