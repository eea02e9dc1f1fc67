"""The relative local ODE error of a batch on the device (emi_interp_dev, emi_ode_error_dev / _host, Alg::ode_error = "device")
against the long-double restatement of tests/ode_error_ref.py, within the bound derived there; the invariants the call promises
(equal bits across calls, batch sizes and forms; a NaN stays in its instance; the context as before).  -m gpu"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ode_error_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LD = np.longdouble
ARG, STATE, UNSUPPORTED = 1, 2, 5


def _bits(t):
    a = t.detach().cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _evaluator(c, B=None):
    """a context on the case's mesh, model and batch"""
    import etol_amd as E
    ev = E.Evaluator(0)
    ev.set_mesh(c["M"], c["t0"], c["tf"], mesh=(c["tau"], c["w"], c["D"]))
    sp = R.SPEC[c["name"]]
    if sp["model"] is None:
        from test_gpu_traced import traced_source
        ev.set_model_source("TracedModel", traced_source(1), c["ns"], c["nc"])
    else:
        ev.set_model(sp["model"], sp["params"])
    ev.set_batch(c["B"] if B is None else B)
    return ev


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()


def _ode(ev, *args, **kw):
    """ev.ode_error between two device-wide synchronisations: the context has a stream of its own, torch another"""
    import torch
    torch.cuda.synchronize()
    out = ev.ode_error(*args, **kw)
    torch.cuda.synchronize()
    return out


def _interp(ev, *args, **kw):
    import torch
    torch.cuda.synchronize()
    out = ev.interp(*args, **kw)
    torch.cuda.synchronize()
    return out


# ---- 1. the product alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", R.PRODUCT_SHAPES)
def test_product_alone(built, K, N):
    import torch
    import etol_amd as E
    ev = E.Evaluator(0)                                     # no mesh, model or batch
    rng = np.random.default_rng(100 * K + N)
    ldk, ldo, Rmax = K + (K & 1), N + 3, max(R.PRODUCT_ROWS)
    OP = np.zeros((N, ldk))
    OP[:, :K] = rng.standard_normal((N, K)) * np.exp(rng.uniform(-3, 3, (N, K)))
    V = rng.standard_normal((Rmax, K)) * np.exp(rng.uniform(-3, 3, (Rmax, K)))
    ref = V.astype(LD) @ OP[:, :K].astype(LD).T
    bound = (K + 1) * R.U53 * (np.abs(V) @ np.abs(OP[:, :K]).T)
    dOP = _dev(OP)
    worst = 0.0
    for rows in R.PRODUCT_ROWS:
        dV = _dev(V[:rows])
        out = torch.full((rows, ldo), float("nan"), dtype=torch.float64, device="cuda")
        _interp(ev, dOP, dV, K=K, out=out)
        got = out.cpu().numpy()
        assert np.isnan(got[:, N:]).all() and np.isfinite(got[:, :N]).all()         # the padding columns stay as they were
        ratio = (np.abs(got[:, :N].astype(LD) - ref[:rows]).astype(np.float64) / bound[:rows]).max()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (K, N, rows, ratio)
        again = torch.full((rows, ldo), float("nan"), dtype=torch.float64, device="cuda")
        _interp(ev, dOP, dV, K=K, out=again)
        assert _same(out[:, :N], again[:, :N])
        for r in sorted({0, rows // 2, rows - 1}):          # a row's bits depend on the row and OP alone
            alone = _interp(ev, dOP, _dev(V[r:r + 1]), K=K)
            assert _same(alone[0], out[r, :N]), (K, N, rows, r)
    print(f"K {K} N {N}: largest |out - ref| / ((K + 1) 2^-53 sum |OP| |v|) = {worst:.3f}")
    Vz = V[:7].copy()
    Vz[3] = 0.0
    z = _interp(ev, dOP, _dev(Vz), K=K).cpu().numpy()
    assert (z[3] == 0.0).all() and (z[2] != 0.0).any()
    ev.close()


def test_product_statuses(built):
    import torch
    import etol_amd as E
    ev = E.Evaluator(0)
    OP, V, out = (torch.zeros(s, dtype=torch.float64, device="cuda") for s in ((5, 4), (3, 4), (3, 5)))
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda K, N, ldk, op, v, rows, ldo, o: ev.lib.emi_interp_dev(ev.ctx, K, N, ldk, op, v, rows, ldo, o)
    assert call(4, 5, 4, p(OP), p(V), 3, 5, p(out)) == 0
    assert call(4, 5, 4, p(OP), None, 0, 5, None) == 0                         # no rows: nothing to do
    assert call(1, 5, 2, p(OP), p(V), 3, 5, p(out)) == ARG                      # K < 2
    assert call(4, 0, 4, p(OP), p(V), 3, 5, p(out)) == ARG                      # N < 1
    assert call(4, 5, 4, p(OP), p(V), -1, 5, p(out)) == ARG                     # R < 0
    assert call(3, 5, 3, p(OP), p(V), 3, 5, p(out)) == ARG                      # odd row length of OP
    assert call(4, 5, 2, p(OP), p(V), 3, 5, p(out)) == ARG                      # rows of OP shorter than K
    assert call(4, 5, 4, p(OP), p(V), 3, 4, p(out)) == ARG                      # rows of the output shorter than N
    assert call(4, 5, 4, None, p(V), 3, 5, p(out)) == ARG
    assert call(4, 5, 4, p(OP), None, 3, 5, p(out)) == ARG
    assert call(4, 5, 4, p(OP), p(V), 3, 5, None) == ARG
    assert ev.lib.emi_interp_dev(None, 4, 5, 4, p(OP), p(V), 3, 5, p(out)) == ARG
    ev.close()
    f32 = E.Evaluator(0, f32=True)
    assert f32.lib.emi_interp_dev(f32.ctx, 4, 5, 4, p(OP), p(V), 3, 5, p(out)) == UNSUPPORTED
    f32.close()


# ---- 2. the full call --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,M", R.SHAPES)
@pytest.mark.parametrize("name", R.MODELS)
def test_full_call_within_the_bound(built, name, B, M):
    c, ref = R.case(name, B, M), R.reference(name, B, M)
    assert ref["clipped"][R.overshoot_instance(B)] >= 1          # the clip is active at at least one point of that instance
    ev = _evaluator(c)
    err, eta = _ode(ev, _dev(c["X"]), _dev(c["U"]), c["ul"], c["uu"])
    err, eta = err.cpu().numpy(), eta.cpu().numpy()
    assert np.isfinite(err).all() and np.isfinite(eta).all() and (eta >= 0).all()
    re, rr = R.ratios(eta, err, ref, M)
    print(f"{name} B {B} M {M}: |eta - ref| {re:.3f}, |err - ref| {rr:.3f} of the bound; err {err.max():.3e}")
    assert re <= 1.0 and rr <= 1.0, (name, B, M, re, rr)
    # without bounds the interpolated controls are not clipped: the estimate of the overshooting instance is another one
    free = R.estimate(c, ref["tq"], clip=False)
    err0, eta0 = _ode(ev, _dev(c["X"]), _dev(c["U"]))
    re0, rr0 = R.ratios(eta0.cpu().numpy(), err0.cpu().numpy(), free, M)
    assert re0 <= 1.0 and rr0 <= 1.0, (name, B, M, re0, rr0)
    ev.close()


@pytest.mark.parametrize("B,M", R.SHAPES)
def test_point_mass_polynomial_has_no_error(built, B, M):
    """x a polynomial in time of degree <= M - 1, u its derivative: the interpolants are the functions themselves, eta = 0 in exact
    arithmetic, so what the device returns is within the bound of 0 (and of the reference)"""
    c, ref = R.case("pointmass", B, M, True), R.reference("pointmass", B, M, True)
    ev = _evaluator(c)
    err, eta = _ode(ev, _dev(c["X"]), _dev(c["U"]), c["ul"], c["uu"])
    eta = eta.cpu().numpy()
    assert ref["clipped"].sum() == 0
    ratio0 = (np.abs(eta) / R.eta_bound(ref, M)).max()
    re, rr = R.ratios(eta, err.cpu().numpy(), ref, M)
    print(f"point mass, polynomial data, B {B} M {M}: |eta| {ratio0:.3f}, |eta - ref| {re:.3f}, |err - ref| {rr:.3f} of the bound")
    assert ratio0 <= 1.0 and re <= 1.0 and rr <= 1.0
    ev.close()


# ---- 3. invariants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,M", [("quadrotor", 5, 9), ("quadrotor", 17, 130), ("traced", 3, 257), ("fixedwing", 3, 3)])
def test_invariants(built, name, B, M):
    import torch
    c = R.case(name, B, M)
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


# ---- 4. the context is as before the call ------------------------------------------------------------------------------------------
def test_context_untouched(built):
    import torch
    import etol_amd as E
    c = R.case("quadrotor", 5, 9)
    ev = _evaluator(c)
    recs = np.zeros((2, E.PATH_REC))
    recs[:, 0], recs[:, 1], recs[:, 2], recs[:, 3] = E.PATH_DISC, (3.0, 6.0), (4.0, 2.0), (0.5, 0.8)
    ev.set_path(recs, 0, 1)
    lay = ev.layout
    X, U = _dev(c["X"]), _dev(c["U"])
    rng = np.random.default_rng(4)
    lamF, lamC = _dev(rng.standard_normal((lay.B, lay.ns, lay.M))), _dev(rng.standard_normal((lay.B, lay.np, lay.M)))

    def passes():
        out = ev.alloc_outputs()
        for t in out:
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        ev.eval_dev(X, U, *out, flags=E.EVAL_ALL)
        G = torch.full((lay.B, lay.ns + lay.nc, lay.M), float("nan"), dtype=torch.float64, device="cuda")
        ev.lagr_grad_dev(out[1], lamF, lamC, 0.7, G)
        torch.cuda.synchronize()
        return out + (G,)

    before = passes()
    err, _ = _ode(ev, X, U, c["ul"], c["uu"])
    after = passes()
    for a, b in zip(before, after):
        assert _same(a, b)
    lay2 = ev.lib.emi_get_layout                                                # mesh, batch and tables as they were
    fresh = E._lib.Layout()
    assert lay2(ev.ctx, C.byref(fresh)) == 0
    assert (fresh.M, fresh.B, fresh.np, fresh.ns, fresh.nc, fresh.t0, fresh.tf) == (lay.M, lay.B, lay.np, lay.ns, lay.nc, lay.t0, lay.tf)
    ref = R.reference("quadrotor", 5, 9)                                        # (the record table played no part)
    assert (np.abs(err.cpu().numpy().astype(LD) - ref["err"]) <= R.err_bound(ref, 9)).all()
    ev.close()


# ---- 5. mesh change ----------------------------------------------------------------------------------------------------------------
def test_mesh_change_rebuilds_the_operator(built):
    ev = None
    for B, M in ((5, 9), (2, 41), (5, 9)):
        c, ref = R.case("quadrotor", B, M), R.reference("quadrotor", B, M)
        if ev is None:
            ev = _evaluator(c)
        else:
            ev.set_mesh(M, c["t0"], c["tf"], mesh=(c["tau"], c["w"], c["D"]))
            ev.set_batch(B)
        err, eta = _ode(ev, _dev(c["X"]), _dev(c["U"]), c["ul"], c["uu"])
        re, rr = R.ratios(eta.cpu().numpy(), err.cpu().numpy(), ref, M)
        assert re <= 1.0 and rr <= 1.0, (B, M, re, rr)
    ev.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    import torch
    import etol_amd as E
    c = R.case("quadrotor", 5, 9)
    X, U = _dev(c["X"]), _dev(c["U"])
    err = torch.zeros(5, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())
    dev = lambda ev: ev.lib.emi_ode_error_dev(ev.ctx, p(X), p(U), None, None, None, p(err))
    herr = np.zeros(5)
    host = lambda ev: ev.lib.emi_ode_error_host(ev.ctx, C.c_void_p(c["X"].ctypes.data), C.c_void_p(c["U"].ctypes.data), None, None, None,
                                                C.c_void_p(herr.ctypes.data))
    sp = R.SPEC["quadrotor"]
    # no mesh, model or batch
    ev = E.Evaluator(0)
    assert dev(ev) == STATE and host(ev) == STATE
    ev.set_mesh(9, c["t0"], c["tf"])
    assert dev(ev) == STATE
    ev.set_model(sp["model"], sp["params"])
    assert dev(ev) == STATE
    ev.set_batch(5)
    assert dev(ev) == 0 and host(ev) == 0
    # arguments
    ul = c["ul"].ctypes.data_as(E._lib._D)
    assert ev.lib.emi_ode_error_dev(ev.ctx, None, p(U), None, None, None, p(err)) == ARG
    assert ev.lib.emi_ode_error_dev(ev.ctx, p(X), None, None, None, None, p(err)) == ARG
    assert ev.lib.emi_ode_error_dev(ev.ctx, p(X), p(U), None, None, None, None) == ARG
    assert ev.lib.emi_ode_error_dev(ev.ctx, p(X), p(U), ul, None, None, p(err)) == ARG          # half a pair of bounds
    assert ev.lib.emi_ode_error_dev(None, p(X), p(U), None, None, None, p(err)) == ARG
    # points-only mesh
    tau, w, _ = E.lgl(9)
    dp = lambda a: a.ctypes.data_as(E._lib._D)
    assert ev.lib.emi_set_mesh(ev.ctx, 9, dp(tau), dp(w), None, c["t0"], c["tf"]) == 0
    assert dev(ev) == STATE and host(ev) == STATE
    assert "points-only" in ev.lib.emi_last_error(ev.ctx).decode()
    ev.set_mesh(9, c["t0"], c["tf"])
    assert dev(ev) == 0
    # delays
    ev.set_delays(0, 1, 0.1)                    # (2 controls = 1 free + its delayed copy)
    assert dev(ev) == UNSUPPORTED and host(ev) == UNSUPPORTED
    assert "delays" in ev.lib.emi_last_error(ev.ctx).decode()
    ev.close()
    # fp32 context
    f32 = E.Evaluator(0, f32=True)
    f32.set_mesh(9, c["t0"], c["tf"])
    f32.set_model(sp["model"], sp["params"])
    f32.set_batch(5)
    assert dev(f32) == UNSUPPORTED and host(f32) == UNSUPPORTED
    f32.close()


# ---- 7. the ETOL class -------------------------------------------------------------------------------------------------------------
def test_etol_class_device_route(built):
    """Alg::ode_error = "device" against the host route on the trajectories of test_gpu_solve.py's estimate test: the rough one within
    that test's own tolerance (the estimate is > 1e-3 there), the stored optimum within the bound on err"""
    import torch  # noqa: F401
    H = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    D_ = C.POINTER(C.c_double)
    for f in (H.harness_ode_error_quadrotor, H.harness_ode_error_quadrotor_dev):
        f.argtypes = [C.c_int, C.c_double, C.c_int, D_, D_, D_]
    prob = json.load(open(os.path.join(GOLD, "solve_optima.json")))["problems"]["quadrotor_41"]
    M, tf = prob["M"], prob["tf"]
    tau, w, D = O.lgl(M)
    rng = np.random.default_rng(3)
    for label in ("optimum", "perturbed"):
        X, U = np.array(prob["optima"][0]["X"]), np.array(prob["optima"][0]["U"])
        if label == "perturbed":
            X = X + 0.05 * rng.standard_normal(X.shape) * np.sin(np.pi * (tau + 1) / 2)
            U = np.clip(U + 0.3 * rng.standard_normal(U.shape), [[0.0], [-1.0]], [[25.0], [1.0]])
        X, U = np.ascontiguousarray(X), np.ascontiguousarray(U)
        host, dev = C.c_double(), C.c_double()
        assert H.harness_ode_error_quadrotor(M - 1, tf / (M - 1), 2, X.ctypes.data_as(D_), U.ctypes.data_as(D_), C.byref(host)) == 0
        assert H.harness_ode_error_quadrotor_dev(M - 1, tf / (M - 1), 2, X.ctypes.data_as(D_), U.ctypes.data_as(D_), C.byref(dev)) == 0
        c = dict(name="quadrotor", B=1, M=M, t0=0.0, tf=tf, tau=tau, w=w, D=D, ns=6, nc=2, ul=np.array([0.0, -1.0]), uu=np.array([25.0, 1.0]),
                 X=X[None], U=U[None])
        ref = R.estimate(c, R.library_points(M, (tau, w)))
        bound = R.err_bound(ref, M)[0]
        print(f"ODE error estimate, {label}: host route {host.value:.6e}, device route {dev.value:.6e}, long double {float(ref['err'][0]):.6e}, "
              f"bound on err {bound:.3e}")
        if label == "perturbed":
            assert abs(dev.value - host.value) < 1e-7 * host.value + 1e-13
            assert dev.value > 1e-3
        else:
            assert abs(dev.value - host.value) <= bound
        assert abs(LD(dev.value) - ref["err"][0]) <= bound
