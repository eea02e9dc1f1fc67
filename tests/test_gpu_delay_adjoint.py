"""The adjoint pass of contexts WITH delays on the device (emi_lagr_grad_total_* / emi_kkt_certificate_total_*,
csrc/emi_adjoint.hip) against numpy.  -m gpu

Reference: tests/delay_adjoint_ref.py -- the gradient on the extended node variables by adjoint_ref.lagr_grad, then the adjoints of
the delayed values folded onto their sources with the interpolation matrices (checked against central differences of the
oracle's Lagrangian in tests/test_delay_adjoint_cpu.py).

Bounds (derived, not tuned).  An entry of G is a nested dot product: M products per delayed copy of its variable, each factor an
entry of Gdel that is itself a dot product of up to M + nv + np + 2 terms, and one more addition.  Whatever the summation order,
device and numpy together differ by at most
        2 (M (1 + copies) + nv + np + 4) eps T          elementwise, T = the same sums over absolute values.
End to end (VALS of the CPU oracle at delayed values formed with the ORACLE's interpolation matrices, folded with those matrices)
two allowances are added: 5e-13 T, the agreement of device and oracle VALS that tests/test_gpu_certificate.py uses, and
1e-12 max(1, |W|max) sum_j |Gdel|, the agreement of emi_delay_matrix with the oracle's matrices that tests/test_gpu_delays.py asserts:
for an entry of G summed over the copies of its variable (the fold with another W), for an entry of Gdel over its own slot (the node
functions were given delayed inputs from another W, which the adjoint of a delayed value sees through their second derivatives).
One directional derivative per shape against central differences of the oracle Lagrangian: 1e-7 relative (see the CPU test).
Certificate: maxima are order-free, so every figure but comp is bitwise numpy's on the device's G; comp: 4 eps relative."""
import ctypes as C
import os

import numpy as np
import pytest

import adjoint_ref as A
import delay_adjoint_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 1e20
P3 = [0.7, 0.3]
DISC = np.array([[1.0, 2.0, 1.5, 0.25, 0, 0, 0, 0]])      # EMI_PATH_DISC, centre (2, 1.5), radius 0.5
DP = C.POINTER(C.c_double)

_source = []


def demo_source():
    """text of the traced delayed model, as eMI355X::setup generates it (tests/harness/etol_harness.cpp, harness_delay_demo)"""
    if not _source:
        import torch  # noqa: F401
        h = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
        h.harness_last_message.restype = C.c_char_p
        z = np.zeros(4 * 9)
        res, vals = np.zeros(64 * 9), np.zeros(256 * 9)
        cost, nres, nvals = C.c_double(), C.c_int(), C.c_int()
        dp = lambda a: a.ctypes.data_as(DP)
        assert h.harness_delay_demo(8, C.c_double(0.5), 3, 1, 0, dp(z), dp(res), res.size, dp(vals), vals.size, C.byref(cost),
                                    C.byref(nres), C.byref(nvals)) == 0
        _source.append(h.harness_last_message().decode())
        assert "struct TracedModel" in _source[0]
    return _source[0]


# name -> kind, M, B
CASES = {"demo_33x3": ("demo", 33, 3), "demo_47x2": ("demo", 47, 2), "demo_128x20": ("demo", 128, 20), "demo_256x40": ("demo", 256, 40),
         "quad_64x1": ("quad", 64, 1), "quad_512x1024": ("quad", 512, 1024)}


def make_case(name, M=None, t0=0.0, tf=6.0):
    """the context of a case and everything the references need; M / t0 / tf override the mesh (mesh-change test)"""
    import etol_amd as E
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    kind, M0, B = CASES[name]
    M = M or M0
    c = dict(name=name, kind=kind, M=M, B=B, t0=t0, tf=tf, mesh=O.lgl(M))
    rng = np.random.default_rng(77 + 13 * M + B)
    if kind == "demo":
        c.update(model=3, params=P3, ns=2, ncf=2, xh=3, uh=1, dt=0.2, recs=DISC)
        t = t0 + (tf - t0) / 2 * (c["mesh"][0] + 1)
        X = np.stack([1 + 0.5 * np.sin(0.7 * t + rng.uniform(0, 3, (B, 1))), 2 - 0.1 * t + 0.3 * np.cos(t + rng.uniform(0, 3, (B, 1)))], axis=1)
        U = np.stack([0.3 * np.cos(t + rng.uniform(0, 3, (B, 1))), 0.2 + 0.1 * np.sin(2 * t + rng.uniform(0, 3, (B, 1)))], axis=1)
    else:
        # the built-in quadrotor with its second control slot declared the delayed copy of the first: one free control
        c.update(model=L.MODEL_QUADROTOR2D, params=W.QUAD_PARAMS, ns=6, ncf=1, xh=0, uh=1, dt=0.15, t0=0.0, tf=W.TF)
        X, U2, recs = W.quadrotor_batch(9, B, M, 2)
        U = U2[:, :1]
        c["recs"] = recs[:1]
    c["X"], c["U"] = np.ascontiguousarray(X), np.ascontiguousarray(U)
    c["nd"] = len(R.slots(c["ns"], c["ncf"], c["xh"], c["uh"]))
    c["nc"] = c["ncf"] + c["nd"]
    return c


def make_evaluator(c):
    import etol_amd as E
    ev = E.Evaluator(0)
    ev.set_mesh(c["M"], c["t0"], c["tf"], mesh=c["mesh"])          # the oracle's D on the device too: one operator on both sides
    configure(ev, c)
    return ev


def configure(ev, c):
    if c["kind"] == "demo":
        ev.set_model_source("TracedModel", demo_source(), 2, 8)
    else:
        ev.set_model(c["model"], c["params"])
    ev.set_delays(c["xh"], c["uh"], c["dt"])
    assert ev.n_delayed == c["nd"] and ev.layout.nc == c["nc"]
    ev.set_batch(c["B"])
    ev.set_path(c["recs"], 0, 1)


def emi_W(c):
    """W(i dt) of the case's mesh from the library's host routine"""
    from etol_amd import _lib as L
    lib = L.load()
    tau, w = (np.ascontiguousarray(a) for a in c["mesh"][:2])
    nd = max(c["xh"] - 1, c["uh"])
    W = np.empty((nd, c["M"], c["M"]))
    for d in range(nd):
        assert lib.emi_delay_matrix(c["M"], tau.ctypes.data_as(DP), w.ctypes.data_as(DP), c["t0"], c["tf"], (d + 1) * c["dt"],
                                    W[d].ctypes.data_as(DP)) == 0
    return W


def oracle_W(c):
    return R.oracle_delay_matrices(c["M"], c["mesh"][0], c["t0"], c["tf"], c["dt"], c["xh"], c["uh"])


def multipliers(c, lay, seed=0):
    rng = np.random.default_rng(4321 + c["M"] + 7 * c["B"] + seed)
    return rng.standard_normal((lay.B, lay.ns, lay.M)), rng.standard_normal((lay.B, lay.np, lay.M)), 0.7


def reference(c, ev, VALS, lamF, lamC, sigma, W):
    lay = ev.layout
    dims = (c["ns"], c["nc"], c["ncf"], c["xh"], c["uh"])
    pat = A.entry_pattern(*ev.jac_structure(), lay.ns, lay.nc, lay.np, lay.M)
    G, Gdel = R.lagr_grad_total(VALS, lamF, lamC, sigma, c["mesh"][2], pat, *dims, W)
    T, Tdel = R.lagr_grad_total(VALS, lamF, lamC, sigma, c["mesh"][2], pat, *dims, W, absolute=True)
    bG, bdel = R.bound(T, Tdel, lay.M, lay.ns + lay.nc, lay.np, R.copies(c["ns"], c["ncf"], c["xh"], c["uh"]))
    return G, Gdel, T, Tdel, bG, bdel


def worst(name, what, err, bnd):
    r = float((err / np.maximum(bnd, 1e-300)).max()) if err.size else 0.0
    print(f"{name}: {what}: max error {float(err.max()) if err.size else 0.0:.3e}, worst error / bound = {r:.3e}")
    return r


@pytest.mark.parametrize("name", list(CASES))
def test_total_gradient_against_the_numpy_fold(built, name):
    c = make_case(name)
    ev = make_evaluator(c)
    lay = ev.layout
    lamF, lamC, sigma = multipliers(c, lay)
    VALS = ev.eval_host(c["X"], c["U"])[1]
    # operator alone: the device's own VALS through numpy, W from emi_delay_matrix
    Gn, Gdn, T, Tdel, bG, bdel = reference(c, ev, VALS, lamF, lamC, sigma, emi_W(c))
    has = R.copies(c["ns"], c["ncf"], c["xh"], c["uh"]) > 0
    Gx = A.lagr_grad(VALS, lamF, lamC, sigma, c["mesh"][2], A.entry_pattern(*ev.jac_structure(), lay.ns, lay.nc, lay.np, lay.M), lay.ns, lay.nc)
    Gx = Gx[:, :lay.ns + c["ncf"]]
    tiles = (0, 1, 2) if name in ("quad_512x1024", "demo_128x20") else (0,)       # by size, then each tile shape forced
    for tile in tiles:
        ev.set_option("adj_fold_tile", tile)
        G, Gdel = ev.lagr_grad_total_host(VALS, lamF, lamC, sigma)
        r1 = worst(name, f"tile {tile}: G, operator alone", np.abs(G - Gn), bG)
        r2 = worst(name, f"tile {tile}: Gdel, operator alone", np.abs(Gdel - Gdn), bdel)
        assert np.all(np.abs(G - Gn) <= bG), r1
        assert np.all(np.abs(Gdel - Gdn) <= bdel), r2
        # the fold is there: the node-local gradient of a variable with delayed copies is not G
        assert np.abs(G[:, has] - Gx[:, has]).max() > 1e3 * bG[:, has].max()
        assert np.all(np.abs(G[:, ~has] - Gx[:, ~has]) <= bG[:, ~has])
    ev.set_option("adj_fold_tile", 0)
    G, Gdel = ev.lagr_grad_total_host(VALS, lamF, lamC, sigma)
    # end to end: oracle VALS at delayed values from the oracle's interpolation matrices, folded with those
    Wo = oracle_W(c)
    Uext = R.extended(c["X"], c["U"], Wo, c["ns"], c["ncf"], c["xh"], c["uh"])
    Vo = O.evaluate(c["model"], c["params"], c["M"], c["mesh"], c["t0"], c["tf"], c["X"], Uext, c["recs"])[1]
    assert Vo.shape == VALS.shape
    Go, Gdo, To, Tdo, bo, bdo = reference(c, ev, Vo, lamF, lamC, sigma, Wo)
    allow = bo + 5e-13 * To + 1e-12 * R.fold_weight(Gdo, Wo, c["ns"], c["ncf"], c["xh"], c["uh"])
    r1 = worst(name, "G, end to end", np.abs(G - Go), allow)
    allow_del = bdo + 5e-13 * Tdo + 1e-12 * R.slot_weight(Gdo, Wo, c["ns"], c["ncf"], c["xh"], c["uh"])
    r2 = worst(name, "Gdel, end to end", np.abs(Gdel - Gdo), allow_del)
    assert np.all(np.abs(G - Go) <= allow), r1
    assert np.all(np.abs(Gdel - Gdo) <= allow_del), r2
    # one directional derivative against central differences of the oracle Lagrangian (a few instances: L is a sum over them)
    idx = sorted({0, lay.B // 2, lay.B - 1})
    rng = np.random.default_rng(5 + c["M"])
    dX, dU = rng.standard_normal((len(idx), c["ns"], c["M"])), rng.standard_normal((len(idx), c["ncf"], c["M"]))
    fd, an = R.directional_check(c["model"], c["params"], c["mesh"], c["t0"], c["tf"], c["X"][idx], c["U"][idx], Wo, c["ns"], c["ncf"],
                                 c["xh"], c["uh"], lamF[idx], lamC[idx], sigma, G[idx], dX, dU, recs=c["recs"])
    print(f"{name}: directional derivative: central difference {fd:.12e}, device <G, d> {an:.12e}, relative {abs(fd - an) / abs(fd):.2e}")
    assert abs(fd - an) <= 1e-7 * abs(fd)
    ev.close()


def test_host_and_device_forms_and_two_calls_are_bit_identical(built):
    import torch
    c = make_case("demo_128x20")
    ev = make_evaluator(c)
    lay = ev.layout
    lamF, lamC, sigma = multipliers(c, lay)
    zl, zu, cl, cu = bounds_for(c, lay, True)
    a = ev.kkt_certificate_total_host(c["X"], c["U"], lamF, lamC, zl, zu, cl, cu, sigma)
    b = ev.kkt_certificate_total_host(c["X"], c["U"], lamF, lamC, zl, zu, cl, cu, sigma)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ev.device)
    X, U, lF, lC, dzl, dzu = (dev(x) for x in (c["X"], c["U"], lamF, lamC, zl, zu))
    RES, VALS, COST = ev.alloc_outputs()
    ev.eval_dev(X, U, RES, VALS, COST)
    kw = dict(dtype=torch.float64, device=ev.device)
    nf = lay.ns + c["ncf"]
    cert = torch.full((lay.B, 6), -1.0, **kw)
    G, Gdel = torch.full((lay.B, nf, lay.M), 7.0, **kw), torch.full((lay.B, c["nd"], lay.M), 7.0, **kw)
    ev.kkt_certificate_total_dev(X, U, RES, VALS, lF, lC, sigma, dzl, dzu, cl, cu, cert, G, Gdel)
    ev.synchronize()
    assert np.array_equal(cert.cpu().numpy(), a[0]) and np.array_equal(G.cpu().numpy(), a[1]) and np.array_equal(Gdel.cpu().numpy(), a[2])
    # G left in the workspace, Gdel not asked for; and the gradient call alone
    cert2 = torch.zeros_like(cert)
    ev.kkt_certificate_total_dev(X, U, RES, VALS, lF, lC, sigma, dzl, dzu, cl, cu, cert2, None, None)
    G2, Gdel2, G3 = torch.zeros_like(G), torch.zeros_like(Gdel), torch.zeros_like(G)
    ev.lagr_grad_total_dev(VALS, lF, lC, sigma, G2, Gdel2)
    ev.lagr_grad_total_dev(VALS, lF, lC, sigma, G3, None)
    ev.synchronize()
    assert torch.equal(cert2, cert) and torch.equal(G2, G) and torch.equal(Gdel2, Gdel) and torch.equal(G3, G)
    Gh, Gdh = ev.lagr_grad_total_host(VALS.cpu().numpy(), lamF, lamC, sigma)
    assert np.array_equal(Gh, a[1]) and np.array_equal(Gdh, a[2])
    ev.close()


def test_results_after_a_mesh_change_agree_with_a_fresh_context(built):
    """set_mesh on a context that has evaluated and certified on another mesh: the transposed stack of W is rebuilt.  The first
    call on each new mesh is the ADJOINT call (VALS from a fresh context): it must build W itself."""
    old = make_case("demo_33x3")
    ev = make_evaluator(old)
    lF, lC, sigma = multipliers(old, ev.layout)
    ev.lagr_grad_total_host(ev.eval_host(old["X"], old["U"])[1], lF, lC, sigma)
    for M, t0, tf in ((128, 0.0, 6.0), (128, 0.0, 9.0), (33, 1.0, 4.0), (47, 0.0, 6.0)):      # larger mesh, new horizon, smaller, odd
        c = make_case("demo_33x3", M=M, t0=t0, tf=tf)
        fresh = make_evaluator(c)
        lamF, lamC, sigma = multipliers(c, fresh.layout)
        VALS = fresh.eval_host(c["X"], c["U"])[1]
        want = fresh.lagr_grad_total_host(VALS, lamF, lamC, sigma)
        fresh.close()
        ev.set_mesh(M, t0, tf, mesh=c["mesh"])
        ev.set_path(c["recs"], 0, 1)
        got = ev.lagr_grad_total_host(VALS, lamF, lamC, sigma)              # before any evaluation on this mesh
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (M, t0, tf)
        ev.eval_host(c["X"], c["U"])                                        # ... and an evaluation after it finds W in place
        again = ev.lagr_grad_total_host(VALS, lamF, lamC, sigma)
        assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    ev.close()


def test_on_a_context_without_delays_the_total_calls_are_the_plain_calls(built):
    import test_gpu_certificate as TC
    for name in ("quad_129x16", "pm_sets_65x16_max"):
        c = TC.make_case(name)
        ev = TC.make_evaluator(c)
        lay = ev.layout
        assert ev.n_delayed == 0
        VALS = ev.eval_host(c["X"], c["U"])[1]
        zl, zu, cl, cu = TC.bounds_for(c, lay, True)
        lamF, lamC, sigma = TC.multipliers(c, lay, "normal")
        G, Gdel = ev.lagr_grad_total_host(VALS, lamF, lamC, sigma)
        assert Gdel.size == 0 and np.array_equal(G, ev.lagr_grad_host(VALS, lamF, lamC, sigma))
        cert, G2, _ = ev.kkt_certificate_total_host(c["X"], c["U"], lamF, lamC, zl, zu, cl, cu, sigma)
        cert0, G0 = ev.kkt_certificate_host(c["X"], c["U"], lamF, lamC, zl, zu, cl, cu, sigma)
        assert np.array_equal(cert, cert0) and np.array_equal(G2, G0) and np.array_equal(G2, G)
        ev.close()


def test_plain_calls_keep_refusing_contexts_with_delays_and_name_the_total_calls(built):
    from etol_amd import _lib as L
    c = make_case("quad_64x1")
    ev = make_evaluator(c)
    lay = ev.layout
    V = np.zeros((lay.B, lay.nvals, lay.M))
    G = np.zeros((lay.B, lay.ns + lay.nc, lay.M))
    lamF = np.ones((lay.B, lay.ns, lay.M))
    lamC = np.ones((lay.B, lay.np, lay.M))
    d = lambda a: a.ctypes.data_as(DP)
    st = ev.lib.emi_lagr_grad_host(ev.ctx, d(V), d(lamF), d(lamC), 1.0, d(G))
    msg = ev.lib.emi_last_error(ev.ctx).decode()
    assert L.STATUS[st] == "EMI_ERR_UNSUPPORTED" and "delay" in msg and "emi_lagr_grad_total" in msg
    ev.close()


def bounds_for(c, lay, per_instance, seed=5):
    """zl / zu [nsets][ns+ncf][M] on the FREE variables and cl / cu [np] that reach every branch (the scheme of
    tests/test_gpu_certificate.py: free, lower-only, upper-only, boxed, fixed, boxed and violated; one- and two-sided rows)"""
    rng = np.random.default_rng(seed)
    nf, M, B = lay.ns + c["ncf"], lay.M, lay.B
    z = np.concatenate([c["X"], c["U"]], axis=1)
    nsets = B if per_instance else 1
    zref = z[:nsets]
    spread = np.abs(z).max(axis=(0, 2), keepdims=True) + 1.0
    kind = rng.integers(0, 6, size=(nsets, nf, M))
    lo = zref - spread * rng.uniform(0.01, 1.0, size=zref.shape)
    up = zref + spread * rng.uniform(0.01, 1.0, size=zref.shape)
    zl = np.where(np.isin(kind, (1, 3)), lo, -INF)
    zu = np.where(np.isin(kind, (2, 3)), up, INF)
    zl = np.where(kind == 4, zref, zl); zu = np.where(kind == 4, zref, zu)
    zl = np.where(kind == 5, up, zl); zu = np.where(kind == 5, up + spread, zu)
    cl, cu = np.full(lay.np, -INF), np.zeros(lay.np)
    if lay.np > 1:
        cl[1::3] = -2.0
    return np.ascontiguousarray(zl), np.ascontiguousarray(zu), cl, cu


@pytest.mark.parametrize("name,per_instance", [("demo_33x3", True), ("demo_47x2", False), ("demo_128x20", True), ("demo_256x40", False),
                                               ("quad_64x1", True), ("quad_512x1024", False)])
def test_total_certificate_against_numpy(built, name, per_instance):
    c = make_case(name)
    ev = make_evaluator(c)
    lay = ev.layout
    RES, VALS, COST = ev.eval_host(c["X"], c["U"])
    zl, zu, cl, cu = bounds_for(c, lay, per_instance)
    for seed in (0, 1):
        lamF, lamC, sigma = multipliers(c, lay, seed)
        cert, G, Gdel = ev.kkt_certificate_total_host(c["X"], c["U"], lamF, lamC, zl, zu, cl, cu, sigma)
        Gg, Gd = ev.lagr_grad_total_host(VALS, lamF, lamC, sigma)
        assert np.array_equal(G, Gg) and np.array_equal(Gdel, Gd)                     # the certificate's G is the gradient call's
        ref = A.certificate(G, RES, c["X"], c["U"], VALS, lamF, lamC, sigma, zl, zu, cl, cu)
        ref[:, 4] = np.abs(sigma * VALS[:, -(lay.ns + lay.nc):]).reshape(lay.B, -1).max(axis=1)     # gmax: over the extended entries
        print(f"{name} seed {seed}: device {cert.max(axis=0)}  numpy {ref.max(axis=0)}")
        for q, f in enumerate(A.FIELDS):
            if f == "comp":
                assert np.all(np.abs(cert[:, q] - ref[:, q]) <= 4 * A.EPS * np.abs(ref[:, q])), (f, cert[:, q], ref[:, q])
            else:
                assert np.array_equal(cert[:, q], ref[:, q]), (f, cert[:, q], ref[:, q])
        assert np.all(cert[:, 3] > 0) and np.all(cert[:, 1] > 0)                      # the bounds above do reach those branches
    ev.close()
