"""The adjoint pass on the device (emi_lagr_grad_* / emi_kkt_certificate_*, csrc/emi_adjoint.hip) against numpy.  -m gpu

Reference: tests/adjoint_ref.py -- G in numpy float64 from the formula of include/emi355x.h, with D from the oracle's own LGL
construction and the COO pattern the library publishes (emi_jac_structure), so traced rows are indexed by that pattern.

Bounds (derived, not tuned).  G is a dot product of M + nv + np + 1 terms per entry; whatever the summation order (the matrix
pipe's included) the forward error of device and numpy together is at most
        2 (M + nv + np + 2) eps T,     T = |sigma costgrad| + sum |VALS| |lam| + |Doff|^T |lamF|     elementwise.
End to end (VALS from the CPU oracle instead of the device's own) 5e-13 T is added: the relative agreement of device and oracle
VALS the parity tests assert.  Certificate: maxima are order-free, so stat / defect / viol / gmax / lmax are bitwise numpy's on
the device's G; comp is one subtraction and one product: 4 eps relative."""
import ctypes as C
import os

import numpy as np
import pytest

import adjoint_ref as A
import cases
import oracle_lib as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = 1e20


def _traced_source(which):
    import torch  # noqa: F401
    lib = C.CDLL(os.path.join(HERE, "harness", "libetol_harness.so"))
    lib.harness_traced_model_source.restype = C.c_char_p
    return lib.harness_traced_model_source(which).decode()


def _pm_recs(E, L, node_t, B, seed):
    """per-instance record sets for the point mass: two ellipses, one disc, two track rows (centres per instance)"""
    rng = np.random.default_rng(seed)
    recs, tx, ty = [], [], []
    for b in range(B):
        a = rng.uniform(1.0, 6.0, 8)
        rows = [E.edge_ellipse(a[0], a[1], a[0] + 0.7, a[1] + 0.4), E.edge_ellipse(a[2], a[3], a[2] - 0.5, a[3] + 0.9)]
        d = np.zeros(L.PATH_REC); d[:4] = [L.PATH_DISC, a[4], a[5], 0.3]
        rows.append(d)
        cx, cy = [], []
        for t in range(2):
            xc, yc = E.track_centres([0.0, 16.0], [a[6], a[7]], [a[7 - t], a[6]], node_t)
            cx.append(xc); cy.append(yc)
            r = np.zeros(L.PATH_REC); r[0], r[1], r[2] = L.PATH_TRACK, t, 0.25
            rows.append(r)
        recs.append(rows); tx.append(cx); ty.append(cy)
    return np.array(recs), np.array(tx), np.array(ty)


def make_case(name):
    """-> dict(ev, model, params, M, B, t0, tf, X, U, recs, tracks, maximize, oracle: bool)"""
    import etol_amd as E
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    c = dict(recs=None, tracks=None, maximize=False, oracle=True, source=None, t0=0.0, tf=W.TF)
    quad = dict(model=L.MODEL_QUADROTOR2D, params=W.QUAD_PARAMS)
    if name == "pm_shipped_33x3":
        c.update(model=L.MODEL_POINTMASS2D, params=[], M=33, B=3, ocp2d=True)
        c["X"], c["U"] = W.pointmass_batch(0, 3, 33)
    elif name == "pm_shipped_33x1024":                 # (a batch that takes the register-accumulating node kernel, 2 + 2 variables)
        c.update(model=L.MODEL_POINTMASS2D, params=[], M=33, B=1024, ocp2d=True)
        c["X"], c["U"] = W.pointmass_batch(2, 1024, 33)
    elif name == "pm_sets_65x16_max":
        c.update(model=L.MODEL_POINTMASS2D, params=[], M=65, B=16, maximize=True, pm_sets=True)
        c["X"], c["U"] = W.pointmass_batch(1, 16, 65)
    elif name == "quad_c3_1024x1024":
        c.update(quad, M=1024, B=1024)
        c["X"], c["U"], c["recs"] = W.quadrotor_batch(2, 1024, 1024, 20)
    elif name == "quad_1000x130":
        c.update(quad, M=1000, B=130, t0=0.5, tf=9.0)
        c["X"], c["U"], r = W.quadrotor_batch(7, 130, 1000, 3)
        c["recs"] = r[:1]
    elif name == "quad_256x3_max":
        c.update(quad, M=256, B=3, maximize=True)
        c["X"], c["U"], c["recs"] = W.quadrotor_batch(1, 3, 256, 2)
    elif name == "quad_5x1":
        c.update(quad, M=5, B=1, tf=1.0)
        c["X"], c["U"], _ = W.quadrotor_batch(8, 1, 5, 0)
    elif name == "quad_129x16":
        c.update(quad, M=129, B=16)
        c["X"], c["U"], c["recs"] = W.quadrotor_batch(3, 16, 129, 4)
    elif name == "quad_1024x1":
        c.update(quad, M=1024, B=1)
        c["X"], c["U"], c["recs"] = W.quadrotor_batch(4, 1, 1024, 20)
    elif name == "fixedwing_129x3_max":
        c.update(model=L.MODEL_FIXEDWING12, params=W.FW_PARAMS, M=129, B=3, tf=20.0, maximize=True)
        c["X"], c["U"] = W.fixedwing_batch(4, 3, 129)
    elif name == "fixedwing_33x130":
        c.update(model=L.MODEL_FIXEDWING12, params=W.FW_PARAMS, M=33, B=130, tf=20.0)
        c["X"], c["U"] = W.fixedwing_batch(5, 130, 33)
    elif name == "fixedwing_33x1024":                  # (... 12 + 4 variables)
        c.update(model=L.MODEL_FIXEDWING12, params=W.FW_PARAMS, M=33, B=1024, tf=20.0)
        c["X"], c["U"] = W.fixedwing_batch(6, 1024, 33)
    elif name == "traced_rows_256x3":
        # a disc and an ellipse traced from callbacks behind one table row: the oracle has the same rows in its table
        disc = np.zeros(L.PATH_REC); disc[:4] = [L.PATH_DISC, 4.0, 3.2, 0.64]
        extra = np.zeros(L.PATH_REC); extra[:4] = [L.PATH_DISC, 6.3, 4.4, 0.49]
        c.update(quad, M=256, B=3, source=(_traced_source(2), 2, (0, 1)), recs=np.array([extra]),
                 oracle_recs=np.array([extra, disc, E.edge_ellipse(3.2, 2.5, 3.4, 2.6)]))
        c["X"], c["U"], _ = W.quadrotor_batch(5, 3, 256, 0)
    elif name == "traced_rows_wide_65x16":
        # four traced rows on six node variables (0 1 2 3 4 6): no oracle for them, operator alone
        extra = np.zeros(L.PATH_REC); extra[:4] = [L.PATH_DISC, 6.3, 4.4, 0.49]
        c.update(quad, M=65, B=16, tf=8.0, source=(_traced_source(3), 4, (0, 1, 2, 3, 4, 6)), recs=np.array([extra]), oracle=False)
        c["X"], c["U"], _ = W.quadrotor_batch(5, 16, 65, 0)
    elif name == "traced_rows_wide_65x1024":           # (... with traced rows on six variables)
        extra = np.zeros(L.PATH_REC); extra[:4] = [L.PATH_DISC, 6.3, 4.4, 0.49]
        c.update(quad, M=65, B=1024, tf=8.0, source=(_traced_source(3), 4, (0, 1, 2, 3, 4, 6)), recs=np.array([extra]), oracle=False)
        c["X"], c["U"], _ = W.quadrotor_batch(6, 1024, 65, 0)
    else:
        raise KeyError(name)
    return c


def make_evaluator(c, B=None, first=0):
    """Evaluator of the case, or of `B` instances of it from `first`"""
    import etol_amd as E
    from etol_amd import _lib as L
    B = c["B"] if B is None else B
    ev = E.Evaluator(0)
    ev.set_mesh(c["M"], c["t0"], c["tf"], mesh=O.lgl(c["M"]))      # the oracle's D on the device too: one operator on both sides
    if c["source"]:
        src, npath, pv = c["source"]
        ns, nc = O.MODEL_DIMS[c["model"]]
        ev.set_model_source("TracedModel", src, ns, nc, params=(), maximize=c["maximize"], npath=npath, path_vars=pv)
    else:
        ev.set_model(c["model"], c["params"], maximize=c["maximize"])
    ev.set_batch(B)
    recs, tracks = c["recs"], c["tracks"]
    if c.get("ocp2d"):
        recs, tx, ty = cases.ocp2d_tables(E.edge_ellipse, E.track_centres, ev.node_t)
        tracks = (tx, ty)
    if c.get("pm_sets"):
        recs, tx, ty = _pm_recs(E, L, ev.node_t, c["B"], 11)
        tracks = (tx, ty)
    sl = slice(first, first + B)
    pick = lambda a: a[sl] if a is not None and a.ndim == 3 and a.shape[0] == c["B"] and c["B"] > 1 else a
    if tracks is not None:
        ev.set_tracks(pick(tracks[0]), pick(tracks[1]))
    if recs is not None:
        ev.set_path(pick(recs), 0, 1)
    c["_recs"], c["_tracks"] = recs, tracks
    return ev


def multipliers(c, lay, kind):
    rng = np.random.default_rng(1234 + c["M"] + 7 * c["B"])
    B, M = lay.B, lay.M
    if kind == "normal":
        return rng.standard_normal((B, lay.ns, M)), rng.standard_normal((B, lay.np, M)), 0.7
    # exact zeros and a single nonzero entry in each array: an indexing slip shows
    lamF, lamC = np.zeros((B, lay.ns, M)), np.zeros((B, lay.np, M))
    lamF[B // 2, lay.ns - 1, (2 * M) // 3] = -1.75
    if lay.np:
        lamC[B - 1, lay.np - 1, M // 3] = 2.5
    return lamF, lamC, 0.0 if kind == "single0" else 1.0


def reference(c, ev, VALS, lamF, lamC, sigma):
    lay = ev.layout
    D = O.lgl(lay.M)[2]
    pat = A.entry_pattern(*ev.jac_structure(), lay.ns, lay.nc, lay.np, lay.M)
    G = A.lagr_grad(VALS, lamF, lamC, sigma, D, pat, lay.ns, lay.nc)
    T = A.lagr_grad(VALS, lamF, lamC, sigma, D, pat, lay.ns, lay.nc, absolute=True)
    return G, T, A.bound(T, lay.M, lay.ns + lay.nc, lay.np)


def oracle_vals(c, ev):
    recs, tracks = c.get("oracle_recs", c["_recs"]), c["_tracks"]
    if c.get("ocp2d"):
        recs, otx, oty = cases.ocp2d_tables(O.edge_ellipse, O.track_centres, ev.node_t)
        tracks = (otx, oty)
    return O.evaluate(c["model"], c["params"], c["M"], O.lgl(c["M"]), c["t0"], c["tf"], c["X"], c["U"], recs, tracks,
                      maximize=c["maximize"])


def worst(name, what, err, bnd):
    r = float((err / np.maximum(bnd, 1e-300)).max())
    print(f"{name}: {what}: max |G_dev - G_np| = {float(err.max()):.3e}, worst error / bound = {r:.3e}")
    return r


CASES = ["pm_shipped_33x3", "pm_sets_65x16_max", "quad_1000x130", "quad_256x3_max", "quad_5x1", "quad_129x16", "quad_1024x1",
         "fixedwing_129x3_max", "fixedwing_33x130", "traced_rows_256x3", "traced_rows_wide_65x16", "pm_shipped_33x1024", "fixedwing_33x1024",
         "traced_rows_wide_65x1024", "quad_c3_1024x1024"]


@pytest.mark.parametrize("name", CASES)
def test_lagrangian_gradient_against_numpy(built, name):
    c = make_case(name)
    ev = make_evaluator(c)
    lay = ev.layout
    RES, VALS, COST = ev.eval_host(c["X"], c["U"])
    oracle = oracle_vals(c, ev)[1] if c["oracle"] else None
    if oracle is not None:
        assert oracle.shape == VALS.shape
    for kind in ("normal", "single1") + (("single0",) if lay.B * lay.M < 200000 else ()):
        lamF, lamC, sigma = multipliers(c, lay, kind)
        G = ev.lagr_grad_host(VALS, lamF, lamC, sigma)
        # operator alone: the device's own VALS through numpy
        Gn, T, bnd = reference(c, ev, VALS, lamF, lamC, sigma)
        r = worst(name, f"{kind}, operator alone", np.abs(G - Gn), bnd)
        assert np.all(np.abs(G - Gn) <= bnd), r
        if kind == "single0":                      # sigma = 0: G is nonzero exactly where the two entries reach
            assert np.array_equal(G == 0, Gn == 0) and 0 < np.count_nonzero(G) <= lay.M + 2 * (lay.ns + lay.nc)
        # end to end: VALS of the CPU oracle
        if oracle is not None:
            Go, To, bo = reference(c, ev, oracle, lamF, lamC, sigma)
            r = worst(name, f"{kind}, end to end", np.abs(G - Go), bo + 5e-13 * To)
            assert np.all(np.abs(G - Go) <= bo + 5e-13 * To), r
    ev.close()


def bounds_for(c, lay, per_instance, seed=5):
    """zl / zu [nsets][nv][M] and cl / cu [np] that reach every branch: free, lower-only, upper-only, boxed and fixed variables,
    bounds the point violates, rows with one and with two bounds"""
    rng = np.random.default_rng(seed)
    nv, M, B = lay.ns + lay.nc, lay.M, lay.B
    z = np.concatenate([c["X"], c["U"]], axis=1)
    nsets = B if per_instance else 1
    zref = z[:nsets]
    spread = np.abs(z).max(axis=(0, 2), keepdims=True) + 1.0
    kind = rng.integers(0, 6, size=(nsets, nv, M))          # 0 free, 1 lower, 2 upper, 3 boxed, 4 fixed, 5 boxed and violated
    lo = zref - spread * rng.uniform(0.01, 1.0, size=zref.shape)
    up = zref + spread * rng.uniform(0.01, 1.0, size=zref.shape)
    zl = np.where(np.isin(kind, (1, 3)), lo, -INF)
    zu = np.where(np.isin(kind, (2, 3)), up, INF)
    zl = np.where(kind == 4, zref, zl); zu = np.where(kind == 4, zref, zu)
    zl = np.where(kind == 5, up, zl); zu = np.where(kind == 5, up + spread, zu)      # z below its lower bound
    cl, cu = np.full(lay.np, -INF), np.zeros(lay.np)                                  # keep-outs: c <= 0
    if lay.np > 1:
        cl[1::3] = -2.0                                                               # two-sided rows
    if lay.np > 2:
        cl[2::3], cu[2::3] = 0.5, INF                                                 # lower-only rows
    return np.ascontiguousarray(zl), np.ascontiguousarray(zu), cl, cu


@pytest.mark.parametrize("name,per_instance", [("pm_sets_65x16_max", True), ("pm_shipped_33x3", False), ("quad_129x16", True),
                                               ("quad_1000x130", False), ("fixedwing_129x3_max", True), ("traced_rows_256x3", False),
                                               ("traced_rows_wide_65x16", True), ("quad_5x1", False), ("quad_1024x1", True),
                                               ("traced_rows_wide_65x1024", False), ("fixedwing_33x1024", True)])
def test_certificate_against_numpy(built, name, per_instance):
    c = make_case(name)
    ev = make_evaluator(c)
    lay = ev.layout
    RES, VALS, COST = ev.eval_host(c["X"], c["U"])
    zl, zu, cl, cu = bounds_for(c, lay, per_instance)
    for kind in ("normal", "single1"):
        lamF, lamC, sigma = multipliers(c, lay, kind)
        cert, G = ev.kkt_certificate_host(c["X"], c["U"], lamF, lamC, zl, zu, cl, cu, sigma)
        assert np.array_equal(G, ev.lagr_grad_host(VALS, lamF, lamC, sigma))         # the certificate's G is the gradient call's
        ref = A.certificate(G, RES, c["X"], c["U"], VALS, lamF, lamC, sigma, zl, zu, cl, cu)
        print(f"{name} {kind}: device {cert.max(axis=0)}  numpy {ref.max(axis=0)}")
        for q, f in enumerate(A.FIELDS):
            if f == "comp":
                assert np.all(np.abs(cert[:, q] - ref[:, q]) <= 4 * A.EPS * np.abs(ref[:, q])), (f, cert[:, q], ref[:, q])
            else:
                assert np.array_equal(cert[:, q], ref[:, q]), (f, cert[:, q], ref[:, q])
        assert np.all(cert[:, 3] > 0) and np.all(cert[:, 1] > 0)                      # the bounds above do reach those branches
    ev.close()


def test_two_calls_are_bit_identical_and_device_form_matches_host_form(built):
    import torch
    c = make_case("quad_1000x130")
    ev = make_evaluator(c)
    lay = ev.layout
    zl, zu, cl, cu = bounds_for(c, lay, True)
    lamF, lamC, sigma = multipliers(c, lay, "normal")
    a = ev.kkt_certificate_host(c["X"], c["U"], lamF, lamC, zl, zu, cl, cu, sigma)
    b = ev.kkt_certificate_host(c["X"], c["U"], lamF, lamC, zl, zu, cl, cu, sigma)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # device-pointer forms, asynchronous on the context's stream; G left in the workspace (dG NULL) and returned
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ev.device)
    X, U, lF, lC, dzl, dzu = (dev(x) for x in (c["X"], c["U"], lamF, lamC, zl, zu))
    RES, VALS, COST = ev.alloc_outputs()
    ev.eval_dev(X, U, RES, VALS, COST)
    cert = torch.full((lay.B, 6), -1.0, dtype=torch.float64, device=ev.device)
    G = torch.full((lay.B, lay.ns + lay.nc, lay.M), 7.0, dtype=torch.float64, device=ev.device)
    ev.kkt_certificate_dev(X, U, RES, VALS, lF, lC, sigma, dzl, dzu, cl, cu, cert, G)
    ev.synchronize()
    assert np.array_equal(cert.cpu().numpy(), a[0]) and np.array_equal(G.cpu().numpy(), a[1])
    cert2 = torch.zeros_like(cert)
    ev.kkt_certificate_dev(X, U, RES, VALS, lF, lC, sigma, dzl, dzu, cl, cu, cert2, None)
    G2 = torch.zeros_like(G)
    ev.lagr_grad_dev(VALS, lF, lC, sigma, G2)
    ev.synchronize()
    assert torch.equal(cert2, cert) and torch.equal(G2, G)
    ev.close()


@pytest.mark.parametrize("name", ["quad_1000x130", "pm_sets_65x16_max", "quad_129x16"])
def test_an_instance_inside_a_batch_and_alone_agree_within_the_bound(built, name):
    c = make_case(name)
    ev = make_evaluator(c)
    lay = ev.layout
    lamF, lamC, sigma = multipliers(c, lay, "normal")
    VALS = ev.eval_host(c["X"], c["U"])[1]
    G = ev.lagr_grad_host(VALS, lamF, lamC, sigma)
    _, T, bnd = reference(c, ev, VALS, lamF, lamC, sigma)
    for b in (0, lay.B // 2, lay.B - 1):
        one = make_evaluator(c, B=1, first=b)
        V1 = one.eval_host(c["X"][b:b + 1], c["U"][b:b + 1])[1]
        G1 = one.lagr_grad_host(V1, lamF[b:b + 1], lamC[b:b + 1], sigma)
        extra = 5e-13 * T[b] if not np.array_equal(V1[0], VALS[b]) else 0.0          # VALS of the two dispatch forms may differ by roundings
        assert np.all(np.abs(G1[0] - G[b]) <= bnd[b] + extra), float((np.abs(G1[0] - G[b]) / np.maximum(bnd[b], 1e-300)).max())
        one.close()
    ev.close()


def test_statuses_of_contexts_without_an_adjoint_pass(built):
    import etol_amd as E
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    lib = L.load()
    M, B = 16, 2
    X, U, _ = W.quadrotor_batch(1, B, M, 0)
    lamF = np.ones((B, 6, M))
    zl, zu = np.full((1, 8, M), -INF), np.full((1, 8, M), INF)

    def status(ev, nc=2):
        V = np.zeros((B, ev.layout.nvals, M))
        G = np.zeros((B, 6 + nc, M))
        cert = np.zeros((B, 6))
        d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        s1 = lib.emi_lagr_grad_host(ev.ctx, d(V), d(lamF), None, 1.0, d(G))
        msg = lib.emi_last_error(ev.ctx).decode()
        s2 = lib.emi_kkt_certificate_host(ev.ctx, d(X), d(U), d(lamF), None, 1.0, d(zl), d(zu), 1, None, None, d(cert), None)
        assert s1 == s2
        return s1, msg

    ev = E.Evaluator(0, f32=True)                       # fp32 context
    ev.set_mesh(M, 0.0, 2.0); ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS); ev.set_batch(B)
    st, msg = status(ev)
    assert L.STATUS[st] == "EMI_ERR_UNSUPPORTED" and "fp32" in msg
    ev.close()
    ev = E.Evaluator(0)                                 # delays: one free control and its delayed copy
    ev.set_mesh(M, 0.0, 2.0); ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS); ev.set_delays(0, 1, 0.1); ev.set_batch(B)
    assert ev.n_delayed == 1
    st, msg = status(ev)
    assert L.STATUS[st] == "EMI_ERR_UNSUPPORTED" and "delay" in msg
    ev.close()
    ev = E.Evaluator(0)                                 # points-only mesh
    tau, w, _ = E.lgl(M)
    d = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.emi_set_mesh(ev.ctx, M, d(tau), d(w), None, 0.0, 2.0) == 0
    ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS); ev.set_batch(B)
    st, msg = status(ev)
    assert L.STATUS[st] == "EMI_ERR_STATE" and "points-only" in msg
    ev.close()
    ev = E.Evaluator(0)                                 # and a context that has one says ok; the mesh may change under it
    ev.set_mesh(M, 0.0, 2.0); ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS); ev.set_batch(B)
    assert status(ev)[0] == 0
    for M2 in (2, 3, 16):
        ev.set_mesh(M2, 0.0, 2.0)
        X2, U2, _ = W.quadrotor_batch(1, B, M2, 0)
        c = dict(M=M2, B=B)
        lF, lC, sigma = multipliers(c, ev.layout, "normal")
        V = ev.eval_host(X2, U2)[1]
        G = ev.lagr_grad_host(V, lF, lC, sigma)
        Gn, T, bnd = reference(c, ev, V, lF, lC, sigma)
        assert np.all(np.abs(G - Gn) <= bnd)
    ev.close()
