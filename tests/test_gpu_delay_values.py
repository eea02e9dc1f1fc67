"""Contexts with delays, element by element.  -m gpu

1. The tap models of tests/delay_ref.py carry the extended node variables [U | x(t - i dt) | u(t - i dt)] out of a nodes-only pass
   without a rounding (control experiment on a context without delays).
2. The delayed values extend_controls (csrc/emi_api_pass.hip) forms, each element against the long-double product with the
   library's own W:  |got - ref| <= (M + 2) u S, no floor; the value of a unit row of W (clamped, or a delayed time exactly on a
   node) is its source's node value itself.  Shapes: delay_ref.CASES.  Outputs hold NaN before every pass; every context is called
   a second time with other inputs (a stale extended buffer).
3. Given those values, a context with delays returns the bits of a context without delays that runs the same model on
   [U | those values] as ordinary controls: RES, VALS, COST and the Hessian, host and device forms, every form of the pass the
   context can take, values-only passes, a pass that keeps the invariant rows around a set_path, and the "slice" option.  The model
   kernels are the instantiations test_gpu_first_order.py and test_gpu_hessian.py hold elementwise, so 2 and 3 together carry
   those bounds over to contexts with delays.

Every check prints its worst ratio and its counts (pytest -s)."""
import numpy as np
import pytest

import delay_ref as R
from etol_amd import workloads as WL
from test_gpu_delay_adjoint import DISC, demo_source

pytestmark = pytest.mark.gpu

_OPEN = []
_MESH = {}


@pytest.fixture(autouse=True)
def close_evaluators():
    yield
    while _OPEN:
        _OPEN.pop().close()


def mesh(M):
    import etol_amd as E
    if M not in _MESH:
        _MESH[M] = E.lgl(M)
    return _MESH[M]


def tap_ev(ns, nc, M, B, t0, tf, delays=None):
    """a context on the tap model; delays: (xh, uh, dt) or None"""
    import etol_amd as E
    ev = E.Evaluator(0)
    _OPEN.append(ev)
    ev.set_mesh(M, t0, tf, mesh=mesh(M))
    ev.set_model_source(*R.tap_source(ns, nc), ns, nc)
    if delays:
        ev.set_delays(*delays)
    ev.set_batch(B)
    return ev


def taps(ev, X, U, h, outs=None):
    """One nodes-only Jacobian pass of a tap context into NaN-filled outputs -> (states [B][ns][M] out of RES, control slots
    [B][nc][M] out of row 0 of VALS) as numpy arrays; X, U numpy"""
    import etol_amd as E
    import torch
    lay = ev.layout
    dX, dU = torch.from_numpy(np.ascontiguousarray(X)).to(ev.device), torch.from_numpy(np.ascontiguousarray(U)).to(ev.device)
    outs = outs or ev.alloc_outputs()
    for t in outs:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    ev.eval_dev(dX, dU, *outs, flags=E.EVAL_NODES)
    ev.synchronize()
    RES, VALS = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert (outs[2].cpu().numpy() == 0).all()
    return -RES[:, :lay.ns] / h, -VALS[:, lay.ns:lay.ns + lay.nc] / h


# ---- 1: the control experiment ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [(0.0, 2.0), (0.5, 8.5)])
def test_taps_return_the_node_variables_of_a_context_without_delays(built, span):
    """X and U back bit for bit, -0.0, denormals and 1e300 among them.  The states come out of RES = -h f with their zeros' signs;
    the control slots out of -h J + 0, which gives +0 for either zero (delay_ref.py): a zero comes back a zero, -0.0 as -0.0, and
    every other double with its bits."""
    ns, nc, M, B = 3, 5, 17, 2
    h = R.half_length(*span)
    ev = tap_ev(ns, nc, M, B, *span)
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((B, ns + nc, M)) * 10.0 ** rng.uniform(-3, 3, (B, ns + nc, M))
    special = [-0.0, 0.0, 5e-324, -2.5e-320, 2.2250738585072014e-308, 1e300, -1e300, 1.0, -1.0 / 3]
    for v in range(ns + nc):
        Z[v % B, v, (np.arange(len(special)) * 2 + v) % M] = special
    X, U = Z[:, :ns], Z[:, ns:]
    gotX, gotU = taps(ev, X, U, h)
    assert R.same_bits(gotX, X)
    assert R.same(gotU, U)
    nz = U != 0
    assert nz.sum() < U.size and R.same_bits(gotU[nz], U[nz])
    neg0 = (U == 0) & np.signbit(U)
    assert neg0.any() and np.signbit(gotU[neg0]).all()
    print(f"taps on [{span[0]}, {span[1]}]: {X.size + U.size} node variables back bit for bit ({int((~nz).sum())} zeros among the control slots by value)")


# ---- 2: delayed values against the long-double product -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_delayed_values_elementwise(built, name):
    c = R.case(name, mesh)
    nclamped_dt, nhit_dt = R.claims_hold(c)
    ns, ncf, xh, uh, M, B = (c[k] for k in ("ns", "ncf", "xh", "uh", "M", "B"))
    dims = (ns, ncf, xh, uh)
    ev = tap_ev(ns, c["nc"], M, B, c["t0"], c["tf"], (xh, uh, c["dt"]))
    assert ev.n_delayed == c["nc"] - ncf
    outs = ev.alloc_outputs()
    seen = []
    for call in range(c["ncalls"]):
        Z = R.inputs(c, call)
        ref, S = R.reference(Z, c["W"], *dims)
        gotX, gotU = taps(ev, Z[:, :ns], Z[:, ns:], c["h"], outs)
        assert R.same_bits(gotX, Z[:, :ns]) and R.same(gotU[:, :ncf], Z[:, ns:])          # the free part is the caller's
        got = gotU[:, ncf:]
        r = R.ratio(got, ref, S, M)
        w = np.unravel_index(np.argmax(r), r.shape)
        ok, nclamped, nhit = R.unit_rows_hold(got, Z, c["W"], c["mesh"], c["t0"], c["tf"], c["dt"], *dims)
        print(f"{name} call {call}: worst |got - ref| / ((M+2) u S) = {r.max():.3f} at (instance, slot, node) {tuple(int(i) for i in w)}; "
              f"rows of W per instance: clamped {nclamped}, hit {nhit} (of W(dt): {nclamped_dt}, {nhit_dt}); unit rows exact: {ok}")
        assert ok, "a unit row of W did not return its source's node value"
        assert r.max() <= 1.0
        assert (got[S == 0] == 0).all()
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])


# ---- 3: whole passes and the Hessian, by bit equality ----------------------------------------------------------------------------------
# name -> model kind, M, B, (xh, uh), dt, (t0, tf)
WHOLE = {
    "demo_33x3":     ("demo", 33, 3, (3, 1), 0.2, (0.0, 8.0)),
    "demo_128x20":   ("demo", 128, 20, (3, 1), 0.2, (0.0, 8.0)),
    "demo_129x49":   ("demo", 129, 49, (3, 1), 0.2, (0.0, 8.0)),
    "quad_128x5":    ("quad", 128, 5, (0, 1), 0.15, (0.0, 16.0)),
    "quad_257x17":   ("quad", 257, 17, (0, 1), 0.15, (0.0, 16.0)),
    "wing_33x3_u1":  ("wing", 33, 3, (0, 1), 0.25, (0.0, 8.0)),
    "wing_33x9_u3":  ("wing", 33, 9, (0, 3), 0.25, (0.0, 8.0)),
    "demo_128x37":   ("demo", 128, 37, (3, 1), 0.2, (0.0, 8.0)),          # the "slice" cases
    "quad_128x37":   ("quad", 128, 37, (0, 1), 0.15, (0.0, 16.0)),
}
DIMS = {"demo": (2, 8), "quad": (6, 2), "wing": (12, 4)}


def whole_inputs(kind, M, B, ncf, t, seed=0):
    rng = np.random.default_rng(31 * M + B + 1000 * seed)
    if kind == "demo":
        X = np.stack([1 + 0.5 * np.sin(0.7 * t + rng.uniform(0, 3, (B, 1))), 2 - 0.1 * t + 0.3 * np.cos(t + rng.uniform(0, 3, (B, 1)))], axis=1)
        U = np.stack([0.3 * np.cos(t + rng.uniform(0, 3, (B, 1))), 0.2 + 0.1 * np.sin(2 * t + rng.uniform(0, 3, (B, 1)))], axis=1)
        recs = DISC
    elif kind == "quad":
        X, U, recs = WL.quadrotor_batch(9 + seed, B, M, 2)
    else:
        X, U = WL.fixedwing_batch(5 + seed, B, M)
        recs = None
    return np.ascontiguousarray(X), np.ascontiguousarray(U[:, :ncf]), recs


def model_ev(kind, M, B, span, recs, delays=None):
    import etol_amd as E
    ev = E.Evaluator(0)
    _OPEN.append(ev)
    ev.set_mesh(M, *span, mesh=mesh(M))
    if kind == "demo":
        ev.set_model_source("TracedModel", demo_source(), 2, 8)
    elif kind == "quad":
        ev.set_model(E.MODEL_QUADROTOR2D, WL.QUAD_PARAMS)
    else:
        ev.set_model(E.MODEL_FIXEDWING12, WL.FW_PARAMS)
    if delays:
        ev.set_delays(*delays)
    ev.set_batch(B)
    if recs is not None:
        ev.set_path(recs, 0, 1)
    return ev


class Pair:
    """the context with delays (D), the plain context on the extended controls (P), and the inputs of both on the device"""

    def __init__(self, name):
        import torch
        kind, M, B, (xh, uh), dt, span = WHOLE[name]
        ns, nc = DIMS[kind]
        ncf = next(n for n in (1, 2, 3) if R.nc_of(ns, n, xh, uh) == nc)
        self.name, self.kind, self.M, self.B, self.ns, self.nc, self.ncf, self.span = name, kind, M, B, ns, nc, ncf, span
        self.h = R.half_length(*span)
        self.delays = (xh, uh, dt)
        t = span[0] + self.h * (mesh(M)[0] + 1.0)
        self.tap = tap_ev(ns, nc, M, B, *span, self.delays)
        self.X, self.U, self.recs = whole_inputs(kind, M, B, ncf, t)
        self.D = model_ev(kind, M, B, span, self.recs, self.delays)
        self.P = model_ev(kind, M, B, span, self.recs)
        assert self.D.n_delayed == nc - ncf and self.P.n_delayed == 0 and self.D.layout.nc == self.P.layout.nc == nc
        self.dX = torch.from_numpy(self.X).to(self.D.device)
        self.set_inputs(self.X, self.U)

    def set_inputs(self, X, U):
        """the delayed values of (X, U) as the DEVICE forms them (tap context), held elementwise by part 2's criterion here too"""
        import torch
        self.X, self.U = X, U
        gotX, ext = taps(self.tap, X, U, self.h)
        assert R.same_bits(gotX, X) and R.same(ext[:, :self.ncf], U)
        xh, uh, dt = self.delays
        W = R.delay_matrices(mesh(self.M), *self.span, dt, xh, uh)
        ref, S = R.reference(np.concatenate([X, U], axis=1), W, self.ns, self.ncf, xh, uh)
        r = R.ratio(ext[:, self.ncf:], ref, S, self.M)
        print(f"{self.name}: delayed values of the tap context: worst |got - ref| / ((M+2) u S) = {r.max():.3f}")
        assert r.max() <= 1.0
        # (a zero comes back from the taps as -0; the product, a sum onto +0, can only give +0)
        self.Uext = np.ascontiguousarray(np.concatenate([U, ext[:, self.ncf:] + 0.0], axis=1))
        self.dX = torch.from_numpy(X).to(self.D.device)
        self.dU = torch.from_numpy(U).to(self.D.device)
        self.dUext = torch.from_numpy(self.Uext).to(self.D.device)

    def both(self, option, value):
        self.D.set_option(option, value)
        self.P.set_option(option, value)

    def passes(self, flags, outsD=None, outsP=None, poison=(True, True, True)):
        """one device pass on each context into (NaN-filled) outputs -> (outputs of D, outputs of P) as numpy arrays"""
        import torch
        outsD, outsP = outsD or self.D.alloc_outputs(), outsP or self.P.alloc_outputs()
        for outs in (outsD, outsP):
            for t, p in zip(outs, poison):
                if p:
                    t.fill_(float("nan"))
        torch.cuda.synchronize()
        self.D.eval_dev(self.dX, self.dU, *outsD, flags=flags)
        self.P.eval_dev(self.dX, self.dUext, *outsP, flags=flags)
        self.D.synchronize()
        self.P.synchronize()
        return [t.cpu().numpy() for t in outsD], [t.cpu().numpy() for t in outsP]


def assert_same_outputs(what, gotD, gotP, vals=True):
    for nm, a, b in zip(("RES", "VALS", "COST"), gotD, gotP):
        if nm == "VALS" and not vals:
            assert np.isnan(a).all() and np.isnan(b).all(), (what, "a values-only pass wrote VALS")
            continue
        assert not np.isnan(b).any(), (what, nm, "the plain context left NaN")
        if not R.same_bits(a, b):
            bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
            raise AssertionError(f"{what}: {nm} differs in {len(bad)} of {a.size} elements, first at {tuple(bad[0])}: "
                                 f"{a[tuple(bad[0])]!r} (delays) vs {b[tuple(bad[0])]!r} (extended controls)")


def rowwise_bound_of_test_gpu_delays(gotD, gotP, tol=1e-12):
    """the default run where the two contexts took different forms: every row in the max norm at 1e-12 (max |row| + 1)"""
    for a, b in zip(gotD, gotP):
        a, b = a.reshape(a.shape[0], -1, a.shape[-1]) if a.ndim == 3 else a[None, None], b.reshape(b.shape[0], -1, b.shape[-1]) if b.ndim == 3 else b[None, None]
        for e in range(a.shape[1]):
            assert np.abs(a[:, e] - b[:, e]).max() <= tol * (np.abs(b[:, e]).max() + 1.0)


def forms_of(p):
    """(label, options) of every form a delayed context of this shape can take; the options are set on both contexts"""
    forms = [("default", {}), ("sequential", {"overlap": 0, "small_rows": 0}), ("one stream", {"overlap_mode": 1, "small_rows": 0}),
             ("two streams", {"overlap_mode": 2, "small_rows": 0}), ("one launch", {"overlap_mode": 3, "small_rows": 0})]
    if p.B * p.ns <= 96:
        forms.append(("skinny product", {"overlap": 0, "small_rows": 96}))
    return forms


DEFAULTS = {"overlap": 1, "overlap_mode": 0, "small_rows": 24}
_KERNELS = {}


@pytest.mark.parametrize("name", [n for n in WHOLE if not n.endswith("x37")])
def test_whole_passes_and_hessian_give_the_bits_of_the_extended_controls(built, name):
    """Every form, device and host calls, full and values-only passes, the Hessian; then a second set of inputs on the same contexts."""
    import etol_amd as E
    import torch
    p = Pair(name)
    rng = np.random.default_rng(len(name) + p.M)
    lay = p.D.layout
    lamF, lamC = rng.standard_normal((p.B, lay.ns, p.M)), rng.standard_normal((p.B, lay.np, p.M))
    assert lay.np == p.P.layout.np and lay.nvals == p.P.layout.nvals and lay.nhess == p.P.layout.nhess
    kernels = _KERNELS.setdefault(name, {})
    for second in (False, True):
        if second:
            t = p.span[0] + p.h * (mesh(p.M)[0] + 1.0)
            X2, U2, _ = whole_inputs(p.kind, p.M, p.B, p.ncf, t, seed=1)
            assert not np.array_equal(U2, p.U)
            p.set_inputs(X2, U2)
        for label, opts in (forms_of(p) if not second else forms_of(p)[:2]):
            for k, v in {**DEFAULTS, **opts}.items():
                p.both(k, v)
            what = f"{name}, {label}" + (", second inputs" if second else "")
            gotD, gotP = p.passes(E.EVAL_ALL)
            kD, kP = (p.D.last_defect_kernel, p.D.uses_fused_kernel), (p.P.last_defect_kernel, p.P.uses_fused_kernel)
            kernels[label] = kD[0]
            if label == "default" and kD != kP:
                print(f"{what}: the default policy took {kD} with delays and {kP} without: held to 1e-12 per row here, bit for bit under the forced forms")
                rowwise_bound_of_test_gpu_delays(gotD, gotP)
            else:
                assert kD == kP, (what, kD, kP)
                assert_same_outputs(what, gotD, gotP)
            print(f"    {what}: {kD[0]}")
            gotD, gotP = p.passes(E.EVAL_ALL | E.EVAL_NOJAC)
            assert (p.D.last_defect_kernel, p.D.uses_fused_kernel) == (p.P.last_defect_kernel, p.P.uses_fused_kernel) or label == "default"
            if label != "default" or kD == kP:
                assert_same_outputs(what + ", values only", gotD, gotP, vals=False)
            hostD, hostP = p.D.eval_host(p.X, p.U), p.P.eval_host(p.X, p.Uext)
            if label != "default" or kD == kP:
                assert_same_outputs(what + ", host call", hostD, hostP)
    if "skinny product" in kernels:
        assert "small" in kernels["skinny product"] and "small" not in kernels["sequential"]
    if p.kind == "quad" and p.M % 128 == 0:
        assert "emi_pass_f64_kernel" in kernels["one launch"], kernels
    # the Hessian on the extended node variables
    HD, HP = p.D.hess_host(p.X, p.U, lamF, lamC, sigma=0.8), p.P.hess_host(p.X, p.Uext, lamF, lamC, sigma=0.8)
    assert np.abs(HP).max() > 0 and R.same_bits(HD, HP), name
    dl = [torch.from_numpy(a).to(p.D.device) for a in (lamF, lamC)]
    Hd = [torch.full((p.B, lay.nhess, p.M), float("nan"), dtype=torch.float64, device=p.D.device) for _ in range(2)]
    torch.cuda.synchronize()
    p.D.hess_dev(p.dX, p.dU, dl[0], dl[1] if lay.np else None, 0.8, Hd[0])
    p.P.hess_dev(p.dX, p.dUext, dl[0], dl[1] if lay.np else None, 0.8, Hd[1])
    p.D.synchronize()
    p.P.synchronize()
    assert R.same_bits(Hd[0].cpu().numpy(), HP) and R.same_bits(Hd[1].cpu().numpy(), HP), name


@pytest.mark.parametrize("name", ["demo_33x3", "quad_128x5"])
def test_pass_that_keeps_the_invariant_rows_around_a_set_path(built, name):
    """A Jacobian pass, set_path with other records, and a pass into the same untouched VALS (the evaluator asks for
    EMI_EVAL_KEEP_INVARIANT; the library decides whether the record still stands): both contexts end with the same bits, and
    those are the bits of a full pass of the plain context into a fresh VALS."""
    import etol_amd as E
    p = Pair(name)
    outsD, outsP = p.D.alloc_outputs(), p.P.alloc_outputs()
    first = p.passes(E.EVAL_ALL, outsD, outsP)
    assert_same_outputs(f"{name}, first pass", *first)
    recs = np.array(p.recs, dtype=np.float64, copy=True)
    recs[..., 1:4] *= 1.125                                  # other centres and radii
    for ev in (p.D, p.P):
        ev.set_path(recs, 0, 1)
    assert outsD[1] is p.D._kept and outsP[1] is p.P._kept
    kept = p.passes(E.EVAL_ALL, outsD, outsP, poison=(True, False, True))
    assert_same_outputs(f"{name}, pass that keeps the invariant rows", *kept)
    fresh = p.passes(E.EVAL_ALL)
    assert_same_outputs(f"{name}, kept against a fresh pass", kept[0], fresh[1])
    assert not R.same_bits(first[0][0], kept[0][0])          # the new records did enter


@pytest.mark.parametrize("name", ["demo_128x37", "quad_128x37"])
def test_slice_option_gives_the_bits_of_the_unsliced_call(built, name):
    """B = 37 with "slice" 16: pieces of 16, 16 and 5 instances, each reading the extended buffer from its first instance on.
    Jacobian passes under the default dispatch.  Values-only passes with "small_rows" 0 and "sym_ksplit" 1: left to itself the
    dispatch gives the 5-instance piece of the two-state model (10 rows) to the skinny product and may cut a small piece's K range
    into slices -- other summation orders than the whole batch's kernel, with or without delays (include/emi355x.h)."""
    import etol_amd as E
    p = Pair(name)
    whole = p.passes(E.EVAL_ALL)
    assert p.D.plan()["piece"] == 0
    assert_same_outputs(f"{name}, unsliced", *whole)
    p.both("slice", 16)
    assert p.D.plan()["piece"] == 16 and p.P.plan()["piece"] == 16
    sliced = p.passes(E.EVAL_ALL)
    print(f"    {name}, sliced: {p.D.last_defect_kernel}")
    assert_same_outputs(f"{name}, sliced", *sliced)
    assert_same_outputs(f"{name}, sliced against unsliced", sliced[0], whole[0])
    host = p.D.eval_host(p.X, p.U)
    assert_same_outputs(f"{name}, sliced host call against unsliced", host, whole[0])
    p.both("sym_ksplit", 1)
    p.both("small_rows", 0)
    values = p.passes(E.EVAL_ALL | E.EVAL_NOJAC)
    print(f"    {name}, sliced, values only: {p.D.last_defect_kernel}")
    assert_same_outputs(f"{name}, sliced, values only", *values, vals=False)
    p.both("slice", 0)
    whole_values = p.passes(E.EVAL_ALL | E.EVAL_NOJAC)
    print(f"    {name}, unsliced, values only: {p.D.last_defect_kernel}")
    assert_same_outputs(f"{name}, unsliced, values only", *whole_values, vals=False)
    assert_same_outputs(f"{name}, sliced against unsliced, values only", values[0], whole_values[0], vals=False)
