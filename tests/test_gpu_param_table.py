"""Per-instance model parameters for a context's batch (emi_set_model_params_batch).  -m gpu

THE REFERENCE THROUGHOUT is a context of the same B, M and tables that holds row b of the table as its shared parameter set
(emi_set_model*), under option "overlap" 0 -- the sequential route a context with a table takes.  Instance b of the tabled context is
compared with instance b of that reference BIT FOR BIT; the shared-parameter path itself is pinned by the parity, Hessian, f32 and
ODE-error tests.  Equal B on both sides keeps the defect kernel (small / general) the same.  Every output goes into a NaN-filled
buffer with 64 poisoned elements behind it, which must keep their bits.  fp64 evaluations are held to the CPU oracle as well, called
once per instance with that instance's row, at the bounds of tests/test_gpu_parity.py.

Two notes on the cases:
  * slicing: the option "slice" takes multiples of 16 instances only, so "slice" 2 on a batch of 7 is refused (asserted here; the batch
    then runs whole) and the sliced case proper is B = 37 with "slice" 16: pieces of 16, 16 and 5 instances, each on its own rows of the
    table;
  * the traced quadrotor with parameters is traced by tests/harness/etol_harness_param_table.cpp with the parameter block as inputs of
    the trace (P.p[i] in the generated text).
The iteration rule of the lock-step case is the project's existing one (tests/test_gpu_lockstep.py): the sum over the batch within
1.5 x the fixture's."""
import ctypes as C

import numpy as np
import pytest

import lockstep_ref as LR
import oracle_lib as O
import param_table_ref as PT

pytestmark = pytest.mark.gpu

ARG, STATE, UNSUPPORTED = 1, 2, 5
POISON = 64
TAIL64, TAIL32 = -1.2345e300, -1.2345e30
B5 = 5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Out:
    """an output array of the context's type: NaN-filled, 64 poisoned elements behind it"""

    def __init__(self, ev, shape):
        import torch
        n = int(np.prod(shape))
        self.flat = torch.full((n + POISON,), float("nan"), dtype=ev.dtype, device=ev.device)
        self.flat[n:] = TAIL32 if ev.f32 else TAIL64
        self.tail = self.flat[n:].cpu().numpy().copy()
        self.t = self.flat[:n].view(*shape)

    def get(self, written=True):
        """the array on the host; the poison behind it untouched; written: no NaN left / still all NaN"""
        a = self.flat.cpu().numpy()
        n = a.size - POISON
        assert np.array_equal(bits(a[n:]), bits(self.tail)), "the elements behind the output were written"
        if written:
            assert not np.isnan(a[:n]).any(), "elements of the output were not written"
        else:
            assert np.isnan(a[:n]).all(), "an output that the call does not produce was written"
        return a[:n].reshape(tuple(self.t.shape)).astype(np.float64)


def problem(kind, B, M):
    """-> dict model, base (nominal parameters), tf, X, U, recs (per-instance record table or None)"""
    import etol_amd as E
    from etol_amd import workloads as W
    if kind == "quad":
        X, U, recs = W.quadrotor_batch(3, B, M, 3)
        return dict(model=E.MODEL_QUADROTOR2D, base=np.array(W.QUAD_PARAMS), tf=W.TF, X=X, U=U, recs=recs)
    if kind == "fixedwing":
        X, U = W.fixedwing_batch(4, B, M)
        return dict(model=E.MODEL_FIXEDWING12, base=np.array(W.FW_PARAMS), tf=20.0, X=X, U=U, recs=None)
    X, U = W.pointmass_batch(5, B, M)
    return dict(model=E.MODEL_POINTMASS2D, base=np.zeros(0), tf=W.TF, X=X, U=U, recs=None)


def context(p, B, M, params, f32=False, overlap0=False):
    import etol_amd as E
    ev = E.Evaluator(0, f32=f32)
    ev.set_mesh(M, 0.0, p["tf"])
    ev.set_model(p["model"], params)
    ev.set_batch(B)
    if p["recs"] is not None:
        ev.set_path(p["recs"], 0, 1)
    if overlap0:
        ev.set_option("overlap", 0)
    return ev


def reshare(ev, p, params):
    """the reference context under another shared set (a new model drops the record table)"""
    ev.set_model(p["model"], params)
    if p["recs"] is not None:
        ev.set_path(p["recs"], 0, 1)


def device_inputs(ev, *arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(ev.dtype).to(ev.device) for a in arrays]
    torch.cuda.synchronize()
    return out


def evaluate(ev, dX, dU, flags):
    """one emi_eval_dev into fresh poisoned buffers -> (RES, VALS or None, COST) as float64 numpy"""
    import torch
    import etol_amd as E
    lay = ev.layout
    RES, VALS, COST = Out(ev, (lay.B, lay.nres, lay.M)), Out(ev, (lay.B, lay.nvals, lay.M)), Out(ev, (lay.B,))
    torch.cuda.synchronize()
    ev.eval_dev(dX, dU, RES.t, VALS.t, COST.t, flags=flags)
    ev.synchronize()
    torch.cuda.synchronize()
    jac = not (flags & E.EVAL_NOJAC)
    vals = VALS.get(written=jac)
    return RES.get(), (vals if jac else None), COST.get()


def same_instance(got, ref, b, what):
    for name, g, r in zip(("RES", "VALS", "COST"), got, ref):
        if g is None:
            assert r is None
            continue
        assert np.array_equal(bits(g[b]), bits(r[b])), f"{what}: {name} of instance {b} differs from the reference with row {b} as the shared set"


# ---- 1. evaluation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32,M", [(False, 33), (False, 128), (True, 128), (True, 50)], ids=["f64-33", "f64-128", "f32-128", "f32-50"])
@pytest.mark.parametrize("kind", ["quad", "fixedwing", "pointmass"])
def test_evaluation_gives_each_instance_its_rows_bits(built, kind, f32, M):
    import etol_amd as E
    import test_gpu_parity as TP
    B = B5
    p = problem(kind, B, M)
    if f32:                                                     # what the device will see
        p["X"], p["U"] = (a.astype(np.float32).astype(np.float64) for a in (p["X"], p["U"]))
    rows = PT.rows_for(p["base"], B)
    assert rows.shape == (B, p["base"].size) and (p["base"].size == 0 or len({tuple(r) for r in rows}) == B)
    ev = context(p, B, M, p["base"], f32)
    if not f32 and M % 128 == 0 and kind == "quad":
        assert ev.plan()["one_launch"] == 1 and ev.uses_fused_kernel           # a pass-eligible mesh ...
    ev.set_model_params(rows)
    assert np.array_equal(ev.get_model_params(), rows)
    plan = ev.plan()
    assert plan["one_launch"] == 0 and plan["mfma_workgroups"] == 0 and plan["piece"] == 0 and not ev.uses_fused_kernel   # ... has left the one-launch form
    ref = context(p, B, M, p["base"], f32, overlap0=True)
    dX, dU = device_inputs(ev, p["X"], p["U"])
    for flags in (E.EVAL_ALL, E.EVAL_ALL | E.EVAL_NOJAC):
        got = evaluate(ev, dX, dU, flags)
        if not f32:
            assert "emi_pass" not in ev.last_defect_kernel and "symdefect" not in ev.last_defect_kernel, ev.last_defect_kernel
        nominal_cost = None
        differs = 0
        for b in range(B):
            reshare(ref, p, rows[b])
            want = evaluate(ref, dX, dU, flags)
            same_instance(got, want, b, f"{kind} M {M} flags {flags}")
            if b == 0:
                nominal_cost = want[2].copy()                   # row 0 is the nominal set: what a kernel that ignores the table computes
            if not f32 and flags == E.EVAL_ALL:
                o = O.evaluate(p["model"], rows[b], M, (ev.tau, ev.w, ev.D), 0.0, p["tf"], p["X"][b:b + 1], p["U"][b:b + 1],
                               None if p["recs"] is None else p["recs"][b:b + 1])
                TP.check(dict(X=p["X"][b:b + 1]), ev, tuple(a[b:b + 1] for a in got), o)
        rel = np.abs(got[2] - nominal_cost) / (np.abs(nominal_cost) + 1.0)
        differs = int((rel > (1e-5 if f32 else 1e-13)).sum())
        print(f"{kind} M {M} f32 {f32} flags {flags}: COST against the nominal set's, relative", rel)
        if p["base"].size:
            assert differs >= 2, rel                            # the rows reach the kernel
    ev.close()
    ref.close()


# ---- 2. table equivalence and removal -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [33, 128])
def test_equal_rows_are_the_shared_set_and_removal_restores_the_default(built, M):
    import etol_amd as E
    B = B5
    p = problem("quad", B, M)
    row = PT.rows_for(p["base"], 2)[1]
    never = context(p, B, M, row)                               # never had a table: the default plan
    seq = context(p, B, M, row, overlap0=True)
    ev = context(p, B, M, row)
    dX, dU = device_inputs(ev, p["X"], p["U"])
    default_plan = never.plan()
    assert ev.plan() == default_plan
    ev.set_model_params(np.tile(row, (B, 1)))
    assert ev.plan()["one_launch"] == 0 and not ev.uses_fused_kernel
    for flags in (E.EVAL_ALL, E.EVAL_ALL | E.EVAL_NOJAC):
        got, want = evaluate(ev, dX, dU, flags), evaluate(seq, dX, dU, flags)
        for b in range(B):
            same_instance(got, want, b, f"equal rows, M {M}")
    ev.set_model_params(None)
    assert ev.get_model_params() is None
    assert ev.plan() == default_plan and ev.uses_fused_kernel == never.uses_fused_kernel
    for flags in (E.EVAL_ALL, E.EVAL_ALL | E.EVAL_NOJAC):
        got, want = evaluate(ev, dX, dU, flags), evaluate(never, dX, dU, flags)
        assert ev.last_defect_kernel == never.last_defect_kernel
        for b in range(B):
            same_instance(got, want, b, f"table removed, M {M}")
    for e in (ev, seq, never):
        e.close()


# ---- 3. slicing ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,slice_", [(7, 2), (37, 16)])
def test_a_sliced_batch_reads_the_rows_of_its_pieces(built, B, slice_):
    import etol_amd as E
    M = 33
    p = problem("quad", B, M)
    rows = PT.rows_for(p["base"], B)
    ev = context(p, B, M, p["base"])
    ev.set_model_params(rows)
    dX, dU = device_inputs(ev, p["X"], p["U"])
    whole = evaluate(ev, dX, dU, E.EVAL_ALL)
    if slice_ % 16:
        with pytest.raises(E.EmiError, match="slice"):          # the option takes whole 16-instance tiles only: this batch stays whole
            ev.set_option("slice", slice_)
    else:
        ev.set_option("slice", slice_)
        assert B > 2 * slice_ and B % slice_                    # pieces and a remainder
    sliced = evaluate(ev, dX, dU, E.EVAL_ALL)
    for b in range(B):
        same_instance(sliced, whole, b, f"B {B} slice {slice_}")
    ref = context(p, B, M, p["base"], overlap0=True)
    for b in (0, B // 2, B - 1):                                # ... and those bits are the reference's (first, a middle and the last piece)
        reshare(ref, p, rows[b])
        same_instance(sliced, evaluate(ref, dX, dU, E.EVAL_ALL), b, f"B {B} slice {slice_}")
    ev.close()
    ref.close()


# ---- 4. Hessian ---------------------------------------------------------------------------------------------------------------------
def hessian(ev, dX, dU, dLF, dLC, sigma):
    import torch
    lay = ev.layout
    H = Out(ev, (lay.B, lay.nhess, lay.M))
    torch.cuda.synchronize()
    ev.hess_dev(dX, dU, dLF, dLC, sigma, H.t)
    ev.synchronize()
    torch.cuda.synchronize()
    return H.get()


@pytest.mark.parametrize("M", [33, 257])
@pytest.mark.parametrize("kind", ["quad", "fixedwing"])
def test_hessian_blocks_take_the_instances_rows(built, kind, M):
    B = B5
    p = problem(kind, B, M)
    rows = PT.rows_for(p["base"], B)
    ev = context(p, B, M, p["base"])
    ev.set_model_params(rows)
    ref = context(p, B, M, p["base"], overlap0=True)
    lay = ev.layout
    rng = np.random.default_rng(11 + M)
    lamF, lamC = rng.standard_normal((B, lay.ns, M)), rng.standard_normal((B, lay.np, M))
    dX, dU, dLF, dLC = device_inputs(ev, p["X"], p["U"], lamF, lamC)
    if lay.np == 0:
        dLC = None
    got = hessian(ev, dX, dU, dLF, dLC, 0.7)
    nominal = None
    for b in range(B):
        reshare(ref, p, rows[b])
        want = hessian(ref, dX, dU, dLF, dLC, 0.7)
        assert np.array_equal(bits(got[b]), bits(want[b])), (kind, M, b)
        nominal = want if b == 0 else nominal
    assert sum(not np.array_equal(got[b], nominal[b]) for b in range(1, B)) >= 2      # the rows reach the kernel
    ev.close()
    ref.close()


# ---- 5. ODE error -------------------------------------------------------------------------------------------------------------------
def ode_error(ev, dX, dU):
    import torch
    lay = ev.layout
    err, eta = Out(ev, (lay.B,)), Out(ev, (lay.B, lay.ns, lay.M - 1))
    torch.cuda.synchronize()
    A = ev._ipm_addr
    ev._ck(ev.lib.emi_ode_error_dev(ev.ctx, A(dX), A(dU), None, None, A(eta.t), A(err.t)), "emi_ode_error_dev")
    ev.synchronize()
    torch.cuda.synchronize()
    return err.get(), eta.get()


def test_ode_error_takes_the_instances_rows(built):
    B, M = B5, 33
    p = problem("quad", B, M)
    rows = PT.rows_for(p["base"], B)
    ev = context(p, B, M, p["base"])
    ev.set_model_params(rows)
    ref = context(p, B, M, p["base"], overlap0=True)
    dX, dU = device_inputs(ev, p["X"], p["U"])
    err, eta = ode_error(ev, dX, dU)
    nominal = None
    for b in range(B):
        reshare(ref, p, rows[b])
        rerr, reta = ode_error(ref, dX, dU)
        assert np.array_equal(bits(err[b]), bits(rerr[b])) and np.array_equal(bits(eta[b]), bits(reta[b])), b
        nominal = reta if b == 0 else nominal
    assert sum(not np.array_equal(eta[b], nominal[b]) for b in range(1, B)) >= 2
    ev.close()
    ref.close()


# ---- 6. traced models ---------------------------------------------------------------------------------------------------------------
def traced_quad_source():
    import os
    h = C.CDLL(os.path.join(LR.ROOT, "tests", "harness", "libetol_harness.so"))
    h.harness_param_table_traced_quad_source.restype = C.c_char_p
    return h.harness_param_table_traced_quad_source().decode()


def test_traced_quadrotor_with_parameters(built):
    import etol_amd as E
    B, M = 3, 33
    p = problem("quad", B, M)
    rows = PT.rows_for(p["base"], B)
    src = traced_quad_source()
    assert "P.p[0]" in src and "P.p[4]" in src

    def traced(params, overlap0):
        ev = E.Evaluator(0)
        ev.set_mesh(M, 0.0, p["tf"])
        ev.set_model_source("TracedModel", src, 6, 2, params=params)
        ev.set_batch(B)
        ev.set_path(p["recs"], 0, 1)
        if overlap0:
            ev.set_option("overlap", 0)
        return ev

    ev = traced(p["base"], False)
    ev.set_model_params(rows)
    assert np.array_equal(ev.get_model_params(), rows)
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG"):        # the count given to emi_set_model_source
        ev.set_model_params(rows[:, :4])
    lay = ev.layout
    rng = np.random.default_rng(5)
    lamF, lamC = rng.standard_normal((B, lay.ns, M)), rng.standard_normal((B, lay.np, M))
    dX, dU, dLF, dLC = device_inputs(ev, p["X"], p["U"], lamF, lamC)
    got = {f: evaluate(ev, dX, dU, f) for f in (E.EVAL_ALL, E.EVAL_ALL | E.EVAL_NOJAC)}
    gotH = hessian(ev, dX, dU, dLF, dLC, 0.7)
    for b in range(B):
        ref = traced(rows[b], True)
        for f, g in got.items():
            same_instance(g, evaluate(ref, dX, dU, f), b, f"traced quadrotor flags {f}")
        assert np.array_equal(bits(gotH[b]), bits(hessian(ref, dX, dU, dLF, dLC, 0.7)[b])), b
        ref.close()
        # the traced equations are the built-in quadrotor's: the oracle with that row, at the parity bounds
        o = O.evaluate(E.MODEL_QUADROTOR2D, rows[b], M, (ev.tau, ev.w, ev.D), 0.0, p["tf"], p["X"][b:b + 1], p["U"][b:b + 1], p["recs"][b:b + 1])
        import test_gpu_parity as TP
        TP.check(dict(X=p["X"][b:b + 1]), ev, tuple(a[b:b + 1] for a in got[E.EVAL_ALL]), o)
    ev.close()


# ---- 7. keep record -----------------------------------------------------------------------------------------------------------------
def test_a_new_table_voids_the_kept_invariant_rows(built):
    import torch
    import etol_amd as E
    B, M = B5, 33
    p = problem("quad", B, M)
    first, second = PT.rows_for(p["base"], B, seed=1), PT.rows_for(p["base"], B, seed=2)
    second[0] = 1.1 * p["base"]
    ev = context(p, B, M, p["base"])
    ev.set_model_params(first)
    dX, dU = device_inputs(ev, p["X"], p["U"])
    lay = ev.layout
    RES, VALS, COST = Out(ev, (B, lay.nres, M)), Out(ev, (B, lay.nvals, M)), Out(ev, (B,))
    torch.cuda.synchronize()
    ev.eval_dev(dX, dU, RES.t, VALS.t, COST.t)                  # a full pass
    ev.synchronize()
    kept = VALS.get().copy()
    ev.set_model_params(second)                                 # a new table
    flags = E.EVAL_ALL | E.EVAL_KEEP_INVARIANT                  # ... and a pass that would keep the invariant rows, into the same VALS
    ev._ck(ev.lib.emi_eval_dev(ev.ctx, C.c_void_p(dX.data_ptr()), C.c_void_p(dU.data_ptr()), C.c_void_p(RES.t.data_ptr()),
                               C.c_void_p(VALS.t.data_ptr()), C.c_void_p(COST.t.data_ptr()), flags), "emi_eval_dev")
    ev.synchronize()
    torch.cuda.synchronize()
    again = (RES.get(), VALS.get(), COST.get())
    fresh_ev = context(p, B, M, p["base"])
    fresh_ev.set_model_params(second)
    fresh = evaluate(fresh_ev, dX, dU, E.EVAL_ALL)
    for b in range(B):
        same_instance(again, fresh, b, "second pass after a new table")
    # the invariant rows depend on the parameters (-h / inertia ...): the first table's are not the second's
    mask = E.invariant_rows(E.MODEL_QUADROTOR2D, lay.np)
    inv = np.flatnonzero(np.asarray(mask))
    assert inv.size and not np.array_equal(kept[:, inv], again[1][:, inv])
    # a pass that asks again, nothing changed in between, does keep them: poison the rows and see them stay
    VALS.t[:, inv.tolist()] = 12345.0
    torch.cuda.synchronize()
    ev._ck(ev.lib.emi_eval_dev(ev.ctx, C.c_void_p(dX.data_ptr()), C.c_void_p(dU.data_ptr()), C.c_void_p(RES.t.data_ptr()),
                               C.c_void_p(VALS.t.data_ptr()), C.c_void_p(COST.t.data_ptr()), flags), "emi_eval_dev")
    ev.synchronize()
    torch.cuda.synchronize()
    third = VALS.get()
    assert (third[:, inv] == 12345.0).all()
    var = np.setdiff1d(np.arange(lay.nvals), inv)
    assert np.array_equal(bits(third[:, var]), bits(fresh[1][:, var]))
    # removing the table voids the record as well
    ev.set_model_params(None)
    ev._ck(ev.lib.emi_eval_dev(ev.ctx, C.c_void_p(dX.data_ptr()), C.c_void_p(dU.data_ptr()), C.c_void_p(RES.t.data_ptr()),
                               C.c_void_p(VALS.t.data_ptr()), C.c_void_p(COST.t.data_ptr()), flags), "emi_eval_dev")
    ev.synchronize()
    torch.cuda.synchronize()
    shared = context(p, B, M, p["base"])
    want = evaluate(shared, dX, dU, E.EVAL_ALL)
    assert np.array_equal(bits(VALS.get()), bits(want[1]))
    for e in (ev, fresh_ev, shared):
        e.close()


# ---- 8. lifetime and refusals -------------------------------------------------------------------------------------------------------
def test_lifetime_and_refusals(built):
    import torch
    import etol_amd as E
    lib = E.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    quad = np.array(LR.QUAD_PARAMS)

    def held(ev):
        ns, npar = C.c_int(-1), C.c_int(-1)
        assert lib.emi_get_model_params_batch(ev.ctx, None, C.byref(ns), C.byref(npar)) == 0
        return ns.value, npar.value

    ev = E.Evaluator(0)
    t4 = PT.rows_for(quad, 4)
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 4, 5) == STATE                # no model
    ev.set_mesh(33, 0.0, 4.0)
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 4, 5) == STATE
    ev.set_model(E.MODEL_QUADROTOR2D, quad)
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 4, 5) == STATE                # no batch
    assert b"emi_set_batch" in lib.emi_last_error(ev.ctx)
    assert lib.emi_set_model_params_batch(ev.ctx, None, 0, 0) == STATE
    ev.set_batch(4)
    assert held(ev) == (0, 5)
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 3, 5) == ARG                  # any other nsets
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 1, 5) == ARG
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 4, 4) == ARG                  # not the model's count
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 4, 16) == ARG
    assert lib.emi_set_model_params_batch(ev.ctx, None, 4, 5) == ARG
    assert held(ev) == (0, 5)
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 4, 5) == 0
    assert held(ev) == (4, 5) and np.array_equal(ev.get_model_params(), t4)
    # survives mesh, path table, tracks, waypoint tables, stream
    ev.set_mesh(50, 0.0, 5.0)
    recs = np.zeros((4, 2, 8)); recs[:, :, 0] = E.PATH_DISC; recs[:, :, 1:4] = [3.0, 3.0, 0.25]
    ev.set_path(recs, 0, 1)
    ev.set_tracks(np.zeros((1, 1, 50)), np.zeros((1, 1, 50)))
    ev.set_track_waypoints(np.array([[0.0, 5.0]]), np.array([[1.0, 2.0]]), np.array([[1.0, 1.0]]))
    s = torch.cuda.Stream()
    ev.use_stream(s.cuda_stream)
    assert held(ev) == (4, 5)
    ev.use_stream(None)
    ev.set_batch(4)                                             # the same B
    assert held(ev) == (4, 5) and np.array_equal(ev.get_model_params(), t4)
    # a refused call leaves the table in force
    assert lib.emi_set_model_params_batch(ev.ctx, dp(t4), 5, 5) == ARG and held(ev) == (4, 5)
    # delays: refused on a context with a table, which stays; and the table refused on a context with delays
    assert lib.emi_set_delays(ev.ctx, 0, 1, 0.1) == UNSUPPORTED
    assert b"parameter table" in lib.emi_last_error(ev.ctx)
    assert ev.n_delayed == 0 and held(ev) == (4, 5)
    # dropped by another batch size, a new model, a new model source; removed by nsets = 0
    ev.set_batch(5)
    assert held(ev) == (0, 5) and ev.get_model_params() is None
    t5 = PT.rows_for(quad, 5)
    ev.set_model_params(t5)
    ev.set_model(E.MODEL_QUADROTOR2D, quad)
    assert held(ev) == (0, 5)
    ev.set_model_params(t5)
    ev.set_model_source("TracedModel", traced_quad_source(), 6, 2, params=quad)
    assert held(ev) == (0, 5)
    ev.set_model_params(t5)
    assert lib.emi_set_model_params_batch(ev.ctx, None, 0, 0) == 0 and held(ev) == (0, 5)
    assert lib.emi_set_model_params_batch(ev.ctx, None, 0, 0) == 0                      # nothing to remove: fine
    ev.set_model(E.MODEL_POINTMASS2D, [])
    assert held(ev) == (0, 0)
    assert lib.emi_set_model_params_batch(ev.ctx, None, 5, 0) == 0 and held(ev) == (5, 0)   # a model without parameters: rows of none
    ev.close()
    d = E.Evaluator(0)
    d.set_mesh(33, 0.0, 4.0)
    d.set_model(E.MODEL_QUADROTOR2D, quad)
    d.set_batch(4)
    d.set_delays(0, 1, 0.1)                                     # one free control and its delayed copy
    assert d.n_delayed == 1
    assert lib.emi_set_model_params_batch(d.ctx, dp(t4), 4, 5) == UNSUPPORTED and held(d) == (0, 5)
    assert b"delays" in lib.emi_last_error(d.ctx)
    d.close()


# ---- 9. lock-step -------------------------------------------------------------------------------------------------------------------
def test_lock_step_solve_with_a_row_per_instance(built):
    import torch
    import etol_amd as E
    import ladder_ref as LD
    import refine_ref as RR
    import test_gpu_ladder as TG
    import test_gpu_lockstep as TL
    import test_gpu_restart as TRS
    tf, M = PT.TF, LR.M_NODES
    fx = PT.fixture()["cases"]
    all_insts = LR.instances(tf)
    insts = [all_insts[i] for i in PT.INSTANCES]
    rows = np.array(PT.ROWS)
    opt = dict(tol=PT.TOL)                                      # default rules
    ev = TL.make_ev(tf, insts)
    ev.set_model_params(rows)
    r = TL.solve(ev, tf, insts, opt)
    res = r["res"]
    for b, q in enumerate(res):
        print(f"instance {PT.INSTANCES[b]} row {b}: status {q['status']} iterations {q['iterations']} (fixture {fx[b]['iterations']}) evaluations "
              f"{q['evaluations']} kkt {q['kkt_error']:.2e} viol {q['constr_viol']:.2e} cost {q['cost']:.9f} (fixture {fx[b]['cost']:.9f})")
    assert [q["status"] for q in res] == [LR.CONVERGED] * 3, [q["status"] for q in res]
    # instance b of three reference batches, each with row b as its shared set
    for b in range(3):
        ref = TL.make_ev(tf, insts)
        ref.set_model(1, rows[b])
        ref.set_path(np.stack([LR.records(i["discs"]) for i in insts]), 0, 1)
        ref.set_option("overlap", 0)
        want = TL.solve(ref, tf, insts, opt)
        ref.close()
        assert TL.same_bits(r, want, (b, b)), b
        assert res[b] == want["res"][b], (b, res[b], want["res"][b])
    for b in range(3):
        assert abs(res[b]["cost"] - fx[b]["cost"]) <= 1e-6 * abs(fx[b]["cost"]), (b, res[b]["cost"], fx[b]["cost"])
    mine, theirs = sum(q["iterations"] for q in res), sum(c["iterations"] for c in fx)
    print(f"{mine} iterations over the batch, fixture {theirs}")
    assert mine <= 1.5 * theirs
    # the certificate of the tabled context, at the bound of tests/test_gpu_lockstep.py
    kw = dict(dtype=torch.float64, device=ev.device)
    RES, VALS, COST = torch.zeros((3, TL.NS + TL.NP, M), **kw), torch.zeros((3, ev.layout.nvals, M), **kw), torch.zeros(3, **kw)
    cert = torch.zeros((3, 6), **kw)
    torch.cuda.synchronize()
    ev.eval_dev(r["tX"], r["tU"], RES, VALS, COST)
    ev.kkt_certificate_dev(r["tX"], r["tU"], RES, VALS, r["tLamF"], r["tLamC"], 1.0, r["tzl"], r["tzu"], LR.CL, LR.CU, cert)
    ev.synchronize()
    cert, cost = cert.cpu().numpy(), COST.cpu().numpy()
    for b in range(3):
        print(f"  certificate {b}: stat {cert[b, 0]:.2e} comp {cert[b, 1]:.2e} defect {cert[b, 2]:.2e} viol {cert[b, 3]:.2e}")
        assert cert[b, 2] <= TL.TOL and cert[b, 3] <= TL.TOL
        assert cost[b] == res[b]["cost"]
    ev.close()
    # the ladder (21, 41) keeps the batch whole and only changes the mesh: the table stays, both rungs converge
    linsts = [LD.instances(tf)[i] for i in PT.INSTANCES]
    lev = TG.fresh_ev(tf, linsts)
    lev.set_model_params(rows)
    lr = TG.climb(lev, tf, linsts, LD.LADDER, dict(tol=PT.TOL))
    for g, Mg in enumerate(LD.LADDER):
        print(f"rung {Mg}:", [(q["status"], q["iterations"], round(q["cost"], 6)) for q in lr["res"][g]])
        assert [q["status"] for q in lr["res"][g]] == [LR.CONVERGED] * 3, (Mg, lr["res"][g])
    assert np.array_equal(lev.get_model_params(), rows) and lev.layout.M == LD.LADDER[-1]
    for b in range(3):                                          # the rows were in force on the last rung: the fixture's optima
        assert abs(lr["res"][-1][b]["cost"] - fx[b]["cost"]) <= 1e-6 * abs(fx[b]["cost"]), (b, lr["res"][-1][b]["cost"])
    # the drivers that compact the batch refuse, and say why
    ladder = RR.LADDER[:2]
    linsts2 = [LD.instances(tf, ladder[0])[i] for i in PT.INSTANCES]
    X0 = TRS.starts_of(linsts2, ladder[0])[0]
    X0d = torch.from_numpy(X0.copy()).to(lev.device)
    with pytest.raises(E.EmiError, match="EMI_ERR_UNSUPPORTED") as e1:
        TRS.refine_from(lev, tf, linsts2, ladder, dict(tol=PT.TOL), X0d)
    assert "parameter table" in str(e1.value)
    with pytest.raises(E.EmiError, match="EMI_ERR_UNSUPPORTED") as e2:
        TRS.restart(lev, tf, linsts2, ladder, dict(tol=PT.TOL), [TRS.LINE], X0=X0)
    assert "parameter table" in str(e2.value)
    assert np.array_equal(lev.get_model_params(), rows) and lev.layout.B == 3
    lev.close()
