"""EMI_EVAL_KEEP_INVARIANT on the GPU: a pass that leaves the model-invariant VALS rows alone must give, in a buffer this
context filled before, bit for bit what a pass that writes everything gives in a fresh one -- and must write everything by
itself wherever the buffer, the mesh, the model or the batch is not what the context's record says.  -m gpu

Shapes: M = 128 is the smallest mesh the one-launch pass takes, M = 24 goes through the general node kernel; B = 17 crosses a
16-instance tile edge; two keep-outs per instance, each instance its own."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

NP = 2
T0, TF = 0.0, 16.0
KEEP_ALL = 3 | 8            # EMI_EVAL_ALL | EMI_EVAL_KEEP_INVARIANT
SENTINEL = 12345.0


def _quad(M, B, node_store=-1, tf=TF, params=None):
    import etol_amd as E
    from etol_amd import workloads as W
    ev = E.Evaluator(0)
    ev.set_mesh(M, T0, tf)
    ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS if params is None else params)
    ev.set_batch(B)
    recs = W.quadrotor_batch(31, B, M, NP)[2]
    ev.set_path(recs, 0, 1)
    if node_store >= 0:
        ev.set_option("node_store", node_store)
    return ev, recs


def _inputs(ev, config, B, M, fixedwing=False):
    """(X, U) as the device sees them: host float64 copies and device tensors in the context's type"""
    import torch
    from etol_amd import workloads as W
    X, U = W.fixedwing_batch(config, B, M) if fixedwing else W.quadrotor_batch(config, B, M, 0)[:2]
    tt = torch.float32 if ev.f32 else torch.float64
    dX, dU = torch.from_numpy(X).to(tt).cuda(), torch.from_numpy(U).to(tt).cuda()
    return dX.cpu().double().numpy(), dU.cpu().double().numpy(), dX, dU


def _nan_outs(ev):
    import torch
    outs = ev.alloc_outputs()
    for t in outs:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    return outs


def _host(ev, outs):
    import torch
    ev.synchronize()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _full_pass_into_fresh_buffers(ev, dX, dU):
    """the reference of every test here: everything written, into buffers nobody has written before"""
    outs = _nan_outs(ev)
    ev.eval_dev(dX, dU, *outs)
    got = _host(ev, outs)
    assert not any(np.isnan(a).any() for a in got)
    return got


def _assert_same_bits(got, want):
    for name, a, b in zip(("RES", "VALS", "COST"), got, want):
        assert not np.isnan(a).any(), f"{name}: {int(np.isnan(a).sum())} entries were not written"
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name


def _check_f64_against_oracle(ev, X, U, recs, got, tf=TF, params=None):
    import etol_amd as E
    from etol_amd import workloads as W
    from test_gpu_parity import check
    p = W.QUAD_PARAMS if params is None else params
    ref = O.evaluate(E.MODEL_QUADROTOR2D, p, X.shape[2], (ev.tau, ev.w, ev.D), T0, tf, X, U, recs)
    check(dict(X=X), ev, got, ref)          # 5e-13 of the row scale on the defect rows, 1e-13 on node rows, VALS entries and COST


def _keep_pass_after_a_full_one(ev, mask, in1, in2):
    """Full pass at point 1; RES, COST and the VARYING rows of VALS to NaN and the INVARIANT rows to a sentinel; flagged pass at point
    2 into the same buffers.  Returns what the buffers hold and what the invariant rows held before the sentinel."""
    import torch
    outs = ev.alloc_outputs()
    ev.eval_dev(in1[2], in1[3], *outs)
    ev.synchronize()
    inv = torch.from_numpy(np.flatnonzero(mask)).cuda()
    var = torch.from_numpy(np.flatnonzero(~mask)).cuda()
    kept = outs[1][:, inv, :].clone()
    outs[0].fill_(float("nan"))
    outs[2].fill_(float("nan"))
    outs[1][:, var, :] = float("nan")
    outs[1][:, inv, :] = SENTINEL
    torch.cuda.synchronize()
    # the flag is given explicitly: the evaluator would not add it by itself after torch writes to VALS, and the library's own
    # record (address, generation) is what is under test here
    ev.eval_dev(in2[2], in2[3], *outs, flags=KEEP_ALL)
    got = _host(ev, outs)
    return got, kept.cpu().numpy(), inv.cpu().numpy()


@pytest.mark.parametrize("M,B,node_store", [(128, B, s) for B in (1, 5, 17) for s in (0, 1, 2, 3)] + [(24, B, -1) for B in (1, 5, 17)])
def test_keep_pass_gives_the_bits_of_a_full_pass(built, M, B, node_store):
    import etol_amd as E
    ev, recs = _quad(M, B, node_store)
    mask = E.invariant_rows(E.MODEL_QUADROTOR2D, NP)
    in1, in2 = _inputs(ev, 32, B, M), _inputs(ev, 33, B, M)
    want = _full_pass_into_fresh_buffers(ev, in2[2], in2[3])
    got, kept, inv = _keep_pass_after_a_full_one(ev, mask, in1, in2)
    assert ("emi_pass_f64_kernel" in ev.last_defect_kernel) == (M == 128), ev.last_defect_kernel
    # the invariant rows were not stored again (every launch form these shapes take has a KEEP instantiation) ...
    assert (got[1][:, inv, :] == SENTINEL).all()
    # ... and what the first pass had left there is what the full pass at the OTHER point writes; with it the buffers are the full pass's
    assert np.array_equal(kept.view(np.uint8), want[1][:, inv, :].copy().view(np.uint8))
    got[1][:, inv, :] = kept
    _assert_same_bits(got, want)
    _check_f64_against_oracle(ev, in2[0], in2[1], recs, got)
    ev.close()


def test_evaluator_adds_the_flag_for_an_untouched_tensor_only(built):
    import torch
    import etol_amd as E
    M, B = 128, 5
    ev, recs = _quad(M, B)
    mask = E.invariant_rows(E.MODEL_QUADROTOR2D, NP)
    row = int(np.flatnonzero(mask)[0])
    in1, in2 = _inputs(ev, 32, B, M), _inputs(ev, 33, B, M)
    want = _full_pass_into_fresh_buffers(ev, in2[2], in2[3])
    outs = ev.alloc_outputs()
    ev.eval_dev(in1[2], in1[3], *outs)
    ev.synchronize()
    # one invariant row overwritten PAST torch (the tensor's version does not move): the next pass keeps it, so the flag was added
    mark = np.full(M, SENTINEL)
    ev._ck(ev.lib.emi_h2d(ev.ctx, C.c_void_p(outs[1][0, row].data_ptr()), C.c_void_p(mark.ctypes.data), mark.nbytes), "emi_h2d")
    ev.eval_dev(in2[2], in2[3], *outs, flags=E.EVAL_ALL | E.EVAL_NOJAC)       # a line-search pass in between changes nothing
    ev.eval_dev(in2[2], in2[3], *outs)
    got = _host(ev, outs)
    assert (got[1][0, row] == SENTINEL).all()
    got[1][0, row] = want[1][0, row]
    _assert_same_bits(got, want)
    # a torch write to VALS: the evaluator passes no flag, the pass writes everything
    outs[1].fill_(float("nan"))
    torch.cuda.synchronize()
    ev.eval_dev(in2[2], in2[3], *outs)
    _assert_same_bits(_host(ev, outs), want)
    ev.close()
    assert ev._kept is None


@pytest.mark.parametrize("what", ["other_buffer", "mesh", "params", "batch", "path", "first_pass_ever"])
def test_flag_is_ignored_where_the_record_does_not_match(built, what):
    """A flagged pass into buffers that hold NaN throughout must still leave complete output."""
    import etol_amd as E
    from etol_amd import workloads as W
    M, B = 128, 5
    ev, recs = _quad(M, B)
    in1, in2 = _inputs(ev, 32, B, M), _inputs(ev, 33, B, M)
    outs = _nan_outs(ev)
    if what != "first_pass_ever":
        ev.eval_dev(in1[2], in1[3], *outs)
        ev.synchronize()
    tf, params = TF, W.QUAD_PARAMS
    if what == "other_buffer":
        outs = _nan_outs(ev)
    elif what == "mesh":
        tf = 9.0
        ev.set_mesh(M, T0, tf)
    elif what == "params":
        params = W.QUAD_PARAMS * np.array([1.5, 1.0, 1.0, 2.0, 1.0])
        ev.set_model(E.MODEL_QUADROTOR2D, params)
        ev.set_path(recs, 0, 1)             # (a new model drops the path rows)
    elif what == "batch":
        ev.set_batch(B)
    elif what == "path":
        recs = recs.copy()
        recs[:, :, 3] *= 1.25
        ev.set_path(recs, 0, 1)
    if what not in ("other_buffer", "first_pass_ever"):
        for t in outs:
            t.fill_(float("nan"))
    ev.eval_dev(in2[2], in2[3], *outs, flags=KEEP_ALL)
    got = _host(ev, outs)
    # the same problem set up from nothing, everything written
    ev2, _ = _quad(M, B, tf=tf, params=params)
    ev2.set_path(recs, 0, 1)
    want = _full_pass_into_fresh_buffers(ev2, in2[2], in2[3])
    _assert_same_bits(got, want)
    _check_f64_against_oracle(ev, in2[0], in2[1], recs, got, tf=tf, params=params)
    ev.close()
    ev2.close()


@pytest.mark.parametrize("M,B,one_launch", [(128, 3, False), (512, 64, True)])
def test_keep_pass_of_an_fp32_context(built, M, B, one_launch):
    """FixedWing12 in fp32: the node kernel behind which the MFMA kernel runs (the default), and the pass as one launch (MFMA-role and
    node-role workgroups in one grid; it needs whole tiles in every XCD, hence the larger shape).  Bits of the full pass; the
    oracle to 2e-6 of the row scale (fp32 rounding, as tests/test_gpu_parity.py has it)."""
    import etol_amd as E
    from etol_amd import workloads as W
    ev = E.Evaluator(0, f32=True)
    ev.set_mesh(M, 0.0, 20.0)
    ev.set_model(E.MODEL_FIXEDWING12, W.FW_PARAMS)
    ev.set_batch(B)
    if one_launch:
        ev.set_option("overlap_mode", 3)
    mask = E.invariant_rows(E.MODEL_FIXEDWING12, 0)
    in1, in2 = _inputs(ev, 34, B, M, fixedwing=True), _inputs(ev, 35, B, M, fixedwing=True)
    want = _full_pass_into_fresh_buffers(ev, in2[2], in2[3])
    got, kept, inv = _keep_pass_after_a_full_one(ev, mask, in1, in2)
    assert ("emi_pass_f32_kernel" in ev.last_defect_kernel) == one_launch, ev.last_defect_kernel
    assert (got[1][:, inv, :] == SENTINEL).all()
    assert np.array_equal(kept.view(np.uint8), want[1][:, inv, :].copy().view(np.uint8))
    got[1][:, inv, :] = kept
    _assert_same_bits(got, want)
    sub = slice(0, min(B, 3))
    X, U = in2[0][sub], in2[1][sub]
    rRES, rVALS, rCOST = O.evaluate(E.MODEL_FIXEDWING12, W.FW_PARAMS, M, (ev.tau, ev.w, ev.D), 0.0, 20.0, X, U)
    RES, VALS, COST = (a[sub].astype(np.float64) for a in got)
    scale = np.einsum("kj,bij->bik", np.abs(ev.D), np.abs(X)) + np.abs(rRES) + 1.0
    assert (np.abs(RES - rRES) / scale).max() < 2e-6
    for e in range(VALS.shape[1]):
        assert np.abs(VALS[:, e] - rVALS[:, e]).max() / (np.abs(rVALS[:, e]).max() + 1.0) < 2e-6, e
    assert np.abs(COST - rCOST).max() / np.abs(rCOST).max() < 2e-6
    ev.close()


def test_traced_model_with_the_flag_writes_everything(built):
    """A model compiled at run time declares no invariant rows: it takes the flag and stores every row."""
    import etol_amd as E
    from test_gpu_traced import traced_source
    M, B = 128, 5
    ev = E.Evaluator(0)
    ev.set_mesh(M, T0, TF)
    ev.set_model_source("TracedModel", traced_source(0), 6, 2)
    ev.set_batch(B)
    from etol_amd import workloads as W
    recs = W.quadrotor_batch(31, B, M, NP)[2]
    ev.set_path(recs, 0, 1)
    in1, in2 = _inputs(ev, 32, B, M), _inputs(ev, 33, B, M)
    want = _full_pass_into_fresh_buffers(ev, in2[2], in2[3])
    outs = ev.alloc_outputs()
    ev.eval_dev(in1[2], in1[3], *outs)
    ev.synchronize()
    for t in outs:
        t.fill_(float("nan"))
    ev.eval_dev(in2[2], in2[3], *outs, flags=KEEP_ALL)
    got = _host(ev, outs)
    _assert_same_bits(got, want)
    _check_f64_against_oracle(ev, in2[0], in2[1], recs, got)
    ev.close()
