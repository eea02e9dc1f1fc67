""""sym_res" 3 on the GPU: the direct-operator forms of the one-launch pass ("sym_dop" 2) with a register allocation that admits three
resident workgroups per CU instead of two.  The same kernel code, instantiated once more: RES, VALS and COST are bit for bit those of
"sym_res" 2 and within the parity tests' bounds of the oracle; the flagged pass leaves the invariant rows alone; a staged form is never
granted the third workgroup.  -m gpu

Shapes: quadrotor, 20 keep-outs per instance, one launch ("overlap_mode" 3), 16-deep K tiles, unsplit, outputs poisoned with NaN first.
M = 128 is the shortest pipelined K loop; B = 1 a partial and 17 a ragged instance tile; B = 704 at M = 128 is 44 instance groups x 3 MFMA
workgroups + 704 node workgroups = 836 workgroups, more than the 768 places of three per CU, so CUs really hold three."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import TOL_DEFECT, TOL_NODE, check

pytestmark = pytest.mark.gpu

NP = 20
T0, TF = 0.0, 16.0
KEEP_ALL = 3 | 8            # EMI_EVAL_ALL | EMI_EVAL_KEEP_INVARIANT
SENTINEL = 12345.0
DIRECT = "[De/Do from L2]"


def _quad(M, B, sym_ct):
    import etol_amd as E
    from etol_amd import workloads as W
    ev = E.Evaluator(0)
    ev.set_mesh(M, T0, TF)
    ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS)
    ev.set_batch(B)
    X, U, recs = W.quadrotor_batch(43, B, M, NP)
    ev.set_path(recs, 0, 1)
    for name, v in (("overlap_mode", 3), ("sym_ct", sym_ct), ("sym_bk", 16), ("sym_ksplit", 1), ("sym_dop", 2)):
        ev.set_option(name, v)
    return ev, X, U, recs


def _pass_into_poisoned_buffers(ev, dX, dU, res, dop=2):
    import torch
    ev.set_option("sym_dop", dop)
    ev.set_option("sym_res", res)
    assert ev.plan_residency() == (3 if res == 3 and dop == 2 else 2)
    outs = ev.alloc_outputs()
    for t in outs:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    ev.eval_dev(dX, dU, *outs)
    ev.synchronize()
    torch.cuda.synchronize()
    name = ev.last_defect_kernel
    assert "emi_pass_f64_kernel" in name and "[K tiles of 16]" in name and (DIRECT in name) == (dop == 2), name
    got = [o.cpu().numpy() for o in outs]
    for what, a in zip(("RES", "VALS", "COST"), got):
        assert not np.isnan(a).any(), f"{what}: {int(np.isnan(a).sum())} entries were not written"
    return got


def _assert_same_bits(got, want):
    for what, a, b in zip(("RES", "VALS", "COST"), got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _three_against_two_and_oracle(M, B, sym_ct, sampled=None):
    import torch
    import etol_amd as E
    from etol_amd import workloads as W
    ev, X, U, recs = _quad(M, B, sym_ct)
    dX, dU = torch.from_numpy(X).cuda(), torch.from_numpy(U).cuda()
    two = _pass_into_poisoned_buffers(ev, dX, dU, 2)
    three = _pass_into_poisoned_buffers(ev, dX, dU, 3)
    assert f"<SW={2 if sym_ct == 6 else 1}>" in ev.last_defect_kernel, ev.last_defect_kernel
    mesh = (ev.tau, ev.w, ev.D)
    if sampled is None:
        ref = O.evaluate(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS, M, mesh, T0, TF, X, U, recs)
        check(dict(X=X), ev, three, ref)        # TOL_DEFECT of the row scale on the defect rows, TOL_NODE on node rows and VALS, 1e-13 on COST
    else:
        err = O.sampled_errors(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS, M, mesh, T0, TF, X, U, recs, three, sampled)
        assert err["instances"] == sorted(sampled)
        assert err["defect"] < TOL_DEFECT and err["path"] < TOL_NODE and err["vals"] < TOL_NODE and err["cost"] < 1e-13, err
    _assert_same_bits(three, two)
    ev.close()


@pytest.mark.parametrize("B", [1, 17])
def test_three_resident_workgroups_give_the_bits_of_two(built, B):
    _three_against_two_and_oracle(128, B, 6)            # two states per MFMA workgroup: the benchmarked form


def test_three_resident_workgroups_where_the_grid_exceeds_the_places(built):
    _three_against_two_and_oracle(128, 704, 6, sampled=[0, 15, 16, 352, 703])


def test_three_resident_workgroups_with_one_state_per_workgroup(built):
    _three_against_two_and_oracle(256, 17, 7)           # SW = 1: 128 registers, 12 KB of LDS


def test_three_resident_workgroups_under_keep_invariant(built):
    """A full pass at one point, then a flagged pass at another into the same buffers, both stating three resident workgroups: the
    invariant rows of VALS are not stored again (the KEEP instantiation ran), everything else is bit for bit the staged form's full pass."""
    import torch
    import etol_amd as E
    from etol_amd import workloads as W
    M, B = 128, 17
    ev, X, U, recs = _quad(M, B, 6)
    X2, U2 = W.quadrotor_batch(44, B, M, 0)[:2]
    dX, dU, dX2, dU2 = (torch.from_numpy(a).cuda() for a in (X, U, X2, U2))
    want = _pass_into_poisoned_buffers(ev, dX2, dU2, 2, dop=1)
    mask = E.invariant_rows(E.MODEL_QUADROTOR2D, NP)
    inv = torch.from_numpy(np.flatnonzero(mask)).cuda()
    var = torch.from_numpy(np.flatnonzero(~mask)).cuda()
    ev.set_option("sym_dop", 2)
    ev.set_option("sym_res", 3)
    assert ev.plan_residency() == 3
    outs = ev.alloc_outputs()
    ev.eval_dev(dX, dU, *outs)
    ev.synchronize()
    kept = outs[1][:, inv, :].clone()
    outs[0].fill_(float("nan"))
    outs[2].fill_(float("nan"))
    outs[1][:, var, :] = float("nan")
    outs[1][:, inv, :] = SENTINEL
    torch.cuda.synchronize()
    ev.eval_dev(dX2, dU2, *outs, flags=KEEP_ALL)       # (given explicitly: torch has written to VALS, the evaluator would not add it)
    ev.synchronize()
    torch.cuda.synchronize()
    assert DIRECT in ev.last_defect_kernel, ev.last_defect_kernel
    got = [o.cpu().numpy() for o in outs]
    inv = inv.cpu().numpy()
    assert (got[1][:, inv, :] == SENTINEL).all()
    got[1][:, inv, :] = kept.cpu().numpy()
    for what, a in zip(("RES", "VALS", "COST"), got):
        assert not np.isnan(a).any(), what
    _assert_same_bits(got, want)
    ref = O.evaluate(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS, M, (ev.tau, ev.w, ev.D), T0, TF, X2, U2, recs)
    check(dict(X=X2), ev, got, ref)
    ev.close()


def test_a_staged_form_is_not_granted_the_third_workgroup(built):
    """ "sym_res" 3 with "sym_dop" 1: the plan reports two resident workgroups, the pass runs in the staged form and matches the oracle"""
    import torch
    import etol_amd as E
    from etol_amd import workloads as W
    M, B = 128, 17
    ev, X, U, recs = _quad(M, B, 6)
    dX, dU = torch.from_numpy(X).cuda(), torch.from_numpy(U).cuda()
    got = _pass_into_poisoned_buffers(ev, dX, dU, 3, dop=1)
    assert ev.plan_residency() == 2
    assert ev.last_defect_kernel == "emi_pass_f64_kernel<SW=2> (MFMA + node roles, one launch) [K tiles of 16]", ev.last_defect_kernel
    ref = O.evaluate(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS, M, (ev.tau, ev.w, ev.D), T0, TF, X, U, recs)
    check(dict(X=X), ev, got, ref)
    ev.close()
