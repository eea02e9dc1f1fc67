""""sym_dop" 2 on the GPU: the MFMA role of the one-launch pass takes its De / Do fragments straight from L2 (a fragment-order copy of
the panels, built at emi_set_mesh) instead of through the operand ring, which then holds the x rows only.  Same operands, same MFMAs
in the same order: against the oracle at the parity tests' tolerances, and RES, VALS and COST bit for bit those of the staged form
("sym_dop" 1).  -m gpu

Shapes: quadrotor, 20 keep-outs per instance.  M = 128 is one column tile and four 16-deep K tiles, the shortest loop the pipelined
form allows (prologue, one pair of steps, the tail step, the last multiply); M = 256 has two column tiles, so the panel base moves
with the tile.  B = 1 is a partial instance tile, 17 and 33 put tiles on both sides of a tile edge."""
import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import check

pytestmark = pytest.mark.gpu

NP = 20
T0, TF = 0.0, 16.0
KEEP_ALL = 3 | 8            # EMI_EVAL_ALL | EMI_EVAL_KEEP_INVARIANT
SENTINEL = 12345.0
SUFFIX = "[De/Do from L2]"


def _quad(M, B, sym_ct):
    import etol_amd as E
    from etol_amd import workloads as W
    ev = E.Evaluator(0)
    ev.set_mesh(M, T0, TF)
    ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS)
    ev.set_batch(B)
    X, U, recs = W.quadrotor_batch(41, B, M, NP)
    ev.set_path(recs, 0, 1)
    for name, v in (("overlap_mode", 3), ("sym_ct", sym_ct), ("sym_bk", 16), ("sym_ksplit", 1)):
        ev.set_option(name, v)
    return ev, X, U, recs


def _pass_into_poisoned_buffers(ev, dX, dU, dop):
    import torch
    ev.set_option("sym_dop", dop)
    outs = ev.alloc_outputs()
    for t in outs:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    ev.eval_dev(dX, dU, *outs)
    ev.synchronize()
    torch.cuda.synchronize()
    name = ev.last_defect_kernel
    assert "emi_pass_f64_kernel" in name and "[K tiles of 16]" in name and (SUFFIX in name) == (dop == 2), name
    got = [o.cpu().numpy() for o in outs]
    for what, a in zip(("RES", "VALS", "COST"), got):
        assert not np.isnan(a).any(), f"{what}: {int(np.isnan(a).sum())} entries were not written"
    return got


def _assert_same_bits(got, want):
    for what, a, b in zip(("RES", "VALS", "COST"), got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _direct_against_staged_and_oracle(M, B, sym_ct):
    import torch
    import etol_amd as E
    from etol_amd import workloads as W
    ev, X, U, recs = _quad(M, B, sym_ct)
    dX, dU = torch.from_numpy(X).cuda(), torch.from_numpy(U).cuda()
    staged = _pass_into_poisoned_buffers(ev, dX, dU, 1)
    direct = _pass_into_poisoned_buffers(ev, dX, dU, 2)
    assert f"<SW={2 if sym_ct == 6 else 1}>" in ev.last_defect_kernel, ev.last_defect_kernel
    ref = O.evaluate(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS, M, (ev.tau, ev.w, ev.D), T0, TF, X, U, recs)
    check(dict(X=X), ev, direct, ref)       # TOL_DEFECT of the row scale on the defect rows, TOL_NODE on node rows and VALS, 1e-13 on COST
    _assert_same_bits(direct, staged)
    ev.close()


@pytest.mark.parametrize("M", [128, 256])
@pytest.mark.parametrize("B", [1, 17, 33])
def test_direct_operator_form_gives_the_bits_of_the_staged_form(built, M, B):
    _direct_against_staged_and_oracle(M, B, 6)          # two states per MFMA workgroup: the benchmarked form


def test_direct_operator_form_with_one_state_per_workgroup(built):
    _direct_against_staged_and_oracle(256, 17, 7)       # SW = 1: one DMA piece per wave and tile, eight MFMAs


def test_direct_operator_form_under_keep_invariant(built):
    """A full pass at one point, then a flagged pass at another into the same buffers, both in the direct form: the invariant rows of
    VALS are not stored again (the KEEP instantiation ran), everything else is bit for bit the staged form's full pass."""
    import torch
    import etol_amd as E
    from etol_amd import workloads as W
    M, B = 128, 17
    ev, X, U, recs = _quad(M, B, 6)
    X2, U2 = W.quadrotor_batch(42, B, M, 0)[:2]
    dX, dU, dX2, dU2 = (torch.from_numpy(a).cuda() for a in (X, U, X2, U2))
    want = _pass_into_poisoned_buffers(ev, dX2, dU2, 1)
    mask = E.invariant_rows(E.MODEL_QUADROTOR2D, NP)
    inv = torch.from_numpy(np.flatnonzero(mask)).cuda()
    var = torch.from_numpy(np.flatnonzero(~mask)).cuda()
    ev.set_option("sym_dop", 2)
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
    assert SUFFIX in ev.last_defect_kernel, ev.last_defect_kernel
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
