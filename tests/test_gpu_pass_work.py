"""The one-launch pass on the GPU with its work table (etol_amd/csrc/emi_pass_work.hpp): every workgroup of emi_pass_f64_kernel takes its
role and its tile from an entry the host built, instead of working pass_role_of and ring_tile_of out for itself.  -m gpu

Every case writes RES, VALS and COST into NaN-filled buffers twice: nothing is left unwritten, the two calls give the same bits, the
second call -- an unchanged context -- uploads no table, and the results are within the parity tests' bounds of the CPU oracle.

Shapes: quadrotor with 20 keep-outs per instance at M = 128 (one column tile, the shortest pipelined K loop): B = 1 a partial instance
tile, 3, 17 a ragged one, 80 the first size with a rounded-up role count on some XCD, 160 more workgroups than places at two per CU, 704
more than at three; M = 256 at B = 33 for more than one column tile.  Then the options that change what the entries hold: column
partitions, the grouped order (B = 256: whole super-blocks on every XCD), the block orders, K slices (a tile's entries carry the slice),
K halves (a node workgroup of 512 threads takes two chunks of one entry), both operand sources, three resident workgroups; the flagged
pass; the 2-state point-mass model."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import TOL_DEFECT, TOL_NODE, check

pytestmark = pytest.mark.gpu

NP = 20
T0, TF = 0.0, 16.0
KEEP_ALL = 3 | 8            # EMI_EVAL_ALL | EMI_EVAL_KEEP_INVARIANT
SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def _quad_inputs(M, B):
    from etol_amd import workloads as W
    X, U, recs = W.quadrotor_batch(47, B, M, NP)
    for a in (X, U, recs):
        a.setflags(write=False)
    return X, U, recs


def _quad(M, B, **options):
    import etol_amd as E
    from etol_amd import workloads as W
    ev = E.Evaluator(0)
    ev.set_mesh(M, T0, TF)
    ev.set_model(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS)
    ev.set_batch(B)
    X, U, recs = _quad_inputs(M, B)
    ev.set_path(recs, 0, 1)
    ev.set_option("overlap_mode", 3)
    for name, v in options.items():
        ev.set_option(name, v)
    return ev, X, U, recs


def _pass_into_poisoned_buffers(ev, dX, dU, outs=None, flags=None):
    import torch
    outs = outs if outs is not None else ev.alloc_outputs()
    for t in outs:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    if flags is None:
        ev.eval_dev(dX, dU, *outs)
    else:
        ev.eval_dev(dX, dU, *outs, flags=flags)
    ev.synchronize()
    torch.cuda.synchronize()
    assert "emi_pass_f64_kernel" in ev.last_defect_kernel, ev.last_defect_kernel
    got = [o.cpu().numpy() for o in outs]
    for what, a in zip(("RES", "VALS", "COST"), got):
        assert not np.isnan(a).any(), f"{what}: {int(np.isnan(a).sum())} entries were not written"
    return got, outs


def _assert_same_bits(got, want):
    for what, a, b in zip(("RES", "VALS", "COST"), got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _twice(ev, X, U, tables=1):
    """two passes into NaN-filled buffers: the same bits, and the second uploads nothing"""
    import torch
    dX, dU = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(U)).cuda()
    before = ev.pass_work_uploads[0]
    first, outs = _pass_into_poisoned_buffers(ev, dX, dU)
    assert ev.pass_work_uploads[0] == before + tables, ev.pass_work_uploads
    second, _ = _pass_into_poisoned_buffers(ev, dX, dU, outs)
    assert ev.pass_work_uploads[0] == before + tables, "the second call on an unchanged context uploaded a table"
    _assert_same_bits(second, first)
    return second


def _against_oracle(ev, M, X, U, recs, got, sampled=None):
    import etol_amd as E
    from etol_amd import workloads as W
    mesh = (ev.tau, ev.w, ev.D)
    if sampled is None:
        ref = O.evaluate(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS, M, mesh, T0, TF, X, U, recs)
        check(dict(X=X), ev, got, ref)          # TOL_DEFECT of the row scale on the defect rows, TOL_NODE on node rows and VALS, 1e-13 on COST
    else:
        err = O.sampled_errors(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS, M, mesh, T0, TF, X, U, recs, got, sampled)
        assert err["instances"] == sorted(sampled)
        assert err["defect"] < TOL_DEFECT and err["path"] < TOL_NODE and err["vals"] < TOL_NODE and err["cost"] < 1e-13, err


def _sample(B):
    return None if B <= 80 else sorted({0, 15, 16, B // 2, B - 17, B - 1})


@pytest.mark.parametrize("B", [1, 3, 17, 80, 160, 704])
def test_the_default_plan_at_128_nodes(built, B):
    ev, X, U, recs = _quad(128, B)
    got = _twice(ev, X, U)
    _against_oracle(ev, 128, X, U, recs, got, _sample(B))
    ev.close()


def test_two_column_tiles(built):
    ev, X, U, recs = _quad(256, 33)
    got = _twice(ev, X, U)
    _against_oracle(ev, 256, X, U, recs, got)
    ev.close()


# what the plan must report for the option to have taken hold: (M, B, options, {plan field: value}, text in the kernel's name)
OPTIONS = {
    "cpart_0": (256, 64, dict(sym_ct=6, sym_cpart=-1), dict(cpart=0), "<SW=2>"),
    "cpart_2": (256, 64, dict(sym_ct=6, sym_cpart=2), dict(cpart=2), "<SW=2>"),
    "grouped": (128, 256, dict(sym_ct=6, sym_gblk=2, sym_ksplit=1), dict(cpart=-2), "<SW=2>"),
    "order_1": (128, 80, dict(pass_order=1), dict(block_order=1), ""),
    "order_110": (128, 80, dict(pass_order=110), dict(block_order=110), ""),
    "order_150": (128, 80, dict(pass_order=150), dict(block_order=150), ""),
    "ksplit_2": (128, 17, dict(sym_ct=7, sym_ksplit=2), dict(ksplit=2), "2 K slices per tile"),
    "ksplit_4": (128, 17, dict(sym_ct=6, sym_ksplit=4), dict(ksplit=4), "4 K slices per tile"),
    "k_halves": (128, 17, dict(sym_ct=6, sym_ksplit=1, sym_hs=2), dict(k_halves=2), "[K range in two halves per workgroup]"),
    "k_halves_odd_chunks": (128, 3, dict(sym_ct=7, sym_ksplit=1, sym_hs=2, sym_bk=16), dict(k_halves=2), "[K range in two halves per workgroup]"),
    "dop_1": (128, 17, dict(sym_ct=6, sym_ksplit=1, sym_bk=16, sym_dop=1), dict(k_tile=16), "[K tiles of 16]"),
    "dop_2": (128, 17, dict(sym_ct=6, sym_ksplit=1, sym_bk=16, sym_dop=2), dict(k_tile=16), "[De/Do from L2]"),
    "res_3": (128, 160, dict(sym_ct=6, sym_ksplit=1, sym_bk=16, sym_dop=2, sym_res=3), dict(k_tile=16), "[De/Do from L2]"),
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_the_options_that_change_the_entries(built, name):
    M, B, options, plan, text = OPTIONS[name]
    ev, X, U, recs = _quad(M, B, **options)
    p = ev.plan()
    assert p["one_launch"] == 1 and all(p[k] == v for k, v in plan.items()), (name, p)
    if name == "res_3":
        assert ev.plan_residency() == 3
    got = _twice(ev, X, U)
    assert text in ev.last_defect_kernel, ev.last_defect_kernel
    _against_oracle(ev, M, X, U, recs, got, _sample(B))
    ev.close()


def test_a_new_batch_builds_a_new_table(built):
    """set_batch, then a batch of another size: one more table; back to the first size: its table is still there"""
    ev, X, U, recs = _quad(128, 17)
    first = _twice(ev, X, U)
    assert ev.pass_work_uploads == (1, 1)
    ev.set_batch(3)
    X3, U3, recs3 = _quad_inputs(128, 3)
    ev.set_path(recs3, 0, 1)
    got = _twice(ev, X3, U3)
    assert ev.pass_work_uploads == (2, 2)
    _against_oracle(ev, 128, X3, U3, recs3, got)
    ev.set_batch(17)
    ev.set_path(recs, 0, 1)
    again = _twice(ev, X, U, tables=0)
    assert ev.pass_work_uploads == (2, 2)
    _assert_same_bits(again, first)
    # more launches than the context has room for tables: the least recently used one gives way, the results stay right
    for B in (1, 2, 4, 5, 6, 7, 8, 9):
        ev.set_batch(B)
        ev.set_path(_quad_inputs(128, B)[2], 0, 1)
        _twice(ev, *_quad_inputs(128, B)[:2])
    assert ev.pass_work_uploads == (10, 8)
    ev.set_batch(17)
    ev.set_path(recs, 0, 1)
    _assert_same_bits(_twice(ev, X, U), first)
    ev.close()


def test_the_flagged_pass(built):
    """A full pass at one point, then a flagged pass (EMI_EVAL_KEEP_INVARIANT) at another into the same buffers: the invariant rows of
    VALS are not stored again, everything else is bit for bit a full pass at that point; the flagged pass reads the table of the full one."""
    import torch
    import etol_amd as E
    from etol_amd import workloads as W
    M, B = 128, 17
    ev, X, U, recs = _quad(M, B)
    X2, U2 = W.quadrotor_batch(48, B, M, 0)[:2]
    dX, dU, dX2, dU2 = (torch.from_numpy(np.array(a)).cuda() for a in (X, U, X2, U2))
    want, _ = _pass_into_poisoned_buffers(ev, dX2, dU2)
    mask = E.invariant_rows(E.MODEL_QUADROTOR2D, NP)
    inv = torch.from_numpy(np.flatnonzero(mask)).cuda()
    var = torch.from_numpy(np.flatnonzero(~mask)).cuda()
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
    assert ev.pass_work_uploads == (1, 1)
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


def test_the_point_mass_model(built):
    import etol_amd as E
    from etol_amd import workloads as W
    M, B, nobs = 128, 33, 2
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, 12.0)
    ev.set_model(E.MODEL_POINTMASS2D, [])
    ev.set_batch(B)
    X, U = W.pointmass_batch(9, B, M)
    recs = np.zeros((B, nobs, 8))
    recs[:, :, 0] = E.PATH_DISC
    recs[:, :, 1:4] = np.random.default_rng(2).uniform(0.5, 3, (B, nobs, 3))
    ev.set_path(recs, 0, 1)
    ev.set_option("overlap_mode", 3)
    got = _twice(ev, X, U)
    ref = O.evaluate(E.MODEL_POINTMASS2D, [], M, (ev.tau, ev.w, ev.D), 0.0, 12.0, X, U, recs)
    check(dict(X=X), ev, got, ref)
    ev.close()
