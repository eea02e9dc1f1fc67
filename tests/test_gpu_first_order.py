"""The first-order outputs of an fp64 evaluation pass against the exact reference of tests/first_ref.py, element by element.  -m gpu

Nodes-only passes (EMI_EVAL_NODES: RES holds -h f by itself): every element of RES, VALS and COST within K_kind u A of the
reference, u = 2^-53, A the magnitude sum of what went into the element, exactly zero where A == 0; the constants are derived in
first_ref.py from the host-compiled model structs and from counted roundings, never from device output.  Full passes (every row of
the pass-form table, every stand-alone MFMA defect kernel, the sequential pair) run on the long horizon first_ref.HORIZON, where
h f outweighs the operator's rounding, and their defect rows are held to first_ref's full-pass bound; their other rows as above.
The inputs are fixture points (tests/golden/first_order_terms.npz, the points of hessian_terms.npz) laid out as [B][M] by index;
the mesh is the oracle's for the nodes-only passes and emi_lgl's for the full ones (the even/odd kernels take a D that is
centro-antisymmetric to the bit), and the reference is built on the mesh the context holds; every output buffer holds NaN before
the pass, and every check prints its worst ratio and where it is (pytest -s).

Out of scope here: the fp32 context (test_gpu_f32.py), contexts with delays (test_gpu_delay_values.py holds the delayed values
elementwise and ties the passes bit for bit to contexts without delays), the TABLED instantiations (test_gpu_param_table.py
ties them bit for bit to untabled contexts).
"""
import numpy as np
import pytest

import first_ref as FR
import hess_ref as HR
import oracle_lib as O
from etol_amd import workloads as W
from test_gpu_parity import _pass_form_rows
from test_gpu_traced import traced_source

pytestmark = pytest.mark.gpu

PARAMS = {0: [], 1: W.QUAD_PARAMS, 2: W.FW_PARAMS}
NAMES = {0: "point mass", 1: "quadrotor", 2: "fixed wing"}
T0, TF = 0.5, 9.0                       # h = 4.25 (the nodes-only cases)
_OPEN = []
_MESH = {}
_REF = {}


@pytest.fixture(autouse=True)
def close_evaluators():
    yield
    while _OPEN:
        _OPEN.pop().close()


def mesh(M):
    if M not in _MESH:
        _MESH[M] = O.lgl(M)
    return _MESH[M]


def make_ev(model, M, B, t0=T0, tf=TF, recs=None, tracks=None, px=0, py=1, maximize=False, traced=False, mesh_of=mesh):
    import etol_amd as E
    ev = E.Evaluator(0)
    _OPEN.append(ev)
    ev.set_mesh(M, t0, tf, mesh=mesh_of(M))
    if traced:
        assert model == 1
        ev.set_model_source("TracedModel", traced_source(0), 6, 2, maximize=maximize)
    else:
        ev.set_model(model, PARAMS[model], maximize=maximize)
    ev.set_batch(B)
    if tracks is not None:
        ev.set_tracks(*tracks)
    if recs is not None:
        ev.set_path(recs, px, py)
    return ev


def device_inputs(ev, model, idx):
    import torch
    X, U = HR.points(model, idx)
    return torch.from_numpy(X).to(ev.device), torch.from_numpy(U).to(ev.device)


def poisoned_pass(ev, dX, dU, outs, flags, poison=(True, True, True)):
    """one pass into outs, the chosen ones NaN-filled first -> numpy (RES, VALS, COST)"""
    import torch
    for t, p in zip(outs, poison):
        if p:
            t.fill_(float("nan"))
    torch.cuda.synchronize()             # the fills and the copies run on torch's stream, the evaluator launches on its own
    ev.eval_dev(dX, dU, *outs, flags=flags)
    ev.synchronize()
    return [t.cpu().numpy() for t in outs]


def edge_heavy(model, B, M):
    """[B][M] fixture rows ending with the model's last row: small meshes get the edge points, large ones every point"""
    n = HR.npoints(model)
    return HR.cycle(model, B, M, start=(n - B * M) % n)


def nodes_case(what, model, idx, recs=None, tracks=None, px=0, py=1, maximize=False, traced=False, nojac=True):
    """A nodes-only pass, and the values-only one, of one context against the reference -> (evaluator, inputs, outputs, r)"""
    import etol_amd as E
    idx = np.asarray(idx)
    B, M = idx.shape
    ev = make_ev(model, M, B, T0, TF, recs, tracks, px, py, maximize, traced)
    dX, dU = device_inputs(ev, model, idx)
    outs = ev.alloc_outputs()
    r = FR.reference(model, idx, mesh(M), T0, TF, maximize, recs, tracks, px, py)
    got = poisoned_pass(ev, dX, dU, outs, E.EVAL_NODES)
    FR.check_pass(what, got, r)
    if nojac:
        got = poisoned_pass(ev, dX, dU, outs, E.EVAL_NODES | E.EVAL_NOJAC)
        FR.check_pass(f"{what}, values only", got, r, vals=False)
    return ev, (dX, dU), outs, r


# ---- 4a: the node kernel alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (2, 257, 514))
@pytest.mark.parametrize("model", (0, 1, 2))
def test_node_kernel_models_and_meshes(built, model, M):
    """The three built-in models, three instances.  M = 2: the smallest mesh; 257: one node per thread, a full 256-thread block and one
    live thread in a second; 514: two nodes per thread, a full block and one pack in a second.  With and without the Jacobian."""
    _, _, _, r = nodes_case(f"{NAMES[model]} M={M}", model, edge_heavy(model, 3, M))
    assert np.abs(r.RES).max() > 0 and (r.A_VALS == 0).any() and (r.A_VALS > 0).any()


@pytest.mark.parametrize("M", (33, 514))
def test_traced_quadrotor_twin(built, M):
    """The quadrotor as a run-time compiled model (generated f, jac, cost, grad), held to the bound of the built-in one, with the
    mixed record tables."""
    import etol_amd as E
    ev, _, _, _ = nodes_case(f"traced quadrotor M={M}", 1, edge_heavy(1, 3, M), HR.mixed_tables(), HR.track_centres(M), traced=True)
    assert ev.layout.model == E.MODEL_SOURCE


def test_maximize(built):
    """sgn = -1: COST and the cost gradient change sign, nothing else does."""
    idx = edge_heavy(1, 3, 33)
    _, _, omax, rmax = nodes_case("quadrotor, maximize", 1, idx, maximize=True, nojac=False)
    assert (rmax.COST < 0).all()
    vmax, cmax = omax[1].cpu().numpy().copy(), omax[2].cpu().numpy().copy()
    _, _, omin, rmin = nodes_case("quadrotor, minimize", 1, idx, nojac=False)
    vmin, cmin = omin[1].cpu().numpy(), omin[2].cpu().numpy()
    assert (rmin.COST > 0).all() and np.array_equal(cmax, -cmin)
    assert np.array_equal(vmax[:, :48], vmin[:, :48]) and np.array_equal(vmax[:, 48:], -vmin[:, 48:]) and (np.abs(vmin[:, 54:]) > 0).any()


@pytest.mark.parametrize("model,px,py,M", [(1, 0, 1, 33), (1, 4, 3, 34), (2, 2, 5, 34), (2, 7, 1, 33)])
def test_keep_out_rows_and_partials(built, model, px, py, M):
    """Five rows per instance -- ellipses, discs and a track, in another order in each instance's table -- on path states in both
    orders and, for the fixed wing, away from (0, 1); one node per thread (M = 33) and two (M = 34).  A wrong set, row stride or
    state puts another record's value into the element."""
    recs, tracks = HR.mixed_tables(), HR.track_centres(M)
    idx = edge_heavy(model, 3, M)
    _, _, outs, r = nodes_case(f"{NAMES[model]} keep-outs on ({px}, {py}) M={M}", model, idx, recs, tracks, px, py)
    ns = r.ns
    assert (np.abs(r.RES[:, ns:]) > 0).all()
    # the tables and the states differ where it matters: the reference with the tables rotated, or the states swapped, is far outside
    other = FR.reference(model, idx, mesh(M), T0, TF, False, recs[[1, 2, 0]], tracks, px, py)
    swapped = FR.reference(model, idx, mesh(M), T0, TF, False, recs, tracks, py, px)
    for wrong in (other, swapped):
        assert not FR.within(outs[0].cpu().numpy()[:, ns:], wrong.RES[:, ns:], wrong.A_RES[:, ns:], 1e6).all(axis=(1, 2)).any()


def test_track_set_per_instance(built):
    """Every instance with its own track centres."""
    M, B = 33, 3
    s = np.linspace(0.0, 1.0, M)
    tracks = (np.stack([(1.5 + b + 0.5 * s)[None] for b in range(B)]), np.stack([(2.0 - 0.25 * (1 + b) * s)[None] for b in range(B)]))
    idx = edge_heavy(1, B, M)
    _, _, outs, r = nodes_case("quadrotor, a track set per instance", 1, idx, HR.mixed_tables(), tracks)
    shared = FR.reference(1, idx, mesh(M), T0, TF, False, HR.mixed_tables(), (tracks[0][:1], tracks[1][:1]))
    rows = 6 + np.array([2, 0, 3])            # the track row of each instance's table
    got = outs[0].cpu().numpy()
    for b in (1, 2):
        assert not FR.within(got[b, rows[b]], shared.RES[b, rows[b]], shared.A_RES[b, rows[b]], 1e6).any()


@pytest.mark.parametrize("model", (1, 2))
def test_pass_that_keeps_the_invariant_rows(built, model):
    """A nodes-only Jacobian pass at one set of points, then one at another into the same, untouched VALS (the evaluator then adds
    EMI_EVAL_KEEP_INVARIANT): the varying rows are held to the same bound at the new points, and the kept rows -- whose reference
    does not depend on the point -- still are what the reference says."""
    import etol_amd as E
    M, B = 34, 3
    recs, tracks = HR.mixed_tables(), HR.track_centres(M)
    ev, _, outs, _ = nodes_case(f"{NAMES[model]}, first pass", model, edge_heavy(model, B, M), recs, tracks, nojac=False)
    idx = HR.cycle(model, B, M, start=5)
    dX, dU = device_inputs(ev, model, idx)
    assert outs[1] is ev._kept and outs[1]._version == ev._kept_version
    got = poisoned_pass(ev, dX, dU, outs, E.EVAL_NODES, poison=(True, False, True))
    r = FR.reference(model, idx, mesh(M), T0, TF, False, recs, tracks)
    keep = E.invariant_rows(model, 5)
    assert keep.any() and not keep.all()
    FR.check_pass(f"{NAMES[model]}, pass that keeps the invariant rows: the varying rows", got, r, keep=keep)
    FR.check_pass(f"{NAMES[model]}, pass that keeps the invariant rows: every row", got, r)


# ---- 4b: f inside the MFMA epilogues, on the long horizon ------------------------------------------------------------------------------
def library_mesh(M):
    """emi_lgl's mesh: its D is centro-antisymmetric to the bit, which the even/odd kernels require (the oracle's need not be)"""
    import etol_amd as E
    if ("emi", M) not in _MESH:
        _MESH["emi", M] = E.lgl(M)
    return _MESH["emi", M]


def horizon_case(model, M, B, accumulated=False):
    """-> (idx, recs, tracks, reference of the full pass): shared by the cases of one shape, never changed"""
    assert (model, M, B) in (FR.SEQUENTIAL_SHAPES if accumulated else FR.HORIZON_SHAPES)      # the CPU test asserts their horizon condition
    key = (model, M, B, accumulated)
    if key not in _REF:
        idx = FR.horizon_points(model, B, M)
        recs, tracks = HR.mixed_tables()[0], HR.track_centres(M)
        r = FR.reference(model, idx, library_mesh(M), *FR.HORIZON, False, recs, tracks, full=True, accumulated=accumulated)
        assert np.percentile(FR.admitted(r), 99) <= 1e-12            # ... and here on the mesh used
        _REF[key] = (idx, recs, tracks, r)
    return _REF[key]


def horizon_ev(model, M, B, accumulated=False):
    idx, recs, tracks, r = horizon_case(model, M, B, accumulated)
    ev = make_ev(model, M, B, *FR.HORIZON, recs, tracks, mesh_of=library_mesh)
    return ev, device_inputs(ev, model, idx), ev.alloc_outputs(), r


def full_pass(what, ev, dXU, outs, r):
    import etol_amd as E
    got = poisoned_pass(ev, *dXU, outs, E.EVAL_ALL)
    FR.check_defect(what, got[0], r)
    FR.check_pass(what, got, r, defect_rows=False)
    return got


@pytest.mark.parametrize("model", (0, 1))
def test_every_row_of_the_pass_form_table(built, model):
    """Every instantiation of emi_pass_f64_kernel the library holds for the point mass and the quadrotor, reached through options as
    tests/test_gpu_parity.py reaches them -- 17 instances on 128 nodes (256 for the rows with two column sub-tiles), 5 instances
    with two K slices for the rows that allow slices -- on the long horizon: the defect rows against the full-pass bound, every
    other output elementwise.  Every row is run and reported before the test fails for any of them."""
    ns = HR.NS[model]
    applies = dict(NS=True, **{"1": True, "2": ns > 2 and ns % 2 == 0, "3": ns > 3 and ns % 3 == 0})
    rows = [r for r in _pass_form_rows() if applies[r["cls"]]]
    assert len(rows) == (7 if ns == 2 else 16)
    reached, outside = 0, []
    for M in (128, 256):
        mine = [r for r in rows if (r["ct"] == 2) == (M == 256)]
        for B, ks in ((17, 1), (5, 2)):
            todo = [r for r in mine if ks == 1 or r["slices"]]
            if not todo:
                continue
            ev, dXU, outs, ref = horizon_ev(model, M, B)
            ev.set_option("overlap_mode", 3)
            for r in todo:
                sw = ns if r["cls"] == "NS" else int(r["cls"])
                for opt, v in (("sym_ct", dict(NS=5, **{"2": 6, "3": 8, "1": 7})[r["cls"]]), ("sym_ksplit", ks), ("sym_nst", r["nst"]), ("sym_bk", r["bk"]),
                               ("sym_ctc", r["ct"]), ("sym_hs", r["hs"]), ("sym_dop", 2 if r["dop"] else 1)):
                    ev.set_option(opt, v)
                plan = ev.plan(B)
                want = dict(one_launch=1, sw=sw, ksplit=ks, ring_stages=r["nst"], k_tile=r["bk"], column_tiles=r["ct"], k_halves=r["hs"], piece=0)
                assert {k: plan[k] for k in want} == want, (r, B, plan)
                try:
                    full_pass(f"{NAMES[model]} ({M}, {B}) SW={sw} nst={r['nst']} bk={r['bk']} ct={r['ct']} hs={r['hs']} dop={r['dop']} ks={ks}", ev, dXU, outs, ref)
                except AssertionError as e:
                    outside.append((r, B, str(e)[:200]))
                assert f"emi_pass_f64_kernel<SW={sw}>" in ev.last_defect_kernel and "one launch" in ev.last_defect_kernel, (r, ev.last_defect_kernel)
                reached += 1
    assert reached == len(rows) + sum(r["slices"] for r in rows)
    assert not outside, (len(outside), "of", reached, outside[:3])


@pytest.mark.parametrize("sym_ct,shape", [(ct, s) for s in ((256, 19), (128, 32)) for ct in (1, 2, 3, 5, 6, 7, 8, 0) if ct != 2 or s[0] % 256 == 0])
def test_every_stand_alone_mfma_defect_kernel(built, sym_ct, shape):
    """The even/odd MFMA defect kernels beside the node kernel on two streams (register-staged with 64- and, on whole 256-node
    tiles, 128-column tiles; one-workgroup ring; state-split rings with SW = 6 / 2 / 1 / 3; the choice by batch size), and the
    split-K forms of the state-split rings with the epilogue in the combining workgroup or kernel."""
    M, B = shape
    ev, dXU, outs, ref = horizon_ev(1, M, B)
    ev.set_option("sym_ct", sym_ct)
    ev.set_option("overlap_mode", 2)
    full_pass(f"quadrotor ({M}, {B}) sym_ct={sym_ct}, two streams", ev, dXU, outs, ref)
    assert ev.uses_fused_kernel
    print("   ", ev.last_defect_kernel)
    if sym_ct in (5, 6, 7, 8):
        ev.set_option("sym_ksplit", 2)
        for combine in (1, 0):
            ev.set_option("sym_combine", combine)
            full_pass(f"quadrotor ({M}, {B}) sym_ct={sym_ct}, 2 K slices, sym_combine={combine}", ev, dXU, outs, ref)
            print("   ", ev.last_defect_kernel)


@pytest.mark.parametrize("model,M,B", FR.SEQUENTIAL_SHAPES)
def test_sequential_pair(built, model, M, B):
    """"overlap" 0: node kernel, then the defect kernel that adds D.X -- the quadrotor, and the fixed wing (whose fp64 pass is this
    pair) on an odd mesh.  The defect kernel adds the products onto -h f, so the bound is the pair's (first_ref.py)."""
    ev, dXU, outs, ref = horizon_ev(model, M, B, accumulated=True)
    ev.set_option("overlap", 0)
    full_pass(f"{NAMES[model]} ({M}, {B}), sequential pair", ev, dXU, outs, ref)
    assert not ev.uses_fused_kernel
