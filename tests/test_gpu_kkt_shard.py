"""emi_kkt_factor_shard_dev / _lowrank_shard_dev / _solve_shard_dev / _solve_refined_shard_dev: the Newton steps of the B instances
of ONE context, device arrays in and out, against numpy (tests/kkt_shard_ref.py) and the single entry points.  -m gpu

Bounds are the project's existing ones for batched solves (tests/test_gpu_kkt.py): backward error max|K x - b| < 1e-9 (max|K| max|x|
+ 1) in the numpy matrix with fixed rows zeroed, agreement with the single path to 1e-9 (max|x| + 1), refined solves to 1e-11 of
the right-hand side at "kkt_refine_exp" 14.  The fixtures that carry low-rank lists are validated by tests/test_kkt_shard_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import kkt_shard_ref as S

pytestmark = pytest.mark.gpu

DC = 1e-9
EPS = np.finfo(np.float64).eps


def make_ev(M, model=1, B=1, f32=False):
    import etol_amd as E
    from etol_amd import workloads as W
    ev = E.Evaluator(0, f32=f32)
    ev.set_mesh(M, 0.0, 4.0)
    ev.set_model(model, W.QUAD_PARAMS if model == 1 else [])
    ev.set_batch(B)
    return ev


def up(ev, a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
    torch.cuda.synchronize()
    return t


def upload(ev, fx):
    lay = ev.layout
    assert (lay.B, lay.nhess, lay.nvals, lay.M) == (fx["B"], fx["Q"].shape[1], fx["VALS"].shape[1], fx["M"])
    return up(ev, fx["Q"]), up(ev, fx["VALS"]), up(ev, fx["fixed"])


def down(ev, t):
    ev.synchronize()
    return t.cpu().numpy()


def masked(fx, b, rhs):
    ref = rhs.reshape(-1).copy()
    ref[np.nonzero(fx["fixed"][b].reshape(-1))[0]] = 0
    return ref


def assert_solves(K, x, ref, what):
    res = np.abs(K @ x - ref).max()
    bound = 1e-9 * (np.abs(K).max() * np.abs(x).max() + 1)
    print(f"{what}: max|K x - b| = {res:.3e}, bound {bound:.3e}")
    assert res < bound, what


def single_path(ev1, fx, b, rhs, dc=DC):
    """emi_kkt_factor_dev + emi_kkt_solve_dev of a B = 1 context on instance b's arrays"""
    Q, V, F = up(ev1, fx["Q"][b]), up(ev1, fx["VALS"][b]), up(ev1, fx["fixed"][b].reshape(-1))
    assert ev1.kkt_factor_dev(Q, V, F, dc) == 0
    x = up(ev1, rhs.reshape(-1))
    ev1.kkt_solve_dev(x)
    return down(ev1, x)


def factor_solve_check(M, model, B, seed, spoil=None):
    import etol_amd as E
    ns, nc, _ = E.model_dims(model)
    nv = ns + nc
    ev = make_ev(M, model, B)
    fx = S.shard_blocks(ev.D, M, ns, nv, B, seed)
    if spoil is not None:
        fx["Q"][spoil, 0, min(3, M - 1)] = -5.0          # node block 3 of that instance is indefinite: not the quasi-definite case
    Q, V, F = upload(ev, fx)
    info = ev.kkt_factor_shard_dev(Q, V, F, DC)
    assert np.array_equal(info, np.zeros(B, dtype=np.int32)), info
    rng = np.random.default_rng(seed + 1)
    ev1 = make_ev(M, model, 1)
    for rep in range(2):                                # one factorisation, two solves
        rhs = rng.standard_normal((B, nv + ns, M))
        x = up(ev, rhs)
        ev.kkt_solve_shard_dev(x)
        x = down(ev, x)
        for b in range(B):
            K = S.matrix(ev.D, fx, b, DC)
            xb, ref = x[b].reshape(-1), masked(fx, b, rhs[b])
            assert_solves(K, xb, ref, f"M {M} B {B} instance {b}")
            assert np.all(xb[np.nonzero(fx["fixed"][b].reshape(-1))[0]] == 0)
            if rep == 0 and b != spoil:
                one = single_path(ev1, fx, b, rhs[b])
                diff = np.abs(xb - one).max()
                print(f"  against the single path: {diff:.3e}")
                assert diff < 1e-9 * (np.abs(one).max() + 1), b
    ev1.close()
    ev.close()


@pytest.mark.parametrize("M,model,B", [(9, 0, 2), (33, 1, 5), (65, 1, 3), (171, 1, 4)])
def test_shard_factor_and_solve_match_numpy_and_the_single_path(built, M, model, B):
    """a partial last Cholesky block at 33 and 65 nodes, a partial last block-inverse block at 171"""
    factor_solve_check(M, model, B, 8000 + M + B)


def test_an_instance_with_an_indefinite_node_block_falls_back_inside_the_call(built):
    factor_solve_check(33, 1, 5, 8100, spoil=4)


def test_singular_instance_is_reported_and_masked_out(built):
    import etol_amd as E
    M, ns, nv, B = 5, 2, 4, 3
    ev = make_ev(M, 0, B)
    fx = S.shard_blocks(ev.D, M, ns, nv, B, 8200)
    fx["Q"][1] = 0.0
    fx["VALS"][1, :ns * nv] = 0.0
    fx["fixed"][1] = 0
    Q, V, F = upload(ev, fx)
    dc = np.array([DC, 0.0, DC])
    info = ev.kkt_factor_shard_dev(Q, V, F, dc)
    assert info[1] > 0 and info[0] == 0 and info[2] == 0, info
    rhs = np.random.default_rng(8201).standard_normal((B, nv + ns, M))
    x = up(ev, rhs)
    with pytest.raises(E.EmiError, match="EMI_ERR_STATE"):
        ev.kkt_solve_shard_dev(x)
    ev.kkt_solve_shard_dev(x, mask=[1, 0, 1])
    x = down(ev, x)
    assert np.array_equal(x[1].view(np.uint8), rhs[1].view(np.uint8))
    for b in (0, 2):
        assert_solves(S.matrix(ev.D, fx, b, DC), x[b].reshape(-1), masked(fx, b, rhs[b]), f"instance {b}")
    ev.close()


def lists_up(ev, fx):
    return up(ev, fx["count"]), up(ev, fx["node"]), up(ev, fx["delta"]), up(ev, fx["vec"])


def lowrank_matrix(D, fx, b, use_lists):
    """K where the correction is active, K~ elsewhere"""
    Kt = S.matrix(D, fx, b, DC)
    r = int(fx["count"][b])
    if not use_lists or r == 0 or r > fx["max_mods"]:
        return Kt
    return S.unmodified(Kt, S.columns(fx, b, fx["node"][b], fx["vec"][b], r), fx["delta"][b, :r])


def test_lowrank_verdicts_from_device_lists(built):
    ev = make_ev(S.LR_M, 1, 4)
    fx = S.lr_fixture(ev.D, S.LR_VERDICTS)
    B, nv, ns, M = fx["B"], fx["nv"], fx["ns"], fx["M"]
    expect = [e[0] for e in S.expected_exact(ev.D, fx, DC)]
    assert expect == [1, 1, 0, 0]
    Q, V, F = upload(ev, fx)
    assert not ev.kkt_factor_shard_dev(Q, V, F, DC).any()
    exact = ev.kkt_lowrank_shard_dev(fx["max_mods"], *lists_up(ev, fx))
    assert list(exact) == expect, exact
    rng = np.random.default_rng(4101)
    rhs = rng.standard_normal((B, nv + ns, M))
    x = up(ev, rhs)
    ev.kkt_solve_shard_dev(x)
    x = down(ev, x)
    for b in range(B):
        assert_solves(lowrank_matrix(ev.D, fx, b, bool(exact[b])), x[b].reshape(-1), masked(fx, b, rhs[b]), f"instance {b} exact {exact[b]}")
    # the answers differ where a correction is active: the check above is not blind to it
    assert np.abs(S.matrix(ev.D, fx, 1, DC) @ x[1].reshape(-1) - masked(fx, 1, rhs[1])).max() > 1e-6
    assert list(ev.kkt_lowrank_shard_dev(0)) == [1, 1, 1, 1]                 # cleared: every instance answers for K~ again
    x = up(ev, rhs)
    ev.kkt_solve_shard_dev(x)
    x = down(ev, x)
    for b in range(B):
        assert_solves(S.matrix(ev.D, fx, b, DC), x[b].reshape(-1), masked(fx, b, rhs[b]), f"cleared, instance {b}")
    ev.close()


def test_lists_of_emi_kkt_blocks_dev_pass_on_without_a_download(built):
    """blocks with reflected eigenvalues through emi_kkt_blocks_dev itself; Q, the lists and the count stay on the device between
    the calls.  The verdict is the inertia of the matrix numpy builds from the downloaded Qexact, the solve answers for it where
    exact and for the matrix of the downloaded Q elsewhere."""
    import torch
    from test_gpu_blocks import make_ev as blocks_ev
    nv, ns, M, B = (S.BLK[k] for k in ("nv", "ns", "M", "B"))
    ev = blocks_ev(nv, M, B, S.BLK["np"])
    case = S.blocks_fixture(ev.D)
    nh, mm = nv * (nv + 1) // 2, nv * M
    kw = dict(device=ev.device)
    H, V, Sg, St, F = (up(ev, case[k]) for k in ("H", "VALS", "Sigma", "SigT", "fixed"))
    Q, Qx = (torch.full((B, nh, M), float("nan"), dtype=torch.float64, **kw) for _ in range(2))
    count = torch.full((B,), -5, dtype=torch.int32, **kw)
    node = torch.full((B, mm), -7, dtype=torch.int32, **kw)
    delta, vec = torch.full((B, mm), float("nan"), dtype=torch.float64, **kw), torch.full((B, mm, nv), float("nan"), dtype=torch.float64, **kw)
    worst = torch.full((B,), float("nan"), dtype=torch.float64, **kw)
    rhs = np.random.default_rng(978).standard_normal((B, nv + ns, M))
    x = up(ev, rhs)
    ev.kkt_blocks_dev(H, V, Sg, St, F, case["dw"], Q, mm, count, node, delta, vec, worst, Qexact=Qx)
    info = ev.kkt_factor_shard_dev(Q, V, F, DC)
    exact = ev.kkt_lowrank_shard_dev(mm, count, node, delta, vec)
    ev.kkt_solve_shard_dev(x)
    x, Qd, Qxd, cnt = down(ev, x), down(ev, Q), down(ev, Qx), down(ev, count)
    assert not info.any() and (cnt > 0).all() and (cnt <= min(mm, 4096)).all()
    fx = dict(M=M, ns=ns, nv=nv, B=B, Q=Qd, VALS=case["VALS"], fixed=case["fixed"])
    for b in range(B):
        K = S.matrix(ev.D, fx, b, DC, Q=Qxd[b])
        assert exact[b] == int(S.inertia_ok(K, M, ns, nv)), (b, exact[b])
        Kref = K if exact[b] else S.matrix(ev.D, fx, b, DC)
        assert_solves(Kref, x[b].reshape(-1), masked(fx, b, rhs[b]), f"instance {b} exact {exact[b]} ({cnt[b]} pairs)")
    ev.close()


@pytest.mark.parametrize("M,B", [(65, 1), (200, 3)])
def test_refined_solves_of_a_shard(built, M, B):
    """emi_kkt_solve_refined_shard_dev at shapes of the existing refined test, its depth ("kkt_refine_exp" 14, 8 steps) and its bound
    (1e-11 of the right-hand side, in the NOMINAL matrix: instance 1's nominal dc is 0 while its factorisation holds 1e-9)"""
    ns, nv = 6, 8
    ev = make_ev(M, 1, B)
    fx = S.shard_blocks(ev.D, M, ns, nv, B, 9200 + M)
    dcs = np.array([1e-9, 0.0, 1e-8][:B])
    Q, V, F = upload(ev, fx)
    assert not ev.kkt_factor_shard_dev(Q, V, F, dcs).any()
    lr = None
    if B >= 3:                  # instance 2 with an active correction K = K~ - d u u^T
        rng = np.random.default_rng(9201)
        fx.update(max_mods=1, count=np.array([0, 0, 1], dtype=np.int32), node=np.full((B, 1), M // 3, dtype=np.int32),
                  delta=np.full((B, 1), 0.5), vec=rng.standard_normal((B, 1, nv)) * 0.3)
        exact = ev.kkt_lowrank_shard_dev(1, up(ev, fx["count"]), up(ev, fx["node"]), up(ev, fx["delta"]), up(ev, fx["vec"]))
        assert list(exact) == [1, 1, 1]
        lr = 2
    rhs = np.random.default_rng(9202 + M).standard_normal((B, nv + ns, M))
    x = up(ev, rhs)
    ev.set_option("kkt_refine_exp", 14)          # (process-wide)
    try:
        out = ev.kkt_solve_refined_shard_dev(x, dcs, max_steps=8)
    finally:
        ev.set_option("kkt_refine_exp", 10)
    x = down(ev, x)
    print(out)
    assert (out["status"] == 0).all() and (out["nsolve"] >= 1).all() and (out["nsolve"] <= 9).all()
    assert np.isin(out["reverted"], (0, 1)).all()
    for b in range(B):
        K = S.matrix(ev.D, fx, b, dcs[b])
        if b == lr:
            K = S.unmodified(K, S.columns(fx, b, fx["node"][b], fx["vec"][b], 1), fx["delta"][b, :1])
        ref = masked(fx, b, rhs[b])
        res = np.abs(K @ x[b].reshape(-1) - ref).max() / max(1.0, np.abs(ref).max())
        print(f"instance {b}: rel {out['rel'][b]:.3e}, numpy {res:.3e}, {out['nsolve'][b]} solves")
        assert out["rel"][b] <= 1e-11 and res < 1e-11
        assert abs(res - out["rel"][b]) < 1e-11
    ev.close()


def test_masks_and_bits(built):
    import etol_amd as E
    ev = make_ev(S.LR_M, 1, 3)
    old = S.lr_fixture(ev.D, S.LR_MASKS)
    B, nv, ns, M = old["B"], old["nv"], old["ns"], old["M"]
    rng = np.random.default_rng(4201)
    rhs = rng.standard_normal((B, nv + ns, M))

    def sequence(e, fx, mask=None):
        Q, V, F = upload(e, fx)
        info = e.kkt_factor_shard_dev(Q, V, F, DC, mask=mask)
        exact = e.kkt_lowrank_shard_dev(fx["max_mods"], *lists_up(e, fx), mask=mask)
        x = up(e, rhs)
        e.kkt_solve_shard_dev(x, mask=mask)
        return info, exact, down(e, x)

    info, exact, x = sequence(ev, old)
    assert not info.any() and list(exact) == [e[0] for e in S.expected_exact(ev.D, old, DC)]
    ev2 = make_ev(S.LR_M, 1, 3)
    _, exact2, x2 = sequence(ev2, old)                      # two identical call sequences: identical bits
    _, exact3, x3 = sequence(ev2, old)
    for e_, x_ in ((exact2, x2), (exact3, x3)):
        assert np.array_equal(exact, e_) and np.array_equal(x.view(np.uint8), x_.view(np.uint8))
    ev2.close()
    # other blocks and lists with instance 1 masked in every call: its slice keeps every bit ...
    new = S.lowrank_fixture(ev.D, M, (S.INEXACT_SCALE, S.INEXACT_SCALE, S.EXACT_SCALE), old["max_mods"], 4300)
    mask = np.array([1, 0, 1], dtype=np.uint8)
    info, exact_new, xm = sequence(ev, new, mask=mask)
    assert info[1] == -1 and exact_new[1] == -1               # (the wrapper's fill: the library did not write them)
    assert np.array_equal(xm[1].view(np.uint8), rhs[1].view(np.uint8))
    for b in (0, 2):
        assert_solves(lowrank_matrix(ev.D, new, b, bool(exact_new[b])), xm[b].reshape(-1), masked(new, b, rhs[b]), f"new instance {b}")
    # ... and a later unmasked solve uses its OLD factors and its old correction
    xa = up(ev, rhs)
    ev.kkt_solve_shard_dev(xa)
    xa = down(ev, xa)
    assert np.array_equal(xa[1].view(np.uint8), x[1].view(np.uint8))
    assert_solves(lowrank_matrix(ev.D, old, 1, bool(exact[1])), xa[1].reshape(-1), masked(old, 1, rhs[1]), "instance 1, old matrix")
    for b in (0, 2):
        assert_solves(lowrank_matrix(ev.D, new, b, bool(exact_new[b])), xa[b].reshape(-1), masked(new, b, rhs[b]), f"new instance {b}, unmasked solve")
    # another mesh: what the workspaces hold is for the old one
    ev.set_mesh(33, 0.0, 4.0)
    xs = up(ev, np.zeros((B, nv + ns, 33)))
    with pytest.raises(E.EmiError, match="EMI_ERR_STATE"):
        ev.kkt_solve_shard_dev(xs)
    with pytest.raises(E.EmiError, match="EMI_ERR_STATE"):
        ev.kkt_lowrank_shard_dev(0)
    ev.close()


def test_status_codes(built):
    import etol_amd as E
    import torch
    M, B, ns, nv = 9, 2, 6, 8
    lib = E.load()

    def calls(ev):
        t = torch.zeros(B * 64 * M, dtype=torch.float64, device=ev.device)
        p = C.c_void_p(t.data_ptr())
        dc, rel = np.full(B, DC), np.zeros(B)
        i4 = [np.zeros(B, dtype=np.int32) for _ in range(4)]
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        return t, [lambda: lib.emi_kkt_factor_shard_dev(ev.ctx, p, p, p, dp(dc), None, ip(i4[0])),
                   lambda: lib.emi_kkt_lowrank_shard_dev(ev.ctx, 0, None, None, None, None, None, ip(i4[0])),
                   lambda: lib.emi_kkt_solve_shard_dev(ev.ctx, p, None),
                   lambda: lib.emi_kkt_solve_refined_shard_dev(ev.ctx, p, None, dp(dc), 4, dp(rel), ip(i4[1]), ip(i4[2]), ip(i4[3]))]

    ev = make_ev(M, 1, B, f32=True)
    keep, fs = calls(ev)
    assert [f() for f in fs] == [5, 5, 5, 5]                        # EMI_ERR_UNSUPPORTED: f32 context
    ev.close()
    ev = make_ev(M, 1, B)
    ev.set_delays(0, 1, 0.1)
    keep, fs = calls(ev)
    assert [f() for f in fs] == [5, 5, 5, 5]                        # delays set
    ev.close()
    ev = make_ev(M, 1, B)
    ev.set_option("kkt_method", 0)
    keep, fs = calls(ev)
    assert [f() for f in fs] == [5, 5, 5, 5]                        # the LU method
    ev.set_option("kkt_method", 1)
    assert [f() for f in fs[1:]] == [2, 2, 2]                       # EMI_ERR_STATE: nothing factorised
    p = C.c_void_p(keep.data_ptr())
    dc, rel, i1 = np.full(B, DC), np.zeros(B), np.zeros(B, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for args in ((None, p, p, dp(dc), None, ip(i1)), (p, None, p, dp(dc), None, ip(i1)), (p, p, None, dp(dc), None, ip(i1)),
                 (p, p, p, None, None, ip(i1)), (p, p, p, dp(dc), None, None)):
        assert lib.emi_kkt_factor_shard_dev(ev.ctx, *args) == 1     # EMI_ERR_ARG: NULL where not optional
    assert lib.emi_kkt_factor_shard_dev(None, p, p, p, dp(dc), None, ip(i1)) == 1
    neg = np.array([DC, -1.0])
    assert lib.emi_kkt_factor_shard_dev(ev.ctx, p, p, p, dp(neg), None, ip(i1)) == 1       # negative dc
    assert lib.emi_kkt_lowrank_shard_dev(ev.ctx, 0, None, None, None, None, None, None) == 1
    assert lib.emi_kkt_lowrank_shard_dev(ev.ctx, 3, p, None, p, p, None, ip(i1)) == 1
    assert lib.emi_kkt_lowrank_shard_dev(ev.ctx, -1, p, p, p, p, None, ip(i1)) == 1
    assert lib.emi_kkt_solve_shard_dev(ev.ctx, None, None) == 1
    assert lib.emi_kkt_solve_shard_dev(None, p, None) == 1
    assert lib.emi_kkt_solve_refined_shard_dev(ev.ctx, None, None, dp(dc), 4, dp(rel), ip(i1), ip(i1), ip(i1)) == 1
    assert lib.emi_kkt_solve_refined_shard_dev(ev.ctx, p, None, None, 4, dp(rel), ip(i1), ip(i1), ip(i1)) == 1
    assert lib.emi_kkt_solve_refined_shard_dev(ev.ctx, p, None, dp(dc), 4, None, ip(i1), ip(i1), ip(i1)) == 1
    assert lib.emi_kkt_solve_refined_shard_dev(ev.ctx, p, None, dp(dc), -1, dp(rel), ip(i1), ip(i1), ip(i1)) == 1
    ev.close()


def test_one_iteration_of_a_shard_on_the_device(built):
    """tests/test_gpu_ipm.py's test_one_iteration_on_the_device at B = 3 with three barrier parameters: evaluation, gradient,
    Hessian, reduction, node blocks WITH lists, the shard's factorisation, its inertia verdict, its refined solve on DZLam whole,
    expansion, trial point, merit, acceptance and KKT error.  Between the stages only info / exact / rel reach the host.  Every
    stage is then checked on ITS downloaded inputs, per instance."""
    import torch
    import ipm_ref as R
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    from test_gpu_ipm import DevBackend, _column
    from test_gpu_ipm import make_ev as ipm_ev
    nv, ns, nc, npth, M, B = 8, 6, 2, 3, 33, 3
    nh, mm = nv * (nv + 1) // 2, nv * M
    c = dict(nv=nv, ns=ns, nc=nc, np=npth, M=M, B=B, nsets=B, model=1, nvals=ns * nv + 2 * npth + nv, rows=R.default_rows(ns, nv, npth),
             cscale=None, rs=None, DefRes=None, RowRes=None)
    ev = ipm_ev(c)
    rng = np.random.default_rng(5)
    X, U, _ = W.quadrotor_batch(7, B, M, 0)
    RES0, _, _ = ev.eval_host(X, U)
    z = np.concatenate([X, U], 1)
    zl, zu = z - (1.0 + np.abs(z)), z + (1.0 + np.abs(z))
    zl[:, nv - 1], zu[:, 3] = -1e20, 1e20
    zl[:, :ns, 0] = zu[:, :ns, 0] = z[:, :ns, 0]
    cl, cu = np.full(npth, -1e20), np.zeros(npth)
    cpath = RES0[:, ns:]
    Sl = np.minimum(cpath, -0.01)
    gap = cpath - Sl
    ee = 0.01 * np.maximum(1.0, np.abs(gap))
    rho = 10.0
    c.update(X=X, U=U, S=Sl, E1=np.maximum(gap, 0) + ee, E2=np.maximum(-gap, 0) + ee, zl=zl, zu=zu, cl=cl, cu=cu,
             LamF=0.1 * rng.standard_normal((B, ns, M)), Y=0.05 * rng.standard_normal((B, npth, M)),
             ZL=np.where((zu > zl) & (zl > -R.INF), 1.0, 0.0), ZU=np.where((zu > zl) & (zu < R.INF), 1.0, 0.0),
             VL=np.zeros((B, npth, M)), VU=np.ones((B, npth, M)),
             par=np.array([[0.1, rho, 0.99, 1.0], [0.05, rho, 0.99, 1.0], [0.2, rho, 0.99, 1.0]]))
    c["W1"], c["W2"] = rho - c["Y"], rho + c["Y"]
    fixed = np.ascontiguousarray((~(zu > zl)).astype(np.uint8))

    be = DevBackend(ev)
    kw = dict(dtype=torch.float64, device=ev.device)
    nan = lambda *s: torch.full(s, float("nan"), **kw)
    pt, du, bd, par = be.group(R.POINT, c), be.group(R.DUALS, c), be.bounds(c), be.up(c["par"])
    fx = be.up(fixed)
    RES, VALS, COST, G, H = nan(B, ns + npth, M), nan(B, c["nvals"], M), nan(B), nan(B, nv, M), nan(B, nh, M)
    el = dict(Sigma=nan(B, nv, M), **{n: nan(B, npth, M) for n in ("SigT", "SigS", "RhatS", "Rt")})
    step = {n: nan(B, nv if n in ("DZL", "DZU") else npth, M) for n in R.STEP[1:]}
    step["DZLam"] = nan(B, nv + ns, M)
    rhs_keep, Q, Qx = nan(B, nv + ns, M), nan(B, nh, M), nan(B, nh, M)
    count, worst = torch.zeros(B, dtype=torch.int32, device=ev.device), nan(B)
    node = torch.full((B, mm), -7, dtype=torch.int32, device=ev.device)
    delta, vec = nan(B, mm), nan(B, mm, nv)
    scal, mer, err = nan(B, 4), nan(B, 2), nan(B, 3)
    trial = dict(X=nan(B, ns, M), U=nan(B, nc, M), **{n: nan(B, npth, M) for n in ("S", "E1", "E2")})
    RESt, COSTt = nan(B, ns + npth, M), nan(B)
    RES2, VALS2, COST2, G2 = nan(B, ns + npth, M), nan(B, c["nvals"], M), nan(B), nan(B, nv, M)
    torch.cuda.synchronize()
    # ---- the chain ---------------------------------------------------------------------------------------------------------------
    ev.eval_dev(pt["X"], pt["U"], RES, VALS, COST)
    ev.lagr_grad_dev(VALS, du["LamF"], du["Y"], 1.0, G)
    ev.hess_dev(pt["X"], pt["U"], du["LamF"], du["Y"], 1.0, H)
    ev.ipm_reduce(pt, du, RES, VALS, G, bd, par, el, step["DZLam"])
    ev.kkt_blocks_dev(H, VALS, el["Sigma"], el["SigT"], fx, 0.0, Q, mm, count, node, delta, vec, worst, Qexact=Qx)
    ev.synchronize()
    rhs_keep.copy_(step["DZLam"])                                           # (kept for the checks below)
    torch.cuda.synchronize()
    info = ev.kkt_factor_shard_dev(Q, VALS, fx, DC)                         # [B] scalars to the host
    exact = ev.kkt_lowrank_shard_dev(mm, count, node, delta, vec)           # [B]
    ref_out = ev.kkt_solve_refined_shard_dev(step["DZLam"], DC, max_steps=8)   # rel, nsolve, reverted, status [B]
    assert not info.any() and (ref_out["status"] == 0).all()
    ev.ipm_expand(pt, du, VALS, bd, par, el, step, scal)
    a_pr, a_du = _column(ev, scal, 0), _column(ev, scal, 1)
    ev.ipm_trial(pt, step, a_pr, trial)
    ev.synchronize()
    S_before = trial["S"].clone()
    torch.cuda.synchronize()
    ev.eval_dev(trial["X"], trial["U"], RESt, None, COSTt, flags=L.EVAL_ALL | L.EVAL_NOJAC)
    ev.ipm_merit(trial, RESt, COSTt, bd, par, mer, reset=True)
    ev.ipm_accept(pt, trial, du, step, bd, par, a_pr, a_du)
    ev.eval_dev(pt["X"], pt["U"], RES2, VALS2, COST2)
    ev.lagr_grad_dev(VALS2, du["LamF"], du["Y"], 1.0, G2)
    ev.ipm_error(pt, du, RES2, G2, bd, par, err)
    ev.synchronize()
    # ---- every stage on its downloaded inputs ------------------------------------------------------------------------------------
    dn = lambda t: t.cpu().numpy()
    c.update(RES=dn(RES), VALS=dn(VALS), G=dn(G), COST=dn(COST))
    red = {n: dn(el[n]) for n in el}
    red["Rhs"] = dn(rhs_keep)
    ref = R.reduce_ref(c)
    for k in ("Sigma", "Rhs", "SigS", "RhatS", "SigT", "Rt"):
        R.check_elementwise(k, red[k], ref[k], print)
    st = {n: dn(step[n]) for n in step}
    sfx = dict(M=M, ns=ns, nv=nv, B=B, Q=dn(Q), VALS=c["VALS"], fixed=fixed)
    Qxd, cnt = dn(Qx), dn(count)
    N = (nv + ns) * M
    for b in range(B):
        # the verdict: the inertia of the matrix of the blocks as assembled; the refined step solves the NOMINAL matrix it belongs to
        Kx = S.matrix(ev.D, sfx, b, DC, Q=Qxd[b])
        assert cnt[b] <= mm and exact[b] == int(S.inertia_ok(Kx, M, ns, nv)), (b, cnt[b], exact[b])
        K = Kx if exact[b] else S.matrix(ev.D, sfx, b, DC)
        x, rb = st["DZLam"][b].reshape(-1), masked(sfx, b, red["Rhs"][b])
        assert_solves(K, x, rb, f"instance {b}: {cnt[b]} pairs, exact {exact[b]}")
        res = np.abs(K @ x - rb).max() / max(1.0, np.abs(rb).max())
        # the device's residual and numpy's are sums of at most N + 1 terms each
        tol = 4 * N * EPS * (np.abs(K).max() * np.abs(x).max() + np.abs(rb).max()) / max(1.0, np.abs(rb).max())
        print(f"  rel {ref_out['rel'][b]:.3e} numpy {res:.3e} (tolerance {tol:.1e}), {ref_out['nsolve'][b]} solves")
        assert abs(res - ref_out["rel"][b]) <= tol and 1 <= ref_out["nsolve"][b] <= 9
    sref = R.expand_ref(c, red, st["DZLam"])
    for k in R.STEP:
        R.check_elementwise(k, st[k], sref[k], print)
    sc = dn(scal)
    rs = R.expand_scalars_ref(c, st)
    for b in range(B):
        r = rs[b]
        R.check_scalar("apr", sc[b, 0], *r["apr"]); R.check_scalar("adu", sc[b, 1], *r["adu"]); R.check_scalar("mmax", sc[b, 3], *r["mmax"])
        R.check_scalar("dphi", sc[b, 2], r["dphi"]["value"], r["dphi"]["tol"])
    tr = {n: dn(trial[n]) for n in trial}
    tref = R.trial_ref(c, st, sc[:, 0])
    S_reset = tr["S"]
    ptm = dict(tr, S=dn(S_before), RES=dn(RESt), COST=dn(COSTt))
    for k in R.POINT:
        R.check_elementwise("t" + k, ptm[k], tref[k], print)
    jump, margin, target, inside = R.reset_ref(c, ptm)
    moved = S_reset != ptm["S"]
    close = np.abs(margin.v) <= margin.bound()
    assert (moved == jump)[~close].all()
    if moved.any():
        R.check_elementwise("Sreset", S_reset[moved], target[moved], print)
    ms = R.merit_ref(c, dict(ptm, S=S_reset))
    mo = dn(mer)
    for b in range(B):
        R.check_scalar("phi", mo[b, 0], ms[b]["phi"]["value"], ms[b]["phi"]["tol"])
        R.check_scalar("infeas", mo[b, 1], ms[b]["infeas"]["value"], ms[b]["infeas"]["tol"])
    new = {n: dn(du[n]) for n in du}
    aref = R.accept_ref(c, tr, st, sc[:, 0], sc[:, 1])
    for k, rr in aref.items():
        R.check_elementwise("a" + k, new[k], rr, print)
    for k in R.POINT:
        assert np.array_equal(dn(pt[k]), tr[k]), k
    c2 = dict(c, **new, **tr, RES=dn(RES2), G=dn(G2))
    es = R.error_ref(c2)
    eo = dn(err)
    for b in range(B):
        e = es[b]
        R.check_scalar("kkt_error", eo[b, 0], *e["kkt"]); R.check_scalar("viol", eo[b, 1], *e["viol"]); R.check_scalar("emax", eo[b, 2], *e["emax"])
        print(f"instance {b}: apr {sc[b, 0]:.3f} adu {sc[b, 1]:.3f} phi {mo[b, 0]:.6e} kkt {eo[b, 0]:.3e}")
    ev.close()
