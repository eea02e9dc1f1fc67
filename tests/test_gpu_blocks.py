"""emi_kkt_blocks_dev / _host / _rows and emi_kkt_factor_dev: the node blocks of the Newton step assembled, screened and made
positive definite on the device, against the numpy reference (tests/blocks_ref.py: numpy.linalg.eigh on the scaled block).  -m gpu

Cases, bounds and checks are the ones tests/test_blocks_cpu.py validates on the host routine (blocks_ref.case_list / check):
assembly within (np + 3) eps sum|terms|; blocks that pass the screen bitwise untouched; in the scaled space
|Q~ - (Q + sum delta v v^T)| <= 8 nv^2 eps, smallest eigenvalue of Q~ >= fl (1 - 1e-6), as many pairs per node as reference
eigenvalues < -fl, delta within 8 nv^2 eps (1 + 2 |lambda|) of 2 |lambda|; rank-deficient PSD blocks: no pair, smallest eigenvalue
>= fl / 2.  Invariants only, never eigenvectors."""
import ctypes as C

import numpy as np
import pytest

import blocks_ref as R

pytestmark = pytest.mark.gpu

KEYS = R.case_list()
SLACK = 64          # poisoned list entries behind the last instance (dev_blocks)
IDS = [f"{k[0]}-nv{k[1]}-M{k[2]}-B{k[3]}-np{k[4]}" for k in KEYS]


def make_ev(nv, M, B, npth, f32=False):
    import etol_amd as E
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    model = R.MODEL_OF_NV[nv][0]
    ev = E.Evaluator(0, f32=f32)
    ev.set_mesh(M, 0.0, 4.0)
    ev.set_model(model, {0: [], 1: W.QUAD_PARAMS, 2: W.FW_PARAMS}[model])
    ev.set_batch(B)
    if npth:
        recs = np.zeros((npth, L.PATH_REC))
        recs[:, 0] = L.PATH_DISC
        recs[:, 1:4] = [[4.0, 3.2, 0.64], [6.3, 4.4, 0.49], [2.5, 1.2, 0.16]][:npth]
        ev.set_path(recs, 0, 1)
    lay = ev.layout
    assert lay.ns + lay.nc == nv and lay.np == npth
    return ev


def dev_blocks(ev, case, max_mods=None, want_exact=True):
    """the _dev form on torch tensors; every output buffer is poisoned first.  Returns numpy arrays (blocks_ref.check's dict)."""
    import torch
    nv, M, B = case["nv"], case["M"], case["B"]
    nh = nv * (nv + 1) // 2
    mm = nv * M if max_mods is None else max_mods
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    H, V, Sg, fx = t(case["H"]), t(case["VALS"]), t(case["Sigma"]), t(case["fixed"])
    St = t(case["SigT"]) if case["np"] else None
    kw = dict(device=ev.device)
    Q = torch.full((B, nh, M), float("nan"), dtype=torch.float64, **kw)
    Qx = torch.full((B, nh, M), float("nan"), dtype=torch.float64, **kw) if want_exact else None
    count = torch.full((B,), -5, dtype=torch.int32, **kw)
    # the three list arrays as ONE poisoned allocation each with SLACK entries behind the last instance: [B][mm] as the call sees
    # it, then room that no correct call touches (an overrun of the last instance would land there, not out of bounds)
    node_all = torch.full((B * mm + SLACK,), -7, dtype=torch.int32, **kw)
    delta_all = torch.full((B * mm + SLACK,), float("nan"), dtype=torch.float64, **kw)
    vec_all = torch.full(((B * mm + SLACK) * nv,), float("nan"), dtype=torch.float64, **kw)
    node, delta, vec = node_all[:B * mm].view(B, mm), delta_all[:B * mm].view(B, mm), vec_all[:B * mm * nv].view(B, mm, nv)
    worst = torch.full((B,), float("nan"), dtype=torch.float64, **kw)
    torch.cuda.synchronize()
    ev.kkt_blocks_dev(H, V, Sg, St, fx, case["dw"], Q, mm, count, node, delta, vec, worst, Qexact=Qx)
    ev.synchronize()
    assert (node_all[B * mm:] == -7).all() and delta_all[B * mm:].isnan().all() and vec_all[B * mm * nv:].isnan().all(), "written behind the lists"
    out = dict(Q=Q, count=count, node=node, delta=delta, vec=vec, worst=worst)
    if want_exact:
        out["Qexact"] = Qx
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


@pytest.fixture(scope="module")
def results(built):
    """(case, device result of the _dev form) of every case, computed once"""
    res = {}
    for key in KEYS:
        case = R.get_case(key)
        ev = make_ev(case["nv"], case["M"], case["B"], case["np"])
        res[key] = (case, dev_blocks(ev, case))
        ev.close()
    return res


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_blocks_against_the_reference(results, key):
    case, out = results[key]
    fig = R.check(case, out, sorted_within_node=True, log=print)
    assert fig["nfail"] > 0
    # nothing behind the list of an instance was written
    for b in range(case["B"]):
        n = out["count"][b]
        assert (out["node"][b, n:] == -7).all() and np.isnan(out["delta"][b, n:]).all() and np.isnan(out["vec"][b, n:]).all()


@pytest.mark.parametrize("key", [k for k in KEYS if k[0] == "inertia" and k[2] == 33 and k[3] == 3], ids=lambda k: f"nv{k[1]}")
def test_overflow_determinism_and_forms(results, key):
    case, full = results[key]
    nv, M, B = case["nv"], case["M"], case["B"]
    ev = make_ev(nv, M, B, case["np"])
    # two calls give the same bits; without Qexact nothing else changes
    again = dev_blocks(ev, case)
    assert same_bits(full, again)
    noex = dev_blocks(ev, case, want_exact=False)
    assert same_bits({k: v for k, v in full.items() if k != "Qexact"}, noex)
    # max_mods smaller than the true count: the count is true, the first max_mods entries are the unbounded call's, nothing behind
    mm = int(full["count"].min()) // 2
    assert mm >= 2
    cut = dev_blocks(ev, case, max_mods=mm)
    assert np.array_equal(cut["count"], full["count"]) and np.array_equal(cut["worst"], full["worst"])
    assert np.array_equal(cut["node"], full["node"][:, :mm]) and np.array_equal(cut["delta"], full["delta"][:, :mm])
    assert np.array_equal(cut["vec"], full["vec"][:, :mm]) and np.array_equal(cut["Q"], full["Q"])
    # a bound between the counts of the instances: the instances below it keep their poison behind their own count, the ones above
    # are cut -- an entry written behind max_mods would show in the next instance's poison or in the slack (dev_blocks asserts it)
    cs = np.sort(full["count"])
    mid = int(cs[0] + cs[-1]) // 2 if cs[0] != cs[-1] else int(cs[0]) + 3
    part = dev_blocks(ev, case, max_mods=mid)
    for b in range(B):
        n = min(int(full["count"][b]), mid)
        assert np.array_equal(part["node"][b, :n], full["node"][b, :n]) and np.array_equal(part["vec"][b, :n], full["vec"][b, :n])
        assert (part["node"][b, n:] == -7).all() and np.isnan(part["delta"][b, n:]).all() and np.isnan(part["vec"][b, n:]).all()
    none = dev_blocks(ev, case, max_mods=0)                       # (poisoned buffers handed over but not to be touched: dev_blocks asserts it)
    assert np.array_equal(none["count"], full["count"]) and np.array_equal(none["Q"], full["Q"])
    # the _host form is the _dev form
    host = ev.kkt_blocks_host(case["H"], case["VALS"], case["Sigma"], case["SigT"], case["fixed"], case["dw"])
    for k in ("Qexact", "Q", "count", "worst"):
        assert np.array_equal(host[k], full[k]), k
    for b in range(B):
        n = full["count"][b]
        assert np.array_equal(host["node"][b, :n], full["node"][b, :n]) and np.array_equal(host["delta"][b, :n], full["delta"][b, :n])
        assert np.array_equal(host["vec"][b, :n], full["vec"][b, :n])
        assert (host["node"][b, n:] == -1).all() and np.isnan(host["delta"][b, n:]).all()
    hcut = ev.kkt_blocks_host(case["H"], case["VALS"], case["Sigma"], case["SigT"], case["fixed"], case["dw"], max_mods=mm)
    assert np.array_equal(hcut["count"], full["count"]) and np.array_equal(hcut["vec"], full["vec"][:, :mm])
    # the generic-nv assembly kernel equals the templated one
    ev.set_option("blocks_generic", 1)
    gen = dev_blocks(ev, case)
    ev.set_option("blocks_generic", 0)
    assert same_bits(full, gen)
    ev.close()


def staging_case(B, want):
    """[B] instances of a "deficient" case (no eigenpair anywhere), each with ONE node taken over from an "inertia" case: a block
    the reference gives want[b] negative eigenvalues.  A block is the [b, :, k] column of the five input arrays, so a column moved
    as a whole brings its verdict along; both cases come from blocks_ref.make_case."""
    nv, ns, M, npth = 8, 6, 33, 2
    case = R.make_case("deficient", nv, ns, M, B, npth, 4242, dw=1e-4)
    donor = R.make_case("inertia", nv, ns, M, B, npth, 4243, dw=1e-4)
    Qd, _ = R.assemble(donor["H"], donor["VALS"], donor["Sigma"], donor["SigT"], donor["fixed"], donor["dw"], donor["rows"], nv)
    nneg = np.array([[R.fix_block(Qd[b, :, k], donor["fixed"][b, :, k], nv)["nneg"] for k in range(M)] for b in range(B)])
    for b in range(B):
        sb, sk = np.argwhere(nneg == want[b])[b]            # (a different donor block per instance)
        for name in ("H", "VALS", "Sigma", "SigT", "fixed"):
            case[name][b, :, 3 + b] = donor[name][sb, :, sk]
    return case


def test_host_forms_share_staging_without_crosstalk(built):
    """emi_kkt_blocks_host and the interior-point host forms stage through the same slots of the context.  Node blocks at batch 2,
    then batch 5 (every slot grows), emi_ipm_trial_host, the node blocks at batch 5 and at batch 2 again: the same bits for the same
    instances every time, nothing written behind an instance's min(count, max_mods) list entries (the wrapper fills node / delta /
    vec with -1 / nan before each call), and emi_eval_host -- whose VALS staging buffer holds the invariant rows -- unchanged."""
    from etol_amd import workloads as W
    nv, ns, M, npth, mm = 8, 6, 33, 2, 2
    want = [1, 3, 1, 2, 1]                                  # eigenpairs per instance: below, at and above max_mods
    c5 = staging_case(5, want)
    c2 = {k: (np.ascontiguousarray(v[:2]) if isinstance(v, np.ndarray) and v.ndim == 3 else v) for k, v in c5.items()}
    X, U, _ = W.quadrotor_batch(11, 2, M, 0)
    ev = make_ev(nv, M, 2, npth)
    blocks = lambda c: ev.kkt_blocks_host(c["H"], c["VALS"], c["Sigma"], c["SigT"], c["fixed"], c["dw"], max_mods=mm)

    def lists_end_at_the_count(out, B):
        for b in range(B):
            assert out["count"][b] >= 1
            n = min(int(out["count"][b]), mm)
            assert (out["node"][b, :n] == 3 + b).all() and np.isfinite(out["delta"][b, :n]).all() and np.isfinite(out["vec"][b, :n]).all()
            assert (out["node"][b, n:] == -1).all() and np.isnan(out["delta"][b, n:]).all() and np.isnan(out["vec"][b, n:]).all()

    vals_before = ev.eval_host(X, U)[1]
    first = blocks(c2)                                      # 1.
    lists_end_at_the_count(first, 2)
    assert list(first["count"]) == want[:2]
    ev.set_batch(5)                                         # 2.
    rng = np.random.default_rng(5)
    r = lambda *shape: rng.standard_normal(shape)
    pt = dict(X=r(5, ns, M), U=r(5, nv - ns, M), S=r(5, npth, M), E1=r(5, npth, M), E2=r(5, npth, M))
    step = dict(DZLam=r(5, nv + ns, M), DS=r(5, npth, M), DE1=r(5, npth, M), DE2=r(5, npth, M))
    trial = {k: np.full_like(v, np.nan) for k, v in pt.items()}
    alpha = rng.uniform(0.1, 1.0, 5)
    ev.ipm_trial(pt, step, alpha, trial, dev=False)         # 3.
    al = alpha[:, None, None]
    for got, x, d in [(np.concatenate([trial["X"], trial["U"]], axis=1), np.concatenate([pt["X"], pt["U"]], axis=1), step["DZLam"][:, :nv]),
                      (trial["S"], pt["S"], step["DS"]), (trial["E1"], pt["E1"], step["DE1"]), (trial["E2"], pt["E2"], step["DE2"])]:
        # x + alpha d with one rounding (fma) or two
        assert (np.abs(got - (x + al * d)) <= 2 * R.EPS * (np.abs(x) + np.abs(al * d))).all()
    wide = blocks(c5)                                       # 4.
    lists_end_at_the_count(wide, 5)
    assert list(wide["count"]) == want
    assert same_bits(first, {k: v[:2] for k, v in wide.items()})
    ev.set_batch(2)                                         # 5.
    again = blocks(c2)
    lists_end_at_the_count(again, 2)
    assert same_bits(first, again)
    assert np.array_equal(ev.eval_host(X, U)[1].view(np.uint8), vals_before.view(np.uint8))
    ev.close()


@pytest.mark.parametrize("ns,nc", [(5, 1), (11, 1), (1, 1)], ids=["nv6", "nv12", "nv2"])
def test_block_sizes_between_the_compiled_ones(built, ns, nc):
    """nv = 6, 12 and 2 (models that exist only for their dimensions): the run-time-nv assembly kernel at an nv that has no compiled
    form, and the eigen-fix with lane groups wider than the block (rows padded with an identity).  Same checks, same bounds."""
    import etol_amd as E
    from test_gpu_kkt_shapes import chain_source
    nv, M, B = ns + nc, 33, 3
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, 4.0)
    ev.set_model_source(*chain_source(ns, nc), ns, nc)
    ev.set_batch(B)
    assert ev.layout.nvals == ns * nv + nv and ev.layout.np == 0
    for kind in ("inertia", "deficient") if nv > 2 else ("inertia",):
        case = R.make_case(kind, nv, ns, M, B, 0, 5000 + nv)
        assert case["rejected"] <= 0.01 * case["drawn"]
        fig = R.check(case, dev_blocks(ev, case), log=print)
        assert fig["nfail"] > 0
    ev.close()


def test_real_blocks_of_the_quadrotor(built):
    """H from emi_hess_dev at a random point of the quadrotor with 3 discs, multipliers of mixed sign; the initial state fixed.
    Every check and bound of the generated cases applies unchanged (blocks_ref.check knows no kind "real")."""
    from etol_amd import workloads as W
    M, B, npth, nv, ns = 33, 3, 3, 8, 6
    ev = make_ev(nv, M, B, npth)
    X, U, _ = W.quadrotor_batch(7, B, M, 0)
    rng = np.random.default_rng(77)
    _, VALS, _ = ev.eval_host(X, U)
    lamF = rng.standard_normal((B, ns, M)) * 10.0 ** rng.uniform(-2, 1, (B, ns, M))
    lamC = rng.standard_normal((B, npth, M))
    H = ev.hess_host(X, U, lamF, lamC, 1.0)
    fixed = np.zeros((B, nv, M), dtype=np.uint8)
    fixed[:, :ns, 0] = 1
    fixed[1, :, M - 1] = 1
    fixed[2, 3, 5] = 1
    Sigma = np.where(fixed != 0, 0.0, 10.0 ** rng.uniform(-2, 1, (B, nv, M)))
    SigT = 10.0 ** rng.uniform(-3, 2, (B, npth, M))
    case = dict(kind="real", nv=nv, ns=ns, M=M, B=B, np=npth, rows=R.default_rows(ns, nv, npth), dw=1e-4, H=H, VALS=VALS, Sigma=Sigma,
                SigT=SigT, fixed=fixed)
    out = dev_blocks(ev, case)
    fig = R.check(case, out, log=print)
    print("real blocks:", fig)
    assert fig["nfail"] > 0 and fig["npairs"] > 0
    ev.close()


def test_traced_rows_take_the_callers_list(built):
    """A context with rows traced by the model has no default list: EMI_ERR_STATE without one; with the list (a table row in
    front of four traced rows on six variables) the same checks as everywhere else."""
    import etol_amd as E
    from etol_amd import _lib as L
    from test_gpu_traced import traced_source
    src = traced_source(3)
    pv = [0, 1, 2, 3, 4, 6]
    M, B, nv, ns = 33, 3, 8, 6
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, 8.0)
    ev.set_model_source("TracedModel", src, 6, 2, npath=4, path_vars=pv)
    ev.set_batch(B)
    extra = np.zeros(L.PATH_REC); extra[:4] = [L.PATH_DISC, 6.3, 4.4, 0.49]
    ev.set_path(extra[None], 0, 1)
    lay = ev.layout
    assert lay.np == 5 and lay.nvals == 82
    rows = [[(0, 48), (1, 49)]] + [[(pv[q], 50 + 6 * j + q) for q in range(6)] for j in range(4)]
    case = R.make_case("inertia", nv, ns, M, B, 5, 4242, rows=rows, dw=1e-3, nvals=82)
    assert case["rejected"] <= 0.01 * case["drawn"]
    with pytest.raises(E.EmiError, match="EMI_ERR_STATE.*row list"):
        dev_blocks(ev, case)
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG.*out of range"):
        ev.kkt_blocks_rows(rows[:4] + [[(8, 50)]])
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG.*out of range"):
        ev.kkt_blocks_rows(rows[:4] + [[(0, 82)]])
    ev.kkt_blocks_rows(rows[:4])                     # a list of another length
    with pytest.raises(E.EmiError, match="EMI_ERR_STATE"):
        dev_blocks(ev, case)
    ev.kkt_blocks_rows(rows)
    R.check(case, dev_blocks(ev, case), log=print)
    ev.close()


def test_error_returns(built):
    import etol_amd as E
    from test_gpu_kkt_shapes import chain_source
    case = R.get_case(KEYS[0])
    ev = make_ev(4, 33, 3, 3, f32=True)
    with pytest.raises(E.EmiError, match="EMI_ERR_UNSUPPORTED.*f64"):
        ev.kkt_blocks_host(case["H"], case["VALS"], case["Sigma"], case["SigT"], case["fixed"])
    ev.close()
    ev = E.Evaluator(0)                             # 24 variables per node
    ev.set_mesh(9, 0.0, 4.0)
    ev.set_model_source(*chain_source(16, 8), 16, 8)
    ev.set_batch(1)
    z = lambda *s: np.zeros(s)
    with pytest.raises(E.EmiError, match="EMI_ERR_UNSUPPORTED.*16"):
        ev.kkt_blocks_host(z(1, 300, 9), z(1, ev.layout.nvals, 9), z(1, 24, 9), None, np.zeros((1, 24, 9), dtype=np.uint8))
    ev.close()
    ev = make_ev(4, 33, 3, 3)
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG"):
        ev.kkt_blocks_rows([[(4, 0)]] * 3)
    lib = E.load()
    assert lib.emi_kkt_blocks_dev(ev.ctx, *([None] * 5), 0.0, None, None, 0, *([None] * 5)) == 1      # EMI_ERR_ARG
    assert lib.emi_kkt_blocks_dev(None, *([None] * 5), 0.0, None, None, 0, *([None] * 5)) == 1
    info = C.c_int()
    assert lib.emi_kkt_factor_dev(ev.ctx, None, None, None, 0.0, C.byref(info)) == 1
    ev.close()


@pytest.mark.parametrize("M", [33, 128])
def test_factor_dev_equals_factor(built, M):
    """emi_kkt_factor_dev is emi_kkt_factor with the uploads replaced by device-to-device copies: for the same inputs the solution
    of one right-hand side is bitwise the same (here: blocks as emi_kkt_blocks_dev leaves them, J = the first ns nv rows of VALS)."""
    import torch
    nv, ns, B = 8, 6, 1
    nh = nv * (nv + 1) // 2
    ev = make_ev(nv, M, B, 0)
    case = R.make_case("inertia", nv, ns, M, B, 0, 900 + M)
    case["fixed"][:] = 0
    case["fixed"][0, :ns, 0] = 1
    for i in range(ns):                                     # the node part of the defect Jacobian carries D's diagonal
        case["VALS"][0, i * nv + i] += np.diag(ev.D)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    H, V, Sg, fx = t(case["H"]), t(case["VALS"]), t(case["Sigma"]), t(case["fixed"])
    Q = torch.zeros((B, nh, M), dtype=torch.float64, device=ev.device)
    count = torch.zeros((B,), dtype=torch.int32, device=ev.device)
    worst = torch.zeros((B,), dtype=torch.float64, device=ev.device)
    torch.cuda.synchronize()
    ev.kkt_blocks_dev(H, V, Sg, None, fx, 0.0, Q, 0, count, None, None, None, worst)
    ev.synchronize()
    rhs = np.random.default_rng(M).standard_normal((nv + ns) * M)
    assert ev.kkt_factor_dev(Q[0], V[0], fx[0], 1e-9) == 0
    x_dev = ev.kkt_solve(rhs)
    Qh = Q[0].cpu().numpy()
    assert ev.kkt_factor(Qh, case["VALS"][0, :ns * nv], case["fixed"][0].reshape(-1), 1e-9) == 0
    x_host = ev.kkt_solve(rhs)
    assert np.isfinite(x_dev).all() and np.array_equal(x_dev, x_host)
    ev.close()
