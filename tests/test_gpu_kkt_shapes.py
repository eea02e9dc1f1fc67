"""The device Newton step (csrc/emi_kkt.hip) against the dense numpy KKT matrix of test_gpu_kkt.py, where that file does not reach:
model dimensions without a compile-time node-inverse kernel (up to nv 16) and the LU beyond them, many right-hand sides in one
call, batches whose scenarios differ (mesh, fixed variables, path through the call, regularisation level, loop forms of the rocBLAS
calls), low-rank corrections with many columns in any order.  Reference: dense K from the same Q, J, fixed, dc and the context's
own D, np.linalg.solve, and the inertia from np.linalg.eigvalsh -- or, at large N, from the certificate "every corrected node block
is positive definite => K has the inertia of K~".  GPU tests are marked one by one; the model-source and mesh checks need no GPU."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from test_gpu_kkt import _random_kkt, dense_kkt

gpu = pytest.mark.gpu
EMI_ERR_ARG, EMI_ERR_UNSUPPORTED = 1, 5
DP = C.POINTER(C.c_double)


def _dp(a):
    return a.ctypes.data_as(DP)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


# ---- models and meshes that exist only for their dimensions -------------------------------------------------------------------

CHAIN_DIMS = [(1, 1), (3, 1), (5, 3), (15, 1), (16, 0), (16, 8)]


def chain_source(ns, nc):
    """A linear chain x_i' = x_(i+1), the last state driven by the first control (without controls: by -x_0), cost sum z_v^2:
    a model struct in the style of PointMass2D (csrc/emi_models.hpp) with ns states and nc controls."""
    name = f"Chain{ns}x{nc}"
    last, jlast = (f"z[{ns}]", f"J[{ns - 1}][{ns}] = T(1);") if nc else ("-z[0]", f"J[{ns - 1}][0] = T(-1);")
    src = f"""template <typename T> struct {name} {{
    static constexpr int NS = {ns}, NC = {nc}, NV = {ns + nc}, NPARAM = 0, NPATH = 0;
    EMI_DEV static void f(const ModelParams<T>&, const T* z, T, T* fo) {{
        for (int i = 0; i + 1 < NS; ++i) fo[i] = z[i + 1];
        fo[NS - 1] = {last};
    }}
    EMI_DEV static void jac(const ModelParams<T>&, const T*, T, T (*J)[NV]) {{
        for (int i = 0; i < NS; ++i)
            for (int v = 0; v < NV; ++v) J[i][v] = T(0);
        for (int i = 0; i + 1 < NS; ++i) J[i][i + 1] = T(1);
        {jlast}
    }}
    EMI_DEV static T cost(const ModelParams<T>&, const T* z, T) {{
        T s = T(0);
        for (int v = 0; v < NV; ++v) s += z[v] * z[v];
        return s;
    }}
    EMI_DEV static void grad(const ModelParams<T>&, const T* z, T, T* g) {{
        for (int v = 0; v < NV; ++v) g[v] = T(2) * z[v];
    }}
    EMI_DEV static void hess(const ModelParams<T>&, const T*, T, T cL, const T*, T* H) {{
        for (int v = 0; v < NV; ++v) H[v * (v + 1) / 2 + v] += T(2) * cL;
    }}
}};
"""
    return name, src


def cgl_mesh(M):
    """Chebyshev-Gauss-Lobatto nodes on [-1, 1] and their differentiation matrix from the barycentric formula
    D_kj = (c_j / c_k) / (x_k - x_j), D_kk = -sum_(j != k) D_kj.  The weights do not enter the KKT matrix: uniform ones."""
    j = np.arange(M)
    x = -np.cos(np.pi * j / (M - 1))
    c = np.where((j == 0) | (j == M - 1), 0.5, 1.0) * (-1.0) ** j
    dx = x[:, None] - x[None, :]
    np.fill_diagonal(dx, 1.0)
    D = (c[None, :] / c[:, None]) / dx
    np.fill_diagonal(D, 0.0)
    np.fill_diagonal(D, -D.sum(axis=1))
    return x, np.full(M, 2.0 / M), D


def test_dimension_models_pass_the_model_source_check(built):
    """Every dimension-only model of this file compiles for gfx950 against the f64 kernel templates (hiprtc needs no GPU)."""
    from etol_amd import _lib
    lib = _lib.load()
    for ns, nc in CHAIN_DIMS:
        name, src = chain_source(ns, nc)
        log = C.create_string_buffer(1 << 16)
        st = lib.emi_check_model_source(name.encode(), src.encode(), ns, nc, 0, 0, 0, log, len(log))
        assert st == 0, (ns, nc, log.value.decode(errors="replace"))


@pytest.mark.parametrize("M", [9, 33, 171])
def test_cgl_differentiation_matrix_is_exact_on_polynomials(M):
    """degree < M: D p(x) = p'(x) up to the rounding of the product (entries of D up to ~ M^2 / 3 against derivatives of 1)"""
    x, _, D = cgl_mesh(M)
    assert np.all(np.diff(x) > 0)
    for n in range(M):
        p = np.polynomial.chebyshev.Chebyshev.basis(n)
        ref = p.deriv()(x)
        assert np.abs(D @ p(x) - ref).max() < 1e-12 * (np.abs(ref).max() + np.abs(D).max()), n


# ---- helpers ------------------------------------------------------------------------------------------------------------------

def _dims(model):
    import etol_amd as E
    if isinstance(model, tuple):
        return model[0], model[0] + model[1]
    ns, nc, _ = E.model_dims(model)
    return ns, ns + nc


def _ev(M, model, mesh=None):
    import etol_amd as E
    from etol_amd import workloads as W
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, 4.0, mesh)
    if isinstance(model, tuple):
        ev.set_model_source(*chain_source(*model), *model)
    else:
        ev.set_model(model, {0: [], 1: W.QUAD_PARAMS, 2: W.FW_PARAMS}[model])
    ev.set_batch(1)
    return ev


@pytest.fixture(scope="module")
def chains(built):
    """The dimension-only models, compiled once for this module (hiprtc, a few seconds each); every later context with the same
    source takes the compiled program from the library's cache."""
    evs = [_ev(9, dims) for dims in CHAIN_DIMS]
    yield True
    for ev in evs:
        ev.close()


def _masked(b, fixed):
    b = b.copy()
    b[np.nonzero(fixed)[0]] = 0
    return b


def _assert_backward(K, x, b, what=None):
    err = np.abs(K @ x - b).max()
    assert err < 1e-10 * (np.abs(K).max() * np.abs(x).max() + 1), (what, err)


def _assert_forward(K, x, b, what=None):
    ref = np.linalg.solve(K, b)
    err = np.abs(x - ref).max()
    assert err < 1e-7 * (np.abs(ref).max() + 1), (what, err)


def _assert_refined(K, x, b, rel, what=None):
    """x from a refined solve: numpy's residual in the matrix K is at round-off and is what the device reported"""
    res = np.abs(K @ x - b).max() / max(1.0, np.abs(b).max())
    assert res < 1e-11 and abs(res - rel) < 1e-11, (what, res, rel)


def _nominal(K, nz, dc):
    """the same matrix with the multipliers' diagonal at 0 instead of -dc (the nominal dc of the refined solves)"""
    K0 = K.copy()
    idx = np.arange(nz, K.shape[0])
    K0[idx, idx] += dc
    return K0


def _lowrank(rng, M, nv, fixed, nodes, per_node, shuffle=True, scale=0.3, dscale=0.3):
    """per_node columns at each of the nodes (entries of fixed variables zero), small enough that every corrected block stays
    positive definite; in a random order unless shuffle is False"""
    node = np.repeat(np.asarray(nodes), per_node).astype(np.int32)
    vec = scale * rng.standard_normal((node.size, nv))
    for a, k in enumerate(node):
        vec[a, fixed[np.arange(nv) * M + k] != 0] = 0
    delta = dscale * (1 + rng.random(node.size))
    if shuffle:
        perm = rng.permutation(node.size)
        node, vec, delta = node[perm], vec[perm], delta[perm]
    return np.ascontiguousarray(node), np.ascontiguousarray(vec), np.ascontiguousarray(delta)


def _corrected(K, M, nv, node, vec, delta):
    K = K.copy()
    for k, u, d in zip(node, vec, delta):
        idx = np.arange(nv) * M + k
        K[np.ix_(idx, idx)] -= d * np.outer(u, u)
    return K


def _blocks_stay_definite(Q, M, nv, fixed, node, vec, delta):
    """the certificate: every corrected node block is positive definite over its free variables"""
    for k in np.unique(node):
        free = fixed[np.arange(nv) * M + k] == 0
        Qk = np.zeros((nv, nv))
        for v in range(nv):
            for q in range(v + 1):
                Qk[v, q] = Qk[q, v] = Q[v * (v + 1) // 2 + q, k]
        for a in np.nonzero(node == k)[0]:
            Qk -= delta[a] * np.outer(vec[a], vec[a])
        if np.linalg.eigvalsh(Qk[np.ix_(free, free)]).min() <= 0:
            return False
    return True


def _inertia_ok(K, nz, md):
    eig = np.linalg.eigvalsh(K)
    return (eig > 0).sum() == nz and (eig < 0).sum() == md


def _refined(lib, ev, b, dc_nominal, steps=8):
    x = b.copy()
    rel, nsv, rev, stat = C.c_double(), C.c_int(), C.c_int(), C.c_int()
    st = lib.emi_kkt_solve_refined(ev.ctx, _dp(x), float(dc_nominal), steps, C.byref(rel), C.byref(nsv), C.byref(rev), C.byref(stat))
    return st, x, rel.value, stat.value


def _factor_batch(lib, evs, probs, dcs):
    n = len(evs)
    ctxs = (C.c_void_p * n)(*[ev.ctx for ev in evs])
    Qp = (DP * n)(*[_dp(p[0]) for p in probs])
    Jp = (DP * n)(*[_dp(p[1]) for p in probs])
    Fp = (C.POINTER(C.c_ubyte) * n)(*[p[2].ctypes.data_as(C.POINTER(C.c_ubyte)) for p in probs])
    dcs = np.ascontiguousarray(dcs, dtype=np.float64)
    info = np.full(n, -7, dtype=np.int32)
    st = lib.emi_kkt_factor_batch(n, ctxs, Qp, Jp, Fp, _dp(dcs), _ip(info))
    return st, info


def _solve_batch(lib, evs, rhs):
    n = len(evs)
    work = [r.copy() for r in rhs]
    ctxs = (C.c_void_p * n)(*[ev.ctx for ev in evs])
    Rp = (DP * n)(*[_dp(w) for w in work])
    return lib.emi_kkt_solve_batch(n, ctxs, Rp), work


def _refined_batch(lib, evs, rhs, dcs, steps=8):
    n = len(evs)
    work = [r.copy() for r in rhs]
    ctxs = (C.c_void_p * n)(*[ev.ctx for ev in evs])
    Rp = (DP * n)(*[_dp(w) for w in work])
    dcs = np.ascontiguousarray(dcs, dtype=np.float64)
    rel = np.zeros(n)
    nsv, rev, stat = (np.zeros(n, dtype=np.int32) for _ in range(3))
    st = lib.emi_kkt_solve_refined_batch(n, ctxs, Rp, _dp(dcs), steps, _dp(rel), _ip(nsv), _ip(rev), _ip(stat))
    return st, work, rel, stat


@contextlib.contextmanager
def _refine_to_round_off(ev):
    """the process-wide "kkt_refine_exp" at 14 inside, at its default 10 afterwards"""
    ev.set_option("kkt_refine_exp", 14)
    try:
        yield
    finally:
        ev.set_option("kkt_refine_exp", 10)


def _batch_roundtrip(lib, evs, probs, M, ns, nv, rng, lowrank=None, rhs=None):
    """emi_kkt_factor_batch, emi_kkt_solve_batch and emi_kkt_solve_refined_batch of n scenarios, each against numpy with ITS own
    matrix (own D, fixed mask, low-rank correction) and against the single entry points.  lowrank: {scenario: (node, vec, delta)}.
    Returns (batched solutions, emi_kkt_is_schur per scenario)."""
    n, N, nz = len(evs), (nv + ns) * M, nv * M
    st, info = _factor_batch(lib, evs, probs, np.full(n, 1e-9))
    assert st == 0, lib.emi_last_error(evs[0].ctx)
    assert np.all(info == 0), info
    schur = [lib.emi_kkt_is_schur(ev.ctx) for ev in evs]
    Ks = []
    for b, (ev, p) in enumerate(zip(evs, probs)):
        K = dense_kkt(ev.D, *p, 1e-9, M, ns, nv)
        if lowrank and b in lowrank:
            assert ev.kkt_lowrank(*lowrank[b])
            K = _corrected(K, M, nv, *lowrank[b])
        Ks.append(K)
    if rhs is None:
        rhs = [rng.standard_normal(N) for _ in range(n)]
    st, work = _solve_batch(lib, evs, rhs)
    assert st == 0, lib.emi_last_error(evs[0].ctx)
    for b in range(n):
        ref = _masked(rhs[b], probs[b][2])
        _assert_backward(Ks[b], work[b], ref, b)
        _assert_forward(Ks[b], work[b], ref, b)
        single = evs[b].kkt_solve(rhs[b])
        assert np.abs(work[b] - single).max() < 1e-9 * (np.abs(single).max() + 1), b
    sch = [b for b in range(n) if schur[b]]
    if sch:
        with _refine_to_round_off(evs[0]):
            st, xr, rel, stat = _refined_batch(lib, [evs[b] for b in sch], [rhs[b] for b in sch], np.zeros(len(sch)))
        assert st == 0, lib.emi_last_error(evs[sch[0]].ctx)
        assert np.all(stat == 0), stat
        for i, b in enumerate(sch):
            _assert_refined(_nominal(Ks[b], nz, 1e-9), xr[i], _masked(rhs[b], probs[b][2]), rel[i], b)
    return work, schur


# ---- A. model dimensions ------------------------------------------------------------------------------------------------------

SHAPES = [(2, 9), (2, 33), (2, 86), (2, 129), ((1, 1), 1031), ((3, 1), 343), ((5, 3), 207), ((15, 1), 69), ((16, 0), 65)]


@gpu
@pytest.mark.parametrize("model,M", SHAPES, ids=[f"{m if isinstance(m, int) else '%dx%d' % m}-{M}" for m, M in SHAPES])
def test_model_dimensions_match_numpy(built, chains, model, M):
    """Both methods, three right-hand sides in one call, a low-rank correction with two columns at each of ~8 nodes (in a random
    order) and the device refinement, for the built-in fixed-wing model (ns 12, nv 16: the generic node-inverse kernels at their
    largest; ns M = 1032 at 86 nodes: two-level Cholesky, block inverses, an 8-row tail) and for chains whose node blocks have no
    compile-time kernel (nv 4 with ns 3, nv 8 with ns 5, nv 16 with 120 and with 136 state pairs; ns M just over 1024)."""
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = _dims(model)
    N, nz, md = (nv + ns) * M, nv * M, ns * M
    rng = np.random.default_rng(31 * M + nv)
    ev = _ev(M, model)
    Q, J, F = _random_kkt(ev, M, ns, nv, rng)
    if nv == ns:
        # no controls: J is square -- fixed initial states would leave K singular up to dc, and a node part of unit size next to D
        # leaves K conditioned at ~2e9 (|x| ~ 1e8 |b|: beyond the forward-error bound and the refined solves' 1e-11); x100: ~5e6
        F[:] = 0
        for i in range(ns):
            J[i * nv + i] = 100 * (J[i * nv + i] - np.diag(ev.D)) + np.diag(ev.D)
            J[i * nv:i * nv + i] *= 100
            J[i * nv + i + 1:(i + 1) * nv] *= 100
    K = dense_kkt(ev.D, Q, J, F, 1e-9, M, ns, nv)
    B = rng.standard_normal((3, N))
    Bm = np.array([_masked(b, F) for b in B])
    node, vec, delta = _lowrank(rng, M, nv, F, np.arange(1, M, max(1, M // 8)), 2)
    Kc = _corrected(K, M, nv, node, vec, delta)
    assert _blocks_stay_definite(Q, M, nv, F, node, vec, delta)
    if N <= 1600:
        assert _inertia_ok(Kc, nz, md)
    try:
        for method in (1, 0):
            ev.set_option("kkt_method", method)
            assert ev.kkt_factor(Q, J, F, 1e-9) == 0
            assert lib.emi_kkt_is_schur(ev.ctx) == method
            X = ev.kkt_solve(B)
            for b, x in zip(Bm, X):
                _assert_backward(K, x, b, method)
            _assert_forward(K, X[0], Bm[0], method)
            assert ev.kkt_lowrank(node, vec, delta) is True
            Xc = ev.kkt_solve(B)
            for b, x in zip(Bm, Xc):
                _assert_backward(Kc, x, b, method)
            _assert_forward(Kc, Xc[1], Bm[1], method)
            with _refine_to_round_off(ev):
                st, x, rel, stat = _refined(lib, ev, B[2], 0.0)
            if method == 1:
                assert st == 0 and stat == 0, lib.emi_last_error(ev.ctx)
                _assert_refined(_nominal(Kc, nz, 1e-9), x, Bm[2], rel)
            else:
                assert st == EMI_ERR_UNSUPPORTED
    finally:
        ev.set_option("kkt_method", 1)
    ev.close()


@gpu
@pytest.mark.parametrize("model,M", [(2, 65), (2, 129), ((15, 1), 69)], ids=["2-65", "2-129", "15x1-69"])
def test_batched_model_dimensions_match_numpy_and_the_single_path(built, chains, model, M):
    """Three scenarios with nv 16 through the batched factorisation, solve and refinement (the generic batched node-inverse
    kernel), one of them with a low-rank correction."""
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = _dims(model)
    rng = np.random.default_rng(4100 + M + nv)
    evs = [_ev(M, model) for _ in range(3)]
    probs = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    lr = {1: _lowrank(rng, M, nv, probs[1][2], [2, M // 2, M - 1], 3)}
    _, schur = _batch_roundtrip(lib, evs, probs, M, ns, nv, rng, lowrank=lr)
    assert schur == [1, 1, 1]
    for ev in evs:
        ev.close()


@gpu
def test_more_than_16_variables_per_node_take_the_lu(built, chains):
    """Traced (16, 8), nv 24: the single factorisation takes the LU and solves against numpy; a low-rank correction of 256 columns
    (8 at each of 32 nodes) gives Woodbury solves of the corrected matrix; the device refinement is not offered; the batched
    factorisation hands every scenario to the single path, and the batched solve follows it."""
    from etol_amd import _lib as L
    lib = L.load()
    model, M = (16, 8), 33
    ns, nv = _dims(model)
    N, nz, md = (nv + ns) * M, nv * M, ns * M
    rng = np.random.default_rng(1624)
    evs = [_ev(M, model) for _ in range(3)]
    probs = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    ev = evs[0]
    Q, J, F = probs[0]
    assert ev.kkt_factor(Q, J, F, 1e-9) == 0
    assert lib.emi_kkt_is_schur(ev.ctx) == 0
    K = dense_kkt(ev.D, Q, J, F, 1e-9, M, ns, nv)
    B = rng.standard_normal((3, N))
    Bm = np.array([_masked(b, F) for b in B])
    X = ev.kkt_solve(B)
    for b, x in zip(Bm, X):
        _assert_backward(K, x, b)
    _assert_forward(K, X[0], Bm[0])
    node, vec, delta = _lowrank(rng, M, nv, F, np.arange(32), 8, scale=0.2, dscale=0.2)
    assert node.size == 256
    assert _blocks_stay_definite(Q, M, nv, F, node, vec, delta)
    Kc = _corrected(K, M, nv, node, vec, delta)
    assert _inertia_ok(Kc, nz, md)
    assert ev.kkt_lowrank(node, vec, delta) is True
    Xc = ev.kkt_solve(B)
    for b, x in zip(Bm, Xc):
        _assert_backward(Kc, x, b)
    _assert_forward(Kc, Xc[0], Bm[0])
    st, *_ = _refined(lib, ev, B[0], 1e-9)
    assert st == EMI_ERR_UNSUPPORTED
    st, info = _factor_batch(lib, evs, probs, np.full(3, 1e-9))
    assert st == 0, lib.emi_last_error(ev.ctx)
    assert np.all(info == 0), info
    assert [lib.emi_kkt_is_schur(e.ctx) for e in evs] == [0, 0, 0]
    rhs = [rng.standard_normal(N) for _ in evs]
    st, work = _solve_batch(lib, evs, rhs)
    assert st == 0, lib.emi_last_error(ev.ctx)
    for e, p, r, x in zip(evs, probs, rhs, work):
        Kb = dense_kkt(e.D, *p, 1e-9, M, ns, nv)
        _assert_backward(Kb, x, _masked(r, p[2]))
        _assert_forward(Kb, x, _masked(r, p[2]))
    for e in evs:
        e.close()


@gpu
@pytest.mark.parametrize("model,M", [(2, 86), (1, 171)], ids=["2-86", "1-171"])
def test_many_right_hand_sides_in_one_call(built, model, M):
    """nrhs 1 (block-inverse gemv solves), 7 (one GEMM per right-hand side, rocsolver dpotrs), 8 and 15 (GEMMs batched over the
    states), 16 and 64 (blk_potrs_multi) in one emi_kkt_solve call each; again with a low-rank correction active, where 65 right-hand
    sides are refused with EMI_ERR_ARG."""
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = _dims(model)
    N = (nv + ns) * M
    rng = np.random.default_rng(6400 + M)
    ev = _ev(M, model)
    Q, J, F = _random_kkt(ev, M, ns, nv, rng)
    assert ev.kkt_factor(Q, J, F, 1e-9) == 0
    assert lib.emi_kkt_is_schur(ev.ctx) == 1
    K = dense_kkt(ev.D, Q, J, F, 1e-9, M, ns, nv)
    B = rng.standard_normal((65, N))
    Bm = np.array([_masked(b, F) for b in B])
    node, vec, delta = _lowrank(rng, M, nv, F, np.arange(0, M, 7), 3)
    assert _blocks_stay_definite(Q, M, nv, F, node, vec, delta)
    Kc = _corrected(K, M, nv, node, vec, delta)
    for Kref, corrected in ((K, False), (Kc, True)):
        if corrected:
            assert ev.kkt_lowrank(node, vec, delta) is True
        first = None
        for nrhs in (1, 7, 8, 15, 16, 64):
            X = ev.kkt_solve(B[:nrhs])
            R = Kref @ X.T - Bm[:nrhs].T
            bound = 1e-10 * (np.abs(Kref).max() * np.abs(X).max(axis=1) + 1)
            assert np.all(np.abs(R).max(axis=0) < bound), (corrected, nrhs)
            _assert_forward(Kref, X[-1], Bm[nrhs - 1], (corrected, nrhs))
            if first is None:
                first = X[0]
            assert np.abs(X[0] - first).max() < 1e-9 * (np.abs(first).max() + 1), (corrected, nrhs)
    many = B.copy()
    assert lib.emi_kkt_solve(ev.ctx, _dp(many), 65) == EMI_ERR_ARG
    ev.close()


# ---- B. batches whose scenarios differ ----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("M", [33, 171])
def test_batch_of_different_meshes_with_the_same_node_count(built, M):
    """LGL and Chebyshev-Gauss-Lobatto contexts with the same M in one batch: each scenario is factorised, solved and refined with
    its OWN differentiation matrix."""
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = 6, 8
    rng = np.random.default_rng(500 + M)
    evs = [_ev(M, 1), _ev(M, 1, cgl_mesh(M)), _ev(M, 1)]
    assert np.abs(evs[1].D - evs[0].D).max() > 1e-3
    probs = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    lr = {1: _lowrank(rng, M, nv, probs[1][2], [1, M // 3], 2)}
    _, schur = _batch_roundtrip(lib, evs, probs, M, ns, nv, rng, lowrank=lr)
    assert schur == [1, 1, 1]
    for ev in evs:
        ev.close()


@gpu
@pytest.mark.parametrize("M", [33, 171])
def test_batch_with_per_scenario_fixed_variables(built, M):
    """Scenario 0 fixes the initial states, 1 also the end-node states and the first control at every node, 2 every variable of
    one interior node (its inverse node block is all zero)."""
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = 6, 8
    rng = np.random.default_rng(600 + M)
    evs = [_ev(M, 1) for _ in range(3)]
    probs = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    probs[1][2][np.arange(ns) * M + M - 1] = 1
    probs[1][2][ns * M:(ns + 1) * M] = 1
    probs[2][2][np.arange(nv) * M + M // 2] = 1
    _, schur = _batch_roundtrip(lib, evs, probs, M, ns, nv, rng)
    assert schur == [1, 1, 1]
    for ev in evs:
        ev.close()


@gpu
@pytest.mark.parametrize("M", [33, 171])
def test_scenarios_leave_the_batch_at_the_front_and_in_the_middle(built, M):
    """Indefinite node blocks in scenarios 0 and 2 of 4: those two take the single path (LU) inside the call, the others stay
    batched; every scenario solves its own matrix."""
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = 6, 8
    rng = np.random.default_rng(700 + M)
    evs = [_ev(M, 1) for _ in range(4)]
    probs = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    for b in (0, 2):
        probs[b][0][0, min(3, M - 1)] = -5.0
    _, schur = _batch_roundtrip(lib, evs, probs, M, ns, nv, rng)
    assert schur == [0, 1, 0, 1]
    for ev in evs:
        ev.close()


def _regularisation(lib, ev):
    dc, dw = C.c_double(), C.c_double()
    assert lib.emi_kkt_last_regularisation(ev.ctx, C.byref(dc), C.byref(dw)) == 0
    return dc.value, dw.value


def _regularised(ev, prob, dc, dw, M, ns, nv):
    """the matrix a factorisation with (dc, dw) holds: dw on the diagonal of the free state variables"""
    Q = prob[0].copy()
    for v in range(ns):
        Q[v * (v + 1) // 2 + v] += dw
    return dense_kkt(ev.D, Q, prob[1], prob[2], dc, M, ns, nv)


@gpu
@pytest.mark.parametrize("M", [33, 171])
def test_batch_with_mixed_regularisation_levels(built, M):
    """One scenario with next to no state curvature between regular ones.  The regular ones report the nominal level and solve
    exactly the matrix they report; the refinement brings them to round-off in their NOMINAL matrix and reports the flat one's
    residual as numpy sees it.  A second batch of benign matrices on the same contexts (the flat one's context starts from its
    sticky level) again solves exactly what each scenario reports, and refines to round-off."""
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = 6, 8
    nh, N = nv * (nv + 1) // 2, (nv + ns) * M
    rng = np.random.default_rng(800 + M)
    evs = [_ev(M, 1) for _ in range(3)]
    probs = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    Jf = 0.01 * rng.standard_normal((ns * nv, M))
    for i in range(ns):
        Jf[i * nv + i] += np.diag(evs[1].D)
    Qf = np.zeros((nh, M))
    for v in range(nv):
        Qf[v * (v + 1) // 2 + v] = 1e-12 if v < ns else 1.0
    probs[1] = (Qf, Jf, probs[1][2])
    rhs = [rng.standard_normal(N) for _ in range(3)]
    st, info = _factor_batch(lib, evs, probs, np.zeros(3))
    assert st == 0 and np.all(info == 0), (st, info)
    regs = [_regularisation(lib, ev) for ev in evs]
    print("regularisation (dc, dw) per scenario:", regs)
    assert regs[0] == regs[2] == (1e-9, 0.0)
    assert regs[1][0] >= 1e-9 and regs[1][1] >= 0.0
    st, work = _solve_batch(lib, evs, rhs)
    assert st == 0
    for b in (0, 2):
        _assert_backward(_regularised(evs[b], probs[b], *regs[b], M, ns, nv), work[b], _masked(rhs[b], probs[b][2]), b)
    with _refine_to_round_off(evs[0]):
        st, xr, rel, stat = _refined_batch(lib, evs, rhs, np.zeros(3))
    assert st == 0 and np.all(stat == 0)
    for b in range(3):
        K0 = dense_kkt(evs[b].D, *probs[b], 0.0, M, ns, nv)
        ref = _masked(rhs[b], probs[b][2])
        if b == 1:
            res = np.abs(K0 @ xr[b] - ref).max() / max(1.0, np.abs(ref).max())
            assert abs(res - rel[b]) <= 1e-6 * max(res, rel[b]) + 1e-13, (res, rel[b])
        else:
            _assert_refined(K0, xr[b], ref, rel[b], b)
    # benign matrices on the same contexts
    probs2 = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    st, info = _factor_batch(lib, evs, probs2, np.zeros(3))
    assert st == 0 and np.all(info == 0), (st, info)
    st, work = _solve_batch(lib, evs, rhs)
    assert st == 0
    for b, ev in enumerate(evs):
        reg = _regularisation(lib, ev)
        _assert_backward(_regularised(ev, probs2[b], *reg, M, ns, nv), work[b], _masked(rhs[b], probs2[b][2]), (b, reg))
    with _refine_to_round_off(evs[0]):
        st, xr, rel, stat = _refined_batch(lib, evs, rhs, np.zeros(3))
    assert st == 0 and np.all(stat == 0)
    for b in range(3):
        K0 = dense_kkt(evs[b].D, *probs2[b], 0.0, M, ns, nv)
        _assert_refined(K0, xr[b], _masked(rhs[b], probs2[b][2]), rel[b], b)
    for ev in evs:
        ev.close()


@gpu
def test_batch_loop_forms_match_numpy_and_the_batched_forms(built):
    """"kkt_batch_gemm_rows" / "kkt_batch_syrk_rows" / "kkt_batch_trtri_rows" 1: the rocBLAS calls of the batched factorisation go
    out once per scenario (the forms for large meshes) -- numpy's solutions, and those of the *_batched forms."""
    from etol_amd import _lib as L
    lib = L.load()
    M, ns, nv = 171, 6, 8
    N = (nv + ns) * M
    rng = np.random.default_rng(171)
    evs = [_ev(M, 1) for _ in range(3)]
    probs = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    rhs = [rng.standard_normal(N) for _ in range(3)]
    try:
        for name in ("kkt_batch_gemm_rows", "kkt_batch_syrk_rows", "kkt_batch_trtri_rows"):
            evs[0].set_option(name, 1)
        loops, _ = _batch_roundtrip(lib, evs, probs, M, ns, nv, rng, rhs=rhs)
    finally:
        evs[0].set_option("kkt_batch_gemm_rows", 1 << 30)
        evs[0].set_option("kkt_batch_syrk_rows", 3072)
        evs[0].set_option("kkt_batch_trtri_rows", 3072)
    batched, _ = _batch_roundtrip(lib, evs, probs, M, ns, nv, rng, rhs=rhs)
    for a, b in zip(loops, batched):
        assert np.abs(a - b).max() < 1e-9 * (np.abs(b).max() + 1)
    for ev in evs:
        ev.close()


@gpu
@pytest.mark.parametrize("M", [33, 171])
def test_batch_of_one_equals_the_single_path(built, M):
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = 6, 8
    rng = np.random.default_rng(900 + M)
    ev = _ev(M, 1)
    prob = _random_kkt(ev, M, ns, nv, rng)
    b = rng.standard_normal((nv + ns) * M)
    xb, _ = _batch_roundtrip(lib, [ev], [prob], M, ns, nv, rng, rhs=[b])
    one = _ev(M, 1)
    assert one.kkt_factor(*prob, dc=1e-9) == 0
    x1 = one.kkt_solve(b)
    assert np.abs(xb[0] - x1).max() < 1e-9 * (np.abs(x1).max() + 1)
    one.close()
    ev.close()


# ---- C. low-rank corrections --------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("M", [33, 171])
def test_lowrank_columns_in_any_order(built, M):
    """Three columns at each of five nodes, given in a random order (not grouped by node): single, batched and refined solves
    (single and batched) against numpy, and the same x as from the columns sorted by node."""
    from etol_amd import _lib as L
    lib = L.load()
    ns, nv = 6, 8
    N, nz = (nv + ns) * M, nv * M
    rng = np.random.default_rng(1000 + M)
    evs = [_ev(M, 1) for _ in range(2)]
    probs = [_random_kkt(ev, M, ns, nv, rng) for ev in evs]
    nodes = [1, 5, M // 2, M - 9, M - 2]
    lr = {b: _lowrank(rng, M, nv, probs[b][2], nodes, 3) for b in range(2)}
    for node, _, _ in lr.values():
        assert any(np.ptp(np.nonzero(node == k)[0]) > 2 for k in nodes)        # some node's columns are not adjacent
    rhs = [rng.standard_normal(N) for _ in range(2)]
    _batch_roundtrip(lib, evs, probs, M, ns, nv, rng, lowrank=lr, rhs=rhs)
    ev, (Q, J, F) = evs[0], probs[0]
    Kc = _corrected(dense_kkt(ev.D, Q, J, F, 1e-9, M, ns, nv), M, nv, *lr[0])
    b = _masked(rhs[0], F)
    x_plain = ev.kkt_solve(rhs[0])
    _assert_backward(Kc, x_plain, b)
    with _refine_to_round_off(ev):
        st, x_ref, rel, stat = _refined(lib, ev, rhs[0], 0.0)
        assert st == 0 and stat == 0
        _assert_refined(_nominal(Kc, nz, 1e-9), x_ref, b, rel)
        order = np.argsort(lr[0][0], kind="stable")
        assert ev.kkt_lowrank(*(np.ascontiguousarray(a[order]) for a in lr[0])) is True
        x_sorted = ev.kkt_solve(rhs[0])
        st, x_ref_sorted, _, _ = _refined(lib, ev, rhs[0], 0.0)
        assert st == 0
    assert np.abs(x_sorted - x_plain).max() <= 1e-12 * np.abs(x_plain).max()
    assert np.abs(x_ref_sorted - x_ref).max() <= 1e-12 * np.abs(x_ref).max()
    for e in evs:
        e.close()


@gpu
def test_refined_solve_with_more_than_4096_lowrank_columns(built):
    """Quadrotor at 520 nodes with 8 columns at every node (r = 4160), every corrected block positive definite so that the verdict
    must be exact: the refinement's residual covers every column (the reported rel is numpy's), and x solves the corrected
    matrix."""
    from etol_amd import _lib as L
    lib = L.load()
    M, ns, nv = 520, 6, 8
    N, nz = (nv + ns) * M, nv * M
    rng = np.random.default_rng(4160)
    ev = _ev(M, 1)
    Q, J, F = _random_kkt(ev, M, ns, nv, rng)
    node, vec, delta = _lowrank(rng, M, nv, F, np.arange(M), 8, shuffle=False, scale=0.2, dscale=0.2)
    assert node.size == 4160
    assert _blocks_stay_definite(Q, M, nv, F, node, vec, delta)
    assert ev.kkt_factor(Q, J, F, 1e-9) == 0
    assert ev.kkt_lowrank(node, vec, delta) is True
    K0 = _nominal(_corrected(dense_kkt(ev.D, Q, J, F, 1e-9, M, ns, nv), M, nv, node, vec, delta), nz, 1e-9)
    rhs = rng.standard_normal(N)
    with _refine_to_round_off(ev):
        st, x, rel, stat = _refined(lib, ev, rhs, 0.0)
    assert st == 0 and stat == 0, lib.emi_last_error(ev.ctx)
    _assert_refined(K0, x, _masked(rhs, F), rel)
    ev.close()
