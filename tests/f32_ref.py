"""Reference pieces for the fp32 context (config 5): numpy only, nothing of the library's arithmetic.

What an fp32 context computes in its defect rows is  R0 + Df . x  with Df its f32 copy of the differentiation matrix, by one of
two routes: the fallback kernel (f32 operands, exact products, f64 accumulation, one rounding at the store) and the MFMA kernels
(the shifted-difference form: every 32-column tile contracts D with x_j - x[tile centre] in f32).  This module restates Df,
derives a rigorous bound for the first route, emulates both routes on the CPU, and generates the seeded inputs that
tests/test_f32_ref_cpu.py (no GPU) and tests/test_gpu_f32.py share -- so that the reference alone is shown to stay inside every
defect-row tolerance before a kernel is held to it.
"""
import numpy as np

import cases
import oracle_lib as O
from etol_amd import _lib as L
from etol_amd import workloads as W

U32 = 2.0 ** -24            # unit roundoff of f32 (round to nearest)
TOL_F32 = 2e-6              # the project's fp32 class: defect rows at M <= 512, path rows, VALS entries, COST (test_f32_context_fixedwing)

NS = {L.MODEL_POINTMASS2D: 2, L.MODEL_QUADROTOR2D: 6, L.MODEL_FIXEDWING12: 12}


def to_f32(a):
    """What an fp32 context sees of a host array: every input goes through this before the device AND the oracle get it."""
    return np.ascontiguousarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def f32_operator(D):
    """The context's f32 copy of D (returned as float64 values that are f32-representable): off-diagonals rounded to f32, diagonal =
    f32 of minus the f64 sum (in column order) of the ROUNDED off-diagonals.  Restated from the comment of upload_operator in
    csrc/emi_api.hip; the rows sum to zero up to the one rounding of the diagonal, which the shifted-difference form relies on."""
    D = np.asarray(D, dtype=np.float64)
    M = D.shape[0]
    Df = D.astype(np.float32).astype(np.float64)
    for i in range(M):
        rs = 0.0
        for j in range(M):
            if j != i:
                rs += Df[i, j]
        Df[i, i] = np.float64(np.float32(-rs))
    return Df


def exact_defect(D, X, R0):
    """R0 + D . X in long double from the f64 matrix (the oracle's own arithmetic for this product): [B][ns][M]."""
    Dl, Xl = np.asarray(D, dtype=np.longdouble), np.asarray(X, dtype=np.longdouble)
    return np.asarray(R0, dtype=np.longdouble) + np.matmul(Xl, Dl.T)


def abs_product(D, X):
    """sum_j |D_kj| |x_j| : [B][ns][M]"""
    return np.matmul(np.abs(np.asarray(X, dtype=np.float64)), np.abs(np.asarray(D, dtype=np.float64)).T)


def fallback_bound(D, X, R0):
    """Elementwise bound on |fallback kernel - (R0 + D x)_k| for f32-representable X and R0, u = 2^-24:

        u ( sum_j |D_kj||x_j|  +  |x_k| sum_j |D_kj|  +  |R0 + (D x)_k| )  +  M 2^-52 sum_j |D_kj||x_j|

    The kernel multiplies f32 operands exactly (24 x 24 bits fit a double), sums them in f64 and rounds once at the store.
      1. Off-diagonals: |Df_kj - D_kj| <= u |D_kj|, so their part of the product is off by at most u sum_{j != k} |D_kj||x_j|.
      2. Diagonal: Df_kk = fl32(-sum_{j != k} Df_kj) carries the off-diagonals' roundings (u sum_{j != k} |D_kj|) plus its own
         (u |D_kk|, D's rows summing to zero): |Df_kk - D_kk| |x_k| <= u |x_k| sum_j |D_kj|.
      3. The store rounds R0 + acc once: u |R0 + (D x)_k|.
      4. The f64 sum of M + 1 terms: at most M 2^-53 sum |terms| to first order; 2^-52 leaves room for |Df| <= (1 + u)|D| and for
         the row-sum residual of the f64 D itself (~1e-16 sum_j |D_kj|).
    Second-order terms (u^2) sit under the j = k summand of term 1, which step 1 does not use.  No margin: the CPU emulation
    (tests/test_f32_ref_cpu.py) has to stay inside as it stands."""
    D = np.asarray(D, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    M = D.shape[0]
    ax = abs_product(D, X)
    rowabs = np.abs(D).sum(axis=1)
    ref = np.abs(np.asarray(exact_defect(D, X, R0), dtype=np.float64))
    return U32 * (ax + np.abs(X) * rowabs + ref) + M * 2.0 ** -52 * ax


def row_scale(D, X, ref):
    """The project's scale of an fp32 defect row element: sum_j |D_kj||x_j| + |ref| + 1 (test_f32_context_fixedwing)."""
    return abs_product(D, X) + np.abs(np.asarray(ref, dtype=np.float64)) + 1.0


def emulate_fallback(Df, X, R0):
    """The fallback kernel in numpy: f64 sum of the exact products of f32 operands, added to R0 in f64, rounded to f32."""
    acc = np.einsum("kj,bij->bik", np.asarray(Df, dtype=np.float64), np.asarray(X, dtype=np.float64))
    return (np.asarray(R0, dtype=np.float64) + acc).astype(np.float32).astype(np.float64)


def emulate_shifted(Df, X, R0):
    """The shifted-difference form in numpy, in f32 throughout: for output node k in the 32-column tile [t0, t0 + 32) the
    contraction runs over x_j - x[t0 + 16]; every product is rounded to f32 and added to an f32 running sum SEQUENTIALLY over j
    (the least favourable order: the matrix cores pair and tree-add some of it); R0 is added last, in f32."""
    Df32 = np.asarray(Df, dtype=np.float32)
    X32 = np.asarray(X, dtype=np.float32)
    M = Df32.shape[0]
    assert M % 32 == 0
    centre = 32 * (np.arange(M) // 32) + 16
    S = X32[..., centre]                                 # [B][ns][M]: the shift of output column k
    acc = np.zeros(X32.shape, dtype=np.float32)
    for j in range(M):
        d = X32[..., j:j + 1] - S                        # f32 subtraction
        acc = acc + d * Df32[:, j]                       # f32 product, then f32 sum (numpy does not fuse them)
    return (np.asarray(R0, dtype=np.float32) + acc).astype(np.float64)


# ---- seeded inputs, as the device sees them ---------------------------------------------------------------------------------
_MESH = {}


def mesh(M):
    """(tau, w, D) of the oracle's LGL mesh; the evaluators are given this mesh too, so both sides hold the same D"""
    if M not in _MESH:
        _MESH[M] = O.lgl(M)
    return _MESH[M]


def start_rows(seed, shape):
    """Random f32-representable starting rows R0 (the res_in of an EVAL_DEFECT call)"""
    return to_f32(np.random.default_rng(seed).uniform(-50.0, 50.0, shape))


QUAD, FW, PM = L.MODEL_QUADROTOR2D, L.MODEL_FIXEDWING12, L.MODEL_POINTMASS2D
QUAD_SEED, FW_SEED = 7, 4
PARAMS = {QUAD: W.QUAD_PARAMS, FW: W.FW_PARAMS, PM: []}


def model_batch(model, B, M, nobs=0):
    """-> X, U, recs (None without obstacles): quadrotor seed 7 / fixed wing seed 4, through to_f32"""
    if model == QUAD:
        X, U, recs = W.quadrotor_batch(QUAD_SEED, B, M, nobs)
        return to_f32(X), to_f32(U), (to_f32(recs) if nobs else None)
    assert model == FW and nobs == 0
    X, U = W.fixedwing_batch(FW_SEED, B, M)
    return to_f32(X), to_f32(U), None


def defect_case(model, B, M):
    """Inputs of an isolated-defect-kernel case: X, U, R0 ([B][ns][M]; no path rows)"""
    X, U, _ = model_batch(model, B, M)
    return X, U, start_rows(1000 * model + 10 * B + M, X.shape)


# the (model, batch) pairs behind the row counts R of the isolated-kernel cases
ROWS = {6: (QUAD, 1), 36: (FW, 3), 114: (QUAD, 19), 168: (FW, 14), 192: (FW, 16), 228: (FW, 19)}
FALLBACK_M = (2, 17, 50, 129, 200, 256)
FALLBACK_R = (6, 36, 114)
SHIFTED_M = (128, 256, 384, 512)


def constant_rows(B, ns, M):
    """X constant along the nodes of each row, a different f32 constant per row, 1e6 and a negative value among them"""
    c = np.random.default_rng(77).uniform(-300.0, 300.0, B * ns)
    c[0], c[1], c[2] = 1.0e6, -123.456, 0.1
    return np.repeat(to_f32(c).reshape(B, ns, 1), M, axis=2)


def whole_pass_case(name):
    """Inputs of a whole-pass case, everything the device sees through to_f32:
    dict(model, params, M, B, t0, tf, X, U, recs (or None), tracks (or None), maximize)"""
    def quad(M, B, nobs, t0, tf, shared=False, seed=QUAD_SEED, maximize=False):
        X, U, recs = W.quadrotor_batch(seed, B, M, nobs)
        recs = to_f32(recs[:1] if shared else recs) if nobs else None
        return dict(model=QUAD, params=W.QUAD_PARAMS, M=M, B=B, t0=t0, tf=tf, X=to_f32(X), U=to_f32(U), recs=recs, tracks=None,
                    maximize=maximize)

    if name == "pointmass_xml":                 # the shipped problem: M = 33, B = 2, 9 ellipse rows + 2 track rows
        c = cases.case_inputs("pointmass_xml")
        node_t = c["t0"] + (c["tf"] - c["t0"]) / 2.0 * (mesh(c["M"])[0] + 1.0)
        recs, tx, ty = cases.ocp2d_tables(O.edge_ellipse, O.track_centres, node_t)
        return dict(model=PM, params=[], M=c["M"], B=c["B"], t0=c["t0"], tf=c["tf"], X=to_f32(c["X"]), U=to_f32(c["U"]),
                    recs=to_f32(recs), tracks=(to_f32(tx), to_f32(ty)), maximize=False)
    if name == "quad_ragged":                   # M = 50, B = 19, one shared obstacle set
        return quad(50, 19, 3, 0.5, 9.0, shared=True)
    if name == "quad_tiny":                     # M = 2, B = 1
        return quad(2, 1, 0, 0.0, 1.0, seed=8)
    if name == "quad_128_obs":                  # three obstacles PER INSTANCE
        return quad(128, 5, 3, 0.0, W.TF)
    if name == "quad_384_obs":
        return quad(384, 19, 3, 0.0, W.TF)
    if name == "quad_128_max":
        return quad(128, 5, 3, 0.0, W.TF, maximize=True)
    if name == "fixedwing_384":
        X, U, _ = model_batch(FW, 14, 384)
        return dict(model=FW, params=W.FW_PARAMS, M=384, B=14, t0=0.0, tf=20.0, X=X, U=U, recs=None, tracks=None, maximize=False)
    if name == "fixedwing_64":
        X, U, _ = model_batch(FW, 2, 64)
        return dict(model=FW, params=W.FW_PARAMS, M=64, B=2, t0=0.0, tf=20.0, X=X, U=U, recs=None, tracks=None, maximize=False)
    raise KeyError(name)


def oracle_pass(c):
    """oracle_lib.evaluate on a whole_pass_case"""
    return O.evaluate(c["model"], c["params"], c["M"], mesh(c["M"]), c["t0"], c["tf"], c["X"], c["U"], c["recs"], c["tracks"],
                      maximize=c["maximize"])


def multipliers(c, seed=11):
    """Seeded multipliers of a whole_pass_case through to_f32: lamF [B][ns][M], lamC [B][np][M]"""
    rng = np.random.default_rng(seed)
    npth = 0 if c["recs"] is None else c["recs"].shape[-2]
    return to_f32(rng.standard_normal(c["X"].shape)), to_f32(rng.standard_normal((c["B"], npth, c["M"])))


SIGMA = 0.75


def oracle_hessian(c, lamF, lamC, sigma):
    return O.hessian(c["model"], c["params"], c["M"], mesh(c["M"]), c["t0"], c["tf"], c["X"], c["U"], lamF, lamC, sigma,
                     c["recs"], c["tracks"], maximize=c["maximize"])


def hessian_reference(c, lamF, lamC, sigma=SIGMA):
    """-> (Href, T): the oracle's Hessian and the term scale T = |sigma||H_cost| + sum_i |lam_i||H_i| built from unit-multiplier
    oracle calls (the Hessian is linear in (sigma, lamF, lamC) and node-local, so a call with lam_i = 1 at every node gives H_i
    at every node): ns + np + 1 calls."""
    ns, npth = lamF.shape[1], lamC.shape[1]
    Href = oracle_hessian(c, lamF, lamC, sigma)
    zF, zC = np.zeros_like(lamF), np.zeros_like(lamC)
    T = abs(sigma) * np.abs(oracle_hessian(c, zF, zC, 1.0))
    for i in range(ns):
        e = zF.copy()
        e[:, i] = 1.0
        T += np.abs(lamF[:, i:i + 1]) * np.abs(oracle_hessian(c, e, zC, 0.0))
    for j in range(npth):
        e = zC.copy()
        e[:, j] = 1.0
        T += np.abs(lamC[:, j:j + 1]) * np.abs(oracle_hessian(c, zF, e, 0.0))
    return Href, T
