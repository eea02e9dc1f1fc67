"""Exact reference of the first-order outputs of an evaluation pass, element by element: the dynamics term -h f of the defect rows,
the dynamics block of VALS, the cost gradient, COST, the rows of the record table with their two partials, and the finished defect
rows (D.X)_k - h f_i.  numpy only; nothing of the kernels.

The documented outputs (include/emi355x.h), per instance b, node k, h = (tf - t0) / 2, sgn = -1 to maximise:

    RES  row i < ns          (D.X)_i,k - h f_i           (a nodes-only pass, EMI_EVAL_NODES, stores -h f_i alone)
    RES  row ns + j          c_j                          disc, track  rsq - (dx^2 + dy^2),  dx = px - xc, dy = py - yc
                                                          ellipse      asq bsq - (bsq delx^2 + asq dely^2),
                                                                       delx = ct dx - st dy, dely = st dx + ct dy
    VALS entry i nv + v      -h df_i/dz_v + (v == i) D_kk
    VALS entry ns nv + 2 j   dc_j/dpx, then dc_j/dpy      disc, track  -2 dx, -2 dy
                                                          ellipse      -2 (bsq delx ct + asq dely st), -2 (asq dely ct - bsq delx st)
    VALS last nv entries     sgn h w_k dL/dz_v
    COST                     sgn h sum_k w_k L_k

f_i, L and their derivatives come from tests/golden/first_order_terms.npz: sympy expressions evaluated at 50 digits and rounded
once to double, one value per entry and fixture point, each with its magnitude sum A (the sum of the absolute values of the
additive terms of the expanded expression).  The record rows are computed here in long double from the record, the track table
and dx, dy AS THE DOUBLES px - xc, py - yc (the subtraction is the kernel's input rounding, not part of what is held).  Everything
is combined in np.longdouble, and every number comes with the magnitude sum of what went into it, so a small entry cannot hide
behind a large one and an entry whose terms cancel is not held to more digits than the format has.

The criterion, for everything but the finished defect rows:   |got - ref| <= K_kind u A,   u = 2^-53,   and exactly zero (either
sign) where A == 0 -- which is every structural zero, and every entry whose only term vanishes at the point.  No floor is added:
the host builds need none at any fixture point.

Where the constants come from -- never from device output:

  K_MODEL   8 times the worst ratio |e - e_ref| / (u A) that f, jac, cost and grad of the built-in model structs of
            csrc/emi_models.hpp reach when they are compiled for the HOST (g++ -O2, plain and with -mfma -ffp-contract=fast) and
            evaluated at every fixture point (tests/test_first_order_ref_cpu.py::test_host_compiled_structs_lie_within_the_bound),
            rounded up to a power of two.  The factor 8 is the margin tests/hess_ref.py gives the device's own sin / cos / tan,
            its contraction and its reciprocals.  Measured worst host ratios, plain / fma (pytest -s prints them):
                point mass  f 0.00 / 0.00   jac 0.00 / 0.00   cost 2.00 / 2.00   grad 0.00 / 0.00     8 x 1.998 -> 16
                quadrotor   f 1.96 / 1.96   jac 1.96 / 1.96   cost 1.97 / 0.00   grad 0.00 / 0.00     8 x 1.97  -> 16
                fixed wing  f 3.30 / 3.30   jac 4.59 / 4.59   cost 3.89 / 1.95   grad 0.00 / 0.00     8 x 4.59  -> 64
            (worst places: quadrotor f_3 and d f_4 / d theta at point 240; fixed wing f_5 at point 105 and d f_5 / d theta
            = sq tan(theta) / cos(theta) at point 62, a product of five rounded factors.)  One constant per model.
  (below: k_def, k_jac, k_grad, k_cost of a model)
  K_DEF     K_MODEL + 1: the product h f_i.
  K_JAC     K_MODEL + 2: the product h df_i/dz_v and the sum with D_kk (one rounding less where they are fused).
  K_GRAD    K_MODEL + 2: the products h w_k and (sgn h w_k) dL/dz_v.
  K_ROWS    8, by counting roundings; the sums of products are explicit single-rounding fma, so the count is fixed.  With
            Ax = |ct dx| + |st dy|, Ay = |st dx| + |ct dy|:
              disc, track   dy dy (1), fma(dx, dx, .) (1), rsq - . (1): 3 u A, A = |rsq| + dx^2 + dy^2; the partials -2 dx, -2 dy
                            are exact.
              ellipse       delx, dely: the product and the fma, 2 u Ax and 2 u Ay.  delx^2: 2 x 2 + 1 = 5 u Ax^2, dely^2 alike;
                            asq (dely^2): 6; the inner fma 7 (bsq delx^2 enters it unrounded: 5, the larger count rules), the
                            outer fma 8: 8 u A, A = |asq bsq| + bsq Ax^2 + asq Ay^2.  Partials: bsq delx 3, asq dely 3, times
                            st 4, the fma 5, times -2 exact: 5 u A, A = 2 (bsq Ax |ct| + asq Ay |st|) and its mirror.
            (second-order terms u^2 are far below the slack between these counts and 8.)
  COST      the sum over k in any order adds (M - 1) u, the final product with sgn h one more:
            |COST - ref| <= (K_MODEL + M) u A,  A = sum_k |sgn h w_k| A_L,k.

The finished defect rows of a full pass, ref = (D.X)_k - h f_i with the product in long double:

    |got - ref| <= c_op(M) u S_op + K_DEF u h A_f + u |ref|,     S = sum_j |D_kj| |x_j|,     c_op(M) = M + 6,   S_op: below.

u |ref| is the rounding of the final combination.  c_op: a dot product of n terms summed in ANY order (MFMA chains, K slices,
partial sums combined later) has forward error at most n u sum |a_j b_j| to first order (gamma_n, Higham, Accuracy and Stability
of Numerical Algorithms, section 3.1).  The direct forms sum M terms: M u S.  The even/odd forms compute, for j < M / 2 and
m = M - 1 - j,  De_kj (x_j + x_m) + Do_kj (x_j - x_m)  with De, Do = (D_kj +- D_km) / 2 rounded on the host (1 u each), the sums
x_j +- x_m rounded (1 u each), two dot products of M / 2 terms (M / 2 u each), and the combination acc_e +- acc_o (1 u):
(M / 2 + 3) u S', S' = sum_{j < M/2} (|D_kj| + |D_km|)(|x_j| + |x_m|).  S' holds S and the cross terms |D_kj| |x_m|: counting the
rounding of x_j +- x_m means counting it at the size of the LARGER of the two.  For trajectories whose magnitudes are alike at
mirrored nodes S' = 2 S and (M / 2 + 3) S' = (M + 6) S, which is c_op(M) -- also above the direct forms' M.  Where one node is far
larger than its mirror image (the fixture's edge points with pitch +-1000 beside pitches below 1: S' / S reaches 990 in the
theta row) the sum S of the direct form does not bound what an even/odd kernel legitimately rounds: a plain double even/odd
evaluation on the CPU misses c_op u S by a factor 4.6 there (tests/test_first_order_ref_cpu.py prints it).  So the scale used is

    S_op = max(S, S' / 2),

equal to S wherever the mirrored magnitudes are alike (its median over the shapes used is 1.00 S), and the bound above stands with
S_op for S.  That the bound still sees f is what the horizon condition checks, from these same numbers.

The sequential pair ("overlap" 0: node kernel, then EMI_EVAL_DEFECT, documented as "accumulate D.X into the defect rows") is not
of the form  dot product, then one combination:  emi_defect_f64_kernel loads -h f_i into the MFMA accumulator and adds the M
products onto it, so -h f_i is one more term of the sum and is carried through all M additions.  On the long horizon the
accumulator stays in the binade of h f_i, every product is rounded to that binade's grid, and the errors add up whatever the
order: a plain double accumulation on the CPU reaches 23 u h |f_i| at (instance 16, theta row, node 115) of the quadrotor's
(128, 17) case, 1.2 times the bound above, and the device gives the same number there.  For the pair the dot-product count
therefore covers the carried value h |f_i| as well (accumulated=True):

    |got - ref| <= c_op(M) u (S_op + h |f_i|) + K_DEF u h A_f + u |ref|.

Beside what the bound above admits this adds (M + 6) u of relative error in h f_i, 1.5e-14 at M = 128: the horizon condition is
asserted for it too.
"""
import os

import numpy as np

import hess_ref as HR

U64 = HR.U64
LD = np.longdouble
NV, NS = HR.NV, HR.NS
ELLIPSE, DISC, TRACK = HR.ELLIPSE, HR.DISC, HR.TRACK
K_MODEL = {0: 16.0, 1: 16.0, 2: 64.0}
K_ROWS = 8.0


def k_def(model):
    return K_MODEL[model] + 1


def k_jac(model):
    return K_MODEL[model] + 2


def k_grad(model):
    return K_MODEL[model] + 2


# the full-pass cases: a horizon on which h f outweighs the operator's rounding (the built-in models do not depend on t), and the
# (model, M, B) they run at: every row of the pass-form table on 128 or 256 nodes with 17 instances, and 5 with two K slices; the
# stand-alone MFMA kernels at (128, 32) and (256, 19); the fixed wing's sequential pair at an odd M
HORIZON = (0.0, 2.0 ** 21)
HORIZON_SHAPES = ([(m, M, B) for m in (0, 1) for M in (128, 256) for B in (17, 5)] + [(1, 128, 32), (1, 256, 19), (2, 33, 3)])
SEQUENTIAL_SHAPES = [(1, 128, 17), (2, 33, 3)]      # ... of which these also run as the sequential pair

_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_order_terms.npz")) as f:
            _FIX = {k: f[k] for k in f.files}
    return _FIX


def horizon_points(model, B, M):
    """fixture rows [B][M] of a full-pass case: every point of the model in turn; for the point mass the seeded points only -- three
    of its 69 points are edge points with a control at zero, f_i = 0 there has no relative error, and they would be 2 % of the
    elements (the nodes-only cases visit them)"""
    if model == 0:
        first, B0, take = HR.batch_rows(0, 0)
        return (np.arange(B * M).reshape(B, M)) % (first + B0 * take)
    return HR.cycle(model, B, M)


def c_op(M):
    return M + 6.0


def k_cost(model, M):
    return K_MODEL[model] + M


def entries(model, idx, gold=False):
    """L, f_i and their derivatives at the fixture points idx (any shape): val, mag [1 + ns] + idx.shape and dval, dmag
    [1 + ns][nv] + idx.shape, long double; gold: the six points of models.json instead"""
    f = fixture()
    g = "gold_" if gold else ""
    idx = np.asarray(idx)
    nv, ns = NV[model], NS[model]
    val = np.asarray(f[f"{g}val{model}"][:, idx], dtype=LD)
    mag = np.asarray(f[f"{g}mag{model}"][:, idx], dtype=LD)
    dval = np.zeros((1 + ns, nv) + idx.shape, dtype=LD)
    dmag = np.zeros_like(dval)
    for t, v, a, m in zip(f[f"dterm{model}"], f[f"dvar{model}"], f[f"{g}dval{model}"], f[f"{g}dmag{model}"]):
        dval[t, v] = a[idx]
        dmag[t, v] = m[idx]
    return val, mag, dval, dmag


class Ref:
    """ref, A (long double) and K (broadcastable) of RES, VALS and COST of one pass"""
    pass


def record_rows(X, recs, tracks, px, py):
    """-> (c, Ac [B][np][M], d, Ad [B][2 np][M]) long double: the rows of the record table and their partials (dpx, dpy per row)"""
    X = np.asarray(X, dtype=np.float64)
    B, _, M = X.shape
    recs = np.asarray(recs, dtype=np.float64)
    if recs.ndim == 2:
        recs = recs[None]
    assert recs.shape[0] in (1, B) and px != py
    npth = recs.shape[1]
    if tracks is not None:
        tx, ty = (np.asarray(a, dtype=np.float64) for a in tracks)
        if tx.ndim == 2:
            tx, ty = tx[None], ty[None]
        assert tx.shape[0] in (1, B) and tx.shape[2] == M
    c, Ac = np.zeros((B, npth, M), dtype=LD), np.zeros((B, npth, M), dtype=LD)
    d, Ad = np.zeros((B, 2 * npth, M), dtype=LD), np.zeros((B, 2 * npth, M), dtype=LD)
    for b in range(B):
        for j, r in enumerate(recs[b if recs.shape[0] > 1 else 0]):
            kind = int(r[0])
            if kind == ELLIPSE:
                xc, yc = r[1], r[2]
            elif kind == DISC:
                xc, yc = r[1], r[2]
            else:
                assert kind == TRACK and tracks is not None
                s = b if tx.shape[0] > 1 else 0
                xc, yc = tx[s, int(r[1])], ty[s, int(r[1])]
            dx = np.asarray(X[b, px] - xc, dtype=LD)          # the doubles the kernel forms: one rounding each, taken as given
            dy = np.asarray(X[b, py] - yc, dtype=LD)
            if kind == ELLIPSE:
                ct, st, asq, bsq = (LD(v) for v in r[3:7])
                delx, dely = ct * dx - st * dy, st * dx + ct * dy
                Ax, Ay = np.abs(ct * dx) + np.abs(st * dy), np.abs(st * dx) + np.abs(ct * dy)
                c[b, j] = asq * bsq - (bsq * delx * delx + asq * dely * dely)
                Ac[b, j] = np.abs(asq * bsq) + np.abs(bsq) * Ax * Ax + np.abs(asq) * Ay * Ay
                d[b, 2 * j] = -2 * (bsq * delx * ct + asq * dely * st)
                d[b, 2 * j + 1] = -2 * (asq * dely * ct - bsq * delx * st)
                Ad[b, 2 * j] = 2 * (np.abs(bsq * ct) * Ax + np.abs(asq * st) * Ay)
                Ad[b, 2 * j + 1] = 2 * (np.abs(asq * ct) * Ay + np.abs(bsq * st) * Ax)
            else:
                rsq = LD(r[3] if kind == DISC else r[2])
                c[b, j] = rsq - (dx * dx + dy * dy)
                Ac[b, j] = np.abs(rsq) + dx * dx + dy * dy
                d[b, 2 * j], d[b, 2 * j + 1] = -2 * dx, -2 * dy
                Ad[b, 2 * j], Ad[b, 2 * j + 1] = 2 * np.abs(dx), 2 * np.abs(dy)
    return c, Ac, d, Ad


def operator_product(D, X):
    """(D.X) and S = sum_j |D_kj| |x_j|, [B][ns][M] long double"""
    Dl, Xl = np.asarray(D, dtype=LD), np.asarray(X, dtype=LD)
    return np.einsum("kj,bij->bik", Dl, Xl), np.einsum("kj,bij->bik", np.abs(Dl), np.abs(Xl))


def mirrored_scale(D, X):
    """S' = sum_{j < M/2} (|D_kj| + |D_km|)(|x_j| + |x_m|), m = M - 1 - j (the middle node of an odd mesh pairs with itself)"""
    Dl, Xl = np.abs(np.asarray(D, dtype=LD)), np.abs(np.asarray(X, dtype=LD))
    return np.einsum("kj,bij->bik", Dl + Dl[:, ::-1], Xl + Xl[..., ::-1]) / 2


def reference(model, idx, mesh, t0, tf, maximize=False, recs=None, tracks=None, px=0, py=1, full=False, accumulated=False):
    """The outputs of one pass at the fixture points idx [B][M] on the mesh (tau, w, D).  -> Ref with RES, A_RES, K_RES
    [B][ns + np][M]; VALS, A_VALS, K_VALS [B][nvals][M]; COST, A_COST [B], K_COST.  full: the defect rows carry D.X, and
    LIM_DEF [B][ns][M] is their bound (A_RES of those rows is then h A_f still, for the horizon condition); accumulated: the
    bound of the sequential pair, which adds D.X onto -h f term by term."""
    idx = np.asarray(idx)
    B, M = idx.shape
    nv, ns = NV[model], NS[model]
    tau, w, D = mesh
    assert np.shape(w) == (M,) and np.shape(D) == (M, M)
    h = (LD(tf) - LD(t0)) / 2
    sgn = LD(-1 if maximize else 1)
    val, mag, dval, dmag = entries(model, idx)                     # [1 + ns][B][M], [1 + ns][nv][B][M]
    X, _ = HR.points(model, idx)
    npth = 0 if recs is None or not np.size(recs) else np.asarray(recs).shape[-2]
    r = Ref()
    r.h, r.ns, r.nv, r.np = h, ns, nv, npth
    # RES
    r.RES, r.A_RES = np.zeros((B, ns + npth, M), dtype=LD), np.zeros((B, ns + npth, M), dtype=LD)
    r.K_RES = np.full((1, ns + npth, 1), k_def(model))
    r.K_RES[:, ns:] = K_ROWS
    r.RES[:, :ns] = np.transpose(-h * val[1:], (1, 0, 2))
    r.A_RES[:, :ns] = np.transpose(h * mag[1:], (1, 0, 2))
    r.MHF = r.RES[:, :ns].copy()                 # -h f by itself
    r.HF = np.abs(r.MHF)
    # VALS
    nvals = ns * nv + 2 * npth + nv
    r.VALS, r.A_VALS = np.zeros((B, nvals, M), dtype=LD), np.zeros((B, nvals, M), dtype=LD)
    r.K_VALS = np.full((1, nvals, 1), k_jac(model))
    r.K_VALS[:, ns * nv:ns * nv + 2 * npth] = K_ROWS
    r.K_VALS[:, ns * nv + 2 * npth:] = k_grad(model)
    dkk = np.asarray(np.diagonal(D), dtype=LD)
    for i in range(ns):
        for v in range(nv):
            r.VALS[:, i * nv + v] = -h * dval[1 + i, v] + (dkk if v == i else 0)
            r.A_VALS[:, i * nv + v] = h * dmag[1 + i, v] + (np.abs(dkk) if v == i else 0)
    cw = sgn * h * np.asarray(w, dtype=LD)
    g0 = ns * nv + 2 * npth
    for v in range(nv):
        r.VALS[:, g0 + v] = cw * dval[0, v]
        r.A_VALS[:, g0 + v] = np.abs(cw) * dmag[0, v]
    if npth:
        c, Ac, d, Ad = record_rows(X, recs, tracks, px, py)
        r.RES[:, ns:], r.A_RES[:, ns:] = c, Ac
        r.VALS[:, ns * nv:g0], r.A_VALS[:, ns * nv:g0] = d, Ad
    # COST
    r.COST, r.A_COST, r.K_COST = (cw * val[0]).sum(axis=1), (np.abs(cw) * mag[0]).sum(axis=1), k_cost(model, M)
    if full:
        DX, S = operator_product(D, X)
        r.S, r.DX, r.SP = S, DX, mirrored_scale(D, X)
        S = np.maximum(S, r.SP / 2) + (r.HF if accumulated else 0)
        r.RES[:, :ns] += DX
        r.LIM_DEF = U64 * (c_op(M) * S + k_def(model) * r.A_RES[:, :ns] + np.abs(r.RES[:, :ns]))
    return r


def worst(got, ref, lim):
    """-> (ratio, position) of the largest |got - ref| / lim over the elements with lim > 0; differences in long double"""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    q = np.zeros(err.shape)
    pos = lim > 0
    q[pos] = np.asarray(err[pos] / lim[pos], dtype=np.float64)
    at = np.unravel_index(int(np.argmax(q)), q.shape) if q.size else ()
    return (float(q[at]) if q.size else 0.0), tuple(int(i) for i in at)


def within(got, ref, A, K):
    """the elementwise criterion as a boolean array: |got - ref| <= K u A, which for A == 0 asks for an exact zero of either sign"""
    got = np.asarray(got)
    ref, A = np.broadcast_to(ref, got.shape), np.broadcast_to(A, got.shape)
    return np.abs(np.asarray(got, dtype=LD) - ref) <= np.broadcast_to(K, got.shape) * U64 * A


def check(what, got, ref, A, K):
    """|got - ref| <= K u A per element, exactly zero where A == 0; prints the worst |got - ref| / (u A) and where it is"""
    got = np.asarray(got)
    assert got.shape == ref.shape and not np.isnan(got).any(), (what, got.shape, ref.shape)
    A = np.broadcast_to(A, got.shape)
    ratio, at = worst(got, ref, U64 * A)
    k = float(np.broadcast_to(K, got.shape)[at]) if got.size else 0.0
    print(f"{what}: worst |got - ref| / (u A) = {ratio:.2f} at {at}, bound {k:g}")
    assert (got[A == 0] == 0).all(), (what, "an entry with no term is not zero")
    ok = within(got, ref, A, K)
    assert ok.all(), (what, ratio, at, "first failures", np.argwhere(~ok)[:4].tolist())
    return ratio, at


def check_pass(what, got, r, defect_rows=True, vals=True, keep=None):
    """RES, VALS and COST of a pass against r, each elementwise.  defect_rows False: a full pass, the defect rows go to
    check_defect; vals False: a values-only pass; keep: boolean [nvals], the rows an EMI_EVAL_KEEP_INVARIANT pass leaves alone."""
    RES, VALS, COST = got
    out = {}
    lo = 0 if defect_rows else r.ns
    if RES.shape[1] > lo:
        out["RES"] = check(f"{what} RES", RES[:, lo:], r.RES[:, lo:], r.A_RES[:, lo:], r.K_RES[:, lo:])
    if vals:
        rows = np.arange(VALS.shape[1]) if keep is None else np.flatnonzero(~keep)
        out["VALS"] = check(f"{what} VALS", VALS[:, rows], r.VALS[:, rows], r.A_VALS[:, rows], r.K_VALS[:, rows])
    out["COST"] = check(f"{what} COST", COST, r.COST, r.A_COST, r.K_COST)
    return out


def check_defect(what, RES, r):
    """the finished defect rows of a full pass against their bound; prints the worst |got - ref| / bound"""
    got = np.asarray(RES)[:, :r.ns]
    assert not np.isnan(got).any(), what
    ratio, at = worst(got, r.RES[:, :r.ns], r.LIM_DEF)
    print(f"{what} defect rows: worst |got - ref| / bound = {ratio:.3f} at (instance, state, node) {at}")
    assert (np.abs(np.asarray(got, dtype=LD) - r.RES[:, :r.ns]) <= r.LIM_DEF).all(), (what, ratio, at)
    return ratio, at


def admitted(r):
    """the relative error in h f_i that the full-pass bound admits, per defect-row element (inf where f_i == 0)"""
    with np.errstate(divide="ignore"):
        return np.asarray(np.where(r.HF > 0, r.LIM_DEF / np.where(r.HF > 0, r.HF, 1), np.inf), dtype=np.float64)
