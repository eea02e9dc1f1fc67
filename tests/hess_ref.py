"""Exact reference of the Lagrangian Hessian node blocks (emi_hess_kernel), element by element.  numpy only; nothing of the kernel.

The kernel's documented formula (csrc/emi_node_kernels.hpp, KH), per instance b and node k, packed lower triangle:

    H = sigma sgn h w_k L_zz  -  h sum_i lamF[i][k] f_i,zz  +  sum_j lamC[j][k] c_j,zz ,      h = (tf - t0) / 2, sgn = -1 to maximise

L_zz and f_i,zz come from tests/golden/hessian_terms.npz: sympy derivatives evaluated at 50 digits and rounded once to double, one
value per non-zero (term, slot) pair and fixture point.  The rows of the record table have closed forms, computed here from the
record in long double:
    disc, track   -2 mu on (px, px) and (py, py)
    ellipse       -2 mu (bsq ct^2 + asq st^2) on xx,  -2 mu (bsq st^2 + asq ct^2) on yy,  -2 mu ct st (asq - bsq) on xy
(record: kind, xc, yc, ct, st, asq, bsq, -- ; the track centres do not enter a second derivative).  Everything is combined in
np.longdouble; T is the sum of the absolute values of the same terms, so a small entry cannot hide behind a large one and an entry
whose terms cancel is not held to more digits than the format has.  Slots that no term touches have T == 0 and must be exactly zero.

The bound.  K is 8 times the worst ratio |H - Href| / (u (T + 1)), u = 2^-53, that the built-in model structs of
csrc/emi_models.hpp reach when they are compiled for the HOST and evaluated at every fixture point
(tests/test_hessian_ref_cpu.py::test_host_compiled_structs_lie_within_the_bound), rounded up to a power of two.  The factor 8 is for
what the device does differently from that host build: sin, cos and tan an ulp or two apart (entering through terms no larger than
T), another set of contracted operations, reciprocals rounded differently.  K comes from the host build and the exact terms, never
from what the device returns.
"""
import os

import numpy as np

U64 = 2.0 ** -53
# Measured worst host ratios |H - Href| / (u (T + 1)), g++ -O2 plain / with -mfma -ffp-contract=fast (pytest -s prints them):
#   point mass 0.00 / 0.00 (2 cL is exact)    quadrotor 2.61 / 2.61 (theta,theta)    fixed wing 13.00 / 10.21 (psi,theta)
# The fixed wing's worst entries are d2/dpsi dtheta of the position rates: each f_i,zz there is itself a sum of products of the
# size of the airspeed that cancel to a few hundredths, which T (one magnitude per term of the formula) does not see.
# 8 x 13.00 = 104, rounded up to a power of two (1.4e-14 (T + 1)):
K = 128.0
LD = np.longdouble
ELLIPSE, DISC, TRACK = 0, 1, 2          # record kinds (include/emi355x.h)
NV = {0: 4, 1: 8, 2: 16}
NS = {0: 2, 1: 6, 2: 12}
SIGMA = 0.7

_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hessian_terms.npz")) as f:
            _FIX = {k: f[k] for k in f.files}
    return _FIX


def npoints(model):
    return fixture()[f"z{model}"].shape[0]


def batch_rows(model, which):
    """(first row, instances, nodes taken) of the fixture rows copied from seeded batch `which` of the model (key batch<m>)"""
    config, B, M, take, first = (int(v) for v in fixture()[f"batch{model}"][which])
    return first, B, take


def points(model, idx):
    """X [B][ns][M], U [B][nc][M] of the fixture points idx [B][M]"""
    z = fixture()[f"z{model}"][np.asarray(idx)]               # [B][M][nv]
    z = np.ascontiguousarray(np.transpose(z, (0, 2, 1)))
    ns = NS[model]
    return np.ascontiguousarray(z[:, :ns]), np.ascontiguousarray(z[:, ns:])


def cycle(model, B, M, stride=1, start=0):
    """point indices [B][M] that walk the whole fixture of the model, instance b continuing where b - 1 stopped"""
    return (start + stride * np.arange(B * M).reshape(B, M)) % npoints(model)


def multipliers(B, ns, npth, M, seed=11):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, ns, M)), rng.standard_normal((B, npth, M))


def model_terms(model, idx):
    """second derivatives of L and of each f_i at the points idx [B][M]: dense long double [1 + ns][B][nh][M]"""
    f = fixture()
    nv, ns = NV[model], NS[model]
    idx = np.asarray(idx)
    out = np.zeros((1 + ns,) + idx.shape[:1] + (nv * (nv + 1) // 2,) + idx.shape[1:], dtype=LD)
    for t, q, v in zip(f[f"term{model}"], f[f"slot{model}"], f[f"val{model}"]):
        out[t, :, q, :] = v[idx]
    return out


def reference(model, idx, w, t0, tf, sigma, maximize, lamF, lamC=None, recs=None, tracks=None, px=0, py=1):
    """-> (Href, T) float64 [B][nh][M].  idx [B][M] fixture rows; w [M] mesh weights; lamF [B][ns][M]; lamC [B][np][M]; recs [np][8]
    (one shared table) or [B][np][8]; tracks (xc, yc) only have their shape checked against the table's track rows."""
    idx = np.asarray(idx)
    B, M = idx.shape
    nv, ns = NV[model], NS[model]
    nh = nv * (nv + 1) // 2
    h = (LD(tf) - LD(t0)) / 2
    sgn = LD(-1 if maximize else 1)
    D = model_terms(model, idx)
    lamF = np.asarray(lamF, dtype=LD)
    assert lamF.shape == (B, ns, M) and np.shape(w) == (M,)
    cL = LD(sigma) * sgn * h * np.asarray(w, dtype=LD)                              # [M]
    H = cL[None, None, :] * D[0]
    T = np.abs(cL)[None, None, :] * np.abs(D[0])
    for i in range(ns):
        c = h * lamF[:, i][:, None, :]
        H -= c * D[1 + i]
        T += np.abs(c) * np.abs(D[1 + i])
    if recs is not None and np.size(recs):
        recs = np.asarray(recs, dtype=np.float64)
        if recs.ndim == 2:
            recs = recs[None]
        assert recs.shape[0] in (1, B) and px != py
        npth = recs.shape[1]
        lamC = np.asarray(lamC, dtype=LD)
        assert lamC.shape == (B, npth, M)
        lo, hi = min(px, py), max(px, py)
        qxx, qyy, qxy = px * (px + 1) // 2 + px, py * (py + 1) // 2 + py, hi * (hi + 1) // 2 + lo
        for b in range(B):
            for j, r in enumerate(recs[b if recs.shape[0] > 1 else 0]):
                kind = int(r[0])
                mu = lamC[b, j]
                if kind == ELLIPSE:
                    ct, st, asq, bsq = (LD(v) for v in r[3:7])
                    cxx, cyy, cxy = -2 * (bsq * ct * ct + asq * st * st), -2 * (bsq * st * st + asq * ct * ct), -2 * ct * st * (asq - bsq)
                else:
                    assert kind in (DISC, TRACK)
                    if kind == TRACK:
                        assert tracks is not None and 0 <= int(r[1]) < np.asarray(tracks[0]).shape[-2]
                    cxx, cyy, cxy = LD(-2), LD(-2), LD(0)
                for q, cq in ((qxx, cxx), (qyy, cyy), (qxy, cxy)):
                    H[b, q] += mu * cq
                    T[b, q] += np.abs(mu * cq)
    return np.asarray(H, dtype=np.float64), np.asarray(T, dtype=np.float64)


def worst(H, Href, T):
    """-> (ratio, (instance, slot, node)) of the largest |H - Href| / (u (T + 1)); differences in long double"""
    r = np.abs(np.asarray(H, dtype=LD) - np.asarray(Href, dtype=LD)) / (U64 * (np.asarray(T, dtype=LD) + 1))
    r = np.asarray(r, dtype=np.float64)
    at = np.unravel_index(int(np.nanargmax(r)) if not np.isnan(r).all() else 0, r.shape)
    return float(r[at]), tuple(int(i) for i in at)


def check(what, H, Href, T, k=K):
    """the elementwise criterion; prints the worst ratio and where it is"""
    H = np.asarray(H)
    assert H.shape == Href.shape and not np.isnan(H).any(), what
    ratio, at = worst(H, Href, T)
    print(f"Hessian {what}: worst |H - Href| / (u (T + 1)) = {ratio:.2f} at (instance, slot, node) {at}, bound {k:g}")
    assert (H[T == 0] == 0).all(), (what, "an entry that no term touches is not zero")
    assert (np.abs(H - Href) <= k * U64 * (T + 1.0)).all(), (what, ratio, at)
    return ratio, at


# ---- record tables of the GPU cases (tests/test_gpu_hessian.py; the CPU test runs the oracle over them) ------------------------
def ellipse(xc, yc, angle, asq, bsq):
    return [ELLIPSE, xc, yc, np.cos(angle), np.sin(angle), asq, bsq, 0.0]


def disc(xc, yc, rsq):
    return [DISC, xc, yc, rsq, 0.0, 0.0, 0.0, 0.0]


def track(index, rsq):
    return [TRACK, float(index), rsq, 0.0, 0.0, 0.0, 0.0, 0.0]


def mixed_tables():
    """[3][5][8]: two ellipses, two discs and one track row per instance, every instance in another order and with its own ellipses"""
    e = lambda b, i: ellipse(2.0 + b, 3.0 - i, 0.3 + 0.7 * b + 1.9 * i, 0.5 + 0.25 * b + 1.5 * i, 0.11 + 0.05 * b + 0.2 * i)
    d = lambda b, i: disc(1.0 + i, 4.0 + b, 0.09 + 0.01 * b)
    t = track(0, 0.25)
    return np.array([[e(0, 0), d(0, 0), t, e(0, 1), d(0, 1)],
                     [t, e(1, 0), e(1, 1), d(1, 0), d(1, 1)],
                     [d(2, 0), d(2, 1), e(2, 0), t, e(2, 1)]])


def track_centres(M):
    """one shared track: (xc, yc) [1][M]"""
    s = np.linspace(0.0, 1.0, M)
    return (1.5 + 0.5 * s)[None], (2.0 - 0.25 * s)[None]


def path_slots(px, py):
    lo, hi = min(px, py), max(px, py)
    return px * (px + 1) // 2 + px, py * (py + 1) // 2 + py, hi * (hi + 1) // 2 + lo
