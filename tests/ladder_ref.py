"""Reference side of the tests of the mesh ladder over the lock-step solve (emi_prolong_*, emi_repair_guess_dev,
emi_ipm_solve_ladder_*).  TEST INFRASTRUCTURE: numpy + the harness.

  * the pairs of meshes of the prolongation tests and their fixture (tests/golden/prolong_matrices.npz: the Lagrange basis of the
    coarse LGL nodes at the fine ones, from mpmath at 50 digits, tests/golden/gen_prolong_golden.py);
  * the prolongation as a numpy matrix (bary_matrix: the barycentric second form) and as a long-double product (prolong_ld);
  * ETOL::mi355x::repair_guess restated in numpy (repair_ref): IEEE doubles, one rounding per operation, in the order the host
    function writes them, so the kernel's bits (contraction off) are these;
  * the inputs of the repair tests (repair_case) and the cases of the ladder tests (the instances of tests/lockstep_ref.py, started
    on 21 nodes; fixture tests/golden/ladder_cases.json, tests/golden/gen_ladder_cases.py).
"""
import ctypes as C
import json
import os

import numpy as np

import lockstep_ref as LR

ROOT = LR.ROOT
PROLONG_FIXTURE = os.path.join(ROOT, "tests", "golden", "prolong_matrices.npz")
LADDER_FIXTURE = os.path.join(ROOT, "tests", "golden", "ladder_cases.json")
PAIRS = ((2, 3), (5, 9), (21, 41), (33, 65), (40, 41), (129, 257))
# elementwise gate of emi_prolong_matrix against the mpmath matrix, in units of 2^-53 sum_j |P*_qj|: the largest ratio measured over
# PAIRS rounded up to the next power of two (tests/test_prolong_cpu.py prints the figures)
PROLONG_GATE = 512.0
LADDER = (21, 41)
D_ = C.POINTER(C.c_double)
I_ = C.POINTER(C.c_int)


# ---- prolongation ------------------------------------------------------------------------------------------------------------------
def prolong_fixture():
    z = np.load(PROLONG_FIXTURE)
    return {(mc, mf): z[f"P_{mc}_{mf}"] for mc, mf in PAIRS}


def bary_matrix(tau_c, w_c, tau_f):
    """P [Mf][Mc] by the barycentric second form with the weights (-1)^j sqrt(w_j) (numpy; what interp_lgl computes)"""
    lam = np.where(np.arange(len(tau_c)) % 2 == 1, -1.0, 1.0) * np.sqrt(w_c)
    P = np.zeros((len(tau_f), len(tau_c)))
    for q, t in enumerate(tau_f):
        d = t - tau_c
        hit = np.nonzero(d == 0.0)[0]
        if hit.size:
            P[q, hit[0]] = 1.0
        else:
            P[q] = (lam / d) / (lam / d).sum()
    return P


def prolong_ld(P, V):
    """(V P^T, sum_j |P_qj| |V_rj|) in long double: [R][Mf] each"""
    Pl, Vl = P.astype(np.longdouble), V.astype(np.longdouble)
    return Vl @ Pl.T, np.abs(Vl) @ np.abs(Pl).T


# ---- repair_guess in numpy -----------------------------------------------------------------------------------------------------------
def repair_ref(X, recs, px=0, py=1, tracks=None):
    """X [B][ns][M], recs [nsets][np][8] (nsets 1 or B), tracks (xc, yc) each [tsets][ntracks][M] or None -> (repaired copy, the
    largest number of sweeps a node moved in).  A node that a sweep does not move is not moved by a later one (nothing else
    changed), so sweeping every node until it rests is the host's loop, which sweeps all nodes until none moves."""
    X = np.array(X, dtype=np.float64, copy=True)
    B, _, M = X.shape
    npath = recs.shape[1]
    if npath == 0 or M <= 2:
        return X, 0
    margin = 0.05
    x, y = X[:, px, 1:-1].copy(), X[:, py, 1:-1].copy()
    active = np.ones(x.shape, dtype=bool)
    sweeps = 0
    col = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1, 1), x.shape)
    with np.errstate(all="ignore"):
        for _ in range(50):
            moved = np.zeros(x.shape, dtype=bool)
            for j in range(npath):
                r = recs[:, j]                                      # [nsets][8]
                kind = r[:, 0].astype(int)
                assert (kind == kind[0]).all(), "one kind per row over the sets (test inputs)"
                if kind[0] == 0:
                    xc, yc, ct, st, asq, bsq = (col(r[:, i]) for i in (1, 2, 3, 4, 5, 6))
                elif kind[0] == 1:
                    xc, yc, asq = (col(r[:, i]) for i in (1, 2, 3))
                    bsq, ct, st = asq, col(1.0), col(0.0)
                else:
                    t = r[:, 1].astype(int)
                    sets = np.arange(B) if tracks[0].shape[0] > 1 else np.zeros(B, dtype=int)
                    tt = t if t.size == B else np.repeat(t, B)
                    xc, yc = tracks[0][sets, tt][:, 1:-1], tracks[1][sets, tt][:, 1:-1]
                    asq = col(r[:, 2])
                    bsq, ct, st = asq, col(1.0), col(0.0)
                ok = active & (asq > 0) & (bsq > 0)
                dx, dy = x - xc, y - yc
                ex, ey = ct * dx - st * dy, st * dx + ct * dy
                q = ex * ex / asq + ey * ey / bsq
                hit = ok & ~(q >= 1.0 + 0.5 * margin)
                dead = q < 1e-12
                g = np.sqrt((1.0 + margin) / q)
                ex = np.where(dead, 0.0, ex * g)
                ey = np.where(dead, np.sqrt(bsq * (1.0 + margin)), ey * g)
                x = np.where(hit, xc + ct * ex + st * ey, x)
                y = np.where(hit, yc - st * ex + ct * ey, y)
                moved |= hit
            if not moved.any():
                break
            active = moved
            sweeps += 1
    X[:, px, 1:-1], X[:, py, 1:-1] = x, y
    return X, sweeps


def repair_case(M, B=3, ns=6, per_instance=False, with_track=False):
    """Inputs of the repair tests on M LGL nodes: positions along the line (1, 1) -> (8, 6) with a little noise, and a table whose
    rows put nodes inside a disc, one node on a disc's dead centre, nodes inside a rotated ellipse, nodes inside two overlapping
    discs (more than one sweep), both end nodes inside discs, and leave the rest outside everything.  per_instance: one table per
    instance (shifted); with_track: one more row of kind EMI_PATH_TRACK whose centre moves along the line."""
    import etol_amd as E
    tau = E.lgl(M)[0]
    s = (tau + 1) / 2
    rng = np.random.default_rng(100 + M)
    X = rng.standard_normal((B, ns, M))
    X[:, 0] = 1 + 7 * s + 0.02 * rng.standard_normal((B, M))
    X[:, 1] = 1 + 5 * s + 0.02 * rng.standard_normal((B, M))
    kc = max(1, M // 3)                                     # the node that sits on the dead centre of row 0 (instance 0)
    cx, cy = float(1 + 7 * s[kc]), float(1 + 5 * s[kc])
    X[0, 0, kc], X[0, 1, kc] = cx, cy
    k2 = max(kc + 1, (2 * M) // 3)                          # a node between the overlapping discs of rows 2 and 3: row 3 pushes it back
    X[0, 0, k2], X[0, 1, k2] = 6.1 - 0.05 * 0.5 / np.hypot(0.6, 0.5), 4.65 + 0.05 * 0.6 / np.hypot(0.6, 0.5)      # into row 2: two sweeps
    a = np.deg2rad(30.0)
    rows = [[1, cx, cy, 0.9 ** 2, 0, 0, 0, 0],
            [0, 4.4, 3.6, np.cos(a), np.sin(a), 1.0, 0.3, 0],
            [1, 5.8, 4.4, 0.7 ** 2, 0, 0, 0, 0],
            [1, 6.4, 4.9, 0.7 ** 2, 0, 0, 0, 0],
            [1, 1.0, 1.0, 0.6 ** 2, 0, 0, 0, 0],            # on the first end node
            [1, 8.0, 6.0, 0.3 ** 2, 0, 0, 0, 0]]            # on the last end node
    tracks = None
    if with_track:
        rows.append([2, 0, 0.4 ** 2, 0, 0, 0, 0, 0])
        txc = np.ascontiguousarray(np.broadcast_to(2.0 + 5.0 * s, (1, 1, M)))
        tyc = np.ascontiguousarray(np.broadcast_to(1.6 + 4.2 * s, (1, 1, M)))
        tracks = (txc, tyc)
    recs = np.array(rows, dtype=np.float64)[None]
    if per_instance:
        recs = np.repeat(recs, B, 0)
        for b in range(B):
            recs[b, :4, 1] += 0.05 * b                      # (instance 0 keeps the dead centre)
            recs[b, :4, 2] -= 0.03 * b
    return dict(M=M, B=B, ns=ns, X=np.ascontiguousarray(X), recs=np.ascontiguousarray(recs), tracks=tracks, kc=kc)


def load_harness():
    h = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    h.harness_repair_guess.argtypes, h.harness_repair_guess.restype = [C.c_int, C.c_int, D_, C.c_int, D_, D_, D_, D_], None
    h.harness_ladder_solve_oracle.argtypes = [C.c_char_p, C.c_int, C.c_double, D_, C.c_int, D_, D_, D_, D_, D_, C.c_double, C.c_int, C.c_int, D_,
                                              I_, D_]
    return h


def repair_host(h, c):
    """the host function on the case's instances, one at a time -> repaired copy of X"""
    X = c["X"].copy()
    dp = lambda a: a.ctypes.data_as(D_)
    for b in range(c["B"]):
        recs = np.ascontiguousarray(c["recs"][b if c["recs"].shape[0] > 1 else 0])
        xs, ys = np.ascontiguousarray(X[b, 0]), np.ascontiguousarray(X[b, 1])
        tx = ty = None
        nt = 0
        if c["tracks"] is not None:
            tx, ty = (np.ascontiguousarray(t[0]) for t in c["tracks"])
            nt = tx.shape[0]
        h.harness_repair_guess(c["M"], recs.shape[0], dp(recs), nt, dp(tx) if nt else None, dp(ty) if nt else None, dp(xs), dp(ys))
        X[b, 0], X[b, 1] = xs, ys
    return X


# ---- the ladder's cases -----------------------------------------------------------------------------------------------------------------
def quad_at(tf, M, discs):
    """lockstep_ref.quad on another number of nodes"""
    import indep_nlp as N
    return N.Nlp(1, LR.QUAD_PARAMS, M, 0.0, tf, LR.records(discs), None, x0=[1, 1, 0, 0, 0, 0], xf=[8, 6, 0, 0, 0, 0],
                 xtol=[0.01, 0.01, 0.01, 0.05, 0.05, 0.05], xlo=[0, 0, -1.2, -6, -6, -4], xup=[10, 10, 1.2, 6, 6, 4], ulo=[0, -1], uup=[25, 1])


def instances(tf, M0=LADDER[0]):
    """lockstep_ref.instances(tf) with their starts on M0 nodes (indep_nlp.starts): list of dict discs, bump, z0"""
    import indep_nlp as N
    P = quad_at(tf, M0, LR.discs_of(LR.FIRST_DISCS[0]))
    z0s = N.starts(P, LR.BUMPS)
    return [dict(discs=LR.discs_of(first), bump=bump, z0=z0) for bump, z0 in zip(LR.BUMPS, z0s) for first in LR.FIRST_DISCS]


def ladder_fixture():
    return json.load(open(LADDER_FIXTURE))
