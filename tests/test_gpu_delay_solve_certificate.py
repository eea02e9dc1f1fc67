"""Sol::certificate / lamL / adjDelayed of ETOL::eMI355X::solve() on a problem with delayed states and controls, through
tests/harness/etol_harness_delay_certify.cpp.  -m gpu

The problem of tests/test_gpu_delays.py::test_delayed_problem_is_solved_through_the_etol_api (setXrhorizon(3), setUrhorizon(1), a
disc of radius 0.9 / 0.5 / none) at 25, 33 and 41 nodes, solved with the Alg of that test (nlp_tolerance 1e-10).

1. Sol::certificate.computed is true, and the six figures agree with the numpy certificate (tests/adjoint_ref.py on the folded
   gradient of tests/delay_adjoint_ref.py) built from ORACLE values at the returned point -- delayed values and fold with the oracle's
   own interpolation matrices.  Allowances as tests/test_gpu_solve_certificate.py derives them, with the fold in tol_G:
   tol_G = max(2 (M (1 + copies) + nv + np + 4) eps T + 5e-13 T + 1e-12 max(1, |W|max) sum |Gdel|)   (adjDelayed: the same per slot).
2. certificate.defect <= 1e-8, the limit the delayed solve test asserts for evaluate() at the solution.
3. With s = max(100, mean |multiplier|) / 100 over lamF and lamC, stationarity / s and complementarity / s are at most
   acceptable_factor * nlp_tolerance, the loosest level at which solve_nlp reports success, for the tolerance the harness passes.
4. |adjDelayed + lamL|max / s is held to the same level: stationarity of the lifted problem in the delayed values (the sign the
   coupling rows are written with, include/ETOL/eMI355X.hpp).
5. One control moved by 1e-3 at an interior node: stationarity or complementarity at least tenfold.
6. With Alg::certify = false the trajectory and the multipliers are bit-identical (certificate not computed, adjDelayed empty)."""
import ctypes as C
import os

import numpy as np
import pytest

import adjoint_ref as A
import delay_adjoint_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
P3 = [0.7, 0.3]
DT, TOL = 0.25, 1e-10


@pytest.fixture(scope="module")
def H(built):
    import torch  # noqa: F401
    lib = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    lib.harness_dc_solve.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
    lib.harness_dc_get.argtypes = [C.c_char_p, DP, C.c_int]
    lib.harness_dc_message.restype = C.c_char_p
    lib.harness_dc_certify.argtypes = [DP, C.c_int, DP, C.c_int, DP, C.c_int, DP, DP, C.c_int]
    yield lib
    lib.harness_dc_release()


def _get(H, name):
    n = H.harness_dc_get(name.encode(), None, 0)
    assert n >= 0, name
    a = np.zeros(max(n, 1))
    H.harness_dc_get(name.encode(), a.ctypes.data_as(DP), n)
    return a[:n]


def _solve(H, nsteps, disc_r, certify):
    rc = H.harness_dc_solve(nsteps, DT, 3, 1, disc_r, TOL, int(certify))
    assert rc == 0, H.harness_dc_message().decode()
    s = {k: _get(H, k) for k in ("X", "U", "lamF", "lamC", "lamL", "adjDelayed", "cert", "zl", "zu", "cl", "cu", "dims", "stats", "recs")}
    ns, ncf, npth, M, nd, xh, uh = (int(v) for v in s["dims"][:7])
    s.update(ns=ns, ncf=ncf, np=npth, M=M, nd=nd, xh=xh, uh=uh, dt=s["dims"][7], t0=s["dims"][8], tf=s["dims"][9])
    assert s["dims"][10] == 0.0                                  # the problem is not left lifted
    for k, r in (("X", ns), ("U", ncf), ("lamF", ns), ("lamC", npth), ("lamL", nd), ("zl", ns + ncf), ("zu", ns + ncf)):
        s[k] = s[k].reshape(r, M)
    return s


def oracle_certificate(s):
    M, ns, ncf, npth, xh, uh = s["M"], s["ns"], s["ncf"], s["np"], s["xh"], s["uh"]
    nc = ncf + s["nd"]
    mesh = O.lgl(M)
    W = R.oracle_delay_matrices(M, mesh[0], s["t0"], s["tf"], s["dt"], xh, uh)
    recs = s["recs"].reshape(npth, 8) if npth else None
    X, U = s["X"][None], s["U"][None]
    RES, VALS, COST = O.evaluate(3, P3, M, mesh, s["t0"], s["tf"], X, R.extended(X, U, W, ns, ncf, xh, uh), recs)
    pat = R.table_pattern(ns, nc, npth)
    assert len(pat) == VALS.shape[1]
    lamF, lamC = s["lamF"][None], s["lamC"][None]
    dims = (ns, nc, ncf, xh, uh)
    G, Gdel = R.lagr_grad_total(VALS, lamF, lamC, 1.0, mesh[2], pat, *dims, W)
    T, Tdel = R.lagr_grad_total(VALS, lamF, lamC, 1.0, mesh[2], pat, *dims, W, absolute=True)
    cert = A.certificate(G, RES, X, U, VALS, lamF, lamC, 1.0, s["zl"], s["zu"], s["cl"], s["cu"])[0]
    cert[4] = np.abs(VALS[0, -(ns + nc):]).max()                 # gmax: over the extended cost-gradient entries
    bG, bdel = R.bound(T, Tdel, M, ns + nc, npth, R.copies(ns, ncf, xh, uh))
    tol_G = float((bG + 5e-13 * T + 1e-12 * R.fold_weight(Gdel, W, ns, ncf, xh, uh)).max())
    tol_del = float((bdel + 5e-13 * Tdel + 1e-12 * R.slot_weight(Gdel, W, ns, ncf, xh, uh)).max())
    z = np.concatenate([X[0], U[0]])
    widest = max(np.where(np.abs(s["zl"]) < 1e19, np.abs(z - s["zl"]), 0.0).max(), np.where(np.abs(s["zu"]) < 1e19, np.abs(s["zu"] - z), 0.0).max())
    cmax = np.abs(RES[0, ns:]).max() + 1.0 if npth else 0.0
    dscale = (np.einsum("kj,ij->ik", np.abs(mesh[2]), np.abs(s["X"])) + np.abs(RES[0, :ns]) + 1.0).max()
    tol = dict(stat=tol_G, comp=tol_G * widest + cert[5] * 5e-13 * cmax, defect=5e-13 * dscale, viol=5e-13 * cmax,
               gmax=5e-13 * (np.abs(VALS[0, -(ns + nc):]).max() + 1.0), lmax=0.0)
    return cert, tol, Gdel[0], tol_del


@pytest.mark.parametrize("nsteps,disc_r", [(24, 0.9), (32, 0.5), (40, 0.0)])
def test_certificate_of_a_delayed_solve(H, nsteps, disc_r):
    off = _solve(H, nsteps, disc_r, False)
    s = _solve(H, nsteps, disc_r, True)                          # the solver of this one stays held for certify()
    name = f"delayed solve, {nsteps + 1} nodes, disc {disc_r}"
    # 6. the certificate step leaves the iterates alone
    assert off["cert"][6] == 0.0 and not off["cert"][:6].any() and off["adjDelayed"].size == 0
    assert s["cert"][6] == 1.0
    assert np.array_equal(off["stats"][:3], s["stats"][:3])
    for k in ("X", "U", "lamF", "lamC", "lamL"):
        assert np.array_equal(off[k], s[k]), k
    assert s["nd"] == 6 and s["lamL"].shape == (6, s["M"]) and s["adjDelayed"].size == 6 * s["M"]
    adj = s["adjDelayed"].reshape(6, s["M"])
    dev = dict(zip(A.FIELDS, s["cert"][:6]))
    # 1. against the oracle
    ref, tol, Gdel_ref, tol_del = oracle_certificate(s)
    for q, f in enumerate(A.FIELDS):
        print(f"{name}: {f}: Sol::certificate {dev[f]:.6e}  oracle {ref[q]:.6e}  allowance {tol[f]:.3e}")
    print(f"{name}: adjDelayed against the oracle's: {np.abs(adj - Gdel_ref).max():.3e}  allowance {tol_del:.3e}")
    for q, f in enumerate(A.FIELDS):
        assert abs(dev[f] - ref[q]) <= tol[f], (f, dev[f], ref[q], tol[f])
    assert np.abs(adj - Gdel_ref).max() <= tol_del
    # 2.
    assert dev["defect"] <= 1e-8
    # 3. / 4.
    mult = np.concatenate([np.abs(s["lamF"]).ravel(), np.abs(s["lamC"]).ravel()])
    sd = max(100.0, mult.mean()) / 100.0
    level = s["stats"][5] * s["stats"][4]
    assert level == 100.0 * TOL
    plus, minus = np.abs(adj + s["lamL"]).max(), np.abs(adj - s["lamL"]).max()
    print(f"{name}: stationarity / s = {dev['stat'] / sd:.3e}, complementarity / s = {dev['comp'] / sd:.3e}, s = {sd:.3e}, level {level:.1e}, "
          f"|adjDelayed + lamL|max = {plus:.3e}, |adjDelayed - lamL|max = {minus:.3e}, |lamL|max = {np.abs(s['lamL']).max():.3e}, "
          f"kkt_error {s['stats'][3]:.3e}, iterations {int(s['stats'][1])}")
    assert dev["stat"] / sd <= level, (dev["stat"], sd)
    assert dev["comp"] / sd <= level, (dev["comp"], sd)
    assert plus / sd <= level, (plus, sd)                         # adjDelayed = -lamL (include/ETOL/eMI355X.hpp)
    assert np.abs(s["lamL"]).max() > 1e3 * level                  # ... and that is not 0 = 0
    # 5. certify() of the returned point is Sol::certificate; of a pushed point it is not
    cert, adj2 = np.zeros(7), np.zeros(6 * s["M"])

    def certify(X, U):
        z = np.ascontiguousarray(np.concatenate([X.ravel(), U.ravel()]))
        lf, lc = np.ascontiguousarray(s["lamF"].ravel()), np.ascontiguousarray(s["lamC"].ravel())
        assert H.harness_dc_certify(z.ctypes.data_as(DP), z.size, lf.ctypes.data_as(DP), lf.size, lc.ctypes.data_as(DP), lc.size,
                                    cert.ctypes.data_as(DP), adj2.ctypes.data_as(DP), adj2.size) == 0
        return cert.copy()

    again = certify(s["X"], s["U"])
    assert np.array_equal(again, s["cert"]) and np.array_equal(adj2, s["adjDelayed"])
    U = s["U"].copy()
    U[1, s["M"] // 2] += 1e-3
    pushed = certify(s["X"], U)
    print(f"{name}: stationarity {again[0]:.3e} / complementarity {again[1]:.3e} at the solution, {pushed[0]:.3e} / {pushed[1]:.3e} "
          f"with one control moved by 1e-3")
    assert pushed[6] == 1.0
    assert (pushed[0] >= 10.0 * again[0] and pushed[0] > 0) or (pushed[1] >= 10.0 * again[1] and pushed[1] > 0)
