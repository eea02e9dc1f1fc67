"""Sol::lamF / lamC / certificate of ETOL::eMI355X::solve() and eMI355X::certify(), through tests/harness/etol_harness_certify.cpp.  -m gpu

Four solves with the default Alg (scaling "none": the iteration's units are the caller's): the shipped problem, the 256-node
quadrotor, the config-3 sized problem (1024 nodes, 20 keep-outs) and the 129-node fixed wing.

1. Sol::certificate against the numpy certificate (tests/adjoint_ref.py) built from ORACLE values at the returned point.  Per
   figure the allowance follows the end-to-end bound of tests/test_gpu_certificate.py, tol_G = max(2 (M + nv + np + 2) eps T +
   5e-13 T): stat: tol_G; comp: tol_G times the largest distance to a finite bound plus lam_max times the path-row agreement 5e-13 (|c|max + 1);
   defect: 5e-13 of sum |D||x| + |row| + 1 (the parity tolerance of the defect rows); viol: 5e-13 (|c|max + 1) (the variables are the
   same numbers on both sides); gmax: 5e-13 (|costgrad|max + 1); lmax: equal.
2. certificate.defect <= 1e-6 (the limit tests/test_gpu_solve.py asserts).
3. With s = max(100, mean |multiplier|) / 100 -- the form of the iteration's own sd (emi_nlp.cpp) over the multipliers the caller
   holds -- stationarity / s and complementarity / s are at most acceptable_factor * nlp_tolerance = 100 * 1e-6, the loosest level
   at which solve_nlp reports success.
4. The config-3 solution pushed off the optimum (1e-3 on one control at one interior node): stationarity at least tenfold -- and,
   because every variable of that problem is boxed (stationarity is 0 on both sides of the comparison), complementarity too.
5. nlp_iterations_total, cost and the trajectories are bit-identical with Alg::certify = false (certificate not computed)."""
import ctypes as C
import os

import numpy as np
import pytest

import adjoint_ref as A
import cases
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)

QUAD_DISCS = [(4.0, 3.2, 0.8), (6.3, 4.4, 0.7), (2.5, 1.2, 0.4), (1.6, 3.4, 0.35), (3.1, 5.2, 0.30), (5.2, 1.4, 0.35),
              (7.4, 2.6, 0.30), (8.6, 4.2, 0.25), (5.0, 6.3, 0.35), (2.2, 7.1, 0.30), (6.9, 7.4, 0.35), (8.9, 7.9, 0.30),
              (0.9, 5.6, 0.25), (3.9, 8.4, 0.30), (9.2, 1.3, 0.30), (7.0, 0.8, 0.25), (4.6, 4.9, 0.20), (2.9, 2.9, 0.20),
              (5.6, 3.0, 0.20), (7.6, 5.4, 0.20)]
# name -> (problem, nsteps, horizon, n)
PROBLEMS = {"shipped": (0, 0, 0.0, 0.0), "quad_256": (1, 255, 4.0, 2.0), "fixedwing_129": (2, 128, 12.0, 20.0), "quad_c3": (1, 1023, 4.0, 20.0)}


@pytest.fixture(scope="module")
def H(built):
    import torch  # noqa: F401
    lib = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    lib.harness_cs_solve.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_double, C.c_double, C.c_int]
    lib.harness_cs_get.argtypes = [C.c_char_p, DP, C.c_int]
    lib.harness_cs_message.restype = C.c_char_p
    lib.harness_cs_certify.argtypes = [DP, C.c_int, DP, C.c_int, DP, C.c_int, DP]
    return lib


def _get(H, name):
    n = H.harness_cs_get(name.encode(), None, 0)
    assert n >= 0, name
    a = np.zeros(max(n, 1))
    H.harness_cs_get(name.encode(), a.ctypes.data_as(DP), n)
    return a[:n]


def _solve(H, name, xmls, certify):
    problem, nsteps, horizon, n = PROBLEMS[name]
    xml = xmls["ocp_2d_ex1.xml"].encode() if problem == 0 else b""
    rc = H.harness_cs_solve(problem, xml, nsteps, horizon, n, int(certify))
    assert rc == 0, H.harness_cs_message().decode()
    out = {k: _get(H, k) for k in ("X", "U", "lamF", "lamC", "cert", "zl", "zu", "cl", "cu", "dims", "stats", "runs", "params", "tau")}
    ns, nc, npth, M = (int(v) for v in out["dims"][:4])
    out.update(ns=ns, nc=nc, np=npth, M=M, model=int(out["dims"][7]), t0=out["dims"][8], tf=out["dims"][9])
    for k, r in (("X", ns), ("U", nc), ("lamF", ns), ("lamC", npth), ("zl", ns + nc), ("zu", ns + nc)):
        out[k] = out[k].reshape(r, M)
    return out


_cache = {}


def solved(H, name, xmls):
    """the problem solved twice in this process: Alg::certify = false, then the default (the solver of the second stays held)"""
    if name not in _cache:
        off = _solve(H, name, xmls, False)
        on = _solve(H, name, xmls, True)
        _cache.clear()                       # one held solver at a time: certify() calls go to the last solve
        _cache[name] = (off, on)
    return _cache[name]


def oracle_certificate(s):
    """numpy certificate from ORACLE values at the returned point, and the allowances of the module docstring"""
    import etol_amd as E
    M, ns, nc, npth = s["M"], s["ns"], s["nc"], s["np"]
    mesh = O.lgl(M)
    node_t = s["t0"] + (s["tf"] - s["t0"]) / 2.0 * (mesh[0] + 1.0)
    recs = tracks = None
    if s["model"] == 0:
        recs, tx, ty = cases.ocp2d_tables(O.edge_ellipse, O.track_centres, node_t)
        tracks = (tx, ty)
    elif npth:
        recs = np.array([[1, x, y, r * r, 0, 0, 0, 0] for x, y, r in QUAD_DISCS[:npth]], dtype=float)
    X, U = s["X"][None], s["U"][None]
    RES, VALS, COST = O.evaluate(s["model"], s["params"], M, mesh, s["t0"], s["tf"], X, U, recs, tracks)
    ev = E.Evaluator(0)                      # only asked for the published pattern of VALS
    ev.set_mesh(M, s["t0"], s["tf"])
    ev.set_model(s["model"], s["params"])
    ev.set_batch(1)
    if tracks is not None:
        ev.set_tracks(*tracks)
    if recs is not None:
        ev.set_path(recs, 0, 1)
    assert ev.layout.np == npth and ev.layout.nvals == VALS.shape[1]
    pat = A.entry_pattern(*ev.jac_structure(), ns, nc, npth, M)
    ev.close()
    lamF, lamC = s["lamF"][None], s["lamC"][None]
    G = A.lagr_grad(VALS, lamF, lamC, 1.0, mesh[2], pat, ns, nc)
    T = A.lagr_grad(VALS, lamF, lamC, 1.0, mesh[2], pat, ns, nc, absolute=True)
    cert = A.certificate(G, RES, X, U, VALS, lamF, lamC, 1.0, s["zl"], s["zu"], s["cl"], s["cu"])[0]
    tol_G = float((A.bound(T, M, ns + nc, npth) + 5e-13 * T).max())
    z = np.concatenate([X[0], U[0]])
    widest = max(np.where(np.abs(s["zl"]) < 1e19, np.abs(z - s["zl"]), 0.0).max(), np.where(np.abs(s["zu"]) < 1e19, np.abs(s["zu"] - z), 0.0).max())
    cmax = np.abs(RES[0, ns:]).max() + 1.0 if npth else 0.0
    dscale = (np.einsum("kj,ij->ik", np.abs(mesh[2]), np.abs(s["X"])) + np.abs(RES[0, :ns]) + 1.0).max()
    tol = dict(stat=tol_G, comp=tol_G * widest + cert[5] * 5e-13 * cmax, defect=5e-13 * dscale, viol=5e-13 * cmax,
               gmax=5e-13 * (np.abs(VALS[0, -(ns + nc):]).max() + 1.0), lmax=0.0)
    return cert, tol


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_certificate_of_a_solve(H, xmls, name):
    off, on = solved(H, name, xmls)
    # 5. the certificate step leaves the iterates alone
    assert off["cert"][6] == 0.0 and not off["cert"][:6].any()
    assert on["cert"][6] == 1.0
    assert off["stats"][1] == on["stats"][1] and off["stats"][0] == on["stats"][0]
    assert np.array_equal(off["X"], on["X"]) and np.array_equal(off["U"], on["U"])
    assert np.array_equal(off["lamF"], on["lamF"]) and np.array_equal(off["lamC"], on["lamC"])
    s = on
    dev = dict(zip(A.FIELDS, s["cert"][:6]))
    # 1. against the oracle
    ref, tol = oracle_certificate(s)
    for q, f in enumerate(A.FIELDS):
        print(f"{name}: {f}: Sol::certificate {dev[f]:.6e}  oracle {ref[q]:.6e}  allowance {tol[f]:.3e}")
    for q, f in enumerate(A.FIELDS):
        assert abs(dev[f] - ref[q]) <= tol[f], (f, dev[f], ref[q], tol[f])
    # 2.
    assert dev["defect"] <= 1e-6
    # 3.
    mult = np.concatenate([np.abs(s["lamF"]).ravel(), np.abs(s["lamC"]).ravel()])
    sd = max(100.0, mult.mean()) / 100.0
    level = s["stats"][6] * s["stats"][5]
    assert level == 100.0 * 1e-6
    print(f"{name}: stationarity / s = {dev['stat'] / sd:.3e}, complementarity / s = {dev['comp'] / sd:.3e}, s = {sd:.3e}, level {level:.1e}, "
          f"kkt_error {s['stats'][3]:.3e}, iterations {int(s['stats'][1])}")
    assert dev["stat"] / sd <= level, (dev["stat"], sd)
    assert dev["comp"] / sd <= level, (dev["comp"], sd)


def test_certificate_tells_a_pushed_point_from_the_config3_solution(H, xmls):
    off, s = solved(H, "quad_c3", xmls)
    M, ns, nc = s["M"], s["ns"], s["nc"]
    cert = np.zeros(7)

    def certify(X, U):
        z = np.ascontiguousarray(np.concatenate([X.ravel(), U.ravel()]))
        lf, lc = np.ascontiguousarray(s["lamF"].ravel()), np.ascontiguousarray(s["lamC"].ravel())
        assert H.harness_cs_certify(z.ctypes.data_as(DP), z.size, lf.ctypes.data_as(DP), lf.size, lc.ctypes.data_as(DP), lc.size,
                                    cert.ctypes.data_as(DP)) == 0
        return cert.copy()

    again = certify(s["X"], s["U"])
    assert np.array_equal(again, s["cert"])                      # certify() of the returned point is Sol::certificate, bit for bit
    U = s["U"].copy()
    U[1, M // 2] += 1e-3
    pushed = certify(s["X"], U)
    print(f"config 3: stationarity {again[0]:.3e} / complementarity {again[1]:.3e} at the solution, {pushed[0]:.3e} / {pushed[1]:.3e} "
          f"with one control moved by 1e-3")
    assert pushed[6] == 1.0 and pushed[0] >= 10.0 * again[0]
    # Every variable of this problem is boxed, so `stationarity` (the part of G on sides WITHOUT a bound) is zero at both points and the
    # line above cannot tell them apart; the gradient the push creates shows where the table puts it for bounded sides: in
    # `complementarity`, G+ (z - zl) / G- (zu - z).  That figure must tell the difference.
    assert again[0] == 0.0 and pushed[1] >= 10.0 * again[1] and pushed[1] > 0
