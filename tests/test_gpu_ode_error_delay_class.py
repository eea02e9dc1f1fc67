"""ETOL::eMI355X on a problem WITH delays: odeError() of a given trajectory, Sol::ode_error after a solve with the default Alg (the
mesh is kept) and a solve with Alg::refine_delayed (the mesh and the count of tests/golden/delay_refine_cases.json), each estimate
against the long-double restatement of tests/ode_error_delay_ref.py within its bound on err.  The problem is the delayed demo of
tests/harness/etol_harness.cpp (oracle model 3) through tests/harness/etol_harness_delay_ode_error.cpp.  -m gpu"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ode_error_delay_ref as D
import ode_error_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
DP = C.POINTER(C.c_double)
NSTEPS, DT, XH, UH = 12, 0.5, 3, 1


def _harness():
    import torch  # noqa: F401
    H = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    H.harness_doe_message.restype = C.c_char_p
    H.harness_doe_ode_error.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, DP, DP, DP, DP]
    H.harness_doe_solve.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, DP, DP, DP, DP, DP,
                                    C.c_int]
    return H


def _solve(H, refine=0, ode_tol=0.0, max_nodes=0, nlp_tol=1e-10):
    """-> dict of harness_doe_solve's figures, X, U [2][M], dims, tau [M]"""
    cap = 64
    stats, dims, tau = np.zeros(14), np.zeros(6), np.zeros(cap)
    X, U = np.zeros(2 * cap), np.zeros(2 * cap)
    rc = H.harness_doe_solve(NSTEPS, DT, XH, UH, 0, refine, ode_tol, max_nodes, nlp_tol, *(a.ctypes.data_as(DP) for a in (stats, dims, X, U, tau)), cap)
    assert rc == 0, H.harness_doe_message()
    names = ("nodes", "mesh_iterations", "ode_error", "cost", "nlp_iterations_total", "defect", "nlp_runs", "error_flag", "stationarity",
             "complementarity", "cert_defect", "cert_computed", "mean_multiplier", "level")
    s = dict(zip(names, stats))
    M = int(s["nodes"])
    s.update(M=M, X=X[:2 * M].reshape(2, M).copy(), U=U[:2 * M].reshape(2, M).copy(), dims=dims, tau=tau[:M].copy())
    return s


def _reference(X, U, dims, tau):
    """the long-double estimate of one trajectory of the demo problem on the class's mesh, and the bound on err"""
    import etol_amd as E
    M = int(dims[0])
    lt, w, Dm = E.lgl(M)
    assert np.array_equal(lt, tau)                       # the class is on the library's LGL mesh
    assert int(dims[1]) == 6 and dims[5] == 0.0         # six delayed slots; the stated problem, not the lifted one
    sp = D.SPEC["demo"]
    c = dict(name="demo", B=1, M=M, t0=dims[2], tf=dims[3], dt=dims[4], tau=lt, w=w, D=Dm, ns=2, ncf=2, nc=8, xh=XH, uh=UH, model=sp["model"],
             params=sp["params"], ul=np.array([-5.0, -5.0]), uu=np.array([5.0, 5.0]), X=np.ascontiguousarray(X[None]), U=np.ascontiguousarray(U[None]))
    ref = D.estimate(c, R.library_points(M, (lt, w)))
    return ref, R.err_bound(ref, M)[0]


def test_ode_error_of_a_given_trajectory(built):
    H = _harness()
    M = NSTEPS + 1
    import etol_amd as E
    t = (NSTEPS * DT) / 2 * (E.lgl(M)[0] + 1)
    X = np.stack([1 + 0.5 * np.sin(0.7 * t + 0.4), 2 - 0.1 * t + 0.3 * np.cos(t + 1.1)])
    U = np.stack([0.3 * np.cos(t + 2.0), 0.2 + 0.1 * np.sin(2 * t + 0.3)])
    z = np.ascontiguousarray(np.concatenate([X, U]))
    got = {}
    for route in (0, 1):                                # "host" and "device": a delayed problem takes the total call on both
        err, dims, tau = C.c_double(), np.zeros(6), np.zeros(M)
        assert H.harness_doe_ode_error(NSTEPS, DT, XH, UH, route, z.ctypes.data_as(DP), C.byref(err), dims.ctypes.data_as(DP),
                                       tau.ctypes.data_as(DP)) == 0, H.harness_doe_message()
        got[route] = err.value
    assert dims[2] == 0.0 and dims[3] == NSTEPS * DT and dims[4] == DT
    ref, bound = _reference(X, U, dims, tau)
    print(f"odeError of a given trajectory: host setting {got[0]:.6e}, device setting {got[1]:.6e}, long double {float(ref['err'][0]):.6e}, "
          f"bound on err {bound:.3e}, |err - ref| / bound {abs(float(LD(got[1]) - ref['err'][0])) / bound:.3f}")
    assert got[0] == got[1]
    assert got[1] > 1e-6                                # (a rough trajectory: the estimate is far above the bound's scale)
    assert abs(LD(got[1]) - ref["err"][0]) <= bound


def test_default_solve_reports_the_estimate_and_keeps_its_mesh(built):
    s = _solve(_harness())
    M = s["M"]
    assert M == NSTEPS + 1 and int(s["mesh_iterations"]) == 1 and int(s["nlp_runs"]) >= 1      # the one mesh, one mesh iteration: nothing is refined
    ref, bound = _reference(s["X"], s["U"], s["dims"], s["tau"])
    print(f"default solve on {M} nodes: cost {s['cost']:.10e}, {int(s['nlp_iterations_total'])} NLP iterations, defect of evaluate() "
          f"{s['defect']:.2e}, Sol::ode_error {s['ode_error']:.6e}, long double {float(ref['err'][0]):.6e}, bound on err {bound:.3e}")
    assert s["ode_error"] > 0.0                         # (0 used to read as a perfectly resolved ODE)
    assert abs(LD(s["ode_error"]) - ref["err"][0]) <= bound


def test_refine_delayed_ends_on_the_fixtures_mesh(built):
    """Alg::refine_delayed on the demo started on 13 nodes, with the tolerance of tests/golden/delay_refine_cases.json (every
    reference estimate of gen_delay_refine_cases.py lies a factor 1.2 away from it)"""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "delay_refine_cases.json")))
    assert (fx["nsteps"], fx["dt"], fx["xh"], fx["uh"]) == (NSTEPS, DT, XH, UH) and fx["meshes"][0] == NSTEPS + 1
    tol = fx["ode_tolerance"]
    assert all(e < tol / 1.2 or e > 1.2 * tol for e in fx["estimates"])
    H = _harness()
    s = _solve(H, refine=1, ode_tol=tol)
    ref, bound = _reference(s["X"], s["U"], s["dims"], s["tau"])
    sd = max(100.0, s["mean_multiplier"]) / 100.0
    print(f"refined solve: {s['M']} nodes after {int(s['mesh_iterations'])} mesh iterations ({int(s['nlp_iterations_total'])} NLP iterations), cost "
          f"{s['cost']:.10e}, Sol::ode_error {s['ode_error']:.6e} (tolerance {tol:.6e}, fixture {fx['estimates']}), long double "
          f"{float(ref['err'][0]):.6e}, bound on err {bound:.3e}; defect of evaluate() {s['defect']:.2e}; certificate: stationarity / s "
          f"{s['stationarity'] / sd:.2e}, complementarity / s {s['complementarity'] / sd:.2e}, defect {s['cert_defect']:.2e}, level {s['level']:.1e}")
    assert s["M"] == fx["final_nodes"] and int(s["mesh_iterations"]) == fx["mesh_iterations"]
    assert s["ode_error"] <= tol
    assert abs(LD(s["ode_error"]) - ref["err"][0]) <= bound
    assert s["dims"][4] == DT and s["dims"][3] == NSTEPS * DT       # the physical delay and the horizon did not change with the mesh
    assert s["defect"] < 1e-8                                       # evaluate() on the stated problem: the DELAYED dynamics hold at the nodes
    # the certificate is at the level of the solve (the rule of tests/test_gpu_delay_solve_certificate.py)
    assert s["cert_computed"] == 1.0 and s["level"] == 100.0 * 1e-10
    assert s["stationarity"] / sd <= s["level"] and s["complementarity"] / sd <= s["level"] and s["cert_defect"] <= 1e-8
    # mr_max_nodes below the next mesh: the solve stops on the present mesh and reports its estimate
    c = _solve(H, refine=1, ode_tol=tol, max_nodes=NSTEPS + 1)
    refc, boundc = _reference(c["X"], c["U"], c["dims"], c["tau"])
    print(f"mr_max_nodes {NSTEPS + 1}: {c['M']} nodes, {int(c['mesh_iterations'])} mesh iteration, Sol::ode_error {c['ode_error']:.6e}")
    assert c["M"] == NSTEPS + 1 and int(c["mesh_iterations"]) == 1
    assert c["ode_error"] > tol and abs(LD(c["ode_error"]) - refc["err"][0]) <= boundc
