"""The mesh strategy of eMI355X::solve() (mi355x::MeshDriver, etol_amd/host/emi_mesh_driver.cpp) without a GPU: its decision tree under
a scripted solver, and one real sequenced solve with the CPU oracle as evaluator."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_decision_tree_under_a_scripted_solver_as_a_stand_alone_program_under_the_host_sanitizers(built, tmp_path):
    """tests/harness/mesh_driver_main.cpp implements the driver's host interface with a script (every NLP call returns the next scripted
    result and records what it was asked) and asserts the whole sequence of solves, mesh changes and printed lines for: a straight
    climb, a failed second rung, a first rung that never converges, a failed warm start on the requested mesh, every start used up,
    the iteration budget, warm patience, refinement falling back and stopping, inflated keep-outs, and the Prob left as it was.
    Built with -fsanitize=address,undefined (`make check-mesh-driver`)."""
    r = subprocess.run(["make", "-C", ROOT, "-j4", "check-mesh-driver", f"MESH_CHECK_OUT={tmp_path / 'mesh_driver_check'}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "mesh driver: ok" in r.stdout


@pytest.fixture(scope="module")
def H(built):
    import torch  # noqa: F401  (one HIP runtime per process: see etol_amd/_lib.py)
    lib = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.harness_solve_example1_sequenced_oracle.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_int, D, D, D, C.c_int,
                                                            I, C.c_int, I, I]
    lib.harness_last_message.restype = C.c_char_p
    return lib


def test_sequenced_solve_on_the_oracle_reaches_the_analytic_optimum(H, xmls):
    """The obstacle-free shipped problem on 97 nodes: the driver climbs 33 -> 65 -> 97 with the oracle's functions and the dense host
    Newton step, every solve converges, and the result is the analytic optimum within the tolerance of
    test_host_cpu.py::test_nlp_iteration_reaches_analytic_optimum (the problem is linear-quadratic: the optimum is the same on every mesh)."""
    g = json.load(open(os.path.join(GOLD, "ocp2d.json")))
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    M = 97
    X, U = np.zeros((2, M)), np.zeros((2, M))
    runs = np.zeros(3 * 8, dtype=np.int32)
    cost, nruns, mesh_iterations = C.c_double(), C.c_int(), C.c_int()
    rc = H.harness_solve_example1_sequenced_oracle(xmls["ocp_2d_ex1.xml"].encode(), os.path.join(ROOT, "oracle", "liboracle.so").encode(), 0, M, 1e-9,
                                                   0, C.byref(cost), X.ctypes.data_as(D), U.ctypes.data_as(D), M, runs.ctypes.data_as(I), 8,
                                                   C.byref(nruns), C.byref(mesh_iterations))
    assert rc == 0, H.harness_last_message().decode()
    r = runs[:3 * nruns.value].reshape(-1, 3)
    assert list(r[:, 0]) == [33, 65, 97] and all(r[:, 2] == 1), r
    assert mesh_iterations.value == 3
    assert abs(cost.value - g["cost"]) < 1e-6 * g["cost"]
    assert np.abs(U[0] - g["u"][0]).max() < 1e-6 and np.abs(U[1] - g["u"][1]).max() < 1e-6
    assert abs(X[0, 0] - 1) < 1e-12 and abs(X[1, 0] - 2) < 1e-12 and abs(X[0, -1] - 5) <= 0.01 + 1e-9 and abs(X[1, -1] - 4) <= 0.01 + 1e-9
