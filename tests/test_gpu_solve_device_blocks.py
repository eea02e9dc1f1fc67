"""ETOL::eMI355X::solve() with Alg::node_blocks = "device": the node blocks of every factorisation attempt assembled and made
positive definite by emi_kkt_blocks_dev and handed to emi_kkt_factor_dev without leaving the device
(tests/harness/etol_harness_blocks.cpp).  -m gpu

The 41-node quadrotor with 2 keep-outs (stored optimum in tests/golden/solve_optima.json) and the 49-node fixed wing (strongly
indefinite 16 x 16 blocks, inertia search); both above the 400-row switch to the device backend.  With "device" each converges
within its budget, lands within 1e-6 relative of the "host" solution of the same run (and of the stored optimum), and returns a
certificate at the level tests/test_gpu_solve_certificate.py asks of a solve: defect <= 1e-6, stationarity / s and
complementarity / s <= acceptable_factor * nlp_tolerance.  The budget is Alg's default (nlp_iter_max 200 per NLP solve).
Iteration counts of both modes are printed here and written to profiles/blocks_times.jsonl by tools/blocks_times.py --part solve
(a test writes nothing into the tree); they are not gated: the Jacobi order differs, so the iterates need not coincide."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
# name -> (problem, nsteps, horizon, n, states, controls)
PROBLEMS = {"quadrotor_41": (1, 40, 4.0, 2.0, 6, 2), "fixedwing_49": (2, 48, 8.0, 10.0, 12, 4)}
TOL = 1e-8          # nlp_tolerance of both modes (what tests/test_gpu_solve.py solves its parity problems with)


@pytest.fixture(scope="module")
def H(built):
    import torch  # noqa: F401
    lib = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    lib.harness_blk_solve.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double]
    lib.harness_blk_get.argtypes = [C.c_char_p, DP, C.c_int]
    lib.harness_blk_message.restype = C.c_char_p
    return lib


def _get(H, name):
    n = H.harness_blk_get(name.encode(), None, 0)
    assert n >= 0, name
    a = np.zeros(max(n, 1))
    H.harness_blk_get(name.encode(), a.ctypes.data_as(DP), n)
    return a[:n]


def _solve(H, name, device_blocks):
    problem, nsteps, horizon, n, ns, nc = PROBLEMS[name]
    rc = H.harness_blk_solve(problem, nsteps, horizon, n, int(device_blocks), TOL)
    assert rc == 0, H.harness_blk_message().decode()
    out = {k: _get(H, k) for k in ("X", "U", "lamF", "lamC", "cert", "stats", "runs", "on_device")}
    H.harness_blk_release()
    M = nsteps + 1
    out["X"], out["U"] = out["X"].reshape(ns, M), out["U"].reshape(nc, M)
    return out


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_solve_with_device_node_blocks(H, name):
    host = _solve(H, name, False)
    dev = _solve(H, name, True)
    assert host["on_device"].tolist() == [1.0, 0.0] and dev["on_device"].tolist() == [1.0, 1.0]      # Newton step, node blocks
    runs = lambda s: s["runs"].reshape(-1, 6)
    print(f"{name}: iterations host {int(host['stats'][1])} / device {int(dev['stats'][1])}; factorisations "
          f"{int(runs(host)[:, 5].sum())} / {int(runs(dev)[:, 5].sum())}; t_blocks {runs(host)[:, 3].sum():.4f} s / {runs(dev)[:, 3].sum():.4f} s; "
          f"cost {host['stats'][0]:.10f} / {dev['stats'][0]:.10f}; kkt_error {host['stats'][3]:.2e} / {dev['stats'][3]:.2e}")
    # within 1e-6 relative of the host mode's solution
    ex = np.abs(dev["X"] - host["X"]).max() / np.abs(host["X"]).max()
    eu = np.abs(dev["U"] - host["U"]).max() / np.abs(host["U"]).max()
    ec = abs(dev["stats"][0] - host["stats"][0]) / abs(host["stats"][0])
    print(f"{name}: device against host: states {ex:.2e}, controls {eu:.2e}, cost {ec:.2e}")
    assert ex < 1e-6 and eu < 1e-6 and ec < 1e-6, (ex, eu, ec)
    if name == "quadrotor_41":          # ... and of the stored optimum
        from test_gpu_solve import _assert_trajectory_parity
        _assert_trajectory_parity("quadrotor_41 (device node blocks)", dev["stats"][0], dev["X"], dev["U"], "quadrotor_41")
    # the certificate, judged as tests/test_gpu_solve_certificate.py judges a solve
    cert = dict(zip(("stat", "comp", "defect", "viol", "gmax", "lmax"), dev["cert"][:6]))
    assert dev["cert"][6] == 1.0
    assert cert["defect"] <= 1e-6
    mult = np.concatenate([np.abs(dev["lamF"]).ravel(), np.abs(dev["lamC"]).ravel()])
    sd = max(100.0, mult.mean()) / 100.0
    level = dev["stats"][6] * dev["stats"][5]
    print(f"{name}: stationarity / s = {cert['stat'] / sd:.3e}, complementarity / s = {cert['comp'] / sd:.3e}, level {level:.1e}")
    assert cert["stat"] / sd <= level and cert["comp"] / sd <= level, (cert, sd, level)
