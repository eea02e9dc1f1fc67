"""Generates tests/golden/delay_refine_cases.json: the fixture of the refinement test of a DELAYED solve
(tests/test_gpu_ode_error_delay_class.py, Alg::refine_delayed).  No GPU needed:  python tests/golden/gen_delay_refine_cases.py

The delayed demo problem (tests/harness/etol_harness_delay_ode_error.cpp; oracle model 3) is solved LIFTED on the CPU oracle on every
mesh the growth rule of MeshDriver::refine_loop visits from 13 nodes, M -> M + max(4, (M - 1) / 2), and after each solve the float64
reference estimate of tests/ode_error_delay_ref.py is taken of the stated problem (states and free controls of the solution).  The
clamp of the delayed values at t0 leaves the solution with kinks at t0 + i dt, so the estimates fall slowly and not monotonically
(2.8e-3, 1.7e-3, 1.9e-3, 1.4e-3 on 13, 19, 28, 41 nodes); the test's solve is to end on the second mesh.  Its tolerance is the
geometric middle of the interval in which the meshes before that one miss it by more than a factor 1.2 and that mesh and every
later one meet it by more than that factor; it is kept only if EVERY estimate lies outside [tol / 1.2, 1.2 tol], so that neither the
device's rounding nor the distance between two converged solves of one mesh (nlp_tolerance 1e-10) can move the mesh the solve ends on."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ode_error_delay_ref as D  # noqa: E402
import ode_error_ref as R  # noqa: E402

NSTEPS, DT, XH, UH = 12, 0.5, 3, 1
END_ON = 1              # index of the mesh the test's solve is to end on (the second mesh: one refinement)
NMESH = 4
DP = C.POINTER(C.c_double)


def meshes(first, n):
    out = [first]
    while len(out) < n:
        out.append(out[-1] + max(4, (out[-1] - 1) // 2))
    return out


def estimate(H, M, tf, delay):
    import etol_amd as E
    Z, cost, iters = np.zeros(10 * M), C.c_double(), C.c_int()
    rc = H.harness_doe_solve_oracle(os.path.join(ROOT, "oracle", "liboracle.so").encode(), M, tf, delay, 1e-10, C.byref(cost), Z.ctypes.data_as(DP),
                                    C.byref(iters))
    assert rc == 0, H.harness_doe_message().decode()
    Z = Z.reshape(10, M)
    tau, w, Dm = E.lgl(M)
    sp = D.SPEC["demo"]
    c = dict(name="demo", B=1, M=M, t0=0.0, tf=tf, dt=delay, tau=tau, w=w, D=Dm, ns=2, ncf=2, nc=8, xh=XH, uh=UH, model=sp["model"], params=sp["params"],
             ul=np.array([-5.0, -5.0]), uu=np.array([5.0, 5.0]), X=np.ascontiguousarray(Z[None, :2]), U=np.ascontiguousarray(Z[None, 2:4]))
    est = D.estimate(c, R.library_points(M, (tau, w)), dtype=np.float64)
    return float(est["err"][0]), cost.value, iters.value


def main():
    import __graft_entry__ as g
    g.build(quiet=True)
    H = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    H.harness_doe_message.restype = C.c_char_p
    H.harness_doe_solve_oracle.argtypes = [C.c_char_p, C.c_int, C.c_double, C.c_double, C.c_double, DP, DP, C.POINTER(C.c_int)]
    tf = NSTEPS * DT
    ms = meshes(NSTEPS + 1, NMESH)
    rows = [estimate(H, M, tf, DT) for M in ms]
    errs = [r[0] for r in rows]
    for M, (e, cost, it) in zip(ms, rows):
        print(f"{M} nodes: cost {cost:.10f}, {it} iterations, reference estimate {e:.6e}")
    lo, hi = 1.2 * max(errs[END_ON:]), min(errs[:END_ON]) / 1.2
    assert lo < hi, (lo, hi, errs)
    tol = float(np.sqrt(lo * hi))
    assert all(e < tol / 1.2 or e > 1.2 * tol for e in errs), (tol, errs)
    out = dict(nsteps=NSTEPS, dt=DT, xh=XH, uh=UH, meshes=ms, estimates=errs, costs=[r[1] for r in rows], ode_tolerance=tol, final_nodes=ms[END_ON],
               mesh_iterations=END_ON + 1)
    with open(os.path.join(HERE, "delay_refine_cases.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"ode_tolerance {tol:.6e}: the solve ends on {ms[END_ON]} nodes after {END_ON + 1} mesh iterations")


if __name__ == "__main__":
    main()
