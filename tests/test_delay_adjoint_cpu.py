"""The adjoint pass of problems with delays without a GPU: the new entry points are declared, bound and refuse a NULL context;
and the numpy fold the GPU tests use as their reference (tests/delay_adjoint_ref.py) against central differences of the ORACLE's
Lagrangian.

The reference check: oracle model 3 (2 states, 2 free controls, state horizon 3, control horizon 1, one disc row), the delayed
values formed with the oracle's own interpolation matrices.  A directional derivative of
    L(X, U) = sigma COST + sum lamF . defect + sum lamC . c
by central differences (h = 1e-5: truncation ~ h^2 and round-off ~ eps |L| / h, both ~ 1e-10 of the derivative) must agree with
<G, direction> within 1e-7 relative.  The threshold sits between what the fold was measured at when the formula was written down
(1e-11 .. 3e-10) and what the gradient WITHOUT the fold gives (2e-3 .. 1.5e-2): a wrong fold cannot pass, round-off cannot fail."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import delay_adjoint_ref as R
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("emi_lagr_grad_total_dev", "emi_lagr_grad_total_host", "emi_kkt_certificate_total_dev", "emi_kkt_certificate_total_host")
P3 = [0.7, 0.3]
DISC = np.array([[1.0, 2.0, 1.5, 0.25, 0, 0, 0, 0]])
NS, NCF, XH, UH = 2, 2, 3, 1


def test_total_entry_points_are_declared_and_bound(built):
    from etol_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "emi355x.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.SYMBOLS and getattr(lib, name).argtypes == L.SYMBOLS[name][1]
    # one trailing pointer more than the calls they extend
    for name in NEW:
        assert len(L.SYMBOLS[name][1]) == len(L.SYMBOLS[name.replace("_total", "")][1]) + 1
    assert lib.emi_abi_version() == 2
    import etol_amd as E
    for m in ("lagr_grad_total_host", "lagr_grad_total_dev", "kkt_certificate_total_host", "kkt_certificate_total_dev"):
        assert callable(getattr(E.Evaluator, m))


def test_total_entry_points_without_a_device_are_an_error_not_a_fallback(built):
    import torch
    from etol_amd import _lib as L
    if torch.cuda.is_available():
        return
    lib = L.load()
    one = np.zeros(8)
    p = one.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.emi_lagr_grad_total_host(None, p, p, p, 1.0, p, p) == 4
    assert lib.emi_lagr_grad_total_dev(None, None, None, None, 1.0, None, None) == 4
    assert lib.emi_kkt_certificate_total_host(None, p, p, p, p, 1.0, p, p, 1, p, p, p, p, p) == 4
    assert lib.emi_kkt_certificate_total_dev(None, None, None, None, None, None, None, 1.0, None, None, 1, None, None, None, None, None) == 4
    assert L.STATUS[4] == "EMI_ERR_NO_DEVICE"


def test_slot_order_is_that_of_emi_set_delays():
    assert R.slots(2, 2, 3, 1) == [(0, 1), (1, 1), (0, 2), (1, 2), (2, 1), (3, 1)]
    assert R.slots(6, 1, 0, 1) == [(6, 1)] and R.slots(6, 1, 1, 0) == []
    assert list(R.copies(2, 2, 3, 1)) == [2, 2, 1, 1]


def delay_case(M, B, seed=0):
    t0, tf, dt = 0.0, 6.0, 0.2
    mesh = O.lgl(M)
    tau = mesh[0]
    t = t0 + (tf - t0) / 2 * (tau + 1)
    rng = np.random.default_rng(1000 * M + B + seed)
    X = np.stack([1 + 0.5 * np.sin(0.7 * t + rng.uniform(0, 3, (B, 1))), 2 - 0.1 * t + 0.3 * np.cos(t + rng.uniform(0, 3, (B, 1)))], axis=1)
    U = np.stack([0.3 * np.cos(t + rng.uniform(0, 3, (B, 1))), 0.2 + 0.1 * np.sin(2 * t + rng.uniform(0, 3, (B, 1)))], axis=1)
    lamF, lamC = rng.standard_normal((B, NS, M)), rng.standard_normal((B, 1, M))
    dX, dU = rng.standard_normal((B, NS, M)), rng.standard_normal((B, NCF, M))
    return dict(M=M, B=B, t0=t0, tf=tf, dt=dt, mesh=mesh, X=np.ascontiguousarray(X), U=np.ascontiguousarray(U), lamF=lamF, lamC=lamC,
                sigma=0.8, dX=dX, dU=dU)


@pytest.mark.parametrize("M,B", [(33, 3), (47, 2), (128, 4)])
def test_numpy_fold_against_central_differences_of_the_oracle_lagrangian(built, M, B):
    c = delay_case(M, B)
    W = R.oracle_delay_matrices(M, c["mesh"][0], c["t0"], c["tf"], c["dt"], XH, UH)
    Uext = R.extended(c["X"], c["U"], W, NS, NCF, XH, UH)
    assert Uext.shape == (B, 8, M)
    VALS = O.evaluate(3, P3, M, c["mesh"], c["t0"], c["tf"], c["X"], Uext, DISC)[1]
    pat = R.table_pattern(NS, 8, 1)
    assert len(pat) == VALS.shape[1]
    G, Gdel = R.lagr_grad_total(VALS, c["lamF"], c["lamC"], c["sigma"], c["mesh"][2], pat, NS, 8, NCF, XH, UH, W)
    assert G.shape == (B, NS + NCF, M) and Gdel.shape == (B, 6, M)
    args = (3, P3, c["mesh"], c["t0"], c["tf"], c["X"], c["U"], W, NS, NCF, XH, UH, c["lamF"], c["lamC"], c["sigma"])
    fd, an = R.directional_check(*args, G, c["dX"], c["dU"], recs=DISC)
    rel = abs(fd - an) / abs(fd)
    # the same without the fold: the node-local gradient alone is not the derivative
    Gx = R.A.lagr_grad(VALS, c["lamF"], c["lamC"], c["sigma"], c["mesh"][2], pat, NS, 8)
    _, an0 = R.directional_check(*args, Gx[:, :NS + NCF], c["dX"], c["dU"], recs=DISC)
    rel0 = abs(fd - an0) / abs(fd)
    print(f"M={M} B={B}: central difference {fd:.12e}, <G, d> {an:.12e}: relative {rel:.2e}; without the fold {rel0:.2e}")
    assert rel <= 1e-7
    assert rel0 > 1e-5
