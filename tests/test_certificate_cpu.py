"""The numpy certificate the GPU tests use as their reference (tests/adjoint_ref.py), checked on an NLP small enough to solve by
hand; and the adjoint entry points of the C ABI on a box without a device.  No GPU needed."""
import ctypes as C

import numpy as np

import adjoint_ref as A

# One node (M = 1, D = [[0]]), one state x, one control u, one "defect" row and one path row:
#     minimise (x - 2)^2 + (u - 1)^2   subject to   x + u - 2 = 0,   x <= 0.5,   -10 <= u <= 10   (x has no bounds)
# KKT point: the path row is active, x = 0.5, u = 1.5;  2 (u - 1) + lamF = 0 -> lamF = -1;
# 2 (x - 2) + lamF + lamC = 0 -> lamC = 4 (>= 0: an active UPPER bound, the sign convention of emi_hess_*).
# Every number is a dyadic rational: the expected figures are exact.
PATTERN = [(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (2, -1, 0), (2, -1, 1)]     # defect/x, defect/u, path/x, path/u, cost/x, cost/u
D1 = np.zeros((1, 1))
ZL = np.array([[[-1e20], [-10.0]]])
ZU = np.array([[[1e20], [10.0]]])
CL, CU = np.array([-1e20]), np.array([0.5])
LAMF, LAMC = np.array([[[-1.0]]]), np.array([[[4.0]]])


def _point(x, u):
    X, U = np.array([[[x]]]), np.array([[[u]]])
    RES = np.array([[[x + u - 2.0], [x]]])
    VALS = np.array([[[1.0], [1.0], [1.0], [0.0], [2.0 * (x - 2.0)], [2.0 * (u - 1.0)]]])
    return X, U, RES, VALS


def _certify(x, u):
    X, U, RES, VALS = _point(x, u)
    G = A.lagr_grad(VALS, LAMF, LAMC, 1.0, D1, PATTERN, 1, 1)
    return G, A.certificate(G, RES, X, U, VALS, LAMF, LAMC, 1.0, ZL, ZU, CL, CU)[0]


def test_numpy_certificate_is_exactly_zero_at_a_hand_solved_kkt_point():
    G, cert = _certify(0.5, 1.5)
    assert np.array_equal(G, np.zeros((1, 2, 1)))
    assert dict(zip(A.FIELDS, cert)) == dict(stat=0.0, comp=0.0, defect=0.0, viol=0.0, gmax=3.0, lmax=4.0)


def test_numpy_certificate_one_step_away_from_the_kkt_point():
    # x = 0.25: G_x = 2 (0.25 - 2) - 1 + 4 = -0.5 on a free variable -> stat 0.5; the path row has slack 0.25 with lamC = 4 -> comp 1
    G, cert = _certify(0.25, 1.5)
    assert G[0, 0, 0] == -0.5 and G[0, 1, 0] == 0.0
    assert dict(zip(A.FIELDS, cert)) == dict(stat=0.5, comp=1.0, defect=0.25, viol=0.0, gmax=3.5, lmax=4.0)
    # u = 10.5 as well: above its upper bound by 0.5; G_u = 2 * 9.5 - 1 = 18 > 0 is a lower-bound multiplier at distance 20.5 from
    # the lower bound -> comp 369; a boxed variable does not enter stat
    G, cert = _certify(0.25, 10.5)
    assert G[0, 1, 0] == 18.0
    assert dict(zip(A.FIELDS, cert)) == dict(stat=0.5, comp=369.0, defect=8.75, viol=0.5, gmax=19.0, lmax=4.0)
    # the path row violated: x = 1 -> c - cu = 0.5, no slack, comp of the row 0
    _, cert = _certify(1.0, 1.0)
    assert cert[3] == 0.5 and cert[2] == 0.0


def test_numpy_certificate_branches_of_the_table():
    X, U, RES, VALS = _point(0.5, 1.5)
    G = np.array([[[-2.0], [3.0]]])
    cert = lambda zl, zu, cl=CL, cu=CU, lc=LAMC: A.certificate(G, RES, X, U, VALS, LAMF, lc, 1.0, zl, zu, cl, cu)[0]
    inf = 1e20
    # both free: |G|
    assert cert([[[-inf], [-inf]]], [[[inf], [inf]]])[0] == 3.0
    # x lower-only at 0: G- = 2 has no upper bound to belong to -> stat 2; u upper-only at 2: G+ = 3 has no lower bound -> stat 3
    c = cert([[[0.0], [-inf]]], [[[inf], [2.0]]])
    assert c[0] == 3.0 and c[1] == 0.0              # G+ of x is 0, G- of u is 0: no complementarity product
    # fixed variables contribute nothing
    c = cert([[[0.5], [1.5]]], [[[0.5], [1.5]]])
    assert c[0] == 0.0 and c[1] == 0.0 and c[3] == 0.0
    # a multiplier of the wrong sign on a one-sided row counts in full: lamC = -4 with no lower bound
    assert cert(ZL, ZU, lc=np.array([[[-4.0]]]))[1] >= 4.0
    # two-sided row 0 <= c <= 0.5 at c = 0.5: lamC- times the distance to the lower bound
    assert cert([[[-inf], [-inf]]], [[[inf], [inf]]], cl=np.array([0.0]), lc=np.array([[[-4.0]]]))[1] == 2.0
    # forward-error bound: elementwise, in units of T
    T = A.lagr_grad(VALS, LAMF, LAMC, 1.0, D1, PATTERN, 1, 1, absolute=True)
    assert np.array_equal(T, np.array([[[8.0], [2.0]]]))
    assert A.bound(T, 1, 2, 1)[0, 0, 0] == 2 * 6 * A.EPS * 8.0


def test_adjoint_entry_points_without_a_device_are_an_error_not_a_fallback(built):
    """No context can exist on a box without a GPU (emi_create: EMI_ERR_NO_DEVICE); the host forms then say so too."""
    import torch
    from etol_amd import _lib as L
    if torch.cuda.is_available():
        return
    lib = L.load()
    one = np.zeros(8)
    p = one.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.emi_lagr_grad_host(None, p, p, p, 1.0, p) == 4
    assert lib.emi_kkt_certificate_host(None, p, p, p, p, 1.0, p, p, 1, p, p, p, p) == 4
    assert lib.emi_lagr_grad_dev(None, None, None, None, 1.0, None) == 4
    assert L.STATUS[4] == "EMI_ERR_NO_DEVICE"
