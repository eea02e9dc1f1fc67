"""emi_ode_error_operator (host) against the mpmath operators and against the structure an interpolation operator has, and the
bound of tests/ode_error_ref.py on the reference alone: on every input the GPU tests use, the float64 restatement of the definition
must stay within the derived bound of the long-double one (ratio <= 1) -- if it does not, the derivation is wrong.  No GPU needed."""
import numpy as np
import pytest

import ode_error_ref as R

LD = np.longdouble


@pytest.fixture(scope="module")
def golden():
    return R.operator_fixture()


def _units(got, star):
    return (np.abs(got - star) / (R.U53 * np.abs(star).sum(1, keepdims=True))).max()


def test_operator_against_mpmath(built, golden):
    import etol_amd as E
    worst = [0.0, 0.0]
    for M in R.OPERATOR_SIZES:
        Es, Eds, tqs = golden[M]
        Eo, Ed, tq = E.Evaluator.ode_error_operator(M)
        assert Eo.shape == Ed.shape == Es.shape == (5 * (M - 1), M) and tq.shape == tqs.shape
        re, rd = _units(Eo, Es), _units(Ed, Eds)
        worst = [max(worst[0], re), max(worst[1], rd)]
        print(f"M {M}: largest |E - E*| / (2^-53 sum |E*|) = {re:.1f}, |E' - E'*| / (2^-53 sum |E'*|) = {rd:.1f}, "
              f"|tq - tq*| = {np.abs(tq - tqs).max():.2e}")
        assert re <= R.E_GATE and rd <= R.ED_GATE, (M, re, rd)
        assert np.abs(tq - tqs).max() <= 4 * np.finfo(float).eps
    print(f"largest ratios over the sizes: E {worst[0]:.1f} (gate {R.E_GATE:g}), E' {worst[1]:.1f} (gate {R.ED_GATE:g})")


@pytest.mark.parametrize("M", R.OPERATOR_SIZES + (130,))
def test_operator_structure(built, M):
    import etol_amd as E
    tau, w, _ = E.lgl(M)
    Eo, Ed, tq = E.Evaluator.ode_error_operator(M)
    nq = M - 1
    aEd = np.abs(Ed).sum(1)
    assert np.abs(Eo.sum(1) - 1.0).max() <= M * 2.0 ** -52
    assert (np.abs(Ed.sum(1)) <= M * 2.0 ** -52 * aEd).all()
    for q in range(5):                  # point q (M-1) + k lies strictly inside interval k, ascending in q
        s = tq[q * nq:(q + 1) * nq]
        assert (s > tau[:-1]).all() and (s < tau[1:]).all()
        if q:
            assert (s > tq[(q - 1) * nq:q * nq]).all()
    # Legendre polynomials up to degree M - 1 and their derivatives are reproduced at tq (long double), in the units of the gate
    aE = np.abs(Eo).sum(1)
    worst = [0.0, 0.0]
    for n in range(M):
        c = np.zeros(n + 1, dtype=LD)
        c[n] = 1
        at_nodes = np.polynomial.legendre.legval(tau.astype(LD), c)
        val = np.polynomial.legendre.legval(tq.astype(LD), c)
        der = np.polynomial.legendre.legval(tq.astype(LD), np.polynomial.legendre.legder(c)) if n else np.zeros(len(tq), dtype=LD)
        # |P_n| <= 1 on the nodes: the units of the gate, 2^-53 sum_j |E_pj| |P_n(tau_j)| <= 2^-53 sum_j |E_pj|
        worst[0] = max(worst[0], float((np.abs(Eo.astype(LD) @ at_nodes - val) / (R.U53 * aE)).max()))
        worst[1] = max(worst[1], float((np.abs(Ed.astype(LD) @ at_nodes - der) / (R.U53 * aEd)).max()))
    print(f"M {M}: Legendre polynomials reproduced within {worst[0]:.1f} units, their derivatives within {worst[1]:.1f}")
    assert worst[0] <= R.E_GATE and worst[1] <= R.ED_GATE


def test_operator_statuses(built):
    import etol_amd as E
    lib = E.load()
    tau, w, _ = E.lgl(3)
    dp = lambda a: a.ctypes.data_as(E._lib._D)
    out = [np.empty((10, 3)), np.empty((10, 3)), np.empty(10)]
    assert lib.emi_ode_error_operator(1, dp(tau), dp(w), *(dp(a) for a in out)) == 1
    for miss in range(5):
        args = [dp(tau), dp(w)] + [dp(a) for a in out]
        args[miss] = None
        assert lib.emi_ode_error_operator(3, *args) == 1, miss
    assert lib.emi_ode_error_operator(3, dp(tau), dp(w), *(dp(a) for a in out)) == 0


@pytest.mark.parametrize("name", R.MODELS)
def test_float64_restatement_within_the_bound(built, name):
    """the bound on the reference alone, on every input of tests/test_gpu_ode_error.py"""
    worst = (0.0, 0.0)
    for B, M in R.SHAPES:
        for poly in ((False, True) if name == "pointmass" else (False,)):
            c, ref = R.case(name, B, M, poly), R.reference(name, B, M, poly)
            f64 = R.estimate(c, ref["tq"], dtype=np.float64)
            re, rr = R.ratios(f64["eta"], f64["err"], ref, M)
            su = (np.abs(f64["eta"].astype(LD) - ref["eta"]).astype(np.float64) / (R.U53 * ref["S"])).max()
            print(f"{name} B {B} M {M}{' polynomial' if poly else ''}: float64 against long double: eta {re:.3f}, err {rr:.3f} of the bound "
                  f"({su:.2f} units of 2^-53 S); err {float(ref['err'].max()):.3e}, clipped points {ref['clipped'].tolist()}")
            assert np.isfinite(ref["eta"].astype(np.float64)).all()
            assert re <= 1.0 and rr <= 1.0, (name, B, M, re, rr)
            assert ref["clipped"][R.overshoot_instance(B)] >= 1 or poly
            if poly:
                assert (np.abs(ref["eta"]).astype(np.float64) <= R.eta_bound(ref, M)).all()
            worst = (max(worst[0], re), max(worst[1], rr))
    print(f"{name}: largest ratios eta {worst[0]:.3f}, err {worst[1]:.3f}")
