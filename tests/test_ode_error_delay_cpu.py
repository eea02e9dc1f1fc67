"""emi_ode_error_delay_operator (host) against the long-double restatement of tests/ode_error_delay_ref.py, the rows the definition
fixes exactly, and the bound of that file on the reference alone: on every input the GPU test uses, the float64 restatement of the
definition must stay within the derived bound of the long-double one (ratio <= 1) -- if it does not, the derivation is wrong.
`make check-ode-delay-operator` runs the operator in a stand-alone program under the host sanitizers.  No GPU needed.

The operator's gate (derived).  Library and restatement take the same rounded (tau, w, x_p) and form the same barycentric row in
extended precision (u64 = 2^-64): each of the M terms lam_j = sw_j / (x - tau_j) carries two roundings (the difference of two doubles
is exact), their sum M - 1 more, the quotient one: (M + 2) u64 times the Lebesgue sum sum_j |ref_pj| on either side, whatever the order
of the sum.  Up to M = 512 that is below 2^-55 sum_j |ref_pj|, a quarter of an ulp of double; the library then rounds its row to
double once (2^-53 |ref_pj|), and the same allowance covers the restatement's side:
        |Edel - ref|_pj <= 2 * 2^-53 sum_j |ref_pj|        elementwise."""
import os
import subprocess

import numpy as np
import pytest

import ode_error_delay_ref as D
import ode_error_ref as R

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (2, 3, 9, 41, 65)
T0, TF = 0.25, 3.0
# delays as fractions of the horizon tf - t0: 0.05, 0.3 and 1.7 of it, 1.7 of the half horizon h (most points clamped, not all), and one
# far beyond the horizon; at 1.7 and 2.5 every row is e_0
FRACTIONS = (0.05, 0.3, 0.85, 1.7, 2.5)


def _operator(M, delay, t0=T0, tf=TF, mesh=None):
    import etol_amd as E
    return E.Evaluator.ode_error_delay_operator(M, mesh, t0, tf, delay)


@pytest.mark.parametrize("M", SIZES)
def test_operator_against_the_long_double_restatement(built, M):
    import etol_amd as E
    tau, w, _ = E.lgl(M)
    tq = E.Evaluator.ode_error_operator(M)[2]
    e0 = np.zeros(M)
    e0[0] = 1.0
    for frac in FRACTIONS:
        delay = frac * (TF - T0)
        got = _operator(M, delay)
        ref = D.delay_operator(tau, w, tq, T0, TF, delay)
        assert got.shape == ref.shape == (5 * (M - 1), M)
        leb = np.abs(ref).sum(1, keepdims=True).astype(np.float64)
        ratio = float((np.abs(got.astype(LD) - ref).astype(np.float64) / (2 * R.U53 * leb)).max())
        rows = float((np.abs(got.astype(LD).sum(1) - 1).astype(np.float64) / (2 * R.U53 * leb[:, 0])).max())
        x, before = D.shifted_points(tq, T0, TF, delay)
        print(f"M {M} delay {frac} of the horizon: |Edel - ref| {ratio:.3f}, |row sum - 1| {rows:.3f} of 2 * 2^-53 sum |ref|; "
              f"{int(before.sum())} of {len(x)} points at or before t0")
        assert ratio <= 1.0 and rows <= 1.0, (M, frac, ratio, rows)
        assert (got[before] == e0).all()                                    # a point with t_p - delay <= t0 gives exactly e_0
        if frac >= 1.0:
            assert before.all() and (got == e0).all()
        else:
            assert before.any() and not before.all()                        # the shorter delays clamp some points and not others


def test_an_abscissa_that_is_a_node_gives_that_nodes_unit_row(built):
    """a delay built so that x_p == tau_j holds in double: the row is e_j, not a division by zero"""
    import etol_amd as E
    found = 0
    for M, t0, tf in ((9, 0.0, 2.0), (41, 0.0, 2.0), (9, T0, TF)):
        tau, w, _ = E.lgl(M)
        tq = E.Evaluator.ode_error_operator(M)[2]
        h = (tf - t0) / 2.0
        tp = t0 + h * (tq + 1.0)
        for p in range(len(tq) - 1, len(tq) - 6, -1):                         # late points, early interior nodes
            for j in range(1, M - 1):
                tj = t0 + h * (tau[j] + 1.0)
                if tj >= tp[p]:
                    break
                cand = tp[p] - tj
                for _ in range(16):                                         # the few doubles around tp - tj
                    x, before = D.shifted_points(tq[p:p + 1], t0, tf, cand)
                    if x[0] == tau[j] and not before[0]:
                        row = _operator(M, cand, t0, tf)[p]
                        want = np.zeros(M)
                        want[j] = 1.0
                        assert (row == want).all(), (M, p, j)
                        found += 1
                        break
                    cand = np.nextafter(cand, np.inf if x[0] > tau[j] else -np.inf)
    print(f"{found} (point, node) pairs with x_p == tau_j in double")
    assert found >= 1


def test_operator_statuses(built):
    import etol_amd as E
    lib = E.load()
    tau, w, _ = E.lgl(3)
    dp = lambda a: a.ctypes.data_as(E._lib._D)
    out = np.empty((10, 3))
    call = lambda M=3, t=dp(tau), ww=dp(w), t0=0.0, tf=1.0, delay=0.1, o=dp(out): lib.emi_ode_error_delay_operator(M, t, ww, t0, tf, delay, o)
    assert call() == 0
    assert call(delay=0.0) == 0
    assert call(M=1) == 1 and call(t=None) == 1 and call(ww=None) == 1 and call(o=None) == 1
    assert call(tf=0.0) == 1 and call(tf=-1.0) == 1 and call(delay=-0.1) == 1


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_float64_restatement_within_the_bound(built, case):
    """the bound on the reference alone, on every input of tests/test_gpu_ode_error_delay.py"""
    name, B, M, dtf = case
    c, ref = D.case(*case), D.reference(*case)
    f64 = D.estimate(c, ref["tq"], dtype=np.float64)
    re, rr = R.ratios(f64["eta"], f64["err"], ref, M)
    print(f"{D.case_id(case)}: float64 against long double: eta {re:.3f}, err {rr:.3f} of the bound; err {float(ref['err'].max()):.3e}, "
          f"clipped points {ref['clipped'].tolist()}, on a delayed control copy {ref['clipped_delayed'].tolist()}")
    assert np.isfinite(ref["eta"].astype(np.float64)).all()
    assert re <= 1.0 and rr <= 1.0, (case, re, rr)
    b = R.overshoot_instance(B)
    assert ref["clipped"][b] >= 1 and ref["clipped_delayed"][b] >= 1
    # the delays are there: without them (every slot the undelayed value) the estimate is another one
    if dtf < 1.0:
        _, before = D.shifted_points(ref["tq"], c["t0"], c["tf"], c["dt"])
        assert before.any() and not before.all()


def test_the_sanitized_program_passes(built, tmp_path_factory):
    """`make check-ode-delay-operator`: the operator in a stand-alone program under -fsanitize=address,undefined"""
    out = tmp_path_factory.mktemp("odel") / "ode_delay_operator_check"
    r = subprocess.run(["make", "-C", ROOT, "check-ode-delay-operator", f"ODE_DEL_CHECK_OUT={out}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ode_delay_operator_check: ok" in r.stdout
