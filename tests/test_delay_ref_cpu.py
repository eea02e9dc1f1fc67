"""The reference of tests/test_gpu_delay_values.py checked without a GPU: the tap models compile, the cases reach the branches of
delay_matrix they claim, the long-double product stands against plain double products in several summation orders within the
bound the device is held to, and emi_delay_matrix itself against the Lagrange product formula at 50 digits."""
import ctypes as C

import numpy as np
import pytest

import delay_adjoint_ref as DA
import delay_ref as R

_MESH = {}


def mesh(M):
    import etol_amd as E
    if M not in _MESH:
        _MESH[M] = E.lgl(M)
    return _MESH[M]


def test_long_double_has_the_significand_the_bound_assumes():
    assert np.finfo(np.longdouble).nmant >= 63


def test_tap_models_pass_the_model_source_check(built):
    """Every tap model the GPU file installs compiles for gfx950 against the f64 kernel templates (hiprtc needs no GPU)."""
    from etol_amd import _lib
    lib = _lib.load()
    assert len(R.TAP_DIMS) <= 6
    for ns, nc in R.TAP_DIMS:
        name, src = R.tap_source(ns, nc)
        log = C.create_string_buffer(1 << 16)
        st = lib.emi_check_model_source(name.encode(), src.encode(), ns, nc, 0, 0, 0, log, len(log))
        assert st == 0, (ns, nc, log.value.decode(errors="replace"))


def test_slot_order_is_that_of_the_adjoint_reference():
    for ns, ncf, xh, uh in [(c["ns"], c["ncf"], c["xh"], c["uh"]) for c in R.CASES.values()] + [(2, 2, 3, 1), (6, 1, 0, 1), (12, 1, 0, 3)]:
        assert R.slots(ns, ncf, xh, uh) == DA.slots(ns, ncf, xh, uh)
        assert len(R.slots(ns, ncf, xh, uh)) == R.nc_of(ns, ncf, xh, uh) - ncf


def test_cases_cover_the_shapes_the_product_kernel_distinguishes():
    """Tiles of 96 rows x 128 nodes: every M of the list; 1 ns, 96, 97 or 98 and more than two tiles of rows at an even and an odd
    M each; every horizon split; free controls 1, 2, 3 with ns != ncf."""
    cs = list(R.CASES.values())
    assert {c["M"] for c in cs} == {2, 3, 17, 127, 128, 129, 257}
    rows = lambda c: {c["B"] * c["ns"]} if c["xh"] > 1 else {c["B"] * c["ncf"]}
    for want in (lambda c, r: c["B"] == 1, lambda c, r: r == 96, lambda c, r: r in (97, 98), lambda c, r: r > 192):
        par = {c["M"] % 2 for c in cs for r in rows(c) if want(c, r)}
        assert par == {0, 1}
    assert {(c["xh"], c["uh"]) for c in cs} == {(2, 0), (0, 1), (1, 3), (3, 1), (4, 2)}
    assert {c["ncf"] for c in cs} == {1, 2, 3} and all(c["ns"] != c["ncf"] for c in cs)
    assert {(c["ns"], R.nc_of(c["ns"], c["ncf"], c["xh"], c["uh"])) for c in cs} <= set(R.TAP_DIMS)
    assert {(c["span"][1] - c["span"][0]) / 2 for c in cs} == {1.0, 4.0}


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_reaches_its_branches_and_double_products_stay_inside_the_bound(built, name):
    """The clamped and hit rows the case claims are there (counted on the library's own W); a numpy product in plain double, in
    five summation orders (one by one both ways, partial sums of 4 and of 16, pairwise), is within (M + 2) u S of the long-double
    reference for every call's inputs, and reproduces the source's value on every unit row."""
    c = R.case(name, mesh)
    nclamped, nhit = R.claims_hold(c)
    dims = (c["ns"], c["ncf"], c["xh"], c["uh"])
    worst = 0.0
    for call in range(c["ncalls"]):
        Z = R.inputs(c, call)
        assert {(b + call) % 3 for b in range(c["B"])} >= ({0, 1, 2} if c["B"] >= 3 else {call})
        ref, S = R.reference(Z, c["W"], *dims)
        inst = sorted(set(range(min(c["B"], 3))) | {c["B"] - 1})            # every kind of instance, and the last one
        ok, _, _ = R.unit_rows_hold(ref, Z, c["W"], c["mesh"], c["t0"], c["tf"], c["dt"], *dims)
        assert ok                                                            # the reference itself is exact on unit rows
        for order in R.ORDERS:
            got = R.emulate(Z, c["W"], *dims, order, inst)
            r = R.ratio(got, ref[inst], S[inst], c["M"])
            worst = max(worst, float(r.max()))
            assert r.max() <= 1.0, (name, call, order, float(r.max()))
            assert R.unit_rows_hold(got, Z[inst], c["W"], c["mesh"], c["t0"], c["tf"], c["dt"], *dims)[0]
        # a relative error of 1e-13 in one delayed element is outside (what the row-wise max norm of test_gpu_delays.py lets pass)
        # -- on the elements that dominate their magnitude sum (|ref| > S / 3; (M + 2) u < 3e-14 for M <= 257)
        bad = ref.copy()
        big = np.abs(ref) > (S / 3).astype(np.float64)
        assert big.any()
        bad[big] *= 1 + 1e-13
        assert (R.ratio(bad, ref, S, c["M"])[big] > 1.0).all()
    print(f"{name}: clamped rows of W(dt) {nclamped}, hit rows {nhit}, worst |double product - ref| / ((M+2) u S) = {worst:.3f}")


def test_hit_and_all_clamped_branches_on_the_host(built):
    """M = 3 on [0, 2] with dt = 1: the round trip t -> ts -> x is exact in double, node 2 lands on node 1 (the hit branch: unit row
    of node 1), node 1 on t0 (the clamp); 2 dt = tf - t0: every row is the unit row of node 0."""
    tau, w, _ = mesh(3)
    assert tau[1] == 0.0
    W = R.delay_matrices((tau, w), 0.0, 2.0, 1.0, 1, 2)
    assert np.array_equal(W[0], np.array([[1.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]]))
    unit, node, clamped, hit = R.row_kinds(W[0], tau, 0.0, 2.0, 1.0)
    assert list(clamped) == [True, True, False] and list(hit) == [False, False, True] and node[2] == 1
    assert np.array_equal(W[1], np.array([[1.0, 0, 0]] * 3))
    # without the hit branch the barycentric form divides by x - tau_1 = 0: the row would not be finite
    with np.errstate(all="ignore"):
        lam = np.array([1.0, -1.0, 1.0]) * np.sqrt(w)
        row = lam / (0.0 - tau)
        assert not np.isfinite(row / row.sum()).all()


@pytest.mark.parametrize("M", R.W_MESHES)
def test_delay_matrix_against_the_product_formula_at_50_digits(built, M):
    """emi_delay_matrix against the Lagrange product formula in mpmath on the double tau at the double x the header defines, for a
    generic delay, one half the horizon long and a short one.  The barycentric weights come from the true LGL nodes while tau is
    rounded, so a relative O(M^2 u) is inherent: the constant is measured (printed here, recorded in DESIGN.md section 2), and
    delay_ref.W_CONST is that worst figure times 4, rounded up to a power of two."""
    tau, w, _ = mesh(M)
    worst = 0.0
    for t0, tf, delay in ((0.0, 2.0, 0.37), (0.0, 8.0, 4.0), (0.5, 8.5, 0.01), (0.0, 2.0, 1.0)):
        W = R.delay_matrices((tau, w), t0, tf, delay, 2, 0)[0]
        worst = max(worst, R.w_ratio(W, tau, t0, tf, delay))
    print(f"M = {M}: worst |W - W_exact| / (u wt) = {worst:.3f} (asserted: {R.W_CONST})")
    assert worst <= R.W_CONST
