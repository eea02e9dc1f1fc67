"""The numpy reference of the interior-point arithmetic (tests/ipm_ref.py) against the HOST functions solve_nlp runs between two
evaluator calls (mi355x::ipm_*, through tests/harness/etol_harness_ipm.cpp), on the cases and under the bounds the GPU test
(tests/test_gpu_ipm.py) applies to the kernels.  No GPU needed.

Also the generator's conditions: in every sum of every case each class of terms (variable barriers, slack barriers, elastic
terms, defect and row residuals) carries at least 1e-3 of the sum of the absolute values, so a dropped term cannot hide inside a
bound; rows whose slack reset is decided within the bound of 0 stay under 1 % of all rows."""
import numpy as np
import pytest

import ipm_ref as R
from ipm_host import HostBackend, load_harness


@pytest.fixture(scope="module")
def H(built):
    return load_harness()


def _cases_hold_what_they_are_meant_to():
    kinds_v, kinds_r, flags = set(), set(), set()
    for key in R.case_list():
        c = R.get_case(key)
        flags.add(c["flag"])
        fixed = ~(c["zu"] > c["zl"])
        assert fixed[:, :c["ns"], 0].all() and fixed[:, 0, -1].all() and not fixed[:, c["ns"]:].any()
        for v in range(c["nv"]):
            k = c["M"] // 2
            kinds_v.add((bool(c["zl"][0, v, k] > -R.INF), bool(c["zu"][0, v, k] < R.INF)))
        for j in range(c["np"]):
            kinds_r.add((bool(c["cl"][j] > -R.INF), bool(c["cu"][j] < R.INF)))
        # strictly interior
        z = np.concatenate([c["X"], c["U"]], 1)
        fr = np.broadcast_to(~fixed, z.shape)
        assert (z > c["zl"])[fr].all() and (z < c["zu"])[fr].all()
    assert kinds_v == {(True, True), (True, False), (False, True), (False, False)}
    assert kinds_r == {(True, False), (False, True), (True, True)}
    assert flags == {"plain", "cscale", "rs", "soc", "rows3"}
    assert any(len(r) == 3 for r in R.get_case(next(k for k in R.case_list() if k[6] == "rows3"))["rows"])
    assert {k[3] for k in R.case_list()} == {5, 33, 257} and {k[4] for k in R.case_list()} == {1, 3}


@pytest.fixture(scope="module")
def figures():
    return {}


@pytest.mark.parametrize("key", R.case_list(), ids=R.case_id)
def test_host_functions_against_the_reference(H, figures, key):
    c = R.get_case(key)
    figures[key] = R.run_checks(c, HostBackend(H), log=print)


def test_the_generator_keeps_every_class_of_terms_visible(H, figures):
    _cases_hold_what_they_are_meant_to()
    rows = exempt = jumped = 0
    for key in R.case_list():
        fig = figures.get(key) or R.run_checks(R.get_case(key), HostBackend(H))
        for name, share in fig["shares"]:
            for cls, s in share.items():
                if cls != "cost":
                    assert s >= 1e-3, (R.case_id(key), name, cls, s)
        rows += fig["reset_rows"]; exempt += fig["reset_exempt"]; jumped += fig["jumped"]
    print(f"slack reset: {rows} rows, {jumped} jump, {exempt} decided within the bound")
    assert exempt <= 0.01 * rows and 0 < jumped < rows
