"""The per-instance parameter table (emi_set_model_params_batch) where no device is needed: the fixture of its lock-step test and
how it regenerates, the launch policy of a context that holds a table, and the two calls in the header, the library and the Python
mirror.  No GPU needed."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import lockstep_ref as LR
import lockstep_rescue_ref as RR
import param_table_ref as PT
from pinned_plans import PINNED_PLANS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("emi_set_model_params_batch", "emi_get_model_params_batch")
# measured on the CPU when the cases were chosen, for the pairs (instance, row) = (0, 0), (4, 1), (8, 2)
MEASURED = ((20, 256.198696907), (13, 398.824587005), (16, 1253.140470865))


def test_the_fixture_holds_the_three_pairs(built):
    fx = PT.fixture()
    assert fx["M"] == LR.M_NODES and fx["tf"] == PT.TF and fx["tol"] == PT.TOL and fx["max_iter"] == PT.MAX_ITER
    assert fx["crawl_limit"] == RR.RULE_OFF_CRAWL_LIMIT > fx["max_iter"]             # the crawl rule is out of reach
    assert [(c["instance"], c["row"]) for c in fx["cases"]] == list(zip(PT.INSTANCES, range(3)))
    insts = LR.instances(PT.TF)
    for c, (its, cost) in zip(fx["cases"], MEASURED):
        assert c["params"] == list(PT.ROWS[c["row"]])
        assert [tuple(d) for d in c["discs"]] == [tuple(d) for d in insts[c["instance"]]["discs"]] and c["bump"] == insts[c["instance"]]["bump"]
        assert c["status"] == "converged" and c["iterations"] == its, c
        assert abs(c["cost"] - cost) <= 5e-10 * cost, c                              # (quoted to nine decimals)
    assert len({c["cost"] for c in fx["cases"]}) == 3


def test_one_pair_regenerates_through_the_harness(built):
    """the pair whose row differs from the nominal set in every entry but gravity: solve_nlp on the CPU oracle with that row"""
    fx = PT.fixture()["cases"]
    h = RR.load_harness()
    for k in (2,):
        c = PT.cases()[k]
        got = PT.solve_oracle(h, c["inst"], c["params"])
        want = {q: fx[k][q] for q in ("status", "iterations", "evaluations", "cost")}
        assert got["status"] == want["status"] and got["iterations"] == want["iterations"] and got["evaluations"] == want["evaluations"], (got, want)
        assert abs(got["cost"] - want["cost"]) <= 1e-12 * abs(want["cost"]), (got, want)
    # ... and the row matters: the same instance under the nominal set is the fixture of tests/lockstep_ref.py, another optimum
    nominal = LR.fixture()["cases"][str(PT.TF)][PT.INSTANCES[2]]
    assert abs(nominal["cost"] - fx[2]["cost"]) > 1e-3 * abs(nominal["cost"])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan") / "param_table_plan_check"
    r = subprocess.run(["make", "-C", ROOT, "check-param-table-plan", f"PARAM_PLAN_CHECK_OUT={out}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "param table plan: ok" in r.stdout
    return str(out)


@pytest.mark.parametrize("B", sorted(PINNED_PLANS))
def test_a_table_takes_the_sequential_form_at_every_pinned_shape(program, B):
    """the contexts of tests/test_pass_plan_cpu.py (6 states, 1024 nodes, 20 keep-outs): without a table the pinned plan, with one
    nothing overlapped, no launch as one, no pieces"""
    r = subprocess.run([program, "plan", "6", "2", "1024", str(B), "20"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = json.loads(r.stdout)
    assert p["shared"]["overlapped"] == 1 and p["shared"]["one_launch"] == 1
    for k, v in PINNED_PLANS[B].items():
        assert p["shared"][k] == v, (B, k, p["shared"])
    assert all(v == 0 for v in p["table"].values()), p["table"]


def test_header_exports_and_mirror_agree_on_the_two_calls(built):
    import etol_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "emi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = {m.group(1): re.sub(r"\s+", " ", m.group(2)).strip() for m in re.finditer(r"\bint\s+(emi_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code)}
    assert proto["emi_set_model_params_batch"] == "emi_ctx_t ctx, const double* params, int nsets, int nparams"
    assert proto["emi_get_model_params_batch"] == "emi_ctx_t ctx, double* params, int* nsets, int* nparams"
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert L.SYMBOLS["emi_set_model_params_batch"] == (C.c_int, [C.c_void_p, D, C.c_int, C.c_int])
    assert L.SYMBOLS["emi_get_model_params_batch"] == (C.c_int, [C.c_void_p, D, I, I])
    lib = L.load()
    for name in CALLS:
        assert getattr(lib, name) is not None
        assert name in hdr[hdr.index("PER-INSTANCE MODEL PARAMETERS"):]             # the header comment stands in front of them
    # a null context is an argument error, not a crash (no device needed for that)
    assert lib.emi_set_model_params_batch(None, None, 0, 0) == 1
    assert lib.emi_get_model_params_batch(None, None, None, None) == 1
    # the evaluator carries both
    import etol_amd as E
    assert callable(E.Evaluator.set_model_params) and callable(E.Evaluator.get_model_params)
