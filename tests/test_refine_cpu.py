"""The host side of the lock-step mesh refinement (emi_ipm_solve_refine_*): the rule emi_ipm_refine_decide over its whole truth table,
the ctypes mirrors of the new structs against the header, and the fixture tests/golden/refine_cases.json re-checked from the JSON
(the band around the tolerances, the recorded split, the rule's answers).  No GPU needed."""
import ctypes as C
import itertools
import os
import re

import numpy as np

import lockstep_ref as LR
import refine_ref as RR

STATUSES = (LR.CONVERGED, LR.ACCEPTABLE, LR.MAX_ITER, 3, 4, 5, 6, -1)          # every EMI_IPM_* and "not solved"
ERRS = dict(met=4e-4, equal=5e-4, missed=6e-4, nan=float("nan"), inf=float("inf"), minus_inf=float("-inf"))
TOL = 5e-4


def test_the_rule_over_its_truth_table(built):
    import etol_amd as E
    from etol_amd import _lib as L
    assert (L.REFINE_MET, L.REFINE_NOT_MET, L.REFINE_FELL_BACK, L.REFINE_FAILED) == (RR.MET, RR.NOT_MET, RR.FELL_BACK, RR.FAILED) == (0, 1, 2, 3)
    n = 0
    for status, (name, err), has_good, is_last in itertools.product(STATUSES, ERRS.items(), (0, 1), (0, 1)):
        ok = status in (LR.CONVERGED, LR.ACCEPTABLE)
        met = name in ("met", "equal")                                  # a NaN or an infinite err of either sign: missed
        retires, verdict = E.Evaluator.refine_decide(status, err, TOL, has_good, is_last)
        what = (status, name, has_good, is_last)
        if ok and met:
            assert (retires, verdict) == (True, RR.MET), what
        elif ok:
            assert (retires, verdict) == (bool(is_last), RR.NOT_MET), what
        else:
            assert (retires, verdict) == (True, RR.FELL_BACK if has_good else RR.FAILED), what
        n += 1
    assert n == len(STATUSES) * len(ERRS) * 4
    # the ends of the tolerance's range: 0 retires nobody whose err is positive, +inf everybody who solved
    assert E.Evaluator.refine_decide(0, 1e-300, 0.0, 0, 0) == (False, RR.NOT_MET) and E.Evaluator.refine_decide(0, 0.0, 0.0, 0, 0) == (True, RR.MET)
    assert E.Evaluator.refine_decide(0, 1e300, float("inf"), 0, 0) == (True, RR.MET)
    assert E.Evaluator.refine_decide(0, float("nan"), float("inf"), 0, 0) == (False, RR.NOT_MET)
    assert E.Evaluator.refine_decide(2, 0.0, float("inf"), 0, 0) == (True, RR.FAILED)
    # a NULL verdict is allowed
    assert E.load().emi_ipm_refine_decide(0, 1.0, 0.5, 0, 0, None) == 0 and E.load().emi_ipm_refine_decide(0, 0.1, 0.5, 0, 0, None) == 1


def _header_struct(name):
    """[(type, field)] of `typedef struct name { .. } name_t;` in include/emi355x.h"""
    hdr = open(os.path.join(LR.ROOT, "include", "emi355x.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + r"_t;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = re.match(r"(const double|double|int)\s+(.*)", decl, flags=re.S).groups()
        for f in names.split(","):
            out.append((ctype + "*" if f.strip().startswith("*") else ctype, f.strip().lstrip("*")))
    return out


def test_the_ctypes_mirrors_follow_the_header(built):
    from etol_amd import _lib as L
    kinds = {"double": C.c_double, "int": C.c_int, "const double*": L._D}
    for name, cls in (("emi_ipm_refine", L.IpmRefine), ("emi_ipm_refine_result", L.IpmRefineResult)):
        want = _header_struct(name)
        assert [(f, t) for f, t in cls._fields_] == [(f, kinds[k]) for k, f in want], (name, want)
    # sizes and offsets of the C layout: double, int, (pad), two pointers; three ints, (pad), double
    assert C.sizeof(L.IpmRefine) == 32 and [getattr(L.IpmRefine, f).offset for f, _ in L.IpmRefine._fields_] == [0, 8, 16, 24]
    assert C.sizeof(L.IpmRefineResult) == 24 and [getattr(L.IpmRefineResult, f).offset for f, _ in L.IpmRefineResult._fields_] == [0, 4, 8, 16]
    for sym in ("emi_ipm_refine_decide", "emi_prolong_rows_dev", "emi_shard_move_dev", "emi_ipm_solve_refine_dev", "emi_ipm_solve_refine_host"):
        assert sym in L.SYMBOLS and getattr(L.load(), sym) is not None
    assert len(L.SYMBOLS["emi_ipm_solve_refine_dev"][1]) == len(L.SYMBOLS["emi_ipm_solve_refine_host"][1]) == 16


def test_the_fixture_keeps_its_band_and_its_split(built):
    fx = RR.fixture()
    assert fx["ladder"] == list(RR.LADDER) and fx["first_check"] == RR.FIRST_CHECK == 1 and fx["band"] == RR.BAND == 1.2
    assert {float(k): v for k, v in fx["tolerances"].items()} == RR.TOLS == {4.0: 5.5e-4, 2.5: 6.6e-4}
    assert RR.band_violations(fx) == []
    for tf in LR.TFS:
        rows, tol = fx["cases"][str(tf)], RR.TOLS[tf]
        assert len(rows) == 9
        split = {}
        for b, row in enumerate(rows):
            assert [g["M"] for g in row["rungs"]] == list(RR.LADDER) and all(g["ok"] for g in row["rungs"]), (tf, b)
            errs = [g["err"] for g in row["rungs"]]
            assert all(np.isfinite(e) and e > 0 for e in errs)
            rung, verdict, solved, taken = RR.walk([g["ok"] for g in row["rungs"]], errs, tol)
            assert (rung, verdict, solved) == (row["rung"], row["verdict"], row["rungs_solved"]), (tf, b)
            # the rule in words: the first checked rung whose err meets the tolerance, else the last
            first = next((r for r in range(RR.FIRST_CHECK, len(errs)) if errs[r] <= tol), None)
            assert (rung, verdict) == ((first, RR.MET) if first is not None else (len(errs) - 1, RR.NOT_MET)), (tf, b)
            assert all(e < tol / RR.BAND or e > tol * RR.BAND for _, e, _ in taken), (tf, b)
            split[rung] = split.get(rung, 0) + 1
        print(f"tf {tf}: tolerance {tol:g}, instances retiring per rung {split}")
        assert split == RR.SPLIT[tf] == {int(k): v for k, v in fx["split"][str(tf)].items()}
    assert RR.SPLIT == {4.0: {1: 6, 3: 3}, 2.5: {1: 5, 3: 4}}
