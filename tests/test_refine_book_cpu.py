"""The bookkeeping of the lock-step ladder and refinement (etol_amd/csrc/emi_refine_book.hpp: who is live, where each live instance sat
in the batch before, which retirees return which rung's iterate, and the caller's results / err / out) has no device in it:
tests/harness/refine_book_main.cpp walks it through the calls of the driver with scripted statuses and estimates, built with
-fsanitize=address,undefined (`make check-refine-book`), and prints every case.  No GPU needed.

What the program printed is held here to tests/refine_ref.py's walk of every instance by itself, with the rule of include/emi355x.h
restated below (not the library's function, which the book calls): nothing expected comes from the object under test."""
import json
import math
import os
import subprocess

import pytest

import lockstep_ref as LR
import refine_ref as RR

OK = (LR.CONVERGED, LR.ACCEPTABLE)


def rule(status, err, tol, has_good, is_last):
    """(retires, verdict): the table of emi_ipm_refine_decide in include/emi355x.h"""
    ok, met = status in OK, math.isfinite(err) and err <= tol
    if ok:
        return (met or is_last), (RR.MET if met else RR.NOT_MET)
    return True, (RR.FELL_BACK if has_good else RR.FAILED)


def expected(c):
    """what the driver has to see per rung and the caller afterwards, from one RR.walk per instance"""
    B, nr, fc, never = c["B"], c["nrungs"], c["first_check"], c["first_check"] < 0
    per = []
    for b in range(B):
        if never:                   # no rung decides anything: solved everywhere, returned from the last rung, no verdict, no estimate
            per.append((nr - 1, RR.FAILED, nr))
        else:
            # (walk takes the status as a flag and hands the rule CONVERGED or MAX_ITER)
            per.append(RR.walk([s in OK for s in c["status"][b]], c["err"][b], c["tol"], fc, rule)[:3])
    lives = [[b for b in range(B) if per[b][2] > r] for r in range(nr)]
    rungs = []
    for r in range(nr):
        live = lives[r]
        if not live:
            break
        before = lives[r - 1] if r else list(range(B))
        pos = [before.index(b) for b in live]
        gone = [b for b in live if per[b][2] == r + 1]
        here = [b for b in gone if per[b][1] != RR.FELL_BACK]
        older = [b for b in gone if per[b][1] == RR.FELL_BACK]
        rungs.append(dict(live=live, pos=pos, row_map=None if live == before else pos, caller_map=None if len(live) == B else live,
                          here_from=[live.index(b) for b in here], here_to=here, older_from=[before.index(b) for b in older], older_to=older))
    status = [c["status"][b][r] if r < per[b][2] else -1 for r in range(nr) for b in range(B)]
    iters = [10 * r + b if r < per[b][2] else 0 for r in range(nr) for b in range(B)]
    err = [c["err"][b][r] if not never and fc <= r < per[b][2] else math.nan for r in range(nr) for b in range(B)]
    out = [[per[b][0], per[b][1], per[b][2], err[per[b][0] * B + b]] for b in range(B)]
    return dict(rungs=rungs, res_status=status, res_iterations=iters, res_err=err, out=out)


def same(a, b):
    """equal, a NaN equal to a NaN"""
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (math.isnan(a) and math.isnan(b))
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return a == b


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path_factory.mktemp("book") / "refine_book_check"
    r = subprocess.run(["make", "-C", root, "check-refine-book", f"BOOK_CHECK_OUT={out}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "refine book: ok" in r.stdout
    return {c["case"]: c for c in (json.loads(line) for line in r.stdout.splitlines() if line.startswith("{"))}


NAMES = ("base", "all retire on rung 1", "first_check 0", "a NaN estimate", "never", "one instance", "one instance, one rung, never")


def test_the_program_walks_every_case(cases):
    assert tuple(cases) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_the_book_against_the_restated_walk(cases, name):
    c = cases[name]
    want = expected(c)
    for r, (got, exp) in enumerate(zip(c["rungs"], want["rungs"])):
        for k in exp:
            assert got[k] == exp[k], (name, r, k, got[k], exp[k])
    assert len(c["rungs"]) == len(want["rungs"]), name
    for k in ("res_status", "res_iterations", "res_err", "out"):
        assert same(c[k], want[k]), (name, k, c[k], want[k])


def test_the_base_case_is_the_one_described(cases):
    """B = 5, four rungs, checked from rung 1: 0 meets on rung 1, 1 fails there with nothing good, 2 fails on rung 2 and falls back to
    rung 1 (from its place in the older batch), 3 climbs to the last rung and misses, 4 meets on rung 3"""
    c = cases["base"]
    assert (c["B"], c["nrungs"], c["first_check"]) == (5, 4, 1)
    assert [q[:3] for q in c["out"]] == [[1, RR.MET, 2], [1, RR.FAILED, 2], [1, RR.FELL_BACK, 3], [3, RR.NOT_MET, 4], [3, RR.MET, 4]]
    r = c["rungs"]
    assert [g["live"] for g in r] == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [2, 3, 4], [3, 4]]
    assert [g["row_map"] for g in r] == [None, None, [2, 3, 4], [1, 2]]
    assert (r[2]["older_from"], r[2]["older_to"]) == ([2], [2]) and (r[3]["here_from"], r[3]["here_to"]) == ([0, 1], [3, 4])
    # the fill of the rungs an instance never reached
    assert c["res_status"][2 * 5 + 0] == -1 and c["res_status"][3 * 5 + 2] == -1 and math.isnan(c["res_err"][2 * 5 + 1])
    assert all(math.isnan(e) for e in c["res_err"][:5])


def test_the_other_cases_are_the_ones_described(cases):
    early, never, one = cases["all retire on rung 1"], cases["never"], cases["one instance"]
    assert len(early["rungs"]) == 2 and all(s == -1 for s in early["res_status"][2 * 3:])          # the loop ends early
    assert cases["first_check 0"]["rungs"][0]["here_to"] == [0, 1]
    nan = cases["a NaN estimate"]
    assert [q[1] for q in nan["out"]] == [RR.MET, RR.MET, RR.FELL_BACK] and nan["out"][0][0] == 2 and math.isinf(nan["out"][2][3])
    ident = list(range(never["B"]))
    assert all(g["row_map"] is None and g["caller_map"] is None and g["live"] == ident for g in never["rungs"])
    assert [g["here_to"] for g in never["rungs"]] == [[], [], ident] and never["rungs"][-1]["here_from"] == ident
    assert all(not g["older_to"] for g in never["rungs"]) and -1 not in never["res_status"]
    assert one["B"] == 1 and one["out"] == [[2, RR.MET, 3, one["err"][0][2]]]
