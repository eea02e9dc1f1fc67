"""The ladder restarts (emi_ipm_solve_restart_*, emi_ipm_restart_decide) as far as they need no device: the declarations and their
ctypes mirror, the host rule, and the bookkeeping (etol_amd/csrc/emi_restart_book.hpp over emi_refine_book.hpp: who is pending, which
attempt owns an instance's output, the per-attempt blocks of results / err / out, the drop rule).
tests/harness/restart_book_main.cpp walks the books through the calls of the driver with scripted statuses, estimates and levels,
built with -fsanitize=address,undefined (`make check-restart-book`), and prints every case.  No GPU needed.

What the program printed is held here to the rules of include/emi355x.h restated below, one attempt and one rung at a time: nothing
expected comes from the objects under test."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MET, NOT_MET, FELL_BACK, FAILED = range(4)
OK = (0, 1)                         # EMI_IPM_CONVERGED, EMI_IPM_ACCEPTABLE
NAN = math.nan


# ---- the declarations and their mirror -------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "emi355x.h")).read()


def declared_args(name):
    """the number of arguments of a function declared in the header"""
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    assert m, name
    return len(m.group(1).split(","))


def test_the_three_symbols_are_declared_and_bound():
    from etol_amd import _lib as L
    n = {f: declared_args(f) for f in ("emi_ipm_restart_decide", "emi_ipm_solve_restart_dev", "emi_ipm_solve_restart_host")}
    assert n == {"emi_ipm_restart_decide": 2, "emi_ipm_solve_restart_dev": 17, "emi_ipm_solve_restart_host": 17}
    for f, k in n.items():
        assert f in L.SYMBOLS and len(L.SYMBOLS[f][1]) == k and L.SYMBOLS[f][0] is C.c_int, f
    assert L.SYMBOLS["emi_ipm_solve_restart_dev"][1] == L.SYMBOLS["emi_ipm_solve_restart_host"][1]
    assert "EMI_RESTART_DROP_FAILED = 1" in header() and L.RESTART_DROP_FAILED == 1


def test_the_structures_have_the_headers_layout(tmp_path):
    """sizes and offsets as the C compiler lays the header's structures out on this ABI"""
    from etol_amd import _lib as L
    fields = {"emi_ipm_restart_t": ("nstarts", "starts", "patience", "retry_mask", "flags"),
              "emi_ipm_restart_result_t": ("attempt", "attempts", "level", "refine")}
    src = ["#include <stddef.h>", "#include <stdio.h>", '#include "emi355x.h"', "int main(void) {"]
    for t, fs in fields.items():
        src.append(f'  printf("{t} %zu\\n", sizeof({t}));')
        src += [f'  printf("{t}.{f} %zu\\n", offsetof({t}, {f}));' for f in fs]
    src += ["  return 0;", "}"]
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src) + "\n")
    subprocess.run([os.environ.get("CC", "gcc"), "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(c)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    mirror = {"emi_ipm_restart_t": L.IpmRestart, "emi_ipm_restart_result_t": L.IpmRestartResult}
    for t, fs in fields.items():
        assert int(got[t]) == C.sizeof(mirror[t]), t
        assert [n for n, _ in mirror[t]._fields_] == list(fs), t
        for f in fs:
            assert int(got[f"{t}.{f}"]) == getattr(mirror[t], f).offset, (t, f)


def decide(verdict, mask):
    """emi_ipm_restart_decide as include/emi355x.h states it"""
    return bool(((mask or 1 << FAILED) >> verdict) & 1)


def test_the_rule_over_its_truth_table(built):
    import etol_amd as E
    masks = (0, 1 << FAILED, 1 << FAILED | 1 << FELL_BACK, 15)
    want = {0: {FAILED}, 1 << FAILED: {FAILED}, 1 << FAILED | 1 << FELL_BACK: {FAILED, FELL_BACK}, 15: {MET, NOT_MET, FELL_BACK, FAILED}}
    for m in masks:
        for v in (MET, NOT_MET, FELL_BACK, FAILED):
            assert E.Evaluator.restart_decide(v, m) == (v in want[m]) == decide(v, m), (v, m)
    assert not E.Evaluator.restart_decide(-1, 15) and not E.Evaluator.restart_decide(4, 15)      # no verdict: nobody is sent on


# ---- the books ---------------------------------------------------------------------------------------------------------------------------
def expected(c):
    """what the driver has to see per attempt and rung and the caller afterwards"""
    B, nr, fc, tol, A, mask, drop = (c[k] for k in ("B", "nrungs", "first_check", "tol", "A", "retry_mask", "drop"))
    never = fc < 0
    at = lambda a, r, b: (a * nr + r) * B + b
    status, iters, err = [-1] * (A * nr * B), [0] * (A * nr * B), [NAN] * (A * nr * B)
    out = [[0, 0, -2, -1, FAILED, 0, NAN] for _ in range(B)]
    pending, attempts = list(range(B)), []
    for a in range(A):
        if not pending:
            break
        live, pos = list(pending), list(range(len(pending)))
        ref = {b: dict(rung=-1, verdict=FAILED, solved=0, err=NAN) for b in pending}
        rungs = []
        for r in range(nr):
            if not live:
                break
            last = r + 1 == nr
            g = dict(live=list(live), caller_map=None if len(live) == B else list(live), here_from=[], here_to=[], older_from=[], older_to=[])
            nxt, nxt_pos = [], []
            for i, b in enumerate(live):
                s = c["status"][a][b][r]
                status[at(a, r, b)], iters[at(a, r, b)], ref[b]["solved"] = s, 100 * a + 10 * r + b, r + 1
                ok = s in OK
                if not never and r >= fc:                           # a rung with a check: the table of emi_ipm_refine_decide
                    e = err[at(a, r, b)] = c["err"][a][b][r]
                    met = math.isfinite(e) and e <= tol
                    if ok and not met and not last:
                        climbs = True
                    else:
                        climbs = False
                        ref[b]["verdict"] = (MET if met else NOT_MET) if ok else (FELL_BACK if r > fc else FAILED)
                elif drop:                                          # the drop rule: a failed solve ends the climb
                    climbs = ok and not last
                else:                                               # the ladder's rule: everybody climbs to the last rung
                    climbs = not last
                if climbs:
                    nxt.append(b)
                    nxt_pos.append(i)
                elif ref[b]["verdict"] == FELL_BACK and not never and r >= fc:
                    g["older_from"].append(pos[i])
                    g["older_to"].append(b)
                    ref[b].update(rung=r - 1, err=err[at(a, r - 1, b)])
                else:
                    g["here_from"].append(i)
                    g["here_to"].append(b)
                    ref[b].update(rung=r, err=err[at(a, r, b)])
            # with no rung checked the verdict is the status on the rung the instance ended on
            for b in g["here_to"]:
                if never:
                    ref[b]["verdict"] = MET if c["status"][a][b][r] in OK else FAILED
            g["sent_here"] = [b for b in g["here_to"] if a == 0 or not decide(ref[b]["verdict"], mask)]
            g["sent_older"] = [b for b in g["older_to"] if a == 0 or not decide(ref[b]["verdict"], mask)]
            rungs.append(g)
            live, pos = nxt, nxt_pos
        attempts.append(dict(pending=list(pending), rungs=rungs))
        nxt = []
        for b in pending:
            again = decide(ref[b]["verdict"], mask)
            out[b][1] = a + 1
            if a == 0 or not again:
                out[b] = [a, a + 1, c["level"][a][b], ref[b]["rung"], ref[b]["verdict"], ref[b]["solved"], ref[b]["err"]]
            if again:
                nxt.append(b)
        pending = nxt
    return dict(attempts=attempts, res_status=status, res_iterations=iters, res_err=err, out=out)


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
    out = tmp_path_factory.mktemp("book") / "restart_book_check"
    r = subprocess.run(["make", "-C", ROOT, "check-restart-book", f"RESTART_CHECK_OUT={out}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "restart book: ok" in r.stdout
    assert "-fsanitize=address,undefined" in r.stdout                                          # an ordinary host executable under the host sanitizers
    return {c["case"]: c for c in (json.loads(line) for line in r.stdout.splitlines() if line.startswith("{"))}


NAMES = ("everybody solved in attempt 0", "everybody pending", "mixed over three attempts", "a fall-back that is retried",
         "the plain ladder with the drop", "the plain ladder without the drop", "without the drop below first_check", "every verdict retried",
         "one instance", "one instance, one rung, one attempt")


def test_the_program_walks_every_case(cases):
    assert tuple(cases) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_the_books_against_the_restated_rules(cases, name):
    c = cases[name]
    want = expected(c)
    assert same(c["attempts"], want["attempts"]), (name, c["attempts"], want["attempts"])
    for k in ("res_status", "res_iterations", "res_err", "out"):
        assert same(c[k], want[k]), (name, k, c[k], want[k])


def test_the_cases_are_the_ones_described(cases):
    first, nobody, mixed = cases["everybody solved in attempt 0"], cases["everybody pending"], cases["mixed over three attempts"]
    assert len(first["attempts"]) == 1 and [q[:2] for q in first["out"]] == [[0, 1]] * 3 and [q[2] for q in first["out"]] == [0, 1, 2]
    assert all(s == -1 for s in first["res_status"][9:])                       # the attempts that never ran
    assert [q[:2] + q[4:5] for q in nobody["out"]] == [[0, 2, FAILED]] * 3 and all(a["pending"] == [0, 1, 2] for a in nobody["attempts"])
    assert all(g["sent_here"] == [] for g in nobody["attempts"][1]["rungs"])    # what attempt 0 left stays
    # drops on rung 0 and on a later rung, a fall-back, an instance pending to the end
    assert [a["pending"] for a in mixed["attempts"]] == [[0, 1, 2, 3, 4, 5], [1, 3, 4], [3, 4]]
    assert mixed["attempts"][0]["rungs"][0]["here_to"] == [1, 4] and mixed["attempts"][1]["rungs"][1]["here_to"] == [1, 4]
    assert mixed["attempts"][0]["rungs"][2]["older_to"] == [2]
    assert [q[:6] for q in mixed["out"]] == [[0, 1, -2, 1, MET, 2], [1, 2, 1, 1, MET, 2], [0, 1, -2, 1, FELL_BACK, 3], [2, 3, -2, 2, MET, 3],
                                             [0, 3, -2, 0, FAILED, 1], [0, 1, -2, 2, NOT_MET, 3]]
    again = cases["a fall-back that is retried"]
    assert again["out"][0][:5] == [1, 2, 1, 2, MET] and again["attempts"][0]["rungs"][2]["sent_older"] == [0]
    one = cases["one instance"]
    assert one["B"] == 1 and one["out"] == [[2, 3, -1, 2, NOT_MET, 3, 5e-3]]
    plain = cases["the plain ladder with the drop"]
    assert [q[3:5] for q in plain["out"]] == [[2, MET], [2, MET], [1, FAILED], [2, FAILED]] and all(math.isnan(e) for e in plain["res_err"])


# ---- the fixture of the restart that matters ---------------------------------------------------------------------------------------------
def test_the_cpu_reference_alone_shows_the_split(built):
    """tests/golden/restart_cases.json: at least two instances end not solved from the line, with the constraints violated by more than
    1e-3 and not merely at the iteration limit, and solved from the planned route; at least one is solved from the line.  One thick
    wall is climbed again here from both starts."""
    import ladder_ref as LD
    import restart_ref as RS
    fx = RS.fixture()
    cases = fx["cases"]
    assert 2 <= len(cases) <= 6 and fx["starts"] == list(RS.STARTS) and fx["ladder"] == list(RS.LADDER) and fx["max_iter"] == RS.MAX_ITER
    assert [c["discs"] for c in cases] == [[list(d) for d in w] for _, w in RS.WALLS]
    restarted = [c for c in cases if c["attempt"] == 1]
    assert len(restarted) >= 2 and any(c["attempt"] == 0 for c in cases)
    for c in cases:
        line, planned = c["climbs"]["line"], c["climbs"]["planned"]
        assert c["attempt"] == (0 if line["solved"] else 1) and c["climbs"][RS.STARTS[c["attempt"]]]["solved"]
        assert c["cost"] == c["climbs"][RS.STARTS[c["attempt"]]]["rungs"][-1]["cost"]
        if c["attempt"] == 1:
            last = line["rungs"][-1]
            assert not last["ok"] and last["constr_viol"] > RS.NOT_SOLVED and planned["solved"] and planned["level"] >= 0, c["name"]
    c = restarted[0]
    h = LD.load_harness()
    for kind in RS.STARTS:
        rows, level = RS.cpu_climb(h, [tuple(d) for d in c["discs"]], kind)
        want = c["climbs"][kind]
        assert level == want["level"] and [r["ok"] for r in rows] == [r["ok"] for r in want["rungs"]], kind
        assert RS.solved(rows) == want["solved"]
        for r, w in zip(rows, want["rungs"]):
            if r["ok"]:
                assert abs(r["cost"] - w["cost"]) <= 1e-9 * abs(w["cost"]), (kind, r, w)
