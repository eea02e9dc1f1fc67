"""Generates tests/golden/restart_cases.json: the fixture of the restart that matters (tests/test_gpu_restart.py).

The instances of tests/restart_ref.py (walls of six discs across the straight line, B = 4) climbed over (21, 41) on the CPU from the
line and from the planned route, as tests/golden/gen_ladder_cases.py climbs: the project's own solve_nlp on the oracle with the reduced
rule set (harness_ladder_solve_oracle), the numpy barycentric prolongation of tests/ladder_ref.py and a clip into the bounds between
the rungs; the planned route is the numpy restatement of tests/plan_ref.py.  A rung that fails ends a climb.  Recorded per instance
and start: the route's level and per rung ok, iterations, cost, kkt_error, constr_viol; per instance the first start whose climb ends
solved (the attempt a restart run from those starts, in that order, returns) and the cost there.

The generator asserts what the tests rely on: at least two instances end NOT solved from the line with constr_viol above 1e-3 (not
merely at the iteration limit) and solved from the planned route, and at least one is solved from the line.  No GPU needed:

    python tests/golden/gen_restart_cases.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ladder_ref as LD  # noqa: E402
import restart_ref as RS  # noqa: E402


def main():
    import __graft_entry__ as g
    g.build(quiet=True)
    h = LD.load_harness()
    out = dict(ladder=list(RS.LADDER), tf=RS.TF, tol=RS.TOL, max_iter=RS.MAX_ITER, starts=list(RS.STARTS), box=RS.BOX, clearance=RS.CLEARANCE,
               rules="solve_nlp with max_shift_trials 0, crawl and stagnation rules off", cases=[])
    for name, discs in RS.WALLS:
        case = dict(name=name, discs=[list(d) for d in discs], climbs={})
        for kind in RS.STARTS:
            rows, level = RS.cpu_climb(h, discs, kind)
            case["climbs"][kind] = dict(level=level, rungs=rows, solved=RS.solved(rows))
            print(name, kind, level, [(r["ok"], r["iterations"], round(r["cost"], 6), f"{r['constr_viol']:.1e}") for r in rows], flush=True)
        won = [a for a, kind in enumerate(RS.STARTS) if case["climbs"][kind]["solved"]]
        assert won, name
        case["attempt"] = won[0]
        case["cost"] = case["climbs"][RS.STARTS[won[0]]]["rungs"][-1]["cost"]
        out["cases"].append(case)
    restarted = [c for c in out["cases"] if c["attempt"] == 1]
    assert len(restarted) >= 2 and any(c["attempt"] == 0 for c in out["cases"]) and len(out["cases"]) <= 6
    for c in restarted:
        last = c["climbs"]["line"]["rungs"][-1]
        assert not last["ok"] and last["constr_viol"] > RS.NOT_SOLVED, (c["name"], last)
    path = RS.FIXTURE
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
