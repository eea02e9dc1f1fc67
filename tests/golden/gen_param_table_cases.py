"""Generates tests/golden/param_table_cases.json: the fixture of the lock-step test of the per-instance parameter table
(emi_set_model_params_batch).

Instances 0, 4, 8 of tests/lockstep_ref.py at final time 4.0 -- their discs, their starts unchanged -- each with its own row of
quadrotor parameters (tests/param_table_ref.py), solved with the project's own solve_nlp through harness_rescue_solve_oracle, which
takes the parameter set: oracle evaluator, dense host factorisation, tol 1e-8, max_iter 200, the device's rule set (inertia
search, stagnation rule and second-order correction off), the crawl rule out of reach (crawl_limit beyond max_iter).  Recorded per
(instance, row) pair: status, iterations, evaluations, cost.  No GPU needed:

    python tests/golden/gen_param_table_cases.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lockstep_ref as LR  # noqa: E402
import lockstep_rescue_ref as RR  # noqa: E402
import param_table_ref as PT  # noqa: E402


def main():
    import __graft_entry__ as g
    g.build(quiet=True)
    h = RR.load_harness()
    out = dict(M=LR.M_NODES, tf=PT.TF, tol=PT.TOL, max_iter=PT.MAX_ITER, crawl_limit=RR.RULE_OFF_CRAWL_LIMIT, crawl_frac=RR.OPTIONS["crawl_frac"],
               rules="solve_nlp with max_shift_trials 0, stagnation rule and second-order correction off, crawl rule out of reach", cases=[])
    for c in PT.cases():
        r = PT.solve_oracle(h, c["inst"], c["params"])
        print(f"instance {c['instance']} row {c['row']} {c['params']}: {r['status']} iterations {r['iterations']} evaluations {r['evaluations']} "
              f"cost {r['cost']:.9f}")
        out["cases"].append(dict(instance=c["instance"], row=c["row"], params=c["params"], discs=[list(d) for d in c["inst"]["discs"]],
                                 bump=c["inst"]["bump"], **r))
    json.dump(out, open(PT.FIXTURE, "w"), indent=1)
    print("wrote", PT.FIXTURE)


if __name__ == "__main__":
    main()
