"""Generates tests/golden/lockstep_rescue_cases.json: the fixture of the tests of the lock-step driver's residual-based acceptance
and crawl rule (EMI_IPM_RULE_RESIDUAL).

Per final time of tests/lockstep_ref.py: the blocked instance (NO_PATH_DISC on the fixed start state) and the nine regular
instances, solved with the project's own solve_nlp -- oracle evaluator, dense host factorisation, tol 1e-8, max_iter 200 -- under
the device's rule set: inertia search, stagnation rule and second-order correction off, crawl_limit 3, crawl_frac 0.3
(tests/harness/etol_harness_rescue.cpp).  Each is solved a second time without the crawl rule (crawl_limit beyond max_iter:
solve_nlp has no switch for the err0 <= 1e-2 branch of the residual-based acceptance, which is all that is left then).  Recorded:
status, iterations, evaluations, newton_steps, restored_steps, cost, rho.  No GPU needed:

    python tests/golden/gen_lockstep_rescue_cases.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lockstep_ref as LR  # noqa: E402
import lockstep_rescue_ref as RR  # noqa: E402


def both(h, tf, inst):
    on = RR.solve_oracle(h, tf, inst, RR.OPTIONS["crawl_limit"], RR.OPTIONS["crawl_frac"])
    off = RR.solve_oracle(h, tf, inst, RR.RULE_OFF_CRAWL_LIMIT, RR.OPTIONS["crawl_frac"])
    return dict(discs=[list(d) for d in inst["discs"]], bump=inst["bump"], rule_on=on, rule_off=off)


def show(tag, row):
    for k in ("rule_on", "rule_off"):
        r = row[k]
        print(f"{tag} {k}: {r['status']} iterations {r['iterations']} evaluations {r['evaluations']} newton {r['newton_steps']} "
              f"restored {r['restored_steps']} rho {r['rho']:g} cost {r['cost']:.6f}")


def main():
    import __graft_entry__ as g
    g.build(quiet=True)
    h = RR.load_harness()
    out = dict(M=LR.M_NODES, tol=1e-8, max_iter=RR.MAX_ITER, crawl_limit=RR.OPTIONS["crawl_limit"], crawl_frac=RR.OPTIONS["crawl_frac"],
               rules="solve_nlp with max_shift_trials 0, stagnation rule and second-order correction off", cases={})
    for tf in LR.TFS:
        blocked = both(h, tf, RR.blocked_instance(tf))
        show(f"tf {tf} blocked", blocked)
        regular = []
        for b, inst in enumerate(LR.instances(tf)):
            regular.append(both(h, tf, inst))
            show(f"tf {tf} instance {b}", regular[-1])
        out["cases"][str(tf)] = dict(blocked=blocked, regular=regular)
    json.dump(out, open(RR.FIXTURE, "w"), indent=1)
    print("wrote", RR.FIXTURE)


if __name__ == "__main__":
    main()
