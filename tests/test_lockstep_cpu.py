"""The lock-step interior-point driver's host-checkable parts.  No GPU needed.

(1) The scalar control rules of etol_amd/csrc/emi_ipm_control.hpp -- the text the control kernels run, here through
    tests/harness/etol_harness_lockstep.cpp -- against the Python restatement of tests/lockstep_ref.py, on seeded inputs and on
    the edge cases: decisions and counters equal, doubles equal (mu after an update within 4 ulp).
(2) kkt_error formed from the error COMPONENTS (lockstep_ref.error_parts_ref) against tests/ipm_ref.py's error reference, within
    that reference's own bound, at mu_t = 0, mu and mu / 5.
(3) The fixture tests/golden/lockstep_cases.json holds the cases of lockstep_ref, all converged."""
import math

import numpy as np
import pytest

import ipm_ref as R
import lockstep_ref as LR


@pytest.fixture(scope="module")
def rules(built):
    return LR.HostRules(LR.load_harness())


def same_state(a, b, what):
    for k in LR.SI:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in LR.SD:
        if k == "mu":
            assert abs(a[k] - b[k]) <= 4 * np.spacing(abs(b[k])), (what, k, a[k], b[k])
        else:
            assert a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])), (what, k, a[k], b[k])


def parts(**kw):
    p = dict(ed=1e-3, sd=1.0, ep=1e-3, sc=1.0, pmin=0.05, pmax=0.2, emax=0.5, ymax=1.0)
    p.update(kw)
    return p


def run_barrier(rules, p, s, o, what):
    a, b = dict(s), dict(s)
    rules.barrier(p, a, o)
    LR.barrier(p, b, o)
    same_state(a, b, what)
    return b


def test_barrier_rule_on_seeded_inputs(rules):
    rng = np.random.default_rng(20251)
    seen = set()
    fired = 0
    for n in range(4000):
        mu = 10.0 ** rng.uniform(-10, -0.5)
        s = LR.start(mu, float(rng.choice([10.0, 100.0, 1e5, 1e6, 1e11, 1e12])))
        s.update(nu=10.0 ** rng.uniform(0, 6), emax_ref=float(rng.choice([1e300, 1e-2, 1e-5])), futile=int(rng.integers(0, 3)),
                 n_acceptable=int(rng.integers(0, 10)), iterations=int(rng.integers(0, 201)))
        scale = 10.0 ** rng.uniform(-12, 0)
        p = parts(ed=scale * rng.uniform(), sd=1.0 + (rng.uniform() < 0.3) * rng.uniform(0, 50), ep=scale * rng.uniform(),
                  sc=1.0 + (rng.uniform() < 0.3) * rng.uniform(0, 50), pmin=mu * rng.uniform(0.2, 1.0) if rng.uniform() < 0.7 else scale * rng.uniform(),
                  pmax=mu * rng.uniform(1.0, 5.0) if rng.uniform() < 0.7 else scale * rng.uniform(),
                  emax=10.0 ** rng.uniform(-12, 0), ymax=10.0 ** rng.uniform(-3, 7))
        if p["pmin"] > p["pmax"]:
            p["pmin"], p["pmax"] = p["pmax"], p["pmin"]
        o = dict(LR.DEFAULTS, has_rows=int(rng.uniform() < 0.85))
        out = run_barrier(rules, p, s, o, n)
        seen.add(out["status"])
        fired += out["mu"] < mu
        assert rules.kkt(p, mu) == LR.kkt(p, mu) and rules.kkt(p, 0.0) == LR.kkt(p, 0.0)
    print("statuses seen", sorted(seen), "barrier updates", fired)
    assert {LR.RUNNING, LR.CONVERGED, LR.ACCEPTABLE, LR.MAX_ITER, LR.INFEASIBLE} <= seen and fired > 200


def test_barrier_rule_edge_cases(rules):
    o = dict(LR.DEFAULTS)
    solved = parts(ed=1e-12, ep=1e-12, pmin=0.0999, pmax=0.1001, emax=1e-12, ymax=0.1)
    # several barrier firings in one call: a point that solves every barrier problem down to the floor
    s = LR.start()
    tight = parts(ed=1e-13, ep=1e-13, pmin=1e-13, pmax=1e-13, emax=1e-12, ymax=0.1)
    out = run_barrier(rules, dict(tight, pmax=2e-8, pmin=1e-9), s, o, "several firings")
    steps, m = 0, 0.1
    while m > o["tol"] / 10 and LR.kkt(dict(tight, pmax=2e-8, pmin=1e-9), m) <= 10 * m:
        m, steps = max(o["tol"] / 10, min(0.2 * m, m * math.sqrt(m))), steps + 1
    assert steps >= 3 and out["mu"] == m and out["status"] == LR.RUNNING and out["tau"] == max(0.99, 1 - m)
    # mu at its floor: no update, and the loop ends
    s = LR.start(o["tol"] / 10.0)
    out = run_barrier(rules, dict(solved, pmin=1e-9, pmax=1e-9, ed=1e-7, ep=1e-7), s, o, "mu at its floor")
    assert out["mu"] == o["tol"] / 10.0 and out["status"] == LR.RUNNING
    # converged, and converged with a relaxed row: escalation (no barrier update in that round), rho >= 1e12: infeasible
    conv = parts(ed=1e-10, ep=1e-10, pmin=0.0, pmax=5e-9, emax=1e-9, ymax=0.1)
    assert run_barrier(rules, conv, LR.start(1e-9), o, "converged")["status"] == LR.CONVERGED
    relaxed = dict(conv, emax=1e-3)
    out = run_barrier(rules, relaxed, LR.start(1e-9), o, "relaxed")
    assert out["status"] == LR.RUNNING and out["rho"] == 100.0 and out["mu"] == 1e-2 and out["escalated"] == 1
    assert run_barrier(rules, relaxed, LR.start(1e-9, 1e12), o, "rho at its cap")["status"] == LR.INFEASIBLE
    assert run_barrier(rules, relaxed, LR.start(1e-9), dict(o, has_rows=0), "no rows")["status"] == LR.CONVERGED
    # the futile counter at its limit, one below it, and an escalation that helped
    s = LR.start(1e-9, 1e6)
    s.update(futile=2, emax_ref=1e-3)
    assert run_barrier(rules, relaxed, s, o, "futile at its limit")["status"] == LR.INFEASIBLE
    s.update(futile=1)
    out = run_barrier(rules, relaxed, s, o, "futile below its limit")
    assert out["status"] == LR.RUNNING and out["futile"] == 2 and out["rho"] == 1e7
    s.update(futile=2, emax_ref=1.0)
    out = run_barrier(rules, relaxed, s, o, "escalation that helped")
    assert out["status"] == LR.RUNNING and out["futile"] == 0 and out["emax_ref"] == 1e-3
    # escalation inside the barrier loop: a multiplier at the penalty weight when the barrier problem is solved
    s = LR.start()
    out = run_barrier(rules, dict(solved, ymax=9.5), s, o, "multiplier at the weight")
    assert out["rho"] == 100.0 and out["mu"] == 0.1 and out["nu"] == 1.0 and out["escalated"] == 1
    # the acceptable counter at its limit, and its reset
    acc = parts(ed=5e-7, ep=1e-9, pmin=0.0, pmax=1e-9, emax=1e-9, ymax=0.1)
    s = LR.start(1e-9)
    s.update(n_acceptable=9)
    assert run_barrier(rules, acc, s, o, "acceptable at its limit")["status"] == LR.ACCEPTABLE
    s.update(n_acceptable=8)
    assert run_barrier(rules, acc, s, o, "acceptable below its limit")["n_acceptable"] == 9
    assert run_barrier(rules, dict(acc, ed=1e-3), s, o, "not acceptable")["n_acceptable"] == 0
    # max_iter, not-finite components, an instance that has ended
    s = LR.start()
    s.update(iterations=200)
    assert run_barrier(rules, parts(), s, o, "max_iter")["status"] == LR.MAX_ITER
    assert run_barrier(rules, parts(ed=float("nan")), LR.start(), o, "nan")["status"] == LR.NOT_FINITE
    assert run_barrier(rules, parts(emax=float("inf")), LR.start(), o, "inf")["status"] == LR.NOT_FINITE
    s = LR.start()
    s.update(status=LR.CONVERGED, evaluations=7)
    assert run_barrier(rules, parts(), s, o, "ended") == dict(s, escalated=0)
    for dc, mu in ((0.0, 0.1), (0.0, 1e-9), (1e-8, 0.1), (3e-6, 1e-3)):
        assert rules.raise_dc(dc, mu) == LR.raise_dc(dc, mu)


def run_search(rules, scal, mer0, trials, s, o, exact, failed=0):
    a, b = dict(s), dict(s)
    rules.search_init(scal, mer0, failed, a)
    LR.search_init(scal, mer0, failed, b)
    same_state(a, b, "init")
    for n, m in enumerate(trials):
        rules.search_step(m, exact, a, o)
        LR.search_step(m, exact, b, o)
        same_state(a, b, ("step", n))
    return b


def test_search_rules(rules):
    o = dict(LR.DEFAULTS)
    rng = np.random.default_rng(20252)
    outcomes = set()
    for n in range(1500):
        s = LR.start(10.0 ** rng.uniform(-9, -1))
        s.update(nu=10.0 ** rng.uniform(0, 5), err0=10.0 ** rng.uniform(-8, 0), emax=10.0 ** rng.uniform(-9, -3),
                 force_modified=int(rng.uniform() < 0.2), iterations=int(rng.integers(0, 50)))
        infeas0 = 0.0 if rng.uniform() < 0.15 else 10.0 ** rng.uniform(-10, 2)
        scal = [rng.uniform(1e-3, 1.0), rng.uniform(1e-3, 1.0), rng.normal() * 10.0 ** rng.uniform(-3, 3), 10.0 ** rng.uniform(-2, 9)]
        phi_b = rng.normal() * 100.0
        never = rng.uniform() < 0.1
        trials = []
        for t in range(41):
            r = rng.uniform()
            phi_t = float("nan") if r < 0.05 else float("inf") if r < 0.1 else phi_b + (1.0 if never else rng.normal()) * 10.0 ** rng.uniform(-6, 1)
            trials.append([phi_t, 1e3 if never else infeas0 * rng.uniform(0.0, 2.0)])
        out = run_search(rules, scal, [phi_b, infeas0], trials, s, o, exact=int(rng.uniform() < 0.5))
        outcomes.add((out["accepted"], out["force_modified"], out["status"]))
        assert not out["searching"] and out["passes"] <= 40
    print(sorted(outcomes))
    assert {(1, 0, LR.RUNNING), (0, 1, LR.RUNNING), (0, 0, LR.LINE_SEARCH)} <= outcomes
    # edge cases (err0 = 1: far from the acceptable level)
    s = LR.start()
    s.update(err0=1.0)
    out = run_search(rules, [0.5, 0.7, -1.0, 2.0], [10.0, 0.0], [[9.0, 0.0]], s, o, 0)          # infeas0 = 0: the multipliers' weight alone
    assert out["nu"] == 2.2 and out["accepted"] == 1 and out["alpha"] == 0.5 and out["adu"] == 0.7 and out["iterations"] == 1
    out = run_search(rules, [1.0, 1.0, -1.0, 0.5], [10.0, 1.0], [[float("nan"), 0.0], [float("inf"), 0.0], [9.0, 0.0]], s, o, 0)
    assert out["accepted"] == 1 and out["passes"] == 2 and out["alpha"] == 0.25 and out["evaluations"] == 3        # a non-finite phi rejects
    out = run_search(rules, [1.0, 1.0, -1.0, 0.5], [10.0, 1.0], [[20.0, 0.0]] * 45, s, o, 1)
    assert out["passes"] == 40 and out["force_modified"] == 1 and out["status"] == LR.RUNNING and out["evaluations"] == 40
    out = run_search(rules, [1.0, 1.0, -1.0, 0.5], [10.0, 1.0], [[20.0, 0.0]] * 40, dict(out), o, 1)
    assert out["force_modified"] == 0 and out["status"] == LR.LINE_SEARCH
    s2 = LR.start()
    s2.update(err0=5e-7, emax=1e-9)
    assert run_search(rules, [1.0, 1.0, -1.0, 0.5], [10.0, 1.0], [[20.0, 0.0]] * 40, s2, o, 0)["status"] == LR.ACCEPTABLE
    assert run_search(rules, [1.0, 1.0, -1.0, 0.5], [10.0, 1.0], [], LR.start(), o, 0, failed=1)["status"] == LR.FACTOR
    nu_old = LR.start()
    nu_old.update(nu=1e6)
    assert run_search(rules, [1.0, 1.0, -1.0, 0.5], [10.0, 1.0], [], nu_old, o, 0)["nu"] == 5e5      # at most halving per iteration


@pytest.mark.parametrize("key", [k for k in R.case_list() if k[3] in (5, 33)], ids=R.case_id)
def test_kkt_error_from_its_components(key):
    c = R.get_case(key)
    got = LR.error_parts_ref(c)
    for frac in (0.0, 1.0, 0.2):
        par = c["par"].copy()
        par[:, 0] = frac * c["par"][:, 0]
        ref = R.error_ref(dict(c, par=par))
        for b in range(c["B"]):
            value, tol = ref[b]["kkt"]
            mine = LR.kkt(got[b][0], par[b, 0])
            print(f"instance {b} mu_t {par[b, 0]:.3e}: {mine:.16e} against {value:.16e} (bound {tol:.1e})")
            assert abs(mine - value) <= tol
            assert abs(got[b][0]["ep"] - ref[b]["viol"][0]) <= ref[b]["viol"][1] and got[b][0]["emax"] == ref[b]["emax"][0]


def test_the_fixture_holds_the_cases_and_all_converged():
    fx = LR.fixture()
    assert fx["M"] == LR.M_NODES and fx["tol"] == 1e-8 and fx["cscale"] == LR.CSCALE.tolist()
    assert sorted(fx["cases"]) == sorted(str(tf) for tf in LR.TFS)
    for tf in LR.TFS:
        rows = fx["cases"][str(tf)]
        want = [(first, bump) for bump in LR.BUMPS for first in LR.FIRST_DISCS]
        assert [(tuple(r["discs"][0]), r["bump"]) for r in rows] == want
        for r in rows:
            assert tuple(r["discs"][1]) == LR.discs_of(tuple(r["discs"][0]))[1]
            assert r["ok"] and r["kkt_error"] <= 1e-8 and 5 <= r["iterations"] <= 60 and r["cost"] > 0 and r["rho"] >= 10.0
