"""Residual-based acceptance and the crawl rule of the lock-step driver (EMI_IPM_RULE_RESIDUAL): the host-checkable parts.  No GPU.

(1) The three rule functions of etol_amd/csrc/emi_ipm_control.hpp (select, decide, crawl update) -- the text
    emi_ipm_rescue_kernel runs, here through tests/harness/etol_harness_rescue.cpp -- against the Python restatement of
    tests/lockstep_rescue_ref.py: every field of both records equal, bit for bit, on seeded inputs and on the edges.
(2) The ctypes mirrors carry the new fields, where include/emi355x.h puts them.
(3) The fixture tests/golden/lockstep_rescue_cases.json: the blocked instance of both final times ends locally infeasible before
    the iteration limit with the rule and runs to the limit without; the regular instances are left alone; one blocked case is
    solved again here and must reproduce its row."""
import ctypes as C
import math

import numpy as np
import pytest

import lockstep_ref as LR
import lockstep_rescue_ref as RR


@pytest.fixture(scope="module")
def host(built):
    return RR.HostRescue(RR.load_harness())


def parts(**kw):
    p = dict(ed=1e-3, sd=1.0, ep=1e-3, sc=1.0, pmin=0.05, pmax=0.2, emax=0.5, ymax=1.0)
    p.update(kw)
    return p


def only_ed(x, mu):
    """components whose KKT error at mu is exactly x (>= 0): ed / 1, nothing else"""
    return parts(ed=x, sd=1.0, ep=0.0, sc=1.0, pmin=mu, pmax=mu)


def searching_state(mu=0.01, err0=1.0, passes=1, **kw):
    s = LR.start(mu)
    s.update(searching=1, passes=passes, err0=err0, alpha=0.25, iterations=7, evaluations=20)
    s.update(kw)
    return s


def same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        assert x == y or (isinstance(x, float) and math.isnan(x) and math.isnan(y)), (what, k, x, y)


def both(host, fn, args, s, r, *rest):
    """one rule function through the header and through the restatement, from the same records; returns the restatement's"""
    s1, r1, s2, r2 = dict(s), dict(r), dict(s), dict(r)
    out1 = getattr(host, fn)(*args, s1, r1, *rest)
    out2 = getattr(RR, fn)(*args, s2, r2, *rest)
    assert bool(out1) == bool(out2), (fn, out1, out2)
    same(s1, s2, fn)
    same(r1, r2, fn)
    return out2, s2, r2


def test_rules_on_seeded_inputs(host):
    rng = np.random.default_rng(20261)
    taken = back = cands = 0
    for n in range(3000):
        mu = 10.0 ** rng.uniform(-9, -1)
        s = searching_state(mu, err0=10.0 ** rng.uniform(-4, 1), passes=int(rng.choice([0, 1, 1, 1, 2])), searching=int(rng.uniform() < 0.9),
                            status=int(rng.choice([LR.RUNNING] * 8 + [LR.CONVERGED, LR.MAX_ITER])), force_modified=int(rng.uniform() < 0.3),
                            accepted=int(rng.uniform() < 0.3), alpha=10.0 ** rng.uniform(-6, 0))
        r = RR.rescue_start()
        r.update(crawl=int(rng.integers(0, 6)), newton_steps=int(rng.integers(0, 5)), restored_steps=int(rng.integers(0, 5)), err_mu=rng.uniform())
        o = dict(RR.OPTIONS, rules=int(rng.uniform() < 0.9), crawl_limit=int(rng.choice([1, 3, 1000000])), crawl_frac=float(rng.choice([0.3, 0.5])))
        scale = 10.0 ** rng.uniform(-8, 0)
        now = parts(ed=scale * rng.uniform(), sd=1.0 + rng.uniform(0, 3), ep=scale * rng.uniform(), sc=1.0 + rng.uniform(0, 3),
                    pmin=mu * rng.uniform(0.2, 1.0), pmax=mu * rng.uniform(1.0, 5.0))
        c, s, r = both(host, "select", (now,), s, r, o)
        cands += c
        assert c == RR.applies(s, r, o) and (not c or r["err_mu"] == LR.kkt(now, s["mu"]))
        f = rng.choice([0.3, 0.85, 0.95, 3.0])
        tr = {k: (v * f if k in ("ed", "ep") else v) for k, v in now.items()}
        if rng.uniform() < 0.05:
            tr[str(rng.choice(LR.PARTS))] = float(rng.choice([np.nan, np.inf, -np.inf]))
        stands, s, r = both(host, "decide", (tr,), s, r)
        taken, back = taken + stands, back + (c and not stands)
        assert r["candidate"] == 0 and (c or not stands)
        both(host, "crawl", ([rng.uniform(0.1, 1.0), 1.0, 0.0, 0.0],), s, r, o)
    print(f"candidates {cands}, steps kept {taken}, taken back {back}")
    assert taken > 100 and back > 100 and cands - taken - back == 0


def test_decide_at_the_threshold_and_with_errors_that_are_not_finite(host):
    mu, err_mu = 0.01, 0.3
    o = dict(RR.OPTIONS)
    bound = 0.9 * err_mu
    for what, x, want in (("equal", bound, True), ("one ulp above", np.nextafter(bound, 1.0), False), ("one ulp below", np.nextafter(bound, 0.0), True),
                          ("nan", math.nan, False), ("+inf", math.inf, False)):
        s, r = searching_state(mu, err0=1e-3, force_modified=1), RR.rescue_start()
        r.update(crawl=2)
        c, s, r = both(host, "select", (only_ed(err_mu, mu),), s, r, o)
        assert c == 1 and r["err_mu"] == err_mu
        stands, s2, r2 = both(host, "decide", (only_ed(float(x), mu),), s, r)
        assert stands == want, what
        assert s2["evaluations"] == s["evaluations"] + 1        # either way the attempt is one evaluation
        if want:
            assert (s2["searching"], s2["accepted"], s2["force_modified"], s2["iterations"]) == (0, 0, 0, s["iterations"] + 1)
            assert (r2["crawl"], r2["newton_steps"], r2["restored_steps"]) == (0, 1, 0)
        else:
            assert (s2["searching"], s2["accepted"], s2["force_modified"], s2["iterations"], s2["alpha"]) == (1, 0, 1, s["iterations"], s["alpha"])
            assert (r2["crawl"], r2["newton_steps"], r2["restored_steps"]) == (2, 0, 1)
    # an error of -inf cannot come out of a maximum with 0; a component that is -inf, or a NaN the maximum drops, takes the step back
    for k, v in (("pmin", -math.inf), ("ed", math.nan), ("emax", math.nan), ("ymax", math.inf)):
        s, r = searching_state(mu, err0=1e-3), RR.rescue_start()
        _, s, r = both(host, "select", (only_ed(err_mu, mu),), s, r, o)
        tr = only_ed(0.0, mu)
        tr[k] = v
        stands, _, r2 = both(host, "decide", (tr,), s, r)
        assert not stands and r2["restored_steps"] == 1, k


def test_who_is_selected(host):
    mu = 0.01
    o = dict(RR.OPTIONS)
    now = only_ed(0.5, mu)
    sel = lambda s, r, oo=o: both(host, "select", (now,), s, r, oo)[0]
    r3 = dict(RR.rescue_start(), crawl=3)
    assert sel(searching_state(mu, err0=1e-2), RR.rescue_start()) == 1                         # err0 at 1e-2: near a solution
    assert sel(searching_state(mu, err0=float(np.nextafter(1e-2, 1.0))), RR.rescue_start()) == 0
    assert sel(searching_state(mu, err0=1.0), dict(RR.rescue_start(), crawl=2)) == 0           # one short of the crawl limit
    assert sel(searching_state(mu, err0=1.0), r3) == 1
    assert sel(searching_state(mu, err0=1.0), r3, dict(o, crawl_limit=1000000)) == 0           # only the err0 branch is left
    assert sel(searching_state(mu, err0=1e-3), r3, dict(o, crawl_limit=1000000)) == 1
    assert sel(searching_state(mu, err0=1e-3, searching=0), r3) == 0                           # accepted its first trial
    assert sel(searching_state(mu, err0=1e-3, passes=0), r3) == 0
    assert sel(searching_state(mu, err0=1e-3, passes=2), r3) == 0
    assert sel(searching_state(mu, err0=1e-3, status=LR.MAX_ITER), r3) == 0                    # has ended
    assert sel(searching_state(mu, err0=1e-3), r3, dict(o, rules=0)) == 0                      # the rule off
    # ... and then decide and the crawl update leave both records as they are
    s, r = searching_state(mu, err0=1e-3, accepted=1, alpha=1e-3), dict(r3, candidate=0)
    stands, s2, r2 = both(host, "decide", (only_ed(0.0, mu),), s, r)
    assert not stands and s2 == s and r2 == r
    _, s2, r2 = both(host, "crawl", ([1.0, 1.0, 0.0, 0.0],), s, r, dict(o, rules=0))
    assert s2 == s and r2 == r


def test_the_crawl_counter_across_rounds(host):
    """accepted short and long steps, a full step kept, one taken back, a round that ends in force_modified"""
    mu, o = 0.01, dict(RR.OPTIONS)
    r = RR.rescue_start()
    apr = 0.8
    scal = [apr, 1.0, 0.0, 0.0]
    seen = []
    rounds = (("accept", 0.3 * apr), ("accept", float(np.nextafter(0.3 * apr, 0.0))), ("accept", 0.1), ("accept", 0.01), ("restore", None),
              ("force_modified", None), ("accept", 0.2), ("take", None), ("accept", 0.05), ("accept", apr))
    for kind, alpha in rounds:
        s = searching_state(mu, err0=1.0)                    # far from a solution: only the crawl counter can select
        c, s, r = both(host, "select", (only_ed(0.5, mu),), s, r, o)
        if kind in ("restore", "take"):
            assert c == 1, (kind, r)
            stands, s, r = both(host, "decide", (only_ed(0.1 if kind == "take" else 0.49, mu),), s, r)
            assert stands == (kind == "take")
        if kind == "accept" or kind == "restore":            # the backtracking goes on and accepts a short step
            s.update(searching=0, accepted=1, alpha=alpha if alpha is not None else 0.01)
        elif kind == "force_modified":
            s.update(searching=0, accepted=0, force_modified=1)
        _, s, r = both(host, "crawl", (scal,), s, r, o)
        seen.append(r["crawl"])
    #             0.3 apr: not short | short | short | short | restored, then short | unchanged | short | kept: 0 | short | long
    assert seen == [0, 1, 2, 3, 4, 4, 5, 0, 1, 0], seen
    assert (r["newton_steps"], r["restored_steps"]) == (1, 1)


def test_the_mirrors_carry_the_new_fields(built):
    import re
    import os
    from etol_amd import _lib as L
    hdr = open(os.path.join(LR.ROOT, "include", "emi355x.h")).read()
    for name, cls in (("emi_ipm_options", L.IpmOptions), ("emi_ipm_result", L.IpmResult)):
        body = re.search(r"typedef struct %s \{(.*?)\}" % name, hdr, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S).strip()
            if decl:
                typ, names = decl.split(None, 1)
                fields += [(n.strip(), C.c_double if typ == "double" else C.c_int) for n in names.split(",")]
        assert fields == list(cls._fields_), name
    assert [n for n, _ in L.IpmOptions._fields_][-3:] == ["rules", "crawl_limit", "crawl_frac"]
    assert [n for n, _ in L.IpmResult._fields_][-2:] == ["newton_steps", "restored_steps"]
    assert dict(L.IpmRung._fields_)["opt"] is L.IpmOptions and L.IPM_RULE_RESIDUAL == 1


def test_the_fixture_holds_the_cases(built):
    fx = RR.fixture()
    lock = LR.fixture()["cases"]
    assert (fx["M"], fx["max_iter"], fx["crawl_limit"], fx["crawl_frac"]) == (LR.M_NODES, 200, 3, 0.3)
    for tf in LR.TFS:
        c = fx["cases"][str(tf)]
        on, off = c["blocked"]["rule_on"], c["blocked"]["rule_off"]
        print(f"tf {tf} blocked: rule on {on}; rule off {off}")
        assert c["blocked"]["discs"][0] == list(LR.NO_PATH_DISC)
        assert on["status"] == "locally infeasible" and on["iterations"] < 200 and on["newton_steps"] >= 1 and on["restored_steps"] >= 1
        assert on["rho"] >= 1e5
        assert off["status"] == "max_iter" and off["iterations"] == 200 and off["newton_steps"] == 0 == off["restored_steps"]
        assert on["iterations"] * 2 < off["iterations"] and on["evaluations"] * 4 < off["evaluations"]
        assert len(c["regular"]) == 9
        for row, inst, ref in zip(c["regular"], LR.instances(tf), lock[str(tf)]):
            assert row["discs"] == [list(d) for d in inst["discs"]] and row["bump"] == inst["bump"]
            a, b = row["rule_on"], row["rule_off"]
            assert a["status"] == b["status"] == "converged"
            assert a == b                                   # no first trial is ever rejected there: the rule leaves them alone
            assert abs(a["cost"] - ref["cost"]) < 1e-6 * abs(ref["cost"])
    b40 = fx["cases"]["4.0"]["blocked"]["rule_on"]
    b25 = fx["cases"]["2.5"]["blocked"]["rule_on"]
    assert [b40[k] for k in ("iterations", "evaluations", "newton_steps", "restored_steps")] == [72, 279, 6, 7]
    assert [b25[k] for k in ("iterations", "evaluations", "newton_steps", "restored_steps")] == [78, 376, 6, 9]


def test_the_blocked_case_reproduces_its_row(built):
    """solve_nlp under the device's rule set (NlpOptions::second_order_correction off) on the blocked instance of tf = 4.0"""
    h = RR.load_harness()
    tf = LR.TFS[0]
    want = RR.fixture()["cases"][str(tf)]["blocked"]["rule_on"]
    got = RR.solve_oracle(h, tf, RR.blocked_instance(tf), RR.OPTIONS["crawl_limit"], RR.OPTIONS["crawl_frac"])
    print(got)
    for k in ("status", "iterations", "evaluations", "newton_steps", "restored_steps", "rho"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["cost"] - want["cost"]) <= 1e-9 * abs(want["cost"])
