"""emi_ipm_solve_restart_dev / _host: the lock-step ladder run again, from the next start, on the instances an attempt did not solve.
-m gpu

The instances, helpers and tolerances are those of tests/ladder_ref.py, refine_ref.py, lockstep_ref.py, test_gpu_refine.py and
test_gpu_lockstep.py: the nine quadrotor instances of a final time on the ladder (21, 41) and, where the ODE check matters, on
(21, 41, 61).  One attempt is held bit for bit to the existing calls; an attempt on a compacted batch to the refine call on a fresh
context that holds those instances alone; an instance that climbs in a compacted batch to the same instance in the whole batch
within 1e-6 relative, the criterion of tests/test_gpu_refine.py.  The restart that matters is held to a CPU fixture of its own
(tests/restart_ref.py, tests/golden/restart_cases.json: walls of discs across the straight line, which only the planned route gets
past): every instance solved, in the fixture's attempt, at the fixture's cost within 1e-6, one of them against the independent
polish."""
import ctypes as C

import numpy as np
import pytest

import ladder_ref as LD
import lockstep_ref as LR
import refine_ref as RR
import restart_ref as RS
import test_gpu_ladder as TG
import test_gpu_lockstep as TL
import test_gpu_refine as TGR
import track_ladder_ref as TR

pytestmark = pytest.mark.gpu

TOL = TL.TOL
NV, NS, NC, NP = TL.NV, TL.NS, TL.NC, TL.NP
ROWS, KEYS, OK = TGR.ROWS, TGR.KEYS, TGR.OK
same = TGR.same
TF = LR.TFS[0]
LADDER = RR.LADDER[:3]              # (21, 41, 61), checked from the second rung on
ODE_TOL = RR.TOLS[TF]
XA, XB = [1.0, 1.0, 0, 0, 0, 0], [8.0, 6.0, 0, 0, 0, 0]            # the end states of ladder_ref.quad_at
LINE = dict(kind=0, xa=XA, xb=XB)                                   # EMI_START_LINE
DROP = 1                                                            # EMI_RESTART_DROP_FAILED
WRONG_SIDE = [0, 1, 2, 6, 7, 8, 3, 4, 5]                            # the instance with the same discs and the opposite bump


def uploader(ev, dev):
    import torch
    return (lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)) if dev else (lambda a: np.ascontiguousarray(a).copy())


def rungs_of(tf, B, ladder, options, up, replicate=False, recs=None):
    rungs = []
    for M in ladder:
        bd = TG.bounds_at(tf, M, lambda a: a)
        if replicate:
            bd["zl"], bd["zu"] = np.repeat(bd["zl"], B, 0), np.repeat(bd["zu"], B, 0)
        bd["zl"], bd["zu"] = up(bd["zl"]), up(bd["zu"])
        rungs.append(dict(M=M, bounds=bd, options=dict(options), repair=0, recs=recs))
    return rungs


def starts_of(insts, M0):
    z0 = np.stack([i["z0"] for i in insts]).reshape(len(insts), NV, M0)
    return np.ascontiguousarray(z0[:, :NS]), np.ascontiguousarray(z0[:, NS:])


def restart(ev, tf, insts, ladder, options, starts, X0=None, tol=ODE_TOL, first_check=RR.FIRST_CHECK, patience=None, flags=0, retry_mask=0,
            dev=True, ldm=None, replicate=False, recs=None):
    """one call into NaN-filled arrays [B][rows][ldm]; X0: None, or numpy [B][NS][ladder[0]]; the controls are the instances' own.
    -> dict X U LamF LamC (numpy), res[attempt][rung][b], err [attempts][rungs][B], out[b]"""
    import torch
    B = len(insts)
    ldm = ldm or max(ladder)
    up = uploader(ev, dev)
    U0 = starts_of(insts, ladder[0])[1]
    rungs = rungs_of(tf, B, ladder, options, up, replicate, recs)
    out = tuple(up(np.full((B, r, ldm), np.nan)) for r in ROWS)
    X0d, U0d = (up(X0) if X0 is not None else None), up(U0)
    if dev:
        torch.cuda.synchronize()
    X, U, LamF, LamC, res, err, summ = ev.ipm_solve_restart(rungs, 0.0, tf, starts, U0d, X0=X0d, ode_tol=tol, first_check=first_check, ul=RR.UL,
                                                            uu=RR.UU, patience=patience, retry_mask=retry_mask, flags=flags, out=out, dev=dev)
    if dev:
        ev.synchronize()
        assert np.array_equal(U0d.cpu().numpy(), U0) and (X0 is None or np.array_equal(X0d.cpu().numpy(), X0))       # only read
        X, U, LamF, LamC = (t.cpu().numpy() for t in (X, U, LamF, LamC))
    return dict(X=X, U=U, LamF=LamF, LamC=LamC, res=res, err=err, out=summ, ladder=tuple(ladder))


def refine_from(ev, tf, insts, ladder, options, X0d, tol=ODE_TOL, first_check=RR.FIRST_CHECK, ldm=None):
    """emi_ipm_solve_refine_dev from the states X0d (a device tensor) and the instances' own controls, into NaN-filled arrays"""
    import torch
    B = len(insts)
    up = uploader(ev, True)
    rungs = rungs_of(tf, B, ladder, options, up)
    out = tuple(up(np.full((B, r, ldm or max(ladder)), np.nan)) for r in ROWS)
    U0d = up(starts_of(insts, ladder[0])[1])
    torch.cuda.synchronize()
    X, U, LamF, LamC, res, err, summ = ev.ipm_solve_refine(rungs, 0.0, tf, X0d, U0d, tol, first_check, RR.UL, RR.UU, out=out)
    ev.synchronize()
    X, U, LamF, LamC = (t.cpu().numpy() for t in (X, U, LamF, LamC))
    return dict(X=X, U=U, LamF=LamF, LamC=LamC, res=res, err=err, out=summ, ladder=tuple(ladder))


def line_start(ev, tf, M0):
    ev.set_mesh(M0, 0.0, tf)
    X0d, _ = ev.start_guess(LINE["kind"], XA, XB)
    ev.synchronize()
    return X0d


REFINE_FIELDS = ("rung", "verdict", "rungs_solved", "err")


def same_refine(q, p):
    return all(same(np.float64(q[k]), np.float64(p[k])) for k in REFINE_FIELDS)


def is_the_refine_call(got, want, attempt=0, who=None, where=None):
    """attempt `attempt` of a restart run for the instances `who` (the caller's numbers) against a refine run's instances `where`"""
    who = list(range(len(want["out"]))) if who is None else who
    where = list(range(len(who))) if where is None else where
    for k in KEYS:
        assert same(got[k][who], want[k][where]), k
    for r in range(len(want["res"])):
        assert [got["res"][attempt][r][b] for b in who] == [want["res"][r][j] for j in where], r
    assert same(got["err"][attempt][:, who], want["err"][:, where])
    for b, j in zip(who, where):
        assert got["out"][b]["attempt"] == attempt and same_refine(got["out"][b], want["out"][j]), (b, got["out"][b], want["out"][j])


def padding_is_kept(r, who=None):
    return TGR.padding_is_kept(dict(r, out=[q for b, q in enumerate(r["out"]) if who is None or b in who],
                                    **{k: r[k][[b for b in range(len(r["out"])) if who is None or b in who]] for k in KEYS}))


def show(tag, r):
    for a, block in enumerate(r["res"]):
        print(f"{tag} attempt {a}: status / iterations per rung", [[(q["status"], q["iterations"]) for q in g] for g in block])
    print(f"{tag} out:", [(q["attempt"], q["attempts"], q["level"], q["rung"], q["verdict"]) for q in r["out"]])


@pytest.fixture(scope="module")
def runs(built):
    insts = LD.instances(TF)
    ev = TG.fresh_ev(TF, insts)
    line = restart(ev, TF, insts, LADDER, dict(tol=TOL), [LINE])
    show("LINE", line)
    yield dict(insts=insts, ev=ev, line=line)
    ev.close()


@pytest.fixture(scope="module")
def some(runs):
    """test 3's run: the budget of rung 0 in attempt 0 is the smallest iteration count of the LINE run there"""
    its = [q["iterations"] for q in runs["line"]["res"][0][0]]
    n = min(its)
    r = restart(runs["ev"], TF, runs["insts"], LADDER, dict(tol=TOL), [LINE, LINE], patience=[n, 0], flags=DROP)
    show("some restart", r)
    return dict(r=r, n=n, winners=[b for b, i in enumerate(its) if i == n], rest=[b for b, i in enumerate(its) if i != n])


# ---- 1. one attempt is the existing call ------------------------------------------------------------------------------------------------
def test_one_attempt_from_a_guess_is_the_refine_call(runs):
    insts = runs["insts"]
    ev = TG.fresh_ev(TF, insts)
    want = TGR.refine(ev, TF, insts, LADDER, dict(tol=TOL), ODE_TOL, ldm=LADDER[-1] + 3)
    got = restart(ev, TF, insts, LADDER, dict(tol=TOL), [], X0=starts_of(insts, LADDER[0])[0], ldm=LADDER[-1] + 3)
    assert ev.layout.B == len(insts) and ev.layout.M == LADDER[max(q["rungs_solved"] for q in want["out"]) - 1]
    ev.close()
    is_the_refine_call(got, want)
    assert all(q["attempts"] == 1 and q["level"] == -2 for q in got["out"]) and len(got["res"]) == 1
    assert TGR.padding_is_kept(got) and len({q["rung"] for q in got["out"]}) > 1          # (somebody left the batch early)


def test_one_attempt_without_a_check_is_the_ladder_call(runs):
    insts = runs["insts"]
    Ml = LD.LADDER[-1]
    ev = TG.fresh_ev(TF, insts)
    want = TG.climb(ev, TF, insts, LD.LADDER, dict(tol=TOL))
    got = restart(ev, TF, insts, LD.LADDER, dict(tol=TOL), [], X0=starts_of(insts, LD.LADDER[0])[0], tol=None, ldm=Ml + 3)
    assert ev.layout.B == len(insts) and ev.layout.M == Ml
    ev.close()
    for k in KEYS:
        assert same(got[k][:, :, :Ml], want[k]) and np.isnan(got[k][:, :, Ml:]).all(), k
    assert got["res"][0] == want["res"] and np.isnan(got["err"]).all()
    for b, q in enumerate(got["out"]):
        ok = want["res"][-1][b]["status"] in OK
        assert (q["attempt"], q["attempts"], q["rung"], q["verdict"], q["rungs_solved"]) == (0, 1, 1, RR.MET if ok else RR.FAILED, 2), q


def test_one_attempt_from_the_line_is_the_start_call_and_the_refine_call(runs):
    insts = runs["insts"]
    ev = TG.fresh_ev(TF, insts)
    want = refine_from(ev, TF, insts, LADDER, dict(tol=TOL), line_start(ev, TF, LADDER[0]))
    ev.close()
    is_the_refine_call(runs["line"], want)
    assert all(q["attempts"] == 1 and q["level"] == -2 for q in runs["line"]["out"]) and TGR.padding_is_kept(runs["line"])


# ---- 2. everybody restarts ----------------------------------------------------------------------------------------------------------------
def test_everybody_restarts(runs):
    insts, ev, line = runs["insts"], runs["ev"], runs["line"]
    B = len(insts)
    # the guess of attempt 0: the start of the instance with the same discs and the opposite bump, which is that fixture instance's
    # own problem from its own start -- and no fixture instance converges on rung 0 in 2 iterations
    cpu = RR.fixture()["cases"][str(TF)]
    assert [insts[j]["discs"] for j in WRONG_SIDE] == [i["discs"] for i in insts] and all(insts[j]["bump"] == -i["bump"] for i, j in zip(insts, WRONG_SIDE))
    assert min(row["rungs"][0]["iterations"] for row in cpu) > 2
    X0 = starts_of(insts, LADDER[0])[0][WRONG_SIDE]
    r = restart(ev, TF, insts, LADDER, dict(tol=TOL), [LINE], X0=X0, patience=[2, 0], flags=DROP)
    show("everybody", r)
    assert all(q["status"] == LR.MAX_ITER and q["iterations"] == 2 for q in r["res"][0][0])
    assert all(q["status"] == -1 for g in r["res"][0][1:] for q in g) and np.isnan(r["err"][0]).all()
    for k in KEYS:                                          # attempt 1 on the whole batch: the LINE run
        assert same(r[k], line[k]), k
    assert r["res"][1] == line["res"][0] and same(r["err"][1], line["err"][0])
    for b in range(B):
        q, p = r["out"][b], line["out"][b]
        assert q["attempts"] == 2 and same_refine(q, p), (b, q, p)
        assert q["attempt"] == (0 if p["verdict"] == RR.FAILED else 1), (b, q)
    assert all(q["attempt"] == 1 for q in r["out"])                 # (the LINE run solves all nine)


# ---- 3. some restart ------------------------------------------------------------------------------------------------------------------------
def test_some_restart(runs, some):
    insts, line, r = runs["insts"], runs["line"], some["r"]
    winners, rest = some["winners"], some["rest"]
    assert winners and rest
    # attempt 0: who converges within the budget climbs in a compacted batch, the rest drop on rung 0
    for b in winners:
        assert r["res"][0][0][b] == line["res"][0][0][b] and r["out"][b]["attempt"] == 0 and r["out"][b]["attempts"] == 1
        q, p = r["out"][b], line["out"][b]
        assert (q["rung"], q["verdict"], q["rungs_solved"]) == (p["rung"], p["verdict"], p["rungs_solved"]), (b, q, p)
        M = LADDER[q["rung"]]
        for k in ("X", "U"):
            d = np.abs(r[k][b, :, :M] - line[k][b, :, :M]).max() / np.abs(line[k][b, :, :M]).max()
            assert d < 1e-6, (b, k, d)
        assert all(g[b]["status"] == -1 for g in r["res"][1])
    for b in rest:
        assert r["res"][0][0][b]["status"] == LR.MAX_ITER and r["res"][0][0][b]["iterations"] == some["n"]
        assert all(g[b]["status"] == -1 for g in r["res"][0][1:]) and r["res"][1][0][b]["status"] != -1
    # attempt 1 solves exactly the dropped ones: the refine call from the LINE start on a context that holds only those, in their order
    sub = [insts[b] for b in rest]
    ev = TG.fresh_ev(TF, sub)
    want = refine_from(ev, TF, sub, LADDER, dict(tol=TOL), line_start(ev, TF, LADDER[0]))
    ev.close()
    solved = [b for b in rest if line["out"][b]["verdict"] != RR.FAILED]
    assert solved
    for b in rest:
        q, p = r["out"][b], line["out"][b]
        assert q["attempts"] == 2 and q["attempt"] == (1 if b in solved else 0), (b, q)
        if b in solved:
            assert (q["rung"], q["verdict"], q["rungs_solved"]) == (p["rung"], p["verdict"], p["rungs_solved"]), (b, q, p)
    is_the_refine_call(r, want, attempt=1, who=solved, where=[rest.index(b) for b in solved])
    for j, b in enumerate(rest):
        assert [g[b] for g in r["res"][1]] == [g[j] for g in want["res"]], b
    assert padding_is_kept(r, winners + solved)


# ---- 4. an instance nobody can solve -----------------------------------------------------------------------------------------------------
def test_an_instance_nobody_can_solve_fails_alone(runs):
    opt = dict(tol=TOL, max_iter=100, rules=1)
    blocked = dict(discs=LR.discs_of(LR.NO_PATH_DISC), bump=0.0, z0=runs["insts"][0]["z0"])
    three = [runs["insts"][2], blocked, runs["insts"][5]]
    X0 = starts_of(three, LADDER[0])[0]
    bend = dict(kind=1, xa=XA, xb=XB, bend=0.15 * 7.0)
    ev = TG.fresh_ev(TF, three)
    r = restart(ev, TF, three, LADDER, opt, [LINE, bend], X0=X0, flags=DROP)
    alone = restart(ev, TF, three, LADDER, opt, [], X0=X0, flags=DROP)
    assert ev.layout.B == 3
    ev.close()
    show("blocked", r)
    bad = r["out"][1]
    assert (bad["verdict"], bad["attempts"], bad["attempt"]) == (RR.FAILED, 3, 0), bad
    assert all(r["res"][a][0][1]["status"] not in OK + (-1,) for a in range(3))
    for b in (0, 2):
        assert r["out"][b]["verdict"] != RR.FAILED and r["out"][b]["attempts"] == 1
        assert all(q[b]["status"] == -1 for a in (1, 2) for q in r["res"][a])
    is_the_refine_call(r, dict(alone, res=alone["res"][0], err=alone["err"][0]), who=[0, 1, 2])
    assert padding_is_kept(r)


# ---- 5. a restart that matters ---------------------------------------------------------------------------------------------------------------
def test_a_restart_that_matters(built):
    """the walls of tests/restart_ref.py: the CPU climb (tests/golden/restart_cases.json) is solved from the line for the thin walls; for
    the thick ones it ends on 41 nodes with the constraints violated from the line and solved from the planned route"""
    import torch
    import etol_amd as E
    import indep_nlp as N
    fx = RS.fixture()
    cases = fx["cases"]
    B, nd, Ml = len(cases), RS.NDISCS, RS.LADDER[-1]
    assert [c["name"] for c in cases] == [n for n, _ in RS.WALLS] and [c["discs"] for c in cases] == [[list(d) for d in w] for _, w in RS.WALLS]
    assert sum(c["attempt"] == 1 for c in cases) >= 2 and any(c["attempt"] == 0 for c in cases)
    discs = [[tuple(d) for d in c["discs"]] for c in cases]
    recs = np.stack([LR.records(d) for d in discs])
    cl, cu, cs = np.full(nd, -1000.0), np.zeros(nd), np.ones(nd)

    def context(recs):
        ev = E.Evaluator(0)
        ev.set_mesh(9, 0.0, 1.0)
        ev.set_model(1, LR.QUAD_PARAMS)
        ev.set_batch(recs.shape[0])
        ev.set_path(recs, 0, 1)
        return ev

    ev = context(recs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
    rungs = []
    for M in RS.LADDER:
        P = RS.quad_at(M, discs[0])
        rungs.append(dict(M=M, bounds=dict(zl=up(P.lo.reshape(1, NV, M)), zu=up(P.up.reshape(1, NV, M)), cl=cl, cu=cu, cscale=cs),
                          options=dict(tol=RS.TOL, max_iter=RS.MAX_ITER), repair=0))
    U0 = up(np.stack([RS.start(RS.LADDER[0], d, "line")[0].reshape(NV, -1)[NS:] for d in discs]))
    common = dict(xa=RS.XA, xb=RS.XB, box=RS.BOX)
    starts = [dict(kind=E.START_LINE, **common), dict(kind=E.START_PLANNED, clearance=RS.CLEARANCE, bend=0.15 * 7.0, **common)]
    assert [s["kind"] for s in starts] == [E.START_LINE, E.START_PLANNED] and fx["starts"] == ["line", "planned"]
    torch.cuda.synchronize()
    X, U, LamF, LamC, res, err, out = ev.ipm_solve_restart(rungs, 0.0, RS.TF, starts, U0, flags=DROP)
    ev.synchronize()
    ev.close()
    X, U = X.cpu().numpy(), U.cpu().numpy()
    for b, (c, q) in enumerate(zip(cases, out)):
        got = res[q["attempt"]][q["rung"]][b]
        print(f"{c['name']}: attempt {q['attempt']} of {q['attempts']} (fixture {c['attempt']}) level {q['level']} rung {q['rung']} verdict {q['verdict']} "
              f"status {got['status']} cost {got['cost']:.9f} (fixture {c['cost']:.9f}); per attempt status / iterations / viol "
              + str([[(g[b]["status"], g[b]["iterations"], f"{g[b]['constr_viol']:.1e}") for g in block] for block in res]))
    for b, (c, q) in enumerate(zip(cases, out)):
        got = res[q["attempt"]][q["rung"]][b]
        assert q["verdict"] == RR.MET and q["rung"] == len(RS.LADDER) - 1 and got["status"] in OK, (b, q)            # every instance solved
        assert (q["attempt"], q["attempts"]) == (c["attempt"], c["attempt"] + 1), (b, q)
        assert q["level"] == (c["climbs"]["planned"]["level"] if c["attempt"] == 1 else -2), (b, q)
        assert abs(got["cost"] - c["cost"]) <= 1e-6 * abs(c["cost"]), (b, got["cost"], c["cost"])
    # one restarted instance against the independent polish, from its own solve to 1e-10 on the last rung
    b = next(b for b, c in enumerate(cases) if c["attempt"] == 1)
    ev = context(recs[b:b + 1])
    ev.set_mesh(Ml, 0.0, RS.TF)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
    Xf, Uf = up(X[b:b + 1, :, :Ml]), up(U[b:b + 1, :, :Ml])
    P = RS.quad_at(Ml, discs[b])
    bd = dict(zl=up(P.lo.reshape(1, NV, Ml)), zu=up(P.up.reshape(1, NV, Ml)), cl=cl, cu=cu, cscale=cs)
    torch.cuda.synchronize()
    _, _, fine = ev.ipm_solve_shard(Xf, Uf, bd, dict(tol=TL.TOL_FINE, max_iter=120, mu_init=1e-4))
    ev.synchronize()
    ev.close()
    assert fine[0]["status"] in OK, fine[0]
    TL.meets_the_solve_criterion(RS.TF, dict(discs=discs[b]), dict(cost=cases[b]["cost"]), X[b, :, :Ml], U[b, :, :Ml],
                                 res[out[b]["attempt"]][out[b]["rung"]][b]["cost"], Xf.cpu().numpy()[0], Uf.cpu().numpy()[0], cases[b]["name"])


# ---- 6. tables and bounds per instance, tracks -------------------------------------------------------------------------------------------
def test_bounds_per_instance_and_tables_per_rung_change_no_bit(runs, some):
    insts, ev = runs["insts"], runs["ev"]
    recs = np.stack([LR.records(i["discs"]) for i in insts])
    r = restart(ev, TF, insts, LADDER, dict(tol=TOL), [LINE, LINE], patience=[some["n"], 0], flags=DROP, replicate=True, recs=recs)
    assert TGR.same_run(r, some["r"])
    # ... nor do end states given per instance, in the caller's numbering: the sets of the pending instances are gathered on the host
    per = dict(LINE, xa=np.tile(XA, (len(insts), 1)), xb=np.tile(XB, (len(insts), 1)))
    r = restart(ev, TF, insts, LADDER, dict(tol=TOL), [per, per], patience=[some["n"], 0], flags=DROP)
    assert TGR.same_run(r, some["r"])


def test_a_track_at_rest_fed_from_waypoints_changes_no_bit(runs, some):
    """the first disc of every instance as a row of kind EMI_PATH_TRACK whose waypoints (one set per instance) do not move: the
    compacted batches read their centres through the set map"""
    import test_gpu_track_ladder as TT
    insts = TR.static_instances(TF)
    ev = TT.track_ev(insts)
    recs = np.stack([i["recs"] for i in insts])
    r = restart(ev, TF, insts, LADDER, dict(tol=TOL), [LINE, LINE], patience=[some["n"], 0], flags=DROP, replicate=True, recs=recs)
    M = ev.layout.M
    assert ev.layout.B == len(insts)
    xc, yc = ev.get_tracks()                                # all B sets again, on the mesh the context is on
    ev.close()
    wx, wy = TR.host_centres([i["way"] for i in insts], M, 0.0, TF)
    assert same(xc, wx) and same(yc, wy)
    assert TGR.same_run(r, some["r"])


# ---- 7. two calls, the host form, the context afterwards -----------------------------------------------------------------------------------
def test_two_calls_the_host_form_and_the_context_afterwards(runs, some):
    insts, ev = runs["insts"], runs["ev"]
    kw = dict(patience=[some["n"], 0], flags=DROP)
    again = restart(ev, TF, insts, LADDER, dict(tol=TOL), [LINE, LINE], **kw)
    assert TGR.same_run(again, some["r"])
    host = restart(ev, TF, insts, LADDER, dict(tol=TOL), [LINE, LINE], dev=False, **kw)
    assert TGR.same_run(host, some["r"])
    # batch, table and mesh of the context: all B instances, every instance's own records, the last rung that was solved (in the last attempt)
    last = max(q["rungs_solved"] for b, q in enumerate(some["r"]["out"]) if some["r"]["res"][1][0][b]["status"] != -1)
    assert ev.layout.B == len(insts) and ev.layout.np == NP and ev.layout.M == LADDER[last - 1]
    ev.set_mesh(TL.M, 0.0, TF)
    at41 = LR.instances(TF)
    after = TL.solve(ev, TF, at41, dict(tol=TOL, max_iter=200))
    fresh = TL.make_ev(TF, at41)
    want = TL.solve(fresh, TF, at41, dict(tol=TOL, max_iter=200))
    fresh.close()
    assert TL.same_bits(after, want) and after["res"] == want["res"]
    # the refine call of tests/test_gpu_refine.py on this context against a fresh one
    mine = TGR.refine(ev, TF, insts, RR.LADDER, dict(tol=TOL), ODE_TOL)
    fresh = TG.fresh_ev(TF, insts)
    theirs = TGR.refine(fresh, TF, insts, RR.LADDER, dict(tol=TOL), ODE_TOL)
    fresh.close()
    assert TGR.same_run(mine, theirs)


# ---- 8. statuses ----------------------------------------------------------------------------------------------------------------------------
def test_restart_statuses(built):
    import torch
    import etol_amd as E
    from etol_amd import _lib as L
    lib = E.load()
    insts = LD.instances(TF)[:2]
    M0, M1 = LD.LADDER
    xa, xb = (np.array([v, v, v]) for v in (XA, XB))

    def call(ev, rs=True, nstarts=1, starts=True, x0=True, nsets=1, patience=None, mask=0, flags=0, rf=True, ldm=M1):
        dev = ev.device
        new = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        keep = [new(2, NS, M0), new(2, NC, M0), new(2, NS, M1), new(2, NC, M1), new(2, NS, M1), new(2, NP, M1)]
        arr = (L.IpmRung * 2)()
        for g, M in zip(arr, LD.LADDER):
            bd = TG.bounds_at(TF, M, lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev))
            keep += [bd["zl"], bd["zu"]]
            g.M, g.bd.zl, g.bd.zu, g.bd.nsets = M, p(bd["zl"]), p(bd["zu"]), 1
            g.bd.cl, g.bd.cu = LR.CL.ctypes.data_as(LD.D_), LR.CU.ctypes.data_as(LD.D_)
            g.opt.max_iter = 2
        r = L.IpmRefine()
        r.ode_tol, r.first_check = 1e-3, 1
        st = (L.Start * 8)()
        for g in st:
            g.kind, g.nsets, g.xa, g.xb = 0, nsets, xa.ctypes.data_as(LD.D_), xb.ctypes.data_as(LD.D_)
        s = L.IpmRestart()
        s.nstarts, s.retry_mask, s.flags = nstarts, mask, flags
        if starts:
            s.starts = st
        if patience is not None:
            pat = (C.c_int * 9)(*patience)
            s.patience = pat
        res, e, o = (L.IpmResult * (9 * 2 * 2))(), np.zeros(9 * 2 * 2), (L.IpmRestartResult * 2)()
        torch.cuda.synchronize()
        code = lib.emi_ipm_solve_restart_dev(ev.ctx, 2, arr, 0.0, TF, C.byref(r) if rf else None, C.byref(s) if rs else None,
                                             p(keep[0]) if x0 else None, p(keep[1]), ldm, p(keep[2]), p(keep[3]), p(keep[4]), p(keep[5]), res,
                                             e.ctypes.data_as(LD.D_), o)
        ev.synchronize()
        return code

    ev = TG.fresh_ev(TF, insts, f32=True)
    assert call(ev) == 5                                        # EMI_ERR_UNSUPPORTED: f32 context
    ev.close()
    ev = TG.fresh_ev(TF, insts)
    track = np.stack([LR.records(i["discs"]) for i in insts])
    track[1, 0, :3] = [2, 0, 0.25]
    ev.set_path(track, 0, 1)
    assert call(ev) == 5                                        # track rows without waypoint tables, as in the ladder call
    ev.set_path(np.stack([LR.records(i["discs"]) for i in insts]), 0, 1)
    lay = L.Layout()                                            # (asked of the library: the evaluator caches its own)

    def refused(**kw):
        assert call(ev, **kw) == 1, kw                          # EMI_ERR_ARG
        assert lib.emi_get_layout(ev.ctx, C.byref(lay)) == 0 and (lay.B, lay.np) == (2, NP)
        assert call(ev) == 0, kw                                # the context still solves

    refused(rs=False)
    refused(nstarts=0, x0=False)                                # no attempt at all
    refused(nstarts=8)                                          # a guess and 8 starts: 9 attempts
    refused(nstarts=-1)
    refused(starts=False)
    refused(nsets=3)
    refused(nsets=0)
    refused(patience=[0, -1])
    refused(mask=16)
    refused(mask=-1)
    refused(flags=2)
    refused(ldm=M1 - 1)
    assert call(ev, nstarts=7) == 0 and call(ev, nstarts=8, x0=False) == 0                   # 8 attempts either way
    assert call(ev, nstarts=0) == 0 and call(ev, x0=False) == 0 and call(ev, rf=False) == 0 and call(ev, nsets=2) == 0
    assert call(ev, patience=[1, 0], mask=15, flags=1) == 0 and call(ev, starts=False, nstarts=0) == 0
    assert lib.emi_get_layout(ev.ctx, C.byref(lay)) == 0 and (lay.B, lay.np) == (2, NP)
    ev.close()
    assert lib.emi_ipm_solve_restart_dev(None, 0, None, 0.0, 1.0, None, None, None, None, 0, None, None, None, None, None, None, None) == 1
