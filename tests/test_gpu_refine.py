"""emi_prolong_rows_dev, emi_shard_move_dev, emi_ipm_solve_refine_dev / _host: the lock-step solve of a context's batch over a mesh
ladder with the instances retired as they meet the ODE tolerance.  -m gpu

References: tests/refine_ref.py.  The two kernels are held bit for bit: a row of the prolongation with a row map to emi_prolong_dev on
its source row, a move to the source's bits with everything it does not name left as it was.  The driver: with a tolerance of 0 to
emi_ipm_solve_ladder_dev and with +inf to emi_ipm_solve_shard_dev on the first rung, bit for bit; on the 2 x 9 instances of
tests/ladder_ref.py over (21, 41, 61, 91) to tests/golden/refine_cases.json (the CPU climb, tests/golden/gen_refine_cases.py): the
same retiring rung and verdict for every instance, the cost there within 1e-6, the certificate of every retiring group, the
returned estimate against the long-double restatement of tests/ode_error_ref.py within the bound derived there, the criterion of
tests/test_gpu_lockstep.py (trajectory within 1e-6 of the KKT point the independent polish reaches from a solve to 1e-10; here the
one-mesh solve of the retiring group on its rung, carried on from what the call returned) for one instance per retiring rung,
iteration sums per rung within 1.5 x the fixture's."""
import ctypes as C

import numpy as np
import pytest

import ladder_ref as LD
import lockstep_ref as LR
import ode_error_ref as OE
import refine_ref as RR
import test_gpu_ladder as TG
import test_gpu_lockstep as TL

pytestmark = pytest.mark.gpu

TOL, TOL_FINE = TL.TOL, TL.TOL_FINE
NV, NS, NC, NP = TL.NV, TL.NS, TL.NC, TL.NP
ROWS = (NS, NC, NS, NP)
KEYS = ("X", "U", "LamF", "LamC")
OK = (LR.CONVERGED, LR.ACCEPTABLE)
bits = TG.bits


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ((21, 41), (40, 41), (5, 9)), ids=lambda p: f"{p[0]}-{p[1]}")
def test_prolongation_with_a_row_map(built, pair):
    import torch
    import etol_amd as E
    ev, (mc, mf) = E.Evaluator(0), pair
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    PT = up(ev.prolong_matrix(mc, mf).T)
    rng = np.random.default_rng(mc * 1000 + mf)
    for R in (1, 7, 54):
        V = up(rng.standard_normal((R, mc)) * np.exp(3 * rng.standard_normal((R, 1))))
        ident = up(np.arange(R, dtype=np.int32))
        perm = rng.permutation(R).astype(np.int32)
        rep = rng.integers(0, R, 2 * R + 3).astype(np.int32)                      # repeats, and more rows out than in
        torch.cuda.synchronize()
        want = ev.prolong(PT, V)
        got = [ev.prolong_rows(PT, V, m) for m in (None, ident, up(perm), up(rep))]
        alone = {r: ev.prolong(PT, V[r:r + 1].contiguous()) for r in {int(perm[0]), int(rep[-1])}}
        ev.synchronize()
        want = want.cpu().numpy()
        none, idn, prm, rpt = (g.cpu().numpy() for g in got)
        assert same(none, want) and same(idn, want), (pair, R)
        assert prm.shape == (R, mf) and rpt.shape == (2 * R + 3, mf)
        assert same(prm, want[perm]) and same(rpt, want[rep]), (pair, R)
        assert same(prm[0], alone[int(perm[0])].cpu().numpy()[0]) and same(rpt[-1], alone[int(rep[-1])].cpu().numpy()[0]), (pair, R)
    ev.close()


@pytest.mark.parametrize("pair", ((5, 9), (40, 41)), ids=lambda p: f"{p[0]}-{p[1]}")
def test_the_two_prolongation_calls_are_one_kernel(built, pair):
    """emi_prolong_dev and emi_prolong_rows_dev without a map: the same bits at R = 1, 5 and 9, the tail groups of the 4-row blocking;
    a unit row of P (the end nodes, which every LGL mesh has) still copies the coarse value bit for bit"""
    import torch
    import etol_amd as E
    ev, (mc, mf) = E.Evaluator(0), pair
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    P = ev.prolong_matrix(mc, mf)
    unit = [(q, int(np.argmax(P[q]))) for q in range(mf) if np.count_nonzero(P[q]) == 1 and P[q].max() == 1.0]
    assert {(0, 0), (mf - 1, mc - 1)} <= set(unit)
    PT = up(P.T)
    rng = np.random.default_rng(mc * 1000 + mf + 1)
    for R in (1, 5, 9):
        V = rng.standard_normal((R, mc)) * np.exp(3 * rng.standard_normal((R, 1)))
        Vd = up(V)
        torch.cuda.synchronize()
        plain, rows = ev.prolong(PT, Vd), ev.prolong_rows(PT, Vd, None)
        ev.synchronize()
        plain, rows = plain.cpu().numpy(), rows.cpu().numpy()
        assert plain.shape == (R, mf) and same(plain, rows), (pair, R)
        for q, j in unit:
            assert same(plain[:, q], V[:, j]), (pair, R, q, j)
    ev.close()


@pytest.mark.parametrize("M", (33, 300))
@pytest.mark.parametrize("pad", (0, 7))
def test_shard_move_copies_bits_and_touches_nothing_else(built, M, pad):
    import torch
    import etol_amd as E
    ev, B, ldm = E.Evaluator(0), 5, M + pad
    rng = np.random.default_rng(M + pad)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    idx = lambda v: up(np.array(v, dtype=np.int32))
    compact = [rng.standard_normal((B, r, M)) for r in ROWS]
    padded = [rng.standard_normal((B + 2, r, ldm)) for r in ROWS]
    for narr in (1, 4):
        for src_list, dst_list in (([], []), ([3], [6]), ([4, 0, 2, 1, 3], [0, 6, 1, 5, 2])):
            # compact -> padded (a scatter into NaN), and padded -> compact (a gather into NaN)
            for src, dst_shape, ld_from, s_l, d_l in ((compact, (B + 2, ldm), M, src_list, dst_list), (padded, (B, M), ldm, dst_list, src_list)):
                dst = [torch.full((dst_shape[0], r, dst_shape[1]), float("nan"), dtype=torch.float64, device=ev.device) for r in ROWS[:narr]]
                srcd = [up(a) for a in src[:narr]]
                torch.cuda.synchronize()
                ev.shard_move(srcd, dst, M, idx(s_l) if s_l else None, idx(d_l) if d_l else None, n=len(s_l))
                ev.synchronize()
                for a, s0, d in zip(src, srcd, dst):
                    d = d.cpu().numpy()
                    assert same(s0.cpu().numpy(), a)                                    # the source is only read
                    want = np.full(d.shape, np.nan)
                    for i, j in zip(s_l, d_l):
                        want[j, :, :M] = a[i, :, :M]
                    assert same(d, want), (M, pad, narr, s_l)
    # the lists default to 0 .. n-1
    dst = [torch.full((B, r, ldm), float("nan"), dtype=torch.float64, device=ev.device) for r in ROWS]
    srcd = [up(a) for a in compact]
    torch.cuda.synchronize()
    ev.shard_move(srcd, dst, M, n=3)
    ev.synchronize()
    for a, d in zip(compact, dst):
        want = np.full((B, a.shape[1], ldm), np.nan)
        want[:3, :, :M] = a[:3]
        assert same(d.cpu().numpy(), want)
    ev.close()


def test_kernel_statuses(built):
    import torch
    import etol_amd as E
    lib, ev = E.load(), E.Evaluator(0)
    t = torch.zeros(64, dtype=torch.float64, device=ev.device)
    p = C.c_void_p(t.data_ptr())
    assert lib.emi_prolong_rows_dev(None, 2, 3, p, p, 1, None, p) == 1
    assert lib.emi_prolong_rows_dev(ev.ctx, 1, 3, p, p, 1, None, p) == 1 and lib.emi_prolong_rows_dev(ev.ctx, 2, 3, None, p, 1, None, p) == 1
    assert lib.emi_prolong_rows_dev(ev.ctx, 2, 3, p, None, 1, None, p) == 1 and lib.emi_prolong_rows_dev(ev.ctx, 2, 3, p, p, -1, None, p) == 1
    assert lib.emi_prolong_rows_dev(ev.ctx, 2, 3, p, p, 0, None, None) == 0                  # no rows: nothing to do
    one, ptr = (C.c_int * 1), (C.c_void_p * 1)

    def move(ctx, n=1, narr=1, rows=2, sld=4, dld=4, length=4, src=p, dst=p, arrays=True):
        return lib.emi_shard_move_dev(ctx, n, None, None, narr, one(rows) if arrays else None, ptr(src.value if src else None), one(sld),
                                      ptr(dst.value if dst else None), one(dld), length)
    assert move(None) == 1 and move(ev.ctx, n=-1) == 1 and move(ev.ctx, narr=0) == 1 and move(ev.ctx, narr=5) == 1
    assert move(ev.ctx, rows=-1) == 1 and move(ev.ctx, sld=3) == 1 and move(ev.ctx, dld=3) == 1 and move(ev.ctx, length=-1) == 1
    assert move(ev.ctx, src=None) == 1 and move(ev.ctx, dst=None) == 1 and move(ev.ctx, arrays=False) == 1
    assert move(ev.ctx, n=0, src=None, dst=None) == 0                                        # an empty list: nothing to do
    ev.close()
    f = E.Evaluator(0, f32=True)
    assert lib.emi_prolong_rows_dev(f.ctx, 2, 3, p, p, 1, None, p) == 5 and move(f.ctx) == 5       # EMI_ERR_UNSUPPORTED
    f.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def refine(ev, tf, insts, ladder, options, tol, first_check=RR.FIRST_CHECK, dev=True, ldm=None, per_rung=None, replicate=False, recs=False,
           clip=True):
    """one call from the instances' starts (on ladder[0] nodes) into NaN-filled arrays [B][rows][ldm] -> dict X U LamF LamC (numpy),
    res[rung][b], err [rungs][B], out[b], the tensors.  per_rung: {rung: options that replace `options` there}; replicate: bounds
    given per instance; recs: every rung brings the context's table."""
    import torch
    B = len(insts)
    ldm = ldm or max(ladder)
    z0 = np.stack([i["z0"] for i in insts]).reshape(B, NV, ladder[0])
    X0, U0 = np.ascontiguousarray(z0[:, :NS]), np.ascontiguousarray(z0[:, NS:])
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)) if dev else (lambda a: np.ascontiguousarray(a).copy())
    rungs = []
    for r, M in enumerate(ladder):
        bd = TG.bounds_at(tf, M, lambda a: a)
        if replicate:
            bd["zl"], bd["zu"] = np.repeat(bd["zl"], B, 0), np.repeat(bd["zu"], B, 0)
        bd["zl"], bd["zu"] = up(bd["zl"]), up(bd["zu"])
        rungs.append(dict(M=M, bounds=bd, options=dict((per_rung or {}).get(r, options)), repair=0,
                          recs=np.stack([LR.records(i["discs"]) for i in insts]) if recs else None))
    out = tuple(up(np.full((B, r, ldm), np.nan)) for r in ROWS)
    X0d, U0d = up(X0), up(U0)
    if dev:
        torch.cuda.synchronize()
    X, U, LamF, LamC, res, err, summ = ev.ipm_solve_refine(rungs, 0.0, tf, X0d, U0d, tol, first_check, RR.UL if clip else None,
                                                           RR.UU if clip else None, out=out, dev=dev)
    if dev:
        ev.synchronize()
        assert np.array_equal(X0d.cpu().numpy(), X0) and np.array_equal(U0d.cpu().numpy(), U0)        # the starts are only read
        X, U, LamF, LamC = (t.cpu().numpy() for t in (X, U, LamF, LamC))
    else:
        assert np.array_equal(X0d, X0) and np.array_equal(U0d, U0)
    return dict(X=X, U=U, LamF=LamF, LamC=LamC, res=res, err=err, out=summ, rungs=rungs, ladder=tuple(ladder))


def same_run(a, b):
    return all(same(a[k], b[k]) for k in KEYS) and a["res"] == b["res"] and same(a["err"], b["err"]) and repr(a["out"]) == repr(b["out"])


def padding_is_kept(r):
    """instance b holds M_rung finite values per row, the columns beyond are the NaN the arrays came with"""
    for b, q in enumerate(r["out"]):
        M = r["ladder"][q["rung"]]
        for k in KEYS:
            if not (np.isfinite(r[k][b, :, :M]).all() and np.isnan(r[k][b, :, M:]).all()):
                return False
    return True


def test_with_a_zero_tolerance_it_is_the_ladder(built):
    tf = LR.TFS[0]
    insts = LD.instances(tf)
    ev = TG.fresh_ev(tf, insts)
    want = TG.climb(ev, tf, insts, LD.LADDER, dict(tol=TOL))
    got = refine(ev, tf, insts, LD.LADDER, dict(tol=TOL), 0.0, first_check=0, ldm=LD.LADDER[-1] + 3)
    assert ev.layout.M == LD.LADDER[-1] and ev.layout.B == len(insts)
    ev.close()
    for k in KEYS:
        assert same(got[k][:, :, :LD.LADDER[-1]], want[k]), k
    assert got["res"] == want["res"] and padding_is_kept(got)
    assert all(q["rung"] == 1 and q["verdict"] == RR.NOT_MET and q["rungs_solved"] == 2 for q in got["out"]), got["out"]
    assert np.isfinite(got["err"]).all() and (got["err"] > 0).all()
    assert [q["err"] for q in got["out"]] == list(got["err"][1])


def test_with_an_infinite_tolerance_it_is_the_first_rung(built):
    import torch
    tf, M0 = LR.TFS[0], LD.LADDER[0]
    insts = LD.instances(tf)
    ev = TG.fresh_ev(tf, insts)
    got = refine(ev, tf, insts, LD.LADDER, dict(tol=TOL), float("inf"), first_check=0)
    assert ev.layout.M == M0 and ev.layout.B == len(insts)                # the last rung that was solved
    z0 = np.stack([i["z0"] for i in insts]).reshape(len(insts), NV, M0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
    X, U = up(z0[:, :NS]), up(z0[:, NS:])
    torch.cuda.synchronize()
    LamF, LamC, res = ev.ipm_solve_shard(X, U, TG.bounds_at(tf, M0, up), dict(tol=TOL))
    ev.synchronize()
    ev.close()
    for k, t in zip(KEYS, (X, U, LamF, LamC)):
        assert same(got[k][:, :, :M0], t.cpu().numpy()), k
    assert got["res"][0] == res and all(q["status"] == -1 and q["iterations"] == 0 for q in got["res"][1]) and np.isnan(got["err"][1]).all()
    assert all(q["rung"] == 0 and q["rungs_solved"] == 1 and q["verdict"] == (RR.MET if s["status"] in OK else RR.FAILED)
               for q, s in zip(got["out"], res)), got["out"]
    assert padding_is_kept(got)


@pytest.fixture(scope="module")
def split_runs(built):
    out, evs = {}, []
    for tf in LR.TFS:
        insts = LD.instances(tf)
        ev = TG.fresh_ev(tf, insts)
        evs.append(ev)
        out[tf] = dict(insts=insts, ev=ev, first=refine(ev, tf, insts, RR.LADDER, dict(tol=TOL), RR.TOLS[tf]))
    yield out
    for ev in evs:
        ev.close()


def group_ev(tf, insts, M):
    ev = TG.fresh_ev(tf, insts)
    ev.set_mesh(M, 0.0, tf)
    return ev


@pytest.mark.parametrize("tf", LR.TFS)
def test_the_split_is_the_fixtures(split_runs, tf):
    import torch
    import indep_nlp as N
    a = split_runs[tf]
    r, insts, tol = a["first"], a["insts"], RR.TOLS[tf]
    fx = RR.fixture()
    cpu = fx["cases"][str(tf)]
    B, nr = len(insts), len(RR.LADDER)
    for b in range(B):
        q = r["out"][b]
        print(f"tf {tf} instance {b}: rung {q['rung']} verdict {q['verdict']} solved {q['rungs_solved']} err {q['err']:.3e} (CPU climb: rung {cpu[b]['rung']} "
              f"verdict {cpu[b]['verdict']}); per rung status / iterations / err " +
              " ".join(f"[{s['status']} {s['iterations']} {e:.3e} | CPU {c['iterations']} {c['err']:.3e}]" for s, e, c in
                       zip((r["res"][g][b] for g in range(nr)), r["err"][:, b], cpu[b]["rungs"])))
    # rung and verdict, and the cost there
    for b in range(B):
        q = r["out"][b]
        assert (q["rung"], q["verdict"], q["rungs_solved"]) == (cpu[b]["rung"], cpu[b]["verdict"], cpu[b]["rungs_solved"]), (tf, b, q)
        mine, theirs = r["res"][q["rung"]][b]["cost"], cpu[b]["rungs"][q["rung"]]["cost"]
        assert abs(mine - theirs) <= 1e-6 * abs(theirs), (tf, b, mine, theirs)
    split = {g: sum(q["rung"] == g for q in r["out"]) for g in range(nr) if any(q["rung"] == g for q in r["out"])}
    assert split == RR.SPLIT[tf], split
    # every decision follows from what the call returned
    for b in range(B):
        solved = r["out"][b]["rungs_solved"]
        oks = [r["res"][g][b]["status"] in OK for g in range(solved)]
        assert all(r["res"][g][b]["status"] == -1 and np.isnan(r["err"][g, b]) for g in range(solved, nr)), (tf, b)
        assert np.isnan(r["err"][:RR.FIRST_CHECK, b]).all() and np.isfinite(r["err"][RR.FIRST_CHECK:solved, b]).all(), (tf, b)
        rung, verdict, n, _ = RR.walk(oks, list(r["err"][:solved, b]), tol)
        assert (rung, verdict, n) == (r["out"][b]["rung"], r["out"][b]["verdict"], solved), (tf, b)
        assert same(np.float64(r["out"][b]["err"]), r["err"][rung, b])
    assert padding_is_kept(r)
    # per retiring rung: the certificate of the group's gathered arrays, and the estimate against the restatement
    shown = set()
    for g, M in enumerate(RR.LADDER):
        grp = [b for b in range(B) if r["out"][b]["rung"] == g]
        if not grp:
            continue
        ev = group_ev(tf, [insts[b] for b in grp], M)
        kw = dict(dtype=torch.float64, device=ev.device)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(ev.device)
        X, U, LamF, LamC = (up(r[k][grp][:, :, :M]) for k in KEYS)
        bd = TG.bounds_at(tf, M, up)
        RES, VALS, COST = torch.zeros((len(grp), NS + NP, M), **kw), torch.zeros((len(grp), ev.layout.nvals, M), **kw), torch.zeros(len(grp), **kw)
        cert = torch.zeros((len(grp), 6), **kw)
        torch.cuda.synchronize()
        ev.eval_dev(X, U, RES, VALS, COST)
        ev.kkt_certificate_dev(X, U, RES, VALS, LamF, LamC, 1.0, bd["zl"], bd["zu"], LR.CL, LR.CU, cert)
        # where the polish starts: the group on its own mesh, solved on to 1e-10 from what the call returned
        Xf, Uf = X.clone(), U.clone()
        _, _, fine = ev.ipm_solve_shard(Xf, Uf, bd, dict(tol=TOL_FINE, max_iter=120, mu_init=1e-4))
        ev.synchronize()
        ev.close()
        cert, cost, Xf, Uf = cert.cpu().numpy(), COST.cpu().numpy(), Xf.cpu().numpy(), Uf.cpu().numpy()
        ref = RR.ode_err(tf, M, r["X"][grp][:, :, :M], r["U"][grp][:, :, :M], dtype=OE.LD)
        bound = OE.err_bound(ref, M)
        for i, b in enumerate(grp):
            got = r["err"][g, b]
            print(f"  rung {M} instance {b}: defect {cert[i, 2]:.2e} viol {cert[i, 3]:.2e}; err {got:.6e} restated {float(ref['err'][i]):.6e} "
                  f"difference / bound {abs(got - float(ref['err'][i])) / bound[i]:.3f}")
            assert cert[i, 2] <= TOL and cert[i, 3] <= TOL, (tf, b)
            assert cost[i] == r["res"][g][b]["cost"], (tf, b)
            assert abs(np.longdouble(got) - ref["err"][i]) <= bound[i], (tf, b)
        # one instance of the group against the polish from its solve to 1e-10
        b = grp[0]
        print(f"  rung {M} instance {b} solved on to {TOL_FINE:g}: status {fine[0]['status']} iterations {fine[0]['iterations']} kkt {fine[0]['kkt_error']:.2e}")
        P = LD.quad_at(tf, M, insts[b]["discs"])
        z, _, _, k = N.polish(P, np.concatenate([Xf[0].ravel(), Uf[0].ravel()]))
        assert N.kkt_ok(k), (tf, b, k)
        Xs, Us = P.split(z)[0][0], P.split(z)[1][0]
        ex = np.abs(r["X"][b, :, :M] - Xs).max() / np.abs(Xs).max()
        eu = np.abs(r["U"][b, :, :M] - Us).max() / np.abs(Us).max()
        print(f"  rung {M} instance {b}: cost {r['res'][g][b]['cost']:.9f} polished {P.cost(z):.9f}; rel err states {ex:.2e} controls {eu:.2e}")
        assert ex < 1e-6 and eu < 1e-6, (tf, b, ex, eu)
        shown.add(g)
    assert shown == set(RR.SPLIT[tf])
    for g, M in enumerate(RR.LADDER):
        who = [b for b in range(B) if r["res"][g][b]["status"] != -1]
        mine, theirs = sum(r["res"][g][b]["iterations"] for b in who), sum(cpu[b]["rungs"][g]["iterations"] for b in who)
        print(f"tf {tf} rung {M}: {len(who)} instances, {mine} iterations, CPU climb {theirs}")
        assert mine <= 1.5 * theirs, (tf, M, mine, theirs)


def test_a_failed_refinement_solve_falls_back(split_runs):
    tf = LR.TFS[0]
    a = split_runs[tf]
    ev, insts, tol = a["ev"], a["insts"], RR.TOLS[tf]
    r = refine(ev, tf, insts, RR.LADDER, dict(tol=TOL), tol, per_rung={2: dict(tol=TOL, max_iter=3)})
    assert ev.layout.M == RR.LADDER[2] and ev.layout.B == len(insts)          # the last rung that was solved
    short = refine(ev, tf, insts, RR.LADDER[:2], dict(tol=TOL), tol, ldm=RR.LADDER[-1])
    reached = [b for b in range(len(insts)) if r["res"][2][b]["status"] != -1]
    assert len(reached) == RR.SPLIT[tf][3]
    for b, q in enumerate(r["out"]):
        if b in reached:
            assert r["res"][2][b]["status"] == LR.MAX_ITER and r["res"][3][b]["status"] == -1
            assert (q["rung"], q["verdict"], q["rungs_solved"]) == (1, RR.FELL_BACK, 3), q
            assert short["out"][b]["verdict"] == RR.NOT_MET and short["out"][b]["rung"] == 1
            assert same(np.float64(q["err"]), r["err"][1, b]) and np.isfinite(r["err"][2, b])
        else:
            assert (q["rung"], q["verdict"]) == (1, RR.MET) and q == short["out"][b]
    for k in KEYS:
        assert same(r[k], short[k]), k
    assert padding_is_kept(r)


def test_an_instance_without_a_feasible_path_fails_alone(split_runs):
    tf = LR.TFS[0]
    a = split_runs[tf]
    tol, opt = RR.TOLS[tf], dict(tol=TOL, max_iter=100, rules=1)           # the rule ends the blocked instance after 70 - 80 iterations
    blocked = dict(discs=LR.discs_of(LR.NO_PATH_DISC), bump=0.0, z0=a["insts"][0]["z0"])
    three, two = [a["insts"][2], blocked, a["insts"][5]], [a["insts"][2], a["insts"][5]]
    ev = TG.fresh_ev(tf, three)
    r = refine(ev, tf, three, RR.LADDER, opt, tol)
    ev.close()
    ev = TG.fresh_ev(tf, two)
    w = refine(ev, tf, two, RR.LADDER, opt, tol)
    ev.close()
    print("with the blocked instance:", r["out"], [[q["status"] for q in g] for g in r["res"]])
    print("without:", w["out"])
    bad = r["out"][1]
    assert (bad["rung"], bad["verdict"], bad["rungs_solved"]) == (RR.FIRST_CHECK, RR.FAILED, RR.FIRST_CHECK + 1), bad
    assert r["res"][RR.FIRST_CHECK][1]["status"] not in OK and r["res"][2][1]["status"] == -1
    for i, j in ((0, 0), (2, 1)):
        p, q = r["out"][i], w["out"][j]
        assert (p["rung"], p["verdict"], p["rungs_solved"]) == (q["rung"], q["verdict"], q["rungs_solved"]) and p["verdict"] == RR.MET, (p, q)
        M = RR.LADDER[p["rung"]]
        for k in ("X", "U"):
            d = np.abs(r[k][i, :, :M] - w[k][j, :, :M]).max() / np.abs(w[k][j, :, :M]).max()
            assert d < 1e-6, (i, k, d)
    assert {r["out"][0]["rung"], r["out"][2]["rung"]} == {1, 3}               # one neighbour climbs on after the failure
    assert padding_is_kept(r)


def test_bounds_per_instance_and_tables_per_rung_change_no_bit(split_runs):
    tf = LR.TFS[0]
    a = split_runs[tf]
    r = refine(a["ev"], tf, a["insts"], RR.LADDER, dict(tol=TOL), RR.TOLS[tf], replicate=True, recs=True)
    assert same_run(r, a["first"])


def test_two_calls_the_host_form_and_the_context_afterwards(split_runs):
    tf = LR.TFS[0]
    a = split_runs[tf]
    ev, insts, tol = a["ev"], a["insts"], RR.TOLS[tf]
    again = refine(ev, tf, insts, RR.LADDER, dict(tol=TOL), tol)
    assert same_run(again, a["first"])
    host = refine(ev, tf, insts, RR.LADDER, dict(tol=TOL), tol, dev=False)
    assert same_run(host, a["first"])
    # batch, mesh and table of the context: the last solved rung, all B instances, every instance's own records
    assert ev.layout.M == RR.LADDER[-1] and ev.layout.B == len(insts) and ev.layout.np == NP
    ev.set_mesh(TL.M, 0.0, tf)
    at41 = LR.instances(tf)
    after = TL.solve(ev, tf, at41, dict(tol=TOL, max_iter=200))
    fresh = TL.make_ev(tf, at41)
    want = TL.solve(fresh, tf, at41, dict(tol=TOL, max_iter=200))
    fresh.close()
    assert TL.same_bits(after, want) and after["res"] == want["res"]


def test_an_instance_that_climbs_in_a_compacted_batch_agrees_with_itself_alone(split_runs):
    tf = LR.TFS[0]
    a = split_runs[tf]
    b = next(b for b, q in enumerate(a["first"]["out"]) if q["rung"] == 3)
    ev = TG.fresh_ev(tf, [a["insts"][b]])
    one = refine(ev, tf, [a["insts"][b]], RR.LADDER, dict(tol=TOL), RR.TOLS[tf])
    ev.close()
    p, q = one["out"][0], a["first"]["out"][b]
    assert (p["rung"], p["verdict"], p["rungs_solved"]) == (q["rung"], q["verdict"], q["rungs_solved"])
    M = RR.LADDER[q["rung"]]
    dx = np.abs(one["X"][0, :, :M] - a["first"]["X"][b, :, :M]).max() / np.abs(one["X"][0, :, :M]).max()
    du = np.abs(one["U"][0, :, :M] - a["first"]["U"][b, :, :M]).max() / np.abs(one["U"][0, :, :M]).max()
    print(f"instance {b}: alone {[g[0]['iterations'] for g in one['res']]} iterations, in the batch "
          f"{[g[b]['iterations'] for g in a['first']['res']]}; {dx:.2e} {du:.2e}")
    assert dx < 1e-6 and du < 1e-6


def test_refine_statuses(built):
    import torch
    import etol_amd as E
    from etol_amd import _lib as L
    lib = E.load()
    tf = LR.TFS[0]
    insts = LD.instances(tf)[:2]
    M0, M1 = LD.LADDER

    def call(ev, nrungs=2, drop=None, tol=1e-3, first_check=1, ldm=M1, rf=True, err=True, out=True, ul=True, uu=True, nsets=1):
        dev = ev.device
        new = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        keep = [new(2, NS, M0), new(2, NC, M0), new(2, NS, M1), new(2, NC, M1), new(2, NS, M1), new(2, NP, M1)]
        arr = (L.IpmRung * 2)()
        for g, M in zip(arr, LD.LADDER):
            bd = TG.bounds_at(tf, M, lambda x: torch.from_numpy(np.ascontiguousarray(np.repeat(x, 3, 0)).copy()).to(dev))
            keep += [bd["zl"], bd["zu"]]
            g.M, g.bd.zl, g.bd.zu, g.bd.nsets = M, p(bd["zl"]), p(bd["zu"]), nsets
            g.bd.cl, g.bd.cu = LR.CL.ctypes.data_as(LD.D_), LR.CU.ctypes.data_as(LD.D_)
            g.opt.max_iter = 2
        args = [p(t) for t in keep[:6]]
        if drop is not None:
            args[drop] = None
        r = L.IpmRefine()
        r.ode_tol, r.first_check = tol, first_check
        if ul:
            r.ul = RR.UL.ctypes.data_as(LD.D_)
        if uu:
            r.uu = RR.UU.ctypes.data_as(LD.D_)
        res, e, o = (L.IpmResult * 4)(), np.zeros(4), (L.IpmRefineResult * 2)()
        torch.cuda.synchronize()
        st = lib.emi_ipm_solve_refine_dev(ev.ctx, nrungs, arr, 0.0, tf, C.byref(r) if rf else None, args[0], args[1], ldm, *args[2:], res,
                                          e.ctypes.data_as(LD.D_) if err else None, o if out else None)
        ev.synchronize()
        return st

    ev = TG.fresh_ev(tf, insts, f32=True)
    assert call(ev) == 5                                        # EMI_ERR_UNSUPPORTED: f32 context
    ev.close()
    ev = TG.fresh_ev(tf, insts)
    track = np.stack([LR.records(i["discs"]) for i in insts])
    track[1, 0, :3] = [2, 0, 0.25]
    ev.set_path(track, 0, 1)
    assert call(ev) == 5                                        # the context's table with a track row
    ev.set_path(np.stack([LR.records(i["discs"]) for i in insts]), 0, 1)
    assert call(ev, nrungs=0) == 1                              # EMI_ERR_ARG from here on
    for drop in range(6):
        assert call(ev, drop=drop) == 1, drop                   # a NULL that is not optional (dX0 first)
    assert call(ev, rf=False) == 1 and call(ev, err=False) == 1 and call(ev, out=False) == 1
    assert call(ev, tol=-1e-9) == 1 and call(ev, tol=float("nan")) == 1
    assert call(ev, first_check=2) == 1 and call(ev, first_check=-1) == 1
    assert call(ev, ldm=M1 - 1) == 1 and call(ev, ul=False) == 1 and call(ev, uu=False) == 1
    assert call(ev, nsets=3) == 1 and call(ev, nsets=0) == 1
    ev.set_option("kkt_method", 0)
    assert call(ev) == 5
    ev.set_option("kkt_method", 1)
    lay = L.Layout()                                            # (asked of the library: the evaluator caches its own)
    assert lib.emi_get_layout(ev.ctx, C.byref(lay)) == 0 and (lay.B, lay.M) == (2, 9)        # a refused call leaves the context as it was
    assert call(ev) == 0 and lib.emi_get_layout(ev.ctx, C.byref(lay)) == 0 and (lay.B, lay.M, lay.np) == (2, M1, NP)
    assert call(ev, nsets=2, ul=False, uu=False, tol=0.0, first_check=0, ldm=M1 + 5) == 0
    ev.close()
    ev = E.Evaluator(0)
    assert call(ev) == 2                                        # EMI_ERR_STATE: no model, no batch
    ev.close()
    assert lib.emi_ipm_solve_refine_dev(None, 0, None, 0.0, 1.0, None, None, None, 0, None, None, None, None, None, None, None) == 1
