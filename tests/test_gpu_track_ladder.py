"""Rows of kind EMI_PATH_TRACK in emi_ipm_solve_ladder_dev and emi_ipm_solve_refine_dev: the centres of the moving discs made per
rung on the device from the waypoint tables of emi_set_track_waypoints.  -m gpu

References: tests/track_ladder_ref.py.  The instances are those of tests/ladder_ref.py with their first disc turned into a track
row, at rest or moving.  A ladder of one rung is held to emi_ipm_solve_shard_dev after emi_set_tracks with the host centres, and
the ladder (21, 41) to the chain of public calls with the host centres, bit for bit.  The criteria of tests/test_gpu_ladder.py are
restated, not relaxed: cost within 1e-6 relative of the fixture (tests/golden/ladder_cases.json for the tracks at rest,
tests/golden/track_ladder_cases.json for the moving ones), the certificate's defect and violation within the solve's tolerance,
iteration sums per rung within 1.5 x the CPU climb's.  The refinement is held to tests/golden/refine_cases.json: with one waypoint
set per instance the live list is the set map of the launch, which is what compacts the centres."""
import numpy as np
import pytest

import ladder_ref as LD
import lockstep_ref as LR
import oracle_lib as O
import refine_ref as RR
import test_gpu_ladder as TG
import test_gpu_lockstep as TL
import test_gpu_refine as TGR
import track_ladder_ref as TR

pytestmark = pytest.mark.gpu

TOL = TL.TOL
NV, NS, NC, NP = TL.NV, TL.NS, TL.NC, TL.NP
M0, M1 = LD.LADDER
TF = TR.TF
OK = (LR.CONVERGED, LR.ACCEPTABLE)
KEYS = ("X", "U", "LamF", "LamC")
bits = TG.bits


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def track_ev(insts, waypoints="per_instance", M=9):
    """a context on some other mesh (the ladder brings its own) with model, batch, the instances' tables (first row: a track) and
    their waypoints: one set per instance, one shared set (the first instance's), or none"""
    import etol_amd as E
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, 1.0)
    ev.set_model(1, LR.QUAD_PARAMS)
    ev.set_batch(len(insts))
    ev.set_path(np.stack([i["recs"] for i in insts]), 0, 1)
    if waypoints == "per_instance":
        ev.set_track_waypoints(*TR.stacked([i["way"] for i in insts]))
    elif waypoints == "shared":
        ev.set_track_waypoints(*TR.stacked([insts[0]["way"]]))
    return ev


def centres(insts, M):
    return TR.host_centres([i["way"] for i in insts], M, 0.0, TF)


def shard(ev, insts, M, X, U, options):
    """emi_ipm_solve_shard_dev on the context's mesh from X, U (device tensors, in place) -> dict like test_gpu_ladder.climb's"""
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
    bd = TG.bounds_at(TF, M, up)
    torch.cuda.synchronize()
    LamF, LamC, res = ev.ipm_solve_shard(X, U, bd, options)
    ev.synchronize()
    return dict(X=X.cpu().numpy(), U=U.cpu().numpy(), LamF=LamF.cpu().numpy(), LamC=LamC.cpu().numpy(), res=res)


def starts(ev, insts, M):
    import torch
    z0 = np.stack([i["z0"] for i in insts]).reshape(len(insts), NV, M)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
    return up(z0[:, :NS]), up(z0[:, NS:])


def chain(ev, insts, options, repair):
    """the ladder (21, 41) as a chain of public calls with the centres from the host: shard solve on 21, emi_prolong_dev with
    emi_prolong_matrix, emi_set_mesh 41, emi_set_tracks, emi_repair_guess_dev where asked, shard solve"""
    import torch
    ev.set_mesh(M0, 0.0, TF)
    ev.set_tracks(*centres(insts, M0))
    X, U = starts(ev, insts, M0)
    if repair:
        ev.repair_guess(X)
    first = shard(ev, insts, M0, X, U, options)
    PT = torch.from_numpy(np.ascontiguousarray(ev.prolong_matrix(M0, M1).T)).to(ev.device)
    torch.cuda.synchronize()
    Xf, Uf = ev.prolong(PT, X), ev.prolong(PT, U)
    ev.set_mesh(M1, 0.0, TF)
    ev.set_tracks(*centres(insts, M1))
    if repair:
        ev.repair_guess(Xf)
    last = shard(ev, insts, M1, Xf, Uf, options)
    return dict(last, res=[first["res"], last["res"]])


# ---- 1. one rung ---------------------------------------------------------------------------------------------------------------------
def test_one_rung_is_the_shard_solve_with_the_host_centres(built):
    insts = TR.moving_instances()
    opt = dict(tol=TOL, max_iter=200)
    ev = track_ev(insts, waypoints=None)
    ev.set_mesh(M0, 0.0, TF)
    ev.set_tracks(*centres(insts, M0))
    X, U = starts(ev, insts, M0)
    want = shard(ev, insts, M0, X, U, opt)
    ev.close()
    ev = track_ev(insts)
    got = TG.climb(ev, TF, insts, (M0,), opt)
    assert ev.layout.M == M0
    xc, yc = ev.get_tracks()
    ev.close()
    assert all(same(got[k], want[k]) for k in KEYS) and got["res"] == [want["res"]], (want["res"], got["res"])
    assert all(q["status"] in OK for q in want["res"])
    wx, wy = centres(insts, M0)
    assert same(xc, wx) and same(yc, wy)
    assert np.ptp(wx, axis=2).min() > 0                                  # (the discs do move)


# ---- 2. two rungs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repair", (0, 1))
def test_two_rungs_are_the_chain_of_public_calls(built, repair):
    insts = TR.moving_instances()
    opt = dict(tol=TOL, max_iter=200)
    ev = track_ev(insts)
    got = TG.climb(ev, TF, insts, LD.LADDER, opt, repair=repair)
    ev.close()
    ev = track_ev(insts, waypoints=None)
    want = chain(ev, insts, opt, repair)
    ev.close()
    for k in KEYS:
        diff = float(np.abs(got[k] - want[k]).max() / max(np.abs(want[k]).max(), 1e-300))
        assert same(got[k], want[k]), (repair, k, diff)
    assert got["res"] == want["res"], (got["res"], want["res"])
    if repair:                                                              # the repair did read the centres: it moved something
        X0 = np.stack([i["z0"] for i in insts]).reshape(len(insts), NV, M0)[:, :NS]
        moved, _ = LD.repair_ref(X0, np.stack([i["recs"] for i in insts]), tracks=centres(insts, M0))
        assert not np.array_equal(moved, X0)


# ---- 3. a track that does not move -------------------------------------------------------------------------------------------------------
def certificate(ev, r, B, M):
    """(cert [B][6], cost [B]) of what a ladder call returned, on the context it left"""
    import torch
    kw = dict(dtype=torch.float64, device=ev.device)
    RES, VALS, COST = torch.zeros((B, NS + NP, M), **kw), torch.zeros((B, ev.layout.nvals, M), **kw), torch.zeros(B, **kw)
    cert = torch.zeros((B, 6), **kw)
    torch.cuda.synchronize()
    assert ev.layout.M == M
    ev.eval_dev(r["tX"], r["tU"], RES, VALS, COST)
    ev.kkt_certificate_dev(r["tX"], r["tU"], RES, VALS, r["tLamF"], r["tLamC"], 1.0, r["tzl"], r["tzu"], LR.CL, LR.CU, cert)
    ev.synchronize()
    return cert.cpu().numpy(), COST.cpu().numpy()


def meets_the_ladder_criteria(tag, ev, r, cpu_rungs):
    """cpu_rungs[b][g]: the CPU climb's row of instance b on rung g"""
    res = r["res"]
    B = len(res[-1])
    for g, M in enumerate(LD.LADDER):
        for b in range(B):
            q = res[g][b]
            print(f"{tag} rung {M} instance {b}: status {q['status']} iterations {q['iterations']} (CPU {cpu_rungs[b][g]['iterations']}) "
                  f"kkt {q['kkt_error']:.2e} viol {q['constr_viol']:.2e} cost {q['cost']:.9f} (CPU {cpu_rungs[b][g]['cost']:.9f})")
            assert q["status"] in OK, (tag, M, b, q)                     # every instance converges on every rung
    cert, cost = certificate(ev, r, B, M1)
    for b in range(B):
        print(f"  certificate {b}: stat {cert[b, 0]:.2e} comp {cert[b, 1]:.2e} defect {cert[b, 2]:.2e} viol {cert[b, 3]:.2e}")
        assert cert[b, 2] <= TOL and cert[b, 3] <= TOL, (tag, b)
        assert cost[b] == res[-1][b]["cost"], (tag, b)
        theirs = cpu_rungs[b][-1]["cost"]
        assert abs(res[-1][b]["cost"] - theirs) <= 1e-6 * abs(theirs), (tag, b, res[-1][b]["cost"], theirs)
    for g, M in enumerate(LD.LADDER):
        mine, theirs = sum(q["iterations"] for q in res[g]), sum(c[g]["iterations"] for c in cpu_rungs)
        print(f"{tag} rung {M}: {mine} iterations over the batch, CPU climb {theirs}")
        assert mine <= 1.5 * theirs, (tag, M, mine, theirs)


def test_a_track_at_rest_reaches_the_discs_optima(built):
    insts = TR.static_instances(TF)
    cpu = LD.ladder_fixture()["cases"][str(TF)]
    assert len(insts) == len(cpu) == 9
    ev = track_ev(insts)
    r = TG.climb(ev, TF, insts, LD.LADDER, dict(tol=TOL))
    meets_the_ladder_criteria("at rest", ev, r, [c["rungs"] for c in cpu])
    ev.close()


# ---- 4. a track that moves ----------------------------------------------------------------------------------------------------------------
def test_a_moving_track_reaches_the_fixtures_optima(built):
    fx = TR.fixture()
    insts = TR.moving_instances()
    assert fx["displacement"] == TR.DISPLACEMENT and len(fx["cases"]) == len(insts)
    ev = track_ev(insts)
    r = TG.climb(ev, TF, insts, LD.LADDER, dict(tol=TOL))
    meets_the_ladder_criteria("moving", ev, r, [c["rungs"] for c in fx["cases"]])
    xc, yc = ev.get_tracks()
    ev.close()
    tracks = centres(insts, M1)
    assert same(xc, tracks[0]) and same(yc, tracks[1])                      # the context holds the centres of the last rung's mesh
    RES = O.evaluate(1, LR.QUAD_PARAMS, M1, O.lgl(M1), 0.0, TF, r["X"], r["U"], recs=np.stack([i["recs"] for i in insts]), tracks=tracks)[0]
    print(f"oracle with the host centres: largest |defect| {np.abs(RES[:, :NS]).max():.2e}, largest keep-out row {RES[:, NS:].max():.2e}, "
          f"track row per instance {RES[:, NS].max(1)}")
    assert np.abs(RES[:, :NS]).max() <= 1e-6 and RES[:, NS:].max() <= 1e-6
    for b, i in enumerate(insts):
        assert -RES[b, NS].max() < 1e-6 * i["discs"][0][2] ** 2, b         # ... on which the moving disc is active, as in the fixture


# ---- 5. refinement ------------------------------------------------------------------------------------------------------------------------
def test_the_refinement_compacts_the_centres_through_the_set_map(built):
    tol = RR.TOLS[TF]
    insts = TR.static_instances(TF)
    cpu = RR.fixture()["cases"][str(TF)]
    B = len(insts)
    ev = track_ev(insts)
    r = TGR.refine(ev, TF, insts, RR.LADDER, dict(tol=TOL), tol, first_check=1)
    Mlast = ev.layout.M
    assert ev.layout.B == B
    xc, yc = ev.get_tracks()                                                # all B sets again, on the mesh the context is on
    wx, wy = TR.host_centres([i["way"] for i in insts], Mlast, 0.0, TF)
    assert same(xc, wx) and same(yc, wy)
    for b in range(B):
        q = r["out"][b]
        print(f"instance {b}: rung {q['rung']} verdict {q['verdict']} solved {q['rungs_solved']} err {q['err']:.3e} (CPU climb: rung {cpu[b]['rung']} "
              f"verdict {cpu[b]['verdict']}) cost {r['res'][q['rung']][b]['cost']:.9f} (CPU {cpu[b]['rungs'][q['rung']]['cost']:.9f})")
    for b in range(B):
        q = r["out"][b]
        assert (q["rung"], q["verdict"], q["rungs_solved"]) == (cpu[b]["rung"], cpu[b]["verdict"], cpu[b]["rungs_solved"]), (b, q)
        mine, theirs = r["res"][q["rung"]][b]["cost"], cpu[b]["rungs"][q["rung"]]["cost"]
        assert abs(mine - theirs) <= 1e-6 * abs(theirs), (b, mine, theirs)
    split = {g: sum(q["rung"] == g for q in r["out"]) for g in range(len(RR.LADDER)) if any(q["rung"] == g for q in r["out"])}
    assert split == RR.SPLIT[TF] == {1: 6, 3: 3}, split
    assert TGR.padding_is_kept(r)
    # a tolerance of zero retires nobody early: the ladder call, bit for bit
    want = TG.climb(ev, TF, insts, LD.LADDER, dict(tol=TOL))
    got = TGR.refine(ev, TF, insts, LD.LADDER, dict(tol=TOL), 0.0, first_check=0, ldm=M1 + 3)
    xc, yc = ev.get_tracks()
    ev.close()
    for k in KEYS:
        assert same(got[k][:, :, :M1], want[k]), k
    assert got["res"] == want["res"]
    wx, wy = TR.host_centres([i["way"] for i in insts], M1, 0.0, TF)
    assert same(xc, wx) and same(yc, wy)


def test_shared_waypoints_are_the_per_instance_form_with_copies(built):
    """three instances with the same (moving) track and different starts, over the refinement's ladder: one waypoint set for all
    against one copy per instance"""
    tol = RR.TOLS[TF]
    every = LD.instances(TF)
    insts = [dict(i, recs=TR.track_records(i["discs"]), way=TR.moving_waypoints(i["discs"], TF, 1.0)) for i in (every[0], every[3], every[6])]
    assert all(i["discs"] == insts[0]["discs"] for i in insts) and len({i["bump"] for i in insts}) == 3
    runs = {}
    for form in ("shared", "per_instance"):
        ev = track_ev(insts, waypoints=form)
        runs[form] = TGR.refine(ev, TF, insts, RR.LADDER, dict(tol=TOL), tol, first_check=1)
        M = ev.layout.M
        xc, yc = ev.get_tracks()
        ev.close()
        wx, wy = TR.host_centres([i["way"] for i in (insts[:1] if form == "shared" else insts)], M, 0.0, TF)
        assert same(xc, wx) and same(yc, wy), form
    print("retiring rungs:", [q["rung"] for q in runs["shared"]["out"]])
    assert TGR.same_run(runs["shared"], runs["per_instance"])


# ---- 6. statuses ----------------------------------------------------------------------------------------------------------------------------
def test_statuses_with_waypoints_held(built):
    import etol_amd as E
    insts = TR.moving_instances()
    B = len(insts)
    opt = dict(tol=TOL, max_iter=2)
    good = np.stack([i["recs"] for i in insts])
    bad = good.copy()
    bad[1, 0, 1] = 1                                                        # track 1 of a table of one track
    ev = track_ev(insts)
    ev.set_path(bad, 0, 1)
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG"):                    # the context's table
        TG.climb(ev, TF, insts, LD.LADDER, opt)
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG"):
        TGR.refine(ev, TF, insts, LD.LADDER, opt, 1e-3)
    ev.set_path(good, 0, 1)

    def with_recs(recs):
        import torch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
        rungs = [dict(M=M, bounds=TG.bounds_at(TF, M, up), options=dict(opt), recs=recs if g == 1 else None) for g, M in enumerate(LD.LADDER)]
        X0, U0 = starts(ev, insts, M0)
        torch.cuda.synchronize()
        try:
            return ev.ipm_solve_ladder(rungs, 0.0, TF, X0, U0)
        finally:
            ev.synchronize()

    with pytest.raises(E.EmiError, match="EMI_ERR_ARG"):                    # a rung's table
        with_recs(bad)
    neg = good.copy()
    neg[2, 0, 1] = -1
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG"):
        with_recs(neg)
    assert len(with_recs(good)[4]) == 2 and ev.layout.M == M1              # (the call does run with the table as it should be)
    ev.set_track_waypoints(*TR.stacked([i["way"] for i in insts[:2]]))      # 2 sets at B = 3
    with pytest.raises(E.EmiError, match="EMI_ERR_ARG"):
        TG.climb(ev, TF, insts, LD.LADDER, opt)
    ev.set_track_waypoints(*TR.stacked([i["way"] for i in insts]))
    assert len(TG.climb(ev, TF, insts, LD.LADDER, opt)["res"]) == 2 and ev.layout.B == B
    ev.close()
