"""emi_prolong_dev, emi_repair_guess_dev, emi_ipm_solve_ladder_dev / _host: the lock-step solve of a context's batch over a mesh
ladder.  -m gpu

References: tests/ladder_ref.py.  The prolongation kernel is held to a long-double product of the same f64 matrix within
(Mc + 1) 2^-53 sum_j |P_qj| |v_j| -- a chain of Mc fused multiply-adds, no margin; the repair kernel to the numpy restatement of
repair_guess bit for bit; a ladder of one rung to emi_ipm_solve_shard_dev bit for bit; the ladder (21, 41) on the 2 x 9 instances of
tests/lockstep_ref.py to the criteria of tests/test_gpu_lockstep.py: statuses, cost within 1e-6 of tests/golden/lockstep_cases.json,
certificate, trajectory within 1e-6 of the KKT point the independent polish reaches from the same ladder run at tol 1e-10, and
iteration sums per rung within 1.5 x those of tests/golden/ladder_cases.json (the CPU ladder, tests/golden/gen_ladder_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import ladder_ref as LD
import lockstep_ref as LR
import test_gpu_lockstep as TL

pytestmark = pytest.mark.gpu

TOL, TOL_FINE = TL.TOL, TL.TOL_FINE
NV, NS, NC, NP = TL.NV, TL.NS, TL.NC, TL.NP
M0, M1 = LD.LADDER


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- 1. prolongation -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain_ev(built):
    import etol_amd as E
    ev = E.Evaluator(0)                     # no mesh, no model, no batch: the call needs none
    yield ev
    ev.close()


@pytest.mark.parametrize("pair", LD.PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_prolongation_kernel(plain_ev, pair):
    import torch
    ev, (mc, mf) = plain_ev, pair
    P = ev.prolong_matrix(mc, mf)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ev.device)
    PT = up(P.T)
    rng = np.random.default_rng(mc * 1000 + mf)
    mid = mc % 2 == 1 and mf % 2 == 1
    for R in (1, 7, 72, 513):
        V = rng.standard_normal((R, mc)) * np.exp(3 * rng.standard_normal((R, 1)))
        if R > 1:
            V[-1] = 3.7                                         # the constant row
        Vd = up(V)
        torch.cuda.synchronize()
        a, b = ev.prolong(PT, Vd), ev.prolong(PT, Vd)
        rows = sorted({0, R // 2, R - 1})
        alone = [ev.prolong(PT, Vd[r:r + 1].contiguous()) for r in rows]
        ev.synchronize()
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(bits(a), bits(b)), (pair, R)                          # two calls
        for r, one in zip(rows, alone):
            assert np.array_equal(bits(a[r]), bits(one.cpu().numpy()[0])), (pair, R, r)        # a row does not depend on R
        assert np.array_equal(bits(a[:, 0]), bits(V[:, 0])) and np.array_equal(bits(a[:, -1]), bits(V[:, -1])), (pair, R)
        if mid:
            assert np.array_equal(bits(a[:, mf // 2]), bits(V[:, mc // 2])), (pair, R)
        want, mag = LD.prolong_ld(P, V)
        ratio = float((np.abs(a.astype(np.longdouble) - want) / ((mc + 1) * 2.0 ** -53 * mag)).max())
        print(f"({mc}, {mf}) R {R}: largest error / bound {ratio:.3f}")
        assert ratio <= 1.0, (pair, R, ratio)
        if R > 1:
            assert np.abs(a[-1] - 3.7).max() <= (mc + 1) * 2.0 ** -53 * 3.7 * np.abs(P).sum(1).max()


def test_prolongation_statuses(plain_ev, built):
    import torch
    import etol_amd as E
    ev, lib = plain_ev, E.load()
    t = torch.zeros(16, dtype=torch.float64, device=ev.device)
    p = C.c_void_p(t.data_ptr())
    assert lib.emi_prolong_dev(None, 2, 3, p, p, 1, p) == 1
    assert lib.emi_prolong_dev(ev.ctx, 1, 3, p, p, 1, p) == 1 and lib.emi_prolong_dev(ev.ctx, 2, 3, None, p, 1, p) == 1
    assert lib.emi_prolong_dev(ev.ctx, 2, 3, p, p, 0, None) == 0                     # no rows: nothing to do
    f = E.Evaluator(0, f32=True)
    assert lib.emi_prolong_dev(f.ctx, 2, 3, p, p, 1, p) == 5                         # EMI_ERR_UNSUPPORTED
    f.close()


# ---- 2. repair ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (9, 41))
@pytest.mark.parametrize("table", ("shared", "per_instance", "track"))
def test_repair_kernel_gives_the_restatements_bits(built, M, table):
    import torch
    import etol_amd as E
    c = LD.repair_case(M, per_instance=table == "per_instance", with_track=table == "track")
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, 4.0)
    ev.set_model(1, LR.QUAD_PARAMS)
    ev.set_batch(c["B"])
    if c["tracks"] is not None:
        assert E.load().emi_set_tracks(ev.ctx, 1, 1, c["tracks"][0].ctypes.data_as(LD.D_), c["tracks"][1].ctypes.data_as(LD.D_)) == 0
    ev.set_path(c["recs"] if c["recs"].shape[0] > 1 else c["recs"][0], 0, 1)
    X = torch.from_numpy(c["X"].copy()).to(ev.device)
    torch.cuda.synchronize()
    ev.repair_guess(X)
    ev.synchronize()
    got = X.cpu().numpy()
    want, sweeps = LD.repair_ref(c["X"], c["recs"], tracks=c["tracks"])
    moved = (want[:, :2] != c["X"][:, :2]).any(1)
    print(f"M {M} {table}: {int(moved.sum())} nodes moved in up to {sweeps} sweeps")
    assert sweeps >= 2 and moved[0, c["kc"]] and moved.sum() >= 3 and not moved.all()
    assert np.array_equal(bits(got), bits(want))
    still = np.broadcast_to(~moved[:, None, :], got.shape)
    assert np.array_equal(bits(got[still]), bits(c["X"][still]))                    # outside already: the same bits
    assert np.array_equal(bits(got[:, :, [0, -1]]), bits(c["X"][:, :, [0, -1]]))      # end nodes, though inside a disc
    d0 = np.hypot(c["X"][:, 0, 0] - 1.0, c["X"][:, 1, 0] - 1.0)
    assert (d0 < 0.6).all()
    ev.close()


def test_repair_statuses(built):
    import torch
    import etol_amd as E
    lib = E.load()
    ev = E.Evaluator(0)
    t = torch.zeros(3 * 6 * 9, dtype=torch.float64, device=ev.device)
    p = C.c_void_p(t.data_ptr())
    assert lib.emi_repair_guess_dev(None, p) == 1 and lib.emi_repair_guess_dev(ev.ctx, p) == 2       # nothing set: EMI_ERR_STATE
    ev.set_mesh(9, 0.0, 4.0)
    ev.set_model(1, LR.QUAD_PARAMS)
    ev.set_batch(3)
    assert lib.emi_repair_guess_dev(ev.ctx, None) == 1
    assert lib.emi_repair_guess_dev(ev.ctx, p) == 0                                # no table: nothing to do
    ev.set_path(np.array([[2, 0, 0.16, 0, 0, 0, 0, 0]], dtype=float), 0, 1)
    assert lib.emi_repair_guess_dev(ev.ctx, p) == 2                                # a track row and no tracks
    ev.close()
    f = E.Evaluator(0, f32=True)
    assert lib.emi_repair_guess_dev(f.ctx, p) == 5
    f.close()


# ---- 3 - 6. the ladder ------------------------------------------------------------------------------------------------------------------
def bounds_at(tf, M, up):
    P = LD.quad_at(tf, M, LR.discs_of(LR.FIRST_DISCS[0]))
    return dict(zl=up(P.lo.reshape(1, NV, M)), zu=up(P.up.reshape(1, NV, M)), cl=LR.CL, cu=LR.CU, cscale=LR.CSCALE)


def fresh_ev(tf, insts, M=9, f32=False):
    """mesh (emi_set_batch wants one; not one of the ladder's, which sets its own), model, batch and table"""
    import etol_amd as E
    ev = E.Evaluator(0, f32=f32)
    ev.set_mesh(M, 0.0, 1.0)
    ev.set_model(1, LR.QUAD_PARAMS)
    ev.set_batch(len(insts))
    ev.set_path(np.stack([LR.records(i["discs"]) for i in insts]), 0, 1)
    return ev


def climb(ev, tf, insts, ladder, options, dev=True, repair=0):
    """one ladder call from the instances' starts (on ladder[0] nodes) -> dict X U LamF LamC (numpy), res[rung][b], the tensors"""
    import torch
    z0 = np.stack([i["z0"] for i in insts]).reshape(len(insts), NV, ladder[0])
    X0, U0 = np.ascontiguousarray(z0[:, :NS]), np.ascontiguousarray(z0[:, NS:])
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)) if dev else (lambda a: np.ascontiguousarray(a).copy())
    rungs = [dict(M=M, bounds=bounds_at(tf, M, up), options=dict(options), repair=repair) for M in ladder]
    X0d, U0d = up(X0), up(U0)
    if dev:
        torch.cuda.synchronize()
    X, U, LamF, LamC, res = ev.ipm_solve_ladder(rungs, 0.0, tf, X0d, U0d, dev=dev)
    keep = dict(tX=X, tU=U, tLamF=LamF, tLamC=LamC, tzl=rungs[-1]["bounds"]["zl"], tzu=rungs[-1]["bounds"]["zu"], rungs=rungs)
    if dev:
        ev.synchronize()
        assert np.array_equal(X0d.cpu().numpy(), X0) and np.array_equal(U0d.cpu().numpy(), U0)        # read only
        X, U, LamF, LamC = (t.cpu().numpy() for t in (X, U, LamF, LamC))
    return dict(X=X, U=U, LamF=LamF, LamC=LamC, res=res, **keep)


def test_one_rung_is_the_existing_call(built):
    tf = LR.TFS[0]
    insts = LR.instances(tf)
    opt = dict(tol=TOL, max_iter=200)
    ev = TL.make_ev(tf, insts)
    want = TL.solve(ev, tf, insts, opt)
    ev.close()
    ev = fresh_ev(tf, insts)                                    # on another mesh and horizon: the ladder brings its own
    got = climb(ev, tf, insts, (LR.M_NODES,), opt)
    assert ev.layout.M == LR.M_NODES
    ev.close()
    assert TL.same_bits(want, got) and got["res"] == [want["res"]], (want["res"], got["res"])
    assert all(q["status"] in (LR.CONVERGED, LR.ACCEPTABLE) for q in want["res"])


@pytest.fixture(scope="module")
def ladder_runs(built):
    out, evs = {}, []
    for tf in LR.TFS:
        insts = LD.instances(tf)
        ev = fresh_ev(tf, insts)
        evs.append(ev)
        out[tf] = dict(insts=insts, ev=ev, first=climb(ev, tf, insts, LD.LADDER, dict(tol=TOL)),
                       fine=climb(ev, tf, insts, LD.LADDER, dict(tol=TOL_FINE, max_iter=120)))
    yield out
    for ev in evs:
        ev.close()


@pytest.mark.parametrize("tf", LR.TFS)
def test_the_ladder_reaches_the_fixtures_optima(ladder_runs, tf):
    import torch
    a = ladder_runs[tf]
    r, res, ev = a["first"], a["first"]["res"], a["ev"]
    rows, lad = LR.fixture()["cases"][str(tf)], LD.ladder_fixture()
    cpu = lad["cases"][str(tf)]
    assert lad["ladder"] == list(LD.LADDER) and lad["replaced"] == [] and len(cpu) == len(res[0]) == 9
    B = len(res[-1])
    for g, M in enumerate(LD.LADDER):
        for b in range(B):
            q = res[g][b]
            print(f"tf {tf} rung {M} instance {b}: status {q['status']} iterations {q['iterations']} (CPU ladder {cpu[b]['rungs'][g]['iterations']}) "
                  f"evaluations {q['evaluations']} kkt {q['kkt_error']:.2e} viol {q['constr_viol']:.2e} emax {q['emax']:.2e} rho {q['rho']:g} "
                  f"cost {q['cost']:.6f} (CPU ladder {cpu[b]['rungs'][g]['cost']:.6f})")
    print(f"tf {tf} solved to {TOL_FINE:g}: status / iterations per rung", [[(q["status"], q["iterations"]) for q in g] for g in a["fine"]["res"]])
    status = [q["status"] for q in res[-1]]
    assert all(s in (LR.CONVERGED, LR.ACCEPTABLE) for s in status) and status.count(LR.ACCEPTABLE) <= 1, status
    kw = dict(dtype=torch.float64, device=ev.device)
    RES, VALS, COST = torch.zeros((B, NS + NP, M1), **kw), torch.zeros((B, ev.layout.nvals, M1), **kw), torch.zeros(B, **kw)
    cert = torch.zeros((B, 6), **kw)
    torch.cuda.synchronize()
    assert ev.layout.M == M1
    ev.eval_dev(r["tX"], r["tU"], RES, VALS, COST)
    ev.kkt_certificate_dev(r["tX"], r["tU"], RES, VALS, r["tLamF"], r["tLamC"], 1.0, r["tzl"], r["tzu"], LR.CL, LR.CU, cert)
    ev.synchronize()
    cert, cost = cert.cpu().numpy(), COST.cpu().numpy()
    for b in range(B):
        print(f"  certificate {b}: stat {cert[b, 0]:.2e} comp {cert[b, 1]:.2e} defect {cert[b, 2]:.2e} viol {cert[b, 3]:.2e}")
        assert cert[b, 2] <= TOL and cert[b, 3] <= TOL
        assert cost[b] == res[-1][b]["cost"]
        TL.meets_the_solve_criterion(tf, a["insts"][b], rows[b], r["X"][b], r["U"][b], res[-1][b]["cost"], a["fine"]["X"][b], a["fine"]["U"][b],
                                     f"tf {tf} instance {b}")
    for g, M in enumerate(LD.LADDER):
        mine, theirs = sum(q["iterations"] for q in res[g]), sum(c["rungs"][g]["iterations"] for c in cpu)
        print(f"tf {tf} rung {M}: {mine} iterations over the batch, CPU ladder {theirs}")
        assert mine <= 1.5 * theirs, (tf, M, mine, theirs)


def test_two_calls_agree_and_the_context_stays_on_the_last_mesh(ladder_runs):
    tf = LR.TFS[0]
    a = ladder_runs[tf]
    ev, insts = a["ev"], a["insts"]
    second = climb(ev, tf, insts, LD.LADDER, dict(tol=TOL))
    assert TL.same_bits(a["first"], second) and a["first"]["res"] == second["res"]
    assert ev.layout.M == M1 and ev.layout.B == len(insts)
    # the one-mesh call on the context the ladder left, and on a fresh one: the same bits
    at41 = LR.instances(tf)
    after = TL.solve(ev, tf, at41, dict(tol=TOL, max_iter=200))
    fresh = TL.make_ev(tf, at41)
    want = TL.solve(fresh, tf, at41, dict(tol=TOL, max_iter=200))
    fresh.close()
    assert TL.same_bits(after, want) and after["res"] == want["res"]


def test_the_host_form_and_a_repaired_climb(ladder_runs):
    """the _host form gives the _dev form's bits; with repair on, starts that cross a keep-out still arrive (the instances' own
    starts: bump 0 goes straight through the first disc)"""
    tf = LR.TFS[0]
    a = ladder_runs[tf]
    insts = a["insts"][:3]
    ev = fresh_ev(tf, insts)
    dev = climb(ev, tf, insts, LD.LADDER, dict(tol=TOL, max_iter=6))
    host = climb(ev, tf, insts, LD.LADDER, dict(tol=TOL, max_iter=6), dev=False)
    assert TL.same_bits(dev, host) and dev["res"] == host["res"]
    assert all(q["status"] == LR.MAX_ITER and q["iterations"] == 6 for g in dev["res"] for q in g)
    rep = climb(ev, tf, insts, LD.LADDER, dict(tol=TOL), repair=1)
    ev.close()
    for b, q in enumerate(rep["res"][-1]):
        print(f"repaired climb, instance {b}: status {q['status']} iterations {[g[b]['iterations'] for g in rep['res']]} cost {q['cost']:.6f}")
        assert q["status"] in (LR.CONVERGED, LR.ACCEPTABLE)


def test_ladder_statuses(built):
    import torch
    import etol_amd as E
    from etol_amd import _lib as L
    lib = E.load()
    tf = LR.TFS[0]
    insts = LD.instances(tf)[:2]

    def call(ev, nrungs=2, drop=None, recs=None):
        dev = ev.device
        new = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())
        keep = [new(2, NS, M0), new(2, NC, M0), new(2, NS, M1), new(2, NC, M1), new(2, NS, M1), new(2, NP, M1)]
        arr = (L.IpmRung * 2)()
        for g, M in zip(arr, LD.LADDER):
            bd = bounds_at(tf, M, lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev))
            keep += [bd["zl"], bd["zu"]]
            g.M, g.bd.zl, g.bd.zu, g.bd.nsets = M, p(bd["zl"]), p(bd["zu"]), 1
            g.bd.cl, g.bd.cu = LR.CL.ctypes.data_as(LD.D_), LR.CU.ctypes.data_as(LD.D_)
            g.opt.max_iter = 2
            if recs is not None:
                g.recs = recs.ctypes.data_as(LD.D_)
        args = [p(t) for t in keep[:6]]
        if drop is not None:
            args[drop] = None
        res = (L.IpmResult * 4)()
        torch.cuda.synchronize()
        st = lib.emi_ipm_solve_ladder_dev(ev.ctx, nrungs, arr, 0.0, tf, *args, res)
        ev.synchronize()
        return st

    ev = fresh_ev(tf, insts, f32=True)
    assert call(ev) == 5                                        # EMI_ERR_UNSUPPORTED: f32 context
    ev.close()
    ev = fresh_ev(tf, insts)
    track = np.stack([LR.records(i["discs"]) for i in insts])
    track[1, 0, :3] = [2, 0, 0.25]
    assert call(ev, recs=track) == 5                            # a rung's table with a track row
    ev.set_path(track, 0, 1)
    assert call(ev) == 5                                        # the context's table with a track row
    ev.set_path(np.stack([LR.records(i["discs"]) for i in insts]), 0, 1)
    assert call(ev, nrungs=0) == 1                              # EMI_ERR_ARG
    for drop in range(6):
        assert call(ev, drop=drop) == 1, drop                   # a NULL that is not optional (dX0 first)
    ev.set_option("kkt_method", 0)
    assert call(ev) == 5
    ev.set_option("kkt_method", 1)
    assert call(ev) == 0 and ev.layout.M == M1
    ev.close()
    ev = E.Evaluator(0)
    assert call(ev) == 2                                        # EMI_ERR_STATE: no model, no batch
    ev.close()
    assert lib.emi_ipm_solve_ladder_dev(None, 0, None, 0.0, 1.0, None, None, None, None, None, None, None) == 1
