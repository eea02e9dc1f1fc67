"""A context with a history gives the bits of a new one.  -m gpu

Every life and every seeded walk of tests/context_life.py is walked on ONE context; after every calling step the same call with the same
inputs runs on fresh(config), a new context set up from the mirror of everything the lived one was given, and every output -- values,
counts, statuses, the poisoned slack behind each buffer -- must be bit-identical, and so must the plan of the one-launch pass where both
contexts take it.  The inputs of consecutive calls differ (a seed per step), so a partial sum, a cost partial or a staged array that a call
read from what the previous one left would show.  The fresh context is closed at once: at most two contexts are alive.

Bit equality is the bar because the lived and the fresh context run the same code on the same plan, and the project asserts bit
reproducibility of every call elsewhere.  That both are wrong in the same way is ruled out by the oracle: the last evaluation of every
f64 life is held to tests/oracle_lib.py with check() of test_gpu_parity.py (5e-13 of the row scale on defect rows, 1e-13 elsewhere)."""
import types

import numpy as np
import pytest

import context_life as CL

pytestmark = pytest.mark.gpu


def against_oracle(last):
    import etol_amd as E
    import oracle_lib as O
    from test_gpu_parity import check
    cfg, X, U, got = last
    assert cfg.source is None and not cfg.f32
    tau, w, D = E.lgl(cfg.M)
    tracks = cfg.tracks
    ref = O.evaluate(cfg.model, list(cfg.params), cfg.M, (tau, w, D), cfg.t0, cfg.tf, X, U, cfg.recs, tracks, maximize=cfg.maximize,
                     **(dict(px=cfg.px, py=cfg.py) if (cfg.px, cfg.py) != (0, 1) else {}))
    check(dict(X=X), types.SimpleNamespace(D=D), got, ref)


@pytest.mark.parametrize("name", ["ladder", "forms", "models", "staging", "f32"])
def test_life(built, name):
    out = CL.walk(CL.LIVES[name](), f32=name == "f32")
    try:
        assert out["last"] is not None
        if name != "f32":
            against_oracle(out["last"])
        if name == "forms":
            assert out["cfg"].options == {}     # the default plan again (walk() has compared the plans of the last pass)
            assert out["plans"] >= len(CL.FORMS)
            # the options did take hold: K tiles of 16, K halves, two column tiles and the three block orders are plans of their own
            distinct = {tuple(sorted(p.items())) for p in out["plan_list"]}
            print(f"forms: {len(distinct)} distinct plans in {out['plans']} compared passes")
            assert len(distinct) >= 5 and {p["k_tile"] for p in out["plan_list"]} >= {8, 16}, distinct
            assert {p["k_halves"] for p in out["plan_list"]} >= {1, 2} and {p["column_tiles"] for p in out["plan_list"]} >= {1, 2}
            assert {p["block_order"] for p in out["plan_list"]} >= {0, 1, 150}
    finally:
        out["lived"].close()


def test_life_batch(built):
    """... and the eviction really happened (the first key's table is uploaded a second time), and K-sliced passes did follow one
    another at different inputs"""
    steps = CL.LIVES["batch"]()
    out = CL.walk(steps)
    try:
        against_oracle(out["last"])
        # the life ends where it began: 17 instances, the options of the first pass ...
        first_call = next(i for i, st in enumerate(steps) if st.kind not in CL.SETTERS)
        assert [st for st in steps[:first_call] if st.kind == "option"] == [CL.S("option", name=k, value=v) for k, v in out["cfg"].options.items()]
        assert steps[2] == CL.S("batch", B=17) and out["cfg"].B == 17
        # ... whose table had given way in between: the first pass after the return uploads it again, into a full cache
        back = max(i for i, st in enumerate(steps) if st.kind == "batch")
        before = [u for i, u in out["uploads"] if i < back][-1]
        after = [u for i, u in out["uploads"] if i > back][0]
        assert before[1] == 8 and after == (before[0] + 1, 8), (before, after)
        assert out["uploads"][-1][1] == after           # and the passes after it upload nothing
        pairs = [(a, b) for a, b in zip(out["ksliced"], out["ksliced"][1:]) if b[0] == a[0] + 1 and b[1] != a[1]]
        assert pairs, out["ksliced"]
    finally:
        out["lived"].close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_walk(built, seed):
    out = CL.walk(CL.seeded_walk(seed))
    out["lived"].close()


def test_drivers(built):
    """The nine instances of tests/golden/lockstep_cases.json on the ladder (21, 41), an unrelated evaluation at 128 nodes, the same
    solve again: the statuses, iteration counts, trajectories, multipliers and costs of the first, and of a fresh context; the
    evaluations in between and after equal a fresh context's."""
    import ladder_ref as LD
    import lockstep_ref as LR
    import test_gpu_ladder as TLad
    import test_gpu_lockstep as TL
    tf = LR.TFS[0]
    insts = LD.instances(tf)
    recs = np.stack([LR.records(i["discs"]) for i in insts])
    cfg = CL.Config(M=9, t0=0.0, tf=1.0, model=CL.QUAD, params=tuple(LR.QUAD_PARAMS), B=len(insts), recs=recs, per_instance=True)
    ev = CL.fresh(cfg)
    solves = []
    try:
        for st in CL.LIVES["drivers"]():
            if st.kind == "ipm_solve_ladder":
                solves.append(TLad.climb(ev, tf, insts, LD.LADDER, dict(tol=TLad.TOL)))
                cfg.M, cfg.t0, cfg.tf = LD.LADDER[-1], 0.0, tf          # the context is on the last rung's mesh afterwards
                assert ev.layout.M == cfg.M
            elif st.kind in CL.SETTERS:
                CL.SETTERS[st.kind](ev, cfg, st)
            else:
                got, _ = CL.run_one(ev, cfg, st)
                fr = CL.fresh(cfg)
                try:
                    want, _ = CL.run_one(fr, cfg, st)
                finally:
                    fr.close()
                CL.same_bits(got, want, str(st))
    finally:
        ev.close()
    fr = TLad.fresh_ev(tf, insts)
    try:
        solves.append(TLad.climb(fr, tf, insts, LD.LADDER, dict(tol=TLad.TOL)))
    finally:
        fr.close()
    first, second, new = solves
    assert all(q["status"] in (LR.CONVERGED, LR.ACCEPTABLE) for q in first["res"][-1])
    for other, who in ((second, "the second solve"), (new, "a fresh context")):
        assert TL.same_bits(first, other), who
        assert first["res"] == other["res"], who            # statuses, iteration counts, costs, errors: every field of every rung
