"""emi_start_guess_dev / _host: the straight line, the bent line and the planned route of a context's whole batch.  -m gpu

Every comparison is bit for bit: the planned rows against emi_plan_route (the host function, which tests/test_plan_route_cpu.py
holds to the specification) called per instance, the line and the bend against numpy (tests/plan_ref.py; the sines are libm's, as
in the library), the repair against tests/ladder_ref.py's restatement of repair_guess.  Shapes (B, M, grid, np): (1, 5, 9, 1);
(3, 33, 33, 4) with a shared table and per-instance ends; (70, 65, 17, 3) with per-instance tables built from every kind of fixture
of tests/golden/plan_cases.json, so that one batch holds the levels 0, 1, 2, -1 and -2; (5, 130, 161, 20), the one shape at the full
grid, where the workspace sizing can go wrong.  Each on the quadrotor (px, py = 0, 1) and on the point mass (px, py = 1, 0)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import ladder_ref as LD
import lockstep_ref as LR
import plan_ref as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "plan_cases.json")))}
MODELS = {"quadrotor": (1, 6, 0, 1), "pointmass": (0, 2, 1, 0)}         # model, ns, px, py
CLEARANCE, BEND = 0.01, 0.7
NAN4 = [float("nan")] * 4
PAD = [1.0, 5.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]                          # a disc without radius: no static record


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def padded(recs, n):
    recs = [list(r) for r in recs]
    assert len(recs) <= n
    return recs + [PAD] * (n - len(recs))


def shape_inputs(shape):
    """recs [sets][np][8], ends [B][4], box [B][4] or None, grid, M of a shape of the module's docstring"""
    if shape == "1x5":
        c = CASES["one_disc"]
        return dict(B=1, M=5, grid=9, recs=np.array([c["recs"]]), ends=np.array([c["ends"]]), box=None)
    if shape == "3x33":
        recs = [[1.0, 5.0, 0.3, 1.0, 0, 0, 0, 0], [1.0, 3.0, -1.0, 0.49, 0, 0, 0, 0],
                [0.0, 7.0, 1.0, np.cos(0.5), np.sin(0.5), 2.25, 0.25, 0], [2.0, 0.0, 0.25, 0, 0, 0, 0, 0]]
        ends = [[0.0, 0.0, 10.0, 0.0], [0.0, -2.0, 10.0, 2.0], [10.0, 1.0, 0.0, -1.0]]
        return dict(B=3, M=33, grid=33, recs=np.array([recs]), ends=np.array(ends), box=None)
    if shape == "70x65":
        names = ["open_everywhere", "gap_closed_at_025", "gap_open_at_0_only", "closed_wall", "tracks_only", "one_disc", "rotated_ellipse",
                 "start_in_grown_disc", "ties", "open_everywhere"]
        recs, ends, box = [], [], []
        for b in range(70):
            c = CASES[names[b % len(names)]]
            recs.append(padded(c["recs"], 3))
            e = np.array(c["ends"])
            if c["box"] is None:
                e = e + np.array([0.0, 0.01 * b, 0.0, -0.005 * b])      # no two instances alike
            ends.append(e)
            box.append(c["box"] if c["box"] is not None else NAN4)        # a non-finite entry: the box round the end points
        return dict(B=70, M=65, grid=17, recs=np.array(recs), ends=np.array(ends), box=np.array(box))
    if shape == "5x130":
        wall = np.array(CASES["wall_gap"]["recs"])
        assert wall.shape == (20, 8)
        recs = []
        for b in range(5):
            w = wall.copy()
            w[:, 1] += 0.5 * b - 1.0                                     # the wall stands elsewhere in every instance
            recs.append(w)
        return dict(B=5, M=130, grid=161, recs=np.array(recs), ends=np.array([CASES["wall_gap"]["ends"]]), box=None)
    raise KeyError(shape)


SHAPES = ("1x5", "3x33", "70x65", "5x130")


def make(model, s, tracks=False):
    """the context of a shape on a model, with the end states xa, xb [sets][ns] that carry the shape's end points"""
    import etol_amd as E
    mid, ns, px, py = MODELS[model]
    ev = E.Evaluator(0)
    ev.set_mesh(s["M"], 0.0, 4.0)
    ev.set_model(mid, LR.QUAD_PARAMS if mid == 1 else ())
    ev.set_batch(s["B"])
    if tracks:
        ev.set_tracks(np.full((1, 2, s["M"]), 100.0), np.full((1, 2, s["M"]), -100.0))
    ev.set_path(s["recs"] if s["recs"].shape[0] > 1 else s["recs"][0], px, py)
    rng = np.random.default_rng(len(model) + s["B"])
    sets = s["ends"].shape[0]
    xa, xb = rng.standard_normal((sets, ns)), rng.standard_normal((sets, ns))
    xa[:, px], xa[:, py], xb[:, px], xb[:, py] = s["ends"].T
    return ev, xa, xb


def expected(ev, model, s, xa, xb, kind, bend=BEND, box="shape", repair=False, tracks=None):
    """(X, level) from emi_plan_route per instance, numpy's line and bend and ladder_ref's repair"""
    import etol_amd as E
    _, ns, px, py = MODELS[model]
    B = s["B"]
    box = s["box"] if isinstance(box, str) else box
    full = lambda a: np.broadcast_to(a, (B,) + a.shape[1:]) if a is not None else None
    A, Bb, bx = full(xa), full(xb), full(box)
    X = PR.line(A, Bb, ev.tau)
    level = np.full(B, -2, dtype=np.int32)
    routeless = np.ones(B, dtype=bool)
    if kind == E.START_PLANNED:
        for b in range(B):
            recs = s["recs"][b if s["recs"].shape[0] > 1 else 0]
            ends = np.array([A[b, px], A[b, py], Bb[b, px], Bb[b, py]])
            xs, ys, level[b], _, _ = E.plan_route(recs, ends, ev.tau, None if bx is None else bx[b], CLEARANCE, s["grid"])
            if level[b] >= 0:
                X[b, px], X[b, py], routeless[b] = xs, ys, False
    if kind != E.START_LINE and bend != 0:
        bent = PR.bend_rows(X.copy(), px, py, ev.tau, bend, bx)
        X[routeless] = bent[routeless]
    if repair:
        for b in range(B):
            recs = s["recs"][b if s["recs"].shape[0] > 1 else 0]
            X[b:b + 1] = LD.repair_ref(X[b:b + 1], recs[None], px, py, tracks=tracks)[0]
    return X, level


def run(ev, kind, xa, xb, dev=True, **kw):
    X, level = ev.start_guess(kind, xa, xb, dev=dev, **kw)
    if dev:
        ev.synchronize()
        return X.cpu().numpy(), level.cpu().numpy()
    return X, level


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("model", MODELS)
def test_planned_route_has_the_host_functions_bits(built, model, shape):
    """PLANNED with the bend as the fallback of the routeless: X and level are emi_plan_route's per instance; a second call and the
    _host form give the same bits"""
    import etol_amd as E
    s = shape_inputs(shape)
    ev, xa, xb = make(model, s)
    kw = dict(box=s["box"], bend=BEND, clearance=CLEARANCE, grid=s["grid"])
    want, wlevel = expected(ev, model, s, xa, xb, E.START_PLANNED)
    got, level = run(ev, E.START_PLANNED, xa, xb, **kw)
    print(f"{model} {shape}: levels {sorted(set(level.tolist()))}")
    assert np.array_equal(level, wlevel), (level, wlevel)
    assert np.array_equal(bits(got), bits(want))
    again, level2 = run(ev, E.START_PLANNED, xa, xb, **kw)
    assert np.array_equal(bits(again), bits(got)) and np.array_equal(level2, level)
    host, level3 = run(ev, E.START_PLANNED, xa, xb, dev=False, **kw)
    assert np.array_equal(bits(host), bits(got)) and np.array_equal(level3, level)
    if shape == "70x65":
        assert set(level.tolist()) == {0, 1, 2, -1, -2}
        # without a bend the routeless keep the line
        plain, _ = run(ev, E.START_PLANNED, xa, xb, **dict(kw, bend=0.0))
        assert np.array_equal(bits(plain), bits(expected(ev, model, s, xa, xb, E.START_PLANNED, bend=0.0)[0]))
        assert not np.array_equal(bits(plain[level < 0]), bits(got[level < 0]))
    if shape == "5x130":
        assert (level == 0).all() and not np.array_equal(got[0], got[4])
    ev.close()


@pytest.mark.parametrize("model", MODELS)
def test_line_and_bend(built, model):
    """the kinds that plan nothing, with one shared set of end states and with one per instance; a finite box clips the bend, no box
    and a box of NaN do not; level is -2 everywhere"""
    import etol_amd as E
    _, ns, px, py = MODELS[model]
    s = shape_inputs("3x33")
    ev, xa, xb = make(model, s)
    tight = np.array([[-1.0, 11.0, -0.25, 0.4]] * 3)
    for sets in (1, 3):
        a, b = xa[:sets], xb[:sets]
        for kind, box in ((E.START_LINE, None), (E.START_BEND, None), (E.START_BEND, tight[:sets]), (E.START_BEND, np.array([NAN4] * sets))):
            got, level = run(ev, kind, a, b, box=box, bend=BEND)
            want, _ = expected(ev, model, s, a, b, kind, box=box)
            assert (level == -2).all()
            assert np.array_equal(bits(got), bits(want)), (sets, kind, box)
        clipped, _ = run(ev, E.START_BEND, a, b, box=tight[:sets], bend=BEND)
        free, _ = run(ev, E.START_BEND, a, b, bend=BEND)
        assert clipped[:, py].max() == 0.4 and free[:, py].max() > 0.4 or clipped[:, py].min() == -0.25 and free[:, py].min() < -0.25
        line, _ = run(ev, E.START_LINE, a, b)
        other = [i for i in range(ns) if i not in (px, py)]
        assert np.array_equal(bits(free[:, other]), bits(line[:, other])) and not np.array_equal(free[:, py], line[:, py])
        assert np.array_equal(line[:, :, 0], np.broadcast_to(a, (3, ns)))
    # a bend of zero is the line; the _host form
    zero, _ = run(ev, E.START_BEND, xa, xb, bend=0.0)
    assert np.array_equal(bits(zero), bits(run(ev, E.START_LINE, xa, xb)[0]))
    host, level = run(ev, E.START_BEND, xa, xb, dev=False, box=tight, bend=BEND)
    assert np.array_equal(bits(host), bits(run(ev, E.START_BEND, xa, xb, box=tight, bend=BEND)[0])) and (level == -2).all()
    ev.close()


def test_an_instance_alone_has_the_bits_it_has_in_the_batch(built):
    import etol_amd as E
    model = "quadrotor"
    s = shape_inputs("70x65")
    ev, xa, xb = make(model, s)
    kw = dict(bend=BEND, clearance=CLEARANCE, grid=s["grid"])
    got, level = run(ev, E.START_PLANNED, xa, xb, box=s["box"], **kw)
    ev.close()
    picked = [int(np.flatnonzero(level == l)[-1]) for l in (0, 1, 2, -1, -2)]
    for b in picked:
        one = dict(s, B=1, recs=s["recs"][b:b + 1], ends=s["ends"][b:b + 1], box=s["box"][b:b + 1])
        ev1, _, _ = make(model, one)
        alone, l1 = run(ev1, E.START_PLANNED, xa[b:b + 1], xb[b:b + 1], box=one["box"], **kw)
        assert l1[0] == level[b] and np.array_equal(bits(alone[0]), bits(got[b])), b
        ev1.close()


@pytest.mark.parametrize("model", MODELS)
def test_repair_on_and_off(built, model):
    """repair set: ladder_ref's repair of the unrepaired start, bit for bit -- of the line through the discs of the shared table
    (nodes move), and of the planned batch with its track rows (centres far away)"""
    import etol_amd as E
    _, ns, px, py = MODELS[model]
    s = shape_inputs("3x33")
    tracks = (np.full((1, 2, 33), 100.0), np.full((1, 2, 33), -100.0))
    ev, xa, xb = make(model, s, tracks=True)
    off, _ = run(ev, E.START_LINE, xa, xb)
    on, _ = run(ev, E.START_LINE, xa, xb, repair=1)
    want, _ = expected(ev, model, s, xa, xb, E.START_LINE, repair=True, tracks=tracks)
    assert np.array_equal(bits(on), bits(want)) and not np.array_equal(on[:, [px, py]], off[:, [px, py]])
    assert np.array_equal(bits(off), bits(expected(ev, model, s, xa, xb, E.START_LINE)[0]))
    ev.close()
    s = shape_inputs("70x65")
    tracks = (np.full((1, 2, 65), 100.0), np.full((1, 2, 65), -100.0))
    ev, xa, xb = make(model, s, tracks=True)
    kw = dict(box=s["box"], bend=BEND, clearance=CLEARANCE, grid=s["grid"])
    on, level = run(ev, E.START_PLANNED, xa, xb, repair=1, **kw)
    want, wlevel = expected(ev, model, s, xa, xb, E.START_PLANNED, repair=True, tracks=tracks)
    assert np.array_equal(level, wlevel) and np.array_equal(bits(on), bits(want))
    off, _ = run(ev, E.START_PLANNED, xa, xb, **kw)
    assert not np.array_equal(on, off)                  # the bent fallbacks cross their discs
    ev.close()


def test_refusals(built):
    import torch
    import etol_amd as E
    import etol_amd._lib as L
    lib = E.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    xa, xb = np.zeros((3, 6)), np.ones((3, 6))
    t = torch.zeros(3 * 6 * 9, dtype=torch.float64, device="cuda:0")
    lv = torch.zeros(3, dtype=torch.int32, device="cuda:0")
    p, pl = C.c_void_p(t.data_ptr()), C.c_void_p(lv.data_ptr())
    st = lambda **kw: L.Start(**dict(dict(kind=2, nsets=3, xa=dp(xa), xb=dp(xb), bend=0.0, clearance=0.01, grid=9, repair=0), **kw))
    call = lambda ev, s, X=p, lvl=pl: lib.emi_start_guess_dev(ev.ctx, C.byref(s), X, lvl)
    ev = E.Evaluator(0)
    assert lib.emi_start_guess_dev(None, C.byref(st()), p, pl) == 1
    assert call(ev, st()) == 2                                              # EMI_ERR_STATE: no mesh
    ev.set_mesh(9, 0.0, 4.0)
    assert call(ev, st()) == 2                                              # no model
    ev.set_model(1, LR.QUAD_PARAMS)
    assert call(ev, st()) == 2                                              # no batch
    ev.set_batch(3)
    assert call(ev, st()) == 0 and call(ev, st(), lvl=None) == 0             # no table: level -2, and the level is optional
    ev.synchronize()
    assert lv.cpu().tolist() == [-2, -2, -2]
    assert lib.emi_start_guess_dev(ev.ctx, None, p, pl) == 1 and call(ev, st(), X=None) == 1
    assert call(ev, st(xa=None)) == 1 and call(ev, st(xb=None)) == 1
    for grid in (-1, 1, 8, 162):
        assert call(ev, st(grid=grid)) == 1, grid
    assert call(ev, st(grid=0)) == 0 and call(ev, st(grid=161)) == 0
    assert call(ev, st(nsets=2)) == 1 and call(ev, st(nsets=0)) == 1 and call(ev, st(nsets=1)) == 0
    assert call(ev, st(kind=3)) == 1 and call(ev, st(kind=-1)) == 1
    assert call(ev, st(bend=float("nan"))) == 1 and call(ev, st(clearance=float("nan"))) == 1
    assert call(ev, st(kind=0, bend=float("inf"))) == 0
    assert lib.emi_start_guess_host(ev.ctx, C.byref(st()), None, None) == 1
    ev.set_path(np.array([[2, 0, 0.16, 0, 0, 0, 0, 0]], dtype=float), 0, 1)
    assert call(ev, st()) == 0 and call(ev, st(repair=1)) == 2               # repair of a track row without centres, as emi_repair_guess_dev
    ev.synchronize()
    ev.close()
    f = E.Evaluator(0, f32=True)
    assert call(f, st()) == 5                                               # EMI_ERR_UNSUPPORTED, before anything else
    f.set_mesh(9, 0.0, 4.0)
    f.set_model(1, LR.QUAD_PARAMS)
    f.set_batch(3)
    assert call(f, st()) == 5 and lib.emi_start_guess_host(f.ctx, C.byref(st()), None, None) == 5
    f.close()
