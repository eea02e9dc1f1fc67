"""emi_plan_route (host): the route of planned_path_guess past the static keep-outs as include/emi355x.h specifies it, and what can
be said of emi_start_guess_* without a GPU.  No GPU needed.

The fixtures are tests/golden/plan_cases.json (gen_plan_cases.py).  The function is held to tests/plan_ref.py, the numpy restatement
of the specification, bit for bit (levels, cells, cost, resampled route); its distances to scipy's Dijkstra on the same weighted
grid; its cells to the grid they were found on.  `make check-plan-route` runs the same fixtures through the function in a
stand-alone program under -fsanitize=address,undefined, and what that program prints is compared with the library's answers."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import plan_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (9, 17, 33, 161)
MESHES = (3, 5, 33, 130)
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_cases.json")))
BY_NAME = {c["name"]: c for c in CASES}
NEW = ("emi_plan_route", "emi_start_guess_dev", "emi_start_guess_host")


def args(c):
    return np.array(c["recs"], dtype=np.float64), np.array(c["ends"], dtype=np.float64), c["box"], c["clearance"]


def test_symbols_are_exported_and_bound(built):
    import etol_amd as E
    import etol_amd._lib as L
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "emi355x.h")).read()
    for name in NEW:
        assert name in L.SYMBOLS and getattr(lib, name) is not None and name + "(" in hdr
    assert (L.START_LINE, L.START_BEND, L.START_PLANNED) == (0, 1, 2) and E.START_PLANNED == 2
    assert callable(E.plan_route) and callable(E.Evaluator.start_guess)
    assert [f for f, _ in L.Start._fields_] == ["kind", "nsets", "xa", "xb", "box", "bend", "clearance", "grid", "repair"]
    assert lib.emi_start_guess_dev(None, None, None, None) == 1 and lib.emi_start_guess_host(None, None, None, None) == 1
    assert lib.emi_abi_version() == 2


@pytest.fixture(scope="module")
def refs():
    """plan_ref's route of every fixture on every grid: computed once, read only"""
    out = {}
    for c in CASES:
        recs, ends, box, cl = args(c)
        for grid in GRIDS:
            out[c["name"], grid] = PR.plan(recs, ends, box, cl, grid)
    return out


@pytest.mark.parametrize("grid", GRIDS)
def test_bits_of_the_specification_on_every_fixture(built, refs, grid):
    import etol_amd as E
    for c in CASES:
        recs, ends, box, cl = args(c)
        ref = refs[c["name"], grid][0]
        assert ref.level == c["levels"][str(grid)], c["name"]
        for M in MESHES:
            tau = E.lgl(M)[0]
            xs, ys, level, cost, cells = E.plan_route(recs, ends, tau, box, cl, grid)
            assert level == ref.level, (c["name"], M)
            if level < 0:
                assert xs is None and cost == 0.0 and len(cells) == 0
                continue
            rx, ry = ref.resample(tau)
            assert np.array_equal(xs, rx) and np.array_equal(ys, ry), (c["name"], M)
            assert cost == ref.cost and cells.tolist() == ref.cells, (c["name"], M)


def test_the_designed_levels_on_the_default_grid(built):
    import etol_amd as E
    tau = E.lgl(5)[0]
    want = {"one_disc": 0, "wall_gap": 0, "rotated_ellipse": 0, "open_everywhere": 0, "gap_closed_at_025": 1, "gap_open_at_0_only": 2,
            "closed_wall": -1, "enclosed_goal": -1, "tracks_only": -2, "start_in_grown_disc": 0, "ties": 0}
    assert set(want) == set(BY_NAME)
    for name, level in want.items():
        recs, ends, box, cl = args(BY_NAME[name])
        assert BY_NAME[name]["level"] == level
        assert E.plan_route(recs, ends, tau, box, cl)[2] == level, name             # grid 0: the default
        assert E.plan_route(recs, ends, tau, box, cl, 161)[2] == level, name


def scipy_distances(g, cost, blocked):
    """Dijkstra of scipy from the start cell on the grid's graph: an edge a -> c of weight step cellcost[c] between unblocked cells"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    N = g.N
    idx = np.arange(N * N).reshape(N, N)
    rows, cols, vals = [], [], []
    for di, dj in PR.NEIGHBOURS:
        a = idx[max(0, -di):N - max(0, di), max(0, -dj):N - max(0, dj)]           # sources a, targets c = a + (di, dj)
        c = idx[max(0, di):N - max(0, -di), max(0, dj):N - max(0, -dj)]
        ok = ~blocked.flat[a.ravel()] & ~blocked.flat[c.ravel()]
        rows.append(a.ravel()[ok]); cols.append(c.ravel()[ok]); vals.append((g.step(di, dj) * cost).flat[c.ravel()[ok]])
    graph = csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N * N, N * N))
    return dijkstra(graph, directed=True, indices=g.start)


@pytest.mark.parametrize("grid", GRIDS)
def test_cost_against_scipy_and_cells_against_the_grid(built, refs, grid):
    """cost is scipy's shortest distance to 1e-12 relative (both fold the weights of a path from the left; the margin is for scipy's
    internals); the cells are 8-adjacent, unblocked at the reported level, run from the start cell to the goal cell, and the left
    fold of their weights is cost bit for bit.  Where there is no route scipy finds none either, at any grow."""
    import etol_amd as E
    tau = E.lgl(5)[0]
    for c in CASES:
        recs, ends, box, cl = args(c)
        fields = refs[c["name"], grid][1]
        xs, ys, level, cost, cells = E.plan_route(recs, ends, tau, box, cl, grid)
        if level == -2:
            continue
        if level == -1:
            g = PR.Geom(ends, box, cl, grid)
            fcost, blocked = PR.grid_fields(g, PR.static_records(recs))
            for l in range(3):
                assert np.isinf(scipy_distances(g, fcost, blocked[l])[g.goal]), (c["name"], l)
            continue
        g, fcost, blocked, dist = fields
        sd = scipy_distances(g, fcost, blocked)
        assert abs(cost - sd[g.goal]) <= 1e-12 * sd[g.goal], (c["name"], cost, sd[g.goal])
        fin = np.isfinite(sd)
        assert np.array_equal(fin, np.isfinite(dist.ravel())) and np.abs(dist.ravel()[fin] - sd[fin]).max() <= 1e-12 * sd[fin].max()
        assert cells[0] == g.start and cells[-1] == g.goal and not blocked.flat[cells].any()
        if level > 0:       # the grows before it have no route
            allb = PR.grid_fields(g, PR.static_records(recs))[1]
            for l in range(level):
                assert np.isinf(scipy_distances(g, fcost, allb[l])[g.goal]), (c["name"], l)
        fold = np.float64(0.0)
        for a, b in zip(cells[:-1], cells[1:]):
            di, dj = b // grid - a // grid, b % grid - a % grid
            assert max(abs(di), abs(dj)) == 1
            fold = fold + g.step(di, dj) * fcost.flat[b]
        assert fold == cost, (c["name"], fold, cost)


def test_the_route_takes_the_gap_of_the_wall(built):
    """the wall of overlapping discs stands on x = 5 with its gap between y = 3 and y = 5: the straight line y = 0 meets the wall,
    the route crosses x = 5 inside the gap and keeps out of every disc"""
    import etol_amd as E
    recs, ends, box, cl = args(BY_NAME["wall_gap"])
    tau = E.lgl(130)[0]
    xs, ys, level, _, _ = E.plan_route(recs, ends, tau, box, cl)
    assert level == 0
    k = int(np.searchsorted(xs, 5.0))
    assert 0 < k < len(xs) and xs[k - 1] < 5.0 <= xs[k]
    y_at = ys[k - 1] + (5.0 - xs[k - 1]) / (xs[k] - xs[k - 1]) * (ys[k] - ys[k - 1])
    assert 3.0 < y_at < 5.0, y_at
    inside = lambda x, y: (((x[:, None] - recs[None, :, 1]) ** 2 + (y[:, None] - recs[None, :, 2]) ** 2) < recs[None, :, 3]).any(1)
    assert not inside(xs, ys).any()
    assert inside(ends[0] + (ends[2] - ends[0]) * 0.5 * (tau + 1.0), np.zeros_like(tau)).any()


def test_ties_are_broken_the_same_way_every_time(built):
    import etol_amd as E
    recs, ends, box, cl = args(BY_NAME["ties"])
    tau = E.lgl(33)[0]
    for grid in (17, 161):
        first = E.plan_route(recs, ends, tau, box, cl, grid)
        ref = PR.plan_route(recs, ends, tau, box, cl, grid)
        for _ in range(3):
            again = E.plan_route(recs, ends, tau, box, cl, grid)
            for a, b, r in zip(first, again, ref):
                assert np.array_equal(a, b) and np.array_equal(a, r)
        # the mirrored problem has the mirrored distances: a tie, which the predecessor rule settles one way
        assert first[3] == E.plan_route(recs * np.array([1, 1, -1, 1, 1, 1, 1, 1.0]), ends, tau, box, cl, grid)[3]


def test_every_refusal(built):
    import etol_amd._lib as L
    lib = L.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rec = np.array([1.0, 5, 0, 1, 0, 0, 0, 0])
    ends, tau = np.array([0.0, 0, 10, 0]), np.array([-1.0, 0.0, 1.0])
    xs, ys, level = np.empty(3), np.empty(3), C.c_int()

    def call(np_=1, r=rec, e=ends, cl=0.01, grid=0, M=3, t=tau, x=xs, y=ys, lv=level):
        return lib.emi_plan_route(np_, dp(r) if r is not None else None, dp(e) if e is not None else None, None, cl, grid, M,
                                  dp(t) if t is not None else None, dp(x) if x is not None else None, dp(y) if y is not None else None,
                                  C.byref(lv) if lv is not None else None, None, None, None)
    assert call() == 0 and level.value == 0
    assert call(np_=-1) == 1 and call(r=None) == 1 and call(e=None) == 1 and call(t=None) == 1
    assert call(x=None) == 1 and call(y=None) == 1 and call(lv=None) == 1
    assert call(cl=float("nan")) == 1 and call(M=1) == 1
    for grid in (-1, 1, 8, 162, 1000):
        assert call(grid=grid) == 1, grid
    for grid in (9, 161):
        assert call(grid=grid) == 0


def test_the_sanitized_program_agrees_with_the_library(built, tmp_path_factory):
    """`make check-plan-route`: the fixtures through emi_plan_route in a stand-alone program under the host sanitizers; what it
    prints (levels, cost, cells, the route at 33 nodes, as hexadecimal doubles) is what the library loaded here answers"""
    import etol_amd as E
    out = tmp_path_factory.mktemp("plan") / "plan_route_check"
    r = subprocess.run(["make", "-C", ROOT, "check-plan-route", f"PLAN_CHECK_OUT={out}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "plan route: ok" in r.stdout
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == len(CASES) * len(GRIDS)
    tau = E.lgl(33)[0]
    for q in lines:
        recs, ends, box, cl = args(BY_NAME[q["case"]])
        xs, ys, level, cost, cells = E.plan_route(recs, ends, tau, box, cl, q["grid"])
        assert level == q["level"] and cost == float.fromhex(q["cost"]) and cells.tolist() == q["cells"], (q["case"], q["grid"])
        if level >= 0:
            assert xs.tolist() == [float.fromhex(v) for v in q["xs"]] and ys.tolist() == [float.fromhex(v) for v in q["ys"]]
