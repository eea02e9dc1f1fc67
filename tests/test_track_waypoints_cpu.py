"""emi_set_track_waypoints, emi_tracks_from_waypoints_dev, emi_get_tracks: what can be said of them without a GPU, and the CPU
reference of the ladder with moving-disc rows.  No GPU needed.

  * the header declares the three calls, the library exports them and the Python mirror types them;
  * without a context (no device here) each of them is an argument error, as every call that takes a context is;
  * tests/harness/etol_harness_track_ladder.cpp reproduces tests/golden/track_ladder_cases.json row for row, the fixture's
    instances are those of tests/track_ladder_ref.py, every one converges on both rungs with its moving disc active, and with the
    track at rest the new harness call gives what the existing one gives with the disc -- the optima of
    tests/golden/ladder_cases.json."""
import ctypes as C
import os
import re

import numpy as np

import ladder_ref as LD
import track_ladder_ref as TR

ROOT = TR.ROOT
CALLS = ("emi_set_track_waypoints", "emi_tracks_from_waypoints_dev", "emi_get_tracks")


def test_the_header_declares_the_calls_and_the_library_exports_them(built):
    import etol_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "emi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.load()
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(\s*emi_ctx_t\b" % name, hdr), name
        assert name in L.SYMBOLS and getattr(lib, name) is not None, name
    import etol_amd as E
    for method in ("set_track_waypoints", "tracks_from_waypoints", "get_tracks"):
        assert callable(getattr(E.Evaluator, method))


def test_without_a_context_every_call_is_an_argument_error(built):
    import etol_amd as E
    lib = E.load()
    t = np.array([0.0, 1.0, 2.0])
    p = t.ctypes.data_as(TR.D_)
    cnt = np.array([3], dtype=np.int32)
    assert lib.emi_set_track_waypoints(None, 1, 1, 3, cnt.ctypes.data_as(TR.I_), p, p, p) == 1
    assert lib.emi_set_track_waypoints(None, 0, 0, 0, None, None, None, None) == 1
    assert lib.emi_tracks_from_waypoints_dev(None, 0, None) == 1
    assert lib.emi_get_tracks(None, p, p) == 1


def test_the_harness_reproduces_the_fixture_row_for_row(built):
    fx = TR.fixture()
    assert fx["ladder"] == list(TR.LADDER) and fx["tf"] == TR.TF and fx["t_mid"] == TR.T_MID and fx["displacement"] == TR.DISPLACEMENT
    assert (fx["displacement"] == 1.0) == (fx["note"] == "")            # another displacement comes with its reason
    insts = TR.moving_instances()
    assert len(fx["cases"]) == len(insts) == TR.N_MOVING
    for M in TR.LADDER:
        assert np.abs(TR.node_times(M, 0.0, TR.TF) - TR.T_MID).min() > 1e-3         # a node time of neither rung
    h = TR.load_harness()
    for b, (inst, row) in enumerate(zip(insts, fx["cases"])):
        assert [list(d) for d in inst["discs"]] == row["discs"] and inst["bump"] == row["bump"]
        t, x, y = inst["way"]
        assert (t[0].tolist(), x[0].tolist(), y[0].tolist()) == (row["waypoints"]["t"], row["waypoints"]["x"], row["waypoints"]["y"])
        assert t[0, 0] == 0.0 and t[0, -1] == TR.TF and t.shape == (1, 3)
        rungs, _ = TR.cpu_climb(h, TR.TF, inst)
        print(f"instance {b}: " + "; ".join(f"M {r['M']} ok {r['ok']} it {r['iterations']} cost {r['cost']:.9f} kkt {r['kkt_error']:.1e}" for r in rungs))
        assert rungs == row["rungs"], (b, rungs, row["rungs"])
        assert all(r["ok"] for r in rungs), b
        assert row["track_slack"] < 1e-6 * inst["discs"][0][2] ** 2, b          # the moving disc is active


def test_a_track_at_rest_is_the_disc(built):
    """the new harness call with every waypoint at the disc's centre against tests/golden/ladder_cases.json (recorded with the
    disc): the centre arithmetic returns the centre exactly and the oracle's track row is its disc row, so the climb is the same"""
    cpu = LD.ladder_fixture()["cases"][str(TR.TF)]
    h = TR.load_harness()
    for b, inst in enumerate(TR.static_instances(TR.TF)[:2]):
        xc, yc = TR.host_centres([inst["way"]], 21, 0.0, TR.TF)
        assert (xc == inst["discs"][0][0]).all() and (yc == inst["discs"][0][1]).all()
        rungs, _ = TR.cpu_climb(h, TR.TF, inst)
        for got, want in zip(rungs, cpu[b]["rungs"]):
            assert (got["ok"], got["iterations"], got["cost"]) == (want["ok"], want["iterations"], want["cost"]), (b, got, want)


def test_the_harness_refuses_a_track_row_without_its_track(built):
    h = TR.load_harness()
    inst = TR.moving_instances()[0]
    recs = np.ascontiguousarray(inst["recs"])
    z = np.zeros(8 * 21)
    dp = lambda a: a.ctypes.data_as(TR.D_)
    out_d, out_i = np.zeros(4), np.zeros(3, dtype=np.int32)
    rc = h.harness_track_ladder_solve_oracle(b"", 21, TR.TF, dp(z), recs.shape[0], dp(recs), 0, None, None, dp(z), dp(z), dp(z), dp(z), 1e-8, 1, 1,
                                             dp(out_d), out_i.ctypes.data_as(TR.I_), dp(z))
    assert rc == 2
