"""The work table of the one-launch pass (etol_amd/csrc/emi_pass_work.hpp): one entry per block of the grid, built on the host from
pass_role_of and ring_tile_of, read by emi_pass_f64_kernel instead of working the two maps out in every workgroup.  No GPU needed.

Through emi_debug_pass_work, against the two maps as emi_debug_pass_roles and emi_debug_tile_order2 return them: every entry equals what
the two functions return, every (tile, K slice) and every node chunk is visited exactly once, every remaining block is idle -- over both
built-in fp64 models, three meshes, twelve batches, five block orders, column partitions and the grouped order where plan_symdefect
admits them, K slices and K halves.  tests/harness/pass_work_main.cpp holds the same (and every SW) as a stand-alone program built with
-fsanitize=address,undefined (`make check-pass-work`)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from etol_amd import _lib as L
from etol_amd.evaluator import debug_pass_work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODELS = {"pointmass": 2, "quadrotor": 6}       # states
MESHES = (128, 256, 1024)
BATCHES = (1, 3, 16, 17, 80, 128, 160, 320, 704, 1024, 2048, 4096)
ORDERS = (0, 1, 110, 150, 400)
CPARTS = (0, 1, 2, 4, 8)
GBLKS = (1, 2, 4)                               # the grouped order: the plan's cpart comes back as -1, -2, -4
KSPLITS = (1, 2, 4)
IDLE, MFMA, NODE = 0, 1, 2


def sw_of(ns, B):
    """states per MFMA workgroup as the default dispatch picks them: one below 128 tiles of the 1024-node mesh, else two (all of two)"""
    return 1 if B < 256 and ns > 2 else 2


def ct_code(ns, sw):
    return 5 if sw == ns else (6 if sw == 2 else (8 if sw == 3 else 7))


@functools.lru_cache(maxsize=None)
def roles_of(nm8, nn8, order):
    out = (C.c_int * (nm8 + nn8))()
    assert L.load().emi_debug_pass_roles(nm8, nn8, order, out, nm8 + nn8) == 0
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=64)
def tiles_of(ns, B, M, sw, cpart, gblk):
    cap = (M // 128) * ((B + 15) // 16) * ns
    out = (C.c_int * cap)()
    tot, cp, cx = C.c_int(), C.c_int(), C.c_int()
    assert L.load().emi_debug_tile_order2(ns, B, M, ct_code(ns, sw), cpart, gblk, 0, out, cap, C.byref(tot), C.byref(cp), C.byref(cx)) == 0
    return np.array(out[:tot.value], dtype=np.int64), cp.value, cx.value


def check_case(ns, B, M, sw, order, cpart, gblk, ksplit, hs):
    got = debug_pass_work(ns, B, M, sw, 1, ksplit, hs, cpart, gblk, 0, order)
    assert got is not None, (ns, B, M, sw)
    table, info = got
    tiles, cp, cx = tiles_of(ns, B, M, sw, cpart, gblk)
    assert (info["cpart"], info["cx"]) == (cp, cx)
    nm, nn, nm8, nn8, nbx, ntiles, ks = (info[k] for k in ("nm", "nn", "nm8", "nn8", "nbx", "ntiles", "ks"))
    assert nm == tiles.size * ks and nn == nbx * B and info["blocks"] == 8 * (nm8 + nn8) == len(table)
    what = (ns, B, M, sw, order, cp, cx, ks, hs)
    # what pass_role_of and ring_tile_of say for every block g of the grid
    g = np.arange(len(table))
    xcd, r = g & 7, roles_of(nm8, nn8, order)[g >> 3]
    want = np.zeros((len(table), 5), dtype=np.int64)
    tid = xcd * nm8 + r
    m = (r >= 0) & (tid < nm)
    code = tiles[tid[m] // ks]
    want[m] = np.stack([np.full(m.sum(), MFMA), code % ntiles, code // ntiles, tid[m] % ks, np.zeros(m.sum(), dtype=np.int64)], axis=1)
    n0 = (xcd * nn8 + (-1 - r)) * hs
    n = (r < 0) & (n0 < nn)
    second = n0[n] + 1 < nn if hs == 2 else np.zeros(n.sum(), dtype=bool)
    want[n] = np.stack([np.full(n.sum(), NODE), n0[n] % nbx, n0[n] // nbx, np.where(second, (n0[n] + 1) % nbx, -1), np.where(second, (n0[n] + 1) // nbx, -1)],
                       axis=1)
    assert np.array_equal(table, want), (what, np.flatnonzero((table != want).any(axis=1))[:5])
    # every (tile, slice) once, every node chunk once, the rest idle
    t = table[table[:, 0] == MFMA]
    assert np.array_equal(np.sort((t[:, 2] * ntiles + t[:, 1]) * ks + t[:, 3]), np.arange(nm)), what
    c = table[table[:, 0] == NODE]
    chunks = c[:, 2] * nbx + c[:, 1]
    if hs == 2:
        chunks = np.concatenate([chunks, (c[:, 4] * nbx + c[:, 3])[c[:, 3] >= 0]])
    assert np.array_equal(np.sort(chunks), np.arange(nn)), what
    idle = table[table[:, 0] == IDLE]
    assert not idle.any() and len(idle) == len(table) - nm - len(c), what
    return cp


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("M", MESHES)
def test_every_entry_is_what_the_two_maps_return(model, M):
    ns = MODELS[model]
    grouped = partitioned = cases = 0
    for B in BATCHES:
        sw = sw_of(ns, B)
        orders = []         # (cpart option, gblk option) plan_symdefect admits here, each once
        for cpart in CPARTS:
            cp = tiles_of(ns, B, M, sw, cpart, 0)[1]
            if cpart == 0 or cp == cpart:
                orders.append((cpart, 0))
        for gblk in GBLKS:
            if tiles_of(ns, B, M, sw, 0, gblk)[1] == -gblk:
                orders.append((0, gblk))
        for cpart, gblk in orders:
            for order in ORDERS:
                for ksplit in KSPLITS:
                    for hs in (1, 2):
                        cp = check_case(ns, B, M, sw, order, cpart, gblk, ksplit, hs)
                        cases += 1
                        grouped += cp < 0
                        partitioned += cp > 0
    # (a 128-node mesh has one column tile: nothing to partition)
    assert cases >= 12 * 5 * 3 * 2 and grouped > 0 and (partitioned > 0 or M == 128), (cases, grouped, partitioned)


def test_every_sw_of_the_form_table_and_the_wide_tiles():
    """the other states per workgroup the forms take (SW = 1 at a large batch, 3 and all six), and two column sub-tiles per workgroup"""
    for sw in (1, 3, 6):
        for B, order in ((17, 1), (320, 150), (1024, 110)):
            check_case(6, B, 1024, sw, order, 0, 0, 1, 1)
    for B, gblk in ((320, 0), (1024, 0), (4096, 2)):
        got = debug_pass_work(6, B, 1024, 2, 2, 1, 1, 0, gblk, 1, 0)
        assert got is not None
        table, info = got
        assert info["ntiles"] == 4 and (info["cpart"] < 0) == (gblk > 0)
        t = table[table[:, 0] == MFMA]
        assert np.array_equal(np.sort(t[:, 2] * 4 + t[:, 1]), np.arange(info["nm"]))
        assert (table[:, 0] == NODE).sum() == info["nn"]


def test_a_launch_that_does_not_exist_is_refused():
    lib = L.load()
    info = (C.c_int * 12)()
    for args in ((6, 16, 1000, 2, 1, 1, 1), (6, 16, 1024, 4, 1, 1, 1), (6, 16, 1024, 2, 3, 1, 1), (6, 16, 1024, 2, 1, 1, 3), (6, 0, 1024, 2, 1, 1, 1)):
        assert lib.emi_debug_pass_work(*args, 0, 0, 0, 0, None, 0, info) != 0, args
    # two column sub-tiles need SW = 2, an unsplit K range and a mesh of whole 256-node tiles
    assert debug_pass_work(6, 16, 128, 2, ctc=2) is None
    assert debug_pass_work(6, 16, 1024, 1, ctc=2) is None


def test_the_builder_under_the_host_sanitizers(tmp_path):
    out = tmp_path / "pass_work_check"
    r = subprocess.run(["make", "-C", ROOT, "check-pass-work", f"PASS_WORK_CHECK_OUT={out}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pass work: ok" in r.stdout and " 0 failures" in r.stdout
