"""The numpy reference of the node blocks (tests/blocks_ref.py) against the HOST routine solve_nlp runs per factorisation attempt
(assemble_node_blocks + convexify_node_blocks, through tests/harness/etol_harness_blocks.cpp), on the cases and under the bounds
the GPU test (tests/test_gpu_blocks.py) applies to the kernels.  No GPU needed.

The generator's rejections (blocks of kinds "inertia" and "late" too close to a branch threshold) stay within 1 % for the
committed seeds: checked here with numpy alone."""
import ctypes as C
import os

import numpy as np
import pytest

import blocks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_ = C.POINTER(C.c_double)
I_ = C.POINTER(C.c_int)
U_ = C.POINTER(C.c_ubyte)


@pytest.fixture(scope="module")
def H(built):
    h = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    h.harness_blocks_host.restype = C.c_int
    h.harness_blocks_host.argtypes = [C.c_int, C.c_int, C.c_int, I_, I_, I_, D_, D_, D_, D_, U_, C.c_double, D_, D_, C.c_int, I_, I_, D_, D_, D_]
    return h


def host_blocks(h, case, max_mods=None):
    """the host routine on every instance of a case -> the dict blocks_ref.check takes"""
    nv, M, B, npth = case["nv"], case["M"], case["B"], case["np"]
    nh = nv * (nv + 1) // 2
    mm = nv * M if max_mods is None else max_mods
    ptr, var, ent = R.rows_csr(case["rows"])
    out = dict(Qexact=np.zeros((B, nh, M)), Q=np.zeros((B, nh, M)), count=np.zeros(B, dtype=np.int32), node=np.full((B, mm), -1, dtype=np.int32),
               delta=np.zeros((B, mm)), vec=np.zeros((B, mm, nv)), worst=np.zeros(B))
    dp = lambda a: a.ctypes.data_as(D_)
    ip = lambda a: a.ctypes.data_as(I_)
    for b in range(B):
        Hb, Vb, Sb, Tb, Fb = (np.ascontiguousarray(case[n][b]) for n in ("H", "VALS", "Sigma", "SigT", "fixed"))
        cnt, worst = C.c_int(), C.c_double()
        Qx, Q, node, delta, vec = out["Qexact"][b], out["Q"][b], out["node"][b], out["delta"][b], out["vec"][b]
        rc = h.harness_blocks_host(nv, M, npth, ip(ptr), ip(var), ip(ent), dp(Hb), dp(Vb), dp(Sb), dp(Tb), Fb.ctypes.data_as(U_), case["dw"],
                                   dp(Qx), dp(Q), mm, C.byref(cnt), ip(node), dp(delta), dp(vec), C.byref(worst))
        assert rc == 0
        out["count"][b], out["worst"][b] = cnt.value, worst.value
    return out


def test_the_generator_rejects_at_most_one_percent():
    drawn = rejected = 0
    for key in R.case_list():
        c = R.get_case(key)
        drawn += c["drawn"]
        rejected += c["rejected"]
        if c["kind"] != "deficient":
            assert c["rejected"] <= 0.01 * c["drawn"], (key, c["rejected"], c["drawn"])
    print(f"blocks drawn {drawn}, rejected {rejected}")
    assert rejected <= 0.01 * drawn


def test_the_cases_hold_what_they_are_meant_to():
    """every kind has blocks that fail the screen and (inertia, late) blocks that pass it; fixed patterns of all three sorts occur"""
    for key in R.case_list():
        c = R.get_case(key)
        Q, _ = R.assemble(c["H"], c["VALS"], c["Sigma"], c["SigT"], c["fixed"], c["dw"], c["rows"], c["nv"])
        res = [R.fix_block(Q[b, :, k], c["fixed"][b, :, k], c["nv"]) for b in range(c["B"]) for k in range(c["M"])]
        npass = sum(r["passes"] for r in res)
        nfx = c["fixed"].sum(axis=1)
        assert (nfx == 0).any() and (nfx == 1).any() and (nfx == c["nv"]).any()
        assert npass < len(res)
        if c["kind"] == "deficient":
            assert all(r["nneg"] == 0 for r in res)
            free = [r for r, n in zip(res, nfx.ravel()) if n == 0]
            assert max(abs(r["lam"][0]) for r in free) < 1e-13          # the scaled eigenvalue "near 1e-17": 0 up to the rounding of the assembly
        else:
            assert npass > 0 and any(r["nneg"] > 1 for r in res)


@pytest.mark.parametrize("key", R.case_list(), ids=lambda k: f"{k[0]}-nv{k[1]}-M{k[2]}-B{k[3]}-np{k[4]}")
def test_host_routine_against_the_reference(H, key):
    case = R.get_case(key)
    R.check(case, host_blocks(H, case), sorted_within_node=False, log=print)


def test_host_shim_overflow_keeps_the_true_count(H):
    case = R.get_case(R.case_list()[1])
    full = host_blocks(H, case)
    cut = host_blocks(H, case, max_mods=3)
    assert np.array_equal(cut["count"], full["count"]) and full["count"][0] > 3
    assert np.array_equal(cut["node"][0], full["node"][0, :3]) and np.array_equal(cut["vec"][0], full["vec"][0, :3])
