"""The launch policy of the fp64 evaluation pass (etol_amd/csrc/emi_pass_plan.hpp: the form table, the band table, resolve_form,
plan_pass, plan_piece) has no device in it: tests/harness/pass_plan_main.cpp walks it over the grid of tools/api_identity.py plan, built
with -fsanitize=address,undefined (`make check-pass-plan`), holds every one-launch plan to the form table, the K loop, the grid size and
the pieces, and prints the plan of any context.  No GPU needed.

Here: the program's own checks pass, its grid is the one the tool walks on the device, the pinned plans of the benchmarked shapes hold on
the CPU as they do on the GPU (tests/test_gpu_parity.py), and the 2-state model reports the kernel that runs."""
import importlib.util
import json
import os
import subprocess

import pytest

from pinned_plans import PINNED_PLANS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan") / "pass_plan_check"
    r = subprocess.run(["make", "-C", ROOT, "check-pass-plan", f"PASS_PLAN_CHECK_OUT={out}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pass plan: ok" in r.stdout
    return str(out)


def plan(program, ns, nc, M, B, **options):
    r = subprocess.run([program, "plan", str(ns), str(nc), str(M), str(B)] + [f"{k}={v}" for k, v in options.items()], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_program_walks_the_grid_of_the_identity_tool(program):
    spec = importlib.util.spec_from_file_location("api_identity", os.path.join(ROOT, "tools", "api_identity.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = subprocess.run([program, "grid"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {c["case"]: c for c in (json.loads(line) for line in r.stdout.splitlines())}
    want = [name for name, *_ in tool.plan_cases((2, 6))]
    assert set(got) == set(want) and len(want) > 8000
    fields = {"case", "one_launch", "sw", "ksplit", "ring_stages", "cpart", "cx", "mfma_workgroups", "store_mode", "block_order", "tiles16", "piece",
              "tail", "k_tile", "column_tiles", "k_halves", "dop"}
    assert all(set(c) == fields for c in got.values())
    # under the default options every point of the grid goes out as one launch
    assert all(c["one_launch"] == 1 for name, c in got.items() if " None=None " in name)


@pytest.mark.parametrize("B", sorted(PINNED_PLANS))
def test_pinned_plans_of_the_six_state_model_at_1024_nodes(program, B):
    """as test_default_dispatch_at_the_benchmarked_shapes_matches_the_oracle sets the context up: 20 keep-outs per instance"""
    p = plan(program, 6, 2, 1024, B, np=20)
    assert p["one_launch"] == 1
    for k, v in PINNED_PLANS[B].items():
        assert p[k] == v, (B, k, p)


def test_the_two_state_model_reports_the_form_that_runs(program):
    """512 instances at 1024 nodes are in the range where two states of a larger model take 16-deep K tiles; both states of the 2-state
    model are all its states, whose only form has 8-deep tiles, three ring stages and an undivided K range -- whatever is asked for"""
    p = plan(program, 2, 2, 1024, 512)
    assert (p["one_launch"], p["sw"], p["k_tile"], p["dop"]) == (1, 2, 8, 0), p
    assert plan(program, 6, 2, 1024, 512)["k_tile"] == 16
    p = plan(program, 2, 2, 1024, 1024)          # (unsplit: more workgroups than the slice rule fills up)
    assert (p["sw"], p["ksplit"], p["k_tile"], p["dop"]) == (2, 1, 8, 0), p
    for options in (dict(sym_nst=4, sym_ct=5), dict(sym_hs=2, sym_ct=6), dict(sym_bk=16, sym_ct=6), dict(sym_ctc=2, sym_ct=6)):
        q = plan(program, 2, 2, 1024, 512, **options)
        assert (q["sw"], q["ring_stages"], q["k_tile"], q["k_halves"], q["column_tiles"]) == (2, 3, 8, 1, 1), (options, q)
        assert q["mfma_workgroups"] == 32 * 8
    # ... and three states per workgroup of the 6-state model likewise
    q = plan(program, 6, 2, 1024, 512, sym_ct=8, sym_nst=4)
    assert (q["sw"], q["ring_stages"]) == (3, 3), q
