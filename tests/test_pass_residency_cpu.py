"""Resident workgroups per CU of the one-launch pass ("sym_res", etol_amd/csrc/emi_pass_plan.hpp): tests/harness/pass_residency_main.cpp
holds the rule without a device, built with -fsanitize=address,undefined (`make check-pass-residency`): three are stated only by a launch
of a direct-operator row, the want is dropped and never the launch, built-in models only, the wants are granted in the order resolve_form
documents, and the default by band is what profiles/residency_notes.md arrives at.  No GPU needed.

Here: the program's own checks pass, and the plans it prints for the 6-state model at 1024 nodes say what the notes say."""
import json
import os
import subprocess

import pytest

from pinned_plans import PINNED_PLANS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# profiles/residency_notes.md section 3: where the default states three resident workgroups per CU ({instances: (residency, block order)});
# everywhere else it states two
THREE_BY_DEFAULT = {152: (3, 1), 160: (3, 1), 1024: (3, 110), 1152: (3, 110), 1280: (3, 110), 1536: (3, 110), 1792: (3, 110), 2048: (3, 110)}
TWO_BY_DEFAULT = (16, 64, 128, 144, 176, 192, 256, 288, 320, 352, 384, 416, 432, 512, 768, 896, 4096)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("residency") / "pass_residency_check"
    r = subprocess.run(["make", "-C", ROOT, "check-pass-residency", f"PASS_RES_CHECK_OUT={out}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pass residency: ok" in r.stdout
    return str(out)


def plan(program, B, **options):
    """the 6-state model at 1024 nodes with 20 keep-outs per instance, as the benchmark sets it up"""
    r = subprocess.run([program, "plan", "6", "2", "1024", str(B), "np=20"] + [f"{k}={v}" for k, v in options.items()], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_default_by_band_is_what_was_measured(program):
    for B, (res, order) in THREE_BY_DEFAULT.items():
        p = plan(program, B)
        assert (p["one_launch"], p["res"], p["dop"], p["block_order"], p["sw"], p["k_tile"]) == (1, res, 1, order, 2, 16), (B, p)
    for B in TWO_BY_DEFAULT:
        p = plan(program, B)
        assert (p["one_launch"], p["res"]) == (1, 2), (B, p)


@pytest.mark.parametrize("B", sorted(PINNED_PLANS))
def test_the_residency_moves_no_pinned_field(program, B):
    for res in (0, 2, 3):
        p = plan(program, B, sym_res=res)
        for k, v in PINNED_PLANS[B].items():
            if k in p:
                assert p[k] == v, (B, res, k, p)


def test_three_only_with_a_direct_operator_row(program):
    # the benchmarked shape takes De / Do from L2 by itself: the want is granted, and nothing else moves
    two, three = plan(program, 1024, sym_res=2), plan(program, 1024, sym_res=3)
    assert (two["res"], three["res"], three["dop"]) == (2, 3, 1)
    assert {k: v for k, v in two.items() if k != "res"} == {k: v for k, v in three.items() if k != "res"}
    # through the ring: dropped, the launch stays
    p = plan(program, 1024, sym_res=3, sym_dop=1)
    assert (p["one_launch"], p["res"], p["dop"], p["k_tile"]) == (1, 2, 0, 16), p
    # 128 instances take the staged form by default, and the direct one when asked
    assert plan(program, 128, sym_res=3)["res"] == 2
    p = plan(program, 128, sym_res=3, sym_dop=2)
    assert (p["res"], p["dop"], p["sw"]) == (3, 1, 2), p
    # whatever takes the direct form away takes the third workgroup with it: K halves, wide tiles, four stages, 8-deep tiles, slices, SW = 3 / NS
    for options in (dict(sym_hs=2), dict(sym_ctc=2, sym_ct=6), dict(sym_nst=4), dict(sym_bk=8), dict(sym_ksplit=2), dict(sym_ct=8), dict(sym_ct=5)):
        p = plan(program, 1024, sym_res=3, sym_dop=2, **options)
        assert (p["one_launch"], p["res"], p["dop"]) == (1, 2, 0), (options, p)
    # one state per workgroup has a direct form too
    p = plan(program, 1024, sym_res=3, sym_dop=2, sym_ct=7, sym_bk=16)
    assert (p["sw"], p["res"], p["dop"]) == (1, 3, 1), p
