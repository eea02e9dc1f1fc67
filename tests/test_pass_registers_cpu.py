"""The register budget of emi_pass_f64_kernel (`make check-pass-registers`, tools/check_pass_registers.py): every instantiation is
cross-compiled for gfx950 and held to the resident workgroups per CU it states -- 3: occupancy 3, at most 168 registers, no scratch;
2: no scratch and the figures tools/pass_registers.json records.  amdgpu_waves_per_eu(2, 3) would let a source change that needs more
registers fall back to two waves per SIMD without a word; this fails instead.  Needs hipcc, no GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_the_record_names_the_instantiations_that_state_two():
    with open(os.path.join(ROOT, "tools", "pass_registers.json")) as f:
        rec = json.load(f)
    assert len(rec) > 100 and all(k.endswith(", 2") for k in rec)
    # the benchmarked instantiation: 160 registers, which is what leaves a third wave its room
    assert rec["Quadrotor2D, 2, 2, 2, 3, 16, 1, 1, true, true, 2"] == dict(vgpr=160, agpr=0, occ=2)
    # every direct-operator instantiation fits the budget of three waves per SIMD with registers to spare
    direct = {k: v for k, v in rec.items() if k.split(", ")[9] == "true"}
    assert direct and all(v["vgpr"] + v["agpr"] <= 168 for v in direct.values())


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="needs hipcc to cross-compile the pass kernels")
def test_every_instantiation_keeps_to_the_residency_it_states():
    r = subprocess.run(["make", "-C", ROOT, "check-pass-registers"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "pass registers: ok" in r.stdout
    assert " 0 failures" in r.stdout
