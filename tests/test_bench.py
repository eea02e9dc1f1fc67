"""bench.py: the plain run (headline only, --steps timed steps) and --dump-outputs.  The dump's sampling on the CPU; a plain
run on the GPU whose dumped outputs are checked against the CPU oracle (-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump(tmp_path, outs, first):
    import torch
    import bench
    d = str(tmp_path)
    bench.dump_outputs(d, outs, first, np, torch)
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("res", "vals", "cost", "instances")}


def _outs(torch, B, dtype):
    g = torch.Generator().manual_seed(3)
    return (torch.rand((B, 5, 16), generator=g, dtype=dtype), torch.rand((B, 9, 16), generator=g, dtype=dtype),
            torch.rand((B,), generator=g, dtype=dtype))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_dump_writes_every_instance_when_it_fits(tmp_path, dtype):
    import torch
    outs = _outs(torch, 12, getattr(torch, dtype))
    got = _dump(tmp_path, outs, 40)
    for name, t in zip(("res", "vals", "cost"), outs):
        assert got[name].dtype == np.dtype(dtype) and np.array_equal(got[name], t.numpy())
    assert got["instances"].dtype == np.float64 and np.array_equal(got["instances"], np.arange(40, 52))


def test_dump_of_a_large_output_is_a_fixed_seeded_sample_within_the_budget(tmp_path, monkeypatch):
    import torch
    import bench
    B = 64
    outs = _outs(torch, B, torch.float64)
    per = (5 + 9) * 16 * 8
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * per + 2 * 8 * B)
    a = _dump(tmp_path / "a", outs, 0)
    b = _dump(tmp_path / "b", outs, 0)
    idx = a["instances"].astype(int)
    assert len(idx) == 10 and np.all(np.diff(idx) > 0) and idx[-1] < B
    assert all(np.array_equal(a[n], b[n]) for n in a)                  # the same sample from run to run
    assert np.array_equal(a["res"], outs[0].numpy()[idx]) and np.array_equal(a["vals"], outs[1].numpy()[idx])
    assert np.array_equal(a["cost"], outs[2].numpy())                  # COST whole
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_what_the_last_step_computed(built, tmp_path):
    """`bench.py --gpus 1 --steps K` without --full: one line with the headline fields over exactly K timed steps and none of
    what --full adds; the outputs it dumps agree with the CPU oracle on instances of the sample (first, middle, last)."""
    import etol_amd as E
    from etol_amd import workloads as W
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--scenarios", "128",
           "--dump-outputs", str(d)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 7 and j["warmup"] == 2 and j["dtype"] == "f64" and j["unit"] == "node-evals/s" and j["higher_is_better"]
    assert j["value"] > 0 and abs(j["value"] - 128 * 1024 / (j["ms_per_step"] * 1e-3)) < 1e-6 * j["value"]
    assert not {"checked", "secondary", "cpu_baseline", "weak_scaling"} & set(j)
    got = {n: np.load(d / (n + ".npy")) for n in ("res", "vals", "cost", "instances")}
    assert sum(v.nbytes for v in got.values()) <= 64e6
    assert all(v.dtype == np.float64 for v in got.values()) and got["cost"].shape == (128,)
    inst = got["instances"].astype(int)
    assert got["res"].shape[0] == got["vals"].shape[0] == len(inst) and np.all(np.diff(inst) > 0)
    M = 1024
    pick = [0, len(inst) // 2, len(inst) - 1]
    runs = [W.quadrotor_batch(3, 1, M, 20, first_instance=int(inst[p])) for p in pick]
    X, U, recs = (np.concatenate([q[i] for q in runs]) for i in range(3))
    dumped = (got["res"][pick], got["vals"][pick], got["cost"][inst[pick]])
    e = O.sampled_errors(E.MODEL_QUADROTOR2D, W.QUAD_PARAMS, M, E.lgl(M), 0.0, W.TF, X, U, recs, dumped, range(len(pick)))
    assert e["defect"] < 5e-13 and e["path"] < 1e-13 and e["vals"] < 1e-13 and e["cost"] < 1e-13, e
