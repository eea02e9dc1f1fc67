"""Which VALS rows a model declares invariant (emi_invariant_rows: what a pass with EMI_EVAL_KEEP_INVARIANT does not store),
checked against the CPU oracle: a flagged row must not move when (X, U) does, an unflagged row must.  No GPU needed.

Rows are compared bit for bit, except that -0.0 counts as +0.0: the oracle takes every derivative by the complex-step method,
and the imaginary part of a product that does not contain the perturbed variable is a zero whose SIGN follows the signs of the
factors (u0 * u0 with the step on x: u0 * 0 + 0 * u0 = -0.0 for u0 < 0).  A structural zero of the oracle is therefore +0.0 at
one node and -0.0 at the next; the kernels write +0.0 (-0.0 when maximising) throughout."""
import numpy as np
import pytest

import oracle_lib as O

M, T0, TF, NP = 12, 0.5, 9.0, 2


def _sets(model):
    """three random (X, U) sets of one instance each, the model's parameters and two disc keep-outs"""
    from etol_amd import _lib as L
    from etol_amd import workloads as W
    if model == L.MODEL_POINTMASS2D:
        xs, params = [W.pointmass_batch(20 + s, 1, M) for s in range(3)], []
    elif model == L.MODEL_QUADROTOR2D:
        xs, params = [W.quadrotor_batch(20 + s, 1, M, 0)[:2] for s in range(3)], W.QUAD_PARAMS
    else:
        xs, params = [W.fixedwing_batch(20 + s, 1, M) for s in range(3)], W.FW_PARAMS
    recs = W.quadrotor_batch(20, 1, M, NP)[2][0]
    return xs, params, recs


@pytest.mark.parametrize("model", [0, 1, 2])
def test_flagged_rows_are_exactly_the_rows_the_oracle_leaves_unchanged(built, model):
    import etol_amd as E
    mask = E.invariant_rows(model, NP)
    ns, nc = O.MODEL_DIMS[model]
    assert mask.shape == (ns * (ns + nc) + 2 * NP + ns + nc,)
    xs, params, recs = _sets(model)
    mesh = O.lgl(M)
    vals = [O.evaluate(model, params, M, mesh, T0, TF, X, U, recs)[1][0] for X, U in xs]      # [nvals][M] each
    for r in range(mask.size):
        bits = [(v[r] + 0.0).view(np.uint64) for v in vals]            # (-0.0 + 0.0 = +0.0; every other value keeps its bits)
        same = all(np.array_equal(bits[0], b) for b in bits[1:])
        if mask[r]:
            assert same, f"model {model}: row {r} is flagged invariant and differs between two (X, U) sets"
        else:
            assert not same, f"model {model}: row {r} is not flagged and is the same for three random (X, U) sets"


def test_quadrotor_with_20_keep_outs_flags_50_rows(built):
    import etol_amd as E
    mask = E.invariant_rows(E.MODEL_QUADROTOR2D, 20)
    assert mask.size == 96 and mask.sum() == 50
    assert mask[:48].sum() == 44 and not mask[48:88].any() and mask[88:].sum() == 6
    varying = {3 * 8 + 2, 3 * 8 + 6, 4 * 8 + 2, 4 * 8 + 6, 88 + 6, 88 + 7}
    assert set(np.flatnonzero(~mask[:48])) | set(88 + np.flatnonzero(~mask[88:])) == varying


def test_argument_errors(built):
    import ctypes as C
    import etol_amd as E
    lib = E.load()
    n = C.c_int(-1)
    assert lib.emi_invariant_rows(E.MODEL_SOURCE, 0, None, C.byref(n)) != 0       # a traced model declares nothing: no mask to give
    assert lib.emi_invariant_rows(7, 0, None, C.byref(n)) != 0
    assert lib.emi_invariant_rows(E.MODEL_QUADROTOR2D, -1, None, C.byref(n)) != 0
    assert lib.emi_invariant_rows(E.MODEL_FIXEDWING12, 3, None, C.byref(n)) == 0 and n.value == 12 * 16 + 6 + 16


def test_record_bookkeeping_as_a_stand_alone_program_under_the_host_sanitizers(tmp_path):
    """The record emi_eval_dev consults (etol_amd/csrc/emi_keep_record.hpp) has no device in it: tests/harness/keep_record_main.cpp
    replays the call sequences of emi_api.hip and emi_api_pass.hip against it, built with -fsanitize=address,undefined (`make check-keep-record`)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-C", root, "check-keep-record", f"KEEP_CHECK_OUT={tmp_path / 'keep_record_check'}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "keep record: ok" in r.stdout
