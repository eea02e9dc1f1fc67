"""The fixtures of tests/test_gpu_kkt_shard.py that carry low-rank lists, checked without a GPU: the verdict the library must
report (C = Delta^-1 - U^T K~^-1 U positive definite, tests/kkt_shard_ref.py) equals the inertia numpy's eigvalsh finds for the
unmodified matrix K (nv M positive, ns M negative eigenvalues), and no verdict hinges on rounding: every eigenvalue of C is away
from zero by more than 1e-6 of the largest.  The seeds in kkt_shard_ref were chosen so that this holds."""
import numpy as np
import pytest

import kkt_shard_ref as S


@pytest.fixture(scope="module")
def D33_24(built):
    import etol_amd as E
    return {M: E.lgl(M)[2] for M in (S.LR_M, S.BLK["M"])}


def _away_from_zero(lam):
    return np.abs(lam).min() > 1e-6 * np.abs(lam).max()


@pytest.mark.parametrize("which", ["LR_VERDICTS", "LR_MASKS"])
def test_list_fixtures_have_the_verdict_of_the_inertia(D33_24, which):
    D = D33_24[S.LR_M]
    fx = S.lr_fixture(D, getattr(S, which))
    M, ns, nv = fx["M"], fx["ns"], fx["nv"]
    exp = S.expected_exact(D, fx, S.LR_DC)
    want = {None: 1, S.EXACT_SCALE: 1, S.INEXACT_SCALE: 0, "over": 0}
    assert [e[0] for e in exp] == [want[k] for k in fx["kinds"]]
    for b, (exact, lam) in enumerate(exp):
        Kt = S.matrix(D, fx, b, S.LR_DC)
        assert np.allclose(Kt, Kt.T) and S.inertia_ok(Kt, M, ns, nv)
        # lists as the device writes them: ordered by node, -1 / nan behind min(count, max_mods)
        n = min(int(fx["count"][b]), fx["max_mods"])
        assert (np.diff(fx["node"][b, :n]) >= 0).all() and (fx["node"][b, n:] == -1).all()
        assert np.isnan(fx["delta"][b, n:]).all() and np.isnan(fx["vec"][b, n:]).all()
        if lam is None:
            continue
        assert _away_from_zero(lam), (b, lam.min(), lam.max())
        r = int(fx["count"][b])
        K = S.unmodified(Kt, S.columns(fx, b, fx["node"][b], fx["vec"][b], r), fx["delta"][b, :r])
        assert S.inertia_ok(K, M, ns, nv) == bool(exact), b


def test_blocks_fixture_has_the_verdict_of_the_inertia(D33_24):
    """the blocks with reflected eigenvalues: K from the assembled blocks, K~ and the lists by numpy's eigh"""
    D = D33_24[S.BLK["M"]]
    case = S.blocks_fixture(D)
    M, ns, nv, B = case["M"], case["ns"], case["nv"], case["B"]
    Qx, Qt, lists = S.blocks_lists_numpy(case)
    fx = dict(M=M, ns=ns, nv=nv, B=B, Q=Qt, VALS=case["VALS"], fixed=case["fixed"])
    for b in range(B):
        node, delta, vec = lists[b]
        assert len(node) > 0
        Kt = S.matrix(D, fx, b, S.LR_DC)
        assert S.inertia_ok(Kt, M, ns, nv)
        U = S.columns(fx, b, node, vec, len(node))
        K = S.unmodified(Kt, U, delta)
        assert np.abs(K - S.matrix(D, fx, b, S.LR_DC, Q=Qx[b])).max() < 1e-9 * np.abs(K).max()      # the lists undo the fix
        ok, lam = S.verdict(Kt, U, delta)
        assert _away_from_zero(lam), (b, lam.min(), lam.max())
        assert ok == S.inertia_ok(K, M, ns, nv), b
