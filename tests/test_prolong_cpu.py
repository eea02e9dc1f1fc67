"""emi_prolong_matrix (host) against the Lagrange basis from mpmath, and the numpy restatement of repair_guess against the host
function.  No GPU needed.

The matrix: unit rows at coincident nodes, row sums, and every entry within PROLONG_GATE 2^-53 sum_j |P*_qj| of the fixture
(tests/golden/prolong_matrices.npz, tests/golden/gen_prolong_golden.py).  The gate is the largest ratio measured over the six pairs,
rounded up to the next power of two (tests/ladder_ref.py).  What it covers: the nodes and weights of emi_lgl are rounded doubles,
and near the ends of a mesh, where neighbouring nodes lie ~ 1 / M^2 apart, a rounding of a node moves tau_f - tau_c by a relative
~ M^2 eps; so do the square roots of the weights used in place of the exact barycentric weights.

repair_guess: the host library is built with contraction allowed, the restatement rounds every operation, so the two are compared
to a bound, not bit for bit: a node is moved to the level 1.05 of a keep-out's quadratic form by at most 50 sweeps over the rows,
each a dozen rounded operations on values of the size of the coordinates: 64 eps max(1, |coordinate|) per sweep taken holds them
together as long as both take the same branches (the inputs keep the quadratic forms away from the thresholds).  The kernel is
held to the restatement bit for bit (tests/test_gpu_ladder.py)."""
import numpy as np
import pytest

import ladder_ref as LD

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return LD.prolong_fixture()


def test_prolong_matrix_against_mpmath(built, golden):
    import etol_amd as E
    worst = 0.0
    for mc, mf in LD.PAIRS:
        P = E.Evaluator.prolong_matrix(mc, mf)
        Ps = golden[(mc, mf)]
        assert P.shape == Ps.shape == (mf, mc)
        unit = [0, mf - 1] + ([mf // 2] if mc % 2 and mf % 2 else [])
        where = [0, mc - 1] + ([mc // 2] if mc % 2 and mf % 2 else [])
        for q, j in zip(unit, where):
            e = np.zeros(mc)
            e[j] = 1.0
            assert np.array_equal(P[q], e) and np.array_equal(Ps[q], e), (mc, mf, q)
        assert np.abs(P.sum(1) - 1.0).max() <= mc * 2.0 ** -52, (mc, mf, np.abs(P.sum(1) - 1.0).max())
        leb = np.abs(Ps).sum(1, keepdims=True)
        ratio = (np.abs(P - Ps) / (2.0 ** -53 * leb)).max()
        worst = max(worst, ratio)
        print(f"({mc}, {mf}): largest |P - P*| / (2^-53 Lebesgue function) = {ratio:.1f}; row sums within {np.abs(P.sum(1) - 1).max():.2e}")
        assert ratio <= LD.PROLONG_GATE, (mc, mf, ratio)
    print(f"largest ratio over the pairs: {worst:.1f} (gate {LD.PROLONG_GATE:g})")
    # the numpy restatement of the tests' CPU ladder is the same matrix to rounding
    tc, wc, _ = E.lgl(21)
    assert np.abs(LD.bary_matrix(tc, wc, E.lgl(41)[0]) - E.Evaluator.prolong_matrix(21, 41)).max() < 64 * EPS
    lib = E.load()
    assert lib.emi_prolong_matrix(1, None, None, 3, None, None) == 1 and lib.emi_prolong_matrix(3, None, None, 3, None, None) == 1


def test_any_pair_of_node_sets(built):
    """not only Mf = 2 Mc - 1, and not only LGL targets: polynomials up to the coarse degree are reproduced at arbitrary points"""
    import etol_amd as E
    tc, wc, _ = E.lgl(12)
    pts = np.array([-1.0, -0.93, -0.2, 0.0, 0.456, 1.0])
    P = E.Evaluator.prolong_matrix(12, len(pts), fine=(pts,))
    for p in range(12):
        assert np.abs(P @ tc ** p - pts ** p).max() < 1e-13, p
    Pd = E.Evaluator.prolong_matrix(9, 5)                      # downwards
    assert np.abs(Pd @ E.lgl(9)[0] ** 3 - E.lgl(5)[0] ** 3).max() < 1e-14


@pytest.mark.parametrize("M", (9, 41))
@pytest.mark.parametrize("per_instance", (False, True))
def test_repair_restatement_against_the_host_function(built, M, per_instance):
    h = LD.load_harness()
    for with_track in (False, True):
        c = LD.repair_case(M, per_instance=per_instance, with_track=with_track)
        want = LD.repair_host(h, c)
        got, sweeps = LD.repair_ref(c["X"], c["recs"], tracks=c["tracks"])
        moved = (want[:, :2] != c["X"][:, :2]).any(1)
        print(f"M {M} per instance {per_instance} track {with_track}: {int(moved.sum())} nodes moved, {sweeps} sweeps, "
              f"largest difference {np.abs(got - want).max():.2e}")
        assert sweeps >= 2 and moved.sum() >= 3
        assert np.array_equal((got[:, :2] != c["X"][:, :2]).any(1), moved)
        assert not moved[:, 0].any() and not moved[:, -1].any()                   # end nodes, though inside a disc
        assert np.array_equal(got[:, 2:].view(np.uint8), c["X"][:, 2:].view(np.uint8))
        assert np.abs(got - want).max() <= 64 * EPS * max(sweeps, 1) * max(1.0, np.abs(want[:, :2]).max())
        # every interior node ends outside every keep-out it can be outside of: the form is at least 1.025 or the sweeps ran out
        again, more = LD.repair_ref(got, c["recs"], tracks=c["tracks"])
        assert sweeps < 50 and more == 0 and np.array_equal(again, got)
        if not with_track:
            assert moved[0, c["kc"]]                                                # the node on the dead centre
