"""emi_hess_kernel in fp64 against the exact reference of tests/hess_ref.py, element by element.  -m gpu

Every check is |H - Href| <= K u (T + 1) per (instance, slot, node), u = 2^-53, T the sum of the magnitudes of the terms added into
the entry and K = hess_ref.K, derived from the host-compiled model structs (tests/test_hessian_ref_cpu.py); entries with T == 0 must
be exactly zero; the worst ratio and its position are printed (pytest -s).  Every result is taken twice: hess_host, and hess_dev
into a buffer that held a NaN bit pattern in every word, which must be overwritten everywhere and give hess_host's bits.
The inputs are fixture points (tests/golden/hessian_terms.npz) laid out as [B][M] by index; the mesh is the oracle's.

Models with delays stay with tests/test_gpu_delay_values.py (the Hessian of a context with delays: the bits of a context without
them on the extended controls) and tests/test_gpu_delays.py, the traced path rows of generated models with tests/test_gpu_traced.py.
"""
import numpy as np
import pytest

import hess_ref as HR
import oracle_lib as O
from etol_amd import workloads as W
from test_gpu_parity import check as check_eval
from test_gpu_traced import traced_source

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF8123456789ABC           # a quiet NaN with a payload nothing computes
PARAMS = {0: [], 1: W.QUAD_PARAMS, 2: W.FW_PARAMS}
NAMES = {0: "point mass", 1: "quadrotor", 2: "fixed wing"}
T0, TF = 0.5, 9.0                       # h = 4.25
_OPEN = []
_MESH = {}


@pytest.fixture(autouse=True)
def close_evaluators():
    yield
    while _OPEN:
        _OPEN.pop().close()


def mesh(M):
    if M not in _MESH:
        _MESH[M] = O.lgl(M)
    return _MESH[M]


def make_ev(model, M, B, recs=None, tracks=None, px=0, py=1, maximize=False, traced=False):
    import etol_amd as E
    ev = E.Evaluator(0)
    _OPEN.append(ev)
    ev.set_mesh(M, T0, TF, mesh=mesh(M))
    if traced:
        assert model == 1
        ev.set_model_source("TracedModel", traced_source(0), 6, 2, maximize=maximize)
    else:
        ev.set_model(model, PARAMS[model], maximize=maximize)
    ev.set_batch(B)
    if tracks is not None:
        ev.set_tracks(*tracks)
    if recs is not None:
        ev.set_path(recs, px, py)
    return ev


def device_hessian(ev, X, U, lamF, lamC, sigma):
    """hess_host, and hess_dev into a poisoned buffer: all of it written, the same bits"""
    import torch
    lay = ev.layout
    H = ev.hess_host(X, U, lamF, lamC, sigma=sigma)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(ev.device)
    dX, dU, dF = dev(X), dev(U), dev(lamF)
    dC = dev(lamC) if lamC is not None and lamC.shape[1] else None
    dH = torch.full((lay.B, lay.nhess, lay.M), NAN_BITS, dtype=torch.int64, device=ev.device)
    torch.cuda.synchronize()             # the fill and the copies run on torch's stream, the evaluator launches on its own
    ev.hess_dev(dX, dU, dF, dC, sigma, dH.view(torch.float64))
    ev.synchronize()
    bits = dH.cpu().numpy()
    assert not (bits == np.int64(NAN_BITS)).any() and not np.isnan(bits.view(np.float64)).any()
    assert np.array_equal(bits, H.view(np.int64))
    return H


def run(what, model, idx, recs=None, tracks=None, px=0, py=1, maximize=False, traced=False, sigma=HR.SIGMA, lam=None, seed=11):
    """-> (H, Href, T) of one case, checked"""
    idx = np.asarray(idx)
    B, M = idx.shape
    npth = 0 if recs is None else np.asarray(recs).shape[-2]
    lamF, lamC = lam if lam is not None else HR.multipliers(B, HR.NS[model], npth, M, seed)
    X, U = HR.points(model, idx)
    ev = make_ev(model, M, B, recs, tracks, px, py, maximize, traced)
    H = device_hessian(ev, X, U, lamF, lamC if npth else None, sigma)
    Href, T = HR.reference(model, idx, mesh(M)[1], T0, TF, sigma, maximize, lamF, lamC, recs, tracks, px, py)
    HR.check(what, H, Href, T)
    return H, Href, T


def edge_heavy(model, B, M):
    """[B][M] fixture rows ending with the model's last row: small meshes get the edge points, large ones every point"""
    n = HR.npoints(model)
    return HR.cycle(model, B, M, start=(n - B * M) % n)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (2, 33, 256, 257))
@pytest.mark.parametrize("model", (0, 1, 2))
def test_models_and_meshes(built, model, M):
    """The three built-in models, three instances: the smallest mesh, an odd one, exactly one thread block of nodes, and one live
    thread in a second block."""
    H, Href, _ = run(f"{NAMES[model]} M={M}", model, edge_heavy(model, 3, M))
    assert np.abs(Href).max() > 0


@pytest.mark.parametrize("shared", (False, True))
def test_quadrotor_mixed_record_tables(built, shared):
    """Five rows per instance, ellipses, discs and a track in another order in each table: a wrong set or row stride puts another
    kind's curvature, or another instance's ellipse, into the entry.  Then one table shared by the batch."""
    M = 33
    recs = HR.mixed_tables()
    recs = recs[1] if shared else recs
    H, Href, T = run(f"quadrotor, {'one shared table' if shared else 'a table per instance'}", 1, HR.cycle(1, 3, M, start=40), recs,
                     HR.track_centres(M))
    qxx, qyy, qxy = HR.path_slots(0, 1)
    assert (np.abs(Href[:, [qxx, qyy, qxy]]) > 0).all()
    if not shared:      # the tables differ where it matters: the reference of instance 0 with instance 1's table is far outside the bound
        lamF, lamC = HR.multipliers(3, 6, 5, M)
        other, _ = HR.reference(1, HR.cycle(1, 3, M, start=40), mesh(M)[1], T0, TF, HR.SIGMA, False, lamF, lamC, recs[[1, 2, 0]],
                                HR.track_centres(M))
        assert (np.abs(other - Href)[:, [qxx, qyy, qxy]].max(axis=(1, 2)) > 1e6 * HR.K * HR.U64 * (T.max() + 1)).all()


@pytest.mark.parametrize("model,px,py", [(1, 0, 1), (1, 3, 4), (1, 4, 3), (0, 1, 0)])
def test_path_states(built, model, px, py):
    """Path rows on other states than (0, 1), and px > py: the xy slot is hi (hi + 1) / 2 + lo, xx and yy follow px and py."""
    M = 33
    recs = HR.mixed_tables()[0]
    H, Href, T = run(f"{NAMES[model]} path states ({px}, {py})", model, HR.cycle(model, 2, M, start=7), recs, HR.track_centres(M), px, py)
    qxx, qyy, qxy = HR.path_slots(px, py)
    assert (np.abs(H[:, [qxx, qyy, qxy]]) > 0).all()
    if px > py:         # xx and yy are not interchangeable here: the swapped reference is far outside the bound
        lamF, lamC = HR.multipliers(2, HR.NS[model], 5, M)
        swapped, _ = HR.reference(model, HR.cycle(model, 2, M, start=7), mesh(M)[1], T0, TF, HR.SIGMA, False, lamF, lamC, recs,
                                  HR.track_centres(M), py, px)
        assert np.abs(swapped - Href).max() > 1e6 * HR.K * HR.U64 * (T.max() + 1)


def test_evaluation_with_path_states_4_3(built):
    """Companion: one evaluation pass with (px, py) = (4, 3) against the oracle (the parity tests evaluate at (3, 4) only)."""
    M, B = 33, 2
    recs, tracks = HR.mixed_tables()[0], HR.track_centres(M)
    X, U = HR.points(1, HR.cycle(1, B, M, start=7))
    ev = make_ev(1, M, B, recs, tracks, 4, 3)
    got = ev.eval_host(X, U)
    ref = O.evaluate(1, PARAMS[1], M, mesh(M), T0, TF, X, U, recs, tracks, px=4, py=3)
    check_eval(dict(X=X), ev, got, ref)


def test_maximize_flips_the_cost_term_only(built):
    """H of a maximising context is the reference with sgn = -1; with sigma = 0 it is the minimising context's H bit for bit."""
    M = 33
    idx = HR.cycle(1, 3, M, start=100)
    recs, tracks = HR.mixed_tables(), HR.track_centres(M)
    Hmax, Href, _ = run("quadrotor, maximize", 1, idx, recs, tracks, maximize=True)
    Hmin, Hrefmin, _ = run("quadrotor, minimize", 1, idx, recs, tracks, maximize=False)
    costs = [6 * 7 // 2 + 6, 7 * 8 // 2 + 7]                      # (T, T) and (tau, tau): L_zz lives there and nowhere else
    rest = [q for q in range(36) if q not in costs]
    assert np.array_equal(Hmax[:, rest], Hmin[:, rest]) and np.array_equal(Hmax[:, costs], -Hmin[:, costs])
    assert (Hrefmin[:, costs] > 0).all() and (Href[:, costs] < 0).all()
    H0max, _, _ = run("quadrotor, maximize, sigma = 0", 1, idx, recs, tracks, maximize=True, sigma=0.0)
    H0min, _, _ = run("quadrotor, minimize, sigma = 0", 1, idx, recs, tracks, maximize=False, sigma=0.0)
    assert np.array_equal(H0max.view(np.int64), H0min.view(np.int64))
    # the fixed wing's cost term sits on four slots
    idx = HR.cycle(2, 3, M, start=30)
    Hmax, _, _ = run("fixed wing, maximize", 2, idx, maximize=True)
    Hmin, _, _ = run("fixed wing, minimize", 2, idx, maximize=False)
    costs = [v * (v + 1) // 2 + v for v in (12, 13, 14, 15)]
    rest = [q for q in range(136) if q not in costs]
    assert np.array_equal(Hmax[:, rest], Hmin[:, rest]) and np.array_equal(Hmax[:, costs], -Hmin[:, costs])


@pytest.mark.parametrize("model", (1, 2))
def test_degenerate_multipliers(built, model):
    """All multipliers zero and sigma = 0: every entry is zero.  lamF = 0 and sigma = 0 with records: the three path slots alone."""
    M, B = 33, 3
    idx = edge_heavy(model, B, M)
    ns = HR.NS[model]
    recs, tracks = HR.mixed_tables(), HR.track_centres(M)
    zero = (np.zeros((B, ns, M)), np.zeros((B, 5, M)))
    H, _, T = run(f"{NAMES[model]}, no multipliers", model, idx, recs, tracks, 1, 0, sigma=0.0, lam=zero)
    assert (T == 0).all() and (H == 0).all()
    lam = (np.zeros((B, ns, M)), HR.multipliers(B, ns, 5, M)[1])
    H, _, T = run(f"{NAMES[model]}, path multipliers only", model, idx, recs, tracks, 1, 0, sigma=0.0, lam=lam)
    slots = list(HR.path_slots(1, 0))
    rest = [q for q in range(H.shape[1]) if q not in slots]
    assert (H[:, rest] == 0).all() and (np.abs(H[:, slots]) > 0).all()


@pytest.mark.parametrize("M", (33, 257))
def test_traced_quadrotor_twin(built, M):
    """The quadrotor as a run-time compiled model (generated second derivatives), held to the bound of the built-in one."""
    import etol_amd as E
    idx = edge_heavy(1, 3, M)
    recs, tracks = HR.mixed_tables(), HR.track_centres(M)
    run(f"traced quadrotor M={M}", 1, idx, recs, tracks, traced=True)
    assert _OPEN[-1].layout.model == E.MODEL_SOURCE
