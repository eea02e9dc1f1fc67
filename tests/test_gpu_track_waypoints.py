"""emi_set_track_waypoints, emi_tracks_from_waypoints_dev, emi_get_tracks: the centres of the track rows on the context's mesh from
waypoint tables kept on the device.  -m gpu

Reference: emi_track_centres per track at the node times t0 + h (tau_k + 1) recomputed in numpy (tests/track_ladder_ref.py:
host_centres), the route through the host that the device call replaces.  Every comparison is bit for bit: the kernel restates that
function's statements with contraction off and a true division, one thread per (set, track, node); an f32 context computes in
double and stores with the conversion emi_set_tracks applies."""
import ctypes as C

import numpy as np
import pytest

import track_ladder_ref as TR

pytestmark = pytest.mark.gpu

T0, TF = 0.5, 4.5
LD_WAY = 7
COUNTS = (2, 4, 7)
D_, I_ = TR.D_, TR.I_


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def tables(M, nsets, ntracks, seed=0):
    """Waypoint tables [nsets][ntracks][LD_WAY] with counts 2, 4, 7 in turn and NaN behind a track's count.  Row r = set * ntracks +
    track: r % 3 == 1 starts after t0, r % 3 == 2 ends before tf, the others span [t0, tf]; about half of the interior waypoint
    times are node times of the M-node mesh exactly (where it has interior nodes inside the table).  -> (ways, counts)"""
    rng = np.random.default_rng(1000 * M + 10 * nsets + ntracks + seed)
    nt = TR.node_times(M, T0, TF)
    ways, counts = [], np.zeros((nsets, ntracks), dtype=np.int32)
    for s in range(nsets):
        t, x, y = (np.full((ntracks, LD_WAY), np.nan) for _ in range(3))
        for k in range(ntracks):
            r = s * ntracks + k
            n = COUNTS[(r + seed) % 3]
            a = T0 + 0.3 if r % 3 == 1 else T0
            b = TF - 0.4 if r % 3 == 2 else TF
            inner = nt[(nt > a) & (nt < b)]
            pick = list(inner[np.linspace(0, len(inner) - 1, min(len(inner), (n - 2 + 1) // 2)).astype(int)]) if len(inner) and n > 2 else []
            pick = sorted(set(pick))
            while len(pick) < n - 2:
                v = float(rng.uniform(a, b))
                if v not in pick and a < v < b:
                    pick = sorted(pick + [v])
            tt = np.array([a] + pick[:n - 2] + [b])
            assert len(tt) == n and (np.diff(tt) > 0).all()
            t[k, :n], x[k, :n], y[k, :n] = tt, rng.uniform(0, 10, n), rng.uniform(0, 10, n)
            counts[s, k] = n
        ways.append((t, x, y))
    return ways, counts


def with_mesh(M, f32=False):
    import etol_amd as E
    ev = E.Evaluator(0, f32=f32)
    ev.set_mesh(M, T0, TF)
    assert np.array_equal(ev.node_t, TR.node_times(M, T0, TF))
    return ev


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (2, 9, 65, 300))
def test_the_device_route_gives_the_host_functions_bits(built, M):
    ev = with_mesh(M)
    nt = ev.node_t
    for nsets in (1, 3):
        for ntracks in (1, 3):
            ways, counts = tables(M, nsets, ntracks)
            t = np.stack([w[0] for w in ways])
            inner = t[np.isfinite(t) & (t > T0) & (t < TF)]
            if M >= 9 and nsets * ntracks >= 3:
                assert np.isin(inner, nt).any() and not np.isin(inner, nt).all()         # waypoints on node times, and off them
                assert np.nanmin(t[:, :, 0]) == T0 and np.nanmax(t[:, :, 0]) > T0           # a table that starts after t0
                assert min(np.nanmax(w[0][k]) for w in ways for k in range(ntracks)) < TF   # ... and one that ends before tf
            ev.set_track_waypoints(*TR.stacked(ways), counts=counts)
            ev.tracks_from_waypoints()
            xc, yc = ev.get_tracks()
            wx, wy = TR.host_centres(ways, M, T0, TF, counts)
            assert xc.shape == (nsets, ntracks, M) and np.isfinite(xc).all() and np.isfinite(yc).all(), (M, nsets, ntracks)     # no padding shows
            assert same(xc, wx) and same(yc, wy), (M, nsets, ntracks)
    # counts NULL: every track has ld waypoints
    ways, _ = tables(M, 2, 2, seed=2)
    full = [tuple(np.ascontiguousarray(a[:, :2]) for a in w) for w in ways]
    ev.set_track_waypoints(*TR.stacked(full))
    ev.tracks_from_waypoints()
    xc, yc = ev.get_tracks()
    wx, wy = TR.host_centres(full, M, T0, TF)
    assert same(xc, wx) and same(yc, wy)
    ev.close()


def test_an_f32_context_stores_the_rounded_double_centres(built):
    M = 9
    ev = with_mesh(M, f32=True)
    ways, counts = tables(M, 3, 3)
    ev.set_track_waypoints(*TR.stacked(ways), counts=counts)
    ev.tracks_from_waypoints()
    xc, yc = ev.get_tracks()
    wx, wy = TR.host_centres(ways, M, T0, TF, counts)
    assert same(xc, wx.astype(np.float32).astype(np.float64)) and same(yc, wy.astype(np.float32).astype(np.float64))
    ev.close()


# ---- 2. maps ---------------------------------------------------------------------------------------------------------------------------
def test_the_set_map_compacts_and_copies(built):
    import torch
    M, nsets, ntracks = 65, 3, 3
    ev = with_mesh(M)
    ways, counts = tables(M, nsets, ntracks)
    ev.set_track_waypoints(*TR.stacked(ways), counts=counts)
    wx, wy = TR.host_centres(ways, M, T0, TF, counts)
    for m in ([0, 1, 2], [2, 0, 1], [1, 1, 0, 2, 1], [2, 0], [1]):
        dm = torch.tensor(m, dtype=torch.int32, device=ev.device)
        torch.cuda.synchronize()
        ev.tracks_from_waypoints(dm)
        a = ev.get_tracks()
        ev.tracks_from_waypoints(dm)
        b = ev.get_tracks()
        assert a[0].shape == (len(m), ntracks, M), m
        assert same(a[0], wx[m]) and same(a[1], wy[m]), m                   # result set i has the bits of waypoint set map[i]
        assert same(a[0], b[0]) and same(a[1], b[1]), m                     # two calls
    ev.tracks_from_waypoints()                                             # no map: every set in order
    a = ev.get_tracks()
    assert same(a[0], wx) and same(a[1], wy)
    ev.close()


# ---- 3. the pass -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32,M", ((False, 33), (True, 9)), ids=("f64-33", "f32-9"))
def test_the_pass_reads_the_same_centres_by_either_route(built, f32, M):
    """point mass, one disc row and one track row, B = 3, waypoints per instance: emi_eval (EMI_EVAL_ALL) after the device route and
    after emi_set_tracks with the host centres"""
    import torch
    import etol_amd as E
    B = 3
    ev = with_mesh(M, f32=f32)
    ev.set_model(E.MODEL_POINTMASS2D)
    ev.set_batch(B)
    recs = np.zeros((B, 2, 8))
    for b in range(B):
        recs[b, 0, :4] = [1, 4.0 + 0.2 * b, 3.0, 0.8 ** 2]
        recs[b, 1, :3] = [2, 0, (0.6 + 0.1 * b) ** 2]
    ev.set_path(recs, 0, 1)
    ways, counts = tables(M, B, 1)
    rng = np.random.default_rng(5)
    s = (ev.tau + 1) / 2
    X = np.stack([np.stack([1 + 7 * s, 1 + 5 * s]) for _ in range(B)]) + 0.3 * rng.standard_normal((B, 2, M))
    U = rng.standard_normal((B, 2, M))
    Xd, Ud = (torch.from_numpy(a).to(ev.device, dtype=ev.dtype).contiguous() for a in (X, U))
    outs = []
    for route in ("device", "host"):
        if route == "device":
            ev.set_track_waypoints(*TR.stacked(ways), counts=counts)
            ev.tracks_from_waypoints()
        else:
            ev.set_tracks(*TR.host_centres(ways, M, T0, TF, counts))
        RES, VALS, COST = ev.alloc_outputs()
        RES.fill_(float("nan")); VALS.fill_(float("nan")); COST.fill_(float("nan"))
        torch.cuda.synchronize()
        ev.eval_dev(Xd, Ud, RES, VALS, COST, E.EVAL_ALL)
        ev.synchronize()
        outs.append(tuple(t.cpu().numpy() for t in (RES, VALS, COST)))
    for name, a, b in zip(("RES", "VALS", "COST"), *outs):
        assert np.isfinite(a).all(), name
        assert same(a, b), name
    ns = ev.layout.ns
    assert np.ptp(outs[0][0][:, ns + 1], axis=1).min() > 0                  # the track row does vary over the nodes
    ev.close()


# ---- 4. life cycle ---------------------------------------------------------------------------------------------------------------------
def test_waypoints_outlive_the_mesh_and_the_centres_do_not(built):
    import etol_amd as E
    lib = E.load()
    ev = E.Evaluator(0)
    ways, counts = tables(9, 2, 2)
    ev.set_track_waypoints(*TR.stacked(ways), counts=counts)              # needs no mesh
    ev.set_mesh(9, T0, TF)
    ev.tracks_from_waypoints()
    a = ev.get_tracks()
    w9 = TR.host_centres(ways, 9, T0, TF, counts)
    assert same(a[0], w9[0]) and same(a[1], w9[1])
    ev.set_mesh(17, T0, TF)
    ev.set_model(E.MODEL_POINTMASS2D)
    ev.set_batch(2)
    buf = np.zeros(2 * 2 * 17)
    assert lib.emi_get_tracks(ev.ctx, buf.ctypes.data_as(D_), buf.ctypes.data_as(D_)) == 2         # the centres went with the mesh
    with pytest.raises(E.EmiError):
        ev.get_tracks()
    ev.tracks_from_waypoints()                                             # ... one call brings them back, on the new mesh
    a = ev.get_tracks()
    w17 = TR.host_centres(ways, 17, T0, TF, counts)
    assert a[0].shape == (2, 2, 17) and same(a[0], w17[0]) and same(a[1], w17[1])
    # emi_set_tracks replaces the centres and leaves the waypoints
    other = (np.arange(17.0).reshape(1, 1, 17), -np.arange(17.0).reshape(1, 1, 17))
    ev.set_tracks(*other)
    a = ev.get_tracks()
    assert same(a[0], other[0]) and same(a[1], other[1])
    ev.tracks_from_waypoints()
    a = ev.get_tracks()
    assert same(a[0], w17[0]) and same(a[1], w17[1])
    # a refused table leaves the one held
    t, x, y = TR.stacked(ways)
    bad = t.copy()
    bad[1, 0, 1] = bad[1, 0, 0]
    assert lib.emi_set_track_waypoints(ev.ctx, 2, 2, LD_WAY, counts.ctypes.data_as(I_), bad.ctypes.data_as(D_), x.ctypes.data_as(D_),
                                       y.ctypes.data_as(D_)) == 1
    ev.tracks_from_waypoints()
    a = ev.get_tracks()
    assert same(a[0], w17[0]) and same(a[1], w17[1])
    # ntracks = 0 drops them
    assert lib.emi_set_track_waypoints(ev.ctx, 0, 0, 0, None, None, None, None) == 0
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, 0, None) == 2
    a = ev.get_tracks()                                                    # (the centres are the context's until the mesh changes)
    assert same(a[0], w17[0])
    ev.close()


# ---- 5. statuses -----------------------------------------------------------------------------------------------------------------------
def test_statuses(built):
    import torch
    import etol_amd as E
    lib = E.load()
    ways, counts = tables(9, 3, 2)
    t, x, y = TR.stacked(ways)
    dp = lambda a: a.ctypes.data_as(D_)
    ip = lambda a: a.ctypes.data_as(I_)
    buf = np.zeros(3 * 2 * 9)

    def set_way(ev, cnt=counts, tt=t, xx=x, yy=y, ld=LD_WAY):
        return lib.emi_set_track_waypoints(ev.ctx, 2, 3, ld, ip(cnt) if cnt is not None else None, dp(tt) if tt is not None else None,
                                           dp(xx) if xx is not None else None, dp(yy) if yy is not None else None)

    ev = E.Evaluator(0)
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, 0, None) == 2          # EMI_ERR_STATE: no mesh (and no waypoints)
    assert set_way(ev) == 0
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, 0, None) == 2          # no mesh
    assert lib.emi_get_tracks(ev.ctx, dp(buf), dp(buf)) == 2
    ev.close()
    ev = E.Evaluator(0)
    ev.set_mesh(9, T0, TF)
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, 0, None) == 2          # no waypoints
    assert lib.emi_get_tracks(ev.ctx, dp(buf), dp(buf)) == 2                # no centres
    for value, where in ((1, (0, 0)), (LD_WAY + 1, (2, 1)), (0, (1, 1))):
        cnt = counts.copy()
        cnt[where] = value
        assert set_way(ev, cnt=cnt) == 1, value                             # EMI_ERR_ARG: a count outside 2 .. ld
        assert f"set {where[0]}, track {where[1]}" in lib.emi_last_error(ev.ctx).decode()
    s, k = 1, 0
    assert counts[s, k] >= 4
    for kind in ("equal", "descending"):
        bad = t.copy()
        bad[s, k, 2] = bad[s, k, 1] if kind == "equal" else bad[s, k, 1] - 0.1
        assert set_way(ev, tt=bad) == 1, kind
        assert f"set {s}, track {k}" in lib.emi_last_error(ev.ctx).decode(), lib.emi_last_error(ev.ctx)
    bad = t.copy()
    bad[0, 0, 1] = np.nan                                                   # (inside the count: not ascending either)
    assert set_way(ev, tt=bad) == 1
    for drop in ("tt", "xx", "yy"):
        assert set_way(ev, **{drop: None}) == 1, drop                      # a NULL table
    assert set_way(ev, ld=1) == 1
    assert lib.emi_set_track_waypoints(ev.ctx, -1, 3, LD_WAY, ip(counts), dp(t), dp(x), dp(y)) == 1
    assert lib.emi_set_track_waypoints(ev.ctx, 2, 0, LD_WAY, ip(counts), dp(t), dp(x), dp(y)) == 1
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, 0, None) == 2          # nothing of the above was kept
    assert set_way(ev) == 0
    m = torch.tensor([0, 2], dtype=torch.int32, device=ev.device)
    torch.cuda.synchronize()
    p = C.c_void_p(m.data_ptr())
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, 2, None) == 1          # n other than 0 or nsets with a NULL map
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, -1, None) == 1 and lib.emi_tracks_from_waypoints_dev(ev.ctx, -1, p) == 1
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, 0, p) == 1             # a map of nothing
    assert lib.emi_get_tracks(ev.ctx, dp(buf), dp(buf)) == 2                # still none
    assert lib.emi_tracks_from_waypoints_dev(ev.ctx, 3, None) == 0 and lib.emi_tracks_from_waypoints_dev(ev.ctx, 2, p) == 0
    assert lib.emi_get_tracks(ev.ctx, None, dp(buf)) == 1 and lib.emi_get_tracks(ev.ctx, dp(buf), dp(buf)) == 0
    # the batch need not match when the centres are made; the next evaluation says so
    ev.set_model(E.MODEL_POINTMASS2D)
    ev.set_batch(3)
    X = torch.zeros((3, 2, 9), dtype=torch.float64, device=ev.device)
    RES, VALS, COST = ev.alloc_outputs()
    torch.cuda.synchronize()
    q = lambda a: C.c_void_p(a.data_ptr())
    assert lib.emi_eval_dev(ev.ctx, q(X), q(X), q(RES), q(VALS), q(COST), E.EVAL_ALL) == 2
    assert b"track table has 2 sets, batch is 3" in lib.emi_last_error(ev.ctx)
    ev.synchronize()
    ev.close()
