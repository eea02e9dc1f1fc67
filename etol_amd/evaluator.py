"""Host-side Python mirror of the eMI355X evaluator (thin wrapper over the C ABI).

PyTorch is used only as plumbing: device allocations (torch tensors whose
data_ptr() is handed to the C ABI) and torch.distributed.  All arithmetic runs
in the HIP kernels of libemi355x.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def lgl(M):
    """LGL nodes, weights and differentiation matrix (host, emi_lgl)."""
    lib = L.load()
    tau = np.empty(M)
    w = np.empty(M)
    D = np.empty((M, M))
    L.check(lib.emi_lgl(M, _dp(tau), _dp(w), _dp(D)), what="emi_lgl")
    return tau, w, D


def model_dims(model):
    lib = L.load()
    ns, nc, npar = C.c_int(), C.c_int(), C.c_int()
    L.check(lib.emi_model_dims(model, C.byref(ns), C.byref(nc), C.byref(npar)), what="emi_model_dims")
    return ns.value, nc.value, npar.value


def edge_ellipse(xa, ya, xb, yb):
    lib = L.load()
    rec = np.zeros(L.PATH_REC)
    L.check(lib.emi_edge_ellipse(xa, ya, xb, yb, _dp(rec)), what="emi_edge_ellipse")
    return rec


def track_centres(t, x, y, node_t):
    lib = L.load()
    t, x, y, node_t = (np.ascontiguousarray(v, dtype=np.float64) for v in (t, x, y, node_t))
    xc, yc = np.empty(len(node_t)), np.empty(len(node_t))
    L.check(lib.emi_track_centres(len(t), _dp(t), _dp(x), _dp(y), len(node_t), _dp(node_t), _dp(xc), _dp(yc)),
            what="emi_track_centres")
    return xc, yc


def invariant_rows(model, np_rows=0):
    """Which VALS rows of a built-in model with np_rows table rows do not depend on (X, U): bool array [nvals]
    (host, emi_invariant_rows)."""
    lib = L.load()
    n = C.c_int()
    L.check(lib.emi_invariant_rows(int(model), int(np_rows), None, C.byref(n)), what="emi_invariant_rows")
    mask = np.zeros(n.value, dtype=np.uint8)
    L.check(lib.emi_invariant_rows(int(model), int(np_rows), mask.ctypes.data_as(C.POINTER(C.c_ubyte)), None), what="emi_invariant_rows")
    return mask.astype(bool)


def plan_route(recs, ends, tau, box=None, clearance=0.01, grid=0):
    """The route of emi_plan_route (host) from (ends[0], ends[1]) to (ends[2], ends[3]) past the static records recs [np][PATH_REC],
    resampled at the node abscissae tau: (xs, ys, level, cost, cells); xs, ys are None and cells is empty without a route
    (level -1: none at any grow of the keep-outs, -2: nothing to plan)."""
    lib = L.load()
    recs = np.ascontiguousarray(recs, dtype=np.float64).reshape(-1, L.PATH_REC)
    ends, tau = (np.ascontiguousarray(a, dtype=np.float64) for a in (ends, tau))
    assert ends.shape == (4,)
    bx = None if box is None else np.ascontiguousarray(box, dtype=np.float64)
    N = int(grid) if grid else 161
    xs, ys, cells = np.empty(len(tau)), np.empty(len(tau)), np.empty(max(N * N, 1), dtype=np.int32)
    level, ncells, cost = C.c_int(), C.c_int(), C.c_double()
    L.check(lib.emi_plan_route(len(recs), _dp(recs) if recs.size else None, _dp(ends), _dp(bx) if bx is not None else None, float(clearance),
                               int(grid), len(tau), _dp(tau), _dp(xs), _dp(ys), C.byref(level), C.byref(cost),
                               cells.ctypes.data_as(C.POINTER(C.c_int)), C.byref(ncells)), what="emi_plan_route")
    if level.value < 0:
        return None, None, level.value, 0.0, cells[:0]
    return xs, ys, level.value, cost.value, cells[:ncells.value].copy()


class Evaluator:
    """One libemi355x context: mesh + model + batch, evaluated on one GPU."""

    def __init__(self, device=0, f32=False):
        self.lib = L.load()
        self.ctx = C.c_void_p()
        self.f32 = bool(f32)
        create = self.lib.emi_create_f32 if f32 else self.lib.emi_create
        L.check(create(int(device), C.byref(self.ctx)), what="emi_create")
        self.device = torch.device("cuda", int(device))
        self.dtype = torch.float32 if f32 else torch.float64
        self._keep = []
        self._lay = None        # cached emi_get_layout / emi_get_delays answers: eval_dev is the timed call of bench.py and of any
        self._nd = None         # batched user, and two ctypes round trips per pass show at 14 - 20 us passes; reset by every set_*
        self._kept = None       # the VALS tensor eval_dev last ran a full Jacobian pass into (held: its address cannot be recycled) ...
        self._kept_version = -1  # ... and its torch version counter then: any torch write to it since shows as another value
        self._wp_shape = None   # (sets, tracks) of the waypoint tables the context holds ...
        self._trk_shape = None  # ... and of its centres on the present mesh (emi_get_tracks takes arrays of that size on trust)

    def _changed(self):
        self._lay = None
        self._nd = None

    def close(self):
        self._kept = None
        if self.ctx:
            self.lib.emi_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st, what):
        L.check(st, self.ctx, what)

    # ---- problem definition -------------------------------------------------
    def set_mesh(self, M, t0, tf, mesh=None):
        tau, w, D = mesh if mesh is not None else lgl(M)
        self.tau, self.w, self.D = (np.ascontiguousarray(a, dtype=np.float64) for a in (tau, w, D))
        self._ck(self.lib.emi_set_mesh(self.ctx, M, _dp(self.tau), _dp(self.w), _dp(self.D), t0, tf), "emi_set_mesh")
        self._changed()
        self._trk_shape = None
        self.node_t = t0 + (tf - t0) / 2.0 * (self.tau + 1.0)

    def set_model(self, model, params=(), maximize=False):
        p = np.ascontiguousarray(params, dtype=np.float64)
        self._ck(self.lib.emi_set_model(self.ctx, model, _dp(p) if p.size else None, p.size, int(maximize)),
                 "emi_set_model")
        self._changed()

    def set_model_source(self, struct_name, source, ns, nc, params=(), maximize=False, npath=0, path_vars=()):
        """Install a model given as the text of a model struct (compiled for gfx950 here).  npath rows traced from
        constraint callbacks depend on the node variables path_vars (ascending; states first, then controls)."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        pv = np.ascontiguousarray(path_vars, dtype=np.int32)
        self._ck(self.lib.emi_set_model_source(self.ctx, struct_name.encode(), source.encode(), ns, nc, npath,
                                               pv.ctypes.data_as(C.POINTER(C.c_int)) if pv.size else None, pv.size,
                                               _dp(p) if p.size else None, p.size, int(maximize)),
                 "emi_set_model_source")
        self._changed()

    def set_batch(self, B):
        self._ck(self.lib.emi_set_batch(self.ctx, B), "emi_set_batch")
        self._changed()

    def set_model_params(self, table):
        """Per-instance model parameters (include/emi355x.h, emi_set_model_params_batch): table [B][nparams], row b the parameter
        set of instance b; None removes the table and the shared set of set_model / set_model_source is in force again."""
        if table is None:
            self._ck(self.lib.emi_set_model_params_batch(self.ctx, None, 0, 0), "emi_set_model_params_batch")
        else:
            t = np.ascontiguousarray(table, dtype=np.float64)
            assert t.ndim == 2, "parameter table: [B][nparams]"
            self._ck(self.lib.emi_set_model_params_batch(self.ctx, _dp(t) if t.size else None, t.shape[0], t.shape[1]),
                     "emi_set_model_params_batch")
        self._changed()

    def get_model_params(self):
        """The per-instance parameter table in force, [B][nparams], or None."""
        ns, npar = C.c_int(), C.c_int()
        self._ck(self.lib.emi_get_model_params_batch(self.ctx, None, C.byref(ns), C.byref(npar)), "emi_get_model_params_batch")
        if ns.value == 0:
            return None
        t = np.empty((ns.value, npar.value), dtype=np.float64)
        self._ck(self.lib.emi_get_model_params_batch(self.ctx, _dp(t) if t.size else None, C.byref(ns), C.byref(npar)),
                 "emi_get_model_params_batch")
        return t

    def set_delays(self, x_horizon, u_horizon, dt):
        """Delayed states / controls as extra inputs of the node functions (include/emi355x.h, emi_set_delays): the model is
        written on nc + (x_horizon - 1) ns + u_horizon nc controls, evaluations keep taking U[B][nc][M]."""
        self._ck(self.lib.emi_set_delays(self.ctx, int(x_horizon), int(u_horizon), float(dt)), "emi_set_delays")
        self._changed()

    @property
    def n_delayed(self):
        if self._nd is None:
            n = C.c_int()
            self._ck(self.lib.emi_get_delays(self.ctx, None, None, C.byref(n)), "emi_get_delays")
            self._nd = n.value
        return self._nd

    def set_path(self, recs, px=0, py=1):
        recs = np.ascontiguousarray(recs, dtype=np.float64)
        if recs.ndim == 2:
            recs = recs[None]
        nsets, npth = recs.shape[0], recs.shape[1]
        self._ck(self.lib.emi_set_path(self.ctx, npth, nsets, _dp(recs) if recs.size else None, px, py), "emi_set_path")
        self._changed()

    def set_tracks(self, xc, yc):
        xc = np.ascontiguousarray(xc, dtype=np.float64)
        yc = np.ascontiguousarray(yc, dtype=np.float64)
        if xc.ndim == 2:
            xc, yc = xc[None], yc[None]
        self._ck(self.lib.emi_set_tracks(self.ctx, xc.shape[1], xc.shape[0], _dp(xc), _dp(yc)), "emi_set_tracks")
        self._changed()
        self._trk_shape = (xc.shape[0], xc.shape[1]) if xc.shape[1] else None

    def set_track_waypoints(self, t, x, y, counts=None):
        """Waypoint tables of the tracks, kept on the device across meshes: t, x, y [nsets][ntracks][ld] (2-D: one shared set),
        counts [nsets][ntracks] waypoints of each track (None: ld everywhere).  An empty table drops them (emi_set_track_waypoints)"""
        t, x, y = (np.ascontiguousarray(v, dtype=np.float64) for v in (t, x, y))
        if t.ndim == 2:
            t, x, y = t[None], x[None], y[None]
        assert t.ndim == 3 and t.shape == x.shape == y.shape
        nsets, ntracks, ld = t.shape
        cnt = None
        if counts is not None:
            cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(nsets, ntracks)
        self._ck(self.lib.emi_set_track_waypoints(self.ctx, ntracks, nsets, ld, cnt.ctypes.data_as(C.POINTER(C.c_int)) if cnt is not None else None,
                                                  _dp(t) if t.size else None, _dp(x) if x.size else None, _dp(y) if y.size else None),
                 "emi_set_track_waypoints")
        self._wp_shape = (nsets, ntracks) if ntracks else None

    def tracks_from_waypoints(self, set_map=None):
        """The centres of the tracks on the present mesh from the waypoint tables, on the device (asynchronous): result set i from
        waypoint set set_map[i] (int32 device tensor; None: every set in order) (emi_tracks_from_waypoints_dev)"""
        if set_map is not None:
            assert set_map.dtype == torch.int32 and set_map.is_contiguous()
        n = 0 if set_map is None else set_map.numel()
        self._ck(self.lib.emi_tracks_from_waypoints_dev(self.ctx, int(n), self._ipm_addr(set_map)), "emi_tracks_from_waypoints_dev")
        self._changed()
        self._trk_shape = (n or self._wp_shape[0], self._wp_shape[1])

    def get_tracks(self):
        """(xc, yc) [sets][ntracks][M]: the centres the context holds (synchronises; emi_get_tracks); EmiError where it holds none"""
        sets, ntracks = self._trk_shape or (0, 0)
        M = self.layout.M
        xc, yc = np.empty((sets, ntracks, max(M, 1))), np.empty((sets, ntracks, max(M, 1)))
        if xc.size == 0:        # nothing to come: the call says why
            xc, yc = np.empty(1), np.empty(1)
        self._ck(self.lib.emi_get_tracks(self.ctx, _dp(xc), _dp(yc)), "emi_get_tracks")
        return xc, yc

    def use_stream(self, stream_ptr):
        self._ck(self.lib.emi_set_stream(self.ctx, C.c_void_p(stream_ptr)), "emi_set_stream")

    @property
    def layout(self):
        if self._lay is None:
            lay = L.Layout()
            self._ck(self.lib.emi_get_layout(self.ctx, C.byref(lay)), "emi_get_layout")
            self._lay = lay
        return self._lay

    def jac_structure(self):
        lay = self.layout
        n = lay.nvals * lay.M
        rows, cols = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        self._ck(self.lib.emi_jac_structure(self.ctx, rows.ctypes.data_as(ip), cols.ctypes.data_as(ip)), "emi_jac_structure")
        return rows, cols

    # ---- device-resident evaluation -----------------------------------------
    def alloc_outputs(self):
        lay = self.layout
        kw = dict(dtype=self.dtype, device=self.device)
        res = torch.empty((lay.B, lay.nres, lay.M), **kw)
        vals = torch.empty((lay.B, lay.nvals, lay.M), **kw)
        cost = torch.empty((lay.B,), **kw)
        return res, vals, cost

    def eval_dev(self, X, U, RES, VALS, COST, flags=L.EVAL_ALL):
        """X,U,RES,VALS,COST: contiguous torch tensors on this evaluator's device.

        A Jacobian pass into the very VALS tensor of this evaluator's previous one, untouched by torch in between, adds
        EVAL_KEEP_INVARIANT by itself: the rows that depend on the mesh and the model alone are not stored again (the library
        checks for its part that mesh, model, batch and tables are still the same).  Code that writes into VALS past torch (a raw
        pointer, another library) must overwrite it through torch once -- VALS.add_(0) will do -- or the rows it destroyed stay destroyed."""
        lay = self.layout
        for t, shape in ((X, (lay.B, lay.ns, lay.M)), (U, (lay.B, lay.nc - self.n_delayed, lay.M)),
                         (RES, (lay.B, lay.nres, lay.M)), (VALS, (lay.B, lay.nvals, lay.M)), (COST, (lay.B,))):
            if t is None:
                continue
            if tuple(t.shape) != shape or t.dtype != self.dtype or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"tensor {tuple(t.shape)} {t.dtype} {t.device} does not match layout {shape} {self.dtype}")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        jac = VALS is not None and (flags & L.EVAL_NODES) and not (flags & L.EVAL_NOJAC)
        if jac and VALS is self._kept and VALS._version == self._kept_version:
            flags |= L.EVAL_KEEP_INVARIANT
        self._ck(self.lib.emi_eval_dev(self.ctx, ptr(X), ptr(U), ptr(RES), ptr(VALS), ptr(COST), flags), "emi_eval_dev")
        if jac:
            self._kept, self._kept_version = VALS, VALS._version

    def hess_dev(self, X, U, lamF, lamC, sigma, H):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self.lib.emi_hess_dev(self.ctx, ptr(X), ptr(U), ptr(lamF), ptr(lamC), float(sigma), ptr(H)), "emi_hess_dev")

    def synchronize(self):
        self._ck(self.lib.emi_synchronize(self.ctx), "emi_synchronize")

    # ---- host-buffer evaluation (numpy in / numpy out) ------------------------
    def eval_host(self, X, U, flags=L.EVAL_ALL, res_in=None):
        lay = self.layout
        X = np.ascontiguousarray(X, dtype=np.float64)
        U = np.ascontiguousarray(U, dtype=np.float64)
        assert X.shape == (lay.B, lay.ns, lay.M) and U.shape == (lay.B, lay.nc - self.n_delayed, lay.M)
        RES = np.zeros((lay.B, lay.nres, lay.M)) if res_in is None else np.ascontiguousarray(res_in, dtype=np.float64).copy()
        VALS = np.zeros((lay.B, lay.nvals, lay.M))
        COST = np.zeros(lay.B)
        self._ck(self.lib.emi_eval_host(self.ctx, _dp(X), _dp(U), _dp(RES), _dp(VALS), _dp(COST), flags), "emi_eval_host")
        return RES, VALS, COST

    def hess_host(self, X, U, lamF, lamC, sigma=1.0):
        lay = self.layout
        X, U, lamF = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, U, lamF))
        lamC = np.ascontiguousarray(lamC if lamC is not None else np.zeros((lay.B, 0, lay.M)), dtype=np.float64)
        H = np.zeros((lay.B, lay.nhess, lay.M))
        self._ck(self.lib.emi_hess_host(self.ctx, _dp(X), _dp(U), _dp(lamF), _dp(lamC) if lamC.size else None,
                                         float(sigma), _dp(H)), "emi_hess_host")
        return H

    # ---- adjoint pass: Lagrangian gradient and KKT certificate ------------------
    CERT_FIELDS = ("stat", "comp", "defect", "viol", "gmax", "lmax")

    def lagr_grad_dev(self, VALS, lamF, lamC, sigma, G):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self.lib.emi_lagr_grad_dev(self.ctx, ptr(VALS), ptr(lamF), ptr(lamC), float(sigma), ptr(G)), "emi_lagr_grad_dev")

    def lagr_grad_host(self, VALS, lamF, lamC, sigma=1.0):
        lay = self.layout
        VALS, lamF = (np.ascontiguousarray(a, dtype=np.float64) for a in (VALS, lamF))
        lamC = np.ascontiguousarray(lamC if lamC is not None else np.zeros((lay.B, 0, lay.M)), dtype=np.float64)
        assert VALS.shape == (lay.B, lay.nvals, lay.M) and lamF.shape == (lay.B, lay.ns, lay.M) and lamC.shape == (lay.B, lay.np, lay.M)
        G = np.zeros((lay.B, lay.ns + lay.nc, lay.M))
        self._ck(self.lib.emi_lagr_grad_host(self.ctx, _dp(VALS), _dp(lamF), _dp(lamC) if lamC.size else None, float(sigma), _dp(G)),
                 "emi_lagr_grad_host")
        return G

    def kkt_certificate_dev(self, X, U, RES, VALS, lamF, lamC, sigma, zl, zu, cl, cu, cert, G=None):
        """Device tensors, except cl / cu (host arrays [np]); zl / zu: [nsets][ns+nc][M], nsets 1 or B; cert: [B][6]."""
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        cl, cu = (np.ascontiguousarray(a, dtype=np.float64) for a in (cl, cu))
        self._ck(self.lib.emi_kkt_certificate_dev(self.ctx, ptr(X), ptr(U), ptr(RES), ptr(VALS), ptr(lamF), ptr(lamC), float(sigma),
                                                  ptr(zl), ptr(zu), int(zl.shape[0]), _dp(cl) if cl.size else None,
                                                  _dp(cu) if cu.size else None, ptr(cert), ptr(G)), "emi_kkt_certificate_dev")

    def kkt_certificate_host(self, X, U, lamF, lamC, zl, zu, cl=(), cu=(), sigma=1.0):
        """Evaluates at (X, U) and certifies; returns (cert [B][6], G [B][ns+nc][M])."""
        lay = self.layout
        X, U, lamF, zl, zu, cl, cu = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, U, lamF, zl, zu, cl, cu))
        lamC = np.ascontiguousarray(lamC if lamC is not None else np.zeros((lay.B, 0, lay.M)), dtype=np.float64)
        nv = lay.ns + lay.nc
        if zl.ndim == 2:
            zl, zu = zl[None], zu[None]
        assert zl.shape == zu.shape and zl.shape[1:] == (nv, lay.M) and cl.shape == cu.shape == (lay.np,)
        cert, G = np.zeros((lay.B, 6)), np.zeros((lay.B, nv, lay.M))
        self._ck(self.lib.emi_kkt_certificate_host(self.ctx, _dp(X), _dp(U), _dp(lamF), _dp(lamC) if lamC.size else None, float(sigma),
                                                   _dp(zl), _dp(zu), zl.shape[0], _dp(cl) if cl.size else None,
                                                   _dp(cu) if cu.size else None, _dp(cert), _dp(G)), "emi_kkt_certificate_host")
        return cert, G

    # ... for the trajectory of a context with delays: G on the ns + ncf free variables, Gdel the adjoints of the delayed values
    def lagr_grad_total_dev(self, VALS, lamF, lamC, sigma, G, Gdel=None):
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self.lib.emi_lagr_grad_total_dev(self.ctx, ptr(VALS), ptr(lamF), ptr(lamC), float(sigma), ptr(G), ptr(Gdel)),
                 "emi_lagr_grad_total_dev")

    def lagr_grad_total_host(self, VALS, lamF, lamC, sigma=1.0):
        """Returns (G [B][ns+ncf][M], Gdel [B][n_delayed][M])."""
        lay = self.layout
        VALS, lamF = (np.ascontiguousarray(a, dtype=np.float64) for a in (VALS, lamF))
        lamC = np.ascontiguousarray(lamC if lamC is not None else np.zeros((lay.B, 0, lay.M)), dtype=np.float64)
        assert VALS.shape == (lay.B, lay.nvals, lay.M) and lamF.shape == (lay.B, lay.ns, lay.M) and lamC.shape == (lay.B, lay.np, lay.M)
        nd = self.n_delayed
        G, Gdel = np.zeros((lay.B, lay.ns + lay.nc - nd, lay.M)), np.zeros((lay.B, nd, lay.M))
        self._ck(self.lib.emi_lagr_grad_total_host(self.ctx, _dp(VALS), _dp(lamF), _dp(lamC) if lamC.size else None, float(sigma), _dp(G),
                                                   _dp(Gdel) if nd else None), "emi_lagr_grad_total_host")
        return G, Gdel

    def kkt_certificate_total_dev(self, X, U, RES, VALS, lamF, lamC, sigma, zl, zu, cl, cu, cert, G=None, Gdel=None):
        """As kkt_certificate_dev with U, zl, zu, G on the free variables ([.][ns+ncf][M]); Gdel: [B][n_delayed][M] or None."""
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        cl, cu = (np.ascontiguousarray(a, dtype=np.float64) for a in (cl, cu))
        self._ck(self.lib.emi_kkt_certificate_total_dev(self.ctx, ptr(X), ptr(U), ptr(RES), ptr(VALS), ptr(lamF), ptr(lamC), float(sigma),
                                                        ptr(zl), ptr(zu), int(zl.shape[0]), _dp(cl) if cl.size else None,
                                                        _dp(cu) if cu.size else None, ptr(cert), ptr(G), ptr(Gdel)),
                 "emi_kkt_certificate_total_dev")

    def kkt_certificate_total_host(self, X, U, lamF, lamC, zl, zu, cl=(), cu=(), sigma=1.0):
        """Evaluates at (X, U) (the delayed values formed on the device) and certifies; returns (cert [B][6], G [B][ns+ncf][M],
        Gdel [B][n_delayed][M])."""
        lay = self.layout
        X, U, lamF, zl, zu, cl, cu = (np.ascontiguousarray(a, dtype=np.float64) for a in (X, U, lamF, zl, zu, cl, cu))
        lamC = np.ascontiguousarray(lamC if lamC is not None else np.zeros((lay.B, 0, lay.M)), dtype=np.float64)
        nd = self.n_delayed
        nf = lay.ns + lay.nc - nd
        if zl.ndim == 2:
            zl, zu = zl[None], zu[None]
        assert X.shape == (lay.B, lay.ns, lay.M) and U.shape == (lay.B, nf - lay.ns, lay.M)
        assert zl.shape == zu.shape and zl.shape[1:] == (nf, lay.M) and cl.shape == cu.shape == (lay.np,)
        cert, G, Gdel = np.zeros((lay.B, 6)), np.zeros((lay.B, nf, lay.M)), np.zeros((lay.B, nd, lay.M))
        self._ck(self.lib.emi_kkt_certificate_total_host(self.ctx, _dp(X), _dp(U), _dp(lamF), _dp(lamC) if lamC.size else None,
                                                         float(sigma), _dp(zl), _dp(zu), zl.shape[0], _dp(cl) if cl.size else None,
                                                         _dp(cu) if cu.size else None, _dp(cert), _dp(G), _dp(Gdel) if nd else None),
                 "emi_kkt_certificate_total_host")
        return cert, G, Gdel

    # ---- Newton step (KKT solve) on the device ----------------------------------
    def kkt_factor(self, Qblk, Jblk, fixed, dc=0.0):
        """Assemble and LU-factorise the KKT matrix of one instance; returns rocSOLVER's info (0 = ok)."""
        lay = self.layout
        nv = lay.ns + lay.nc
        Qblk = np.ascontiguousarray(Qblk, dtype=np.float64)
        Jblk = np.ascontiguousarray(Jblk, dtype=np.float64)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        assert Qblk.shape == (lay.nhess, lay.M) and Jblk.shape == (lay.ns * nv, lay.M) and fixed.shape == (nv * lay.M,)
        info = C.c_int(-1)
        self._ck(self.lib.emi_kkt_factor(self.ctx, _dp(Qblk), _dp(Jblk), fixed.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                         float(dc), C.byref(info)), "emi_kkt_factor")
        return info.value

    def kkt_factor_dev(self, Qblk, Jblk, fixed, dc=0.0):
        """kkt_factor on device tensors (Qblk [nhess][M] and Jblk [>= ns*nv][M] float64, fixed [nv*M] uint8); returns info."""
        info = C.c_int(-1)
        self._ck(self.lib.emi_kkt_factor_dev(self.ctx, C.c_void_p(Qblk.data_ptr()), C.c_void_p(Jblk.data_ptr()),
                                             C.c_void_p(fixed.data_ptr()), float(dc), C.byref(info)), "emi_kkt_factor_dev")
        return info.value

    # ---- node blocks of the Newton step: assembly, Cholesky screen, eigen-fix (emi_kkt_blocks_*) ------------------------
    def kkt_blocks_rows(self, rows):
        """rows: per path row a list of (variable, VALS entry) pairs"""
        ptr, var, ent = [0], [], []
        for r in rows:
            var += [int(v) for v, _ in r]
            ent += [int(e) for _, e in r]
            ptr.append(len(var))
        ia = lambda a: (C.c_int * max(len(a), 1))(*a)
        self._ck(self.lib.emi_kkt_blocks_rows(self.ctx, len(rows), ia(ptr), ia(var), ia(ent)), "emi_kkt_blocks_rows")

    def kkt_blocks_dev(self, H, VALS, Sigma, SigT, fixed, dw_shift, Q, max_mods, count, node, delta, vec, worst, Qexact=None):
        """Device tensors in the layouts of include/emi355x.h (SigT, Qexact, and with max_mods 0 node / delta / vec may be None);
        asynchronous on the context's stream."""
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self.lib.emi_kkt_blocks_dev(self.ctx, ptr(H), ptr(VALS), ptr(Sigma), ptr(SigT), ptr(fixed), float(dw_shift), ptr(Qexact),
                                             ptr(Q), int(max_mods), ptr(count), ptr(node), ptr(delta), ptr(vec), ptr(worst)),
                 "emi_kkt_blocks_dev")

    def kkt_blocks_host(self, H, VALS, Sigma, SigT, fixed, dw_shift=0.0, max_mods=None):
        """numpy in / numpy out: dict Qexact, Q [B][nhess][M], count [B], node [B][max_mods], delta, vec [B][max_mods][nv], worst [B]
        (max_mods defaults to nv * M: every pair fits; entries beyond count keep -1 / nan)."""
        lay = self.layout
        nv = lay.ns + lay.nc
        mm = nv * lay.M if max_mods is None else int(max_mods)
        H, VALS, Sigma = (np.ascontiguousarray(a, dtype=np.float64) for a in (H, VALS, Sigma))
        SigT = np.ascontiguousarray(SigT if SigT is not None else np.zeros((lay.B, 0, lay.M)), dtype=np.float64)
        fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        assert H.shape == (lay.B, lay.nhess, lay.M) and VALS.shape == (lay.B, lay.nvals, lay.M) and Sigma.shape == (lay.B, nv, lay.M)
        assert SigT.shape == (lay.B, lay.np, lay.M) and fixed.shape == (lay.B, nv, lay.M)
        out = dict(Qexact=np.zeros_like(H), Q=np.zeros_like(H), count=np.zeros(lay.B, dtype=np.int32),
                   node=np.full((lay.B, mm), -1, dtype=np.int32), delta=np.full((lay.B, mm), np.nan),
                   vec=np.full((lay.B, mm, nv), np.nan), worst=np.zeros(lay.B))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._ck(self.lib.emi_kkt_blocks_host(self.ctx, _dp(H), _dp(VALS), _dp(Sigma), _dp(SigT) if SigT.size else None,
                                              fixed.ctypes.data_as(C.POINTER(C.c_ubyte)), float(dw_shift), _dp(out["Qexact"]), _dp(out["Q"]),
                                              mm, ip(out["count"]), ip(out["node"]) if mm else None, _dp(out["delta"]) if mm else None,
                                              _dp(out["vec"]) if mm else None, _dp(out["worst"])), "emi_kkt_blocks_host")
        return out

    def kkt_lowrank(self, node, vec, delta):
        """K = K~ - sum delta_c u_c u_c^T; returns True iff K has the inertia of K~ (solves are then with K)."""
        node = np.ascontiguousarray(node, dtype=np.int32)
        vec = np.ascontiguousarray(vec, dtype=np.float64)
        delta = np.ascontiguousarray(delta, dtype=np.float64)
        exact = C.c_int(0)
        r = node.size
        self._ck(self.lib.emi_kkt_lowrank(self.ctx, r, node.ctypes.data_as(C.POINTER(C.c_int)) if r else None,
                                          _dp(vec) if r else None, _dp(delta) if r else None, C.byref(exact)), "emi_kkt_lowrank")
        return bool(exact.value)

    def kkt_solve(self, rhs):
        """rhs: [N] or [nrhs][N]; returns the solution(s) in the same shape."""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64).copy()
        nrhs = 1 if rhs.ndim == 1 else rhs.shape[0]
        self._ck(self.lib.emi_kkt_solve(self.ctx, _dp(rhs), nrhs), "emi_kkt_solve")
        return rhs

    def kkt_solve_dev(self, rhs):
        """kkt_solve on a device tensor ([N] or [nrhs][N] float64), in place; asynchronous on the context's stream."""
        nrhs = 1 if rhs.dim() == 1 else rhs.shape[0]
        self._ck(self.lib.emi_kkt_solve_dev(self.ctx, C.c_void_p(rhs.data_ptr()), nrhs), "emi_kkt_solve_dev")

    # ---- the Newton steps of the whole batch, device tensors in and out (emi_kkt_*_shard_dev) -----------------------------
    # Tensors in the layouts of include/emi355x.h; mask: None (every instance) or B flags; the per-instance scalars come back as
    # numpy arrays of length B (entries of masked instances are -1 / nan: the library does not write them).
    def _shard_mask(self, mask):
        if mask is None:
            return None, None
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.shape == (self.layout.B,)
        return m, m.ctypes.data_as(C.POINTER(C.c_ubyte))

    def kkt_factor_shard_dev(self, Q, VALS, fixed, dc, mask=None):
        """Factorise the Newton systems of the batch (Q [B][nhess][M], VALS [B][nvals][M] float64, fixed [B][nv][M] uint8, dc a
        scalar or B values); returns info [B]: 0 factorised, > 0 singular."""
        B = self.layout.B
        dc = np.ascontiguousarray(np.broadcast_to(np.asarray(dc, dtype=np.float64), (B,)))
        info = np.full(B, -1, dtype=np.int32)
        m, mp = self._shard_mask(mask)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self.lib.emi_kkt_factor_shard_dev(self.ctx, ptr(Q), ptr(VALS), ptr(fixed), _dp(dc), mp,
                                                   info.ctypes.data_as(C.POINTER(C.c_int))), "emi_kkt_factor_shard_dev")
        return info

    def kkt_lowrank_shard_dev(self, max_mods, count=None, node=None, delta=None, vec=None, mask=None):
        """Inertia verdict and Woodbury set-up per instance from the lists of kkt_blocks_dev (device tensors); max_mods 0 clears.
        Returns exact [B] (1: solves of that instance answer for the unmodified matrix)."""
        exact = np.full(self.layout.B, -1, dtype=np.int32)
        m, mp = self._shard_mask(mask)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self._ck(self.lib.emi_kkt_lowrank_shard_dev(self.ctx, int(max_mods), ptr(count), ptr(node), ptr(delta), ptr(vec), mp,
                                                    exact.ctypes.data_as(C.POINTER(C.c_int))), "emi_kkt_lowrank_shard_dev")
        return exact

    def kkt_solve_shard_dev(self, rhs, mask=None):
        """rhs [B][2 ns + nc][M] float64 device tensor, solved in place; asynchronous on the context's stream."""
        m, mp = self._shard_mask(mask)
        self._ck(self.lib.emi_kkt_solve_shard_dev(self.ctx, C.c_void_p(rhs.data_ptr()) if rhs is not None else None, mp),
                 "emi_kkt_solve_shard_dev")

    def kkt_solve_refined_shard_dev(self, rhs, dc_nominal, max_steps=10, mask=None):
        """The solve with its iterative refinement on the device, in place on rhs; returns dict rel, nsolve, reverted, status [B]."""
        B = self.layout.B
        dcn = np.ascontiguousarray(np.broadcast_to(np.asarray(dc_nominal, dtype=np.float64), (B,)))
        out = dict(rel=np.full(B, np.nan), nsolve=np.full(B, -1, dtype=np.int32), reverted=np.full(B, -1, dtype=np.int32),
                   status=np.full(B, -1, dtype=np.int32))
        m, mp = self._shard_mask(mask)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        self._ck(self.lib.emi_kkt_solve_refined_shard_dev(self.ctx, C.c_void_p(rhs.data_ptr()) if rhs is not None else None, mp, _dp(dcn),
                                                          int(max_steps), _dp(out["rel"]), ip(out["nsolve"]), ip(out["reverted"]),
                                                          ip(out["status"])), "emi_kkt_solve_refined_shard_dev")
        return out

    # ---- the array arithmetic of an interior-point iteration, batched (emi_ipm_*) ----------------------------------------
    # Argument groups are dicts keyed as the structs of include/emi355x.h (X U S E1 E2 | LamF Y ZL ZU VL VU W1 W2 | DZLam DS DY DE1
    # DE2 DZL DZU DVL DVU DW1 DW2 | Sigma SigT SigS RhatS Rt); bounds: dict zl, zu ([nsets][nv][M]) and cl, cu, cscale (host, [np];
    # cscale optional).  dev=True: torch tensors on this device, asynchronous; dev=False: contiguous float64 numpy arrays (uint8
    # for the mask), read and written in place, synchronised on return.  A missing key or None is a NULL pointer.
    @staticmethod
    def _ipm_addr(a):
        if a is None:
            return None
        return C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else C.c_void_p(a.ctypes.data)

    def _ipm_group(self, cls, d, keep):
        if d is None:
            return None
        g = cls()
        for f in cls.FIELDS:
            a = d.get(f)
            if a is not None and not isinstance(a, torch.Tensor):
                assert a.dtype == np.float64 and a.flags.c_contiguous, f
            setattr(g, f, self._ipm_addr(a))
        keep.append(g)
        return C.byref(g)

    def _ipm_bounds(self, bd, keep):
        if bd is None:
            return None
        g = L.IpmBounds()
        g.zl, g.zu, g.nsets = self._ipm_addr(bd.get("zl")), self._ipm_addr(bd.get("zu")), int(bd["zl"].shape[0]) if bd.get("zl") is not None else 0
        for f in ("cl", "cu", "cscale"):
            a = bd.get(f)
            if a is not None and len(a):
                a = np.ascontiguousarray(a, dtype=np.float64)
                keep.append(a)
                setattr(g, f, _dp(a))
        keep.append(g)
        return C.byref(g)

    def _ipm_call(self, name, dev, build):
        keep = []
        fn = getattr(self.lib, f"emi_ipm_{name}_{'dev' if dev else 'host'}")
        self._ck(fn(self.ctx, *build(keep)), fn.__name__)

    def ipm_reduce(self, point, duals, RES, VALS, G, bounds, par, elim, rhs, DefRes=None, RowRes=None, dev=True):
        A, pt, du, el = self._ipm_addr, L.IpmPoint, L.IpmDuals, L.IpmElim
        self._ipm_call("reduce", dev, lambda k: (self._ipm_group(pt, point, k), self._ipm_group(du, duals, k), A(RES), A(VALS), A(G),
                                                 self._ipm_bounds(bounds, k), A(par), A(DefRes), A(RowRes), self._ipm_group(el, elim, k), A(rhs)))

    def ipm_expand(self, point, duals, VALS, bounds, par, elim, step, scal, rs=None, dev=True):
        A = self._ipm_addr
        self._ipm_call("expand", dev, lambda k: (self._ipm_group(L.IpmPoint, point, k), self._ipm_group(L.IpmDuals, duals, k), A(VALS),
                                                 self._ipm_bounds(bounds, k), A(par), self._ipm_group(L.IpmElim, elim, k), A(rs),
                                                 self._ipm_group(L.IpmStep, step, k), A(scal)))

    def ipm_trial(self, point, step, alpha, trial, dev=True):
        self._ipm_call("trial", dev, lambda k: (self._ipm_group(L.IpmPoint, point, k), self._ipm_group(L.IpmStep, step, k), self._ipm_addr(alpha),
                                                self._ipm_group(L.IpmPoint, trial, k)))

    def ipm_merit(self, point, RES, COST, bounds, par, out, rs=None, reset=False, dev=True):
        A = self._ipm_addr
        self._ipm_call("merit", dev, lambda k: (self._ipm_group(L.IpmPoint, point, k), A(RES), A(COST), self._ipm_bounds(bounds, k), A(par), A(rs),
                                                int(bool(reset)), A(out)))

    def ipm_accept(self, point, trial, duals, step, bounds, par, a_pr, a_du, mask=None, dev=True):
        A = self._ipm_addr
        self._ipm_call("accept", dev, lambda k: (self._ipm_group(L.IpmPoint, point, k), self._ipm_group(L.IpmPoint, trial, k),
                                                 self._ipm_group(L.IpmDuals, duals, k), self._ipm_group(L.IpmStep, step, k),
                                                 self._ipm_bounds(bounds, k), A(par), A(a_pr), A(a_du), A(mask)))

    def ipm_error(self, point, duals, RES, G, bounds, par, out, dev=True):
        A = self._ipm_addr
        self._ipm_call("error", dev, lambda k: (self._ipm_group(L.IpmPoint, point, k), self._ipm_group(L.IpmDuals, duals, k), A(RES), A(G),
                                                self._ipm_bounds(bounds, k), A(par), A(out)))

    def ipm_error_parts(self, point, duals, RES, G, bounds, par, out, dev=True):
        """out [B][8] = {ed, sd, ep, sc, pmin, pmax, emax, ymax}: the components of ipm_error's KKT error (any barrier parameter)"""
        A = self._ipm_addr
        self._ipm_call("error_parts", dev, lambda k: (self._ipm_group(L.IpmPoint, point, k), self._ipm_group(L.IpmDuals, duals, k), A(RES), A(G),
                                                      self._ipm_bounds(bounds, k), A(par), A(out)))

    def ipm_keep(self, point, duals, kept_point, kept_duals, mask=None, restore=False, dev=True):
        """the iterate (X U S E1 E2 | LamF Y ZL ZU VL VU W1 W2) of the instances of mask ([B] uint8, None: all) copied live -> kept, or
        kept -> live with restore; an instance the mask leaves out keeps every bit (include/emi355x.h: emi_ipm_keep_dev)"""
        self._ipm_call("keep", dev, lambda k: (self._ipm_group(L.IpmPoint, point, k), self._ipm_group(L.IpmDuals, duals, k),
                                               self._ipm_group(L.IpmPoint, kept_point, k), self._ipm_group(L.IpmDuals, kept_duals, k),
                                               self._ipm_addr(mask), int(bool(restore))))

    def ipm_start(self, phase, point, duals, bounds, RES=None, par=None, fixed=None, mask=None, bound_push=1e-2, bound_frac=1e-2):
        """solve_nlp's start() on device tensors: phase 0 interior push of X, U and the fixed bytes; 1 slacks, elastics and multipliers
        from the first evaluation; 2 the reset of W1, W2 (include/emi355x.h: emi_ipm_start_dev)"""
        keep = []
        A = self._ipm_addr
        self._ck(self.lib.emi_ipm_start_dev(self.ctx, int(phase), self._ipm_group(L.IpmPoint, point, keep), self._ipm_group(L.IpmDuals, duals, keep),
                                            A(RES), self._ipm_bounds(bounds, keep), A(par), float(bound_push), float(bound_frac), A(fixed), A(mask)),
                 "emi_ipm_start_dev")

    # ---- lock-step interior-point solve of the whole batch on this mesh (emi_ipm_solve_shard_*) ---------------------------------
    def ipm_solve_shard(self, X, U, bounds, options=None, dev=True):
        """X [B][ns][M], U [B][nc][M]: the starts on entry, the final iterates on return (in place); bounds as for the ipm_* calls;
        options: dict of emi_ipm_options_t fields (missing ones take solve_nlp's defaults).  dev=True: torch tensors on this device,
        dev=False: contiguous float64 numpy arrays.  Returns (LamF [B][ns][M], LamC [B][np][M], results): the multipliers in the
        kind of array given, and one dict per instance with the fields of emi_ipm_result_t."""
        lay = self.layout
        opt = L.IpmOptions()
        for k, v in (options or {}).items():
            setattr(opt, k, v)
        if dev:
            kw = dict(dtype=torch.float64, device=X.device)
            LamF, LamC = torch.zeros((lay.B, lay.ns, lay.M), **kw), torch.zeros((lay.B, lay.np, lay.M), **kw)
        else:
            assert all(a.dtype == np.float64 and a.flags.c_contiguous for a in (X, U))
            LamF, LamC = np.zeros((lay.B, lay.ns, lay.M)), np.zeros((lay.B, lay.np, lay.M))
        res = (L.IpmResult * lay.B)()
        keep = []
        A = self._ipm_addr
        fn = self.lib.emi_ipm_solve_shard_dev if dev else self.lib.emi_ipm_solve_shard_host
        self._ck(fn(self.ctx, A(X), A(U), self._ipm_bounds(bounds, keep), C.byref(opt), A(LamF), A(LamC) if lay.np else None, res), fn.__name__)
        return LamF, LamC, [{n: getattr(r, n) for n, _ in L.IpmResult._fields_} for r in res]

    # ---- the mesh ladder over the lock-step solve (emi_prolong_*, emi_repair_guess_dev, emi_ipm_solve_ladder_*) -----------------
    @staticmethod
    def prolong_matrix(Mc, Mf, coarse=None, fine=None):
        """P [Mf][Mc]: the Lagrange basis of the coarse LGL nodes at the fine ones (host, emi_prolong_matrix); coarse / fine: (tau, w,
        ..) of other node sets than lgl(Mc) / lgl(Mf)"""
        lib = L.load()
        tc, wc = (np.ascontiguousarray(a, dtype=np.float64) for a in (coarse if coarse is not None else lgl(Mc))[:2])
        tf_ = np.ascontiguousarray((fine if fine is not None else lgl(Mf))[0], dtype=np.float64)
        P = np.empty((Mf, Mc))
        L.check(lib.emi_prolong_matrix(int(Mc), _dp(tc), _dp(wc), int(Mf), _dp(tf_), _dp(P)), what="emi_prolong_matrix")
        return P

    def prolong(self, PT, Vc, Vf=None):
        """Vf [.., Mf] = Vc [.., Mc] P^T on the device from PT [Mc][Mf] = P transposed (torch tensors, float64); asynchronous"""
        Mc, Mf = PT.shape
        assert Vc.shape[-1] == Mc and PT.is_contiguous() and Vc.is_contiguous()
        R = Vc.numel() // Mc
        if Vf is None:
            Vf = torch.empty(tuple(Vc.shape[:-1]) + (Mf,), dtype=torch.float64, device=Vc.device)
        assert Vf.is_contiguous() and Vf.numel() == R * Mf
        self._ck(self.lib.emi_prolong_dev(self.ctx, int(Mc), int(Mf), C.c_void_p(PT.data_ptr()), C.c_void_p(Vc.data_ptr()), int(R),
                                          C.c_void_p(Vf.data_ptr())), "emi_prolong_dev")
        return Vf

    def repair_guess(self, X):
        """interior nodes of X [B][ns][M] (device tensor, in place) inside a keep-out of the record table moved out of it; asynchronous"""
        self._ck(self.lib.emi_repair_guess_dev(self.ctx, C.c_void_p(X.data_ptr()) if X is not None else None), "emi_repair_guess_dev")

    def start_guess(self, kind, xa, xb, box=None, bend=0.0, clearance=0.01, grid=0, repair=0, X=None, dev=True):
        """The starts of the whole batch on the present mesh (emi_start_guess_*): kind START_LINE / START_BEND / START_PLANNED; xa, xb
        [nsets][ns] (1-D: one shared set) the states at t0 and tf, box [nsets][4] {xl, xu, yl, yu} of the position states or None.
        Returns (X [B][ns][M], level [B] int32): torch tensors on this device (asynchronous; X may be given), or numpy arrays
        with dev=False."""
        lay = self.layout
        xa, xb = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1, lay.ns) for a in (xa, xb))
        assert xa.shape == xb.shape
        st = L.Start(kind=int(kind), nsets=xa.shape[0], xa=_dp(xa), xb=_dp(xb), bend=float(bend), clearance=float(clearance), grid=int(grid),
                     repair=int(bool(repair)))
        if box is not None:
            box = np.ascontiguousarray(box, dtype=np.float64).reshape(-1, 4)
            assert box.shape[0] == xa.shape[0]
            st.box = _dp(box)
        if dev:
            if X is None:
                X = torch.empty((lay.B, lay.ns, lay.M), dtype=torch.float64, device=self.device)
            assert X.dtype == torch.float64 and X.is_contiguous() and tuple(X.shape) == (lay.B, lay.ns, lay.M)
            level = torch.empty((lay.B,), dtype=torch.int32, device=self.device)
            fn = self.lib.emi_start_guess_dev
        else:
            X, level = np.empty((lay.B, lay.ns, lay.M)), np.empty(lay.B, dtype=np.int32)
            fn = self.lib.emi_start_guess_host
        self._ck(fn(self.ctx, C.byref(st), self._ipm_addr(X), self._ipm_addr(level)), fn.__name__)
        return X, level

    def _ipm_rungs(self, rungs, keep):
        """the emi_ipm_rung_t array of a list of dict M, bounds, recs, options, repair (ipm_solve_ladder); keep: what must outlive the call"""
        arr = (L.IpmRung * max(1, len(rungs)))()
        for g, r in zip(arr, rungs):
            g.M = int(r["M"])
            bd = r["bounds"]
            g.bd.zl, g.bd.zu, g.bd.nsets = self._ipm_addr(bd.get("zl")), self._ipm_addr(bd.get("zu")), int(bd["zl"].shape[0])
            for f in ("cl", "cu", "cscale"):
                a = bd.get(f)
                if a is not None and len(a):
                    a = np.ascontiguousarray(a, dtype=np.float64)
                    keep.append(a)
                    setattr(g.bd, f, _dp(a))
            if r.get("recs") is not None:
                a = np.ascontiguousarray(r["recs"], dtype=np.float64)
                keep.append(a)
                g.recs = _dp(a)
            for k, v in (r.get("options") or {}).items():
                setattr(g.opt, k, v)
            g.repair = int(bool(r.get("repair")))
        return arr

    def ipm_solve_ladder(self, rungs, t0, tf, X0, U0, dev=True):
        """rungs: list of dict M, bounds (as for the ipm_* calls, at this M), and optionally recs (record table of emi_set_path's
        shape), options (dict of emi_ipm_options_t fields), repair.  X0 [B][ns][M_0], U0 [B][nc][M_0] are read only.  dev=True: torch
        tensors on this device; dev=False: contiguous float64 numpy arrays.  Returns (X, U, LamF, LamC, results[rung][b]) on the last
        rung's mesh, which is the context's mesh afterwards."""
        lay = self.layout
        B, ns, nc, npth, Ml = lay.B, lay.ns, lay.nc, lay.np, int(rungs[-1]["M"]) if rungs else 0
        keep = []
        arr = self._ipm_rungs(rungs, keep)
        if dev:
            kw = dict(dtype=torch.float64, device=X0.device)
            new = lambda *s: torch.zeros(s, **kw)
        else:
            assert all(a.dtype == np.float64 and a.flags.c_contiguous for a in (X0, U0))
            new = lambda *s: np.zeros(s)
        X, U, LamF, LamC = new(B, ns, Ml), new(B, nc, Ml), new(B, ns, Ml), new(B, npth, Ml)
        res = (L.IpmResult * max(1, len(rungs) * B))()
        A = self._ipm_addr
        fn = self.lib.emi_ipm_solve_ladder_dev if dev else self.lib.emi_ipm_solve_ladder_host
        st = fn(self.ctx, len(rungs), arr, float(t0), float(tf), A(X0), A(U0), A(X), A(U), A(LamF), A(LamC) if npth else None, res)
        self._changed()
        self._trk_shape = self._wp_shape    # (an upper bound after an error)
        self._ck(st, fn.__name__)
        self.tau, self.w, self.D = lgl(Ml)
        self.node_t = t0 + (tf - t0) / 2.0 * (self.tau + 1.0)
        fields = [n for n, _ in L.IpmResult._fields_]
        return X, U, LamF, LamC, [[{n: getattr(res[r * B + b], n) for n in fields} for b in range(B)] for r in range(len(rungs))]

    # ---- the ladder with refinement: instances that meet the ODE tolerance leave the batch (emi_ipm_solve_refine_*) -------------
    @staticmethod
    def refine_decide(status, err, ode_tol, has_good, is_last):
        """(retires, verdict): the rule of emi_ipm_solve_refine_* for one instance after a solve (host, emi_ipm_refine_decide)"""
        v = C.c_int(-1)
        r = L.load().emi_ipm_refine_decide(int(status), float(err), float(ode_tol), int(bool(has_good)), int(bool(is_last)), C.byref(v))
        return bool(r), v.value

    def prolong_rows(self, PT, Vc, row_map=None, Vf=None):
        """Vf [R][Mf]: row r = P Vc[row_map[r]] (row_map: int32 device tensor [R], None: the identity and R = the rows of Vc);
        torch tensors, float64; asynchronous (emi_prolong_rows_dev)"""
        Mc, Mf = PT.shape
        assert Vc.shape[-1] == Mc and PT.is_contiguous() and Vc.is_contiguous()
        if row_map is not None:
            assert row_map.dtype == torch.int32 and row_map.is_contiguous()
        R = Vc.numel() // Mc if row_map is None else row_map.numel()
        if Vf is None:
            Vf = torch.empty((R, Mf), dtype=torch.float64, device=Vc.device)
        assert Vf.is_contiguous() and Vf.numel() == R * Mf
        self._ck(self.lib.emi_prolong_rows_dev(self.ctx, int(Mc), int(Mf), C.c_void_p(PT.data_ptr()), C.c_void_p(Vc.data_ptr()), int(R),
                                               self._ipm_addr(row_map), C.c_void_p(Vf.data_ptr())), "emi_prolong_rows_dev")
        return Vf

    def shard_move(self, src, dst, length, src_idx=None, dst_idx=None, n=None):
        """the instances of a list moved between up to 4 pairs of arrays: src[a] [.., rows_a, src_ld_a] -> dst[a] [.., rows_a, dst_ld_a]
        (float64 device tensors), entry i: the first `length` values of every row of instance src_idx[i] to instance dst_idx[i]
        (int32 device tensors, None: 0 .. n-1); asynchronous (emi_shard_move_dev)"""
        na = len(src)
        assert na == len(dst) and all(a.is_contiguous() and a.dtype == torch.float64 for a in list(src) + list(dst))
        for ix in (src_idx, dst_idx):
            assert ix is None or (ix.dtype == torch.int32 and ix.is_contiguous())
        if n is None:
            n = next((ix.numel() for ix in (src_idx, dst_idx) if ix is not None), src[0].shape[0] if na else 0)
        ints = lambda v: (C.c_int * max(1, na))(*v)
        ptrs = lambda ts: (C.c_void_p * max(1, na))(*[t.data_ptr() for t in ts])
        rows = [int(a.shape[-2]) for a in src]
        assert rows == [int(a.shape[-2]) for a in dst]
        self._ck(self.lib.emi_shard_move_dev(self.ctx, int(n), self._ipm_addr(src_idx), self._ipm_addr(dst_idx), na, ints(rows), ptrs(src),
                                             ints([a.shape[-1] for a in src]), ptrs(dst), ints([a.shape[-1] for a in dst]), int(length)),
                 "emi_shard_move_dev")

    def ipm_solve_refine(self, rungs, t0, tf, X0, U0, ode_tol, first_check=0, ul=None, uu=None, ldm=None, out=None, dev=True):
        """The ladder of ipm_solve_ladder with the instances retired as they meet ode_tol from rung first_check on (include/emi355x.h:
        emi_ipm_solve_refine_*).  out: (X, U, LamF, LamC) [B][rows][ldm] to write into (the columns beyond an instance's mesh keep
        their bits), None: zeros with ldm = the largest rung.  Returns (X, U, LamF, LamC, results[rung][b], err [rungs][B],
        summary[b] = dict rung, verdict, rungs_solved, err).  The context is on the last solved rung's mesh afterwards."""
        lay = self.layout
        B, ns, nc, npth = lay.B, lay.ns, lay.nc, lay.np
        keep = []
        arr = self._ipm_rungs(rungs, keep)
        ldm = int(ldm if ldm is not None else (out[0].shape[-1] if out is not None else max([int(r["M"]) for r in rungs] or [0])))
        if out is not None:
            X, U, LamF, LamC = out
        elif dev:
            kw = dict(dtype=torch.float64, device=X0.device)
            X, U, LamF, LamC = (torch.zeros((B, r, ldm), **kw) for r in (ns, nc, ns, npth))
        else:
            X, U, LamF, LamC = (np.zeros((B, r, ldm)) for r in (ns, nc, ns, npth))
        if not dev:
            assert all(a.dtype == np.float64 and a.flags.c_contiguous for a in (X0, U0, X, U, LamF, LamC))
        rf = L.IpmRefine()
        rf.ode_tol, rf.first_check = float(ode_tol), int(first_check)
        for f, a in (("ul", ul), ("uu", uu)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                keep.append(a)
                setattr(rf, f, _dp(a))
        nr = len(rungs)
        res = (L.IpmResult * max(1, nr * B))()
        err = np.full((max(1, nr), B), np.nan)
        summ = (L.IpmRefineResult * B)()
        A = self._ipm_addr
        fn = self.lib.emi_ipm_solve_refine_dev if dev else self.lib.emi_ipm_solve_refine_host
        st = fn(self.ctx, nr, arr, float(t0), float(tf), C.byref(rf), A(X0), A(U0), ldm, A(X), A(U), A(LamF), A(LamC) if npth else None, res,
                _dp(err), summ)
        self._changed()
        self._trk_shape = self._wp_shape    # (an upper bound after an error)
        self._ck(st, fn.__name__)
        Ml = self.layout.M
        self.tau, self.w, self.D = lgl(Ml)
        self.node_t = t0 + (tf - t0) / 2.0 * (self.tau + 1.0)
        fields = [n for n, _ in L.IpmResult._fields_]
        results = [[{n: getattr(res[r * B + b], n) for n in fields} for b in range(B)] for r in range(nr)]
        return X, U, LamF, LamC, results, err[:nr], [{n: getattr(q, n) for n, _ in L.IpmRefineResult._fields_} for q in summ]

    # ---- ladder restarts: the instances an attempt did not solve are solved again from the next start (emi_ipm_solve_restart_*) ---
    @staticmethod
    def restart_decide(verdict, retry_mask=0):
        """whether an instance that ended an attempt with `verdict` goes to the next attempt (host, emi_ipm_restart_decide)"""
        return bool(L.load().emi_ipm_restart_decide(int(verdict), int(retry_mask)))

    def _ipm_starts(self, starts, keep):
        """the emi_start_t array of a list of dict kind, xa, xb and optionally box, bend, clearance, grid, repair (the arguments of
        start_guess); keep: what must outlive the call"""
        ns = self.layout.ns
        arr = (L.Start * max(1, len(starts)))()
        for g, d in zip(arr, starts):
            xa, xb = (np.ascontiguousarray(d[k], dtype=np.float64).reshape(-1, ns) for k in ("xa", "xb"))
            assert xa.shape == xb.shape
            keep += [xa, xb]
            g.kind, g.nsets, g.xa, g.xb = int(d["kind"]), xa.shape[0], _dp(xa), _dp(xb)
            if d.get("box") is not None:
                box = np.ascontiguousarray(d["box"], dtype=np.float64).reshape(-1, 4)
                assert box.shape[0] == xa.shape[0]
                keep.append(box)
                g.box = _dp(box)
            g.bend, g.clearance = float(d.get("bend", 0.0)), float(d.get("clearance", 0.01))
            g.grid, g.repair = int(d.get("grid", 0)), int(bool(d.get("repair")))
        return arr

    def ipm_solve_restart(self, rungs, t0, tf, starts, U0, X0=None, ode_tol=None, first_check=0, ul=None, uu=None, patience=None,
                          retry_mask=0, flags=0, ldm=None, out=None, dev=True):
        """The rung loop of ipm_solve_refine (ode_tol None: of ipm_solve_ladder) run again from the next start on the instances an
        attempt did not solve (include/emi355x.h: emi_ipm_solve_restart_*).  Attempt 0 starts from X0 where given; the others from
        `starts`, a list of dict kind, xa, xb, box, bend, clearance, grid, repair as for start_guess.  patience: list of max_iter of
        rung 0 per attempt (0: the rung's own); flags: RESTART_DROP_FAILED.  out: (X, U, LamF, LamC) [B][rows][ldm] to write into.
        Returns (X, U, LamF, LamC, results[attempt][rung][b], err [attempts][rungs][B], summary[b] = dict attempt, attempts, level,
        rung, verdict, rungs_solved, err)."""
        lay = self.layout
        B, ns, nc, npth = lay.B, lay.ns, lay.nc, lay.np
        keep = []
        arr = self._ipm_rungs(rungs, keep)
        ldm = int(ldm if ldm is not None else (out[0].shape[-1] if out is not None else max([int(r["M"]) for r in rungs] or [0])))
        if out is not None:
            X, U, LamF, LamC = out
        elif dev:
            kw = dict(dtype=torch.float64, device=U0.device)
            X, U, LamF, LamC = (torch.zeros((B, r, ldm), **kw) for r in (ns, nc, ns, npth))
        else:
            X, U, LamF, LamC = (np.zeros((B, r, ldm)) for r in (ns, nc, ns, npth))
        if not dev:
            assert all(a is None or (a.dtype == np.float64 and a.flags.c_contiguous) for a in (X0, U0, X, U, LamF, LamC))
        rf = None
        if ode_tol is not None:
            rf = L.IpmRefine()
            rf.ode_tol, rf.first_check = float(ode_tol), int(first_check)
            for f, a in (("ul", ul), ("uu", uu)):
                if a is not None:
                    a = np.ascontiguousarray(a, dtype=np.float64)
                    keep.append(a)
                    setattr(rf, f, _dp(a))
        rs = L.IpmRestart()
        rs.nstarts, rs.retry_mask, rs.flags = len(starts), int(retry_mask), int(flags)
        if len(starts):
            rs.starts = self._ipm_starts(starts, keep)
        nat = max(1, min(len(starts) + (X0 is not None), 8))
        if patience is not None:
            pat = np.ascontiguousarray(patience, dtype=np.int32)
            assert pat.size >= nat
            keep.append(pat)
            rs.patience = pat.ctypes.data_as(C.POINTER(C.c_int))
        nr = len(rungs)
        res = (L.IpmResult * max(1, nat * nr * B))()
        err = np.full((nat, max(1, nr), B), np.nan)
        summ = (L.IpmRestartResult * B)()
        A = self._ipm_addr
        fn = self.lib.emi_ipm_solve_restart_dev if dev else self.lib.emi_ipm_solve_restart_host
        st = fn(self.ctx, nr, arr, float(t0), float(tf), C.byref(rf) if rf is not None else None, C.byref(rs), A(X0), A(U0), ldm, A(X), A(U),
                A(LamF), A(LamC) if npth else None, res, _dp(err), summ)
        self._changed()
        self._trk_shape = self._wp_shape    # (an upper bound after an error)
        self._ck(st, fn.__name__)
        Ml = self.layout.M
        self.tau, self.w, self.D = lgl(Ml)
        self.node_t = t0 + (tf - t0) / 2.0 * (self.tau + 1.0)
        fields = [n for n, _ in L.IpmResult._fields_]
        results = [[[{n: getattr(res[(a * nr + r) * B + b], n) for n in fields} for b in range(B)] for r in range(nr)] for a in range(nat)]
        summary = [dict(attempt=q.attempt, attempts=q.attempts, level=q.level,
                        **{n: getattr(q.refine, n) for n, _ in L.IpmRefineResult._fields_}) for q in summ]
        return X, U, LamF, LamC, results, err[:, :nr], summary

    # ---- relative local ODE error of the batch on the collocation mesh (emi_ode_error_*, emi_interp_dev) ------------------------
    @staticmethod
    def ode_error_operator(M, mesh=None):
        """(E, Ed, tq): interpolation operator and its tau-derivative [5 (M-1)][M] at the Gauss points tq [5 (M-1)] of the mesh
        intervals, point q (M-1) + k = Gauss point q of interval k (host, emi_ode_error_operator); mesh: (tau, w, ..) of another
        node set than lgl(M)"""
        lib = L.load()
        tau, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (mesh if mesh is not None else lgl(M))[:2])
        n = 5 * (int(M) - 1)
        E, Ed, tq = np.empty((n, int(M))), np.empty((n, int(M))), np.empty(n)
        L.check(lib.emi_ode_error_operator(int(M), _dp(tau), _dp(w), _dp(E), _dp(Ed), _dp(tq)), what="emi_ode_error_operator")
        return E, Ed, tq

    def interp(self, OP, V, K=None, out=None):
        """out [.., :N] = V [.., K] OP[:, :K]^T on the matrix pipe (emi_interp_dev): OP [N][ldk] with ldk even and its rows zero
        padded beyond K (default K = ldk), torch tensors, float64; out's rows may be longer than N, the rest is not written;
        asynchronous"""
        N, ldk = OP.shape
        K = int(ldk if K is None else K)
        assert V.shape[-1] == K and OP.is_contiguous() and V.is_contiguous()
        R = V.numel() // K
        if out is None:
            out = torch.empty(tuple(V.shape[:-1]) + (N,), dtype=torch.float64, device=V.device)
        assert out.is_contiguous() and out.numel() == R * out.shape[-1]
        self._ck(self.lib.emi_interp_dev(self.ctx, K, int(N), int(ldk), C.c_void_p(OP.data_ptr()), C.c_void_p(V.data_ptr()), int(R),
                                         int(out.shape[-1]), C.c_void_p(out.data_ptr())), "emi_interp_dev")
        return out

    def ode_error(self, X, U, ul=None, uu=None, eta=True, dev=True):
        """(err [B], eta [B][ns][M-1] or None): the relative local ODE error of X [B][ns][M], U [B][nc][M] on the context's
        collocation mesh (include/emi355x.h, emi_ode_error_*); ul, uu [nc]: the controls' bounds the interpolated controls are
        clipped to.  dev=True: torch tensors on this device, asynchronous; dev=False: contiguous float64 numpy arrays."""
        lay = self.layout
        bd = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (ul, uu)]
        pb = [None if a is None else _dp(a) for a in bd]
        if dev:
            kw = dict(dtype=torch.float64, device=X.device)
            err = torch.empty((lay.B,), **kw)
            Eta = torch.empty((lay.B, lay.ns, lay.M - 1), **kw) if eta else None
        else:
            assert all(a.dtype == np.float64 and a.flags.c_contiguous for a in (X, U))
            err, Eta = np.empty(lay.B), (np.empty((lay.B, lay.ns, lay.M - 1)) if eta else None)
        A = self._ipm_addr
        fn = self.lib.emi_ode_error_dev if dev else self.lib.emi_ode_error_host
        self._ck(fn(self.ctx, A(X), A(U), pb[0], pb[1], A(Eta), A(err)), fn.__name__)
        return err, Eta

    @staticmethod
    def ode_error_delay_operator(M, mesh=None, t0=0.0, tf=1.0, delay=0.0):
        """Edel [5 (M-1)][M]: row p is the Lagrange basis of the mesh at the node coordinate of max(t_p - delay, t0), t_p the time
        of point p of ode_error_operator on [t0, tf] (host, emi_ode_error_delay_operator)"""
        lib = L.load()
        tau, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (mesh if mesh is not None else lgl(M))[:2])
        Edel = np.empty((5 * (int(M) - 1), int(M)))
        L.check(lib.emi_ode_error_delay_operator(int(M), _dp(tau), _dp(w), float(t0), float(tf), float(delay), _dp(Edel)),
                what="emi_ode_error_delay_operator")
        return Edel

    def ode_error_total(self, X, U, ul=None, uu=None, eta=True, dev=True):
        """ode_error for a context with or without delays (emi_ode_error_total_*): U [B][ncf][M] holds the FREE controls and ul, uu
        [ncf] their bounds; the delayed values between the nodes are those of the interpolants at max(t - i dt, t0), a delayed
        control clipped with its source's bounds.  Without delays this is ode_error, bit for bit."""
        lay = self.layout
        bd = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (ul, uu)]
        pb = [None if a is None else _dp(a) for a in bd]
        if dev:
            kw = dict(dtype=torch.float64, device=X.device)
            err = torch.empty((lay.B,), **kw)
            Eta = torch.empty((lay.B, lay.ns, lay.M - 1), **kw) if eta else None
        else:
            assert all(a.dtype == np.float64 and a.flags.c_contiguous for a in (X, U))
            err, Eta = np.empty(lay.B), (np.empty((lay.B, lay.ns, lay.M - 1)) if eta else None)
        A = self._ipm_addr
        fn = self.lib.emi_ode_error_total_dev if dev else self.lib.emi_ode_error_total_host
        self._ck(fn(self.ctx, A(X), A(U), pb[0], pb[1], A(Eta), A(err)), fn.__name__)
        return err, Eta

    # ---- measurement -----------------------------------------------------------
    def timer_start(self):
        self._ck(self.lib.emi_timer_start(self.ctx), "emi_timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._ck(self.lib.emi_timer_stop(self.ctx, C.byref(ms)), "emi_timer_stop")
        return ms.value

    def profile(self, level):
        """0 off, 1 every bracket, 2 the defect (MFMA) kernel only, 3 the node kernel only (include/emi355x.h)"""
        self._ck(self.lib.emi_profile_enable(self.ctx, int(level)), "emi_profile_enable")

    def profile_read(self):
        nm, dm, fm = C.c_float(), C.c_float(), C.c_float()
        nl, dl, fl = C.c_int(), C.c_int(), C.c_int()
        self._ck(self.lib.emi_profile_read(self.ctx, C.byref(nm), C.byref(nl), C.byref(dm), C.byref(dl), C.byref(fm),
                                           C.byref(fl)), "emi_profile_read")
        return dict(node_ms=nm.value, node_launches=nl.value, defect_ms=dm.value, defect_launches=dl.value,
                    pass_ms=fm.value, overlapped_passes=fl.value)

    def set_option(self, name, value):
        self._ck(self.lib.emi_set_option(self.ctx, name.encode(), int(value)), "emi_set_option")

    def plan(self, B=None):
        """What the default dispatch does with a batch of B instances (default: the batch set): dict of emi_pass_plan_t."""
        p = L.PassPlan()
        self._ck(self.lib.emi_plan_pass(self.ctx, int(B if B is not None else self.layout.B), C.byref(p)), "emi_plan_pass")
        return {n: getattr(p, n) for n, _ in L.PassPlan._fields_}

    def plan_residency(self, B=None):
        """Resident workgroups per CU the (first) launch of plan(B) states: 2 or 3; 0 where the pass does not go out as one launch."""
        res = C.c_int(0)
        self._ck(self.lib.emi_plan_pass_residency(self.ctx, int(B if B is not None else self.layout.B), C.byref(res)), "emi_plan_pass_residency")
        return res.value

    @property
    def pass_work_uploads(self):
        """(work tables of the one-launch pass this context has built and uploaded so far, tables it holds now): a call whose launch
        was seen before uploads nothing."""
        n, held = C.c_ulonglong(0), C.c_int(0)
        self._ck(self.lib.emi_debug_pass_work_uploads(self.ctx, C.byref(n), C.byref(held)), "emi_debug_pass_work_uploads")
        return n.value, held.value

    @property
    def last_defect_kernel(self):
        return self.lib.emi_last_defect_kernel(self.ctx).decode()

    @property
    def uses_fused_kernel(self):
        f = C.c_int()
        self._ck(self.lib.emi_last_path(self.ctx, C.byref(f)), "emi_last_path")
        return bool(f.value)



PASS_WORK_INFO = ("blocks", "nm", "nn", "nm8", "nn8", "nbx", "ntiles", "ngrp", "cpart", "cx", "ks", "nsg")


def debug_pass_work(ns, B, M, sw, ctc=1, ksplit=1, hs=1, sym_cpart=0, sym_gblk=0, sym_cx=0, order=0):
    """The work table of a launch of the one-launch pass, without a device (emi_debug_pass_work): (table, info) or None where
    plan_symdefect admits no such launch.  table[g] = (role, ntile | bx, grp | b, K slice | second bx, second b) of grid block g."""
    lib = L.load()
    info = (C.c_int * 12)()
    args = [int(v) for v in (ns, B, M, sw, ctc, ksplit, hs, sym_cpart, sym_gblk, sym_cx, order)]
    if lib.emi_debug_pass_work(*args, None, 0, info) != 0:
        return None
    table = np.zeros((info[0], 5), dtype=np.intc)
    st = lib.emi_debug_pass_work(*args, table.ctypes.data_as(C.POINTER(C.c_int)), table.size, info)
    if st != 0:
        raise L.EmiError(f"emi_debug_pass_work: status {st}")
    return table, dict(zip(PASS_WORK_INFO, info))
