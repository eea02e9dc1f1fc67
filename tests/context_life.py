"""A context with a history: the configuration mirror, the step alphabet, the lives and the seeded walks that
tests/test_gpu_context_life.py and tests/test_gpu_stream_order.py run, and tests/test_context_life_cpu.py checks without a GPU.

A life is a list of Step.  A SETTER step changes the lived context and the Config that mirrors it; a CALLING step draws its inputs from
its own seed (no two steps of a life share one), runs one call of the library into poisoned buffers with a poisoned slack region behind
each, and is then repeated with the same inputs on fresh(config): a new Evaluator set up from the mirror in the canonical order
    create, set_mesh, set_model / set_model_source, set_delays, set_batch, set_track_waypoints, tracks_from_waypoints /
    set_tracks, set_path, kkt_blocks_rows, options by name
which is closed at once.  Every output must have the bits of the fresh context's.

A call is built in two phases (make_call): the device tensors of its inputs and its poisoned outputs first, invoke() second.  The
stream-order test puts its own protocol between the two; run_call() here is the suite's usual one (device synchronised before, context
synchronised after).  Importing this module needs neither the GPU nor the native library."""
import copy
import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = 64                  # poisoned elements behind every output buffer
NAN = float("nan")
INF = 1e20
DC = 1e-9
QUAD, POINTMASS, FIXEDWING = 1, 0, 2


# ---- the mirror --------------------------------------------------------------------------------------------------------------------
@dataclass
class Config:
    """everything that was applied to a context and is still in force (what the library drops, the mirror drops: emi_set_mesh the
    track centres, emi_set_model* the delays and the record table)"""
    f32: bool = False
    M: int = 0
    t0: float = 0.0
    tf: float = 1.0
    model: object = None            # a built-in model's number, or None with `source`
    source: object = None           # key of SOURCES
    params: tuple = ()
    maximize: bool = False
    B: int = 0
    recs: object = None             # [np][8] or [B][np][8]
    per_instance: bool = False      # the table has a set per instance (and follows the batch)
    px: int = 0
    py: int = 1
    tracks: object = None           # (xc, yc) given with set_tracks
    waypoints: object = None        # (t, x, y, counts): the tables, which outlive a mesh
    wp_map: object = None           # "all" or a list: the centres on this mesh were made from the tables
    delays: object = None           # (x_horizon, u_horizon, dt)
    blk_rows: object = None
    options: dict = field(default_factory=dict)     # every option that is not at its default


OPTION_DEFAULTS = dict(overlap=1, sym_ct=0, node_store=-1, overlap_mode=0, sym_ksplit=0, sym_combine=1, sym_cpart=0, sym_gblk=0, sym_nst=3,
                       pass_order=-1, sym_hs=0, sym_ctc=0, sym_bk=0, sym_dop=0, sym_res=0, f32_ring=1, f32_one_launch=0, small_rows=24)


def _harness():
    h = C.CDLL(os.path.join(ROOT, "tests", "harness", "libetol_harness.so"))
    h.harness_last_message.restype = C.c_char_p
    h.harness_traced_model_source.restype = C.c_char_p
    return h


def _traced_rows_source():
    return _harness().harness_traced_model_source(2).decode()


def _delayed_source():
    h = _harness()
    z, res, vals = np.zeros(4 * 9), np.zeros(64 * 9), np.zeros(256 * 9)
    cost, nres, nvals = C.c_double(), C.c_int(), C.c_int()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert h.harness_delay_demo(8, C.c_double(0.5), 3, 1, 0, dp(z), dp(res), res.size, dp(vals), vals.size, C.byref(cost), C.byref(nres),
                                C.byref(nvals)) == 0
    return h.harness_last_message().decode()


# key -> (text, ns, nc as compiled, npath, path_vars, states like this built-in model)
SOURCES = {
    "traced_rows": (_traced_rows_source, 6, 2, 2, (0, 1), QUAD),    # the quadrotor with a disc and an edge ellipse as traced rows
    "delayed": (_delayed_source, 2, 8, 0, (), POINTMASS),           # 2 states, 2 free controls + x(t-dt), x(t-2dt), u(t-dt)
}
_source_text = {}


def source_text(key):
    if key not in _source_text:
        _source_text[key] = SOURCES[key][0]()
    return _source_text[key]


def fresh(cfg):
    """a new Evaluator from the mirror, in the canonical order, and nothing else (on its own stream: a context is put on a caller's
    stream by the test that is about that, tests/test_gpu_stream_order.py)"""
    import torch
    import etol_amd as E
    ev = E.Evaluator(0, f32=cfg.f32)
    ev.set_mesh(cfg.M, cfg.t0, cfg.tf)
    if cfg.source is not None:
        _, ns, nc, npath, pv, _ = SOURCES[cfg.source]
        ev.set_model_source("TracedModel", source_text(cfg.source), ns, nc, params=cfg.params, maximize=cfg.maximize, npath=npath, path_vars=pv)
    else:
        ev.set_model(cfg.model, cfg.params, maximize=cfg.maximize)
    if cfg.delays is not None:
        ev.set_delays(*cfg.delays)
    ev.set_batch(cfg.B)
    if cfg.waypoints is not None:
        t, x, y, counts = cfg.waypoints
        ev.set_track_waypoints(t, x, y, counts)
        if cfg.wp_map is not None:
            ev.tracks_from_waypoints(None if cfg.wp_map == "all" else torch.tensor(cfg.wp_map, dtype=torch.int32, device=ev.device))
    if cfg.tracks is not None:
        ev.set_tracks(*cfg.tracks)
    if cfg.recs is not None:
        ev.set_path(cfg.recs, cfg.px, cfg.py)
    if cfg.blk_rows is not None:
        ev.kkt_blocks_rows(cfg.blk_rows)
    for name in sorted(cfg.options):
        ev.set_option(name, cfg.options[name])
    return ev


# ---- steps -------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Step:
    kind: str
    args: tuple = ()        # sorted (name, value) pairs of a setter, or of a call's variant
    seed: int = -1          # calling steps: the seed of the inputs

    def __str__(self):
        a = ", ".join(f"{k}={v}" for k, v in self.args)
        return f"{self.kind}({a})" + (f" seed {self.seed}" if self.seed >= 0 else "")

    def arg(self, name, default=None):
        return dict(self.args).get(name, default)


def S(kind, seed=-1, **args):
    return Step(kind, tuple(sorted(args.items())), seed)


def disc_records(seed, sets, npth):
    """[sets][np][8] discs inside the box the inputs live in (a shared table: sets = 1)"""
    rng = np.random.default_rng(seed)
    recs = np.zeros((sets, npth, 8))
    recs[:, :, 0] = 1
    recs[:, :, 1:3] = rng.uniform(1.0, 9.0, (sets, npth, 2))
    recs[:, :, 3] = rng.uniform(0.2, 0.6, (sets, npth)) ** 2
    return recs


def waypoint_tables(seed, sets, ntracks, ld=4):
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(0.5, 6.0, (sets, ntracks, ld)), axis=2)
    t[:, :, 0] = 0.0
    return t, rng.uniform(0, 7, (sets, ntracks, ld)), rng.uniform(0, 7, (sets, ntracks, ld)), rng.integers(2, ld + 1, (sets, ntracks))


def track_records(ntracks, discs_seed, ndiscs):
    """a shared table: the moving discs first, then static ones"""
    recs = np.zeros((ntracks + ndiscs, 8))
    recs[:ntracks, 0], recs[:ntracks, 1], recs[:ntracks, 2] = 2, np.arange(ntracks), 0.16
    recs[ntracks:] = disc_records(discs_seed, 1, ndiscs)[0]
    return recs


def default_rows(ns, nv, npth, px=0, py=1):
    return [[(px, ns * nv + 2 * j), (py, ns * nv + 2 * j + 1)] for j in range(npth)]


# setters: name -> f(ev or None, cfg, step).  Each changes the mirror and, where there is a context, the context in the same way.
def _set_mesh(ev, cfg, st):
    cfg.M, cfg.t0, cfg.tf = st.arg("M"), st.arg("t0", cfg.t0), st.arg("tf", cfg.tf)
    cfg.tracks, cfg.wp_map = None, None
    if ev is not None:
        ev.set_mesh(cfg.M, cfg.t0, cfg.tf)


def _set_model(ev, cfg, st):
    from etol_amd import workloads as W
    cfg.model, cfg.source, cfg.maximize = st.arg("model"), st.arg("source"), bool(st.arg("maximize", False))
    cfg.params = tuple({QUAD: W.QUAD_PARAMS, FIXEDWING: W.FW_PARAMS}.get(cfg.model, ()))
    cfg.delays, cfg.recs, cfg.per_instance = None, None, False
    if ev is None:
        return
    if cfg.source is not None:
        _, ns, nc, npath, pv, _ = SOURCES[cfg.source]
        ev.set_model_source("TracedModel", source_text(cfg.source), ns, nc, params=cfg.params, maximize=cfg.maximize, npath=npath, path_vars=pv)
    else:
        ev.set_model(cfg.model, cfg.params, maximize=cfg.maximize)


def _set_batch(ev, cfg, st):
    """the batch, and with a table per instance the table of that many sets (the library refuses another number of sets)"""
    cfg.B = st.arg("B")
    if ev is not None:
        ev.set_batch(cfg.B)
    if cfg.recs is not None and cfg.per_instance:
        cfg.recs = disc_records(st.arg("table", 7), cfg.B, cfg.recs.shape[1])
        if ev is not None:
            ev.set_path(cfg.recs, cfg.px, cfg.py)


def _set_path(ev, cfg, st):
    npth, per = st.arg("np"), st.arg("per_instance", False)
    cfg.per_instance = bool(per) and not st.arg("tracks")
    if st.arg("tracks"):
        cfg.recs = track_records(st.arg("tracks"), st.arg("table", 7), npth)
    else:
        cfg.recs = disc_records(st.arg("table", 7), cfg.B if per else 1, npth)
    cfg.px, cfg.py = st.arg("px", 0), st.arg("py", 1)
    if ev is not None:
        ev.set_path(cfg.recs, cfg.px, cfg.py)


def _set_tracks(ev, cfg, st):
    rng = np.random.default_rng(st.arg("table", 3))
    n = st.arg("n")
    cfg.tracks, cfg.wp_map = (rng.uniform(0, 7, (1, n, cfg.M)), rng.uniform(0, 7, (1, n, cfg.M))), None
    if ev is not None:
        ev.set_tracks(*cfg.tracks)


def _set_waypoints(ev, cfg, st):
    cfg.waypoints = waypoint_tables(st.arg("table", 5), st.arg("sets", 1), st.arg("n"))
    if ev is not None:
        ev.set_track_waypoints(*cfg.waypoints)


def _set_delays(ev, cfg, st):
    d = (st.arg("xh"), st.arg("uh"), st.arg("dt"))
    cfg.delays = d if (d[0] > 1 or d[1] > 0) else None
    if ev is not None:
        ev.set_delays(*d)


def _set_rows(ev, cfg, st):
    cfg.blk_rows = default_rows(st.arg("ns"), st.arg("nv"), st.arg("np"))
    if ev is not None:
        ev.kkt_blocks_rows(cfg.blk_rows)


def _set_option(ev, cfg, st):
    name, value = st.arg("name"), st.arg("value")
    if value == OPTION_DEFAULTS[name]:
        cfg.options.pop(name, None)
    else:
        cfg.options[name] = value
    if ev is not None:
        ev.set_option(name, value)


SETTERS = {"mesh": _set_mesh, "model": _set_model, "batch": _set_batch, "path": _set_path, "tracks": _set_tracks, "waypoints": _set_waypoints,
           "delays": _set_delays, "rows": _set_rows, "option": _set_option}

# ---- calls -------------------------------------------------------------------------------------------------------------------------
DEV_CALLS = ("eval_all", "eval_nojac", "eval_split", "eval_repeat", "eval_flagged", "hess", "lagr_grad", "certificate", "lagr_grad_total", "certificate_total",
             "ode_error", "ode_error_total", "blocks", "shard", "factor_solve", "ipm", "prolong_rows", "shard_move", "repair_guess", "start_guess",
             "tracks_from_waypoints", "kkt_solve", "shard_solve")
HOST_CALLS = ("eval_host", "hess_host", "lagr_grad_host", "certificate_host", "lagr_grad_total_host", "certificate_total_host", "ode_error_host",
              "ode_error_total_host", "blocks_host", "ipm_host", "start_guess_host", "factor_solve_host")
DRIVER_CALLS = ("ipm_solve_ladder",)
CALLS = DEV_CALLS + HOST_CALLS + DRIVER_CALLS


def like_model(cfg):
    return SOURCES[cfg.source][5] if cfg.source is not None else cfg.model


def point(cfg, rng, B, ns, ncf, M):
    """(X [B][ns][M], U [B][ncf][M]) where the model's functions are smooth, new for every seed"""
    m = like_model(cfg)
    u = lambda lo, hi, *s: rng.uniform(lo, hi, s)
    if m == QUAD:
        lo, hi = np.array([0, 0, -np.pi / 4, -2, -2, -1.0]), np.array([10, 10, np.pi / 4, 2, 2, 1.0])
        X = lo[:, None] + (hi - lo)[:, None] * u(0, 1, B, 6, M)
        U = np.stack([9.81 * u(0.5, 1.5, B, M), u(-0.1, 0.1, B, M)], axis=1)
    elif m == FIXEDWING:
        sx = np.array([100, 100, 50, 0.4, 0.3, 3.0, 5, 2, 2, 0.5, 0.5, 0.5])
        ox = np.array([0, 0, -100, 0, 0, 0, 25, 0, 0, 0, 0, 0.0])
        X = ox[:, None] + sx[:, None] * u(-1, 1, B, 12, M)
        U = np.array([30, 0, 0, 0.0])[:, None] + np.array([20, 0.3, 0.3, 0.3])[:, None] * u(-1, 1, B, 4, M)
    else:
        X, U = 7.0 * u(0, 1, B, ns, M), u(-0.5, 0.5, B, ncf, M)
    assert X.shape == (B, ns, M) and U.shape == (B, ncf, M)
    if cfg.f32:
        X, U = X.astype(np.float32), U.astype(np.float32)
    return np.ascontiguousarray(X), np.ascontiguousarray(U)


class Call:
    """one call of the library: device inputs (name -> tensor holding the real values), poisoned outputs with their slack, invoke()"""

    def __init__(self, ev, kind):
        import torch
        self.ev, self.kind, self.torch = ev, kind, torch
        self.inputs, self.outputs, self.host, self._guards = {}, {}, {}, []
        self.synchronising = False          # the entry point is documented to synchronise (it returns host values)

    def put(self, name, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).copy()).to(self.ev.device)
        self.inputs[name] = t
        return t

    def out(self, name, shape, dtype=None, fill=NAN):
        n = int(np.prod(shape))
        flat = self.torch.full((n + SLACK,), fill, dtype=dtype or self.ev.dtype, device=self.ev.device)
        self._guards.append((name, flat, n, fill))
        self.outputs[name] = flat[:n].view(*shape)
        return self.outputs[name]

    def inout(self, name, a):
        """an array the call changes in place: an input whose buffer has a slack region, and an output"""
        a = np.ascontiguousarray(a)
        t = self.out(name, a.shape, dtype=self.torch.float64)
        t.copy_(self.torch.from_numpy(a.copy()))
        self.inputs[name] = t
        return t

    def check_slack(self):
        for name, flat, n, fill in self._guards:
            tail = flat[n:]
            ok = tail.isnan().all() if isinstance(fill, float) and np.isnan(fill) else (tail == fill).all()
            assert bool(ok), f"{self.kind}: written behind {name}"

    def results(self):
        """every output as numpy (after a synchronisation of whatever stream the call ran on)"""
        out = {k: v.cpu().numpy() for k, v in self.outputs.items()}
        out.update({k: np.asarray(v) for k, v in self.host.items()})
        return out


def _bounds(rng, Z, nsets):
    """zl, zu [nsets][nv][M] round the point Z [B][nv][M]: free, lower, upper, boxed, fixed and violated entries"""
    zref = Z[:nsets].astype(np.float64)
    spread = np.abs(Z).max(axis=(0, 2), keepdims=True) + 1.0
    kind = rng.integers(0, 6, size=zref.shape)
    lo, up = zref - spread * rng.uniform(0.01, 1.0, zref.shape), zref + spread * rng.uniform(0.01, 1.0, zref.shape)
    zl, zu = np.where(np.isin(kind, (1, 3)), lo, -INF), np.where(np.isin(kind, (2, 3)), up, INF)
    zl, zu = np.where(kind == 4, zref, zl), np.where(kind == 4, zref, zu)
    zl, zu = np.where(kind == 5, up, zl), np.where(kind == 5, up + spread, zu)
    return np.ascontiguousarray(zl), np.ascontiguousarray(zu)


def _row_bounds(npth):
    cl, cu = np.full(npth, -INF), np.zeros(npth)
    cl[1::3] = -2.0
    cl[2::3], cu[2::3] = 0.5, INF
    return cl, cu


def _spd_blocks(rng, B, nv, M):
    """packed lower triangles [B][nh][M] of A A^T + nv I"""
    A = rng.standard_normal((B, M, nv, nv))
    Q = np.einsum("bkij,bklj->bkil", A, A) + nv * np.eye(nv)
    il = np.tril_indices(nv)
    return np.ascontiguousarray(np.transpose(Q[:, :, il[0], il[1]], (0, 2, 1)))


def _newton_inputs(ev, rng, lay):
    """Q, VALS, fixed of kkt_shard_ref.shard_blocks' kind for the whole batch: SPD node blocks, Jacobian entries with diag D added, the
    initial state fixed"""
    B, ns, nv, M = lay.B, lay.ns, lay.ns + lay.nc, lay.M
    Q = _spd_blocks(rng, B, nv, M)
    VALS = rng.standard_normal((B, lay.nvals, M))
    for i in range(ns):
        VALS[:, i * nv + i] += np.diag(ev.D)
    fixed = np.zeros((B, nv, M), dtype=np.uint8)
    fixed[:, :ns, 0] = 1
    return Q, VALS, fixed


def _blocks_inputs(rng, lay):
    """H, VALS, Sigma, SigT, fixed: node blocks of which about a third are indefinite (they get pairs), with fixed variables"""
    B, nv, M, npth = lay.B, lay.ns + lay.nc, lay.M, lay.np
    A = rng.standard_normal((B, M, nv, nv)) / np.sqrt(nv)
    sgn = np.where(rng.random((B, M, nv)) < 0.02, -1.0, 1.0) * rng.uniform(0.5, 2.0, (B, M, nv))
    Q = np.einsum("bkij,bkj,bklj->bkil", A + np.eye(nv), sgn, A + np.eye(nv))
    il = np.tril_indices(nv)
    H = np.ascontiguousarray(np.transpose(Q[:, :, il[0], il[1]], (0, 2, 1)))
    fixed = np.zeros((B, nv, M), dtype=np.uint8)
    pat = rng.random((B, M))
    fixed[:, :, :][np.broadcast_to((pat < 0.1)[:, None, :], fixed.shape)] = 1
    fixed[:, 0, :][(pat >= 0.1) & (pat < 0.3)] = 1
    Sigma = np.where(fixed != 0, 0.0, rng.uniform(0, 1, (B, nv, M)) * (rng.random((B, nv, M)) < 0.7))
    return H, 0.3 * rng.standard_normal((B, lay.nvals, M)), Sigma, 10.0 ** rng.uniform(-3, 0, (B, npth, M)), fixed


def make_call(ev, cfg, st):
    """the Call of a calling step on ev (the lived context or a fresh one): same step, same tensors' values"""
    import torch
    import etol_amd as E
    kind, rng = st.kind, np.random.default_rng(st.seed)
    lay = ev.layout
    B, ns, nc, npth, M, nvals = lay.B, lay.ns, lay.nc, lay.np, lay.M, lay.nvals
    nd = ev.n_delayed
    ncf, nv, nvf = nc - nd, ns + nc, ns + nc - nd
    c = Call(ev, kind)
    f64 = torch.float64
    X, U = point(cfg, rng, B, ns, ncf, M)
    real = (lambda a: a.astype(np.float32)) if cfg.f32 else (lambda a: a)

    if kind in ("eval_all", "eval_nojac", "eval_split"):
        dX, dU = c.put("X", X), c.put("U", U)
        RES, VALS, COST = c.out("RES", (B, lay.nres, M)), c.out("VALS", (B, nvals, M)), c.out("COST", (B,))
        if kind == "eval_split":
            def invoke():
                ev.eval_dev(dX, dU, RES, VALS, COST, flags=E.EVAL_NODES)
                ev.eval_dev(dX, dU, RES, None, None, flags=E.EVAL_DEFECT)
        else:
            flags = E.EVAL_ALL | (E.EVAL_NOJAC if kind == "eval_nojac" else 0)
            invoke = lambda: ev.eval_dev(dX, dU, RES, VALS, COST, flags=flags)
        c.point = (X, U)
    elif kind == "hess":
        dX, dU = c.put("X", X), c.put("U", U)
        lF, lC = c.put("lamF", real(rng.standard_normal((B, ns, M)))), c.put("lamC", real(rng.standard_normal((B, npth, M)))) if npth else None
        H = c.out("H", (B, lay.nhess, M))
        sigma = float(rng.uniform(0.5, 1.5))
        invoke = lambda: ev.hess_dev(dX, dU, lF, lC, sigma, H)
    elif kind in ("lagr_grad", "lagr_grad_total", "certificate", "certificate_total"):
        total = kind.endswith("total")
        nu = nvf if total else nv
        V = c.put("VALS", rng.standard_normal((B, nvals, M)))
        lF, lC = c.put("lamF", rng.standard_normal((B, ns, M))), c.put("lamC", rng.standard_normal((B, npth, M))) if npth else None
        sigma = float(rng.uniform(0.5, 1.5))
        G = c.out("G", (B, nu, M), dtype=f64)
        Gdel = c.out("Gdel", (B, nd, M), dtype=f64) if total and nd else None
        if kind == "lagr_grad":
            invoke = lambda: ev.lagr_grad_dev(V, lF, lC, sigma, G)
        elif kind == "lagr_grad_total":
            invoke = lambda: ev.lagr_grad_total_dev(V, lF, lC, sigma, G, Gdel)
        else:
            Uc = U if total else np.concatenate([U, rng.uniform(-0.5, 0.5, (B, nd, M))], axis=1)
            dX, dU, R = c.put("X", X), c.put("U", Uc), c.put("RES", rng.standard_normal((B, lay.nres, M)))
            nsets = B if st.seed % 2 else 1
            zl, zu = _bounds(rng, np.concatenate([X, Uc], axis=1), nsets)
            dzl, dzu = c.put("zl", zl), c.put("zu", zu)
            cl, cu = _row_bounds(npth)
            cert = c.out("cert", (B, 6), dtype=f64)
            if total:
                invoke = lambda: ev.kkt_certificate_total_dev(dX, dU, R, V, lF, lC, sigma, dzl, dzu, cl, cu, cert, G, Gdel)
            else:
                invoke = lambda: ev.kkt_certificate_dev(dX, dU, R, V, lF, lC, sigma, dzl, dzu, cl, cu, cert, G)
    elif kind in ("ode_error", "ode_error_total"):
        dX, dU = c.put("X", X), c.put("U", U)
        ul, uu = U.min(axis=(0, 2)) + 0.1, U.max(axis=(0, 2)) - 0.1        # the interpolated controls do reach them
        fn = ev.lib.emi_ode_error_dev if kind == "ode_error" else ev.lib.emi_ode_error_total_dev
        err, eta = c.out("err", (B,), dtype=f64), c.out("eta", (B, ns, M - 1), dtype=f64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        A = ev._ipm_addr
        invoke = lambda: ev._ck(fn(ev.ctx, A(dX), A(dU), dp(ul), dp(uu), A(eta), A(err)), kind)
    elif kind in ("blocks", "shard"):
        H, V, Sg, St, fx = _blocks_inputs(rng, lay)
        if kind == "shard":                 # the Jacobian entries a factorisation needs: diag D on the states' own entries
            for i in range(ns):
                V[:, i * nv + i] += np.diag(ev.D)
            fx[:] = 0
            fx[:, :ns, 0] = 1
            Sg = np.where(fx != 0, 0.0, Sg)
        dH, dV, dSg, dfx = c.put("H", H), c.put("VALS", V), c.put("Sigma", Sg), c.put("fixed", fx)
        dSt = c.put("SigT", St) if npth else None
        mm = nv * M
        Q, Qx = c.out("Q", (B, lay.nhess, M), dtype=f64), c.out("Qexact", (B, lay.nhess, M), dtype=f64)
        count, node = c.out("count", (B,), dtype=torch.int32, fill=-5), c.out("node", (B, mm), dtype=torch.int32, fill=-7)
        delta, vec, worst = c.out("delta", (B, mm), dtype=f64), c.out("vec", (B, mm, nv), dtype=f64), c.out("worst", (B,), dtype=f64)
        blocks = lambda: ev.kkt_blocks_dev(dH, dV, dSg, dSt, dfx, 1e-4 if npth else 0.0, Q, mm, count, node, delta, vec, worst, Qexact=Qx)
        if kind == "blocks":
            invoke = blocks
        else:
            rhs = c.inout("rhs", rng.standard_normal((B, nv + ns, M)))
            c.synchronising = True

            def invoke():
                blocks()
                c.host["info"] = ev.kkt_factor_shard_dev(Q, dV, dfx, DC)
                c.host["exact"] = ev.kkt_lowrank_shard_dev(mm, count, node, delta, vec)
                out = ev.kkt_solve_refined_shard_dev(rhs, DC, max_steps=4)
                c.host.update({"refined." + k: v for k, v in out.items()})
    elif kind == "factor_solve":
        Q, V, fx = _newton_inputs(ev, rng, lay)
        dQ, dV, dfx = c.put("Q", Q[0]), c.put("J", V[0]), c.put("fixed", fx[0].reshape(-1))
        rhs = c.inout("rhs", rng.standard_normal((2, (nv + ns) * M)))
        c.synchronising = True

        def invoke():
            c.host["info"] = np.array([ev.kkt_factor_dev(dQ, dV, dfx, DC)])
            ev.kkt_solve_dev(rhs)
    elif kind in ("kkt_solve", "shard_solve"):
        # the asynchronous solve on its own: the factorisation it answers for is made here, synchronised (kkt_factor*_dev return host
        # values), so that invoke() is one entry point that returns nothing to the host
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
        Q, V, fx = _newton_inputs(ev, rng, lay)
        torch.cuda.synchronize()
        if kind == "kkt_solve":
            assert ev.kkt_factor_dev(up(Q[0]), up(V[0]), up(fx[0].reshape(-1)), DC) == 0
            rhs = c.inout("rhs", rng.standard_normal((2, (nv + ns) * M)))
            invoke = lambda: ev.kkt_solve_dev(rhs)
        else:
            assert not ev.kkt_factor_shard_dev(up(Q), up(V), up(fx), DC).any()
            assert (ev.kkt_lowrank_shard_dev(0) == 1).all()
            rhs = c.inout("rhs", rng.standard_normal((B, nv + ns, M)))
            invoke = lambda: ev.kkt_solve_shard_dev(rhs)
    elif kind == "prolong_rows":
        Mc = int(rng.choice([9, 21, 33, 65]))
        R, rows = 3 * B + 1, 5 * B
        PT = c.put("PT", np.ascontiguousarray(E.Evaluator.prolong_matrix(Mc, M).T))
        Vc = c.put("Vc", rng.standard_normal((rows, Mc)))
        rmap = c.put("row_map", rng.integers(0, rows, R).astype(np.int32))
        Vf = c.out("Vf", (R, M), dtype=f64)
        invoke = lambda: ev.prolong_rows(PT, Vc, rmap, Vf)
    elif kind == "shard_move":
        n, ld = max(1, B // 2), M + 3
        src = [c.put(f"src{q}", rng.standard_normal((B, r, M))) for q, r in enumerate((ns, ncf, 1))]
        dst = [c.out(f"dst{q}", (B, r, ld), dtype=f64) for q, r in enumerate((ns, ncf, 1))]
        si, di = c.put("src_idx", rng.permutation(B)[:n].astype(np.int32)), c.put("dst_idx", rng.permutation(B)[:n].astype(np.int32))
        invoke = lambda: ev.shard_move(src, dst, M - 1, si, di)
    elif kind == "repair_guess":
        dX = c.inout("X", X)
        invoke = lambda: ev.repair_guess(dX)
    elif kind == "start_guess":
        which = (E.START_LINE, E.START_BEND, E.START_PLANNED)[st.seed % 3]
        xa, xb = (np.ascontiguousarray(a, dtype=np.float64) for a in point(cfg, rng, B, ns, ncf, 2)[0].transpose(2, 0, 1))
        Xs, level = c.out("X", (B, ns, M), dtype=f64), c.out("level", (B,), dtype=torch.int32, fill=-9)
        stt = E._lib.Start(kind=int(which), nsets=B, xa=xa.ctypes.data_as(C.POINTER(C.c_double)), xb=xb.ctypes.data_as(C.POINTER(C.c_double)),
                           bend=0.7, clearance=0.01, grid=17, repair=int(st.seed % 2))
        c.keep = (xa, xb, stt)
        invoke = lambda: ev._ck(ev.lib.emi_start_guess_dev(ev.ctx, C.byref(stt), ev._ipm_addr(Xs), ev._ipm_addr(level)), "emi_start_guess_dev")
    else:
        raise KeyError(kind)
    c.invoke = invoke
    return c


def run_call(c):
    """the suite's usual manner: device synchronised before the call, the context after it"""
    c.torch.cuda.synchronize()
    c.invoke()
    c.ev.synchronize()
    c.torch.cuda.synchronize()
    c.check_slack()
    return c.results()


def adjoint_forks(B, ns, M, cus=256):
    """whether emi_lagr_grad_* runs the operator product on the context's second stream beside the node kernel (adjoint_side_by_side in
    etol_amd/csrc/emi_adjoint.hip; tests/test_context_life_cpu.py holds this copy to that text)"""
    return ((B * ns + 95) // 96) * ((M + 127) // 128) >= cus


# ---- calls that are not one entry point on device tensors --------------------------------------------------------------------------
def ipm_case(ev, cfg, st):
    import ipm_ref as R
    lay = ev.layout
    nv = lay.ns + lay.nc
    c = R.make_case(nv, lay.ns, lay.np, lay.M, lay.B, 1 if st.seed % 2 else lay.B, st.seed, cscale=bool(0 < lay.np <= 3 and st.seed % 3 == 0),
                    rs=st.seed % 5 == 0, soc=st.seed % 7 == 0, rows=cfg.blk_rows)
    assert c["nvals"] == lay.nvals
    return c


def run_ipm(ev, cfg, st, dev):
    """every output of reduce, expand, trial, merit (both resets), accept and error (test_gpu_ipm.all_outputs) on a case of this seed;
    the device form's poisoned outputs get a slack region each"""
    import torch
    import test_gpu_ipm as TI

    class Guarded(TI.DevBackend):
        def __init__(self, ev, dev):
            super().__init__(ev, dev=dev)
            self.guards = []

        def poison(self, *shape):
            n = int(np.prod(shape))
            if not n:
                return None
            if not self.dev:
                return np.full(shape, np.nan)
            flat = torch.full((n + SLACK,), NAN, dtype=torch.float64, device=self.ev.device)
            self.guards.append((flat, n))
            return flat[:n].view(*shape)

    be = Guarded(ev, dev=dev)
    out = TI.all_outputs(ipm_case(ev, cfg, st), be)[0]
    for flat, n in be.guards:
        assert bool(flat[n:].isnan().all()), "ipm: written behind an output"
    return out


def run_host(ev, cfg, st):
    """the _host form of a call on numpy arrays (the wrapper owns the output arrays: no slack there)"""
    import etol_amd as E
    kind, rng = st.kind, np.random.default_rng(st.seed)
    lay = ev.layout
    B, ns, nc, npth, M, nvals = lay.B, lay.ns, lay.nc, lay.np, lay.M, lay.nvals
    nd = ev.n_delayed
    ncf, nv = nc - nd, ns + nc
    X, U = (a.astype(np.float64) for a in point(cfg, rng, B, ns, ncf, M))
    lamF, lamC, sigma = rng.standard_normal((B, ns, M)), rng.standard_normal((B, npth, M)), float(rng.uniform(0.5, 1.5))
    if kind == "eval_host":
        out = dict(zip(("RES", "VALS", "COST"), ev.eval_host(X, U)))
        out["point"] = (X, U)
        return out
    if kind == "hess_host":
        return dict(H=ev.hess_host(X, U, lamF, lamC, sigma))
    if kind == "lagr_grad_host":
        return dict(G=ev.lagr_grad_host(rng.standard_normal((B, nvals, M)), lamF, lamC, sigma))
    if kind == "lagr_grad_total_host":
        return dict(zip(("G", "Gdel"), ev.lagr_grad_total_host(rng.standard_normal((B, nvals, M)), lamF, lamC, sigma)))
    if kind in ("certificate_host", "certificate_total_host"):
        total = kind == "certificate_total_host"
        Uc = U if total else np.concatenate([U, rng.uniform(-0.5, 0.5, (B, nd, M))], axis=1)
        zl, zu = _bounds(rng, np.concatenate([X, Uc], axis=1), B if st.seed % 2 else 1)
        cl, cu = _row_bounds(npth)
        fn = ev.kkt_certificate_total_host if total else ev.kkt_certificate_host
        return dict(zip(("cert", "G", "Gdel"), fn(X, Uc, lamF, lamC, zl, zu, cl, cu, sigma)))
    if kind in ("ode_error_host", "ode_error_total_host"):
        ul, uu = U.min(axis=(0, 2)) + 0.1, U.max(axis=(0, 2)) - 0.1
        fn = ev.ode_error if kind == "ode_error_host" else ev.ode_error_total
        return dict(zip(("err", "eta"), fn(X, U, ul, uu, dev=False)))
    if kind == "blocks_host":
        H, V, Sg, St, fx = _blocks_inputs(rng, lay)
        return ev.kkt_blocks_host(H, V, Sg, St if npth else None, fx, 1e-4 if npth else 0.0)
    if kind == "ipm_host":
        return run_ipm(ev, cfg, st, dev=False)
    if kind == "factor_solve_host":         # emi_kkt_factor, emi_kkt_lowrank, emi_kkt_solve: instance 0 through the context's own workspace
        Q, V, fx = _newton_inputs(ev, rng, lay)
        info = ev.kkt_factor(Q[0], V[0, :ns * nv], fx[0].reshape(-1), DC)
        rhs = rng.standard_normal((2, (nv + ns) * M))
        plain = ev.kkt_solve(rhs)
        r = 2
        node, vec, delta = np.array([M // 3, M - 1], dtype=np.int32), 0.3 * rng.standard_normal((r, nv)), np.array([0.5, 0.25])
        exact = ev.kkt_lowrank(node, vec, delta)
        return dict(info=np.array([info]), x=plain, exact=np.array([exact]), x_lowrank=ev.kkt_solve(rhs))
    if kind == "start_guess_host":
        xa, xb = (np.ascontiguousarray(a, dtype=np.float64) for a in point(cfg, rng, B, ns, ncf, 2)[0].transpose(2, 0, 1))
        return dict(zip(("X", "level"), ev.start_guess((E.START_LINE, E.START_BEND, E.START_PLANNED)[st.seed % 3], xa, xb, bend=0.7, grid=17,
                                                       repair=st.seed % 2, dev=False)))
    raise KeyError(kind)


class Lived:
    """the lived context with what belongs to it between the steps: the mirror, and the result buffers its repeat passes go into"""

    def __init__(self, f32=False):
        import etol_amd as E
        self.cfg = Config(f32=f32)
        self.ev = E.Evaluator(0, f32=f32)
        self.state = {}             # what its calls leave for later ones (run_one)

    def close(self):
        self.state = {}
        self.ev.close()


def run_repeat(ev, cfg, st, kept):
    """A Jacobian pass into the VALS tensor of this Evaluator's previous one, which torch has not touched since: the Evaluator adds
    EMI_EVAL_KEEP_INVARIANT by itself, and the library honours it only while mesh, model, batch and tables are what they were.  With
    no such tensor of this shape (always so on a fresh context) a full pass at another point comes first.  Returns (results, kept)."""
    import torch
    lay = ev.layout
    shapes = ((lay.B, lay.nres, lay.M), (lay.B, lay.nvals, lay.M), (lay.B,))
    rng = np.random.default_rng(st.seed)
    ncf = lay.nc - ev.n_delayed
    first, second = point(cfg, rng, lay.B, lay.ns, ncf, lay.M), point(cfg, rng, lay.B, lay.ns, ncf, lay.M)
    up = lambda a: torch.from_numpy(a).to(ev.device)
    flagged = kept is not None and tuple(tuple(t.shape) for t in kept[1]) == shapes and kept[1][1] is ev._kept and kept[1][1]._version == ev._kept_version
    if not flagged:         # (another Jacobian pass went elsewhere since, or the shapes changed)
        c = Call(ev, "eval_repeat")
        outs = [c.out(n, s) for n, s in zip(("RES", "VALS", "COST"), shapes)]
        dX, dU = up(first[0]), up(first[1])
        torch.cuda.synchronize()
        ev.eval_dev(dX, dU, *outs)
        ev.synchronize()
        kept = (c, outs)
    c, outs = kept
    outs[0].fill_(NAN)
    outs[2].fill_(NAN)
    dX, dU = up(second[0]), up(second[1])
    torch.cuda.synchronize()
    assert outs[1] is ev._kept and outs[1]._version == ev._kept_version, "the repeat pass is not one the Evaluator flags"
    c.flagged_across_steps = flagged
    ev.eval_dev(dX, dU, *outs)
    ev.synchronize()
    torch.cuda.synchronize()
    c.check_slack()
    return c.results(), kept


def run_flagged(ev, cfg, st, state):
    """A pass with EMI_EVAL_KEEP_INVARIANT given by the CALLER, into a view at the start of one arena the context's earlier passes of this
    kind went into: the same address under whatever layout is in force now.  The library may leave the invariant rows alone only if
    nothing that enters them or moves them has changed since it filled that very buffer; on a fresh context (a new arena full of NaN)
    it has to write every row.  The arena has no poisoned slack (what lies behind the view is an earlier layout's rows)."""
    import torch
    import etol_amd as E
    lay = ev.layout
    n = lay.B * lay.nvals * lay.M
    arena = state.get("arena")
    if arena is None or arena.numel() < n:
        arena = state["arena"] = torch.full((max(n, 1 << 20),), NAN, dtype=ev.dtype, device=ev.device)
    c = Call(ev, "eval_flagged")
    X, U = point(cfg, np.random.default_rng(st.seed), lay.B, lay.ns, lay.nc - ev.n_delayed, lay.M)
    dX, dU = c.put("X", X), c.put("U", U)
    RES, COST = c.out("RES", (lay.B, lay.nres, lay.M)), c.out("COST", (lay.B,))
    c.outputs["VALS"] = arena[:n].view(lay.B, lay.nvals, lay.M)
    c.invoke = lambda: ev.eval_dev(dX, dU, RES, c.outputs["VALS"], COST, flags=E.EVAL_ALL | E.EVAL_KEEP_INVARIANT)
    return run_call(c)


def run_tracks_from_waypoints(ev, cfg, st, mirror):
    """centres of the tracks on the present mesh from the tables, then read back; a setter too (mirror: the Config to update)"""
    import torch
    sets = cfg.waypoints[0].shape[0]
    m = st.arg("map")
    if mirror is not None:
        mirror.wp_map, mirror.tracks = ("all" if m is None else list(m)), None
    torch.cuda.synchronize()
    ev.tracks_from_waypoints(None if m is None else torch.tensor(list(m), dtype=torch.int32, device=ev.device))
    ev.synchronize()
    xc, yc = ev.get_tracks()
    assert xc.shape[0] == (sets if m is None else len(m))
    return dict(xc=xc, yc=yc)


def same_bits(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in sorted(got):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            diff = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)) // a.dtype.itemsize
            i = np.unravel_index(int(diff[0]), a.shape) if a.ndim else ()
            raise AssertionError(f"{what}: {k} differs from the fresh context's in {len(np.unique(diff))} of {a.size} elements, first at {i}: "
                                 f"{a[i]!r} against {b[i]!r}")


def run_one(ev, cfg, st, state=None, mirror=None):
    """one calling step on one context -> (results, point of an evaluation or None); state: dict of what the context's earlier steps
    left for its later ones (the tensors of the repeat pass, the arena of the flagged one), None: a context without a past"""
    state = {} if state is None else state
    if st.kind == "eval_repeat":
        res, state["kept"] = run_repeat(ev, cfg, st, state.get("kept"))
        return res, None
    if st.kind == "eval_flagged":
        return run_flagged(ev, cfg, st, state), None
    if st.kind == "tracks_from_waypoints":
        return run_tracks_from_waypoints(ev, cfg, st, mirror), None
    if st.kind == "ipm":
        return run_ipm(ev, cfg, st, dev=True), None
    if st.kind in HOST_CALLS:
        res = run_host(ev, cfg, st)
        return res, res.pop("point", None)
    c = make_call(ev, cfg, st)
    return run_call(c), getattr(c, "point", None)


def walk(steps, f32=False, compare=True, log=None):
    """Walk a new context through `steps`; after every calling step the same call on fresh(config), every output bit for bit.  Returns
    dict: ev (the lived context, open), cfg, last (the last evaluation: cfg, X, U, (RES, VALS, COST)), ksliced, uploads.  A failure names
    the steps walked so far."""
    lv = Lived(f32=f32)
    done = []
    out = dict(last=None, ksliced=[], plans=0, uploads=[], plan_list=[])
    try:
        for st in steps:
            done.append(st)
            if st.kind in SETTERS:
                SETTERS[st.kind](lv.ev, lv.cfg, st)
                continue
            if st.kind == "bundle":         # several calls that share ONE fresh context (run-time compiled models: few compilations)
                subs = [Step(k, (), st.seed * 100 + q) for q, k in enumerate(st.arg("calls"))]
                got = []
                for sub in subs:
                    r, pt = run_one(lv.ev, lv.cfg, sub, lv.state)
                    got.append(r)
                    if sub.kind == "eval_all":
                        out["last"] = (copy.deepcopy(lv.cfg), pt[0], pt[1], (r["RES"], r["VALS"], r["COST"]))
                if compare:
                    fr, fstate = fresh(lv.cfg), {}
                    try:
                        for sub, r in zip(subs, got):
                            want, _ = run_one(fr, lv.cfg, sub, fstate)
                            same_bits(r, want, f"{st}: {sub}")
                    finally:
                        fstate.clear()
                        fr.close()
                continue
            got, pt = run_one(lv.ev, lv.cfg, st, lv.state, mirror=lv.cfg)
            kernel, plan = lv.ev.last_defect_kernel, lv.ev.plan()
            out["uploads"].append((len(done) - 1, lv.ev.pass_work_uploads))
            if st.kind.startswith("eval") and "K slices" in kernel and "emi_pass_f64_kernel" in kernel:
                out["ksliced"].append((len(done) - 1, st.seed))
            if pt is not None and st.kind in ("eval_all", "eval_host"):
                out["last"] = (copy.deepcopy(lv.cfg), pt[0], pt[1], (got["RES"], got["VALS"], got["COST"]))
            if not compare:
                continue
            fr = fresh(lv.cfg)
            try:
                want, _ = run_one(fr, lv.cfg, st)
                if st.kind.startswith("eval"):
                    assert fr.last_defect_kernel == kernel, (kernel, fr.last_defect_kernel)
                fplan = fr.plan()
                if st.kind.startswith("eval") and plan["one_launch"] and fplan["one_launch"]:
                    assert plan == fplan, (plan, fplan)
                    out["plans"] += 1
                    out["plan_list"].append(plan)
            finally:
                fr.close()
            same_bits(got, want, str(st))
    except BaseException as e:
        lv.close()
        trail = "\n".join(f"  {i:3d} {s}" for i, s in enumerate(done))
        if isinstance(e, AssertionError):
            raise AssertionError(f"{e}\nsteps up to the failing one:\n{trail}") from e
        print(f"steps up to the failing one:\n{trail}")
        raise
    out.update(ev=lv.ev, cfg=lv.cfg, lived=lv)
    return out


# ---- the lives ---------------------------------------------------------------------------------------------------------------------
class _Seeds:
    """seeds that never repeat: life number * 10000 + the step's count"""

    def __init__(self, life):
        self.base, self.n = 10000 * life, 0

    def __call__(self):
        self.n += 1
        return self.base + self.n


def _opt(name, value):
    return S("option", name=name, value=value)


RUNG_CALLS = ("eval_all", "eval_repeat", "hess", "lagr_grad", "certificate", "ode_error", "blocks", "shard", "factor_solve", "kkt_solve", "shard_solve",
              "factor_solve_host", "prolong_rows", "shard_move", "start_guess")


def life_ladder():
    """operators d_D / d_De / d_Do / d_Dfrag with has_dfrag (33 and 65: no symmetric halves in use, 128 and 256: fragments), the
    adj / ode dirty flags per rung, the Newton workspaces by shape, one work table per rung, the keep record across set_mesh and across
    a set_path of the same shape"""
    s = _Seeds(1)
    steps = [S("mesh", M=33, t0=0.0, tf=16.0), S("model", model=QUAD), S("batch", B=17), S("path", np=3, per_instance=True, table=11)]
    for i, (M, tf) in enumerate(((33, 16.0), (65, 16.0), (128, 16.0), (256, 16.0), (128, 9.0), (33, 16.0))):
        if i:
            steps.append(S("mesh", M=M, t0=0.0, tf=tf))
        steps += [S(k, s()) for k in RUNG_CALLS]
        if M == 128:
            steps += [S("path", np=3, per_instance=True, table=12 + i), S("eval_repeat", s())]      # same shape, other records
            # the caller's own flag on one buffer while the table loses and regains a row: the rows behind the path entries move
            steps += [S("eval_flagged", s()), S("eval_flagged", s()), S("path", np=2, per_instance=True, table=12 + i), S("eval_flagged", s()),
                      S("path", np=3, per_instance=True, table=12 + i), S("eval_flagged", s())]
    steps += [S("ode_error_total", s()), S("eval_all", s())]
    return steps


BATCHES = (17, 5, 3, 80, 704, 17, 33, 1, 160, 48, 17)


def life_batch():
    """more than eight work-table keys and back to the first (LRU eviction and re-upload), d_slab / d_tile_ticket / d_ticket and
    d_cost_part growing after they shrank, sym_combine, sym_ksplit, overlap_mode and node_store switched in between"""
    s = _Seeds(2)
    steps = [S("mesh", M=128, t0=0.0, tf=16.0), S("model", model=QUAD), S("batch", B=17), S("path", np=20, per_instance=True, table=21),
             _opt("overlap_mode", 3)]
    between = {1: [_opt("sym_combine", 0)], 2: [_opt("sym_combine", 1), _opt("sym_ksplit", 2)], 3: [_opt("sym_ksplit", 0), _opt("overlap_mode", 1)],
               4: [_opt("overlap_mode", 2), _opt("node_store", 1)], 5: [_opt("overlap_mode", 3), _opt("node_store", -1)],
               6: [_opt("node_store", 2)], 7: [_opt("node_store", -1), _opt("overlap_mode", 0)], 8: [_opt("overlap_mode", 3)],
               9: [_opt("sym_ksplit", 4)], 10: [_opt("sym_ksplit", 0)]}
    for i, B in enumerate(BATCHES):
        if i:
            steps.append(S("batch", B=B, table=21))
        steps += between.get(i, [])
        steps += [S("eval_all", s()), S("eval_all", s())]           # two passes of one plan at different points, back to back
        if B <= 80:
            steps += [S("eval_nojac", s()), S("eval_split", s())]
        if i in (6, 8, 9):          # three more block orders each: with these the first key's table has given way before the end
            for order in (0, 1, 150):
                steps += [_opt("pass_order", order), S("eval_all", s())]
            steps.append(_opt("pass_order", -1))
    steps.append(S("eval_all", s()))
    return steps


# the forced forms in turn: (options set for the form, options reset after it)
FORMS = ((("sym_bk", 16),), ()), ((("sym_dop", 2),), ()), ((("sym_res", 3),), ("sym_res", "sym_dop", "sym_bk")), ((("sym_hs", 2),), ("sym_hs",)),
FORMS += ((("sym_ctc", 2),), ("sym_ctc",)), ((("sym_nst", 4),), ("sym_nst",)), ((("pass_order", 0),), ()), ((("pass_order", 1),), ()),
FORMS += ((("pass_order", 150),), ("pass_order",)),


def life_forms():
    """every forced form of the one-launch pass in turn on one context (work tables by plan, the operator copies each form reads: the
    16-deep K tiles, De / Do from L2 and three resident workgroups build on one another, the others stand alone), then every option
    back at its default: the last result is the default plan's"""
    s = _Seeds(3)
    steps = [S("mesh", M=256, t0=0.0, tf=16.0), S("model", model=QUAD), S("batch", B=33), S("path", np=20, per_instance=True, table=31),
             _opt("overlap_mode", 3), _opt("sym_ct", 6), _opt("sym_ksplit", 1)]
    for sets, resets in FORMS:
        steps += [_opt(name, value) for name, value in sets]
        steps += [S("eval_all", s()), S("eval_repeat", s()), S("eval_repeat", s())]
        steps += [_opt(name, OPTION_DEFAULTS[name]) for name in resets]
    for name in ("sym_ct", "sym_ksplit", "overlap_mode"):
        steps.append(_opt(name, OPTION_DEFAULTS[name]))
    steps.append(S("eval_all", s()))
    return steps


def life_models():
    """rtc, pvars, blk_key / ipm_key (lists rebuilt per layout), d_W / d_uext / the delay dirty flags, the keep record and
    path_has_track across changes of the model"""
    s = _Seeds(4)
    three = lambda: [S("eval_all", s()), S("blocks", s()), S("ipm", s())]
    steps = [S("mesh", M=65, t0=0.0, tf=16.0), S("model", model=QUAD), S("batch", B=5), S("path", np=3, per_instance=True, table=41)] + three()
    steps += [S("model", model=POINTMASS), S("waypoints", n=2, sets=1, table=42), S("tracks_from_waypoints", s()),
              S("path", np=2, tracks=2, table=43), S("repair_guess", s())] + three()
    steps += [S("tracks", n=2, table=47), S("eval_all", s()), S("repair_guess", s())]        # centres given, in place of the tables'
    steps += [S("model", source="traced_rows"), S("path", np=1, table=44), S("rows", ns=6, nv=8, np=3),
              S("bundle", s(), calls=("eval_all", "blocks", "ipm", "hess", "lagr_grad"))]
    steps += [S("model", source="delayed"), S("delays", xh=3, uh=1, dt=0.25), S("path", np=1, table=45), S("rows", ns=2, nv=10, np=1),
              S("bundle", s(), calls=("eval_all", "eval_repeat", "blocks", "lagr_grad_total", "certificate_total", "ode_error_total")),
              S("mesh", M=128, t0=0.0, tf=16.0),
              S("bundle", s(), calls=("eval_all", "eval_repeat", "blocks", "lagr_grad_total", "ode_error_total")),
              S("delays", xh=0, uh=0, dt=0.25), S("bundle", s(), calls=("eval_all", "hess"))]
    steps += [S("model", model=QUAD), S("path", np=3, per_instance=True, table=46), S("rows", ns=6, nv=8, np=3)] + three()
    steps += [S("eval_repeat", s()), S("eval_all", s())]
    return steps


def life_staging():
    """the named staging buffers s_X .. s_Gdel and the slots of host_stage while the batch grows and shrinks; a flagged pass right after
    a host evaluation (s_VALS is the buffer the keep record tracks), a certificate host form between two eval_host calls"""
    s = _Seeds(5)
    steps = [S("mesh", M=65, t0=0.0, tf=16.0), S("model", model=QUAD), S("batch", B=3), S("path", np=3, per_instance=True, table=51)]
    for i, B in enumerate((3, 17, 5, 33, 2)):
        if i:
            steps.append(S("batch", B=B, table=51))
        steps += [S("eval_host", s()), S("eval_repeat", s()), S("certificate_host", s()), S("eval_host", s()), S("eval_all", s()),
                  S(("hess_host", "blocks_host", "lagr_grad_host", "ipm_host", "ode_error_host")[i], s()),
                  S(("hess", "blocks", "lagr_grad", "ipm", "ode_error")[i], s()), S("factor_solve_host", s()),
                  S(("start_guess_host", "lagr_grad_total_host", "certificate_total_host", "ode_error_total_host", "start_guess_host")[i], s())]
    steps.append(S("eval_host", s()))
    return steps


def life_f32():
    """the fp32 context: ring, register-staged and fallback defect kernels, the one-launch pass, the flagged pass; d_cost_part2 and
    the operator copies in fp32 across 128 -> 512 -> 128 nodes"""
    s = _Seeds(6)
    steps = [S("mesh", M=128, t0=0.0, tf=20.0), S("model", model=FIXEDWING), S("batch", B=16)]
    for i, M in enumerate((128, 512, 128)):
        if i:
            steps.append(S("mesh", M=M, t0=0.0, tf=20.0))
        steps += [S("eval_all", s()), S("eval_repeat", s()), _opt("f32_ring", 0), S("eval_all", s()), _opt("f32_one_launch", 1), S("eval_all", s()),
                  S("eval_repeat", s()), _opt("overlap_mode", 2), S("eval_all", s()), _opt("overlap", 0), S("eval_all", s()), S("eval_nojac", s()),
                  _opt("overlap", 1), _opt("overlap_mode", 0), _opt("f32_one_launch", 0), _opt("f32_ring", 1), S("hess", s())]
    steps.append(S("eval_all", s()))
    return steps


def life_drivers():
    """IpmSolveWs / IpmLadderWs and the Newton workspaces the drivers leave behind: the nine-instance ladder (21, 41), an unrelated
    evaluation at 128 nodes, the same ladder again (run by test_gpu_context_life.test_drivers)"""
    s = _Seeds(7)
    return [S("ipm_solve_ladder", s()), S("mesh", M=128, t0=0.0, tf=16.0), S("eval_all", s()), S("ipm_solve_ladder", s()), S("eval_all", s())]


LIVES = dict(ladder=life_ladder, batch=life_batch, forms=life_forms, models=life_models, staging=life_staging, f32=life_f32, drivers=life_drivers)

# which members of emi_ctx_s a life is after
TARGETS = {
    "ladder": ("d_D", "d_De", "d_Do", "d_Dfrag", "has_dfrag", "adj_dirty", "ode_dirty", "kkt", "kkt_shard", "pass_work", "keep", "start_guess"),
    "batch": ("pass_work", "d_slab", "d_tile_ticket", "d_ticket", "d_cost_part"),
    "forms": ("pass_work", "d_De", "d_Do", "d_Dfrag", "keep"),
    "models": ("rtc", "pvars", "blk_key", "ipm_key", "d_W", "d_uext", "delay_dirty", "adjw_dirty", "odel_dirty", "keep", "path_has_track"),
    "staging": ("s_X", "s_VALS", "host_stage", "keep"),
    "f32": ("d_D", "d_cost_part2", "keep"),
    "drivers": ("ipm_solve", "ipm_ladder", "kkt_shard"),
}

WALK_CALLS = ("eval_all", "eval_nojac", "eval_split", "eval_repeat", "eval_flagged", "hess", "lagr_grad", "certificate", "lagr_grad_total", "ode_error",
              "ode_error_total", "blocks", "shard", "factor_solve", "ipm", "prolong_rows", "shard_move", "repair_guess", "start_guess",
              "eval_host", "hess_host", "certificate_host", "blocks_host", "factor_solve_host", "kkt_solve", "shard_solve")
WALK_OPTIONS = (("overlap_mode", (0, 1, 2, 3)), ("sym_combine", (0, 1)), ("node_store", (-1, 0, 1, 2)), ("sym_ksplit", (0, 2)), ("pass_order", (-1, 0, 1)))


def seeded_walk(seed, n=30):
    """thirty steps over the cheap part of the alphabet: built-in models, M in {33, 65, 128, 256}, B <= 80"""
    rng = np.random.default_rng(seed)
    s = _Seeds(100 + seed)
    M, B = int(rng.choice([33, 65, 128, 256])), int(rng.choice([3, 17, 33]))
    steps = [S("mesh", M=M, t0=0.0, tf=16.0), S("model", model=QUAD), S("batch", B=B), S("path", np=3, per_instance=True, table=int(rng.integers(100, 200)))]
    while len(steps) < n + 4:
        r = rng.random()
        if r < 0.10:
            M = int(rng.choice([33, 65, 128, 256]))
            steps.append(S("mesh", M=M, t0=0.0, tf=float(rng.choice([9.0, 16.0]))))
        elif r < 0.20:
            B = int(rng.choice([1, 3, 5, 17, 33, 48, 80]))
            steps.append(S("batch", B=B, table=int(rng.integers(100, 200))))
        elif r < 0.25:
            model = int(rng.choice([QUAD, POINTMASS]))
            steps += [S("model", model=model), S("path", np=int(rng.choice([1, 3])), per_instance=bool(rng.integers(2)), table=int(rng.integers(100, 200)))]
        elif r < 0.30:
            steps.append(S("path", np=int(rng.choice([1, 3, 20])), per_instance=bool(rng.integers(2)), table=int(rng.integers(100, 200))))
        elif r < 0.40:
            name, values = WALK_OPTIONS[int(rng.integers(len(WALK_OPTIONS)))]
            steps.append(_opt(name, int(rng.choice(values))))
        else:
            kind = str(rng.choice(WALK_CALLS))
            if kind == "shard_solve" and B * M > 17 * 256:
                kind = "kkt_solve"
            if kind == "shard" and B * M > 17 * 256:        # (a factorisation per instance: kept to the sizes of the ladder life)
                kind = "blocks"
            steps.append(S(kind, s()))
    return steps[:n + 4]


def calling_steps(steps):
    """(kind, seed) of every call of a life, the calls of a bundle one by one (they share the bundle's seed base)"""
    out = []
    for st in steps:
        if st.kind == "bundle":
            out += [(k, st.seed * 100 + q) for q, k in enumerate(st.arg("calls"))]
        elif st.kind not in SETTERS:
            out.append((st.kind, st.seed))
    return out
