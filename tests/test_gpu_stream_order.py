"""Calls on the caller's stream are ordered on it: emi_set_stream (Evaluator.use_stream) with a torch.cuda.Stream.  -m gpu

Every other GPU test brackets a call with a device-wide synchronisation and runs the context on its own stream, so a launch that went to
the context's second stream, to a Newton workspace's rocBLAS handle or to the ladder's stream without waiting for the context's stream, or
that was not joined back before the outputs may be consumed, would be invisible there.  Here the device is NOT synchronised between:

  1. the input buffers of the call hold NaN, the outputs NaN (both synchronised);
  2. on the caller's stream s: a delay, then device-to-device copies of the real inputs into the input buffers, then an event;
  3. the call;
  4. directly after it returns the event must still be pending -- the inputs were not valid yet when the call was issued, so a run that
     cannot tell fails instead of passing vacuously (entry points that return host values synchronise by contract: no assertion there);
  5. on s: every output is cloned, then the inputs are filled with NaN again;
  6. after s.synchronize() the clones have the bits of the same call on the same context in the suite's usual manner (own stream,
     synchronised before and after).

Step 2 is deterministic: work that does not wait for s reads NaN.  Step 5 is only probabilistic: a kernel that was not joined back, or
that reads its inputs late, shows only if the clone or the NaN fill happens to overtake it.

Entry points that synchronise by contract -- those that return host values, the _host forms, the drivers -- run on the caller's stream
too, behind the same delay and with steps 5 and 6; only the assertion of step 4 is left out.

The delay is DELAY_MS on the device (torch.cuda._sleep, calibrated once; a chain of matrix products where that does not wait), at least
ten times the slowest host-side duration of an asynchronous call of the list and below 100 ms.  The last test of the file asserts that
over HOST_MS, which the tests before it fill in file order: run alone, it measures one emi_eval_dev call and checks the figure for that."""
import ctypes as C
import time

import numpy as np
import pytest

import context_life as CL
from context_life import S

pytestmark = pytest.mark.gpu

DELAY_MS = 20.0
HOST_MS = {}            # case -> host-side duration of its asynchronous call


@pytest.fixture(scope="module")
def delay(built):
    """delay(stream): enqueue DELAY_MS of waiting on the current stream"""
    import torch

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    probe = 20_000_000
    torch.cuda._sleep(1000)
    ms = timed(lambda: torch.cuda._sleep(probe))
    if ms > 1.0:
        cycles = int(probe * DELAY_MS / ms)
        wait = lambda: torch.cuda._sleep(cycles)
    else:                   # _sleep does not wait here: large products instead
        a = torch.randn(4096, 4096, device="cuda")
        timed(lambda: a @ a)
        n = max(1, int(np.ceil(DELAY_MS / timed(lambda: a @ a))))

        def wait():
            b = a
            for _ in range(n):
                b = a @ b
    got = timed(wait)
    assert DELAY_MS * 0.8 <= got < 100.0, got
    return wait


def config(model=CL.QUAD, M=128, B=17, npth=3, f32=False, source=None, delays=None, rows=None, tf=16.0, **options):
    cfg = CL.Config(f32=f32)
    steps = [S("mesh", M=M, t0=0.0, tf=tf), S("model", model=model, source=source)]
    if delays:
        steps.append(S("delays", xh=delays[0], uh=delays[1], dt=delays[2]))
    steps.append(S("batch", B=B))
    if npth:
        steps.append(S("path", np=npth, per_instance=True, table=91))
    if rows:
        steps.append(S("rows", ns=rows[0], nv=rows[1], np=rows[2]))
    steps += [S("option", name=k, value=v) for k, v in options.items()]
    for st in steps:
        CL.SETTERS[st.kind](None, cfg, st)
    return cfg


def on_stream(c, s, delay, case):
    """steps 1 - 6 of the module's docstring for one Call; returns its results"""
    import torch
    real = {k: t.clone() for k, t in c.inputs.items() if t.is_floating_point()}
    for k in real:
        c.inputs[k].fill_(CL.NAN)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay()
        for k, r in real.items():
            c.inputs[k].copy_(r)
        valid = torch.cuda.Event()
        valid.record(s)
        t0 = time.perf_counter()
        c.invoke()
        host_ms = 1e3 * (time.perf_counter() - t0)
        pending = not valid.query()
        clones = {k: v.clone() for k, v in c.outputs.items()}
        for k in real:
            c.inputs[k].fill_(CL.NAN)
    s.synchronize()
    if not c.synchronising:
        assert pending, f"{case}: the inputs were already valid when the call returned (after {host_ms:.3f} ms on the host): the run cannot tell"
        HOST_MS[case] = host_ms
    c.check_slack()
    out = {k: v.cpu().numpy() for k, v in clones.items()}
    out.update({k: np.asarray(v) for k, v in c.host.items()})
    return out


def ordered(cfg, kind, seed, delay, case):
    """warm-up at another point in the usual manner, the call on a caller's stream, the same call in the usual manner: the same bits.
    (The warm-up's seed is 6 on: calls that take their variant from the seed modulo 2 or 3 warm up the variant that is tested.)"""
    import torch
    ev = CL.fresh(cfg)
    s = torch.cuda.Stream()
    try:
        CL.run_call(CL.make_call(ev, cfg, S(kind, seed + 6)))
        ev.use_stream(s.cuda_stream)
        got = on_stream(CL.make_call(ev, cfg, S(kind, seed)), s, delay, case)
        ev.use_stream(0)
        want = CL.run_call(CL.make_call(ev, cfg, S(kind, seed)))
        CL.same_bits(got, want, case)
        assert not any(np.isnan(v).any() for k, v in want.items() if v.dtype.kind == "f" and k in ("RES", "COST", "G", "H", "cert", "err", "Vf"))
    finally:
        ev.close()


@pytest.mark.parametrize("B", [17, 80])
@pytest.mark.parametrize("mode", [1, 2, 3, 0])
def test_eval_dev(built, delay, mode, B):
    ordered(config(B=B, overlap_mode=mode), "eval_all", 500 + 10 * mode + B, delay, f"eval_dev mode {mode} B {B}")


@pytest.mark.parametrize("kind", ["eval_nojac", "eval_split"])
def test_eval_dev_flags(built, delay, kind):
    ordered(config(B=17), kind, 540, delay, kind)


def test_eval_dev_f32_two_streams(built, delay):
    cfg = config(model=CL.FIXEDWING, M=128, B=16, npth=0, f32=True, tf=20.0, overlap_mode=2)
    ordered(cfg, "eval_all", 550, delay, "eval_dev f32, two streams")


def test_eval_dev_delayed_model(built, delay):
    cfg = config(model=None, source="delayed", delays=(3, 1, 0.25), M=128, B=20, npth=1)
    ordered(cfg, "eval_all", 560, delay, "eval_dev, delayed model")


# (name, configuration, call): the adjoint calls once at a batch that the library runs back to back and once where the operator product
# goes to the context's second stream beside the node kernel (emi_adjoint.hip, adjoint_side_by_side: ceil(6 B / 96) ceil(M / 128) >= 256)
BIG = dict(M=256, B=2048, npth=0)
CALLS = [
    ("hess_dev", dict(), "hess"),
    ("lagr_grad_dev", dict(), "lagr_grad"),
    ("kkt_certificate_dev", dict(), "certificate"),
    ("lagr_grad_total_dev", dict(), "lagr_grad_total"),
    ("kkt_certificate_total_dev", dict(), "certificate_total"),
    ("lagr_grad_dev, second stream", BIG, "lagr_grad"),
    ("kkt_certificate_dev, second stream", BIG, "certificate"),
    ("lagr_grad_total_dev, second stream", BIG, "lagr_grad_total"),
    ("kkt_certificate_total_dev, second stream", BIG, "certificate_total"),
    ("kkt_blocks_dev", dict(), "blocks"),
    ("kkt_factor_dev + kkt_solve_dev", dict(M=65, B=1), "factor_solve"),
    ("kkt_solve_dev", dict(M=65, B=1), "kkt_solve"),
    ("the shard calls", dict(M=65, B=5), "shard"),
    ("kkt_solve_shard_dev", dict(M=65, B=5), "shard_solve"),
    ("prolong_rows", dict(), "prolong_rows"),
    ("shard_move", dict(), "shard_move"),
    ("repair_guess", dict(), "repair_guess"),
    ("ode_error", dict(), "ode_error"),
    ("ode_error_total", dict(), "ode_error_total"),
    ("start_guess", dict(M=65), "start_guess"),
]


@pytest.mark.parametrize("name,shape,kind", CALLS, ids=[c[0] for c in CALLS])
def test_call(built, delay, name, shape, kind):
    ordered(config(**shape), kind, 600 + 7 * [c[0] for c in CALLS].index(name), delay, name)


def test_the_second_stream_cases_are_at_a_shape_that_forks(built):
    """... by the library's own condition, which context_life.adjoint_forks restates (held to the source by test_context_life_cpu.py)"""
    assert CL.adjoint_forks(BIG["B"], 6, BIG["M"]) and not CL.adjoint_forks(17, 6, 128)


def test_ipm_dev_kernels(built, delay):
    """reduce, expand, trial, merit, accept, error: steps 1 - 6 per kernel.  Every method of the backend uploads its own arrays, so after
    a kernel ALL of them -- inputs, outputs, and what accept and merit update in place -- are cloned on s and then filled with NaN on s;
    the results are read from the clones."""
    import torch
    import test_gpu_ipm as TI
    cfg = config(M=65, B=5)
    ev = CL.fresh(cfg)
    s = torch.cuda.Stream()

    class OnStream(TI.DevBackend):
        def __init__(self, ev):
            super().__init__(ev, dev=True)
            self.mine, self.clones = [], {}

        def down(self, t, shape=None):
            if t is not None and id(t) in self.clones:
                return self.clones[id(t)][1].cpu().numpy()
            return super().down(t, shape)

        def up(self, a):
            t = super().up(a)
            if t is not None and t.is_floating_point():
                self.mine.append(t)
            return t

        def run(self, name, *args, **kw):
            real = [(t, t.clone()) for t in self.mine]
            self.mine = []
            for t, _ in real:
                t.fill_(CL.NAN)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                delay()
                for t, r in real:
                    t.copy_(r)
                valid = torch.cuda.Event()
                valid.record(s)
                t0 = time.perf_counter()
                getattr(self.ev, "ipm_" + name)(*args, dev=True, **kw)
                HOST_MS["ipm_" + name] = 1e3 * (time.perf_counter() - t0)
                assert not valid.query(), f"ipm_{name}: the inputs were already valid when the call returned"
                for t, _ in real:
                    self.clones[id(t)] = (t, t.clone())         # (the tensor is held: its id stays its own)
                for t, _ in real:
                    t.fill_(CL.NAN)
            s.synchronize()

    try:
        case = CL.ipm_case(ev, cfg, S("ipm", 700))
        TI.all_outputs(CL.ipm_case(ev, cfg, S("ipm", 701)), TI.DevBackend(ev))
        ev.use_stream(s.cuda_stream)
        got = TI.all_outputs(case, OnStream(ev))[0]
        ev.use_stream(0)
        want = TI.all_outputs(case, TI.DevBackend(ev))[0]
        CL.same_bits(got, want, "ipm kernels")
    finally:
        ev.close()


@pytest.mark.parametrize("kind", ["eval_host", "certificate_host", "factor_solve_host"])
def test_host_form_on_the_callers_stream(built, delay, kind):
    """a _host form (synchronises by contract) behind the delay on the caller's stream: its staging copies and launches go to that
    stream; the bits of the usual run"""
    import torch
    cfg = config(M=65, B=5)
    ev = CL.fresh(cfg)
    s = torch.cuda.Stream()
    try:
        CL.run_host(ev, cfg, S(kind, 1006))
        ev.use_stream(s.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay()
            got = CL.run_host(ev, cfg, S(kind, 1000))
            busy = torch.full((1 << 20,), CL.NAN, device=ev.device)       # work of the caller's right behind it
        s.synchronize()
        ev.use_stream(0)
        want = CL.run_host(ev, cfg, S(kind, 1000))
        for d in (got, want):
            d.pop("point", None)
        CL.same_bits(got, want, kind)
        assert busy.isnan().all()
    finally:
        ev.close()


def test_ladder_driver_on_the_callers_stream(built, delay):
    """emi_ipm_solve_ladder_dev (synchronises by contract) with the context on a caller's stream: starts and bounds become valid on that
    stream only behind the delay, the results are cloned and the inputs overwritten on it right after; statuses, iteration counts,
    trajectories and multipliers are those of the same solve in the usual manner"""
    import torch
    import ladder_ref as LD
    import lockstep_ref as LR
    import test_gpu_ladder as TLad
    import test_gpu_lockstep as TL
    tf = LR.TFS[0]
    insts = LD.instances(tf)
    ev = TLad.fresh_ev(tf, insts)
    s = torch.cuda.Stream()
    try:
        want = TLad.climb(ev, tf, insts, LD.LADDER, dict(tol=TLad.TOL))
        ev.set_mesh(9, 0.0, 1.0)
        ev.use_stream(s.cuda_stream)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(ev.device)
        z0 = np.stack([i["z0"] for i in insts]).reshape(len(insts), TL.NV, LD.LADDER[0])
        X0, U0 = up(z0[:, :TL.NS]), up(z0[:, TL.NS:])
        rungs = [dict(M=M, bounds=TLad.bounds_at(tf, M, up), options=dict(tol=TLad.TOL), repair=0) for M in LD.LADDER]
        inputs = [X0, U0] + [r["bounds"][k] for r in rungs for k in ("zl", "zu")]
        real = [t.clone() for t in inputs]
        for t in inputs:
            t.fill_(CL.NAN)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay()
            for t, r in zip(inputs, real):
                t.copy_(r)
            X, U, LamF, LamC, res = ev.ipm_solve_ladder(rungs, 0.0, tf, X0, U0, dev=True)
            clones = [t.clone() for t in (X, U, LamF, LamC)]
            for t in inputs:
                t.fill_(CL.NAN)
        s.synchronize()
        got = dict(zip(("X", "U", "LamF", "LamC"), (t.cpu().numpy() for t in clones)))
        assert TL.same_bits(got, want) and res == want["res"]
        assert all(q["status"] in (LR.CONVERGED, LR.ACCEPTABLE) for q in res[-1])
    finally:
        ev.close()


def test_tracks_from_waypoints(built, delay):
    """no array of the caller's but the set map: the centres are those of the usual manner, and the call does not wait for the stream"""
    import torch
    cfg = config(model=CL.POINTMASS, M=65, B=5, npth=0)
    CL.SETTERS["waypoints"](None, cfg, S("waypoints", n=2, sets=3, table=5))
    ev = CL.fresh(cfg)
    s = torch.cuda.Stream()
    try:
        m = torch.tensor([2, 0, 1, 1, 0], dtype=torch.int32, device=ev.device)
        ev.tracks_from_waypoints(m)
        ev.synchronize()
        want = ev.get_tracks()
        ev.set_mesh(cfg.M, cfg.t0, cfg.tf)              # drops the centres
        ev.use_stream(s.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay()
            valid = torch.cuda.Event()
            valid.record(s)
            ev.tracks_from_waypoints(m)
            assert not valid.query()
        got = ev.get_tracks()                           # (synchronises)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))
    finally:
        ev.close()


def test_comm_gather_of_one_rank(built, delay):
    import torch
    from etol_amd import _lib as L
    lib = L.load()
    ident = (C.c_char * 128)()
    assert lib.emi_comm_unique_id(ident) == 0, lib.emi_comm_last_error(None)
    comm = C.c_void_p()
    assert lib.emi_comm_create(0, 1, 0, ident, C.byref(comm)) == 0, lib.emi_comm_last_error(None)
    s = torch.cuda.Stream()
    try:
        real = torch.randn(1 << 16, dtype=torch.float64, device="cuda:0")
        src, dst = torch.full_like(real, CL.NAN), torch.full_like(real, CL.NAN)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay()
            src.copy_(real)
            valid = torch.cuda.Event()
            valid.record(s)
            assert lib.emi_comm_gather(comm, src.data_ptr(), dst.data_ptr(), src.numel() * 8, 0, C.c_void_p(s.cuda_stream)) == 0
            assert not valid.query()
            got = dst.clone()
            src.fill_(CL.NAN)
        s.synchronize()
        assert torch.equal(got, real)
    finally:
        assert lib.emi_comm_destroy(comm) == 0


def test_two_contexts_on_one_stream_called_alternately(built, delay):
    import torch
    cfgs = [config(B=17, overlap_mode=2), config(B=33, M=256, overlap_mode=3)]
    evs = [CL.fresh(c) for c in cfgs]
    s = torch.cuda.Stream()
    try:
        for ev, cfg in zip(evs, cfgs):
            CL.run_call(CL.make_call(ev, cfg, S("eval_all", 800)))
            ev.use_stream(s.cuda_stream)
        calls = [CL.make_call(evs[i % 2], cfgs[i % 2], S("eval_all", 801 + i)) for i in range(6)]
        reals = [{k: t.clone() for k, t in c.inputs.items()} for c in calls]
        for c in calls:
            for t in c.inputs.values():
                t.fill_(CL.NAN)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay()
            for c, real in zip(calls, reals):
                for k, r in real.items():
                    c.inputs[k].copy_(r)
            valid = torch.cuda.Event()
            valid.record(s)
            for c in calls:
                c.invoke()
            assert not valid.query()
            clones = [{k: v.clone() for k, v in c.outputs.items()} for c in calls]
            for c in calls:
                for t in c.inputs.values():
                    t.fill_(CL.NAN)
        s.synchronize()
        for ev in evs:
            ev.use_stream(0)
        for i, (c, got) in enumerate(zip(calls, clones)):
            c.check_slack()
            want = CL.run_call(CL.make_call(evs[i % 2], cfgs[i % 2], S("eval_all", 801 + i)))
            CL.same_bits({k: v.cpu().numpy() for k, v in got.items()}, want, f"call {i}")
    finally:
        for ev in evs:
            ev.close()


def test_moving_between_streams_keeps_the_cached_work_table(built, delay):
    """own stream -> a caller's -> another caller's -> own again, a pass on each: one table upload in all, the same bits throughout, and
    emi_get_stream answers what was set"""
    import torch
    cfg = config(B=17, overlap_mode=3)
    ev = CL.fresh(cfg)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def stream_of():
        p = C.c_void_p()
        assert ev.lib.emi_get_stream(ev.ctx, C.byref(p)) == 0
        return p.value or 0

    try:
        own = stream_of()
        assert own != 0
        want = CL.run_call(CL.make_call(ev, cfg, S("eval_all", 900)))
        assert ev.pass_work_uploads == (1, 1)
        for s in (s1, s2):
            ev.use_stream(s.cuda_stream)
            assert stream_of() == s.cuda_stream
            got = on_stream(CL.make_call(ev, cfg, S("eval_all", 900)), s, delay, "eval_dev after a move")
            CL.same_bits(got, want, "on a caller's stream")
            assert ev.pass_work_uploads == (1, 1)
        ev.use_stream(0)
        assert stream_of() not in (0, s1.cuda_stream, s2.cuda_stream)
        CL.same_bits(CL.run_call(CL.make_call(ev, cfg, S("eval_all", 900))), want, "back on its own stream")
        assert ev.pass_work_uploads == (1, 1)
    finally:
        ev.close()


def test_closing_a_context_leaves_the_callers_stream_alone(built, delay):
    import torch
    cfg = config(B=17)
    ev = CL.fresh(cfg)
    s = torch.cuda.Stream()
    ev.use_stream(s.cuda_stream)
    c = CL.make_call(ev, cfg, S("eval_all", 950))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        delay()
        c.invoke()
    ev.close()                                      # drains the stream, destroys only what the context made
    with torch.cuda.stream(s):
        a = torch.arange(1 << 20, dtype=torch.float64, device="cuda")
        b = (a * 2).sum()
    s.synchronize()
    assert b.item() == float((1 << 20) * ((1 << 20) - 1))
    assert not c.outputs["COST"].isnan().any()


def test_the_delay_is_ten_times_the_slowest_call(built, delay):
    if not HOST_MS:
        ordered(config(B=17), "eval_all", 990, delay, "eval_dev")
    worst = max(HOST_MS, key=HOST_MS.get)
    print(f"slowest host-side duration: {worst} {HOST_MS[worst]:.3f} ms; delay {DELAY_MS} ms")
    assert 10.0 * HOST_MS[worst] <= DELAY_MS < 100.0, (worst, HOST_MS[worst])
