"""The fp32 context (Evaluator(0, f32=True), BASELINE config 5) per defect kernel, launch form and model.  -m gpu

Kernel bodies: emi_defect_f32_ring_kernel, emi_defect_f32_mfma_kernel (register-staged), the atomic body inside
emi_pass_f32_kernel, and the f64-accumulating fallback emi_defect_f32_kernel.  Launch forms: sequential, two streams
("overlap_mode" 2) and one launch ("overlap_mode" 3).  Every case names the kernel it meant to run through last_defect_kernel.

References: numpy long double for the isolated product R0 + D.X (tests/f32_ref.py), oracle_lib.evaluate / oracle_lib.hessian for
whole passes -- never the f64 device context.  Every input goes through f32_ref.to_f32 before the device and the oracle get it.
Tolerances: the fallback's derived bound (f32_ref.fallback_bound, no margin); 2e-6 of the row scale for the MFMA forms, which
tests/test_f32_ref_cpu.py shows attainable by a sequential-f32 emulation on these very inputs (worst 7.8e-7); the project's 2e-6
class for node rows, VALS, COST and the Hessian (test_f32_context_fixedwing).  Figures measured on the device: DESIGN.md section 2."""
import functools

import numpy as np
import pytest

import f32_ref as F

pytestmark = pytest.mark.gpu

RING, STAGED, FALLBACK = "emi_defect_f32_ring_kernel", "emi_defect_f32_mfma_kernel", "emi_defect_f32_kernel"
ONE_LAUNCH = "emi_pass_f32_kernel"
# the MFMA kernel's variants: name -> (options, kernel name reported)
VARIANTS = {"ring": (dict(f32_ring=1, f32_ring_wgs=2), RING), "ring_wgs1": (dict(f32_ring=1, f32_ring_wgs=1), RING),
            "staged": (dict(f32_ring=0), STAGED)}
NAN_BITS = 0x7FC12345           # a quiet NaN with a payload nothing computes

_OPEN = []                      # every evaluator a test made


@pytest.fixture(autouse=True)
def close_evaluators():
    """a failed assertion ahead of ev.close() must not leave the context, its streams and its buffers to the rest of the session"""
    yield
    while _OPEN:
        _OPEN.pop().close()


def make_ev(model, params, M, B, t0=0.0, tf=F.W.TF, recs=None, tracks=None, maximize=False, **options):
    import etol_amd as E
    ev = E.Evaluator(0, f32=True)
    _OPEN.append(ev)
    ev.set_mesh(M, t0, tf, mesh=F.mesh(M))          # the oracle's mesh: both sides hold the same D
    ev.set_model(model, params, maximize=maximize)
    ev.set_batch(B)
    if tracks is not None:
        ev.set_tracks(*tracks)
    if recs is not None:
        ev.set_path(recs, 0, 1)
    for k, v in options.items():
        ev.set_option(k, v)
    assert ev.layout.real_bytes == 4 and not ev.uses_fused_kernel
    return ev


def case_ev(c, **options):
    return make_ev(c["model"], c["params"], c["M"], c["B"], c["t0"], c["tf"], c["recs"], c["tracks"], c["maximize"], **options)


def defect_only(model, B, M, X, U, R0, expect, **options):
    """R0 + D.X by the defect kernel alone (EVAL_DEFECT with res_in), on a fresh context"""
    import etol_amd as E
    ev = make_ev(model, F.PARAMS[model], M, B, **options)
    RES, _, _ = ev.eval_host(X, U, flags=E.EVAL_DEFECT, res_in=R0)
    name = ev.last_defect_kernel
    ev.close()
    assert name == expect, (name, expect, options)
    return RES


@functools.lru_cache(maxsize=None)
def defect_reference(M, R):
    model, B = F.ROWS[R]
    X, U, R0 = F.defect_case(model, B, M)
    D = F.mesh(M)[2]
    ref = F.exact_defect(D, X, R0)
    return model, B, X, U, R0, ref, F.row_scale(D, X, ref)


# ---- a. each defect kernel alone --------------------------------------------------------------------------------------------
# workgroups = ceil(R/64) * (M/128): below 8 | above 8, not a multiple | a multiple of 8; M = 128 and M = 384 with a ragged last
# row tile (R % 64 != 0); (256, .) and (512, .) are the ring tails 2 and 4 behind a main loop, 128 the tail 4 alone, 384 the tail 6
MFMA_SHAPES = [(128, 6), (128, 114), (128, 228),                 # 1, 2, 4 workgroups, all ragged; K loop never entered
               (256, 36), (256, 192), (256, 228),               # 2, 6, 8
               (384, 36), (384, 168), (384, 192), (384, 228),   # 3, 9 (ragged), 9 (full tiles), 12
               (512, 114), (512, 168), (512, 228)]              # 8, 12, 16


def test_the_mfma_shapes_cover_every_class_the_remap_and_the_tail_have():
    wgs = {(M, R): -(-R // 64) * (M // 128) for M, R in MFMA_SHAPES}
    assert any(w < 8 for w in wgs.values()) and any(w > 8 and w % 8 for w in wgs.values()) and any(w % 8 == 0 for w in wgs.values())
    for M in (128, 384):
        assert any(m == M and R % 64 for m, R in MFMA_SHAPES)
    assert {(M // 32 - 1) % 6 + 1 for M, _ in MFMA_SHAPES} == {4, 2, 6}         # tiles left to the ring's tail


@pytest.mark.parametrize("M,R", MFMA_SHAPES)
def test_mfma_defect_kernels_alone(built, M, R):
    """R0 + D.X from the ring kernel (two and one workgroup per CU) and the register-staged kernel, each within 2e-6 of the row
    scale of the long-double product, and of each other, on every element."""
    model, B, X, U, R0, ref, scale = defect_reference(M, R)
    got = {}
    for v, (options, name) in VARIANTS.items():
        got[v] = defect_only(model, B, M, X, U, R0, name, **options)
        err = (np.abs(np.asarray(got[v] - ref, dtype=np.float64)) / scale).max()
        print(f"f32 {v} M={M} R={R}: max err {err:.3e} of the row scale")
        assert err < F.TOL_F32, (v, M, R, err)
    assert (np.abs(got["ring"] - got["staged"]) <= F.TOL_F32 * scale).all()
    assert np.array_equal(got["ring"], got["ring_wgs1"])        # the same kernel with another LDS request


@pytest.mark.parametrize("M", F.FALLBACK_M)
def test_fallback_defect_kernel_alone(built, M):
    """emi_defect_f32_kernel where its guards k < M, n < M, r < R decide (M off 16 and 64, R off 16): elementwise within the
    derived bound, which has no margin.  M = 256 reaches it through "overlap" 0."""
    D = F.mesh(M)[2]
    for R in F.FALLBACK_R:
        model, B = F.ROWS[R]
        X, U, R0 = F.defect_case(model, B, M)
        RES = defect_only(model, B, M, X, U, R0, FALLBACK, **(dict(overlap=0) if M % 128 == 0 else {}))
        err = np.abs(np.asarray(RES - F.exact_defect(D, X, R0), dtype=np.float64))
        bound = F.fallback_bound(D, X, R0)
        print(f"f32 fallback M={M} R={R}: max err/bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (M, R, float((err / bound).max()))


# ---- b. exactness that the shifted form promises ------------------------------------------------------------------------------
@pytest.mark.parametrize("M", (128, 384))
def test_constant_rows_leave_the_starting_rows_bit_for_bit(built, M):
    """X constant along the nodes of each row (1e6 and a negative constant among them): x_j - s is exactly 0, so the MFMA forms
    add exactly 0 and return R0 bit for bit.  The fallback is NOT exact here -- its f32 diagonal is a rounded sum, so the row
    of Df does not annihilate the constant -- and is held to its bound instead."""
    B = 3
    X = F.constant_rows(B, 12, M)
    U = F.model_batch(F.FW, B, M)[1]
    R0 = F.start_rows(5, X.shape)
    for v in ("ring", "staged"):
        options, name = VARIANTS[v]
        assert np.array_equal(defect_only(F.FW, B, M, X, U, R0, name, **options), R0), v
    D = F.mesh(M)[2]
    RES = defect_only(F.FW, B, M, X, U, R0, FALLBACK, overlap=0)
    assert (np.abs(np.asarray(RES - F.exact_defect(D, X, R0), dtype=np.float64)) <= F.fallback_bound(D, X, R0)).all()


# ---- c. nothing is written past the batch -------------------------------------------------------------------------------------
def nan_outputs(ev, extra=0):
    """RES, VALS, COST for B + extra instances, every word NAN_BITS"""
    import torch
    lay = ev.layout
    mk = lambda *shape: torch.full(shape, NAN_BITS, dtype=torch.int32, device=ev.device).view(torch.float32)
    return mk(lay.B + extra, lay.nres, lay.M), mk(lay.B + extra, lay.nvals, lay.M), mk(lay.B + extra)


def run_dev(ev, X, U, outs, times=1, flags=None):
    import torch
    import etol_amd as E
    dX = torch.from_numpy(X.astype(np.float32)).to(ev.device)
    dU = torch.from_numpy(U.astype(np.float32)).to(ev.device)
    torch.cuda.synchronize()                 # the fills and copies run on torch's stream, the evaluator launches on its own
    for _ in range(times):
        ev.eval_dev(dX, dU, *outs, flags=E.EVAL_ALL if flags is None else flags)
    ev.synchronize()
    torch.cuda.synchronize()
    return [o.cpu().numpy().astype(np.float64) for o in outs]


# quadrotor B = 9: R = 54 rows, a ragged tile whose rows 54 .. 63 would be instances 9 and 10 -- the two guard instances;
# with three obstacles per instance nres = 9 > ns.  (128, 128) fixed wing: the smallest one-launch shape, full tiles only.
@pytest.mark.parametrize("form", ("ring", "ring_wgs1", "staged", "fallback", "one_launch"))
def test_nothing_is_written_past_the_batch(built, form):
    import torch
    if form == "one_launch":
        M, B = 128, 128
        X, U, recs = F.model_batch(F.FW, B, M)
        ev = make_ev(F.FW, F.W.FW_PARAMS, M, B, tf=20.0, f32_ring=0, overlap_mode=3)
        expect = ONE_LAUNCH
    else:
        M, B = (50 if form == "fallback" else 128), 9
        X, U, recs = F.model_batch(F.QUAD, B, M, 3)
        options, expect = VARIANTS[form] if form != "fallback" else ({}, FALLBACK)
        ev = make_ev(F.QUAD, F.W.QUAD_PARAMS, M, B, recs=recs, **options)
        assert ev.layout.nres == 9
    full = nan_outputs(ev, extra=2)
    got = run_dev(ev, X, U, [t[:B] for t in full])
    assert expect in ev.last_defect_kernel, ev.last_defect_kernel
    ev.close()
    assert not any(np.isnan(a).any() for a in got)
    for t in full:
        assert (t[B:].contiguous().view(torch.int32) == NAN_BITS).all().item()


# ---- d. the whole pass against the oracle: models, path rows ------------------------------------------------------------------
def check_defect_rows(c, got, ref, what, tol=F.TOL_F32):
    """the defect rows: tol (2e-6 at M <= 512, test_f32_context_fixedwing) of the row scale"""
    ns = c["X"].shape[1]
    e_def = (np.abs(got[0][:, :ns] - ref[0][:, :ns]) / F.row_scale(F.mesh(c["M"])[2], c["X"], ref[0][:, :ns])).max()
    print(f"f32 pass {what}: defect {e_def:.2e}")
    assert e_def < tol, what


def check_node_outputs(c, got, ref, what):
    """what the node kernel leaves, as test_f32_context_fixedwing holds it: path rows and each VALS entry to 2e-6 of the largest
    magnitude + 1, COST to 2e-6 relative"""
    ns = c["X"].shape[1]
    (RES, VALS, COST), (rRES, rVALS, rCOST) = got, ref
    e_path = np.abs(RES[:, ns:] - rRES[:, ns:]).max() / (np.abs(rRES[:, ns:]).max() + 1.0) if RES.shape[1] > ns else 0.0
    e_vals = max(np.abs(VALS[:, e] - rVALS[:, e]).max() / (np.abs(rVALS[:, e]).max() + 1.0) for e in range(VALS.shape[1]))
    e_cost = np.abs(COST - rCOST).max() / np.abs(rCOST).max()
    print(f"f32 pass {what}: path {e_path:.2e} vals {e_vals:.2e} cost {e_cost:.2e}")
    assert e_path < F.TOL_F32 and e_vals < F.TOL_F32 and e_cost < F.TOL_F32, what


def check_pass(c, got, ref, what):
    check_defect_rows(c, got, ref, what)
    check_node_outputs(c, got, ref, what)


def both_dispatches(c):
    """the pass at default dispatch and with "overlap" 0 (the fallback where the default is the ring), each on a fresh context"""
    out = {}
    mfma = c["M"] >= 128 and c["M"] % 128 == 0
    for overlap in (1, 0):
        ev = case_ev(c, overlap=overlap)
        out[overlap] = ev.eval_host(c["X"], c["U"])
        assert ev.last_defect_kernel == (RING if mfma and overlap else FALLBACK), (overlap, ev.last_defect_kernel)
        ev.close()
    return out


@pytest.mark.parametrize("name", ("pointmass_xml", "quad_ragged", "quad_tiny", "quad_128_obs", "quad_384_obs", "fixedwing_384",
                                  "quad_128_max"))
def test_whole_pass_against_the_oracle(built, name):
    import etol_amd as E
    c = F.whole_pass_case(name)
    ref = F.oracle_pass(c)
    out = both_dispatches(c)
    for overlap, got in out.items():
        check_pass(c, got, ref, f"{name} overlap={overlap}")
    ns = c["X"].shape[1]
    assert np.array_equal(out[1][1], out[0][1]) and np.array_equal(out[1][2], out[0][2])        # node kernel's work in both
    if name in ("quad_128_obs", "quad_384_obs"):
        # per-instance obstacles, nres = 9 > ns: the path rows are the node kernel's work whichever defect kernel follows, and a
        # defect epilogue that strayed into them (inst * ns for inst * nres) would change their bits
        ev = case_ev(c)
        nodes_only = ev.eval_host(c["X"], c["U"], flags=E.EVAL_NODES)
        ev.close()
        assert out[1][0].shape[1] == ns + 3
        assert np.array_equal(out[1][0][:, ns:], out[0][0][:, ns:])
        assert np.array_equal(out[1][0][:, ns:], nodes_only[0][:, ns:])
    if name == "quad_128_max":
        plain = dict(c, maximize=False)
        ev = case_ev(plain)
        pos = ev.eval_host(c["X"], c["U"])
        ev.close()
        nv = ns + c["U"].shape[1]
        assert (out[1][2] < 0).all() and np.array_equal(out[1][2], -pos[2])
        assert np.array_equal(out[1][1][:, -nv:], -pos[1][:, -nv:]) and np.abs(pos[1][:, -nv:]).max() > 0
        assert np.array_equal(out[1][0], pos[0])


# ---- e. flag forms in fp32 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("quad_384_obs", "quad_ragged"))
def test_nojac_and_split_passes_in_f32(built, name):
    """EVAL_ALL | EVAL_NOJAC leaves the RES and COST bits of EVAL_ALL; EVAL_NODES then EVAL_DEFECT onto its rows gives the bits
    of the single call (all of them the sequential form, which is what those flags select)."""
    import etol_amd as E
    c = F.whole_pass_case(name)
    expect = RING if c["M"] % 128 == 0 else FALLBACK
    ev = case_ev(c)
    RES, VALS, COST = ev.eval_host(c["X"], c["U"])
    assert ev.last_defect_kernel == expect
    RES2, _, COST2 = ev.eval_host(c["X"], c["U"], flags=E.EVAL_ALL | E.EVAL_NOJAC)
    assert ev.last_defect_kernel == expect
    assert np.array_equal(RES2, RES) and np.array_equal(COST2, COST)
    RESn, VALSn, COSTn = ev.eval_host(c["X"], c["U"], flags=E.EVAL_NODES)
    RESd, _, _ = ev.eval_host(c["X"], c["U"], flags=E.EVAL_DEFECT, res_in=RESn)
    assert ev.last_defect_kernel == expect
    ev.close()
    assert not np.array_equal(RESn, RES)
    assert np.array_equal(RESd, RES) and np.array_equal(VALSn, VALS) and np.array_equal(COSTn, COST)


# ---- f. two-stream form -------------------------------------------------------------------------------------------------------
def passes_profiled_as_overlapped(ev, X, U):
    """one more pass under the profiler: 1 if the library ran it as an overlapped (two-stream or one-launch) form"""
    ev.profile(1)
    run_dev(ev, X, U, list(ev.alloc_outputs()))
    n = ev.profile_read()["overlapped_passes"]
    ev.profile(0)
    return n


@pytest.mark.parametrize("name", ("quad_128_obs", "fixedwing_384"))
@pytest.mark.parametrize("ring", (1, 0))
def test_two_stream_form_gives_the_sequential_bits(built, name, ring):
    """"overlap_mode" 2: a values-only node kernel and the MFMA kernel on one stream, the full node kernel (np = 0 in the first
    leaves the path rows to it) beside them on a second; "f32_ring_wgs" 1 forks the second stream later.  RES (defect and path
    rows), VALS and COST are the sequential form's bits, twice running on NaN-filled buffers."""
    c = F.whole_pass_case(name)
    expect = RING if ring else STAGED
    ev = case_ev(c, f32_ring=ring, overlap_mode=1)
    seq = run_dev(ev, c["X"], c["U"], nan_outputs(ev))
    assert ev.last_defect_kernel == expect and passes_profiled_as_overlapped(ev, c["X"], c["U"]) == 0
    ev.close()
    assert not any(np.isnan(a).any() for a in seq)
    for wgs in (2, 1):
        ev = case_ev(c, f32_ring=ring, f32_ring_wgs=wgs, overlap_mode=2)
        two = run_dev(ev, c["X"], c["U"], nan_outputs(ev), times=2)
        assert ev.last_defect_kernel == expect
        assert passes_profiled_as_overlapped(ev, c["X"], c["U"]) == 1          # ... and it WAS the two-stream form
        ev.close()
        for q in range(3):
            assert np.array_equal(two[q], seq[q]), (wgs, q)


def test_two_stream_form_declines_a_mesh_off_the_tile(built):
    """M = 50: "overlap_mode" 2 reports the fallback kernel (the sequential form) and still matches"""
    c = F.whole_pass_case("quad_ragged")
    res = {}
    for mode in (1, 2):
        ev = case_ev(c, overlap_mode=mode)
        res[mode] = run_dev(ev, c["X"], c["U"], nan_outputs(ev), times=2)
        assert ev.last_defect_kernel == FALLBACK and passes_profiled_as_overlapped(ev, c["X"], c["U"]) == 0
        ev.close()
    for q in range(3):
        assert np.array_equal(res[2][q], res[1][q]) and not np.isnan(res[2][q]).any()
    check_pass(c, res[2], F.oracle_pass(c), "quad_ragged overlap_mode=2")


# ---- g. one-launch form -------------------------------------------------------------------------------------------------------
def fixedwing_pass(M, B):
    X, U, _ = F.model_batch(F.FW, B, M)
    return dict(model=F.FW, params=F.W.FW_PARAMS, M=M, B=B, t0=0.0, tf=20.0, X=X + 0.0, U=U, recs=None, tracks=None, maximize=False)


@pytest.mark.parametrize("M,B", [(512, 32), (128, 128), (1024, 16)])
def test_one_launch_form_at_its_smallest_shapes(built, M, B):
    """emi_pass_f32_kernel at the smallest shapes pass_f32_supported admits (R % 64 == 0, MFMA and node workgroups both multiples of
    8): the bits of the sequential pair with the register-staged kernel (signed zeros aside: both roles ADD onto zeroed rows),
    twice on NaN-filled buffers, in the interleaved and in a front-loaded block order ("pass_order" 0, 125: test_abi.py,
    test_front_loaded_pass_orders_match_the_oracle); the oracle's values on instances 0 .. 3."""
    c = fixedwing_pass(M, B)
    ev = case_ev(c, f32_ring=0, overlap_mode=1)
    seq = run_dev(ev, c["X"], c["U"], nan_outputs(ev))
    assert ev.last_defect_kernel == STAGED
    ev.close()
    for order in (-1, 0, 125):
        ev = case_ev(c, f32_ring=0, overlap_mode=3, pass_order=order)
        one = run_dev(ev, c["X"], c["U"], nan_outputs(ev), times=2)
        assert ONE_LAUNCH in ev.last_defect_kernel, ev.last_defect_kernel
        ev.close()
        for q in range(3):
            assert not np.isnan(one[q]).any() and np.array_equal(one[q], seq[q]), (order, q)
    sub = dict(c, B=4, X=c["X"][:4], U=c["U"][:4])
    ref = F.oracle_pass(sub)
    got = [a[:4] for a in one]
    # defect rows: 2e-6 up to 512 nodes, above them the project's 5e-6 (test_f32_pass_as_one_launch_matches_...)
    check_defect_rows(sub, got, ref, f"one launch ({M},{B})", tol=F.TOL_F32 if M <= 512 else 5e-6)
    check_node_outputs(sub, got, ref, f"one launch ({M},{B})")


@pytest.mark.parametrize("model,M,B", [(F.FW, 384, 64), (F.FW, 128, 16), (F.QUAD, 512, 32)])
def test_one_launch_form_declines_what_it_does_not_support(built, model, M, B):
    """36 and 3 MFMA workgroups (not multiples of 8), and a model the kernel is not built for: "overlap_mode" 3 succeeds, reports
    a sequential kernel and gives the sequential bits."""
    X, U, _ = F.model_batch(model, B, M)
    res = {}
    for mode in (1, 3):
        ev = make_ev(model, F.PARAMS[model], M, B, overlap_mode=mode)
        res[mode] = run_dev(ev, X, U, nan_outputs(ev))
        assert ev.last_defect_kernel == RING, (mode, ev.last_defect_kernel)
        ev.close()
    for q in range(3):
        assert np.array_equal(res[3][q], res[1][q]) and not np.isnan(res[3][q]).any()


# ---- h. fp32 Hessian ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("pointmass_xml", "quad_ragged", "fixedwing_64"))
def test_f32_hessian_against_the_oracle(built, name):
    """emi_hess_kernel<float> against oracle_lib.hessian, element by element (slot, instance, node): |H - Href| <= 2e-6 (T + 1),
    T = |sigma||H_cost| + sum_i |lam_i||H_i| the size of the terms that were summed there (unit-multiplier oracle calls): a
    small entry cannot hide behind a large one, and an entry whose terms cancel is not held to more digits than fp32 has.  The
    oracle's own noise in these units is below 1.2e-8 (tests/test_f32_ref_cpu.py).  Prints the worst elementwise ratio and, as
    a diagnostic, the worst ratio of the per-slot maxima; hess_dev on f32 tensors gives hess_host's bits."""
    import torch
    c = F.whole_pass_case(name)
    lamF, lamC = F.multipliers(c)
    Href, T = F.hessian_reference(c, lamF, lamC)
    ev = case_ev(c)
    H = ev.hess_host(c["X"], c["U"], lamF, lamC if lamC.shape[1] else None, sigma=F.SIGMA)
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).to(ev.device)
    dX, dU, dF, dC = f32(c["X"]), f32(c["U"]), f32(lamF), (f32(lamC) if lamC.shape[1] else None)
    dH = torch.full((c["B"], ev.layout.nhess, c["M"]), NAN_BITS, dtype=torch.int32, device=ev.device).view(torch.float32)
    torch.cuda.synchronize()
    ev.hess_dev(dX, dU, dF, dC, F.SIGMA, dH)
    ev.synchronize()
    ev.close()
    assert np.array_equal(dH.cpu().numpy().astype(np.float64), H)
    diff = np.abs(H - Href)
    slot = diff.max(axis=(0, 2)) / (T.max(axis=(0, 2)) + 1.0)
    ratio = diff / (T + 1.0)
    worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"f32 Hessian {name}: worst elementwise ratio {ratio.max():.3e} at (instance, slot, node) {tuple(int(i) for i in worst)}; "
          f"of the per-slot maxima {slot.max():.3e} (slot {int(slot.argmax())})")
    assert np.abs(Href).max() > 0 and (diff <= F.TOL_F32 * (T + 1.0)).all(), (name, worst, float(ratio.max()))
