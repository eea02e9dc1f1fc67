"""The exact first-order reference of tests/first_ref.py by itself, on the CPU: the fixture against hessian_terms.npz and the sympy
golden values, its structural pattern against emi_invariant_rows, the oracle's complex-step noise against it, the built-in model
structs compiled for the host against it (which is where first_ref.K_MODEL comes from), two perturbed structs that the elementwise
bound rejects at a size the check() of tests/test_gpu_parity.py accepts on its own cases, and the long-horizon condition of the
full-pass defect rows.  Prints the measured figures (pytest -s).  No GPU needed."""
import ctypes as C
import json
import os
import subprocess
import types

import numpy as np
import pytest

import cases
import first_ref as FR
import hess_ref as HR
import oracle_lib as O
from test_gpu_parity import TOL_DEFECT, TOL_NODE, check as parity_check
from test_hessian_ref_cpu import BUILDS, PARAMS, PRELUDE, STRUCTS, struct_text

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = json.load(open(os.path.join(HERE, "golden", "models.json")))
LD = FR.LD

# one call per model: n points z [n][NV] -> f [n][NS], J [n][NS][NV], L [n], g [n][NV].  emi_eps[2] are the relative perturbations of
# the two mutants (zero: the structs as they stand)
EPS = "extern \"C\" { double emi_eps[2] = {0.0, 0.0}; }\n"
POSTLUDE = r"""
template <class MODEL> static void run(int n, const double* p, int np, const double* z, double* f, double* J, double* L, double* g) {
    ModelParams<double> P = {};
    for (int i = 0; i < np; ++i) P.p[i] = p[i];
    constexpr int NS = MODEL::NS, NV = MODEL::NV;
    for (int k = 0; k < n; ++k) {
        double Jm[NS][NV];
        MODEL::f(P, z + k * NV, 0.0, f + k * NS);
        MODEL::jac(P, z + k * NV, 0.0, Jm);
        for (int i = 0; i < NS; ++i)
            for (int v = 0; v < NV; ++v) J[(k * NS + i) * NV + v] = Jm[i][v];
        L[k] = MODEL::cost(P, z + k * NV, 0.0);
        MODEL::grad(P, z + k * NV, 0.0, g + k * NV);
    }
}
extern "C" void first0(int n, const double* p, int np, const double* z, double* f, double* J, double* L, double* g) { run<PointMass2D<double>>(n, p, np, z, f, J, L, g); }
extern "C" void first1(int n, const double* p, int np, const double* z, double* f, double* J, double* L, double* g) { run<Quadrotor2D<double>>(n, p, np, z, f, J, L, g); }
extern "C" void first2(int n, const double* p, int np, const double* z, double* f, double* J, double* L, double* g) { run<FixedWing12<double>>(n, p, np, z, f, J, L, g); }
"""
# the mutants: the gravity term of Quadrotor2D::f; the drag term of d f6 / d wb of FixedWing12::jac (about 0.07 beside -qq)
MUTANTS = {1: ("fo[4] = a * c - P.p[2];", "fo[4] = a * c - P.p[2] * (T(1) + T(emi_eps[0]));"),
           2: ("J[6][8] = -qq - qS * dCD / m;", "J[6][8] = -qq - qS * dCD / m * (T(1) + T(emi_eps[1]));")}


def compile_structs(tmp_path, name, flags, patch=None):
    text = {m: struct_text(m) for m in STRUCTS}
    for m, (old, new) in (patch or {}).items():
        assert text[m].count(old) == 1, old
        text[m] = text[m].replace(old, new)
    cpp = tmp_path / f"{name}.cpp"
    cpp.write_text(PRELUDE + EPS + "".join(text[m] for m in sorted(text)) + POSTLUDE)
    so = tmp_path / f"{name}.so"
    subprocess.check_call(["g++", "-O2", "-Wno-unknown-pragmas", *flags, "-shared", "-fPIC", "-o", str(so), str(cpp)])
    lib = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    for m in STRUCTS:
        getattr(lib, f"first{m}").argtypes = [C.c_int, dp, C.c_int, dp, dp, dp, dp, dp]
    return lib


def host_first(lib, model, z):
    """-> f [ns][n], J [ns][nv][n], L [n], g [nv][n] of the host-compiled struct at the points z [n][nv]"""
    z = np.ascontiguousarray(z, dtype=np.float64)
    n, nv, ns = len(z), HR.NV[model], HR.NS[model]
    p = np.ascontiguousarray(PARAMS[model], dtype=np.float64)
    f, J, L, g = np.full((n, ns), np.nan), np.full((n, ns, nv), np.nan), np.full(n, np.nan), np.full((n, nv), np.nan)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    getattr(lib, f"first{model}")(n, dp(p) if p.size else None, p.size, dp(z), dp(f), dp(J), dp(L), dp(g))
    return f.T, np.transpose(J, (1, 2, 0)), L, g.T


def set_eps(lib, which, value):
    (C.c_double * 2).in_dll(lib, "emi_eps")[which] = value


# ---- the fixture -------------------------------------------------------------------------------------------------------------
def test_fixture_points_and_parameters_are_those_of_the_hessian_fixture():
    f, h = FR.fixture(), HR.fixture()
    for m in STRUCTS:
        assert f[f"z{m}"].tobytes() == h[f"z{m}"].tobytes() and f[f"params{m}"].tobytes() == h[f"params{m}"].tobytes()
        n, ns = HR.npoints(m), HR.NS[m]
        assert f[f"val{m}"].shape == f[f"mag{m}"].shape == (1 + ns, n)
        assert f[f"dval{m}"].shape == f[f"dmag{m}"].shape == (len(f[f"dterm{m}"]), n)
        assert (f[f"mag{m}"] >= np.abs(f[f"val{m}"])).all() and (f[f"dmag{m}"] >= np.abs(f[f"dval{m}"])).all()
    assert [len(f[f"dterm{m}"]) for m in (0, 1, 2)] == [4, 10, 65]
    assert os.path.getsize(os.path.join(HERE, "golden", "first_order_terms.npz")) < 1 << 20


@pytest.mark.parametrize("model", sorted(STRUCTS))
def test_fixture_entries_reproduce_the_golden_first_derivatives(model):
    """The entry functions at the six points of models.json give the f, J, L and gL stored there within 4 u A (models.json
    substitutes Python floats into the expression, so products of floats are rounded in double before its 40-digit evaluation: an
    ulp or two), and zero where nothing is stored."""
    val, mag, dval, dmag = FR.entries(model, np.arange(6), gold=True)
    for n, pt in enumerate(MODELS[str(model)]["points"]):
        gv = np.array([pt["L"]] + pt["f"], dtype=LD)
        gd = np.array([pt["gL"]] + pt["J"], dtype=LD)
        assert (np.abs(val[:, n] - gv) <= 4 * FR.U64 * mag[:, n]).all(), (model, n)
        assert (np.abs(dval[:, :, n] - gd) <= 4 * FR.U64 * dmag[:, :, n]).all(), (model, n)
        assert (gd[dmag[:, :, n] == 0] == 0).all()


@pytest.mark.parametrize("model", sorted(STRUCTS))
def test_invariant_rows_of_the_library_have_a_constant_magnitude(built, model):
    """Every VALS row that emi_invariant_rows flags (the rows an EMI_EVAL_KEEP_INVARIANT pass does not store) is, in the fixture, a
    structural zero or an entry whose value and magnitude sum are the same at every point; every other dynamics or gradient row
    is stored and varies."""
    import etol_amd as E
    nv, ns = HR.NV[model], HR.NS[model]
    mask = E.invariant_rows(model, 2)
    assert mask.shape == (ns * nv + 4 + nv,) and not mask[ns * nv:ns * nv + 4].any()
    val, mag, dval, dmag = FR.entries(model, np.arange(HR.npoints(model)))
    rows = [(i * nv + v, 1 + i, v) for i in range(ns) for v in range(nv)] + [(ns * nv + 4 + v, 0, v) for v in range(nv)]
    for row, t, v in rows:
        constant = (dmag[t, v] == dmag[t, v][0]).all() and (dval[t, v] == dval[t, v][0]).all()
        assert constant == bool(mask[row]), (model, row, t, v)


# ---- the oracle's noise in exact units -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(STRUCTS))
def test_oracle_noise_against_the_exact_reference(built, model):
    """oracle_lib.evaluate (complex-step derivatives, long-double D.X) against the reference in units of u A, at every fixture point
    with the mixed record tables: it is a second witness of the reference's plumbing -- a record, a set, a state or a sign read
    wrongly would be off by the size of an entry -- and its own noise is printed.  Measured: VALS within 4.72 u A, record rows
    3.56, COST 0.69, the finished defect rows (the oracle always adds D.X) within 0.04 of their bound."""
    M, B = 33, 3
    mesh, (t0, tf) = O.lgl(M), (0.5, 9.0)
    idx = HR.cycle(model, B, M, start=HR.npoints(model) - B * M)
    X, U = HR.points(model, idx)
    recs, tracks = HR.mixed_tables(), HR.track_centres(M)
    px, py = (1, 0) if model == 0 else (4, 3)
    r = FR.reference(model, idx, mesh, t0, tf, True, recs, tracks, px, py, full=True)
    RES, VALS, COST = O.evaluate(model, PARAMS[model], M, mesh, t0, tf, X, U, recs, tracks, px=px, py=py, maximize=True)
    ns = r.ns
    noise = {"-h f rows": FR.worst(RES[:, :ns], r.RES[:, :ns], r.LIM_DEF),
             "path rows": FR.worst(RES[:, ns:], r.RES[:, ns:], FR.U64 * r.A_RES[:, ns:]),
             "VALS": FR.worst(VALS, r.VALS, FR.U64 * r.A_VALS),
             "COST": FR.worst(COST, r.COST, FR.U64 * r.A_COST)}
    print(f"oracle, model {model}: " + ", ".join(f"{k} {v[0]:.2f} at {v[1]}" for k, v in noise.items()) + "  (defect rows in units of their bound, the rest of u A)")
    assert noise["-h f rows"][0] <= 1.0
    assert max(noise[k][0] for k in ("path rows", "VALS")) <= 8.0 and noise["COST"][0] <= FR.k_cost(model, M)
    assert (VALS[np.broadcast_to(r.A_VALS == 0, VALS.shape)] == 0).all()


# ---- the built-in structs on the host: where K_MODEL comes from ----------------------------------------------------------------------
def host_ratios(lib, model):
    """worst |e - ref| / (u A) of f, jac, cost, grad at every fixture point -> {name: (ratio, position)}; exact zeros asserted"""
    n = HR.npoints(model)
    val, mag, dval, dmag = FR.entries(model, np.arange(n))
    f, J, L, g = host_first(lib, model, HR.fixture()[f"z{model}"])
    out = {}
    for name, got, ref, A in (("f", f, val[1:], mag[1:]), ("jac", J, dval[1:], dmag[1:]), ("cost", L, val[0], mag[0]), ("grad", g, dval[0], dmag[0])):
        assert not np.isnan(got).any() and (got[A == 0] == 0).all(), (model, name)
        out[name] = FR.worst(got, ref, FR.U64 * A)
    return out


def test_host_compiled_structs_lie_within_the_bound(tmp_path):
    """PointMass2D, Quadrotor2D and FixedWing12 as they stand in csrc/emi_models.hpp, compiled by g++ plain and with fused
    multiply-adds, at every fixture point: every entry of f, jac, cost and grad within K_MODEL u A, entries with A == 0 exactly
    zero.  K_MODEL (tests/first_ref.py) is 8 times the worst ratio printed here, rounded up to a power of two."""
    top = {m: 0.0 for m in STRUCTS}
    for build, flags in BUILDS.items():
        lib = compile_structs(tmp_path, build, flags)
        for model in sorted(STRUCTS):
            r = host_ratios(lib, model)
            print(f"host build '{build}' of {STRUCTS[model]}: " + ", ".join(f"{k} {v[0]:.2f} at {v[1]}" for k, v in r.items()) +
                  "   (|e - ref| / (u A); position: (entry.., fixture point))")
            top[model] = max(top[model], *(v[0] for v in r.values()))
    for model in sorted(STRUCTS):
        derived = 2.0 ** np.ceil(np.log2(8.0 * top[model]))
        print(f"{STRUCTS[model]}: worst host ratio {top[model]:.4f}: 8 x rounded up to a power of two = {derived:g}; first_ref.K_MODEL = {FR.K_MODEL[model]:g}")
        assert 8.0 * top[model] <= FR.K_MODEL[model]      # another libm may move the ratio; K_MODEL stays the figure derived in first_ref.py


# ---- two mutants: what the criterion of test_gpu_parity.check admits, and the new one does not ------------------------------------------
def parity_case(name):
    """one case of tests/cases.py as check() of test_gpu_parity sees it: inputs, the oracle's result, the mesh"""
    c = cases.case_inputs(name)
    mesh = O.lgl(c["M"])
    ref = O.evaluate(c["model"], c["params"], c["M"], mesh, c["t0"], c["tf"], c["X"], c["U"], c.get("recs"))
    return c, mesh, ref


def mutant_outputs(lib, c, mesh, ref):
    """(RES, VALS, COST) with the defect rows and the dynamics block of VALS from the host-compiled struct -- D.X in long double
    plus the struct's -h f, rounded once; -h J + D_kk -- and every other row as the oracle has it"""
    model, M = c["model"], c["M"]
    ns, nv = HR.NS[model], HR.NV[model]
    h = (c["tf"] - c["t0"]) / 2.0
    RES, VALS, COST = (a.copy() for a in ref)
    DX, _ = FR.operator_product(mesh[2], c["X"])
    dkk = np.diagonal(mesh[2])
    for b in range(c["B"]):
        z = np.concatenate([c["X"][b], c["U"][b]]).T
        f, J, _, _ = host_first(lib, model, z)
        RES[b, :ns] = np.asarray(DX[b] + np.asarray(-h * f, dtype=LD), dtype=np.float64)
        for i in range(ns):
            for v in range(nv):
                VALS[b, i * nv + v] = -h * J[i, v] + (dkk if v == i else 0.0)
    return RES, VALS, COST


QUAD_CASES = ("quad_256", "quad_1024_obs", "quad_ragged", "quad_tiny")


def test_elementwise_bound_rejects_what_the_parity_criterion_admits(tmp_path):
    """A relative error eps in the gravity term of Quadrotor2D::f, and one in the drag term of d f6 / d wb of FixedWing12::jac.
    For each, the largest eps that check() of tests/test_gpu_parity.py accepts on every one of its own cases of that model is
    worked out from the criterion's own scales (the error is eps times a known term) and then handed to check() itself, which
    must accept it; the elementwise criterion must reject the same struct at the fixture points.  Both sizes are printed beside
    the smallest eps the new criterion could still miss."""
    lib = compile_structs(tmp_path, "mutants", [], MUTANTS)
    # -- f: the error of defect row 4 is h g eps at every element
    g = PARAMS[1][2]
    room = []
    for name in QUAD_CASES:
        c, mesh, ref = parity_case(name)
        h = (c["tf"] - c["t0"]) / 2.0
        got = mutant_outputs(lib, c, mesh, ref)
        parity_check(c, types.SimpleNamespace(D=mesh[2]), got, ref)                  # the struct as it stands passes
        scale = np.einsum("kj,bij->bik", np.abs(mesh[2]), np.abs(c["X"])) + np.abs(ref[0][:, :6]) + 1.0
        slack = TOL_DEFECT * scale[:, 4] - np.abs(got[0][:, 4] - ref[0][:, 4])
        room.append((slack / (h * g)).min())
        print(f"f mutant, {name}: check() admits eps up to {room[-1]:.2e}")
    eps_f = 0.9 * min(room)
    set_eps(lib, 0, eps_f)
    for name in QUAD_CASES:
        c, mesh, ref = parity_case(name)
        parity_check(c, types.SimpleNamespace(D=mesh[2]), mutant_outputs(lib, c, mesh, ref), ref)
    val, mag, _, _ = FR.entries(1, np.arange(HR.npoints(1)))
    f, _, _, _ = host_first(lib, 1, HR.fixture()["z1"])
    ok = FR.within(f, val[1:], mag[1:], FR.K_MODEL[1])
    ratio, at = FR.worst(f, val[1:], FR.U64 * mag[1:])
    print(f"f mutant: eps = {eps_f:.2e} passes check() on {', '.join(QUAD_CASES)}; elementwise ratio {ratio:.3g} at {at} (bound {FR.K_MODEL[1]:g}): "
          f"{(~ok[4]).sum()} of {ok[4].size} points of f_4 rejected; the new criterion admits at most eps = {FR.K_MODEL[1] * FR.U64 * float((mag[5] / g).max()):.1e}")
    assert not ok[4].any() and ok[[0, 1, 2, 3, 5]].all()
    # ... and the full-pass bound on the long horizon rejects it in (nearly) every element of row 4
    M, B = 128, 17
    mesh = O.lgl(M)
    r = FR.reference(1, FR.horizon_points(1, B, M), mesh, *FR.HORIZON, full=True)
    z = HR.fixture()["z1"][FR.horizon_points(1, B, M)].reshape(B * M, -1)
    fm = host_first(lib, 1, z)[0].reshape(6, B, M).transpose(1, 0, 2)
    got = np.asarray(r.DX + np.asarray(-float(r.h) * fm, dtype=LD), dtype=np.float64)
    bad = np.abs(np.asarray(got, dtype=LD) - r.RES[:, :6]) > r.LIM_DEF
    print(f"f mutant, full pass at tf = 2^21, ({M}, {B}): {bad[:, 4].mean():.1%} of row 4 outside the bound, {bad[:, [0, 1, 2, 3, 5]].sum()} elsewhere")
    assert bad[:, 4].mean() > 0.99 and not bad[:, [0, 1, 2, 3, 5]].any()
    set_eps(lib, 0, 0.0)
    # -- jac: the error of VALS entry (6, 8) is h qS dCD / m eps, dCD = 2 CDk CL CLa / V
    c, mesh, ref = parity_case("fixedwing_64")
    h = (c["tf"] - c["t0"]) / 2.0
    P = PARAMS[2]
    CL = P[6] + P[7] * c["X"][:, 8] / P[13]
    term = h * P[5] * 2.0 * P[9] * CL * P[7] / P[13] / P[0]
    e = 6 * 16 + 8
    got = mutant_outputs(lib, c, mesh, ref)
    parity_check(c, types.SimpleNamespace(D=mesh[2]), got, ref)
    s = np.abs(ref[1][:, e]).max() + 1.0
    eps_j = 0.9 * ((TOL_NODE * s - np.abs(got[1][:, e] - ref[1][:, e]).max()) / np.abs(term).max())
    set_eps(lib, 1, eps_j)
    parity_check(c, types.SimpleNamespace(D=mesh[2]), mutant_outputs(lib, c, mesh, ref), ref)
    _, _, dval, dmag = FR.entries(2, np.arange(HR.npoints(2)))
    _, J, _, _ = host_first(lib, 2, HR.fixture()["z2"])
    ok = FR.within(J, dval[1:], dmag[1:], FR.K_MODEL[2])
    ratio, at = FR.worst(J, dval[1:], FR.U64 * dmag[1:])
    print(f"jac mutant: eps = {eps_j:.2e} passes check() on fixedwing_64 (entry about {np.abs(ref[1][:, e]).mean() / h:.2f}, row scale {s / h:.2f}); "
          f"elementwise ratio {ratio:.3g} at {at} (bound {FR.K_MODEL[2]:g}): {(~ok[6, 8]).sum()} of {ok[6, 8].size} points rejected")
    assert (~ok[6, 8]).mean() > 0.9
    ok[6, 8] = True
    assert ok.all()


# ---- the long horizon of the full-pass cases -------------------------------------------------------------------------------------
def even_odd_product(D, X):
    """D.X in double the way the even/odd kernels form it: De, Do and x_j +- x_m rounded, two half-length dot products, combined"""
    M = D.shape[0]
    H = M // 2
    De, Do = (D[:, :H] + D[:, ::-1][:, :H]) / 2.0, (D[:, :H] - D[:, ::-1][:, :H]) / 2.0
    e, o = X[..., :H] + X[..., ::-1][..., :H], X[..., :H] - X[..., ::-1][..., :H]
    return np.einsum("kj,bij->bik", De, e) + np.einsum("kj,bij->bik", Do, o)


@pytest.mark.parametrize("model,M,B", FR.HORIZON_SHAPES)
def test_long_horizon_lets_the_defect_bound_see_f(built, model, M, B):
    """On t0 = 0, tf = 2^21 the full-pass bound admits a relative error in h f_i of at most 1e-12 in at least 99 % of the
    defect-row elements of every shape tests/test_gpu_first_order.py uses (from the reference alone); at tf = 9 it does not.
    Also: a plain double evaluation of D.X -- even/odd for even M, direct otherwise -- minus the exactly rounded h f lies within
    the bound; what it reaches against the bound with S in place of S_op, and S' / S of the derivation in first_ref.py, are printed."""
    mesh = O.lgl(M)
    idx = FR.horizon_points(model, B, M)
    r = FR.reference(model, idx, mesh, *FR.HORIZON, full=True)
    adm = FR.admitted(r)
    p50, p99 = np.percentile(adm, 50), np.percentile(adm, 99)
    short = np.percentile(FR.admitted(FR.reference(model, idx, mesh, 0.0, 9.0, full=True)), 99)
    X, _ = HR.points(model, idx)
    D = mesh[2]
    dx = even_odd_product(D, X) if M % 2 == 0 else np.einsum("kj,bij->bik", D, X)
    got = dx + np.asarray(r.MHF, dtype=np.float64)
    ratio, at = FR.worst(got, r.RES[:, :r.ns], r.LIM_DEF)
    plain = FR.worst(got, r.RES[:, :r.ns], FR.U64 * (FR.c_op(M) * r.S + FR.k_def(model) * r.A_RES[:, :r.ns] + np.abs(r.RES[:, :r.ns])))[0]
    sprime = np.asarray(r.SP / r.S, dtype=np.float64)
    if (model, M, B) in FR.SEQUENTIAL_SHAPES:
        # the pair adds the products onto -h f: emulated in that order, held to the pair's bound, which must meet the condition too
        ra = FR.reference(model, idx, mesh, *FR.HORIZON, full=True, accumulated=True)
        acc = np.asarray(r.MHF, dtype=np.float64)
        for j in range(M):
            acc = acc + X[:, :, j][:, :, None] * D[None, None, :, j]
        seq, pair = FR.worst(acc, r.RES[:, :r.ns], r.LIM_DEF), FR.worst(acc, ra.RES[:, :ra.ns], ra.LIM_DEF)
        pp99 = np.percentile(FR.admitted(ra), 99)
        print(f"model {model} ({M}, {B}) accumulated onto -h f in double: worst |got - ref| / bound {seq[0]:.3f} at {seq[1]} of the one-combination "
              f"bound, {pair[0]:.3f} of the pair's; the pair's bound admits {pp99:.1e} (99th percentile)")
        assert pair[0] <= 1.0 and pp99 <= 1e-12
    print(f"model {model} ({M}, {B}) tf = 2^21: admitted relative error in h f_i median {p50:.1e}, 99th percentile {p99:.1e} (tf = 9: {short:.1e}); "
          f"double evaluation: worst |got - ref| / bound {ratio:.3f} at {at} (with S for S_op: {plain:.3f}); S' / S median {np.median(sprime):.2f}, max {sprime.max():.1f}")
    assert p99 <= 1e-12 and ratio <= 1.0 and short > 1e-12
