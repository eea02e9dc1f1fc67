"""The exact Hessian reference of tests/hess_ref.py by itself, on the CPU: the fixture against the sympy golden values, the oracle's
finite-difference noise against it, the built-in model structs compiled for the host against it (which is where the bound constant K
of tests/hess_ref.py comes from), and two perturbed structs that the elementwise bound rejects and the global 1e-7 criterion of
test_hessian_blocks accepts.  Prints the measured figures (pytest -s).  No GPU needed."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cases
import hess_ref as HR
import oracle_lib as O
from etol_amd import workloads as W

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = json.load(open(os.path.join(HERE, "golden", "models.json")))
PARAMS = {0: np.zeros(0), 1: W.QUAD_PARAMS, 2: W.FW_PARAMS}
STRUCTS = {0: "PointMass2D", 1: "Quadrotor2D", 2: "FixedWing12"}
BUILDS = {"plain": [], "fma": ["-mfma", "-ffp-contract=fast"]}

PRELUDE = r"""
#include <cmath>
#define EMI_DEV inline
#define EMI_MAX_PARAMS 16
template <typename T> struct ModelParams { T p[EMI_MAX_PARAMS]; };
inline void emi_sincos(double a, double* s, double* c) { *s = std::sin(a); *c = std::cos(a); }
inline double emi_sin(double a) { return std::sin(a); }
inline double emi_cos(double a) { return std::cos(a); }
inline double emi_tan(double a) { return std::tan(a); }
"""
# one call per model: n points z [n][NV], the cost coefficient cL [n] and the state coefficients cf [n][NS] -> H [n][NH]
POSTLUDE = r"""
template <class MODEL> static void run(int n, const double* p, int np, const double* z, const double* cL, const double* cf, double* H) {
    ModelParams<double> P = {};
    for (int i = 0; i < np; ++i) P.p[i] = p[i];
    const int NH = MODEL::NV * (MODEL::NV + 1) / 2;
    for (int k = 0; k < n; ++k) {
        for (int q = 0; q < NH; ++q) H[k * NH + q] = 0;
        MODEL::hess(P, z + k * MODEL::NV, 0.0, cL[k], cf + k * MODEL::NS, H + k * NH);
    }
}
extern "C" void hess0(int n, const double* p, int np, const double* z, const double* cL, const double* cf, double* H) { run<PointMass2D<double>>(n, p, np, z, cL, cf, H); }
extern "C" void hess1(int n, const double* p, int np, const double* z, const double* cL, const double* cf, double* H) { run<Quadrotor2D<double>>(n, p, np, z, cL, cf, H); }
extern "C" void hess2(int n, const double* p, int np, const double* z, const double* cL, const double* cf, double* H) { run<FixedWing12<double>>(n, p, np, z, cL, cf, H); }
"""


def struct_text(model):
    src = open(os.path.join(os.path.dirname(HERE), "etol_amd", "csrc", "emi_models.hpp")).read()
    a = src.index(f"template <typename T> struct {STRUCTS[model]} {{")
    return src[a:src.index("\n};", a) + 3] + "\n"


def compile_structs(tmp_path, name, flags, patch=None):
    """the three structs of emi_models.hpp behind the host prelude; patch: {model: (old, new)} applied to the copy in tmp_path"""
    text = {m: struct_text(m) for m in STRUCTS}
    for m, (old, new) in (patch or {}).items():
        assert text[m].count(old) == 1, old
        text[m] = text[m].replace(old, new)
    cpp = tmp_path / f"{name}.cpp"
    cpp.write_text(PRELUDE + "".join(text[m] for m in sorted(text)) + POSTLUDE)
    so = tmp_path / f"{name}.so"
    subprocess.check_call(["g++", "-O2", "-Wno-unknown-pragmas", *flags, "-shared", "-fPIC", "-o", str(so), str(cpp)])
    lib = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    for m in STRUCTS:
        getattr(lib, f"hess{m}").argtypes = [C.c_int, dp, C.c_int, dp, dp, dp, dp]
    return lib


MESH = dict(t0=0.0, tf=16.0)


def host_case(model):
    """every fixture point of the model as the nodes of one instance; seeded multipliers and weights"""
    n = HR.npoints(model)
    idx = np.arange(n)[None, :]
    lamF, _ = HR.multipliers(1, HR.NS[model], 0, n)
    w = np.random.default_rng(3).uniform(1e-4, 1.0, n)
    return idx, w, lamF


def host_hessian(lib, model, idx, w, lamF, sigma=HR.SIGMA, maximize=False):
    """what emi_hess_kernel hands to Model::hess, in double: cL = sigma sgn h w_k, cf_i = -h lamF_i; -> H [1][nh][n]"""
    n = idx.shape[1]
    nv, ns = HR.NV[model], HR.NS[model]
    nh = nv * (nv + 1) // 2
    h = (MESH["tf"] - MESH["t0"]) / 2.0
    z = np.ascontiguousarray(HR.fixture()[f"z{model}"][idx[0]])
    cL = np.ascontiguousarray(sigma * (-1.0 if maximize else 1.0) * h * w)
    cf = np.ascontiguousarray((-h * lamF[0]).T)
    p = np.ascontiguousarray(PARAMS[model], dtype=np.float64)
    H = np.full((n, nh), np.nan)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    getattr(lib, f"hess{model}")(n, dp(p) if p.size else None, p.size, dp(z), dp(cL), dp(cf), dp(H))
    return np.ascontiguousarray(H.T)[None]


# ---- the fixture -------------------------------------------------------------------------------------------------------------
def test_fixture_parameters_and_points_are_the_workloads(built):
    """The generator restates the parameter sets and the seeded batches; they must be the product's, bit for bit."""
    f = HR.fixture()
    batch = {0: lambda c, B, M: np.concatenate(W.pointmass_batch(c, B, M), axis=1),
             1: lambda c, B, M: np.concatenate(W.quadrotor_batch(c, B, M, 0)[:2], axis=1),
             2: lambda c, B, M: np.concatenate(W.fixedwing_batch(c, B, M), axis=1)}
    for m in STRUCTS:
        assert np.array_equal(f[f"params{m}"], np.asarray(PARAMS[m], dtype=np.float64))
        assert f[f"z{m}"].shape[1] == HR.NV[m] and f[f"val{m}"].shape == (len(f[f"term{m}"]), HR.npoints(m))
        for config, B, M, take, first in f[f"batch{m}"]:
            z = np.transpose(batch[m](int(config), int(B), int(M)), (0, 2, 1))[:, :take].reshape(B * take, -1)
            assert np.array_equal(f[f"z{m}"][first:first + B * take], z), (m, config)
        assert HR.npoints(m) > int(f[f"batch{m}"][-1][4] + f[f"batch{m}"][-1][1] * f[f"batch{m}"][-1][3])      # edge points follow
    assert len(f["term2"]) == 74 and len(set(f["slot2"].tolist())) == 32
    z1, z2 = f["z1"], f["z2"]
    assert np.abs(z1[:, 2]).max() > np.pi and (z1[:, 6] == 0).any() and np.signbit(z1[:, 6:][z1[:, 6:] == 0]).any()
    assert (z2[:, 4] == 1.2).any() and (z2[:, 4] == -1.2).any()


@pytest.mark.parametrize("model", sorted(STRUCTS))
def test_fixture_terms_reproduce_the_golden_hessians(model):
    """The term functions evaluated at the six points of models.json and combined with each point's cL and cf in long double give
    that point's H (sympy, 40 digits, the Lagrangian differentiated as a whole) to 1e-15 of the terms' magnitudes."""
    f = HR.fixture()
    nv = HR.NV[model]
    for n, pt in enumerate(MODELS[str(model)]["points"]):
        coef = np.array([pt["cL"]] + pt["cf"], dtype=HR.LD)
        H = np.zeros(nv * (nv + 1) // 2, dtype=HR.LD)
        T = np.zeros_like(H)
        for t, q, v in zip(f[f"term{model}"], f[f"slot{model}"], f[f"gold{model}"]):
            H[q] += coef[t] * v[n]
            T[q] += abs(coef[t] * v[n])
        gold = np.array(pt["H"], dtype=HR.LD)
        assert (gold[T == 0] == 0).all()
        assert (np.abs(H - gold) <= 1e-15 * T).all(), (model, n, float((np.abs(H - gold) / np.maximum(T, 1e-300)).max()))


# ---- the oracle's noise in exact units -------------------------------------------------------------------------------------------
def oracle_case(name):
    """the cases of test_hessian_blocks (quad_ragged: its first four instances, the ones the fixture holds) -> dict for both sides"""
    c = cases.case_inputs(name)
    model = c["model"]
    first, B, take = HR.batch_rows(model, 0)
    assert take == c["M"]
    idx = first + np.arange(B * take).reshape(B, take)
    mesh = O.lgl(c["M"])
    recs, tracks = c.get("recs"), None
    if c.get("ocp2d"):
        node_t = c["t0"] + (c["tf"] - c["t0"]) / 2.0 * (mesh[0] + 1.0)
        recs, tx, ty = cases.ocp2d_tables(O.edge_ellipse, O.track_centres, node_t)
        tracks = (tx, ty)
    X, U = HR.points(model, idx)
    assert np.array_equal(X, c["X"][:B]) and np.array_equal(U, c["U"][:B])
    return dict(model=model, params=c["params"], M=c["M"], B=B, t0=c["t0"], tf=c["tf"], X=X, U=U, recs=recs, tracks=tracks,
                idx=idx, mesh=mesh)


@pytest.mark.parametrize("name", ("pointmass_xml", "quad_ragged", "fixedwing_64"))
def test_oracle_hessian_noise_against_the_exact_reference(built, name):
    """oracle_lib.hessian (central differences of complex-step gradients) against (Href, T), element by element, within the noise
    tests/test_f32_ref_cpu.py found for it from its linearity residual: 1.2e-8 (T + 1).  Measured here against the exact terms:
    9.0e-11 (pointmass_xml), 7.3e-9 (quad_ragged), 7.1e-9 (fixedwing_64) of T + 1."""
    c = oracle_case(name)
    npth = 0 if c["recs"] is None else np.asarray(c["recs"]).shape[-2]
    lamF, lamC = HR.multipliers(c["B"], HR.NS[c["model"]], npth, c["M"])
    Href, T = HR.reference(c["model"], c["idx"], c["mesh"][1], c["t0"], c["tf"], HR.SIGMA, False, lamF, lamC, c["recs"], c["tracks"])
    Ho = O.hessian(c["model"], c["params"], c["M"], c["mesh"], c["t0"], c["tf"], c["X"], c["U"], lamF, lamC, HR.SIGMA, c["recs"],
                   c["tracks"])
    noise = np.abs(Ho - Href) / (T + 1.0)
    at = np.unravel_index(int(noise.argmax()), noise.shape)
    print(f"oracle Hessian {name}: worst |H_oracle - Href| / (T + 1) = {noise.max():.2e} at (instance, slot, node) {tuple(int(i) for i in at)}")
    assert np.abs(Href).max() > 0 and noise.max() <= 1.2e-8


@pytest.mark.parametrize("model,px,py,shared,maximize", [(1, 0, 1, False, False), (1, 0, 1, True, False), (1, 3, 4, False, False),
                                                         (1, 4, 3, False, True), (0, 1, 0, False, False), (2, 1, 0, False, True)])
def test_reference_reads_tables_states_and_sign_as_the_oracle_does(built, model, px, py, shared, maximize):
    """The reference's own plumbing on the inputs of the GPU cases -- a table per instance or one shared, ellipse, disc and track
    rows in every order, (px, py) in both orders, the maximize sign -- against the oracle, within the oracle's 1.2e-8 (T + 1): a
    reference that read a record, a set or a slot wrongly would be off by the size of an entry."""
    M, B = 17, 3
    mesh, t0, tf = O.lgl(M), 0.5, 9.0
    recs = HR.mixed_tables()[1] if shared else HR.mixed_tables()
    tracks = HR.track_centres(M)
    idx = HR.cycle(model, B, M, start=40)
    X, U = HR.points(model, idx)
    lamF, lamC = HR.multipliers(B, HR.NS[model], 5, M)
    Href, T = HR.reference(model, idx, mesh[1], t0, tf, HR.SIGMA, maximize, lamF, lamC, recs, tracks, px, py)
    Ho = O.hessian(model, PARAMS[model], M, mesh, t0, tf, X, U, lamF, lamC, HR.SIGMA, recs, tracks, px, py, maximize)
    noise = np.abs(Ho - Href) / (T + 1.0)
    print(f"oracle Hessian model {model} ({px}, {py}) shared={shared} maximize={maximize}: worst {noise.max():.2e} of T + 1")
    assert (np.abs(Href[:, list(HR.path_slots(px, py))]) > 0).all() and noise.max() <= 1.2e-8


# ---- the built-in structs on the host: where K comes from --------------------------------------------------------------------------
def test_host_compiled_structs_lie_within_the_bound(tmp_path):
    """PointMass2D, Quadrotor2D and FixedWing12 as they stand in csrc/emi_models.hpp, compiled by g++ plain and with fused
    multiply-adds, at every fixture point: |H - Href| <= K u (T + 1) for every entry, entries that no term touches exactly zero.
    K (tests/hess_ref.py) is 8 times the worst ratio printed here, rounded up to a power of two."""
    top = 0.0
    for build, flags in BUILDS.items():
        lib = compile_structs(tmp_path, build, flags)
        for model in sorted(STRUCTS):
            idx, w, lamF = host_case(model)
            Href, T = HR.reference(model, idx, w, MESH["t0"], MESH["tf"], HR.SIGMA, False, lamF)
            H = host_hessian(lib, model, idx, w, lamF)
            ratio, at = HR.check(f"host build '{build}' of {STRUCTS[model]} (node = fixture point)", H, Href, T)
            top = max(top, ratio)
    derived = 2.0 ** np.ceil(np.log2(8.0 * top))
    print(f"worst host ratio {top:.2f}: 8 x rounded up to a power of two = {derived:g}; hess_ref.K = {HR.K:g}")
    assert 8.0 * top <= HR.K            # another libm may move the ratio; K stays the figure derived where hess_ref.py says


def test_elementwise_bound_sees_what_the_global_criterion_does_not(tmp_path):
    """A relative error of 1e-9 in one product of Quadrotor2D::hess (a * s) and in one generated product of FixedWing12::hess
    (v35 = cos(phi) sin(theta)): the elementwise bound rejects both, 1e-7 (|Href|.max() + 1) accepts both."""
    patch = {1: ("cf[3] * (a * s)", "cf[3] * (a * s * (T(1) + T(1e-9)))"),
             2: ("const T v35 = v17 * v18;", "const T v35 = v17 * v18 * (T(1) + T(1e-9));")}
    lib = compile_structs(tmp_path, "perturbed", [], patch)
    for model in patch:
        idx, w, lamF = host_case(model)
        Href, T = HR.reference(model, idx, w, MESH["t0"], MESH["tf"], HR.SIGMA, False, lamF)
        H = host_hessian(lib, model, idx, w, lamF)
        ratio, at = HR.worst(H, Href, T)
        old = np.abs(H - Href).max() / (np.abs(Href).max() + 1.0)
        print(f"perturbed {STRUCTS[model]}: worst elementwise ratio {ratio:.3g} (bound {HR.K:g}) at {at}; global criterion {old:.2e} (bound 1e-7)")
        assert not (np.abs(H - Href) <= HR.K * HR.U64 * (T + 1.0)).all()
        assert old < 1e-7
