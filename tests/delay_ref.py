"""Delayed values of a context with delays, element by element: the tap models that carry the extended node variables out of a
pass, and the long-double reference of the products extend_controls (csrc/emi_api_pass.hip) forms.  Test infrastructure.

The tap model.  Tap<ns>x<nc> passes its inputs through: f_i = z[i] and J[0][ns+q] = z[ns+q], cost and gradient zero.  On a horizon
whose half-length h is a power of two the node kernel stores -h f and -h J + 0 (the entries are off the diagonal: no D_kk), so a
nodes-only Jacobian pass returns control slot q of every node as -VALS[0 nv + ns + q] / h and state i as -RES[i] / h, every
operation exact.  One thing the Jacobian route does not carry is the sign of a zero: -h z + 0 is +0 for z = +0 and for z = -0, so
a zero comes back as -0.  Every nonzero double, denormals included, comes back bit for bit, and two finite doubles that compare
equal and are not zero have the same bits; same() therefore compares values and refuses NaN.

The reference.  W_i is the library's own host routine emi_delay_matrix (the function that fills d_W), the product with the node
values is formed in numpy.longdouble (64-bit significand on x86) together with S = sum_j |W_kj| |z_j|.  The device forms an
M-term dot product, in some order, onto rows zeroed beforehand: M roundings at most on any path from a product to the result
(FMA or not), so |got - exact| <= M u S (1 + O(M u)), u = 2^-53.  The reference rounded to double is within u |exact| / 2 +
M 2^-64 S <= u S of the exact value for M <= 2048.  Hence
        |got - ref| <= (M + 2) u S          elementwise, no floor (S = 0: got must be 0).
A unit row of W (clamped to node 0, or a delayed time exactly on a node) has products with 0 and 1 only and sums of zeros: the
delayed value must be the source's node value itself."""
import ctypes as C

import numpy as np

U53 = 2.0 ** -53
DP = C.POINTER(C.c_double)

# (ns, nc) of every tap model the tests use (each costs a run-time compilation: six at most)
TAP_DIMS = ((3, 5), (2, 10), (1, 9), (2, 8), (6, 2), (12, 4))
_sources = {}


def tap_source(ns, nc):
    """(struct name, text) of the tap model with ns states and nc control slots, in the style of PointMass2D (csrc/emi_models.hpp)"""
    if (ns, nc) not in _sources:
        assert (ns, nc) in TAP_DIMS, "a new tap model is a new run-time compilation: add it to TAP_DIMS on purpose"
        name = f"Tap{ns}x{nc}"
        _sources[ns, nc] = (name, f"""template <typename T> struct {name} {{
    static constexpr int NS = {ns}, NC = {nc}, NV = {ns + nc}, NPARAM = 0, NPATH = 0;
    EMI_DEV static void f(const ModelParams<T>&, const T* z, T, T* fo) {{
        for (int i = 0; i < NS; ++i) fo[i] = z[i];
    }}
    EMI_DEV static void jac(const ModelParams<T>&, const T* z, T, T (*J)[NV]) {{
        for (int i = 0; i < NS; ++i)
            for (int v = 0; v < NV; ++v) J[i][v] = T(0);
        for (int q = 0; q < NC; ++q) J[0][NS + q] = z[NS + q];
    }}
    EMI_DEV static T cost(const ModelParams<T>&, const T*, T) {{ return T(0); }}
    EMI_DEV static void grad(const ModelParams<T>&, const T*, T, T* g) {{
        for (int v = 0; v < NV; ++v) g[v] = T(0);
    }}
    EMI_DEV static void hess(const ModelParams<T>&, const T*, T, T, const T*, T*) {{}}
}};
""")
    return _sources[ns, nc]


def nc_of(ns, ncf, xh, uh):
    """control slots of a model written on ncf free controls with horizons (xh, uh): [U | x(t - i dt) | u(t - i dt)]"""
    return ncf + max(xh - 1, 0) * ns + uh * ncf


def slots(ns, ncf, xh, uh):
    """(source variable among [x | u_free], delay index i) of every delayed slot, in the order extend_controls lays them out"""
    out = [(st, i) for i in range(1, xh) for st in range(ns)]
    return out + [(ns + c, i) for i in range(1, uh + 1) for c in range(ncf)]


def half_length(t0, tf):
    h = (tf - t0) / 2.0
    m, _ = np.frexp(h)
    assert m == 0.5, "the taps are exact on horizons whose half-length is a power of two"
    return h


def delay_matrices(mesh, t0, tf, dt, xh, uh):
    """W [nd][M][M], W[i-1] = W(i dt), from emi_delay_matrix: the bits the context uploads"""
    from etol_amd import _lib as L
    lib = L.load()
    tau, w = (np.ascontiguousarray(a, dtype=np.float64) for a in mesh[:2])
    M, nd = len(tau), max(xh - 1, uh)
    W = np.empty((nd, M, M))
    for d in range(nd):
        assert lib.emi_delay_matrix(M, tau.ctypes.data_as(DP), w.ctypes.data_as(DP), t0, tf, (d + 1) * dt, W[d].ctypes.data_as(DP)) == 0
    return W


def row_kinds(Wi, tau, t0, tf, delay):
    """(unit, src, clamped, hit) of the rows of W(delay): unit[k] the row is a unit row, of node src[k]; clamped[k] the delayed time
    of node k is at or before t0 (formed in double as the header states it); hit[k] a unit row that is not clamped: the delayed
    time is a node's, exactly"""
    tau = np.asarray(tau, dtype=np.float64)
    hh = (tf - t0) / 2.0
    ts = t0 + hh * (tau + 1.0) - delay
    clamped = ts <= t0
    unit = ((Wi == 0.0).sum(axis=1) == Wi.shape[1] - 1) & ((Wi == 1.0).sum(axis=1) == 1)
    src = np.argmax(Wi == 1.0, axis=1)
    return unit, src, clamped, unit & ~clamped


def reference(Z, W, ns, ncf, xh, uh):
    """Z [B][ns+ncf][M] = [X | U_free]  ->  (ref [B][nd][M] float64, the long-double products rounded once; S [B][nd][M] long double,
    the magnitude sums)"""
    Zl = np.asarray(Z, dtype=np.longdouble)
    Wl = np.asarray(W, dtype=np.longdouble)
    sl = slots(ns, ncf, xh, uh)
    ref = np.empty((Z.shape[0], len(sl), Z.shape[2]))
    S = np.empty(ref.shape, dtype=np.longdouble)
    for q, (src, i) in enumerate(sl):
        ref[:, q] = (Zl[:, src] @ Wl[i - 1].T).astype(np.float64)            # [b][k] = sum_j W[k][j] z[b][j]
        S[:, q] = np.abs(Zl[:, src]) @ np.abs(Wl[i - 1]).T
    return ref, S


def bound(S, M):
    return (M + 2) * np.longdouble(U53) * S


def ratio(got, ref, S, M):
    """|got - ref| / ((M + 2) u S) elementwise, 0 where both sides of the inequality are 0, inf where only the bound is (or got is
    not finite)"""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - np.asarray(ref, dtype=np.longdouble))
    bnd = bound(S, M)
    r = np.where(err == 0, 0.0, np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), np.inf)).astype(np.float64)
    return np.where(np.isfinite(np.asarray(got, dtype=np.float64)), r, np.inf)


def same(a, b):
    """a and b hold the same doubles: equal values, no NaN (for everything but a zero's sign, which the Jacobian taps do not carry:
    the same bits)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def unit_rows_hold(got, Z, W, mesh, t0, tf, dt, ns, ncf, xh, uh):
    """(ok, clamped rows, hit rows): every delayed value of a unit row is its source's node value; the counts are over the slots"""
    ok, nclamped, nhit = True, 0, 0
    for q, (src, i) in enumerate(slots(ns, ncf, xh, uh)):
        unit, node, clamped, hit = row_kinds(W[i - 1], mesh[0], t0, tf, i * dt)
        assert (unit | ~clamped).all() and (node[clamped] == 0).all()         # a clamped row is the unit row of node 0
        ok = ok and same(got[:, q][:, unit], Z[:, src][:, node[unit]])
        nclamped += int(clamped.sum())
        nhit += int(hit.sum())
    return ok, nclamped, nhit


# ---- the cases of the delayed-value tests: the smallest shapes at which the product can still go wrong -----------------------------
# name -> ns, ncf, xh, uh, M, B, (t0, tf), dt, what the case claims to reach.  Tiles of the product kernel: 96 rows x 128 nodes, K
# tiles of 16, an unaligned instantiation for odd M.  Rows of a product: B ns (states), B ncf (controls).
#   clamp: "node0" only node 0 of W(dt) is clamped; "half" about half its rows are; "mixed" anything in between
#   later_all: from this delay index on every row is clamped (i dt >= tf - t0), 0: for no index
#   hit: rows of W(dt) whose delayed time is another node's, exactly
CASES = {
    # M = 2 (even): one instance, 3 state rows; node 1 interpolates between the two nodes
    "m2_rows3":        dict(ns=3, ncf=2, xh=2, uh=0, M=2, B=1, span=(0.0, 2.0), dt=0.5, clamp="node0", later_all=0, hit=0),
    # M = 3 on [0, 2], dt = 1: node 1 lands on t0 (clamped), node 2 on node 1 (hit); 2 dt and 3 dt reach past the horizon; one row
    "m3_hit_rows1":    dict(ns=12, ncf=1, xh=1, uh=3, M=3, B=1, span=(0.0, 2.0), dt=1.0, clamp="mixed", later_all=2, hit=1),
    # M = 17 (odd): 97 state rows, 194 control rows (three row tiles); dt half the horizon, 2 dt and 3 dt past it
    "m17_rows97":      dict(ns=1, ncf=2, xh=4, uh=2, M=17, B=97, span=(0.5, 8.5), dt=4.0, clamp="half", later_all=2, hit=1),
    # M = 127 (odd, one column tile less one): 96 state rows exactly, 144 control rows; dt below the first node spacing
    "m127_rows96":     dict(ns=2, ncf=3, xh=3, uh=1, M=127, B=48, span=(0.0, 2.0), dt=2.0 ** -12, clamp="node0", later_all=0, hit=0),
    # M = 128 (even, one column tile): 96 state rows exactly; half the rows clamped
    "m128_rows96":     dict(ns=3, ncf=2, xh=2, uh=0, M=128, B=32, span=(1.0, 9.0), dt=4.0, clamp="half", later_all=0, hit=0),
    # M = 128: 98 control rows (one row tile and two rows)
    "m128_rows98":     dict(ns=6, ncf=1, xh=0, uh=1, M=128, B=98, span=(0.0, 2.0), dt=0.37, clamp="mixed", later_all=0, hit=0),
    # M = 128: 201 state rows (three row tiles)
    "m128_rows201":    dict(ns=3, ncf=2, xh=2, uh=0, M=128, B=67, span=(0.0, 8.0), dt=0.3, clamp="mixed", later_all=0, hit=0),
    # M = 129 (odd, two column tiles): 98 state rows, 147 control rows; dt half the horizon: the last node lands on the middle one
    "m129_rows98_hit": dict(ns=2, ncf=3, xh=3, uh=1, M=129, B=49, span=(0.0, 8.0), dt=4.0, clamp="half", later_all=2, hit=1),
    # M = 257 (odd, three column tiles): one state row
    "m257_rows1":      dict(ns=1, ncf=2, xh=4, uh=2, M=257, B=1, span=(0.0, 2.0), dt=0.3, clamp="mixed", later_all=0, hit=0),
    # M = 257: 201 state rows (three row tiles) on an odd mesh
    "m257_rows201":    dict(ns=3, ncf=2, xh=2, uh=0, M=257, B=67, span=(0.0, 2.0), dt=2.0 ** -14, clamp="node0", later_all=0, hit=0),
}


def case(name, mesh_of):
    c = dict(CASES[name], name=name)
    c["t0"], c["tf"] = c["span"]
    c["h"] = half_length(c["t0"], c["tf"])
    assert c["h"] in (1.0, 4.0) and c["ns"] != c["ncf"]
    c["nc"] = nc_of(c["ns"], c["ncf"], c["xh"], c["uh"])
    assert (c["ns"], c["nc"]) in TAP_DIMS
    c["mesh"] = mesh_of(c["M"])
    c["W"] = delay_matrices(c["mesh"], c["t0"], c["tf"], c["dt"], c["xh"], c["uh"])
    c["ncalls"] = 3 if c["B"] < 3 else 2          # every kind of instance (inputs) occurs in some call
    return c


def claims_hold(c):
    """The case reaches the branches of delay_matrix it says it reaches -> (clamped rows, hit rows) of W(dt), for the report"""
    M, nd = c["M"], c["W"].shape[0]
    unit, node, clamped, hit = row_kinds(c["W"][0], c["mesh"][0], c["t0"], c["tf"], c["dt"])
    assert clamped[0] and not clamped.all() and np.array_equal(unit, clamped | hit)
    if c["clamp"] == "node0":
        assert clamped.sum() == 1
    elif c["clamp"] == "half":
        assert M // 2 <= clamped.sum() <= M // 2 + 1
    else:
        assert 1 < clamped.sum() < M
    assert hit.sum() == c["hit"] and (node[hit] > 0).all()
    for i in range(2, nd + 1):
        allc = row_kinds(c["W"][i - 1], c["mesh"][0], c["t0"], c["tf"], i * c["dt"])[2].all()
        assert allc == (c["later_all"] > 0 and i >= c["later_all"]) and allc == (i * c["dt"] >= c["tf"] - c["t0"])
        if allc:
            assert np.array_equal(c["W"][i - 1], np.eye(M)[np.zeros(M, dtype=int)])
    return int(clamped.sum()), int(hit.sum())


def inputs(c, call):
    """Z [B][ns+ncf][M] = [X | U_free] of call `call`: instance b is of kind (b + call) % 3 --
    0 smooth in time plus noise; 1 one nonzero node value per row (an indexing slip shows); 2 magnitudes from 1e-8 to 1e8"""
    B, nf, M = c["B"], c["ns"] + c["ncf"], c["M"]
    rng = np.random.default_rng(1000 * call + 7 * M + B)
    t = c["t0"] + c["h"] * (np.asarray(c["mesh"][0]) + 1.0)
    Z = np.zeros((B, nf, M))
    for b in range(B):
        kind = (b + call) % 3
        for v in range(nf):
            if kind == 0:
                Z[b, v] = (1 + 0.3 * v) * np.sin((0.4 + 0.1 * v) * t + rng.uniform(0, 3)) + 0.2 * b + 0.05 * rng.standard_normal(M)
            elif kind == 1:
                Z[b, v, (7 * v + 3 * b + call) % M] = (-1.0) ** (v + b) * (1.5 + v + 0.25 * b)
            else:
                Z[b, v] = rng.choice([-1.0, 1.0], M) * 10.0 ** rng.uniform(-8, 8, M)
                Z[b, v, rng.integers(M)], Z[b, v, rng.integers(M)] = 1e-8, 1e8
    return Z


# ---- numpy emulations of the product in plain double, in several summation orders ---------------------------------------------------
def _product_in_order(W, z, order):
    """sum_j W[k][j] z[j] in double for every k, the terms added in the order named"""
    P = W * z[None, :]                                             # every product rounded once
    M = P.shape[1]
    if order == "forward":
        acc = np.zeros(P.shape[0])
        for j in range(M):
            acc = acc + P[:, j]
        return acc
    if order == "backward":
        acc = np.zeros(P.shape[0])
        for j in range(M - 1, -1, -1):
            acc = acc + P[:, j]
        return acc
    if order in ("fours", "tiles16"):                              # partial sums of 4 (one MFMA's K) / of 16 (one K tile), then forward
        g = 4 if order == "fours" else 16
        acc = np.zeros(P.shape[0])
        for j0 in range(0, M, g):
            part = np.zeros(P.shape[0])
            for j in range(j0, min(j0 + g, M)):
                part = part + P[:, j]
            acc = acc + part
        return acc
    if order == "pairwise":
        cols = [P[:, j] for j in range(M)]
        while len(cols) > 1:
            cols = [cols[i] + cols[i + 1] if i + 1 < len(cols) else cols[i] for i in range(0, len(cols), 2)]
        return cols[0]
    raise ValueError(order)


ORDERS = ("forward", "backward", "fours", "tiles16", "pairwise")


def emulate(Z, W, ns, ncf, xh, uh, order, instances=None):
    """the delayed values [len(instances)][nd][M] by the double-precision product in `order`"""
    inst = range(Z.shape[0]) if instances is None else instances
    sl = slots(ns, ncf, xh, uh)
    out = np.empty((len(inst), len(sl), Z.shape[2]))
    for n, b in enumerate(inst):
        for q, (src, i) in enumerate(sl):
            out[n, q] = _product_in_order(W[i - 1], Z[b, src], order)
    return out


# ---- W against the Lagrange product formula at 50 digits ---------------------------------------------------------------------------
W_MESHES = (2, 3, 17, 129)
# Elementwise |W - W_exact| <= W_CONST u wt, wt as in w_ratio; the constant is the worst ratio measured against mpmath (4.66, at
# M = 129; tests/test_delay_ref_cpu.py prints it) times 4, rounded up to a power of two
W_CONST = 32.0


def w_exact(tau, t0, tf, delay, dps=50):
    """(W_exact [M][M] as mpmath numbers by the Lagrange product formula on the double tau, at the double x emi_delay_matrix forms;
    x [M]); unit rows where x is a node or the time is clamped, as the header defines"""
    import mpmath as mp
    mp.mp.dps = dps
    tau = [float(v) for v in tau]
    M = len(tau)
    hh = (tf - t0) / 2.0
    tm = [mp.mpf(v) for v in tau]
    denom = []
    for j in range(M):
        p = mp.mpf(1)
        for m in range(M):
            if m != j:
                p *= tm[j] - tm[m]
        denom.append(p)
    rows, xs = [], []
    for k in range(M):
        ts = t0 + hh * (tau[k] + 1.0) - delay
        if ts < t0:
            ts = t0
        x = (ts - t0) / hh - 1.0
        xs.append(x)
        if ts <= t0 or x in tau:
            hit = 0 if ts <= t0 else max(j for j in range(M) if tau[j] == x)
            rows.append([mp.mpf(1 if j == hit else 0) for j in range(M)])
            continue
        xm = mp.mpf(x)
        ell = mp.mpf(1)                             # l_j(x) = prod_m (x - tau_m) / ((x - tau_j) prod_(m != j) (tau_j - tau_m))
        for m in range(M):
            ell *= xm - tm[m]
        row = [ell / ((xm - tm[j]) * denom[j]) for j in range(M)]
        rows.append(row)
    return rows, xs


def w_ratio(W, tau, t0, tf, delay):
    """worst |W - W_exact| / (u wt) over the elements, wt_kj = |W_exact_kj| (1 + c_kj + sum_m |W_exact_km| c_km) with
    c_km = 1 / |x_k - tau_m|: the barycentric form divides by x - tau_m, a difference of numbers up to 1 carrying an error u, in
    the element's own term and in every term of the normalising sum.  Exact (unit) rows must agree exactly."""
    import mpmath as mp
    We, xs = w_exact(tau, t0, tf, delay)
    M = len(tau)
    assert np.isfinite(W).all()
    worst = 0.0
    for k in range(M):
        c = [1 / abs(mp.mpf(xs[k]) - mp.mpf(float(t))) if xs[k] != float(t) else mp.mpf(0) for t in tau]
        common = sum(abs(We[k][m]) * c[m] for m in range(M))
        for j in range(M):
            err = abs(mp.mpf(float(W[k, j])) - We[k][j])
            if err == 0:
                continue
            wt = abs(We[k][j]) * (1 + c[j] + common)
            assert wt > 0, (k, j)
            worst = max(worst, float(err / (mp.mpf(U53) * wt)))
    return worst
