"""numpy reference for the node blocks of the Newton step (emi_kkt_blocks_* and the host loop of solve_nlp), by an independent
route: the same assembly, then scaling, Cholesky screen and fix with numpy.linalg.eigh on the scaled block instead of Jacobi.

Also the generator of the test blocks and the checks that the CPU test (host routine through the shim) and the GPU test (the
kernels) share -- same cases, same bounds.

Layouts as include/emi355x.h: H[B][nh][M] packed lower triangles, VALS[B][nvals][M], Sigma[B][nv][M], SigT[B][np][M],
fixed[B][nv][M] bytes; rows: per path row a list of (variable, VALS entry) pairs."""
import numpy as np

FL = 1e-9
EPS = np.finfo(np.float64).eps


def tri(v, q):
    return v * (v + 1) // 2 + q


def default_rows(ns, nv, npth, px=0, py=1):
    return [[(px, ns * nv + 2 * j), (py, ns * nv + 2 * j + 1)] for j in range(npth)]


def rows_csr(rows):
    """CSR arrays (int32) of a row list; var / entry hold at least one element so that they are never null pointers."""
    ptr, var, ent = [0], [], []
    for r in rows:
        var += [v for v, _ in r]
        ent += [e for _, e in r]
        ptr.append(len(var))
    return np.array(ptr, dtype=np.int32), np.array(var or [0], dtype=np.int32), np.array(ent or [0], dtype=np.int32)


def assemble(H, VALS, Sigma, SigT, fixed, dw, rows, nv):
    """Q[B][nh][M] in the order of the host loop, and T = sum |terms| of every entry (for the rounding bound)."""
    Q = H.copy()
    T = np.abs(H)
    for v in range(nv):
        add = Sigma[:, v, :] + np.where(fixed[:, v, :] != 0, 0.0, dw)
        Q[:, tri(v, v), :] += add
        T[:, tri(v, v), :] += np.abs(add)
    for j, row in enumerate(rows):
        for a in range(len(row)):
            for b in range(a + 1):
                hi, lo = max(row[a][0], row[b][0]), min(row[a][0], row[b][0])
                term = SigT[:, j, :] * VALS[:, row[a][1], :] * VALS[:, row[b][1], :]
                Q[:, tri(hi, lo), :] += term
                T[:, tri(hi, lo), :] += np.abs(term)
    return Q, T


def unpack(Qk, nv):
    """[nh] packed lower triangle -> full symmetric [nv][nv]"""
    A = np.zeros((nv, nv))
    il = np.tril_indices(nv)
    A[il] = Qk
    return A + np.tril(A, -1).T


def working(Qk, fx, nv):
    """The working block of one node: identity rows / columns for fixed variables, the scaling d and the scaled block."""
    A = unpack(Qk, nv)
    f = fx != 0
    A[f, :] = 0.0
    A[:, f] = 0.0
    A[f, f] = 1.0
    amax = np.abs(A).max()
    if amax == 0.0:
        amax = 1.0
    d = np.sqrt(np.maximum(np.abs(np.diag(A)), 1e-12 * amax))
    return A, d, A / np.outer(d, d)


def screen(As):
    """The Cholesky screen (row by row, a pivot <= 10 fl fails).  Returns (passes, pivots computed up to the verdict)."""
    n = As.shape[0]
    L = np.zeros((n, n))
    piv = []
    for i in range(n):
        for j in range(i + 1):
            s = As[i, j] - L[i, :j] @ L[j, :j]
            if i == j:
                piv.append(s)
                if not s > 10.0 * FL:
                    return False, piv
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    return True, piv


def fix_block(Qk, fx, nv):
    """Reference treatment of one node.  dict: passes, d, As, lam (ascending eigenvalues of the scaled block), nneg (number
    < -fl), piv."""
    A, d, As = working(Qk, fx, nv)
    ok, piv = screen(As)
    lam = np.linalg.eigvalsh(As)
    return dict(passes=ok, d=d, As=As, lam=lam, nneg=int((lam < -FL).sum()), piv=piv)


# ---- generator ---------------------------------------------------------------------------------------------------------------
KINDS = ("inertia", "late", "deficient")


def _target_block(rng, nv, kind):
    """One unscaled target block E A E.  A = L diag(s) L^T with a unit lower triangular L close to the identity: the inertia is
    that of the prescribed signs s (Sylvester), the diagonal stays near s and the scaled entries below 1 in magnitude."""
    if kind == "deficient":
        G = rng.standard_normal((nv, nv - 1))
        G /= np.linalg.norm(G, axis=1)[:, None]
        A = G @ G.T                                         # rank nv - 1, unit diagonal
        E = 10.0 ** rng.uniform(0, 1, nv)
    else:
        # 40 % pass the screen ("indefinite", for the measurements only: none does)
        nneg = 0 if kind != "indefinite" and rng.random() < 0.4 else int(rng.integers(1, nv + 1))
        s = rng.uniform(0.5, 2.0, nv)
        s[rng.permutation(nv)[:nneg]] *= -1.0
        L = np.eye(nv) + np.tril(rng.uniform(-1, 1, (nv, nv)), -1) * (0.3 / np.sqrt(nv))
        A = (L * s) @ L.T
        A = 0.5 * (A + A.T)
        E = 10.0 ** (rng.uniform(-1, 5, nv) if kind == "late" else rng.uniform(-1, 1, nv))      # late: diagonals 1e-2 .. 1e10
    return A * np.outer(E, E)


def make_case(kind, nv, ns, M, B, npth, seed, rows=None, dw=0.0, nvals=None, fixed_patterns=True):
    """Random terms whose assembled blocks are of the given kind, with fixed-variable patterns (none / one variable / the whole
    node).  Kinds "inertia" and "late" avoid the branch thresholds: a block with a scaled eigenvalue inside [-1e-6, 1e-6] or a
    screen pivot within 1e-6 relative of 10 fl is drawn again (counted: drawn, rejected)."""
    rng = np.random.default_rng(seed)
    nh = nv * (nv + 1) // 2
    nvals = ns * nv + 2 * npth + nv if nvals is None else nvals
    rows = default_rows(ns, nv, npth) if rows is None else rows
    VALS = rng.standard_normal((B, nvals, M))
    SigT = 10.0 ** rng.uniform(-3, -1 if kind == "deficient" else 2, (B, npth, M))    # (deficient: little cancellation in H)
    fixed = np.zeros((B, nv, M), dtype=np.uint8)
    pat = rng.random((B, M))
    for b in range(B):
        for k in range(M):
            if not fixed_patterns:
                continue
            if pat[b, k] < 0.15:
                fixed[b, :, k] = 1
            elif pat[b, k] < 0.40:
                fixed[b, rng.integers(nv), k] = 1
    Sigma = np.zeros((B, nv, M))
    H = np.zeros((B, nh, M))
    il = np.tril_indices(nv)
    drawn = rejected = 0
    zero = np.zeros((B, nh, M))
    for b in range(B):
        for k in range(M):
            while True:
                drawn += 1
                Tg = _target_block(rng, nv, kind)
                sg = np.where(fixed[b, :, k] != 0, 0.0, 0.9 * np.maximum(np.diag(Tg), 0.0) * (rng.random(nv) < 0.7))
                Sigma[b, :, k] = sg
                # H = target - everything else the assembly adds (so the assembled block is the target to rounding)
                one = lambda a: a[b:b + 1, :, k:k + 1]
                C, _ = assemble(one(zero), one(VALS), one(Sigma), one(SigT), one(fixed), dw, rows, nv)
                H[b, :, k] = Tg[il] - C[0, :, 0]
                if kind == "deficient":
                    break
                Qk, _ = assemble(one(H), one(VALS), one(Sigma), one(SigT), one(fixed), dw, rows, nv)
                r = fix_block(Qk[0, :, 0], fixed[b, :, k], nv)
                near = np.abs(r["lam"]).min() <= 1e-6 or any(abs(p - 10.0 * FL) <= 1e-6 * 10.0 * FL for p in r["piv"])
                if not near:
                    break
                rejected += 1
    return dict(kind=kind, nv=nv, ns=ns, M=M, B=B, np=npth, rows=rows, dw=dw, H=H, VALS=VALS, Sigma=Sigma, SigT=SigT, fixed=fixed,
                drawn=drawn, rejected=rejected, seed=seed)


# the shapes of the tests: nv = 4 (point mass), 8 (quadrotor), 16 (fixed wing); M = 33 (a tail wave, odd) and 128; B = 1 and 3;
# np = 0 and 3.  Every (kind, nv) at (33, 3, 3) and (128, 1, 0); the other two pairings at nv = 8.
MODEL_OF_NV = {4: (0, 2), 8: (1, 6), 16: (2, 12)}       # nv -> (built-in model, ns)


def case_list():
    out = []
    for ki, kind in enumerate(KINDS):
        for nv in (4, 8, 16):
            shapes = [(33, 3, 3), (128, 1, 0)] + ([(33, 1, 0), (128, 3, 3)] if nv == 8 and kind == "inertia" else [])
            for M, B, npth in shapes:
                out.append((kind, nv, M, B, npth, 1000 * ki + 100 * nv + M + 7 * B + npth))
    return out


_cases = {}


def get_case(key):
    """make_case of one entry of case_list(), made once per process"""
    if key not in _cases:
        kind, nv, M, B, npth, seed = key
        _cases[key] = make_case(kind, nv, MODEL_OF_NV[nv][1], M, B, npth, seed, dw=1e-4 if npth else 0.0)
    return _cases[key]


# ---- the checks (shared by the host-routine test and the GPU test) ---------------------------------------------------------
def check(case, out, sorted_within_node=True, log=None):
    """out: dict Qexact, Q [B][nh][M]; count [B]; node [B][mm], delta [B][mm], vec [B][mm][nv] (mm >= count); worst [B].
    Asserts the bounds of the issue; returns the measured figures."""
    nv, M, B, npth, kind = case["nv"], case["M"], case["B"], case["np"], case["kind"]
    Qref, T = assemble(case["H"], case["VALS"], case["Sigma"], case["SigT"], case["fixed"], case["dw"], case["rows"], nv)
    fig = dict(asm=0.0, fix=0.0, mineig=np.inf, delta=0.0, nfail=0, npairs=0)
    # assembly: a sum of at most np + 2 terms
    err = np.abs(out["Qexact"] - Qref)
    bound = (npth + 3) * EPS * T
    fig["asm"] = float((err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), f"assembly: {fig['asm']:.3f} of the bound"
    tol = 8 * nv * nv * EPS
    for b in range(B):
        cnt = int(out["count"][b])
        nodes = out["node"][b][:cnt]
        assert (np.diff(nodes) >= 0).all(), "list not in ascending node order"
        worst = 0.0
        total = 0
        for k in range(M):
            fx = case["fixed"][b, :, k]
            r = fix_block(out["Qexact"][b, :, k], fx, nv)
            sel = np.nonzero(nodes == k)[0]
            if r["passes"]:
                assert np.array_equal(out["Q"][b, :, k], out["Qexact"][b, :, k]), f"screen: block ({b},{k}) passes and was touched"
                assert sel.size == 0
                continue
            fig["nfail"] += 1
            # entries with a fixed variable keep their assembled value
            f = fx != 0
            Qt, Qx = unpack(out["Q"][b, :, k], nv), unpack(out["Qexact"][b, :, k], nv)
            keep = f[:, None] | f[None, :]
            assert np.array_equal(Qt[keep], Qx[keep])
            d = r["d"]
            Qts = unpack(out["Q"][b, :, k], nv)
            Qts[f, :] = 0.0
            Qts[:, f] = 0.0
            Qts[f, f] = 1.0
            Qts = Qts / np.outer(d, d)                     # the device's block in the scaling of the assembled one
            assert sel.size == r["nneg"], f"block ({b},{k}): {sel.size} pairs recorded, {r['nneg']} reference eigenvalues < -fl"
            total += sel.size
            rec = r["As"].copy()
            ray = []
            for c in sel:
                u = out["vec"][b, c] / d
                rec += out["delta"][b, c] * np.outer(u, u)
                ray.append(u @ r["As"] @ u / (u @ u))
                worst = max(worst, out["delta"][b, c] * d[0] * d[0])
            mineig = np.linalg.eigvalsh(Qts).min()
            fig["mineig"] = min(fig["mineig"], float(mineig))
            if kind == "deficient":
                assert sel.size == 0 and mineig >= FL / 2, f"deficient block ({b},{k}): smallest scaled eigenvalue {mineig:.3e}"
                continue
            e = np.abs(Qts - rec).max()
            fig["fix"] = max(fig["fix"], float(e / tol))
            assert e <= tol, f"block ({b},{k}): |Q~ - (Q + sum delta v v^T)| = {e:.3e} > {tol:.3e}"
            assert mineig >= FL * (1 - 1e-6), f"block ({b},{k}): smallest scaled eigenvalue {mineig:.3e}"
            lam_neg = r["lam"][:r["nneg"]]                 # ascending
            dl = np.sort(out["delta"][b, sel])[::-1]
            de = np.abs(dl - 2 * np.abs(lam_neg)) / (tol * (1 + 2 * np.abs(lam_neg)))
            if de.size:
                fig["delta"] = max(fig["delta"], float(de.max()))
                assert de.max() <= 1.0, f"block ({b},{k}): delta off by {de.max():.3f} of the bound"
            if sorted_within_node and sel.size > 1:
                assert (np.diff(out["delta"][b, sel]) <= tol * (1 + 2 * np.abs(lam_neg[:-1]))).all() and \
                       (np.diff(ray) >= -2 * tol * (1 + np.abs(lam_neg[:-1]))).all(), f"block ({b},{k}): pairs not in ascending eigenvalue order"
        assert cnt == total
        fig["npairs"] += total
        assert abs(out["worst"][b] - worst) <= 1e-10 * max(worst, 1e-300), (out["worst"][b], worst)
    if log is not None:
        log(f"{kind} nv={nv} M={M} B={B} np={npth}: failing blocks {fig['nfail']}, pairs {fig['npairs']}, assembly {fig['asm']:.3f} of its bound, "
            f"fix {fig['fix']:.3f}, delta {fig['delta']:.3f}, smallest scaled eigenvalue {fig['mineig']:.3e}")
    return fig
