"""numpy reference and fixtures for the Newton steps of a context's whole batch (emi_kkt_*_shard_dev).

The matrix of one instance is tests/test_gpu_kkt.py's dense_kkt (imported, not copied):
    K~ = [[Q~, J^T], [J, -dc I]],   J = D (x) [I 0] + node entries,   identity rows / columns for fixed variables,
the unmodified matrix is K = K~ - sum_c delta_c u_c u_c^T with one column u_c = (vec_c at node_c, 0) per list entry, and the
verdict "K has the inertia of K~" (nv M positive, ns M negative eigenvalues) is  C = Delta^-1 - U^T K~^-1 U  positive definite.

Layouts as include/emi355x.h: Q[B][nh][M] packed lower triangles, VALS[B][nvals][M] with the ns nv Jacobian rows first,
fixed[B][nv][M] bytes; lists as emi_kkt_blocks_dev writes them: count[B], node[B][mm] (-1 behind count), delta[B][mm] and
vec[B][mm][nv] (nan behind count), ordered by node."""
import numpy as np

from test_gpu_kkt import dense_kkt


def random_blocks(D, M, ns, nv, rng):
    """One instance: random SPD node blocks, Jacobian node entries with diag D added, the initial state fixed."""
    nh = nv * (nv + 1) // 2
    Q = np.zeros((nh, M))
    for k in range(M):
        A = rng.standard_normal((nv, nv))
        Qk = A @ A.T + nv * np.eye(nv)
        for v in range(nv):
            for q in range(v + 1):
                Q[v * (v + 1) // 2 + q, k] = Qk[v, q]
    J = rng.standard_normal((ns * nv, M))
    for i in range(ns):
        J[i * nv + i] += np.diag(D)
    fixed = np.zeros((nv, M), dtype=np.uint8)
    fixed[:ns, 0] = 1
    return Q, J, fixed


def shard_blocks(D, M, ns, nv, B, seed, nvals=None):
    """B instances in the shard's layouts; VALS rows behind the Jacobian's are filled with numbers no call may read as J."""
    rng = np.random.default_rng(seed)
    nvals = ns * nv + nv if nvals is None else nvals
    Q, VALS, fixed = [], np.full((B, nvals, M), 1e30), []
    for b in range(B):
        q, j, f = random_blocks(D, M, ns, nv, rng)
        Q.append(q); fixed.append(f)
        VALS[b, :ns * nv] = j
    return dict(M=M, ns=ns, nv=nv, B=B, Q=np.array(Q), VALS=VALS, fixed=np.array(fixed), seed=seed)


def matrix(D, fx, b, dc, Q=None):
    """K~ of instance b of a fixture (Q: other node blocks than the fixture's)"""
    M, ns, nv = fx["M"], fx["ns"], fx["nv"]
    return dense_kkt(D, fx["Q"][b] if Q is None else Q, fx["VALS"][b, :ns * nv], fx["fixed"][b].reshape(-1), dc, M, ns, nv)


def columns(fx, b, node, vec, r):
    """U [N][r] of the first r list entries of an instance (entries of fixed variables are zero: their rows are the identity's)"""
    M, ns, nv = fx["M"], fx["ns"], fx["nv"]
    U = np.zeros(((nv + ns) * M, r))
    f = fx["fixed"][b].reshape(-1) != 0
    for c in range(r):
        idx = np.arange(nv) * M + node[c]
        U[idx, c] = np.where(f[idx], 0.0, vec[c])
    return U


def unmodified(Kt, U, delta):
    """K = K~ - sum delta u u^T"""
    return Kt - (U * delta) @ U.T


def verdict(Kt, U, delta):
    """(C positive definite, eigenvalues of C)"""
    if U.shape[1] == 0:
        return True, np.ones(1)
    Cm = np.diag(1.0 / delta) - U.T @ np.linalg.solve(Kt, U)
    lam = np.linalg.eigvalsh(0.5 * (Cm + Cm.T))
    return bool(lam.min() > 0.0), lam


def inertia_ok(K, M, ns, nv):
    lam = np.linalg.eigvalsh(K)
    return bool((lam > 0).sum() == nv * M and (lam < 0).sum() == ns * M)


# ---- low-rank fixtures -------------------------------------------------------------------------------------------------------
# kinds per instance: None no pairs; a number: reflected eigen-directions at every third node with delta = scale (1 + U(0, 1)) --
# the two scales of tests/test_gpu_kkt.py's low-rank test, 0.05 (K keeps the inertia) and 50 (it does not); "over": more pairs
# than max_mods (the list is cut, the count is true)
EXACT_SCALE, INEXACT_SCALE = 0.05, 50.0


def lowrank_fixture(D, M, kinds, max_mods, seed, ns=6, nv=8):
    fx = shard_blocks(D, M, ns, nv, len(kinds), seed)
    rng = np.random.default_rng(seed + 1)
    B = len(kinds)
    count = np.zeros(B, dtype=np.int32)
    node = np.full((B, max_mods), -1, dtype=np.int32)
    delta = np.full((B, max_mods), np.nan)
    vec = np.full((B, max_mods, nv), np.nan)
    for b, kind in enumerate(kinds):
        if kind is None:
            continue
        nodes = [k for k in range(M) if k % 3 == 1] if kind != "over" else list(range(1, M))
        scale = EXACT_SCALE if kind == "over" else kind
        count[b] = len(nodes)
        for c, k in enumerate(nodes[:max_mods]):
            u = rng.standard_normal(nv)
            u[fx["fixed"][b, :, k] != 0] = 0.0
            node[b, c], delta[b, c], vec[b, c] = k, scale * (1 + rng.random()), u
    fx.update(kinds=list(kinds), max_mods=max_mods, count=count, node=node, delta=delta, vec=vec)
    return fx


def expected_exact(D, fx, dc):
    """per instance: (exact as the library must report it, eigenvalues of C or None where no C is formed)"""
    out = []
    for b in range(fx["B"]):
        r = int(fx["count"][b])
        if r == 0:
            out.append((1, None))
        elif r > fx["max_mods"]:
            out.append((0, None))
        else:
            ok, lam = verdict(matrix(D, fx, b, dc), columns(fx, b, fx["node"][b], fx["vec"][b], r), fx["delta"][b, :r])
            out.append((int(ok), lam))
    return out


# the fixtures with lists that tests/test_gpu_kkt_shard.py uses (checked on the CPU by tests/test_kkt_shard_ref_cpu.py)
LR_M, LR_MAX_MODS, LR_DC = 24, 10, 1e-9
LR_VERDICTS = dict(kinds=(None, EXACT_SCALE, INEXACT_SCALE, "over"), seed=4100)          # test 4
LR_MASKS = dict(kinds=(EXACT_SCALE, EXACT_SCALE, INEXACT_SCALE), seed=4200)              # test 6


def lr_fixture(D, which):
    return lowrank_fixture(D, LR_M, which["kinds"], LR_MAX_MODS, which["seed"])


# ---- blocks with reflected eigenvalues (tests/blocks_ref.py) as a shard fixture ---------------------------------------------
BLK = dict(nv=8, ns=6, M=33, B=3, np=3, seed=977)


def blocks_fixture(D):
    """blocks_ref's "inertia" blocks without fixed variables; the Jacobian rows of VALS get diag D like every other fixture (the
    path rows of the assembly read entries behind them)"""
    import blocks_ref as R
    case = R.make_case("inertia", BLK["nv"], BLK["ns"], BLK["M"], BLK["B"], BLK["np"], BLK["seed"], fixed_patterns=False)
    nv, ns = BLK["nv"], BLK["ns"]
    for i in range(ns):
        case["VALS"][:, i * nv + i, :] += np.diag(D)
    return case


def blocks_lists_numpy(case):
    """What emi_kkt_blocks_dev records, by numpy.linalg.eigh on the scaled block: Qexact, Q~, and per instance the pairs
    (node, delta = 2 |lambda|, vec = d * eigenvector) of every scaled eigenvalue below -fl, ordered by node."""
    import blocks_ref as R
    nv, M, B = case["nv"], case["M"], case["B"]
    Qx, _ = R.assemble(case["H"], case["VALS"], case["Sigma"], case["SigT"], case["fixed"], case["dw"], case["rows"], nv)
    Qt = Qx.copy()
    il = np.tril_indices(nv)
    lists = []
    for b in range(B):
        node, delta, vec = [], [], []
        for k in range(M):
            r = R.fix_block(Qx[b, :, k], case["fixed"][b, :, k], nv)
            if r["passes"]:
                continue
            lam, W = np.linalg.eigh(r["As"])
            A = R.unpack(Qx[b, :, k], nv)
            for c in np.nonzero(lam < -R.FL)[0]:
                v = r["d"] * W[:, c]
                node.append(k); delta.append(2 * abs(lam[c])); vec.append(v)
                A = A + 2 * abs(lam[c]) * np.outer(v, v)
            Qt[b, :, k] = A[il]
        lists.append((np.array(node, dtype=np.int32), np.array(delta), np.array(vec).reshape(-1, nv)))
    return Qx, Qt, lists
