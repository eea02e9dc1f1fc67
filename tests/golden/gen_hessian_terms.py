#!/usr/bin/env python3
"""Generates tests/golden/hessian_terms.npz: exact second derivatives of the three node models, term by term.

For each model of gen_golden.py (model_syms: 0 point mass, 1 planar quadrotor, 2 fixed wing) and each seeded point z, the file holds
one value per non-zero (term, packed slot) pair: d2 e / dz_v dz_q with e = L (term 0) or f_i (term 1 + i), differentiated by sympy,
evaluated by a lambdified mpmath function at 50 digits from the doubles z and the double parameters, and rounded once to double.
Slots are those of the packed lower triangle, v (v + 1) / 2 + q with q <= v.  A pair is stored when the symbolic derivative is not
identically zero; every other pair is a structural zero.  tests/hess_ref.py combines the terms with multipliers in long double.

Keys, m = 0, 1, 2:
  params<m>   the model parameters (literals below; a CPU test holds them to etol_amd.workloads)
  z<m>        [n][nv] the points
  batch<m>    [nb][5] int: config, instances, nodes, nodes taken, first row -- the points copied from the seeded test workloads (the
              stream of etol_amd/workloads.py restated below: SplitMix64, seed 0xE70100 + 0x100 config + instance); rows after the
              last batch are the edge points listed in edge_points()
  term<m>, slot<m>  [npairs] int
  val<m>      [npairs][n]
  gold<m>     [npairs][6] the same functions at the six points of models.json (read as data), which tests/test_hessian_ref_cpu.py
              ties to the H stored there

Nothing here imports the product or the oracle.  The archive is written with fixed time stamps: two runs give the same bytes.
Regenerate (CPU only, sympy and mpmath; a few seconds):

    python tests/golden/gen_hessian_terms.py
"""
import io
import json
import os
import zipfile

import mpmath as mp
import numpy as np
import sympy as sp

from gen_golden import model_syms

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))

PARAMS = {0: [],
          1: [1.0, 0.01, 9.81, 1.0, 1.0],
          2: [10.0, 0.8, 1.1, 1.8, 9.81, 120.0, 0.3, 4.5, 0.03, 0.05, 0.08, -0.6, 0.06, 25.0, 0.9, 1.0]}
# (config, instances, nodes of the batch, nodes taken of each instance): cases pointmass_xml; quad_ragged (first four instances),
# quad_tiny and the head of quad_256; fixedwing_64 of tests/cases.py
BATCHES = {0: [(0, 2, 33, 33)], 1: [(7, 4, 50, 50), (8, 1, 2, 2), (1, 1, 256, 48)], 2: [(4, 2, 64, 64)]}


# ---- the seeded workloads, restated ------------------------------------------------------------------------------------------
def splitmix_uniform(seed, shape, lo, hi):
    """lo + (hi - lo) u, u the top 53 bits of the SplitMix64 outputs 1, 2, .. of the seed, in row-major order"""
    mask = (1 << 64) - 1
    out = np.empty(int(np.prod(shape)))
    s = seed & mask
    for i in range(out.size):
        s = (s + 0x9E3779B97F4A7C15) & mask
        x = s
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & mask
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & mask
        x ^= x >> 31
        out[i] = float(x >> 11) * (1.0 / (1 << 53))
    return (lo + (hi - lo) * out).reshape(shape)


def batch_points(model, config, B, M, take):
    """[B * take][nv]: instance-major, the first `take` nodes of each instance"""
    pts = []
    for b in range(B):
        seed = 0xE70100 + 0x100 * config + b
        if model == 0:
            u = splitmix_uniform(seed, (4, M), 0.0, 1.0)
            z = np.vstack([7.0 * u[:2], -0.5 + u[2:]])
        elif model == 1:
            u = splitmix_uniform(seed, (8, M), 0.0, 1.0)
            lo = np.array([0, 0, -np.pi / 4, -2, -2, -1.0])
            hi = np.array([10, 10, np.pi / 4, 2, 2, 1.0])
            mg = PARAMS[1][0] * PARAMS[1][2]
            z = np.vstack([lo[:, None] + (hi - lo)[:, None] * u[:6], (0.5 + u[6:7]) * mg, -0.1 + 0.2 * u[7:8]])
        else:
            u = splitmix_uniform(seed, (16, M), -1.0, 1.0)
            sx = np.array([100, 100, 50, 0.4, 0.3, 3.0, 25, 2, 2, 0.5, 0.5, 0.5])
            ox = np.array([0, 0, -100, 0, 0, 0, 25, 0, 0, 0, 0, 0.0])
            su = np.array([20, 0.3, 0.3, 0.3])
            ou = np.array([30, 0, 0, 0.0])
            scale = np.where(np.arange(12)[:, None] == 6, 0.2, 1.0)
            z = np.vstack([ox[:, None] + sx[:, None] * u[:12] * scale, ou[:, None] + su[:, None] * u[12:]])
        pts.append(z.T[:take])
    return np.vstack(pts)


def edge_points(model, base):
    """Copies of the first seeded points with one coordinate moved to an edge"""
    def moved(row, **kw):
        z = base[row].copy()
        for k, v in kw.items():
            z[int(k[1:])] = v
        return z

    if model == 0:
        return [moved(0, v2=-0.0), moved(1, v2=0.0, v3=-0.0), moved(2, v0=0.0, v1=0.0)]
    if model == 1:
        # pitch beyond +-pi (argument reduction of sin / cos), zero thrust, negative-zero controls
        th = [3.5, -3.5, 6.5, -6.5, 25.0, -40.0, 1000.0, -1000.0]
        return ([moved(i, v2=t) for i, t in enumerate(th)] +
                [moved(8, v6=0.0), moved(9, v6=-0.0), moved(10, v7=-0.0), moved(11, v2=0.0), moved(12, v2=-0.0, v6=0.0)])
    # fixed wing: pitch +-1.2 (1 / cos^2 and tan grow), roll and yaw beyond +-pi, zero thrust, negative-zero surfaces
    return [moved(0, v4=1.2), moved(1, v4=-1.2), moved(2, v4=1.2, v3=-0.4), moved(3, v4=-1.2, v5=3.0),
            moved(4, v3=3.5, v5=-7.0), moved(5, v3=-9.0, v5=40.0), moved(6, v12=0.0), moved(7, v13=-0.0, v14=-0.0, v15=-0.0),
            moved(8, v4=0.0), moved(9, v9=0.0, v10=0.0, v11=0.0)]


# ---- exact terms -------------------------------------------------------------------------------------------------------------
def term_functions(model):
    """-> (term [npairs], slot [npairs], evaluate(z rows) -> [npairs][n] doubles)"""
    z, p, f, L = model_syms(model)
    nv = len(z)
    term, slot, exprs = [], [], []
    for t, e in enumerate([L] + f):
        for v in range(nv):
            for q in range(v + 1):
                d = sp.diff(e, z[v], z[q])
                if d != 0:
                    term.append(t)
                    slot.append(v * (v + 1) // 2 + q)
                    exprs.append(d)
    fn = sp.lambdify(list(z) + list(p), exprs, modules="mpmath")
    par = [mp.mpf(float(v)) for v in PARAMS[model]]

    def evaluate(rows):
        out = np.empty((len(exprs), len(rows)))
        for n, row in enumerate(rows):
            vals = fn(*([mp.mpf(float(v)) for v in row] + par))
            out[:, n] = [float(mp.mpf(v)) for v in vals]
        return out

    return np.array(term, dtype=np.int32), np.array(slot, dtype=np.int32), evaluate


def write_npz(path, arrays):
    """an uncompressed .npz with fixed member time stamps (numpy.load reads it like any other)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    golden = json.load(open(os.path.join(HERE, "models.json")))
    out = {}
    for model in (0, 1, 2):
        rows, table, first = [], [], 0
        for config, B, M, take in BATCHES[model]:
            pts = batch_points(model, config, B, M, take)
            table.append((config, B, M, take, first))
            first += len(pts)
            rows.append(pts)
        base = rows[0]
        rows.append(np.array(edge_points(model, base)))
        zs = np.vstack(rows)
        term, slot, evaluate = term_functions(model)
        assert golden[str(model)]["params"] == PARAMS[model]
        out[f"params{model}"] = np.array(PARAMS[model], dtype=np.float64)
        out[f"z{model}"] = zs
        out[f"batch{model}"] = np.array(table, dtype=np.int32)
        out[f"term{model}"], out[f"slot{model}"] = term, slot
        out[f"val{model}"] = evaluate(zs)
        out[f"gold{model}"] = evaluate([pt["z"] for pt in golden[str(model)]["points"]])
        print(f"model {model}: {len(zs)} points, {len(term)} non-zero (term, slot) pairs in {len(set(slot.tolist()))} slots")
    assert len(out["term2"]) == 74 and len(set(out["slot2"].tolist())) == 32
    path = os.path.join(HERE, "hessian_terms.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
