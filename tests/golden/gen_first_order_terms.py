#!/usr/bin/env python3
"""Generates tests/golden/first_order_terms.npz: exact values and first derivatives of the three node models, entry by entry, each
with the magnitude sum of its additive terms.

For each model of gen_golden.py (model_syms: 0 point mass, 1 planar quadrotor, 2 fixed wing) and each point z of
hessian_terms.npz (read as data: its seeded batches, its edge points and its parameter sets, copied bit for bit), the file holds

  the value of e = L (term 0) and e = f_i (term 1 + i), and
  the value of de / dz_v for every (term, variable) pair whose symbolic derivative is not identically zero,

evaluated by a lambdified mpmath function at 50 digits from the doubles z and the double parameters and rounded once to double.
Beside each value stands its magnitude sum A: the sum of the absolute values of the additive terms of sympy.expand(expression),
evaluated in the same way.  For a one-term expression A = |value|.  A pair that is not stored is a structural zero.
tests/first_ref.py combines the entries with the mesh in long double and holds a kernel to a multiple of u A.

Keys, m = 0, 1, 2:
  params<m>          the model parameters              (= hessian_terms.npz)
  z<m>               [n][nv] the points                (= hessian_terms.npz)
  val<m>, mag<m>     [1 + ns][n]   L, f_0 .. f_{ns-1} and their magnitude sums
  dterm<m>, dvar<m>  [npairs] int  the (term, variable) index of each stored derivative
  dval<m>, dmag<m>   [npairs][n]
  gold_val<m>, gold_mag<m> [1 + ns][6], gold_dval<m>, gold_dmag<m> [npairs][6]: the same functions at the six points of
                     models.json (read as data), which tests/test_first_order_ref_cpu.py ties to the f, J, L, gL stored there

Nothing here imports the product or the oracle.  The archive is written with fixed time stamps: two runs give the same bytes.
Regenerate (CPU only, sympy and mpmath; a few seconds):

    python tests/golden/gen_first_order_terms.py
"""
import json
import os

import mpmath as mp
import numpy as np
import sympy as sp

from gen_golden import model_syms
from gen_hessian_terms import write_npz

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))


def magnitude(expr):
    """sum of |additive term| of the expanded expression (a sympy expression in the same symbols)"""
    return sp.Add(*[sp.Abs(t) for t in sp.Add.make_args(sp.expand(expr))])


def entry_functions(model, params):
    """-> (dterm [npairs], dvar [npairs], evaluate(z rows) -> (val, mag [1 + ns][n], dval, dmag [npairs][n]) doubles)"""
    z, p, f, L = model_syms(model)
    exprs = [L] + f
    dterm, dvar, dexprs = [], [], []
    for t, e in enumerate(exprs):
        for v, zv in enumerate(z):
            d = sp.diff(e, zv)
            if d != 0:
                dterm.append(t)
                dvar.append(v)
                dexprs.append(d)
    every = exprs + dexprs
    fn = sp.lambdify(list(z) + list(p), every + [magnitude(e) for e in every], modules="mpmath")
    par = [mp.mpf(float(v)) for v in params]
    ne, nd = len(exprs), len(dexprs)

    def evaluate(rows):
        out = np.empty((2 * (ne + nd), len(rows)))
        for n, row in enumerate(rows):
            vals = fn(*([mp.mpf(float(v)) for v in row] + par))
            out[:, n] = [float(mp.mpf(v)) for v in vals]
        val, dval, mag, dmag = out[:ne], out[ne:ne + nd], out[ne + nd:2 * ne + nd], out[2 * ne + nd:]
        assert (mag >= np.abs(val)).all() and (dmag >= np.abs(dval)).all()
        return val, mag, dval, dmag

    return np.array(dterm, dtype=np.int32), np.array(dvar, dtype=np.int32), evaluate


def main():
    golden = json.load(open(os.path.join(HERE, "models.json")))
    with np.load(os.path.join(HERE, "hessian_terms.npz")) as f:
        hess = {k: f[k] for k in f.files}
    out = {}
    for model in (0, 1, 2):
        params, zs = hess[f"params{model}"], hess[f"z{model}"]
        assert golden[str(model)]["params"] == params.tolist()
        dterm, dvar, evaluate = entry_functions(model, params)
        out[f"params{model}"], out[f"z{model}"] = params, zs
        out[f"dterm{model}"], out[f"dvar{model}"] = dterm, dvar
        out[f"val{model}"], out[f"mag{model}"], out[f"dval{model}"], out[f"dmag{model}"] = evaluate(zs)
        (out[f"gold_val{model}"], out[f"gold_mag{model}"], out[f"gold_dval{model}"],
         out[f"gold_dmag{model}"]) = evaluate([pt["z"] for pt in golden[str(model)]["points"]])
        assert out[f"params{model}"].tobytes() == hess[f"params{model}"].tobytes() and out[f"z{model}"].tobytes() == zs.tobytes()
        print(f"model {model}: {len(zs)} points, {len(dterm)} non-zero (term, variable) pairs")
    path = os.path.join(HERE, "first_order_terms.npz")
    write_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
