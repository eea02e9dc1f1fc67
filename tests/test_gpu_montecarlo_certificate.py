"""etol_mi355x_montecarlo with EMI_MC_CERTIFY=1: one batched certificate call per rank and mesh size.  -m gpu

At the reduced size tests/test_gpu_solve.py runs the example with (6 scenarios, 41 nodes, 4 keep-outs, 3 threads):
the .cert.csv has one line per solved scenario; everything else the program writes (the trajectory CSV files) is byte-identical
to a run without the variable; and each line matches the certificate of that scenario ALONE (a one-instance context through the
Python mirror, at full precision from the program's own inputs dump) within the bound of tests/test_gpu_certificate.py:
|G_batch - G_alone| <= 2 (M + nv + np + 2) eps T elementwise, hence stat within its maximum, comp within that times the largest
distance to a bound; defect / viol / gmax / lmax come from the same evaluation kernels and one-instance dispatch may differ from
the batch's by roundings of VALS: 5e-13 of their scale."""
import json
import os
import subprocess

import numpy as np
import pytest

import adjoint_ref as A
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(d, **extra):
    exe = os.path.join(ROOT, "etol_amd", "lib", "etol_mi355x_montecarlo")
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", EMI_MC_GATHER="1", EMI_MC_SAVE=d, **extra)
    r = subprocess.run([exe, "6", "40", "4", "3"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.strip().split("\n")


def test_montecarlo_certifies_its_solved_scenarios_in_one_batched_call(built, tmp_path):
    import etol_amd as E
    plain, cert = str(tmp_path / "plain"), str(tmp_path / "cert")
    os.makedirs(plain), os.makedirs(cert)
    lines0 = _run(plain)
    lines1 = _run(cert, EMI_MC_CERTIFY="1", EMI_MC_CERT_INPUTS=os.path.join(cert, "inputs.f64"))
    # what the program wrote before is unchanged, byte for byte; the run prints the same scenario lines up to the timing
    names = sorted(os.listdir(plain))
    assert len(names) == 12 and sorted(set(os.listdir(cert)) - {"montecarlo.cert.csv", "inputs.f64"}) == names
    for n in names:
        assert open(os.path.join(plain, n), "rb").read() == open(os.path.join(cert, n), "rb").read(), n
    strip = lambda ls: [" ".join(l.split()[:12]) for l in ls if l.startswith("scenario")]
    assert strip(lines0) == strip(lines1) and not any("certified" in l for l in lines0)
    summary = json.loads([l for l in lines1 if l.startswith('{"certified"')][-1])
    assert summary["certified"] == 6 and sum("in one call" in l for l in lines1) == 1
    rows = open(os.path.join(cert, "montecarlo.cert.csv")).read().strip().split("\n")
    assert rows[0] == "scenario,stat,comp,defect,viol,gmax,lmax" and len(rows) == 1 + 6
    table = {int(r.split(",")[0]): np.array([float(v) for v in r.split(",")[1:]]) for r in rows[1:]}
    assert sorted(table) == list(range(6))
    for q, f in enumerate(A.FIELDS):
        assert summary[f"worst_{f}"] == pytest.approx(max(t[q] for t in table.values()), rel=1e-6, abs=1e-300)
        assert table[summary[f"worst_{f}_scenario"]][q] == max(t[q] for t in table.values())
    # every scenario alone, from the inputs of the batched call
    raw = np.fromfile(os.path.join(cert, "inputs.f64"))
    B, M, ns, nc, npth = (int(v) for v in raw[:5])
    assert (B, M, ns, nc, npth) == (6, 41, 6, 2, 4)
    nv, pos, per = ns + nc, 5, []
    for b in range(B):
        sizes = [1, ns * M, nc * M, ns * M, npth * M, npth * 8]
        parts = []
        for n in sizes:
            parts.append(raw[pos:pos + n]); pos += n
        per.append(parts)
    zl, zu = raw[pos:pos + nv * M].reshape(nv, M), raw[pos + nv * M:pos + 2 * nv * M].reshape(nv, M)
    cl, cu = raw[pos + 2 * nv * M:pos + 2 * nv * M + npth], raw[pos + 2 * nv * M + npth:pos + 2 * nv * M + 2 * npth]
    assert pos + 2 * nv * M + 2 * npth == raw.size
    ev = E.Evaluator(0)
    ev.set_mesh(M, 0.0, 4.0)
    ev.set_model(E.MODEL_QUADROTOR2D, [1.0, 0.01, 9.81, 1.0, 1.0])
    ev.set_batch(1)
    for sid, X, U, lamF, lamC, recs in per:
        X, U, lamF, lamC = X.reshape(1, ns, M), U.reshape(1, nc, M), lamF.reshape(1, ns, M), lamC.reshape(1, npth, M)
        ev.set_path(recs.reshape(npth, 8), 0, 1)
        RES, VALS, _ = ev.eval_host(X, U)
        one, G = ev.kkt_certificate_host(X, U, lamF, lamC, zl, zu, cl, cu, 1.0)
        pat = A.entry_pattern(*ev.jac_structure(), ns, nc, npth, M)
        T = A.lagr_grad(VALS, lamF, lamC, 1.0, ev.D, pat, ns, nc, absolute=True)
        tol_G = float(A.bound(T, M, nv, npth).max())
        z = np.concatenate([X[0], U[0]])
        widest = max(np.where(np.abs(zl) < 1e19, np.abs(z - zl), 0.0).max(), np.where(np.abs(zu) < 1e19, np.abs(zu - z), 0.0).max())
        cmax = np.abs(RES[0, ns:]).max() + 1.0
        dscale = (np.einsum("kj,ij->ik", np.abs(ev.D), np.abs(X[0])) + np.abs(RES[0, :ns]) + 1.0).max()
        tol = [tol_G, tol_G * widest + one[0, 5] * 5e-13 * cmax, 5e-13 * dscale, 5e-13 * cmax, 5e-13 * (np.abs(VALS[0, -nv:]).max() + 1.0), 0.0]
        got = table[int(sid[0])]
        print(f"scenario {int(sid[0])}: batched {got}  alone {one[0]}")
        for q, f in enumerate(A.FIELDS):
            assert abs(got[q] - one[0, q]) <= tol[q], (int(sid[0]), f, got[q], one[0, q], tol[q])
        assert got[2] <= 1e-6 and got[3] == 0.0
    ev.close()
