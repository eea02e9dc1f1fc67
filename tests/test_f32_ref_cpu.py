"""The fp32 reference pieces of tests/f32_ref.py by themselves, on the CPU: the emulations of the two defect-kernel routes stay
inside every defect-row tolerance that tests/test_gpu_f32.py holds the kernels to, on the same inputs.  A failure on the GPU
then means the kernel.  Prints the measured maxima (pytest -s); DESIGN.md section 2 quotes them.  No GPU needed."""
import numpy as np
import pytest

import f32_ref as F


def test_f32_operator_rows_sum_to_zero_up_to_one_rounding(built):
    """f32_operator's own properties: f32 values, off-diagonals f32(D), and rows that sum to zero up to the diagonal's one rounding,
    which is what lets the shifted form subtract any constant.  (That the CONTEXT holds this matrix is the GPU fallback test's to
    show: its bound is derived for this operator.)"""
    for M in (2, 17, 128):
        D = F.mesh(M)[2]
        Df = F.f32_operator(D)
        assert np.array_equal(Df, Df.astype(np.float32).astype(np.float64))
        off = ~np.eye(M, dtype=bool)
        assert np.array_equal(Df[off], D.astype(np.float32).astype(np.float64)[off])
        rs = np.array([sum(Df[i, j] for j in range(M) if j != i) for i in range(M)])
        assert np.array_equal(np.diag(Df), (-rs).astype(np.float32).astype(np.float64))
        assert (np.abs(Df.sum(axis=1)) <= F.U32 * np.abs(np.diag(Df)) + 1e-12 * np.abs(Df).sum(axis=1)).all()


@pytest.mark.parametrize("M", F.FALLBACK_M)
def test_fallback_emulation_lies_within_the_derived_bound(built, M):
    D = F.mesh(M)[2]
    Df = F.f32_operator(D)
    for R in F.FALLBACK_R:
        model, B = F.ROWS[R]
        X, _, R0 = F.defect_case(model, B, M)
        ref = F.exact_defect(D, X, R0)
        err = np.abs(np.asarray(F.emulate_fallback(Df, X, R0) - ref, dtype=np.float64))
        bound = F.fallback_bound(D, X, R0)
        of_scale = (err / (F.abs_product(D, X) + 1.0)).max()
        print(f"fallback emulation M={M} R={R}: max err/bound {(err / bound).max():.3f}, {of_scale:.2e} of sum|D||x| + 1, "
              f"{(err / F.row_scale(D, X, ref)).max():.2e} of the row scale")
        assert (err <= bound).all(), (M, R, float((err / bound).max()))
        assert (bound <= F.TOL_F32 * F.row_scale(D, X, ref)).all()          # the derived bound is the tighter of the two


@pytest.mark.parametrize("M", F.SHIFTED_M)
def test_shifted_emulation_lies_within_2e_6_of_the_row_scale(built, M):
    """Sequential f32 accumulation of the shifted differences -- the least favourable order the MFMA kernels could take -- on
    every row count the GPU cases use."""
    D = F.mesh(M)[2]
    Df = F.f32_operator(D)
    for R, (model, B) in sorted(F.ROWS.items()):
        X, _, R0 = F.defect_case(model, B, M)
        ref = F.exact_defect(D, X, R0)
        err = np.abs(np.asarray(F.emulate_shifted(Df, X, R0) - ref, dtype=np.float64)) / F.row_scale(D, X, ref)
        print(f"shifted emulation M={M} R={R}: max err {err.max():.3e} of the row scale")
        assert err.max() < F.TOL_F32, (M, R, err.max())


@pytest.mark.parametrize("M", (128, 384))
def test_shifted_form_annihilates_constant_rows_exactly(built, M):
    """x_j - s is exactly 0 on a constant row, so the shifted form adds exactly 0 to R0, whatever the constant; the fallback,
    whose f32 diagonal is a rounded sum, does not (it stays within its bound)."""
    D = F.mesh(M)[2]
    Df = F.f32_operator(D)
    X = F.constant_rows(3, 12, M)
    assert (X[0, 0] == 1.0e6).all() and (X[0, 1] < 0).all()
    R0 = F.start_rows(5, X.shape)
    assert np.array_equal(F.emulate_shifted(Df, X, R0), R0)
    fb = F.emulate_fallback(Df, X, R0)
    assert not np.array_equal(fb, R0)
    assert (np.abs(np.asarray(fb - F.exact_defect(D, X, R0), dtype=np.float64)) <= F.fallback_bound(D, X, R0)).all()


@pytest.mark.parametrize("name", ("pointmass_xml", "quad_ragged", "fixedwing_64"))
def test_oracle_hessian_noise_is_far_below_the_fp32_tolerance(built, name):
    """The oracle's Hessian is a central difference of complex-step gradients.  It is linear in (sigma, lamF, lamC): the
    combination of the unit-multiplier calls that build the term scale T must reproduce the full call, and the difference --
    the oracle's own noise in the units of the fp32 Hessian test -- has to stay below a tenth of that test's 2e-6."""
    c = F.whole_pass_case(name)
    lamF, lamC = F.multipliers(c)
    Href, T = F.hessian_reference(c, lamF, lamC)
    zF, zC = np.zeros_like(lamF), np.zeros_like(lamC)
    S = F.SIGMA * F.oracle_hessian(c, zF, zC, 1.0)
    for i in range(lamF.shape[1]):
        e = zF.copy()
        e[:, i] = 1.0
        S += lamF[:, i:i + 1] * F.oracle_hessian(c, e, zC, 0.0)
    for j in range(lamC.shape[1]):
        e = zC.copy()
        e[:, j] = 1.0
        S += lamC[:, j:j + 1] * F.oracle_hessian(c, zF, e, 0.0)
    noise = (np.abs(S - Href) / (T + 1.0)).max()
    print(f"oracle Hessian {name}: linearity residual {noise:.2e} of T + 1")
    assert noise < 0.1 * F.TOL_F32
