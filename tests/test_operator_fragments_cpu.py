"""emi_debug_operator_fragments (host only): De / Do of a mesh in the order the MFMA role of the one-launch pass loads them straight
into registers ("sym_dop" 2), element by element against the index formula of include/emi355x.h restated in numpy.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest


def _fragments(M, D):
    from etol_amd import _lib as L
    lib = L.load()
    D = np.ascontiguousarray(D, dtype=np.float64)
    out = np.full(2 * (M // 2) ** 2, np.nan)
    st = lib.emi_debug_operator_fragments(M, D.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
    return st, out


@pytest.mark.parametrize("M", [128, 256])
def test_fragment_order_follows_the_index_formula(built, M):
    import etol_amd as E
    D = E.lgl(M)[2]
    st, out = _fragments(M, D)
    assert st == 0 and not np.isnan(out).any()
    N, Hh, nkt = M - 1, M // 2, M // 32
    # the even / odd halves as emi_set_mesh forms them
    De = 0.5 * (D[:Hh, :Hh] + D[:Hh, N - np.arange(Hh)])
    Do = 0.5 * (D[:Hh, :Hh] - D[:Hh, N - np.arange(Hh)])
    pairs = out.reshape(Hh // 64, 4, nkt, 4, 64, 2)       # [ct][w][kt][q][lane][pair]
    ct, w, kt, q, lane = np.meshgrid(*(np.arange(n) for n in pairs.shape[:5]), indexing="ij")
    h, odd, kq, r16 = q >> 1, q & 1, lane >> 4, lane & 15
    row, col = 64 * ct + 16 * w + r16, 16 * kt + 8 * h + 2 * kq
    for k in (0, 1):
        want = np.where(odd == 0, De[row, col + k], Do[row, col + k])
        assert np.array_equal(pairs[..., k].view(np.uint64), want.view(np.uint64)), k
    # every entry of both panels exactly once: the copy is as large as De and Do together
    assert out.size == De.size + Do.size
    seen = np.zeros((2, Hh, Hh), dtype=np.int64)
    for k in (0, 1):
        np.add.at(seen, (odd, row, col + k), 1)
    assert (seen == 1).all()


def test_fragment_packing_refuses_what_the_pass_does_not_take(built):
    import etol_amd as E
    D = E.lgl(128)[2]
    assert _fragments(96, E.lgl(96)[2])[0] == 1           # not whole 128-node tiles: an argument error
    from etol_amd import _lib as L
    assert L.load().emi_debug_operator_fragments(128, None, None) == 1
    Dn = D.copy()
    Dn[3, 5] += 1.0                                       # no longer centro-antisymmetric: there are no even / odd halves
    st, out = _fragments(128, Dn)
    assert st != 0 and np.isnan(out).all()
