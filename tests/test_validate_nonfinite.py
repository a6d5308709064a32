"""The struct path's SparseFrame_validate (both host libraries) on a factor that holds a NaN: no device is involved (the pattern of
tests/test_host_solve.py: the Lsx handed to the struct is the oracle's).  The solution is then NaN in some or all rows; the residual
must be NaN, which fails every `residual <= tol`.  With fmax -- which returns its non-NaN operand -- for the four maxima, an x that
is NaN everywhere gave |r|_inf = |x|_inf = 0 and a reported residual of exactly 0.0."""
import numpy as np
import pytest

from test_host_solve import _solve
from util import sf, gen


def _chol():
    N = 8
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    perm = sf.grid_nd_perm(N, N, N)
    return n, Cp, Ci, Cx, perm, sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30)


@pytest.mark.parametrize("where", ["first_panel", "last_diagonal"])
def test_cholesky_host_validate_reports_a_nan_factor(oracle, monkeypatch, where):
    n, Cp, Ci, Cx, perm, S = _chol()
    Lsx, info, _ = oracle.chol_factorize(S)
    assert info == 0
    Lsx = np.where(oracle.lower_mask(S), Lsx, 0.0)
    res, x = _solve(sf.MatrixInfo, n, Cp, Ci, Cx, perm, True, Lsx, 1, monkeypatch)
    assert res <= 1e-13 and np.all(np.isfinite(x))
    bad = Lsx.copy()
    if where == "first_panel":
        bad[S.Lsxp[0]] = np.nan                     # the first pivot: the NaN spreads through both sweeps
    else:
        s = S.nsuper - 1
        nscol, nsrow = S.Super[s + 1] - S.Super[s], S.Lsip[s + 1] - S.Lsip[s]
        bad[S.Lsxp[s] + (nscol - 1) * nsrow + (nscol - 1)] = np.nan       # the last pivot
    res, x = _solve(sf.MatrixInfo, n, Cp, Ci, Cx, perm, True, bad, 1, monkeypatch)
    print(f"{where}: {int(np.isnan(x).sum())} of {n} entries of x are NaN, residual = {res}")
    assert np.isnan(x).any()
    assert np.isnan(res)


def test_lu_host_validate_reports_a_nan_factor(oracle, monkeypatch):
    N = 8
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, extra_per_row=0, drop=0.2, seed=4)
    perm = sf.grid_nd_perm(N, N, N, 3, 2)
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    Lsx, info, _ = oracle.lu_factorize(S)
    assert info == 0
    res, x = _solve(sf.LUMatrixInfo, n, Cp, Ci, Cx, perm, False, Lsx, 1, monkeypatch)
    assert res <= 1e-13 and np.all(np.isfinite(x))
    bad = Lsx.copy()
    bad[S.Lsxp[0]] = np.nan                         # U(0, 0) of the first panel
    res, x = _solve(sf.LUMatrixInfo, n, Cp, Ci, Cx, perm, False, bad, 1, monkeypatch)
    print(f"LU: {int(np.isnan(x).sum())} of {n} entries of x are NaN, residual = {res}")
    assert np.isnan(x).any()
    assert np.isnan(res)
