"""CPU pins of the references the GPU tests of the transposed solves and the condition estimate lean on (tests/lu_trans_ref.py,
tests/condest_ref.py): lu_solve_t on the CPU oracle's factor against dense solves with A^T, with and without interchanges, and
the estimator with dense solves against the exact |A^-1|_1."""
import numpy as np
import pytest

from util import sf, gen, nd_perm_py
from test_lu_pivot import pivot_cases
from lu_trans_ref import lu_solve_t
from condest_ref import condest_ref, condest_cases, analyze_case, dense_permuted


def trans_cases():
    """(name, n, Cp, Ci, Cx, perm, pivot tol)"""
    c = []
    for N, seed in ((6, 5), (10, 6)):
        n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=seed)
        c.append((f"stencil_{N}", n, Cp, Ci, Cx, nd_perm_py(N, N, N), 0.0))
    for p in pivot_cases():
        if p[0] in ("dense_200_tol01", "zero_diag_12", "general_14_tol03"):
            c.append(p[:7])
    return c


@pytest.mark.parametrize("case", trans_cases(), ids=lambda c: c[0])
def test_lu_solve_t_against_dense_transposed_solve(oracle, case):
    """the acceptance of oracle.lu_solve_pivot in tests/test_lu_pivot_oracle.py, for A^T: three refinement steps (they absorb the
    growth of block-restricted pivoting), then the scaled residual is <= 1e-10.  The dense solution then differs by at most
    kappa_inf(A^T) times the two residuals."""
    name, n, Cp, Ci, Cx, perm, tol = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    if tol > 0:
        Lsx, info, pivpos, _, _ = oracle.lu_factorize_pivot(S, tol=tol)
        assert np.count_nonzero(pivpos != np.arange(n)) > 0
    else:
        Lsx, info, _ = oracle.lu_factorize(S)
        pivpos = None
    assert info == 0
    At = dense_permuted(S).T
    b = 1 + np.arange(n) / n
    x = lu_solve_t(S, Lsx, pivpos, b)
    x0 = x.copy()
    for _ in range(3):
        x = x + lu_solve_t(S, Lsx, pivpos, b - At @ x)
    scale = np.abs(At).sum(axis=0).max() * np.abs(x).max() + np.abs(b).max()
    res = np.abs(At @ x - b).max() / scale
    res0 = np.abs(At @ x0 - b).max() / scale
    print(name, "scaled residual", res0, "refined", res)
    assert res <= 1e-10, (name, res)
    want = np.linalg.solve(At, b)
    kappa = np.linalg.cond(At, np.inf)
    assert np.abs(x - want).max() <= 2e-10 * kappa * np.abs(want).max(), name
    # without interchanges the plain sweeps are backward stable on these dominant stencils: no refinement needed
    if tol == 0:
        assert res0 <= 1e-13, (name, res0)
    # and it is NOT the untransposed solve
    assert np.abs(x0 - oracle.lu_solve_pivot(S, Lsx, pivpos if pivpos is not None else np.arange(n), b)).max() > 1e-6 * np.abs(x0).max()


@pytest.mark.parametrize("case", condest_cases(), ids=lambda c: c[0])
def test_condest_ref_with_dense_solves(case):
    S = analyze_case(case)
    A = dense_permuted(S)
    n = S.n
    Ainv = np.linalg.inv(A)
    exact = np.abs(Ainv).sum(axis=0).max()
    est, solves = condest_ref(lambda v: np.linalg.solve(A, v), lambda v: np.linalg.solve(A.T, v), n)
    kappa = np.abs(A).sum(axis=0).max() * exact
    print(case[0], "exact", exact, "estimate", est, "solves", solves, "kappa_1", kappa)
    assert solves <= 11
    assert est <= exact * (1 + 100 * n * 2.0 ** -53 * kappa)       # never above by more than the solves' rounding
    assert est >= exact / 3
