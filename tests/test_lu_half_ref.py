"""CPU pins of tests/lu_half_ref.py, the reference the GPU tests of the LU half solves and of C^T A^-1 B lean on: each half against
dense triangular and permutation algebra on the CPU oracle's factor (and pivots), the compositions against dense solves with A and
A^T, cross_gram_ref against C^T inv(A) B and the saddle elimination against a dense solve of the assembled system.

The dense statement shares nothing with the supernodal one but the factor: L and U are scattered into n x n arrays through the row
lists once, and F is applied 64-column block by block as a permutation matrix of the block and a dense unit-lower elimination."""
import numpy as np
import pytest
import scipy.linalg

import lu_half_ref as R
from condest_ref import dense_permuted
from test_lu_pivot import pivot_cases
from util import sf, gen, nd_perm_py, small_cases

NB = 64
ULP = 1.1102230246251565e-16
WHICH = ("L", "U", "Ut", "Lt")


def _dense_factor(F):
    """(L, U, blocks): n x n arrays (L strictly lower, the unit diagonal implied) and the 64-column pivot blocks [g0, g1)"""
    n = int(F.Super[-1])
    L, U, blocks = np.zeros((n, n)), np.zeros((n, n)), []
    for s in range(F.nsuper):
        c0, nc, rows, P = F.panel(F.PL, s)
        L[np.ix_(rows, np.arange(c0, c0 + nc))] = np.vstack([np.tril(P[:nc], -1), P[nc:]])
        _, _, _, Q = F.panel(F.PU, s)
        U[np.ix_(np.arange(c0, c0 + nc), rows)] = np.vstack([np.tril(Q[:nc]), Q[nc:]]).T
        blocks += [(c0 + k0, c0 + min(k0 + NB, nc)) for k0 in range(0, nc, NB)]
    return L, U, blocks


def _dense_half(L, U, blocks, piv, b, which):
    x = np.array(b, dtype=np.float64)
    if which == "U":
        return scipy.linalg.solve_triangular(U, x, lower=False)
    if which == "Ut":
        return scipy.linalg.solve_triangular(U.T, x, lower=True)
    n = L.shape[0]
    for g0, g1 in (blocks if which == "L" else blocks[::-1]):
        w = g1 - g0
        P = np.eye(w)
        if piv is not None:
            P = np.zeros((w, w))
            P[piv[g0:g1] - g0, np.arange(w)] = 1.0              # (P x)[pivpos[g]] = x[g]
        D = L[g0:g1, g0:g1] + np.eye(w)
        if which == "L":
            x[g0:g1] = scipy.linalg.solve_triangular(D, P @ x[g0:g1], lower=True, unit_diagonal=True)
            x[g1:n] -= L[g1:, g0:g1] @ x[g0:g1]
        else:
            x[g0:g1] -= L[g1:, g0:g1].T @ x[g1:n]
            x[g0:g1] = P.T @ scipy.linalg.solve_triangular(D.T, x[g0:g1], lower=False, unit_diagonal=True)
    return x


def _oracle_factor(oracle, S, tol):
    if tol > 0:
        Lsx, info, pivpos, _, _ = oracle.lu_factorize_pivot(S, tol=tol)
        assert np.count_nonzero(pivpos != np.arange(S.n)) > 0
    else:
        Lsx, info, _ = oracle.lu_factorize(S)
        pivpos = None
    assert info == 0
    return np.array(Lsx, dtype=np.float64), pivpos


def _check_halves(name, S, Lsx, piv, exact_tol):
    """every half of lu_half_ref against the dense statement.  exact_tol: the bound where nothing is ill-conditioned; None: the
    bound is max(1e-12, 8 x spread), spread = how far the DENSE statement itself moves when every entry of the factor moves by one
    ulp at random -- the yardstick of tests/test_lu_transposed.py for triangles that amplify a change of summation order"""
    F = R.Factor(S, Lsx, piv)
    L, U, blocks = _dense_factor(F)
    n = S.n
    rng = np.random.default_rng(1)
    B = rng.standard_normal((n, 3))
    for which in WHICH:
        got = R.half(F, B, which)
        want = _dense_half(L, U, blocks, piv, B, which)
        scale = np.abs(want).max(axis=0)
        err = float((np.abs(got - want).max(axis=0) / scale).max())
        bound = exact_tol
        if bound is None:
            spread = 0.0
            for _ in range(5):
                Fm = R.Factor(S, Lsx * (1.0 + rng.integers(-1, 2, Lsx.size) * ULP), piv)
                Lm, Um, _ = _dense_factor(Fm)
                spread = max(spread, float((np.abs(_dense_half(Lm, Um, blocks, piv, B, which) - want).max(axis=0) / scale).max()))
            bound = max(1e-12, 8.0 * spread)
        print(name, which, "err", err, "bound", bound)
        assert err <= bound, (name, which, err, bound)
        # one column is the first column of the block (to rounding: BLAS sums a vector and a block in different orders)
        one = R.half(F, np.ascontiguousarray(B[:, 0]), which)
        assert one.shape == (n,) and np.abs(one - got[:, 0]).max() <= max(bound, 1e-12) * scale[0], (name, which)
    # F^T is the transpose of F, whatever the interchanges
    c, b = B[:, 0], B[:, 1]
    lhs, rhs = float(c @ R.half(F, b, "L")), float(R.half(F, c, "Lt") @ b)
    assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs), np.abs(c).max() * np.abs(b).max()), (name, lhs, rhs)
    return F


def _check_compositions(name, S, F):
    """L then U is A^-1, Ut then Lt is A^-T, Z^T Y is C^T A^-1 B: 1e-10 of the largest entry of the dense result"""
    A = dense_permuted(S)
    n = S.n
    rng = np.random.default_rng(2)
    B, C = rng.standard_normal((n, 3)), rng.standard_normal((n, 2))
    for trans, M in ((False, A), (True, A.T)):
        want = np.linalg.solve(M, B)
        got = R.half(F, R.half(F, B, "Ut"), "Lt") if trans else R.half(F, R.half(F, B, "L"), "U")
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print(name, "trans" if trans else "plain", "err", err)
        assert err <= 1e-10, (name, trans, err)
        assert np.array_equal(got, R.solve(F, B, trans))
    G, Z, Y = R.cross_gram_ref(F, C, B)
    want = C.T @ np.linalg.inv(A) @ B
    err = float(np.abs(G - want).max() / np.abs(want).max())
    print(name, "cross_gram_ref err", err)
    assert G.shape == (2, 3) and err <= 1e-10, (name, err)
    assert np.array_equal(Z, R.half(F, C, "Ut")) and np.array_equal(Y, R.half(F, B, "L"))


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_small_cases_as_lu(oracle, case):
    name, n, Cp, Ci, Cx, perm, slot = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", True)
    Lsx, piv = _oracle_factor(oracle, S, 0.0)
    F = _check_halves(name, S, Lsx, piv, 1e-12)
    _check_compositions(name, S, F)


@pytest.mark.parametrize("N", [6, 10])
def test_unsymmetric_stencils(oracle, N):
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
    S = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", False)
    Lsx, piv = _oracle_factor(oracle, S, 0.0)
    F = _check_halves(f"stencil_{N}", S, Lsx, piv, 1e-12)
    _check_compositions(f"stencil_{N}", S, F)
    # and A^-T is not A^-1 here
    b = 1 + np.arange(n) / n
    assert np.abs(R.solve(F, b) - R.solve(F, b, True)).max() > 1e-6 * np.abs(R.solve(F, b)).max()


@pytest.mark.parametrize("case", pivot_cases(), ids=lambda c: c[0])
def test_pivot_cases(oracle, case):
    """the oracle's factor and pivots.  The compositions are checked through the residual of three refinement steps, which absorb the
    growth of block-restricted pivoting (the acceptance of tests/test_lu_trans_ref.py): scaled residual <= 1e-10, both directions"""
    name, n, Cp, Ci, Cx, perm, tol, _ = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    Lsx, piv = _oracle_factor(oracle, S, tol)
    F = _check_halves(name, S, Lsx, piv, None)
    A = dense_permuted(S)
    b = 1 + np.arange(n) / n
    for trans, M in ((False, A), (True, A.T)):
        x = R.solve(F, b, trans)
        for _ in range(3):
            x = x + R.solve(F, b - M @ x, trans)
        res = float(np.abs(M @ x - b).max() / (np.abs(M).sum(axis=0).max() * np.abs(x).max() + np.abs(b).max()))
        print(name, "trans" if trans else "plain", "refined scaled residual", res)
        assert res <= 1e-10, (name, trans, res)
    # the plain composition is the oracle's own pivoted solve
    xo = oracle.lu_solve_pivot(S, Lsx, piv, b)
    xr = R.solve(F, b)
    assert np.abs(xr - xo).max() <= 1e-9 * np.abs(xo).max(), name


@pytest.mark.parametrize("with_D", [False, True], ids=["D=0", "D!=0"])
def test_saddle_elimination(oracle, with_D):
    N = 6
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
    S = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", False)
    Lsx, piv = _oracle_factor(oracle, S, 0.0)
    F = R.Factor(S, Lsx, piv)
    A = dense_permuted(S)
    rng = np.random.default_rng(3)
    k = 4
    B, C = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    f, g = rng.standard_normal(n), rng.standard_normal(k)
    D = rng.standard_normal((k, k)) + 3 * np.eye(k) if with_D else None
    x, y = R.saddle_ref(F, B, C, f, g, D)
    K = R.saddle_matrix(A, B, C, D)
    want = np.linalg.solve(K, np.concatenate([f, g]))
    err = float(np.abs(np.concatenate([x, y]) - want).max() / np.abs(want).max())
    print("saddle err", err, "cond", np.linalg.cond(K))
    assert err <= 1e-10
    assert R.saddle_residual(A, B, C, D, x, y, f, g) <= 1e-12
