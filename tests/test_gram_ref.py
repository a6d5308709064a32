"""tests/gram_ref.py against independent statements: Y^T Y over the supernodal forward sweep against B^T inv(A) B from a dense inverse
of the permuted matrix, and the block elimination of the bordered system against a dense solve of the assembled one."""
import numpy as np
import pytest

import gram_ref
from util import sf, small_cases, dense_reference_factor


def _factor(oracle, case):
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    Lsx, info, _ = oracle.chol_factorize(sym)
    assert info == 0
    return sym, Lsx


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_gram_against_dense_inverse(oracle, case):
    sym, Lsx = _factor(oracle, case)
    n = sym.n
    A, _ = dense_reference_factor(sym)
    B = np.random.default_rng(1).standard_normal((n, 5))
    G, Y = gram_ref.gram(sym, Lsx, B)
    want = B.T @ np.linalg.inv(A) @ B
    scale = np.abs(G).max()
    assert G.shape == (5, 5) and np.abs(G - want).max() <= 1e-10 * scale, float(np.abs(G - want).max() / scale)
    assert np.array_equal(G, G.T)
    # the bound's matrix dominates G entry by entry, with equality on the diagonal
    lim = gram_ref.bound(Y)
    assert np.all(np.abs(G) <= lim * (1 + 1e-13)) and np.allclose(np.diag(lim), np.diag(G), rtol=1e-13, atol=0.0)
    ok, ratio = gram_ref.within(G, G, Y, 0.0)
    assert ok and ratio == 0.0


def test_sym_matvec_against_dense():
    case = [c for c in small_cases() if c[0] == "band_500"][0]
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    A, _ = dense_reference_factor(sym)
    X = np.random.default_rng(2).standard_normal((n, 3))
    assert np.allclose(gram_ref.sym_matvec(sym, X), A @ X, rtol=1e-13, atol=1e-13 * np.abs(A @ X).max())
    assert np.allclose(gram_ref.sym_matvec(sym, X[:, 0]), A @ X[:, 0], rtol=1e-13, atol=1e-13 * np.abs(A @ X).max())


@pytest.mark.parametrize("with_C", [False, True], ids=["C=0", "C!=0"])
def test_bordered_formula_against_dense_solve(oracle, with_C):
    case = [c for c in small_cases() if c[0] == "lap3d_8_nd"][0]
    sym, Lsx = _factor(oracle, case)
    n, k = sym.n, 4
    A, _ = dense_reference_factor(sym)
    rng = np.random.default_rng(3)
    B = rng.standard_normal((n, k))
    f, g = rng.standard_normal(n), rng.standard_normal(k)
    C = None
    if with_C:
        M = rng.standard_normal((k, k))
        C = M @ M.T + np.eye(k)
    K = np.block([[A, B], [B.T, -(C if with_C else np.zeros((k, k)))]])
    want = np.linalg.solve(K, np.concatenate([f, g]))
    x, y = gram_ref.solve_bordered(sym, Lsx, B, f, g, C)
    scale = np.abs(want).max()
    assert np.abs(x - want[:n]).max() <= 1e-10 * scale and np.abs(y - want[n:]).max() <= 1e-10 * scale
    assert gram_ref.bordered_residual(sym, B, C, x, y, f, g) <= 1e-12
    assert gram_ref.bordered_residual(sym, B, C, want[:n], want[n:], f, g) <= 1e-12
