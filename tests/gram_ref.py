"""Plain-numpy statements of what sf_chol_plan_gram (sf_gram.hip) and CholPlan.schur / .solve_bordered compute, over the supernodal
half solve of tests/sample_ref.py: with A = L L^T (permuted space) and Y = L^-1 B,  G = B^T A^-1 B = Y^T Y."""
import numpy as np

import sample_ref


def gram(sym, Lsx, B):
    """(G, Y): Y = L^-1 B by the numpy forward sweep over the factor Lsx (reference layout), G = Y^T Y; B of shape (n, k)"""
    Y = sample_ref.half_solve(sym, Lsx, np.asarray(B, dtype=np.float64), "L")
    return Y.T @ Y, Y


def bound(Y):
    """(|Y|^T |Y|)_ij: what a rounding error in Y or in the dot product of its columns i and j scales with"""
    Ya = np.abs(Y)
    return Ya.T @ Ya


def within(G, Gref, Y, tol):
    """the componentwise acceptance bound |G - Gref|_ij <= tol (|Y|^T |Y|)_ij, and the largest ratio seen (for messages)"""
    err, lim = np.abs(np.asarray(G) - Gref), bound(Y)
    ratio = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    return bool(np.all(err <= tol * lim)), ratio


def solve(sym, Lsx, b):
    """A^-1 b: the two half sweeps one after the other"""
    return sample_ref.half_solve(sym, Lsx, sample_ref.half_solve(sym, Lsx, b, "L"), "Lt")


def solve_bordered(sym, Lsx, B, f, g, C=None):
    """(x, y) of [[A, B], [B^T, -C]] [x; y] = [f; g] by block elimination: one Gram matrix of [B f] gives S0 = B^T A^-1 B and
    t = B^T A^-1 f; (C + S0) y = t - g; x = A^-1 (f - B y)"""
    B = np.asarray(B, dtype=np.float64)
    k = B.shape[1]
    G, _ = gram(sym, Lsx, np.column_stack([B, f]))
    S, t = G[:k, :k], G[:k, k]
    if C is not None:
        S = S + C
    y = np.linalg.solve(S, t - g)
    return solve(sym, Lsx, f - B @ y), y


def sym_matvec(sym, X):
    """A X for the permuted matrix whose lower triangle is the CSC (Lp, Li, Lx) of `sym`; X of shape (n,) or (n, k)"""
    g = (lambda key: sym[key]) if isinstance(sym, dict) else (lambda key: getattr(sym, key))
    Lp, Li, Lx = (np.asarray(g(key)) for key in ("Lp", "Li", "Lx"))
    n = len(Lp) - 1
    X = np.asarray(X, dtype=np.float64)
    cols = np.repeat(np.arange(n), np.diff(Lp))
    V = Lx.reshape((-1,) + (1,) * (X.ndim - 1))
    out = np.zeros_like(X)
    np.add.at(out, Li, V * X[cols])
    off = Li != cols
    np.add.at(out, cols[off], V[off] * X[Li[off]])
    return out


def bordered_residual(sym, B, C, x, y, f, g):
    """|[[A, B], [B^T, -C]] [x; y] - [f; g]|_2 / |[f; g]|_2"""
    r1 = sym_matvec(sym, x) + B @ y - f
    r2 = B.T @ x - (C @ y if C is not None else 0.0) - g
    return float(np.sqrt(r1 @ r1 + r2 @ r2) / np.sqrt(f @ f + g @ g))
