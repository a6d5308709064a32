"""Extended-precision references for the residual / refinement tests (tests/test_refine.py).

The matrix is rebuilt on the host from the analysis' arrays the way the plan reads them: one triangle used symmetrically
(Cholesky, LU of a symmetric input), or U by row -- with the diagonal, which the LU factorization takes from U -- plus L's
strictly lower entries by column; an entry given twice in its column counts once, with its LAST value (loadA).

Bounds (u = 2^-53 and SAFETY as in kernel_ref.py).  r_i = b_i - sum of m_i products, each product and each partial sum rounded
once (FMA), in any order, then one subtraction:
    |r^_i - r_i| <= SAFETY (m_i + 2) u w_i,      w_i = (|A| |x| + |b|)_i
and w_i itself, a sum of m_i + 1 non-negative terms, holds to (m_i + 2) u relative.  So berr = max_i |r_i| / w_i moves by at most
    FLOOR = SAFETY (max_i m_i + 2) u
and so does nerr, whose denominator |A|_1 |x|_inf + |b|_inf is no smaller than max_i w_i up to |A|_inf / |A|_1 (1 for the
symmetric cases, within SAFETY for the unsymmetric stencils used here)."""
import numpy as np

from kernel_ref import LD, U, SAFETY


def _last_of_duplicates(n, ptr, idx, val):
    """(run, idx, val) of a compressed structure with every (run, idx) pair kept once: its last occurrence"""
    ptr, idx, val = np.asarray(ptr), np.asarray(idx), np.asarray(val)
    run = np.repeat(np.arange(n), np.diff(ptr))
    key = run * n + idx
    _, first_rev = np.unique(key[::-1], return_index=True)
    keep = np.sort(len(key) - 1 - first_rev)
    return run[keep], idx[keep], val[keep]


def matrix_coo(S, Lx=None, Ux=None):
    """(rows, cols, vals) of the permuted matrix the plan holds; Lx / Ux default to the analysis' values"""
    n = S.n
    Lx = S.Lx if Lx is None else np.asarray(Lx)
    unsym = bool(getattr(S, "lu", 0)) and not bool(getattr(S, "symmetric", 1))
    c, r, v = _last_of_duplicates(n, S.Lp, S.Li, Lx)
    off = r != c
    if not unsym:
        return np.concatenate([r, c[off]]), np.concatenate([c, r[off]]), np.concatenate([v, v[off]])
    Ux = S.Ux if Ux is None else np.asarray(Ux)
    ur, uc, uv = _last_of_duplicates(n, S.Up, S.Ui, Ux)
    return np.concatenate([ur, r[off]]), np.concatenate([uc, c[off]]), np.concatenate([uv, v[off]])


def dense_ld(n, rows, cols, vals):
    """(A in longdouble, entries per row)"""
    A = np.zeros((n, n), dtype=LD)
    A[rows, cols] = np.asarray(vals, dtype=LD)
    return A, np.bincount(rows, minlength=n)


def floor(m):
    return SAFETY * (int(np.max(m)) + 2) * U if len(m) else SAFETY * 2 * U


def residual_ld(A, x, b):
    """longdouble r = b - A x, w = |A| |x| + |b|, berr = max r_i / w_i over w_i > 0, nerr = |r|_inf / (|A|_1 |x|_inf + |b|_inf)"""
    x, b = np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    r = b - A @ x
    w = np.abs(A) @ np.abs(x) + np.abs(b)
    pos = w > 0
    berr = float(np.max(np.abs(r[pos]) / w[pos])) if pos.any() else 0.0
    den = np.abs(A).sum(axis=0).max() * np.abs(x).max() + np.abs(b).max()
    nerr = float(np.abs(r).max() / den) if np.abs(r).max() > 0 else 0.0
    return r, w, berr, nerr


def host_refine(plan, A64, b, steps):
    """the hand-rolled loop (tests/test_lu_pivot.py): x = solve(b), then x += solve(b - A x) in fp64; every iterate"""
    xs = [plan.solve(b)]
    for _ in range(steps):
        xs.append(xs[-1] + plan.solve(b - A64 @ xs[-1]))
    return xs
