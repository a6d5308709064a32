"""Hager's 1-norm estimator as in Higham (LAPACK xLACON) over two callables, the statement the device driver (sf_*_plan_condest,
sf_solve_t.hip) is compared with.  solve(v) = A^-1 v, solve_t(v) = A^-T v; returns (estimate of |A^-1|_1, solves used).

One deliberate difference from xLACON, shared with the device code: when a later column norm |A^-1 e_j|_1 is not larger than the
estimate so far, xLACON stops AND takes the smaller value; here the larger one is kept (both are norms of columns of A^-1, so
both are lower bounds of |A^-1|_1)."""
import numpy as np

ITMAX = 5


def _sign(v):
    return np.where(v >= 0.0, 1.0, -1.0)


def altsgn(n):
    i = np.arange(n)
    return np.where(i % 2 == 0, 1.0, -1.0) * (1.0 + i / (n - 1))


def condest_ref(solve, solve_t, n):
    solves = 1
    y = solve(np.full(n, 1.0 / n))
    est = float(np.abs(y).sum())
    if n == 1 or not np.isfinite(est):
        return est, solves
    xi = _sign(y)
    j = -1
    for it in range(1, ITMAX + 1):
        x = solve_t(xi)
        solves += 1
        jlast, j = j, int(np.argmax(np.abs(x)))                  # the first of equals
        if it > 1 and (it >= ITMAX or x[jlast] == np.abs(x[j])):
            break
        e = np.zeros(n)
        e[j] = 1.0
        y = solve(e)
        solves += 1
        nrm = float(np.abs(y).sum())
        same = bool(np.all(_sign(y) == xi))
        go_on = (not same) and nrm > est
        est = max(est, nrm) if np.isfinite(nrm) else nrm
        if not go_on:
            break
        xi = _sign(y)
    if not np.isfinite(est):
        return est, solves
    y = solve(altsgn(n))
    solves += 1
    return max(est, 2.0 * float(np.abs(y).sum()) / (3.0 * n)), solves


def condest_cases():
    """(name, method, n, Cp, Ci, Cx, perm, pivot tol) -- the matrices of tests/test_condest.py; tests/test_lu_trans_ref.py holds
    the estimator to its factor 3 on each of them with dense solves"""
    from util import sf, gen, nd_perm_py
    from test_lu_pivot import pivot_cases, _dense_csc
    c = []
    n, Cp, Ci, Cx = gen.laplacian_lower(8, 8, 8)
    c.append(("chol_lap3d_8", "chol", n, Cp, Ci, Cx, sf.grid_nd_perm(8, 8, 8), 0.0))
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(8, 8, 8, seed=5)
    c.append(("lu_stencil_8", "lu", n, Cp, Ci, Cx, nd_perm_py(8, 8, 8), 0.0))
    name, n, Cp, Ci, Cx, perm, tol, _ = [p for p in pivot_cases() if p[0] == "dense_200_tol01"][0]
    c.append((name, "lu", n, Cp, Ci, Cx, perm, tol))
    # prescribed singular values 1 .. 1e-8 between two random orthogonal factors: kappa_2 = 1e8
    rng = np.random.default_rng(17)
    Q1, _ = np.linalg.qr(rng.standard_normal((200, 200)))
    Q2, _ = np.linalg.qr(rng.standard_normal((200, 200)))
    A = (Q1 * np.logspace(0, -8, 200)) @ Q2.T
    c.append(("svd_200_kappa1e8", "lu", *_dense_csc(A), None, 0.1))
    return c


def analyze_case(case):
    from util import sf
    name, method, n, Cp, Ci, Cx, perm, tol = case
    if method == "lu":
        return sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    return sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30)


def dense_permuted(S):
    """the permuted matrix the plan holds, dense"""
    from refine_ref import matrix_coo
    r, c, v = matrix_coo(S)
    A = np.zeros((S.n, S.n))
    A[r, c] = v
    return A
