"""numpy reference of the adjoints on the pattern (sf_*_plan_adjoint_values, sf_*_plan_logdet_grad_values), in longdouble.

A structure is (n, Lp, Li) for a Cholesky plan, (n, Lp, Li, None, None) for an LU plan whose U aliases L, (n, Lp, Li, Up, Ui) for an
LU plan with its own U (L by columns, U by rows).  The assembly reads a position unless the same (row, column) is given again
later in its column (row of U) -- and never the diagonal positions of the L structure of an LU plan, whose diagonal is U's.

    marks(S)                    per side the two masks (a, b): position p at (i, j) feeds M(i, j) / M(j, i)
    assemble(S, VL, VU)         the dense M(V)
    adjoint_values(S, Y, X, a)  out with sum(out * dV) = a * sum_c y_c^T M(dV) x_c, and the sums of |products| of the bound
    logdet_grad_values(S, Sg, a) out with sum(out * dV) = a * tr(Sg M(dV)) for a dense Sg = A^-1
"""
import numpy as np

LD = np.longdouble


def columns(ptr):
    ptr = np.asarray(ptr, dtype=np.int64)
    return np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))


def live_positions(ptr, idx):
    """True where no later position of the same column names the same index"""
    idx = np.asarray(idx, dtype=np.int64)
    j = columns(ptr)
    live = np.ones(len(idx), dtype=bool)
    seen = set()
    for p in range(len(idx) - 1, -1, -1):
        key = (int(j[p]), int(idx[p]))
        if key in seen:
            live[p] = False
        seen.add(key)
    return live


def is_lu(S):
    return len(S) == 5


def own_u(S):
    return is_lu(S) and S[3] is not None


def marks(S):
    """[(rows, cols, a, b)] per side: L's positions, then U's of a structure with its own U.  (rows, cols) = (i, j) of the formulas:
    for U's side the position of ROW j with column c = Ui[p] is listed as (i, j) = (c, j) with the b mask (M(j, c))."""
    n, Lp, Li = S[0], np.asarray(S[1], dtype=np.int64), np.asarray(S[2], dtype=np.int64)
    j = columns(Lp)
    live = live_positions(Lp, Li)
    off = Li != j
    if not is_lu(S):
        return [(Li, j, live, live & off)]
    if not own_u(S):
        return [(Li, j, live, live & off)]          # a: M(i, j) below the diagonal and the diagonal itself (from U = the alias)
    Up, Ui = np.asarray(S[3], dtype=np.int64), np.asarray(S[4], dtype=np.int64)
    r = columns(Up)
    return [(Li, j, live & off, np.zeros(len(Li), dtype=bool)), (Ui, r, np.zeros(len(Ui), dtype=bool), live_positions(Up, Ui))]


def assemble(S, VL, VU=None, dtype=LD):
    n = S[0]
    M = np.zeros((n, n), dtype=dtype)
    vals = [VL, VU]
    for side, (i, j, a, b) in enumerate(marks(S)):
        V = np.asarray(vals[side], dtype=dtype)
        M[i[a], j[a]] = V[a]
        M[j[b], i[b]] = V[b]
    return M


def adjoint_values(S, Y, X, alpha=1.0):
    """([outL, outU?], [sumsL, sumsU?]) in longdouble; sums[p] = sum_c (|Y_ic X_jc| + |Y_jc X_ic|) over the products the position collects"""
    Y = np.asarray(Y, dtype=LD).reshape(S[0], -1)
    X = np.asarray(X, dtype=LD).reshape(S[0], -1)
    outs, sums = [], []
    for i, j, a, b in marks(S):
        ta = Y[i] * X[j]
        tb = Y[j] * X[i]
        o = ta.sum(axis=1) * a + tb.sum(axis=1) * b
        outs.append(LD(alpha) * np.where(a | b, o, LD(0)))
        sums.append(np.abs(ta).sum(axis=1) * a + np.abs(tb).sum(axis=1) * b)
    return outs, sums


def logdet_grad_values(S, Sg, alpha=1.0):
    """[outL, outU?]: d(alpha log|det M(V)|) / dV = alpha * (Sg(j, i) where V feeds M(i, j)) summed over where it feeds"""
    Sg = np.asarray(Sg, dtype=LD)
    outs = []
    for i, j, a, b in marks(S):
        outs.append(LD(alpha) * (Sg[j, i] * a + Sg[i, j] * b))
    return outs
