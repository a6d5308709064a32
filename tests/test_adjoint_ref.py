"""The numpy reference of the adjoints on the pattern (tests/adjoint_ref.py) against its own definition and against central finite
differences of dense numpy solve / slogdet / b^T A^-1 b in longdouble, n <= 12: the mathematics the device tests then lean on -- the
factor 2 off the diagonal of a symmetric plan, the transposed Sigma of an LU plan, the zero at positions the assembly ignores."""
import numpy as np
import pytest

import adjoint_ref as ar

LD = np.longdouble


def _structure(kind, rng, n=11):
    """a random pattern with entries given twice and (LU) diagonal positions in L: `kind` in chol / lu_alias / lu_own"""
    def side(n_):
        ptr, idx = [0], []
        for j in range(n_):
            below = [i for i in range(j + 1, n_) if rng.random() < 0.35]
            col = [j] + below
            if below and rng.random() < 0.6:
                col.insert(0, below[-1])            # given again later in the column: this copy is ignored
            if rng.random() < 0.3:
                col.insert(0, j)                    # ... and the diagonal twice
            idx += col
            ptr.append(len(idx))
        return np.array(ptr, dtype=np.int64), np.array(idx, dtype=np.int64)
    Lp, Li = side(n)
    if kind == "chol":
        return (n, Lp, Li)
    if kind == "lu_alias":
        return (n, Lp, Li, None, None)
    Up, Ui = side(n)
    return (n, Lp, Li, Up, Ui)


def _values(S, rng):
    """values of a well-conditioned M: small off the diagonal, about n on it"""
    vals = []
    for i, j, a, b in ar.marks(S):
        V = rng.uniform(-1, 1, len(i))
        V[i == j] = S[0] + rng.uniform(0, 1, int(np.count_nonzero(i == j)))
        vals.append(V.astype(LD))
    if ar.own_u(S):                                 # (the L diagonal is ignored: anything)
        vals[0][np.asarray(S[2]) == ar.columns(S[1])] = 99.0
    return vals + [None] * (2 - len(vals))


def _solve(M, B):
    """longdouble solve by Gaussian elimination with partial pivoting (numpy.linalg has no longdouble)"""
    M, B = M.astype(LD).copy(), B.astype(LD).copy()
    n = M.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
            B[[k, p]] = B[[p, k]]
        f = M[k + 1:, k] / M[k, k]
        M[k + 1:] -= np.outer(f, M[k])
        B[k + 1:] -= np.outer(f, B[k])
    for k in range(n - 1, -1, -1):
        B[k] = (B[k] - M[k, k + 1:] @ B[k + 1:]) / M[k, k]
    return B


def _logabsdet(M):
    M = M.astype(LD).copy()
    n = M.shape[0]
    s = LD(0)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        s += np.log(np.abs(M[k, k]))
        f = M[k + 1:, k] / M[k, k]
        M[k + 1:] -= np.outer(f, M[k])
    return s


KINDS = ("chol", "lu_alias", "lu_own")


@pytest.mark.parametrize("kind", KINDS)
def test_defining_identity(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    S = _structure(kind, rng)
    n = S[0]
    for k in (0, 1, 3):
        Y, X = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
        outs, sums = ar.adjoint_values(S, Y, X, 0.3)
        for _ in range(3):
            dV = [rng.uniform(-1, 1, len(o)).astype(LD) for o in outs] + [None]
            M = ar.assemble(S, dV[0], dV[1])
            want = LD(0.3) * sum(Y[:, c].astype(LD) @ M @ X[:, c].astype(LD) for c in range(k))
            got = sum((o * d).sum() for o, d in zip(outs, dV))
            assert abs(got - want) <= 1e-16 * max(1.0, float(sum(s.sum() for s in sums)))
    # a position the assembly ignores: exactly 0, and M does not depend on it
    Y, X = rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 2))
    outs, _ = ar.adjoint_values(S, Y, X)
    for o, (i, j, a, b) in zip(outs, ar.marks(S)):
        dead = ~(a | b)
        assert np.all(o[dead] == 0)
    assert sum(int(np.count_nonzero(~(a | b))) for _, _, a, b in ar.marks(S)) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_against_finite_differences(kind):
    """d/dV[p] of  <W, M^-1 B>,  <W, M^-T B> (LU),  sum_c g_c b_c^T M^-1 b_c  and  log|det M|  by central differences"""
    rng = np.random.default_rng(10 + KINDS.index(kind))
    S = _structure(kind, rng, n=9)
    n, k = S[0], 2
    VL, VU = _values(S, rng)
    B, W, g = rng.uniform(-1, 1, (n, k)).astype(LD), rng.uniform(-1, 1, (n, k)).astype(LD), rng.uniform(0.5, 1.5, k).astype(LD)

    def M_of(vals):
        return ar.assemble(S, vals[0], vals[1])

    M = M_of((VL, VU))
    X, Lam = _solve(M, B), _solve(M.T, W)
    Xt, Lamt = _solve(M.T, B), _solve(M, W)
    Sg = _solve(M, np.eye(n, dtype=LD))
    grads = {
        "solve": (lambda Mx: (W * _solve(Mx, B)).sum(), ar.adjoint_values(S, Lam, X, -1.0)[0]),
        "solve_t": (lambda Mx: (W * _solve(Mx.T, B)).sum(), ar.adjoint_values(S, Xt, Lamt, -1.0)[0]),
        "quadform": (lambda Mx: ((B * _solve(Mx, B)).sum(axis=0) * g).sum(), ar.adjoint_values(S, Xt * g, X, -1.0)[0]),
        "logdet": (lambda Mx: _logabsdet(Mx), ar.logdet_grad_values(S, Sg)),
    }
    h = LD(1e-6)
    vals = [VL, VU]
    for name, (f, outs) in grads.items():
        for side, out in enumerate(outs):
            for p in range(len(out)):
                keep = vals[side][p]
                vals[side][p] = keep + h
                up = f(M_of(vals))
                vals[side][p] = keep - h
                dn = f(M_of(vals))
                vals[side][p] = keep
                fd = (up - dn) / (2 * h)
                assert abs(fd - out[p]) <= 1e-9 * (1 + abs(out[p])), (name, side, p, float(fd), float(out[p]))
    # the symmetric factor 2: an off-diagonal position of a Cholesky structure moves two entries of M
    if kind == "chol":
        i, j, a, b = ar.marks(S)[0]
        p = int(np.flatnonzero(b)[0])
        assert abs(grads["logdet"][1][0][p] - 2 * Sg[i[p], j[p]]) <= 1e-15 * abs(Sg[i[p], j[p]])
