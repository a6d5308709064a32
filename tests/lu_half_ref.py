"""Plain-numpy statements of what sf_lu_plan_solve_half, sf_lu_plan_gram and LUPlan.schur_complement / .solve_saddle compute
(sf_gram_lu.hip), over the panels of a supernodal LU factor as the device holds them: device_panels(sym, Lsx) of the
packed layout of LUPlan.get_factor, and the pivots of LUPlan.get_pivots (None: no interchanges).

Permuted space, A = L U.  F is what the forward sweep of the solve applies: 64-column block by block, first the block's row
interchanges P_k (x_new[pivpos[g]] = x_old[g]), then the elimination E_k^-1 with the block's stored L columns (the entries left
of a block keep their old rows).  So A^-1 = U^-1 F and A^-T = F^T U^-T, and the four halves are
    "L"  F b      "U"  U^-1 b      "Ut"  U^-T b      "Lt"  F^T b
The forward halves are written out here; the transposed ones restate the two sweeps of tests/lu_trans_ref.py one at a time.
b is one right-hand side (n,) or a block (n, k), every column on its own."""
import numpy as np
import scipy.linalg

from lu_selinv_ref import device_panels

NB = 64
LD = np.longdouble


class Factor:
    """one factor, its panels unpacked once"""

    def __init__(self, sym, Lsx, pivpos=None):
        self.sym = sym
        self.Super, self.Lsip, self.Lsi = (np.asarray(getattr(sym, k)) for k in ("Super", "Lsip", "Lsi"))
        self.nsuper = int(sym.nsuper)
        self.Xp, self.PL, self.PU = device_panels(sym, np.asarray(Lsx, dtype=np.float64))
        self.piv = None if pivpos is None else np.asarray(pivpos)

    def panel(self, P, s):
        """(c0, nc, rows, the nsrow x nscol panel s of P)"""
        c0, c1 = int(self.Super[s]), int(self.Super[s + 1])
        nr = int(self.Lsip[s + 1] - self.Lsip[s])
        return c0, c1 - c0, self.Lsi[self.Lsip[s]:self.Lsip[s + 1]], P[self.Xp[s]:self.Xp[s + 1]].reshape(c1 - c0, nr).T


def half(F, b, which):
    x = np.array(b, dtype=np.float64)
    order = range(F.nsuper) if which in ("L", "Ut") else range(F.nsuper - 1, -1, -1)
    for s in order:
        if which == "L":
            # F: per 64-column block the interchanges, the unit-lower chain, then the block's columns eliminated from all rows below
            c0, nc, rows, L = F.panel(F.PL, s)
            y = x[c0:c0 + nc].copy()
            for k0 in range(0, nc, NB):
                k1 = min(k0 + NB, nc)
                if F.piv is not None:
                    moved = np.empty_like(y[k0:k1])
                    moved[F.piv[c0 + k0:c0 + k1] - c0 - k0] = y[k0:k1]          # x_new[pivpos[g]] = x_old[g] (same block)
                    y[k0:k1] = moved
                D = np.tril(L[k0:k1, k0:k1], -1) + np.eye(k1 - k0)       # only the strict lower part of the stored block is L
                y[k0:k1] = scipy.linalg.solve_triangular(D, y[k0:k1], lower=True, unit_diagonal=True)
                y[k1:] -= L[k1:nc, k0:k1] @ y[k0:k1]
                if len(rows) > nc:
                    np.subtract.at(x, rows[nc:], L[nc:, k0:k1] @ y[k0:k1])
            x[c0:c0 + nc] = y
        elif which == "U":
            # U x = y: U(C, C) = Ut[:nc]^T (upper), U(C, R) = Ut[nc:]^T
            c0, nc, rows, Ut = F.panel(F.PU, s)
            y = x[c0:c0 + nc].copy()
            if len(rows) > nc:
                y -= Ut[nc:].T @ x[rows[nc:]]
            x[c0:c0 + nc] = scipy.linalg.solve_triangular(Ut[:nc].T, y, lower=False)
        elif which == "Ut":
            c0, nc, rows, Ut = F.panel(F.PU, s)
            x[c0:c0 + nc] = scipy.linalg.solve_triangular(Ut[:nc], x[c0:c0 + nc], lower=True)
            if len(rows) > nc:
                np.subtract.at(x, rows[nc:], Ut[nc:] @ x[c0:c0 + nc])
        elif which == "Lt":
            c0, nc, rows, L = F.panel(F.PL, s)
            y = x[c0:c0 + nc].copy()
            if len(rows) > nc:
                y -= L[nc:].T @ x[rows[nc:]]
            for k0 in range(((nc - 1) // NB) * NB, -1, -NB):
                k1 = min(k0 + NB, nc)
                y[k0:k1] -= L[k1:nc, k0:k1].T @ y[k1:]
                D = np.tril(L[k0:k1, k0:k1], -1) + np.eye(k1 - k0)
                y[k0:k1] = scipy.linalg.solve_triangular(D.T, y[k0:k1], lower=False, unit_diagonal=True)
                if F.piv is not None:
                    y[k0:k1] = y[F.piv[c0 + k0:c0 + k1] - c0]             # x_new[g] = x_old[pivpos[g]]
            x[c0:c0 + nc] = y
        else:
            raise ValueError(which)
    return x


def solve(F, b, trans=False):
    return half(F, half(F, b, "Ut"), "Lt") if trans else half(F, half(F, b, "L"), "U")


def cross_gram_ref(F, C, B):
    """(G, Z, Y): Z = U^-T C, Y = F B, G = C^T A^-1 B = Z^T Y; C (n, m), B (n, k)"""
    Z = half(F, np.asarray(C, dtype=np.float64), "Ut")
    Y = half(F, np.asarray(B, dtype=np.float64), "L")
    return Z.T @ Y, Z, Y


def bound(Z, Y):
    """(|Z|^T |Y|)_ij: what a rounding error in Z, in Y or in the dot product of column i of Z and column j of Y scales with"""
    return np.abs(Z).T @ np.abs(Y)


def within(G, Gref, Z, Y, tol, extra=None):
    """the componentwise acceptance bound |G - Gref|_ij <= max(tol (|Z|^T |Y|)_ij, extra_ij), and the largest ratio seen"""
    err, lim = np.abs(np.asarray(G) - Gref), tol * bound(Z, Y)
    if extra is not None:
        lim = np.maximum(lim, extra)
    ratio = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    return bool(np.all(err <= lim)), ratio


def saddle_ref(F, B, C, f, g, D=None):
    """(x, y) of [[A, B], [C^T, -D]] [x; y] = [f; g] by block elimination: one cross_gram_ref(C, [B f]) gives S0 = C^T A^-1 B and
    t = C^T A^-1 f; (D + S0) y = t - g; x = A^-1 (f - B y)"""
    B = np.asarray(B, dtype=np.float64)
    k = B.shape[1]
    G, _, _ = cross_gram_ref(F, C, np.column_stack([B, f]))
    S, t = G[:, :k], G[:, k]
    if D is not None:
        S = S + D
    y = np.linalg.solve(S, t - g)
    return solve(F, f - B @ y), y


def saddle_matrix(A, B, C, D=None):
    """the assembled (n + k) x (n + k) matrix, dense, in the dtype of A"""
    n, k = A.shape[0], B.shape[1]
    K = np.zeros((n + k, n + k), dtype=A.dtype)
    K[:n, :n] = A
    K[:n, n:] = B
    K[n:, :n] = np.asarray(C).T
    if D is not None:
        K[n:, n:] = -np.asarray(D)
    return K


def saddle_residual(A, B, C, D, x, y, f, g):
    """|K [x; y] - [f; g]|_2 / |[f; g]|_2 in longdouble, K = the assembled system with the dense (longdouble) A"""
    K = saddle_matrix(np.asarray(A, dtype=LD), np.asarray(B, dtype=LD), np.asarray(C, dtype=LD), None if D is None else np.asarray(D, dtype=LD))
    v = np.concatenate([x, y]).astype(LD)
    r = np.concatenate([f, g]).astype(LD)
    d = K @ v - r
    return float(np.sqrt(d @ d) / np.sqrt(r @ r))
