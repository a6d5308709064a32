"""numpy statement of the transposed solve with a supernodal LU factor, x = A^-T b, as the device runs it (sf_solve_t.hip): a
forward sweep over the U^T panels (lower, non-unit diagonal, no interchanges), then a backward sweep over the L panels with the
diagonal implied, 64-column block by block from the last to the first, each block's row interchanges undone after its
substitution.  Takes the factor in the packed layout of LUPlan.get_factor and the pivots of LUPlan.get_pivots (None: no
interchanges); b is one right-hand side (n,) or a block of them (n, k), every column on its own."""
import numpy as np
import scipy.linalg

from lu_selinv_ref import device_panels

NB = 64


def lu_solve_t(sym, Lsx, pivpos, b, panels=None):
    """panels: device_panels(sym, Lsx) when the caller has them already (several calls on one factor)"""
    Super, Lsip, Lsi = (np.asarray(getattr(sym, k)) for k in ("Super", "Lsip", "Lsi"))
    nsuper = int(sym.nsuper)
    Xp, PL, PU = panels if panels is not None else device_panels(sym, np.asarray(Lsx, dtype=np.float64))
    x = np.array(b, dtype=np.float64)
    if pivpos is not None:
        pivpos = np.asarray(pivpos)
    # (U^T)^-1: U^T(i, j) = U(j, i) is lower triangular with U's diagonal
    for s in range(nsuper):
        c0, c1 = int(Super[s]), int(Super[s + 1])
        nc, nr = c1 - c0, int(Lsip[s + 1] - Lsip[s])
        rows = Lsi[Lsip[s]:Lsip[s + 1]]
        Ut = PU[Xp[s]:Xp[s + 1]].reshape(nc, nr).T             # rows x columns
        x[c0:c1] = scipy.linalg.solve_triangular(Ut[:nc], x[c0:c1], lower=True)
        if nr > nc:
            np.subtract.at(x, rows[nc:], Ut[nc:] @ x[c0:c1])
    # L^-T with the interchanges: A^-T = P_1^T E_1^-T ... P_K^T E_K^-T U^-T, E_k = the elimination with the stored L columns of
    # 64-column block k (entries left of a block keep their old rows), P_k: x_new[pivpos[g]] = x_old[g]
    for s in range(nsuper - 1, -1, -1):
        c0, c1 = int(Super[s]), int(Super[s + 1])
        nc, nr = c1 - c0, int(Lsip[s + 1] - Lsip[s])
        rows = Lsi[Lsip[s]:Lsip[s + 1]]
        L = PL[Xp[s]:Xp[s + 1]].reshape(nc, nr).T
        y = x[c0:c1].copy()
        if nr > nc:
            y -= L[nc:].T @ x[rows[nc:]]
        for k0 in range(((nc - 1) // NB) * NB, -1, -NB):
            k1 = min(k0 + NB, nc)
            y[k0:k1] -= L[k1:nc, k0:k1].T @ y[k1:]
            D = np.tril(L[k0:k1, k0:k1], -1) + np.eye(k1 - k0)    # only the strict lower part of the stored block is L
            y[k0:k1] = scipy.linalg.solve_triangular(D.T, y[k0:k1], lower=False, unit_diagonal=True)
            if pivpos is not None:
                y[k0:k1] = y[pivpos[c0 + k0:c0 + k1] - c0]          # x_new[g] = x_old[pivpos[g]] (same block)
        x[c0:c1] = y
    return x
