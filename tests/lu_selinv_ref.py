"""numpy selected inversion of a supernodal no-pivot LU factor, with the unit decomposition, the two arenas and the addressing of
the device code (sf_selinv_lu.hip): Sigma(R,R) is read through the relative maps of the scatter problems (J, a) from
SL(r, c) = Sigma(row r, column c) when the panel position of the row is not before the column's, and from SU(r, c) = Sigma(c, r)
otherwise.  Takes the factor and returns Sigma in the packed layout of LUPlan.get_factor: per panel the full diagonal block,
Sigma(R,C), Sigma(C,R)^T."""
import numpy as np

from selinv_ref import units, unit_flops, UW  # noqa: F401  (the units are those of the Cholesky selected inversion)


def flops(sym):
    """every product of a unit once per panel set: twice the Cholesky count of the same decomposition"""
    Lsip = np.asarray(sym.Lsip)
    return sum(2.0 * unit_flops(float(Lsip[J + 1] - Lsip[J] - cb - w), float(w)) for J, cb, w in units(sym))


def device_panels(sym, Lsx):
    """packed (2 nsrow - nscol) x nscol panels -> (Xp, PL, PU): nsrow x nscol panels, PL(i,j) = L(i,j) below the diagonal (the
    diagonal block's upper part holds U11, as on the device after a download), PU(i,j) = U(j,i)"""
    Super, Lsip, Lsxp = (np.asarray(getattr(sym, k)) for k in ("Super", "Lsip", "Lsxp"))
    nsuper = int(sym.nsuper)
    ncol, nsrow = np.diff(Super), np.diff(Lsip)
    Xp = np.concatenate([[0], np.cumsum(ncol * nsrow)]).astype(np.int64)
    PL, PU = np.zeros(int(Xp[-1])), np.zeros(int(Xp[-1]))
    for s in range(nsuper):
        nc, nr = int(ncol[s]), int(nsrow[s])
        P = np.asarray(Lsx[Lsxp[s]:Lsxp[s + 1]]).reshape(nc, 2 * nr - nc).T       # rows x columns
        L = P[:nr, :].copy()
        U = np.zeros((nr, nc))
        U[:nc, :] = np.triu(P[:nc, :]).T
        U[nc:, :] = P[nr:, :]
        PL[Xp[s]:Xp[s + 1]] = L.T.ravel()
        PU[Xp[s]:Xp[s + 1]] = U.T.ravel()
    return Xp, PL, PU


def pack(sym, Xp, SL, SU):
    Super, Lsip, Lsxp = (np.asarray(getattr(sym, k)) for k in ("Super", "Lsip", "Lsxp"))
    out = np.zeros(int(sym.xsize))
    for s in range(int(sym.nsuper)):
        nc, nr = int(Super[s + 1] - Super[s]), int(Lsip[s + 1] - Lsip[s])
        A = SL[Xp[s]:Xp[s + 1]].reshape(nc, nr)           # [column][row]
        B = SU[Xp[s]:Xp[s + 1]].reshape(nc, nr)
        out[Lsxp[s]:Lsxp[s + 1]] = np.hstack([A, B[:, nc:]]).ravel()
    return out


def lu_selinv_ref(sym, Lsx):
    Super, SuperMap, Lsip, Lsi = (np.asarray(getattr(sym, k)) for k in ("Super", "SuperMap", "Lsip", "Lsi"))
    nsuper = int(sym.nsuper)
    Xp, PL, PU = device_panels(sym, np.asarray(Lsx, dtype=np.float64))
    # scatter problems (J, a): first panel row i, relative map (panel row positions in a of J's rows i ..)
    pairs = [[] for _ in range(nsuper)]
    relmap = []
    off = 0
    for s in range(nsuper):
        ncol, nsrow = int(Super[s + 1] - Super[s]), int(Lsip[s + 1] - Lsip[s])
        rows = Lsi[Lsip[s]:Lsip[s + 1]]
        i = ncol
        while i < nsrow:
            a = SuperMap[rows[i]]
            e = i
            while e < nsrow and SuperMap[rows[e]] == a:
                e += 1
            arows = Lsi[Lsip[a]:Lsip[a + 1]]
            anc = int(Super[a + 1] - Super[a])
            g = rows[i:]
            rm = np.where(np.arange(len(g)) < e - i, g - Super[a], anc + np.searchsorted(arows[anc:], g))
            relmap.append(rm)
            pairs[s].append((i, off))
            off += len(g)
            i = e
    relmap = np.concatenate(relmap) if relmap else np.zeros(0, np.int64)
    SL, SU = np.zeros(int(Xp[-1])), np.zeros(int(Xp[-1]))

    def col(J, q, ncol, nsrow):
        """(base, moff) of panel position q of J as a column of a panel set; moff None: J's own column"""
        if q < ncol:
            return Xp[J] + q * nsrow, None
        i, mo = [p for p in pairs[J] if p[0] <= q][-1]
        g = Lsi[Lsip[J] + q]
        a = SuperMap[g]
        return Xp[a] + (g - Super[a]) * (Lsip[a + 1] - Lsip[a]), mo - i

    for J, cb, w in units(sym):
        ncol, nsrow = int(Super[J + 1] - Super[J]), int(Lsip[J + 1] - Lsip[J])
        L = PL[Xp[J]:Xp[J] + ncol * nsrow].reshape(ncol, nsrow).T      # panels, rows x columns
        U = PU[Xp[J]:Xp[J] + ncol * nsrow].reshape(ncol, nsrow).T
        ce = cb + w
        m = nsrow - ce
        Tli = np.linalg.inv(np.tril(L[cb:ce, cb:ce], -1) + np.eye(w))
        Tui = np.linalg.inv(np.tril(U[cb:ce, cb:ce]))
        Yl = L[ce:, cb:ce] @ Tli
        Yu = U[ce:, cb:ce] @ Tui
        G = np.zeros((m, m))
        for y in range(m):                        # column y of G from SL and row y of G from SU, positions x >= y, through y's addressing
            base, moff = col(J, ce + y, ncol, nsrow)
            hi = np.arange(ce + y, nsrow)
            at = base + (hi if moff is None else relmap[moff + hi])
            G[y, y:] = SU[at]
            G[y:, y] = SL[at]
        Zl = G @ Yl
        Zu = G.T @ Yu
        Sc = Tui.T @ Tli + Yu.T @ Zl
        base = Xp[J]
        inside = max(0, ncol - ce)                # R rows that are J's own (later) columns: the other set's diagonal block
        for c in range(w):
            SL[base + (cb + c) * nsrow + ce: base + (cb + c + 1) * nsrow] = -Zl[:, c]
            SU[base + (cb + c) * nsrow + ce: base + (cb + c + 1) * nsrow] = -Zu[:, c]
            SU[base + (ce + np.arange(inside)) * nsrow + cb + c] = -Zl[:inside, c]
            SL[base + (ce + np.arange(inside)) * nsrow + cb + c] = -Zu[:inside, c]
        for j in range(w):
            SL[base + (cb + j) * nsrow + cb: base + (cb + j) * nsrow + ce] = Sc[:, j]
            SU[base + (cb + j) * nsrow + cb: base + (cb + j) * nsrow + ce] = Sc[j, :]
    return pack(sym, Xp, SL, SU)
