"""numpy supernodal selected inversion over the analysis arrays, with the unit decomposition and the addressing of the device
code (sf_selinv.hip): Sigma(R,R) is read through the relative maps of the scatter problems (J, a), as k_build_relmaps builds them.
Returns the arena: Sigma = A^-1 on the pattern of L in the factor's layout, diagonal blocks full symmetric."""
import numpy as np

UW = 512            # sf::SEL_UW
SMALL_W, SMALL_M, SMALL_Y = 64, 512, 4096


def _levels(Super, SuperMap, Lsip, Lsi, nsuper):
    lev = np.zeros(nsuper, dtype=np.int64)
    for s in range(nsuper):
        nscol, nsrow = Super[s + 1] - Super[s], Lsip[s + 1] - Lsip[s]
        if nscol < nsrow:
            par = SuperMap[Lsi[Lsip[s] + nscol]]
            lev[par] = max(lev[par], lev[s] + 1)
    return lev


def units(sym):
    """[(J, cb, w)] in execution order: levels from the top, a level's units before the next one's; inside a supernode from its
    last unit to its first.  Narrow supernodes are one unit."""
    Super, SuperMap, Lsip, Lsi = (np.asarray(getattr(sym, k)) for k in ("Super", "SuperMap", "Lsip", "Lsi"))
    nsuper = int(sym.nsuper)
    lev = _levels(Super, SuperMap, Lsip, Lsi, nsuper)
    out = []
    for lv in range(int(lev.max()) if nsuper else -1, -1, -1):
        for s in np.nonzero(lev == lv)[0]:
            ncol, nsrow = int(Super[s + 1] - Super[s]), int(Lsip[s + 1] - Lsip[s])
            mb = nsrow - ncol
            if ncol <= SMALL_W and mb <= SMALL_M and mb * ncol <= SMALL_Y:
                out.append((int(s), 0, ncol))
                continue
            for cb in range(((ncol - 1) // UW) * UW, -1, -UW):
                out.append((int(s), cb, min(UW, ncol - cb)))
    return out


def unit_flops(m, w):
    return 2.0 * m * m * w + 2.0 * m * w * w + 2.0 / 3.0 * w ** 3


def flops(sym):
    Lsip = np.asarray(sym.Lsip)
    return sum(unit_flops(float(Lsip[J + 1] - Lsip[J] - cb - w), float(w)) for J, cb, w in units(sym))


def selinv_ref(sym, Lsx):
    Super, SuperMap, Lsip, Lsi, Lsxp = (np.asarray(getattr(sym, k)) for k in ("Super", "SuperMap", "Lsip", "Lsi", "Lsxp"))
    nsuper = int(sym.nsuper)
    Lsx = np.asarray(Lsx, dtype=np.float64)
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
    S = np.zeros(int(sym.xsize))

    def col(J, q, ncol, nsrow):
        """(base, moff) of panel position q of J as a column of Sigma; moff None: J's own column"""
        if q < ncol:
            return Lsxp[J] + q * nsrow, None
        i, mo = [p for p in pairs[J] if p[0] <= q][-1]
        g = Lsi[Lsip[J] + q]
        a = SuperMap[g]
        return Lsxp[a] + (g - Super[a]) * (Lsip[a + 1] - Lsip[a]), mo - i

    for J, cb, w in units(sym):
        ncol, nsrow = int(Super[J + 1] - Super[J]), int(Lsip[J + 1] - Lsip[J])
        P = Lsx[Lsxp[J]:Lsxp[J] + ncol * nsrow].reshape(ncol, nsrow).T      # panel, rows x columns
        ce = cb + w
        m = nsrow - ce
        Linv = np.linalg.inv(np.tril(P[cb:ce, cb:ce]))
        Y = P[ce:, cb:ce] @ Linv
        G = np.zeros((m, m))
        for y in range(m):                        # column y of Sigma(R,R), rows x >= y, through the column's addressing
            base, moff = col(J, ce + y, ncol, nsrow)
            hi = np.arange(ce + y, nsrow)
            G[y:, y] = S[base + (hi if moff is None else relmap[moff + hi])]
        G = np.tril(G) + np.tril(G, -1).T
        Z = G @ Y
        Sc = Linv.T @ Linv + Y.T @ Z
        base = Lsxp[J]
        inside = max(0, ncol - ce)                # R rows that are J's own (later) columns: mirrored above the diagonal block
        for c in range(w):
            S[base + (cb + c) * nsrow + ce: base + (cb + c + 1) * nsrow] = -Z[:, c]
            S[base + (ce + np.arange(inside)) * nsrow + cb + c] = -Z[:inside, c]
        Sfull = np.tril(Sc) + np.tril(Sc, -1).T
        for j in range(w):
            S[base + (cb + j) * nsrow + cb: base + (cb + j) * nsrow + ce] = Sfull[:, j]
    return S
