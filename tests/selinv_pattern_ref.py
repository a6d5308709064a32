"""numpy restatement of sf_*_plan_selinv_values / _trace / _entries (sf_selinv_pattern.hip) over the analysis arrays: where
every entry of the structure a plan was created with sits in the selected inverse as get_selinv() returns it -- the factor's layout
for a Cholesky plan (selinv_ref), get_factor's packed layout for an LU plan (lu_selinv_ref) -- and what the three entry points
make of it.  Everything is in permuted space."""
import numpy as np


def _arr(sym, *names):
    return (np.asarray(getattr(sym, k)) for k in names)


def positions(sym, Lp, Li):
    """(s, c, r, found) per entry p of the by-column structure (Lp, Li): supernode of its column j, column inside the panel, panel
    row of Li[p] (inside the supernode: its column offset; below: nscol + its place in the row list), and whether that row is
    there -- the walk of k_build_loadmap with no entry left out"""
    Super, SuperMap, Lsip, Lsi = _arr(sym, "Super", "SuperMap", "Lsip", "Lsi")
    Lp, Li = np.asarray(Lp), np.asarray(Li)
    j = np.repeat(np.arange(len(Lp) - 1), np.diff(Lp))
    return _locate(Super, SuperMap, Lsip, Lsi, Li, j)


def _locate(Super, SuperMap, Lsip, Lsi, i, j):
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    s = SuperMap[j].astype(np.int64) if len(j) else np.zeros(0, np.int64)
    nscol = Super[s + 1] - Super[s]
    c = j - Super[s]
    r = i - Super[s]
    # the rows below of all supernodes as one ascending list of keys (supernode, row): one search for every entry
    nsuper, n = len(Super) - 1, int(Super[-1])
    ncol_all = np.diff(Super)
    sid = np.repeat(np.arange(nsuper), np.diff(Lsip) - ncol_all)
    pos = np.arange(len(Lsi))
    is_below = pos - np.repeat(Lsip[:-1], np.diff(Lsip)) >= np.repeat(ncol_all, np.diff(Lsip))
    keys = sid * (n + 1) + Lsi[is_below]
    start = np.concatenate([[0], np.cumsum(np.diff(Lsip) - ncol_all)])
    below = i >= Super[s + 1]
    b = np.searchsorted(keys, s * (n + 1) + i)
    hit = (b < len(keys)) & (keys[np.minimum(b, max(len(keys) - 1, 0))] == s * (n + 1) + i) if len(keys) else np.zeros(len(i), dtype=bool)
    found = ~below | hit
    r = np.where(below, nscol + b - start[s], r)
    return s, c, r, found


def live_mask(Lp, Li, skip_diag=False):
    """the entries the assembly loads: of several entries of one column with the same row the last one; skip_diag: not the diagonal
    (the L structure of an LU plan)"""
    Lp, Li = np.asarray(Lp), np.asarray(Li, dtype=np.int64)
    j = np.repeat(np.arange(len(Lp) - 1), np.diff(Lp))
    key = j * (len(Lp) + int(Li.max(initial=0)) + 1) + Li
    order = np.argsort(key, kind="stable")              # equal (column, row) pairs stay in position order
    last = np.ones(len(Li), dtype=bool)
    last[:-1] = key[order][1:] != key[order][:-1]
    live = np.zeros(len(Li), dtype=bool)
    live[order] = last
    return live & (Li != j) if skip_diag else live


def chol_offsets(sym, Lp, Li):
    """offset in the arena (the factor's layout) of Sigma(Li[p], j) for every entry"""
    Lsip, Lsxp = _arr(sym, "Lsip", "Lsxp")
    s, c, r, found = positions(sym, Lp, Li)
    assert np.all(found)
    return Lsxp[s] + c * (Lsip[s + 1] - Lsip[s]) + r


def _lu_offsets(sym, s, c, r):
    """(offset of Sigma(row of r, column c), offset of Sigma(column c, row of r)) in the packed layout of LUPlan.get_selinv: per
    panel, (2 nsrow - nscol) x nscol column-major, the full diagonal block, Sigma(R,C), Sigma(C,R)^T"""
    Super, Lsip, Lsxp = _arr(sym, "Super", "Lsip", "Lsxp")
    nscol, nsrow = Super[s + 1] - Super[s], Lsip[s + 1] - Lsip[s]
    lda = 2 * nsrow - nscol
    direct = Lsxp[s] + c * lda + r
    inside = r < nscol
    trans = np.where(inside, Lsxp[s] + np.where(inside, r, 0) * lda + c, Lsxp[s] + c * lda + nsrow + (r - nscol))
    return direct, trans


def lu_offsets(sym, Lp, Li):
    s, c, r, found = positions(sym, Lp, Li)
    assert np.all(found)
    return _lu_offsets(sym, s, c, r)


def chol_values(sym, S, Lp=None, Li=None):
    """what CholPlan.selinv_values() returns, gathered on the host out of get_selinv()"""
    Lp, Li = (sym.Lp, sym.Li) if Lp is None else (Lp, Li)
    return np.asarray(S)[chol_offsets(sym, Lp, Li)]


def lu_values(sym, S, aliased, transposed=False, Lp=None, Li=None, Up=None, Ui=None):
    """what LUPlan.selinv_values(transposed) returns: (SL, SU), SU None when U aliases L.  SL[p] = Sigma(Li[p], j),
    SU[p] = Sigma(j, Ui[p]); transposed: Sigma(j, Li[p]) and Sigma(Ui[p], j)"""
    S = np.asarray(S)
    Lp, Li = (sym.Lp, sym.Li) if Lp is None else (Lp, Li)
    d, t = lu_offsets(sym, Lp, Li)
    SL = S[t if transposed else d]
    if aliased:
        return SL, None
    Up, Ui = (sym.Up, sym.Ui) if Up is None else (Up, Ui)
    d, t = lu_offsets(sym, Up, Ui)          # (row j of U walks column j of the U^T panels: `direct` is then Sigma(Ui[p], j))
    return SL, S[d if transposed else t]


def _cols(V, rows):
    V = np.asarray(V, dtype=np.float64)
    V = V.reshape(rows, -1) if V.ndim == 1 else V
    assert V.shape[0] == rows
    return V


def chol_trace_terms(sym, S, V, Lp=None, Li=None):
    """the products whose sum is tr(Sigma M(V_t)), one row per live entry, one column per t: Sigma_jj V_jj on the diagonal,
    2 Sigma_ij V_ij off it"""
    Lp, Li = (sym.Lp, sym.Li) if Lp is None else (Lp, Li)
    Lp, Li = np.asarray(Lp), np.asarray(Li)
    V = _cols(V, len(Li))
    j = np.repeat(np.arange(len(Lp) - 1), np.diff(Lp))
    w = np.where(Li == j, 1.0, 2.0)
    live = live_mask(Lp, Li)
    sig = chol_values(sym, S, Lp, Li)
    return ((w * sig)[:, None] * V)[live]


def lu_trace_terms(sym, S, aliased, VL, VU=None, Lp=None, Li=None, Up=None, Ui=None):
    """the products of tr(Sigma M) = sum_ij Sigma(j, i) M_ij: every live L entry (the diagonal is not one) with the transposed
    Sigma at its position, every live U entry likewise; U aliasing L: the structure of L once more, diagonal included, VL's values"""
    Lp, Li = (sym.Lp, sym.Li) if Lp is None else (Lp, Li)
    VL = _cols(VL, len(np.asarray(Li)))
    tL, tU = lu_values(sym, S, aliased, True, Lp, Li, Up, Ui)
    terms = [(tL[:, None] * VL)[live_mask(Lp, Li, skip_diag=True)]]
    if aliased:
        dL, _ = lu_values(sym, S, True, False, Lp, Li)
        terms.append((dL[:, None] * VL)[live_mask(Lp, Li)])
    else:
        Up, Ui = (sym.Up, sym.Ui) if Up is None else (Up, Ui)
        VU = _cols(VU, len(np.asarray(Ui)))
        terms.append((tU[:, None] * VU)[live_mask(Up, Ui)])
    return np.vstack(terms)


def mapped_columns(vmap, A):
    """the value arrays a mapped call reads: V[p] = A[vmap[p]], 0 where the map has -1"""
    vmap = np.asarray(vmap)
    A = np.asarray(A, dtype=np.float64)
    A = A.reshape(len(A), -1)
    return np.where((vmap >= 0)[:, None], A[np.maximum(vmap, 0)], 0.0)


def entries(sym, S, rows, cols, lu=False):
    """(values, outside) of selinv_entries: Sigma(rows[k], cols[k]); NaN and counted where the pair is outside the pattern"""
    Super, SuperMap, Lsip, Lsi, Lsxp = _arr(sym, "Super", "SuperMap", "Lsip", "Lsi", "Lsxp")
    S = np.asarray(S)
    i, j = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    s, c, r, found = _locate(Super, SuperMap, Lsip, Lsi, hi, lo)
    r = np.where(found, r, 0)
    if lu:
        d, t = _lu_offsets(sym, s, c, r)
        off = np.where(i >= j, d, t)
    else:
        off = Lsxp[s] + c * (Lsip[s + 1] - Lsip[s]) + r
    out = np.where(found, S[np.where(found, off, 0)], np.nan)
    return out, int(np.count_nonzero(~found))


def pattern_pairs(sym):
    """(rows, cols): every position of the factor's pattern, lower triangle"""
    Super, Lsip, Lsi = _arr(sym, "Super", "Lsip", "Lsi")
    rr, cc = [], []
    for s in range(int(sym.nsuper)):
        rows = Lsi[Lsip[s]:Lsip[s + 1]]
        for c in range(int(Super[s]), int(Super[s + 1])):
            k = c - int(Super[s])
            rr.append(rows[k:])
            cc.append(np.full(len(rows) - k, c))
    return np.concatenate(rr).astype(np.int64), np.concatenate(cc).astype(np.int64)
