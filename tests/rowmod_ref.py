"""Reference for row deletion / addition on a supernodal Cholesky factor (csrc/sf_rowmod.hip), on updown_ref.Structure.

* lists: the three lists of sf_chol_plan_rowmod_path by brute force, admissible_index: the rule for rowadd's indices.
* zero/column/sweep emulations: numpy restatements of ONE launch of each kernel, the same operations in the same order, in fp64
  without fused multiply-adds.
* rowdel_emulate / rowadd_emulate: the host loops of the two entry points, the rank-1 step through ur.update_emulate.
* deleted: A with row and column j replaced by the identity's.
"""
import numpy as np

import updown_ref as ur

UPD_B = ur.UPD_B


def locate(st, j):
    s = int(st.SuperMap[j])
    return s, j - int(st.Super[s])


def admissible_index(st, j, i):
    s, _ = locate(st, j)
    if i < j:
        si = int(st.SuperMap[i])
        return si == s or j in st.below(si)
    return i == j or i in st.rows(s)


def lists(st, j, idx=None):
    """{"rows": [(p, position of j in rows(p))], "sweep": [...], "update": [...]} for row j and rowadd's indices idx"""
    s, c = locate(st, j)
    rows = [(p, int(np.flatnonzero(st.rows(p) == j)[0])) for p in range(s) if j in st.below(p)]
    sweep = set()
    for i in ([] if idx is None else idx):
        p = int(st.SuperMap[i])
        while i < j and p != s:
            sweep.add(p)
            p = st.parent(p)
            assert 0 <= p <= s
    w = st.rows(s)[c + 1:]
    return {"rows": rows, "sweep": sorted(sweep), "update": st.path([w]) if len(w) else []}


def deleted(A, j):
    A1 = np.array(A)
    A1[j, :] = 0.0
    A1[:, j] = 0.0
    A1[j, j] = 1.0
    return A1


def column_of(st, A, j):
    """(idx, vals) of column j of the symmetric A on its own pattern, the diagonal included"""
    idx = np.flatnonzero(A[:, j])
    idx = np.union1d(idx, [j])
    return idx, A[idx, j].copy()


def rowdel_column_emulate(col, Wr):
    """k_rowdel_column: col = the panel's column from L_jj down (in place), Wr = the rows of W of the entries below the diagonal"""
    Wr[:] = col[1:]
    col[1:] = 0.0
    col[0] = 1.0


def sweep_diag_emulate(D, w):
    """k_rowadd_sweep_diag: D y = w on the lower triangle of D; w is zeroed as the kernel leaves it; returns y"""
    b = len(w)
    y = np.zeros(b)
    for j in range(b):
        y[j] = w[j] / D[j, j]
        w[j + 1:] = w[j + 1:] - D[j + 1:, j] * y[j]
    w[:] = 0.0
    return y


def sweep_rows_emulate(P, Wr, y, target):
    """k_rowadd_sweep_rows: the rows P (nrows x b, in place), their entries Wr of W (in place); target: mask of the row that takes y"""
    P[target, :] = y
    for j in range(len(y)):
        Wr[:] = Wr - P[:, j] * y[j]


def rowadd_column_emulate(col, Wr, d):
    """k_rowadd_column: (failed, what W[j] holds afterwards).  col from L_jj down and Wr (in place) are written on success only"""
    if not d > 0.0:
        return True, d
    r = np.sqrt(d)
    col[0] = r
    v = Wr / r
    col[1:] = v
    Wr[:] = v
    return False, 0.0


def rowdel_emulate(st, Lsx, j):
    """the whole of sf_chol_plan_rowdel: (new Lsx, lists)"""
    L = np.array(Lsx, dtype=np.float64)
    s, c = locate(st, j)
    what = lists(st, j)
    for p, pos in what["rows"]:
        st.panel(L, p)[pos, :] = 0.0
    P = st.panel(L, s)
    P[c, :c] = 0.0
    w = np.zeros(st.n)
    r = st.rows(s)[c + 1:]
    Wr = w[r]
    rowdel_column_emulate(P[c:, c], Wr)
    w[r] = Wr
    if len(r):
        L, failed, _ = ur.update_emulate(st, L, w, +1)
        assert not failed
    return L, what


def rowadd_emulate(st, Lsx, j, idx, vals):
    """the whole of sf_chol_plan_rowadd on a factor whose row and column j are the identity's: (new Lsx, failed, lists)"""
    L = np.array(Lsx, dtype=np.float64)
    s, c = locate(st, j)
    idx = np.asarray(idx, dtype=np.int64)
    for i in idx:
        if not admissible_index(st, j, int(i)):
            raise ValueError(f"index {int(i)} is not admissible for row {j}")
    what = lists(st, j, idx)
    W = np.zeros(st.n)
    W[idx] = vals
    for p in what["sweep"] + [s]:
        P, rows, c0 = st.panel(L, p), st.rows(p), int(st.Super[p])
        ncols = c if p == s else st.nscol(p)
        for j0 in range(0, ncols, UPD_B):
            b = min(UPD_B, ncols - j0)
            y = sweep_diag_emulate(P[j0:j0 + b, j0:j0 + b], W[c0 + j0:c0 + j0 + b])
            r = rows[j0 + b:]
            Wr = W[r]
            sweep_rows_emulate(P[j0 + b:, j0:j0 + b], Wr, y, r == j)
            W[r] = Wr
    P = st.panel(L, s)
    r = st.rows(s)[c + 1:]
    Wr = W[r]
    failed, W[j] = rowadd_column_emulate(P[c:, c], Wr, W[j])
    W[r] = Wr
    if failed:
        return L, True, what
    if len(r):
        L, failed, _ = ur.update_emulate(st, L, W, -1)
    return L, failed, what


def write_set(st, j, what):
    """mask over Lsx of the documented write set of either call: row j of every panel that holds it below its own columns, the
    panels of the update path, and -- where s is not on that path, j being its last column or the last row of all -- row c and
    column c of the panel of s; lower triangles only"""
    s, c = locate(st, j)
    m = st.panel_mask(what["update"])
    for p, pos in what["rows"]:
        st.panel(m, p)[pos, :] = True
    P = st.panel(m, s)
    P[c, :c + 1] = True
    P[c:, c] = True
    return m & st.lower_mask()


def rows_to_try(st, seed):
    """the rows every case is tried on: the first column of the first leaf, the last column of a leaf, the middle of the widest
    supernode, the last column of the last root, two seeded random ones"""
    widest = int(np.argmax(np.diff(st.Super)))
    rng = np.random.default_rng(seed)
    rows = [0, int(st.Super[1]) - 1, int(st.Super[widest]) + st.nscol(widest) // 2, st.n - 1] + [int(v) for v in rng.integers(st.n, size=2)]
    out = []
    for r in rows:
        if r not in out:
            out.append(r)
    return out
