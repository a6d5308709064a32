"""Reference for the rank-k update / downdate of a supernodal Cholesky factor (csrc/sf_updown.hip).

* Structure: the supernodal arrays of a Symbolic, with the forest's parents, the brute-force path and the admissibility rule.
* diag_emulate / rows_emulate: numpy restatements of ONE launch of k_updown_diag / k_updown_rows -- the same rotations in the same
  (j, t) order with the same formulas (1 / c formed once per rotation), in fp64 without fused multiply-adds.
* update_emulate: the host loop of sf_chol_plan_update over the path, block by block, chunks of 16 columns.
* backward_error: |L L^T - A|_F / |A|_F in longdouble, panel by panel.
"""
import numpy as np

import kernel_ref as kr

LD = np.longdouble
UPD_W, UPD_B = 16, 64


class Structure:
    def __init__(self, sym):
        g = (lambda k: sym[k]) if isinstance(sym, dict) else (lambda k: getattr(sym, k))
        self.n, self.nsuper, self.xsize = int(g("n")), int(g("nsuper")), int(g("xsize"))
        self.Super, self.SuperMap, self.Lsip, self.Lsi, self.Lsxp = (np.asarray(g(k), dtype=np.int64) for k in
                                                                     ("Super", "SuperMap", "Lsip", "Lsi", "Lsxp"))

    def nscol(self, s):
        return int(self.Super[s + 1] - self.Super[s])

    def nsrow(self, s):
        return int(self.Lsip[s + 1] - self.Lsip[s])

    def rows(self, s):
        return self.Lsi[self.Lsip[s]:self.Lsip[s + 1]]

    def below(self, s):
        return self.rows(s)[self.nscol(s):]

    def parent(self, s):
        b = self.below(s)
        return int(self.SuperMap[b[0]]) if len(b) else -1

    def panel(self, Lsx, s):
        """the nsrow x nscol panel of s as a (writable) column-major view of Lsx"""
        r, c = self.nsrow(s), self.nscol(s)
        return Lsx[self.Lsxp[s]:self.Lsxp[s] + r * c].reshape(c, r).T

    def admissible(self, rows):
        rows = np.sort(np.asarray(rows, dtype=np.int64))
        if len(rows) == 0:
            return True
        s0 = int(self.SuperMap[rows[0]])
        return bool(np.all(np.isin(rows[1:], self.rows(s0))))

    def path(self, columns):
        """brute force: every ancestor of the supernode of each column's smallest row, by walking the parents"""
        out = set()
        for rows in columns:
            if len(rows) == 0:
                continue
            s = int(self.SuperMap[min(rows)])
            while s >= 0:
                out.add(s)
                s = self.parent(s)
        return sorted(out)

    def clique(self, s0, j0=None, count=None):
        """an admissible full column starting at column j0 of s0: j0 and everything s0 has from there on (optionally the first `count`)"""
        j0 = int(self.Super[s0]) if j0 is None else j0
        r = self.rows(s0)
        r = r[r >= j0]
        return r if count is None else r[:count]

    def dense(self, Lsx, dtype=np.float64):
        L = np.zeros((self.n, self.n), dtype=dtype)
        for s in range(self.nsuper):
            P = self.panel(Lsx, s)
            c0 = int(self.Super[s])
            for c in range(self.nscol(s)):
                L[self.rows(s)[c:], c0 + c] = P[c:, c]
        return L

    def lower_mask(self):
        m = np.zeros(self.xsize, dtype=bool)
        for s in range(self.nsuper):
            r, c = self.nsrow(s), self.nscol(s)
            M = m[self.Lsxp[s]:self.Lsxp[s] + r * c].reshape(c, r).T
            for j in range(c):
                M[j:, j] = True
        return m

    def panel_mask(self, supers):
        m = np.zeros(self.xsize, dtype=bool)
        for s in supers:
            m[self.Lsxp[s]:self.Lsxp[s] + self.nsrow(s) * self.nscol(s)] = True
        return m


def dense_matrix(sym):
    """the permuted matrix (both triangles) the plan assembles from (Lp, Li, Lx)"""
    n = sym.n
    Lp, Li, Lx = np.asarray(sym.Lp), np.asarray(sym.Li), np.asarray(sym.Lx)
    j = np.repeat(np.arange(n), np.diff(Lp))
    A = np.zeros((n, n))
    A[Li, j] = Lx
    A[j, Li] = Lx
    return A


def values_of(sym, A):
    """Lx of the dense symmetric A on the pattern of the plan (entries outside it must be zero)"""
    Lp, Li = np.asarray(sym.Lp), np.asarray(sym.Li)
    j = np.repeat(np.arange(sym.n), np.diff(Lp))
    return np.ascontiguousarray(A[Li, j])


def _rotation(d, w, sign, bad):
    r2 = (d - w) * (d + w) if sign < 0 else d * d + w * w
    bad = bad or not (r2 > 0.0)
    if bad:
        return d, 1.0, 0.0, True
    r = np.sqrt(r2)
    return r, r / d, w / d, False


def diag_emulate(D, Wb, sign, bad=False):
    """one launch of k_updown_diag on the b x b block D (lower triangle read and written, in place) and its b x K rows of W (zeroed,
    as the kernel leaves them); returns (rot[b, K, 2], bad)"""
    b, K = Wb.shape
    rot = np.zeros((b, K, 2))
    for j in range(b):
        for t in range(K):
            r, c, s, bad = _rotation(D[j, j], Wb[j, t], sign, bad)
            ci = 1.0 / c
            D[j, j] = r
            x = (D[j + 1:, j] + sign * (s * Wb[j + 1:, t])) * ci
            Wb[j + 1:, t] = c * Wb[j + 1:, t] - s * x
            D[j + 1:, j] = x
            rot[j, t] = (c, s)
    Wb[:, :] = 0.0
    return rot, bad


def rows_emulate(P, Wr, rot, sign):
    """one launch of k_updown_rows: the rows P (nrows x b, in place) with their rows Wr of W (nrows x K, in place)"""
    b, K = rot.shape[:2]
    for j in range(b):
        x = P[:, j].copy()
        for t in range(K):
            c, s = rot[j, t]
            x = (x + sign * (s * Wr[:, t])) * (1.0 / c)
            Wr[:, t] = c * Wr[:, t] - s * x
        P[:, j] = x


def update_emulate(st, Lsx, W, sign):
    """the whole of sf_chol_plan_update: (new Lsx, failed, path).  W: dense (n, k), each column's non-zeros its pattern"""
    Lsx = np.array(Lsx, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64).reshape(st.n, -1)
    columns = [np.flatnonzero(W[:, t]) for t in range(W.shape[1])]
    for t, rows in enumerate(columns):
        if not st.admissible(rows):
            raise ValueError(f"column {t} is not admissible")
    path = st.path(columns)
    bad = False
    for t0 in range(0, W.shape[1], UPD_W):
        Wc = np.array(W[:, t0:t0 + UPD_W])
        for s in path:
            P, rows, c0, nscol = st.panel(Lsx, s), st.rows(s), int(st.Super[s]), st.nscol(s)
            for j0 in range(0, nscol, UPD_B):
                b = min(UPD_B, nscol - j0)
                Wb = Wc[c0 + j0:c0 + j0 + b]
                rot, bad = diag_emulate(P[j0:j0 + b, j0:j0 + b], Wb, sign, bad)
                if P.shape[0] > j0 + b:
                    r = rows[j0 + b:]
                    Wr = Wc[r]
                    rows_emulate(P[j0 + b:, j0:j0 + b], Wr, rot, sign)
                    Wc[r] = Wr
    return Lsx, bad, path


def backward_error(st, Lsx, A):
    """|L L^T - A|_F / |A|_F in longdouble, the product formed panel by panel (a panel's rows x rows block)"""
    R = np.array(A, dtype=LD)
    for s in range(st.nsuper):
        P = np.array(st.panel(Lsx, s), dtype=LD)
        c = st.nscol(s)
        P[:c, :c] = np.tril(P[:c, :c])
        rows = st.rows(s)
        R[np.ix_(rows, rows)] -= kr.matmul_ld(P, P.T)
    return float(np.sqrt(np.sum(R * R)) / np.sqrt(np.sum(np.array(A, dtype=LD) ** 2)))


def chol_panels(sym, st, A):
    """the longdouble Cholesky factor of A in the supernodal layout (float64 xsize array, upper parts of diagonal blocks zero)"""
    L = kr.chol_ld(A)
    out = np.zeros(st.xsize)
    for s in range(st.nsuper):
        P = st.panel(out, s)
        c0 = int(st.Super[s])
        for c in range(st.nscol(s)):
            P[c:, c] = L[st.rows(s)[c:], c0 + c].astype(np.float64)
    return out
