"""Extended-precision references and per-element error bounds for the single-launch kernel tests (tests/test_kernels.py).

References are computed in np.longdouble (64-bit mantissa on x86-64: 11 more bits than fp64), so the reference's own
rounding is far below the bounds.  Every bound is per ELEMENT, of the form the algorithm satisfies in fp64
(u = 2^-53, SAFETY = small constant for the fused / reordered summations):
    GEMM / update  |C^ - C|       <= SAFETY (K + 2) u (|C0| + |Y| |X|^T)
    POTRF          |A - L^ L^T|   <= SAFETY (b + 2) u |L^| |L^T|
    GETRF          |PA - L^ U^|   <= SAFETY (b + 2) u |L^| |U^|
    TRSM           |X^ D^T - B|   <= SAFETY (b + 2) u |X^| |D^T|
    LU panel       |A - L~ U~|    <= SAFETY (terms + 2) u |L~| |U~|      (fused steps, from the stored factor: lu_panel_check)
    solve sweeps   |sum of an equation's terms - its right-hand side| <= SAFETY (terms) u (sum of the terms' magnitudes)
    selinv GEMM    |C^ - C|       <= SAFETY (K_z + 2) u (|C0| + |op(A)| |B|)   per K slab z (K_z = its K range; an empty slab: +0.0)
    selinv trinv   |T X^ - I|     <= SAFETY (w + 2) u |T| |X^|                 (unit or stored diagonal; strict upper part +0.0)
    selinv small   forward bound through T^-1 -> Y -> Z -> Sigma(C,C) with absolute-value matrices (small_ref)
    selinv sum / finish / diag / pack: bit for bit;  logdet: SAFETY (8 + ceil(np / 256) + 2) u sum|log| + u sum|log|
A max-normalised metric (max error / max |ref|) would hide an error in a row scaled by 1e-6; these do not.

Arena: the tests place every operand in one fp64 host image (the probe copies it to the device, launches once and copies
it back).  Each region is surrounded by guard bands of GUARD doubles (64 KiB) holding NaN; elements of a region outside
a kernel's documented read footprint hold NaN too, so a read that leaks into a stored result shows up as a non-finite
value; every element outside the documented write footprint is compared bit for bit with its value before the launch.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SAFETY = 4.0
GUARD = 8192                 # doubles: 64 KiB


def have_longdouble():
    return np.finfo(np.longdouble).nmant >= 63


class Arena:
    """a host image of a device double arena: regions separated by NaN guard bands"""

    def __init__(self):
        self.size = GUARD
        self.regions = []

    def alloc(self, count, align=1, skew=0):
        """offset of a new region of `count` doubles; the region starts `skew` doubles past an `align` boundary (odd skews
        make 16-byte loads from 8-byte-aligned addresses)"""
        off = self.size
        off += (-off) % align + skew
        self.regions.append((off, count))
        self.size = off + count + GUARD
        return off

    def image(self):
        a = np.full(self.size, np.nan)
        return a


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_unchanged(before, after, written_mask, what):
    """every element outside the write footprint is bit-identical to its value before the launch"""
    keep = ~written_mask
    diff = bits(before)[keep] != bits(after)[keep]
    if diff.any():
        idx = np.flatnonzero(keep)[np.flatnonzero(diff)[:8]]
        raise AssertionError(f"{what}: {int(diff.sum())} elements outside the write footprint changed, first at {idx.tolist()}")


def assert_within(got, ref, bound, what):
    """got (fp64) finite and |got - ref| <= bound elementwise (ref, bound: longdouble)"""
    got = np.asarray(got)
    if not np.all(np.isfinite(got)):
        bad = np.argwhere(~np.isfinite(got))[:8]
        raise AssertionError(f"{what}: non-finite stored results at {bad.tolist()}")
    err = np.abs(got.astype(LD) - ref)
    viol = err > bound
    if viol.any():
        k = np.argwhere(viol)[0]
        ratio = float(np.max(err[viol] / np.maximum(bound[viol], np.finfo(LD).tiny)))
        raise AssertionError(f"{what}: {int(viol.sum())} of {viol.size} elements beyond the bound, first at {k.tolist()} "
                             f"(err {float(err[tuple(k)]):.3e}, bound {float(bound[tuple(k)]):.3e}, worst ratio {ratio:.3g})")


def scalings(rng, n, lo=1e-6, hi=1e6):
    """n scale factors log-uniform over [lo, hi]"""
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def matmul_ld(a, b):
    """longdouble product (numpy has no BLAS for it: row blocks keep the temporaries small)"""
    a = np.asarray(a, dtype=LD)
    b = np.asarray(b, dtype=LD)
    out = np.empty((a.shape[0], b.shape[1]), dtype=LD)
    step = max(1, (1 << 22) // max(1, a.shape[1] * b.shape[1]))
    for r in range(0, a.shape[0], step):
        out[r:r + step] = np.einsum("ik,kj->ij", a[r:r + step], b)
    return out


def gemm_ref(C0, Y, X, strict):
    """C0 - Y X^T, its bound, and the mask of the produced entries (the lower trapezoid ci >= cj + strict)"""
    M, K = Y.shape
    N = X.shape[0]
    ref = np.asarray(C0, dtype=LD) - matmul_ld(Y, X.T)
    bound = SAFETY * (K + 2) * U * (np.abs(np.asarray(C0, dtype=LD)) + matmul_ld(np.abs(Y), np.abs(X).T))
    mask = np.tril(np.ones((M, N), dtype=bool), -strict)
    return ref, bound, mask


def potrf_check(A, Lh, what):
    """A (b x b symmetric, lower used) against the computed lower factor Lh"""
    b = A.shape[0]
    L = np.tril(Lh).astype(LD)
    res = np.asarray(np.tril(A), dtype=LD) - np.tril(matmul_ld(L, L.T))
    bound = np.tril(SAFETY * (b + 2) * U * matmul_ld(np.abs(L), np.abs(L).T))
    assert np.all(np.isfinite(np.tril(Lh))), f"{what}: non-finite entries in the factor"
    viol = np.abs(res) > bound
    assert not viol.any(), f"{what}: |A - L L^T| beyond the bound at {np.argwhere(viol)[:4].tolist()}"


def chol_ld(A):
    """unpivoted Cholesky in longdouble (lower)"""
    A = np.array(A, dtype=LD)
    b = A.shape[0]
    L = np.zeros_like(A)
    for j in range(b):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def getrf_rule(A, tol, eps):
    """longdouble restatement of the block pivoting rule (sf_kernels.h, PivotCtl): returns (pos, L, U, perturbed, margin) with
    pos[r] = position that row r ends up in, perturbed = the columns whose pivot was replaced by +-eps, margin = smallest
    relative distance of a pivoting decision from its threshold (ties: the lowest row, as the kernel's arg-max)"""
    A = np.array(A, dtype=LD)
    b = A.shape[0]
    active = np.ones(b, dtype=bool)
    pos = np.arange(b)
    row_at = np.full(b, -1)
    perturbed = []
    margin = np.inf
    for j in range(b):
        p = j
        col = np.abs(A[:, j])
        if tol > 0:
            amax = np.max(col[active]) if active.any() else LD(0)
            nat = col[j]
            if amax > 0 and not (active[j] and nat == amax):
                margin = min(margin, float(abs(nat - LD(tol) * amax) / amax))
            if not (active[j] and nat >= LD(tol) * amax and nat != 0):
                cand = np.flatnonzero(active)
                order = np.argsort(-col[cand], kind="stable")
                p = int(cand[order[0]])
                if len(order) > 1 and col[cand[order[0]]] > 0:
                    margin = min(margin, float((col[cand[order[0]]] - col[cand[order[1]]]) / col[cand[order[0]]]))
        piv = A[p, j]
        if eps > 0 and abs(piv) < eps:
            piv = LD(-eps) if piv < 0 else LD(eps)
            A[p, j] = piv
            perturbed.append(j)
        elim = active.copy()
        elim[p] = False
        A[elim, j] /= piv
        A[np.ix_(elim, np.arange(j + 1, b))] -= np.outer(A[elim, j], A[p, j + 1:])
        active[p] = False
        pos[p] = j
        row_at[j] = p
    F = A[row_at]           # rows in pivot order
    L = np.tril(F, -1) + np.eye(b, dtype=LD)
    Uu = np.triu(F)
    return pos, L, Uu, perturbed, margin


def assert_equations(total, rhs, nterms, mag, cols, what):
    """one equation per element: `total` (longdouble: the sum of the equation's products, formed from the stored results)
    against its right-hand side, |total - rhs| <= SAFETY nterms u mag with nterms = the number of terms of the sum and mag = the
    sum of their magnitudes (|rhs| among them where rhs is itself a summand).  Only the columns `cols` are checked (the others may hold a planted NaN).  Returns the worst err / bound over them."""
    total, mag = np.asarray(total, dtype=LD)[:, cols], np.asarray(mag, dtype=LD)[:, cols]
    rhs = np.asarray(rhs, dtype=LD)[:, cols]
    if not np.all(np.isfinite(total)):
        raise AssertionError(f"{what}: non-finite stored results at {np.argwhere(~np.isfinite(total))[:8].tolist()}")
    err = np.abs(total - rhs)
    bound = SAFETY * np.asarray(nterms, dtype=LD).reshape(-1, 1) * U * mag
    viol = err > bound
    worst = float(np.max(err / np.maximum(bound, np.finfo(LD).tiny), initial=0.0))
    if viol.any():
        k = tuple(np.argwhere(viol)[0])
        raise AssertionError(f"{what}: {int(viol.sum())} of {viol.size} equations beyond the bound, first at {list(k)} "
                             f"(err {float(err[k]):.3e}, bound {float(bound[k]):.3e}, worst err / bound {worst:.3g})")
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the transposed backward launch of the device solve (csrc/sf_solve_t.hip): tests/test_kernels_tsolve.py
# ---------------------------------------------------------------------------------------------------------------------
def tsolve_matrix(D, pos, nb=64):
    """M of one panel's block as the forward launch with unit = 1 and the same interchanges sees it (the statement the transposed
    launch is the adjoint of): S = the strictly lower part of D with a unit diagonal; inside each nb-row sub-block, row l of the
    diagonal sub-block is S[pos[l]]; left of the sub-block the rows are their own."""
    b = D.shape[0]
    S = np.tril(D, -1) + np.eye(b)
    M = S.copy()
    for s in range(0, b, nb):
        M[s:s + nb, s:s + nb] = S[pos[s:s + nb], s:s + nb]
    return M


TSOLVE_FAULTS = ("forward permutation", "late interchange", "stored diagonal")


def tsolve_emulate(D, Lb, pos, xblk, xrows, fault=None, nb=64):
    """plain float64 emulation of the transposed backward launch on one panel: the tiles subtract Lb^T x[rows]; then the sub-blocks
    from the last to the first: the unit upper chain (L^T of the sub-block, from its last row up), the inverse interchange
    z[l] = w[pos[l]], then the subtraction from the earlier sub-blocks.  fault: one of TSOLVE_FAULTS, a single corruption --
    z[pos[l]] = w[l]; the earlier sub-blocks read before the interchange; D's own diagonal in place of the implied 1."""
    assert fault is None or fault in TSOLVE_FAULTS
    b = D.shape[0]
    v = np.array(xblk, dtype=np.float64)
    v -= Lb.T @ xrows
    for s in reversed(range(0, b, nb)):
        e = min(s + nb, b)
        w = v[s:e].copy()
        for j in reversed(range(s, e)):
            if fault == "stored diagonal":
                w[j - s] = w[j - s] / D[j, j]
            w[:j - s] -= D[j, s:j, None] * w[j - s]
        local = pos[s:e] - s
        z = np.empty_like(w)
        if fault == "forward permutation":
            z[local] = w
        else:
            z = w[local]
        v[s:e] = z
        v[:s] -= D[s:e, :s].T @ (w if fault == "late interchange" else z)
    return v


# ---------------------------------------------------------------------------------------------------------------------
# LU panels factored by fused 64-column steps (k_step<true>): tests/test_kernels_lu.py
# ---------------------------------------------------------------------------------------------------------------------
LU_NB = 64


def _solve_right_upper(B, Uu):
    """X with X Uu = B (Uu upper triangular), longdouble, column by column"""
    X = np.array(B, dtype=LD)
    for c in range(Uu.shape[0]):
        X[:, c] = (X[:, c] - X[:, :c] @ Uu[:c, c]) / Uu[c, c]
    return X


def _solve_left_unit_lower(L, B):
    """Y with L Y = B (L unit lower triangular), longdouble, row by row"""
    Y = np.array(B, dtype=LD)
    for r in range(1, L.shape[0]):
        Y[r] -= L[r, :r] @ Y[:r]
    return Y


def lu_full(A11, A21, A12):
    """the panel's matrix [[A11, A12], [A21, nan]] with its rows and columns in original order (the corner is never formed)"""
    nscol, below = A11.shape[0], A21.shape[0]
    A = np.full((nscol + below, nscol + below), np.nan)
    A[:nscol, :nscol], A[nscol:, :nscol], A[:nscol, nscol:] = A11, A21, A12
    return A


def lu_panel_ref(A11, A21, A12, tol, eps, J=0):
    """longdouble restatement of what the fused LU steps of one panel compute from column J on (sf_plan_build.hip, fused_step;
    sf_kernels.h, PivotCtl).  For each 64-column block in turn: the block, the rows below it and the columns to its right are
    updated with all earlier blocks (L rows in ORIGINAL order: interchanges stay inside a block), getrf_rule factors the
    diagonal block, then L21 = A21' U11^-1 and U12 = L11^-1 P A12'.
    Returns (pos, PL, PU, perturbed, margin): pos[r] = position of original row r (identity before J); PL / PU = the factor as
    the device stores it, nsrow x nscol each (L strictly lower, U^T lower with the diagonal; what no task writes is NaN);
    perturbed = the panel columns whose pivot was replaced; margin = the smallest decision margin over all blocks."""
    nscol, below = A11.shape[0], A21.shape[0]
    nsrow = nscol + below
    A = lu_full(A11, A21, A12).astype(LD)
    PL = np.full((nsrow, nscol), np.nan, dtype=LD)
    PU = np.full((nsrow, nscol), np.nan, dtype=LD)
    pos = np.arange(nscol)
    perturbed, margin = [], np.inf
    for c0 in range(J, nscol, LU_NB):
        c1 = min(c0 + LU_NB, nscol)
        b = c1 - c0
        S = A[c0:, c0:c1] - matmul_ld(PL[c0:, J:c0], PU[c0:c1, J:c0].T)       # rows c0.. of the block's columns
        T = A[c0:c1, c1:] - matmul_ld(PL[c0:c1, J:c0], PU[c1:, J:c0].T)       # the block's rows of the columns to its right
        p, L, Uu, pert, m = getrf_rule(S[:b], tol, eps)
        row_at = np.argsort(p)
        pos[c0:c1] = c0 + p
        perturbed += [c0 + j for j in pert]
        margin = min(margin, m)
        lo = np.tril(np.ones((b, b), dtype=bool), -1)
        PL[c0:c1, c0:c1][lo] = L[lo]
        PU[c0:c1, c0:c1][~lo.T] = Uu.T[~lo.T]
        PL[c1:, c0:c1] = _solve_right_upper(S[b:], Uu)
        PU[c1:, c0:c1] = _solve_left_unit_lower(L, T[row_at]).T
    return pos, PL, PU, perturbed, margin


def lu_panel_check(A11, A21, A12, PL, PU, pos, perturbed, J, what):
    """The STORED factor (PL, PU: nsrow x nscol, fp64, as the device leaves them) against the panel's matrix, element by element, no
    reference factor needed.  With L~ = the stored L rows put back in original row order inside their own block (unit diagonal
    added; entries left of the block are stored in original order already) and U~(i, c) = PU(c, i), c >= i:
        A(r, c) = sum_i L~(r, i) U~(i, c)       for every (r, c) outside the (below x below) corner,
        |A - L~ U~|(r, c) <= SAFETY (terms + 2) u (|L~| |U~|)(r, c),   terms = min(end of r's block, c + 1) - J,
    i.e. the number of products the sum can hold.  The diagonal entry of a perturbed column is exempt.  Returns the worst
    err / bound over the checked elements."""
    nscol, below = A11.shape[0], A21.shape[0]
    nsrow = nscol + below
    n = nscol - J
    A = lu_full(A11, A21, A12)[J:, J:].astype(LD)
    PL, PU = np.asarray(PL)[J:, J:], np.asarray(PU)[J:, J:]
    Lt = np.zeros((nsrow - J, n), dtype=LD)
    Ut = np.zeros((n, nsrow - J), dtype=LD)
    limit = np.full(nsrow - J, n)
    for c0 in range(0, n, LU_NB):
        c1 = min(c0 + LU_NB, n)
        b = c1 - c0
        p = np.asarray(pos[J + c0:J + c1]) - (J + c0)
        assert sorted(p.tolist()) == list(range(b)), f"{what}: pos is no permutation inside the block at column {J + c0}"
        Lt[c0:c1, :c0] = PL[c0:c1, :c0]
        Lt[c0:c1, c0:c1] = (np.tril(PL[c0:c1, c0:c1], -1) + np.eye(b))[p]
        Lt[c1:, c0:c1] = PL[c1:, c0:c1]
        Ut[c0:c1, c0:c1] = np.triu(PU[c0:c1, c0:c1].T)
        Ut[c0:c1, c1:] = PU[c1:, c0:c1].T
        limit[c0:c1] = c1
    if not (np.all(np.isfinite(Lt)) and np.all(np.isfinite(Ut))):
        raise AssertionError(f"{what}: non-finite stored factor entries")
    terms = np.minimum(limit[:, None], np.arange(nsrow - J)[None, :] + 1)
    mag = matmul_ld(np.abs(Lt), np.abs(Ut))
    err = np.abs(A - matmul_ld(Lt, Ut))
    bound = SAFETY * (terms + 2) * U * mag
    check = np.ones(A.shape, dtype=bool)
    check[n:, n:] = False
    for j in perturbed:                     # the factorization is of A + E, E on the replaced pivot
        check[np.flatnonzero(np.asarray(pos[J:]) == j)[0], j - J] = False
    viol = check & ~(err <= bound)
    if viol.any():
        k = tuple(np.argwhere(viol)[0])
        raise AssertionError(f"{what}: {int(viol.sum())} elements of |A - L U| beyond the bound, first at row {k[0] + J} column {k[1] + J} "
                             f"(err {float(err[k]):.3e}, bound {float(bound[k]):.3e})")
    return float(np.max(np.where(check, err / np.maximum(bound, np.finfo(LD).tiny), 0)))


# ---------------------------------------------------------------------------------------------------------------------
# the selected inversion, one launch at a time (csrc/sf_selinv.hip, sf_selinv_lu.hip): tests/test_kernels_selinv.py
# ---------------------------------------------------------------------------------------------------------------------
SG_K = 16                    # K chunk of k_selinv_gemm
SEL_FAULTS = ("swap arenas", "wrong pair", "dropped chunk", "slab overlap", "stored diagonal", "mirror outside J")


def within_ratio(got, ref, bound, what):
    """assert_within, returning the worst err / bound (0 / 0 counts as 0)"""
    assert_within(got, ref, bound, what)
    err = np.abs(np.asarray(got).astype(LD) - ref)
    return float(np.max(np.where(err > 0, err / np.maximum(bound, np.finfo(LD).tiny), 0), initial=0.0))


class SelTables:
    """The pair table and the relative maps of a supernodal structure as sf_selinv_schedule and k_build_relmaps lay them out: for
    every supernode J and every ancestor a that J's rows below fall into, in row order, one pair (i, map_off) -- i = the panel
    position of J's first row in a, relmap[map_off + k] = the position of J's panel row i + k in the row list of a, for ALL rows
    from i to the end of J's list.  Written with a dictionary lookup, not with the searchsorted of selinv_ref.py."""

    def __init__(self, Super, Lsip, Lsi, Xp, pad=0):
        self.Super, self.Lsip, self.Lsi, self.Xp = (np.asarray(v) for v in (Super, Lsip, Lsi, Xp))
        self.nsuper = len(self.Super) - 1
        self.n = int(self.Super[-1])
        self.SuperMap = np.repeat(np.arange(self.nsuper), np.diff(self.Super)).astype(np.int32)
        self.pairs, self.pair0, relmap = [], [0], [np.full(pad, -(1 << 30), dtype=np.int64)]
        off = pad
        for s in range(self.nsuper):
            ncol, rows = self.ncol(s), self.rows(s)
            i = ncol
            while i < len(rows):
                a = self.SuperMap[rows[i]]
                where = {int(g): k for k, g in enumerate(self.rows(a))}
                self.pairs.append((off, i))
                relmap.append(np.array([where[int(g)] for g in rows[i:]], dtype=np.int64))
                off += len(rows) - i
                while i < len(rows) and self.SuperMap[rows[i]] == a:
                    i += 1
            self.pair0.append(len(self.pairs))
        self.relmap = np.concatenate(relmap)

    def ncol(self, s):
        return int(self.Super[s + 1] - self.Super[s])

    def nsrow(self, s):
        return int(self.Lsip[s + 1] - self.Lsip[s])

    def rows(self, s):
        return self.Lsi[self.Lsip[s]:self.Lsip[s + 1]]

    def gather_index(self, J, ce, fault=None):
        """idx (m x m): entry (x, y) of Sigma(R,R) of the unit of J whose R starts at panel position ce lies at arena index
        idx[x, y]: in column min(x, y)'s panel at the row position of max(x, y) (sel_col / sel_at).  fault "wrong pair": a column
        of J's second or later pair is addressed with the pair before it."""
        ns, nc = self.nsrow(J), self.ncol(J)
        m = ns - ce
        idx = np.zeros((m, m), dtype=np.int64)
        prs = self.pairs[self.pair0[J]:self.pair0[J + 1]]
        for y in range(m):
            q = ce + y
            hi = np.arange(q, ns)
            if q < nc:
                at = self.Xp[J] + q * ns + hi
            else:
                k = max(t for t, pr in enumerate(prs) if pr[1] <= q)
                if fault == "wrong pair" and k > 0:
                    k -= 1
                g = self.Lsi[self.Lsip[J] + q]
                a = self.SuperMap[g]
                at = self.Xp[a] + (g - self.Super[a]) * self.nsrow(a) + self.relmap[prs[k][0] - prs[k][1] + hi]
            idx[y:, y] = at
            idx[y, y:] = at
        return idx

    def gather(self, J, ce, S, S2, fault=None):
        """Sigma(R,R): on and below the diagonal from S, above it from S2 ("swap arenas": the other way round)"""
        idx = self.gather_index(J, ce, fault)
        if fault == "swap arenas":
            S, S2 = S2, S
        low = np.tril(np.ones(idx.shape, dtype=bool))
        return np.where(low, S[idx], S2[idx]), idx


def sel_slabs(K, slabs, fault=None):
    """[k0, k1) of every slab as selinv_gemm cuts K: kslab = the share of a slab rounded up to a multiple of the 16-deep chunk.
    Faults: the last partial chunk of a slab dropped; every slab but the last running one chunk into the next."""
    kslab = ((K + slabs - 1) // slabs + SG_K - 1) // SG_K * SG_K
    out = []
    for z in range(slabs):
        k0 = min(K, z * kslab)
        k1 = min(K, k0 + kslab)
        if fault == "dropped chunk":
            k1 -= (k1 - k0) % SG_K
        if fault == "slab overlap" and z < slabs - 1:
            k1 = min(K, k1 + SG_K)
        out.append((k0, k1))
    return out


def selgemm_emulate(opA, B, C0, slabs, acc_in, fault=None):
    """float64 emulation of one k_selinv_gemm launch: slab z = op(A)[:, k0:k1] B[k0:k1] (+ its own prior content when acc_in).
    C0: slabs x M x N.  Returns slabs x M x N."""
    out = np.zeros(C0.shape)
    for z, (k0, k1) in enumerate(sel_slabs(opA.shape[1], slabs, fault)):
        out[z] = opA[:, k0:k1] @ B[k0:k1]
        if acc_in:
            out[z] = C0[z] + out[z]
    return out


def selgemm_check(got, opA, B, C0, slabs, acc_in, what):
    """every slab against the longdouble product over its own K range; returns the worst err / bound"""
    worst = 0.0
    for z, (k0, k1) in enumerate(sel_slabs(opA.shape[1], slabs)):
        prior = np.abs(np.asarray(C0[z], dtype=LD)) if acc_in else 0
        ref = matmul_ld(opA[:, k0:k1], B[k0:k1]) + (np.asarray(C0[z], dtype=LD) if acc_in else 0)
        bound = SAFETY * (k1 - k0 + 2) * U * (prior + matmul_ld(np.abs(opA[:, k0:k1]), np.abs(B[k0:k1])))
        if k1 == k0 and not acc_in and np.any(bits(got[z]) != 0):
            raise AssertionError(f"{what}: slab {z} has no K range and is beyond the bound: it does not hold +0.0 throughout")
        worst = max(worst, within_ratio(got[z], ref, bound, f"{what} slab {z} K [{k0}, {k1})"))
    return worst


def tri_lower(T, unit):
    """the triangle a trinv launch reads: the strict lower part of T with an implied unit diagonal, or with the stored one"""
    return np.tril(T, -1) + (np.eye(T.shape[0]) if unit else np.diag(np.diag(T)))


def trinv_emulate(T, unit, fault=None, dtype=np.float64):
    """column-oriented forward substitution T X = I as the kernels do it (all columns at once); "stored diagonal": unit ignored"""
    w = T.shape[0]
    T = np.asarray(T, dtype=dtype)
    Bm = np.eye(w, dtype=dtype)
    X = np.zeros((w, w), dtype=dtype)
    for i in range(w):
        X[i] = Bm[i] if (unit and fault != "stored diagonal") else Bm[i] / T[i, i]
        X[i, i + 1:] = 0
        Bm[i + 1:] -= np.outer(T[i + 1:, i], X[i])
    return X


def trinv_check(T, Xh, unit, what):
    """|T X^ - I| <= SAFETY (w + 2) u |T| |X^| elementwise (the residual bound of a substitution), the strict upper triangle of X^
    exactly +0.0, everything finite.  Returns the worst err / bound."""
    w = T.shape[0]
    if not np.all(np.isfinite(Xh)):
        raise AssertionError(f"{what}: non-finite stored results at {np.argwhere(~np.isfinite(Xh))[:8].tolist()}")
    up = np.triu(np.ones((w, w), dtype=bool), 1)
    if np.any(bits(Xh)[up] != 0):
        raise AssertionError(f"{what}: the strict upper triangle is beyond the bound: it does not hold +0.0")
    Tl = tri_lower(T, unit)
    return assert_equations(matmul_ld(Tl, Xh), np.eye(w), np.full(w, (w + 2) / 1.0), matmul_ld(np.abs(Tl), np.abs(Xh)), np.arange(w), what)


def small_ref(Tl, unit_l, Pl, Tu, unit_u, Pu, G):
    """What k_selinv_small / k_lu_selinv_small compute for one unit, in longdouble, with a first-order forward bound.
        Xl = Tl^-1, Xu = Tu^-1, Yl = Pl Xl, Yu = Pu Xu, Zl = G Yl, Zu = G^T Yu, Scc = Xu^T Xl + Yu^T Zl
    (Cholesky: both sides are the one L, G symmetric, so Zu = Zl and Scc = Linv^T Linv + Y^T Z).  Each computed stage is the exact
    operation on its computed inputs plus its own rounding; to first order, with c = SAFETY u and every product's own rounding
    c (terms + 2) times its absolute product:
        dX   <= c (w + 2) |X| |T| |X|                              (substitution: the residual bound of T X^ = I times |X|)
        dY   <= |P| dX + c (w + 2) |P| |X|
        dZ   <= |G| dY + c (m + 2) |G| |Y|                         (G is input data: exact)
        dScc <= dXu^T |Xl| + |Xu|^T dXl + c (w + 2) |Xu|^T |Xl| + dYu^T |Zl| + |Yu|^T dZl + c (m + 2) |Yu|^T |Zl|
    Returns (Zl, dZl, Zu, dZu, Scc, dScc).  The bound is a sum of magnitudes along the chain, so it is only as sharp as the chain is
    well conditioned: the tests use diagonally dominant T."""
    c = SAFETY * U
    w, m = Tl.shape[0], Pl.shape[0]
    G = np.asarray(G, dtype=LD)
    side = []
    for T, unit, P, Gs in ((Tl, unit_l, Pl, G), (Tu, unit_u, Pu, G.T)):
        Tt = tri_lower(T, unit).astype(LD)
        X = np.zeros((w, w), dtype=LD)          # T X = I row by row (inner products): not the column sweep of trinv_emulate
        for i in range(w):
            X[i, :i] = -(Tt[i, :i] @ X[:i, :i]) / Tt[i, i]
            X[i, i] = 1 / Tt[i, i]
        dX = c * (w + 2) * matmul_ld(np.abs(X), matmul_ld(np.abs(Tt), np.abs(X)))
        P = np.asarray(P, dtype=LD)
        Y = matmul_ld(P, X)
        dY = matmul_ld(np.abs(P), dX) + c * (w + 2) * matmul_ld(np.abs(P), np.abs(X))
        Z = matmul_ld(Gs, Y)
        dZ = matmul_ld(np.abs(Gs), dY) + c * (m + 2) * matmul_ld(np.abs(Gs), np.abs(Y))
        side.append((X, dX, Y, dY, Z, dZ))
    (Xl, dXl, Yl, dYl, Zl, dZl), (Xu, dXu, Yu, dYu, Zu, dZu) = side
    Scc = matmul_ld(Xu.T, Xl) + matmul_ld(Yu.T, Zl)
    dScc = (matmul_ld(dXu.T, np.abs(Xl)) + matmul_ld(np.abs(Xu).T, dXl) + c * (w + 2) * matmul_ld(np.abs(Xu).T, np.abs(Xl))
            + matmul_ld(dYu.T, np.abs(Zl)) + matmul_ld(np.abs(Yu).T, dZl) + c * (m + 2) * matmul_ld(np.abs(Yu).T, np.abs(Zl)))
    return Zl, dZl, Zu, dZu, Scc, dScc


def small_emulate(Tl, unit_l, Pl, Tu, unit_u, Pu, G, fault=None):
    """float64 emulation of the same chain; returns (Zl, Zu, Scc)"""
    Xl, Xu = trinv_emulate(Tl, unit_l, fault), trinv_emulate(Tu, unit_u, fault)
    Yl, Yu = Pl @ Xl, Pu @ Xu
    Zl, Zu = G @ Yl, G.T @ Yu
    return Zl, Zu, Xu.T @ Xl + Yu.T @ Zl


def logdet_bound(logs):
    """a 256-leaf tree (8 levels), then ceil(np / 256) terms per lane and the same tree; plus u |log| per term for log itself"""
    mag = np.sum(np.abs(np.asarray(logs, dtype=LD)))
    nparts = (len(logs) + 255) // 256
    return (SAFETY * (8 + (nparts + 255) // 256 + 2) + 1) * U * mag
