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
import types

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


# ---------------------------------------------------------------------------------------------------------------------
# residual, refinement, reductions, sampling and transfers, one launch at a time: tests/test_kernels_apply.py
# (csrc/sf_kernels.hip: k_resid_*, k_loadmap_drop; sf_refine.hip; sf_gram.hip, sf_gram_lu.hip; sf_sample.hip; sf_device_io.hip)
# ---------------------------------------------------------------------------------------------------------------------
GRID_CAP = 1024              # workgroups of the strided launches (QF_MAXB, DIO_MAXB, the norms launches, k_loadmap_drop)
GRAM_SLAB_ROWS, GRAM_MAX_SLABS, GRAM_STRETCH, SVM_W = 2048, 256, 64, 16
# every single fault the emulations below can inject; tests/test_kernels_apply.py shows for each that a checker rejects it
APPLY_FAULTS = ("dropped tail group", "slab overlap", "wave offset", "no mirror", "padding written", "inverse perm", "ld is n", "no stride",
                "duplicate summed", "pos from direct", "nan dropped", "map -1 read", "best overwritten")


def nan_max(a):
    """the maximum that keeps a NaN (np.max does; np.fmax.reduce is the parent's NaN-dropping one)"""
    a = np.asarray(a, dtype=np.float64)
    return float(np.max(a)) if a.size else 0.0


def strided_visit(n, per_group, fault=None):
    """(nb, passes): workgroups of a launch that caps its grid at GRID_CAP and strides over the rest, per_group elements per workgroup
    and pass.  "no stride": every workgroup makes one pass only, so elements past GRID_CAP * per_group are never visited."""
    nb = min(GRID_CAP, -(-n // per_group))
    passes = -(-n // (nb * per_group))
    return nb, (1 if fault == "no stride" else passes)


# ---- launch_residual ----
def resid_ref(n, Lp, Li, Lx, Up, Ui, Ux, x):
    """longdouble r = A x - b with b_i = 1 + i / n, per row: mag = sum |a_ij| |x_j| + |b_i| and cnt = the entries of the row;
    colsum = the column sums of |A|.  Up None: (Lp, Li, Lx) is one triangle used symmetrically; else L by column and U by row (its
    diagonal entries skipped: the L part holds the diagonal)."""
    b = 1.0 + np.arange(n, dtype=np.float64) / np.float64(n)
    rows, cols, vals = [np.asarray(Li, dtype=np.int64)], [np.repeat(np.arange(n), np.diff(Lp))], [np.asarray(Lx, dtype=np.float64)]
    if Up is None:
        off = rows[0] != cols[0]
        rows.append(cols[0][off]); cols.append(rows[0][off]); vals.append(vals[0][off])
    else:
        ur, uc = np.repeat(np.arange(n), np.diff(Up)), np.asarray(Ui, dtype=np.int64)
        off = ur != uc
        rows.append(ur[off]); cols.append(uc[off]); vals.append(np.asarray(Ux, dtype=np.float64)[off])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals).astype(LD)
    xl = np.asarray(x, dtype=LD)
    r, mag, colsum = -b.astype(LD), np.abs(b).astype(LD), np.zeros(n, dtype=LD)
    np.add.at(r, rows, vals * xl[cols])
    np.add.at(mag, rows, np.abs(vals) * np.abs(xl[cols]))
    np.add.at(colsum, cols, np.abs(vals))
    cnt = np.bincount(rows, minlength=n)
    ccnt = np.bincount(cols, minlength=n)
    return types.SimpleNamespace(b=b, r=r, mag=mag, colsum=colsum, cnt=cnt, ccnt=ccnt)


def resid_norms_emulate(r, colsum, x, b, fault=None):
    """the four maxima as k_resid_norms takes them.  "nan dropped": fmax, which returns its non-NaN operand -- the parent's maximum,
    the fault that the NaN-keeping maximum of k_resid_norms fixes; "no stride": nothing past GRID_CAP * 256 elements is visited"""
    n = len(r)
    nb, passes = strided_visit(n, 256, fault)
    lim = min(n, nb * 256 * passes)
    red = (lambda a: float(np.fmax.reduce(a, initial=0.0))) if fault == "nan dropped" else nan_max
    return np.array([red(np.abs(r[:lim])), red(colsum[:lim]), red(np.abs(x[:lim])), red(np.abs(b[:lim]))])


def resid_norms_check(norms, r, colsum, x, b, what):
    """norms[k] = the maximum of the launch's OWN r, colsum, x, b, bit for bit (a maximum does not round); a NaN among them is kept.
    Returns the residual formed from norms[] as sf_chol_plan_validate forms it."""
    for k, a in enumerate((np.abs(r), colsum, np.abs(x), np.abs(b))):
        want = nan_max(a)
        if np.isnan(want):
            if not np.isnan(norms[k]):
                raise AssertionError(f"{what}: norms[{k}] = {norms[k]!r} is beyond the bound: a NaN among its inputs was dropped")
        elif bits(np.array([norms[k]]))[0] != bits(np.array([want]))[0]:
            raise AssertionError(f"{what}: norms[{k}] = {norms[k]!r} is beyond the bound: the maximum is {want!r}")
    with np.errstate(invalid="ignore"):
        res = norms[0] / (norms[1] * norms[2] + norms[3])
    if not (np.all(np.isfinite(r)) and np.all(np.isfinite(x))) and not np.isnan(res):
        raise AssertionError(f"{what}: a non-finite r or x gives the residual {res!r}, not NaN")
    return res


def resid_check(ref, r, colsum, b, what):
    """r and colsum per element: the launch sums with floating-point atomics, so the order is free -- per row the depth is (entries
    of the row + 1) (every product and b_i enter one chain in the worst order) on mag = sum |a_ij| |x_j| + |b_i|; colsum likewise
    with the entries of the column.  b_i = 1 + i / n bit for bit.  Returns the worst err / bound."""
    if np.any(bits(b) != bits(ref.b)):
        raise AssertionError(f"{what}: b is beyond the bound: not 1 + i / n bit for bit at {np.flatnonzero(bits(b) != bits(ref.b))[:8].tolist()}")
    w1 = within_ratio(r, ref.r, SAFETY * (ref.cnt + 1) * U * ref.mag, what + " r")
    w2 = within_ratio(colsum, ref.colsum, SAFETY * np.maximum(ref.ccnt, 1) * U * ref.colsum, what + " colsum")
    return max(w1, w2)


# ---- launch_refine_resid / _abs_sums / _norms ----
RF_G = 8


def refine_emulate(ptr, col, pos, Vd, Vt, x, b, fault=None):
    """float64 emulation of k_refine_resid<false>: lane g of a row takes the entries g, g + 8, ... with fma, then xor 4, 2, 1.
    "duplicate summed": the slot after a row's first entry (a superseded duplicate, left out of the form) is summed too;
    "pos from direct": ~pos read from the direct array.  Returns (r, w)."""
    n = len(ptr) - 1
    r, w = np.empty(n), np.empty(n)
    for i in range(n):
        lanes, mags = np.zeros(RF_G), np.zeros(RF_G)
        for k, e in enumerate(range(ptr[i], ptr[i + 1])):
            ps = int(pos[e])
            a = Vd[ps] if ps >= 0 else (Vd[~ps] if fault == "pos from direct" else Vt[~ps])
            if fault == "duplicate summed" and k == 0:
                a = a + (Vd[ps + 1] if ps >= 0 else Vt[~ps + 1])
            lanes[k % RF_G] += a * x[col[e]]
            mags[k % RF_G] += abs(a) * abs(x[col[e]])
        for m in (4, 2, 1):
            lanes, mags = lanes + lanes[np.arange(RF_G) ^ m], mags + mags[np.arange(RF_G) ^ m]
        r[i], w[i] = b[i] - lanes[0], mags[0] + abs(b[i])
    return r, w


def refine_ref(ptr, col, pos, Vd, Vt, x, b):
    """longdouble (r, w, sums, depth): r = b - A x, w = |A| |x| + |b|, sums = the rows' sums of |a|; depth = the longest chain of
    additions of a row: ceil(len / 8) lane-serial fma steps, 3 xor steps, the subtraction from b_i"""
    n = len(ptr) - 1
    pos = np.asarray(pos, dtype=np.int64)
    a = np.where(pos >= 0, np.asarray(Vd)[np.maximum(pos, 0)], np.asarray(Vt)[np.maximum(~pos, 0)]).astype(LD) if len(pos) else np.zeros(0, dtype=LD)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    xl = np.asarray(x, dtype=LD)[np.asarray(col[:len(pos)], dtype=np.int64)] if len(pos) else np.zeros(0, dtype=LD)
    ax, mag, sums = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    np.add.at(ax, rows, a * xl)
    np.add.at(mag, rows, np.abs(a) * np.abs(xl))
    np.add.at(sums, rows, np.abs(a))
    bl = np.asarray(b, dtype=LD)
    depth = -(-np.diff(ptr) // RF_G) + 3 + 1
    return bl - ax, mag + np.abs(bl), sums, depth


def refine_check(ref, r, w, what):
    rr, ww, _, depth = ref
    bound = SAFETY * depth * U * ww
    return max(within_ratio(r, rr, bound, what + " r"), within_ratio(w, ww, bound, what + " w"))


def refine_norms_ref(r, w, x, b, info):
    """the five words k_refine_norms leaves in zeroed words: maxima that drop a NaN (they are bit patterns merged by an integer
    maximum; a maximum of 0 is never written), the flag word as an integer"""
    r, x, b = np.abs(r), np.abs(x), np.abs(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(w > 0, r / np.where(w > 0, w, 1.0), 0.0)
    fm = lambda a: float(np.fmax.reduce(a, initial=0.0))
    bad = not (np.all(np.isfinite(r)) and np.all(np.isfinite(x)) and np.all(np.isfinite(b)))
    return np.array([fm(q), fm(r), fm(x), fm(b)]), int(bad) | (2 if info else 0)


def refine_norms_emulate(r, w, x, b, info, s0, fault=None):
    """k_refine_norms on the five words s0 (four doubles and the flag word as an integer): workgroups stride over the rows; a maximum
    is merged into its word only when it is > 0 (integer maximum of the bit patterns of non-negative doubles).  "no stride": nothing
    past GRID_CAP * 256 rows is visited.  Returns (words, flags)."""
    n = len(r)
    nb, passes = strided_visit(n, 256, fault)
    lim = min(n, nb * 256 * passes)
    m, flags = refine_norms_ref(r[:lim], w[:lim], x[:lim], b[:lim], info)
    out = np.array(s0[0], dtype=np.float64)
    for k in range(4):
        if m[k] > 0 and bits(m[k:k + 1])[0] > bits(out[k:k + 1])[0]:
            out[k] = m[k]
    return out, int(s0[1]) | flags


def refine_update_emulate(x, d, best, save, fault=None):
    """k_refine_update: best <- x when save, then x += d.  "best overwritten": best is written although save == 0"""
    if save or fault == "best overwritten":
        best[:len(x)] = x
    x += d
    return x, best


def gather_values_emulate(Ax, map_, out, fault=None):
    """k_dev_gather_values: out[p] = Ax[map[p]], 0.0 where map[p] < 0.  "map -1 read": the entry -1 is used as an index"""
    m = np.asarray(map_)
    out[:len(m)] = Ax[m] if fault == "map -1 read" else np.where(m >= 0, Ax[np.maximum(m, 0)], 0.0)
    return out


# ---- the fixed-order sums: launch_dot, launch_quadform ----
def two_pass_sum(terms, W, fault=None):
    """float64 emulation of k_dot_part / _final (W = 1, terms = x_i y_i) and k_quadform_part / _final<W> (terms = the row-major
    n x W block of squares): G = 256 / W row groups per workgroup, nb = min(GRID_CAP, ceil(n / G)) workgroups striding over the rows
    serially, a tree over the groups, then one workgroup over the nb parts in the same way.  Returns the W sums."""
    def tree(v):                # v: (..., G, W)
        while v.shape[-2] > 1:
            h = v.shape[-2] // 2
            v = v[..., :h, :] + v[..., h:, :]
        return v[..., 0, :]
    terms = np.asarray(terms, dtype=np.float64).reshape(-1, W)
    n, G = terms.shape[0], 256 // W
    nb, passes = strided_visit(n, G, fault)
    pad = np.zeros((nb * G * passes, W))
    lim = min(n, len(pad))
    pad[:lim] = terms[:lim]
    v = np.zeros((nb, G, W))
    for t in pad.reshape(passes, nb, G, W):
        v = v + t
    part = tree(v)                                       # nb x W
    p2 = -(-nb // G)
    pad2 = np.zeros((p2 * G, W))
    pad2[:nb] = part
    v = np.zeros((G, W))
    for t in pad2.reshape(p2, G, W):
        v = v + t
    return tree(v)


def two_pass_depth(n, W):
    """the longest chain of additions behind one result of two_pass_sum: the products' own rounding (1), ceil(n / (nb G)) serial
    steps, log2(G) tree levels; then ceil(nb / G) serial steps and the same tree"""
    G = 256 // W
    nb, passes = strided_visit(n, G)
    lv = G.bit_length() - 1
    return 1 + passes + lv + -(-nb // G) + lv


def sum_check(got, terms, W, what):
    """got (W sums) against the longdouble column sums of `terms` (n x W) within SAFETY depth u sum |terms|"""
    t = np.asarray(terms, dtype=LD).reshape(-1, W)
    return within_ratio(np.asarray(got), t.sum(axis=0), SAFETY * two_pass_depth(t.shape[0], W) * U * np.abs(t).sum(axis=0), what)


# ---- the Gram reductions: launch_gram_row, launch_gram2_col ----
def gram_slabs(n):
    """(ns, slab_rows) as sf::gram_slabs cuts the rows"""
    want = min(GRAM_MAX_SLABS, max(1, -(-n // GRAM_SLAB_ROWS)))
    rows = -(-(-(-n // want)) // GRAM_STRETCH) * GRAM_STRETCH
    return -(-n // rows), rows


def gram_depth(n):
    """the longest chain of additions behind one entry of G: a slab has slab_rows / 64 stretches, an accumulator chain takes one
    four-row group of each (4 products per MFMA: slab_rows / 16 additions), the four chains are added pairwise (2), the four
    waves in order (3), the ns slabs in order (ns), and each product rounds once (1)"""
    ns, rows = gram_slabs(n)
    return rows // 16 + 2 + 3 + ns + 1


def gram_tile_emulate(Ya, Yb, fault=None):
    """float64 emulation of one 16 x 16 tile Ya^T Yb (n x 16 each) in the kernels' order: slab by slab; in a slab wave w and chain u
    take the four-row groups at 4 w + 16 u of every 64-row stretch.  Faults: the last partial four-row group of a slab dropped; the
    first row of the next slab counted in both; wave 1's groups one stretch late (its first stretch is never read)."""
    n = Ya.shape[0]
    ns, rows = gram_slabs(n)
    out = np.zeros((SVM_W, SVM_W))
    for s in range(ns):
        r0, r1 = s * rows, min(n, (s + 1) * rows)
        if fault == "slab overlap" and r1 < n:
            r1 += 1
        if fault == "dropped tail group":
            r1 -= (r1 - r0) % 4
        A, B = np.zeros((-(-(r1 - r0) // 64) * 64, SVM_W)), np.zeros((-(-(r1 - r0) // 64) * 64, SVM_W))
        A[:r1 - r0], B[:r1 - r0] = Ya[r0:r1], Yb[r0:r1]
        A, B = A.reshape(-1, 4, 4, 4, SVM_W), B.reshape(-1, 4, 4, 4, SVM_W)          # stretch, chain u, wave w, row of the group
        if fault == "wave offset":
            A = A.copy()
            A[0, :, 1] = 0.0
        acc = np.zeros((4, 4, SVM_W, SVM_W))
        for t in range(A.shape[0]):
            acc = acc + np.einsum("uwqi,uwqj->uwij", A[t], B[t])
        wave = (acc[0] + acc[1]) + (acc[2] + acc[3])
        part = wave[0]
        for w in range(1, 4):
            part = part + wave[w]
        out = out + part
    return out


def gram_row_emulate(Y, n, a, k, G, fault=None):
    """launch_gram_row on the chunks Y[0 .. a] (each n x 16) into the column-major k x k G (a 2-D array, G[i, j], any leading
    dimension >= k): the tiles (a, b <= a) and their mirrors; a diagonal tile mirrors its lower triangle from one value.
    Faults: an off-diagonal tile's mirror not written; the indices >= k written."""
    for b in range(a + 1):
        T = gram_tile_emulate(Y[a], Y[b], fault)
        for i in range(SVM_W):
            for j in range(SVM_W):
                gi, gj = a * SVM_W + i, b * SVM_W + j
                lim = G.shape[0] if fault == "padding written" else k
                if gi >= lim or gj >= lim or gj >= G.shape[1] or (a == b and i < j):
                    continue
                G[gi, gj] = T[i, j]
                if gi != gj and not (fault == "no mirror" and a != b) and gi < G.shape[1]:
                    G[gj, gi] = T[i, j]
    return G


def gram2_col_emulate(Z, Yb, n, b, m, k, G, fault=None):
    """launch_gram2_col: the tiles (a < nza, b) of Z^T Y into the column-major m x k G; nothing mirrored"""
    for a in range(len(Z)):
        T = gram_tile_emulate(Z[a], Yb, fault)
        for i in range(SVM_W):
            for j in range(SVM_W):
                gi, gj = a * SVM_W + i, b * SVM_W + j
                if fault == "padding written":
                    if gi < G.shape[0] and gj < G.shape[1]:
                        G[gi, gj] = T[i, j]
                elif gi < m and gj < k:
                    G[gi, gj] = T[i, j]
    return G


def gram_check(G0, G1, Zc, Yc, n, rows_of, cols_of, m, k, mirror, what):
    """G1 (after) against G0 (before), both 2-D [row, column] views with the padding of the leading dimension as extra rows.
    Written: entry (16 a + i, 16 b + j) for the (a, b) tiles of the launch -- rows_of / cols_of = the chunk indices, Zc[a] / Yc[b] the
    n x 16 chunks -- with row < m and column < k; mirror: also the transposed entry, and the two must agree bit for bit.
    Each against the longdouble sum within SAFETY gram_depth(n) u sum |terms|; everything else bit-identical.  Returns the worst ratio."""
    written = np.zeros(G0.shape, dtype=bool)
    worst = 0.0
    depth = gram_depth(n)
    for a in rows_of:
        for b in cols_of(a):
            ref = matmul_ld(np.asarray(Zc[a]).T, Yc[b])
            bound = SAFETY * depth * U * matmul_ld(np.abs(np.asarray(Zc[a])).T, np.abs(Yc[b]))
            ni, nj = max(0, min(SVM_W, m - a * SVM_W)), max(0, min(SVM_W, k - b * SVM_W))
            got = G1[a * SVM_W:a * SVM_W + ni, b * SVM_W:b * SVM_W + nj]
            written[a * SVM_W:a * SVM_W + ni, b * SVM_W:b * SVM_W + nj] = True
            worst = max(worst, within_ratio(got, ref[:ni, :nj], bound[:ni, :nj], f"{what} tile ({a}, {b})"))
            if mirror:
                written[b * SVM_W:b * SVM_W + nj, a * SVM_W:a * SVM_W + ni] = True
                back = G1[b * SVM_W:b * SVM_W + nj, a * SVM_W:a * SVM_W + ni].T
                if np.any(bits(back) != bits(np.ascontiguousarray(got))):
                    raise AssertionError(f"{what} tile ({a}, {b}): beyond the bound: the mirror differs from the tile")
    assert_unchanged(G0, G1, written, what)
    return worst


# ---- the transfers of sf_device_io.hip ----
def _perm_index(perm, n, fault):
    if perm is None:
        return np.arange(n)
    return np.argsort(perm) if fault == "inverse perm" else np.asarray(perm)


def load1_emulate(B, perm, n, x, fault=None):
    x[:n] = B[_perm_index(perm, n, fault)]
    return x


def store1_emulate(x, perm, n, X, fault=None):
    X[_perm_index(perm, n, fault)] = x[:n]
    return X


def pack_emulate(B, ldb, perm, n, cw, X, fault=None):
    """X (flat, row-major n x 16 in front) from the column-major chunk B (flat, leading dimension ldb); columns >= cw zero"""
    src = _perm_index(perm, n, fault)
    ld = n if fault == "ld is n" else ldb
    blk = np.zeros((n, SVM_W))
    for c in range(cw):
        blk[:, c] = B[src + c * ld]
    if fault == "padding written" and cw < SVM_W:
        blk[:, cw] = B[src]
    X[:n * SVM_W] = blk.ravel()
    return X


def unpack_emulate(X, perm, n, cw, D, ldx, fault=None):
    dst = _perm_index(perm, n, fault)
    ld = n if fault == "ld is n" else ldx
    blk = X[:n * SVM_W].reshape(n, SVM_W)
    for c in range(cw + (1 if fault == "padding written" and cw < SVM_W else 0)):
        D[dst + c * ld] = blk[:, c]
    return D


def assert_bits(got, want, what):
    bad = bits(np.asarray(got, dtype=np.float64)) != bits(np.asarray(want, dtype=np.float64))
    if bad.any():
        raise AssertionError(f"{what}: {int(bad.sum())} elements are beyond the bound (bit for bit), first at {np.argwhere(bad)[:8].tolist()}")


def absmax_emulate(v, fault=None):
    """the parts of k_dev_absmax: workgroup blk strides over v; fmax drops a NaN, as documented"""
    n = len(v)
    nb, passes = strided_visit(n, 256, fault)
    pad = np.zeros(nb * 256 * passes)
    lim = min(n, len(pad))
    pad[:lim] = np.abs(v[:lim])
    return np.fmax.reduce(pad.reshape(passes, nb, 256), axis=(0, 2), initial=0.0)


def loadmap_drop_emulate(drop, map_, fault=None):
    nb, passes = strided_visit(len(drop), 256, fault)
    map_[drop[:nb * 256 * passes]] = -1
    return map_


# ---------------------------------------------------------------------------------------------------------------------
# Sigma on the pattern of A, one launch at a time (csrc/sf_selinv_pattern.hip): tests/test_kernels_selpat.py
# ---------------------------------------------------------------------------------------------------------------------
SELPAT_TILE, SELPAT_EPT, SELPAT_CHUNK, SELPAT_GATHER_GRID = 2048, 8, 8, 4096     # sf_kernels.h
# depth of one part: the lane's 8 fused multiply-adds, 6 shuffle levels, 2 additions of the four waves' sums (the weight 2 is exact)
SELPAT_PART_DEPTH = SELPAT_EPT + 6 + 2
# every single fault the emulations below can inject; tests/test_kernels_selpat.py shows for each that a checker rejects it
SELPAT_FAULTS = ("weight everywhere", "dead entry read", "tail lane dropped", "part0 ignored", "stride is own tiles", "column past m",
                 "shift ignored", "vmap ignored", "first 256 parts", "32-bit product", "diagonal row searched", "offd inverted", "no end guard",
                 "triangle swapped", "counter reset", "gather no stride")


def selpat_tiles(count):
    return -(-max(int(count), 0) // SELPAT_TILE)


def selpat_final_depth(nparts):
    """the longest chain of additions behind one result of k_selpat_final: ceil(nparts / 256) serial steps, 8 tree levels"""
    return -(-int(nparts) // 256) + 8


def _wrap32(v):
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def selpat_build_emulate(tb, Lp, Li, pos, offd, fault=None):
    """k_selpat_build on the structure tb (SelTables): pos[p] = Xp[s] + (j - c0) nsrow + (the row's position in the supernode's row
    list) for every entry p of column j, offd[p] = (row != j) when offd is given.  Columns without entries are skipped, as a lane
    with an empty loop is.  Faults: "32-bit product" -- (j - c0) nsrow wraps as a signed 32-bit product; "diagonal row searched" -- the
    nscol offset is missing for a row below the diagonal block; "offd inverted" -- the diagonal is marked instead."""
    for j in np.flatnonzero(np.diff(Lp)):
        j = int(j)
        s = int(tb.SuperMap[j])
        c0, c1 = int(tb.Super[s]), int(tb.Super[s + 1])
        nsrow, nscol = tb.nsrow(s), c1 - c0
        prod = (j - c0) * nsrow
        col = int(tb.Xp[s]) + (_wrap32(prod) if fault == "32-bit product" else prod)
        below = tb.rows(s)[nscol:]
        for p in range(int(Lp[j]), int(Lp[j + 1])):
            i = int(Li[p])
            if i < c1:
                si = i - c0
            else:
                si = (0 if fault == "diagonal row searched" else nscol) + int(np.searchsorted(below, i))
            pos[p] = col + si
            if offd is not None:
                offd[p] = (i == j) if fault == "offd inverted" else (i != j)
    return pos, offd


def selpat_gather_emulate(pos, count, S, out, fault=None):
    """k_selpat_gather: out[p] = S[pos[p]], p < count.  "gather no stride": the 4096 workgroups make one pass only"""
    lim = min(count, SELPAT_GATHER_GRID * 256) if fault == "gather no stride" else count
    out[:lim] = S[pos[:lim]]
    return out


def selpat_part_emulate(buf, mapped, map_, offd, vmap, count, s_off, shift, v_off, ldv, m, part_off, part0, nparts, fault=None):
    """k_selpat_part on the image buf, in float64 and in the documented order: lane tid of tile b sums its entries b 2048 + tid + 256 e
    in order of e (s v + acc rounded twice here, fused in the kernel -- the checkers bound the sum, they do not ask for its bits), a
    6-level halving tree over the wave's 64 lanes, then (w0 + w1) + (w2 + w3).  Returns the number of tiles.  Faults: see SELPAT_FAULTS
    and the table of tests/test_kernels_selpat.py."""
    if count <= 0:
        return 0
    nt = selpat_tiles(count)
    n_used = count // 256 * 256 if fault == "tail lane dropped" else count
    pad = nt * SELPAT_TILE
    p = np.arange(pad)
    q = np.full(pad, -1, dtype=np.int64)
    q[:n_used] = map_[:n_used]
    live = q >= 0
    if fault == "dead entry read":
        live = p < n_used
    sh = 0 if fault == "shift ignored" else shift
    s = np.where(live, buf[np.where(live, s_off + q + sh, 0)], 0.0)
    if offd is not None:
        w = np.zeros(pad, dtype=bool)
        w[:count] = np.asarray(offd[:count]) != 0
        s = np.where(live & (w | (fault == "weight everywhere")), 2.0 * s, s)
    if mapped and fault != "vmap ignored":
        vq = np.full(pad, -1, dtype=np.int64)
        vq[:count] = vmap[:count]
        vq = np.where(live, vq, -1)
    else:
        vq = np.where(live, p, -1)
    has_v = vq >= 0
    shape = (nt, SELPAT_EPT, 256)
    s, vq, has_v = s.reshape(shape), vq.reshape(shape), has_v.reshape(shape)
    stride = nt if fault == "stride is own tiles" else nparts
    first = 0 if fault == "part0 ignored" else part0
    ncol = -(-m // SELPAT_CHUNK) * SELPAT_CHUNK if fault == "column past m" else m
    for t in range(ncol):
        acc = np.zeros((nt, 256))
        if t < m:
            for e in range(SELPAT_EPT):
                v = buf[np.where(has_v[:, e], v_off + vq[:, e] + t * ldv, 0)]
                acc = np.where(has_v[:, e], s[:, e] * v + acc, acc)
        wv = acc.reshape(nt, 4, 64)
        h = 32
        while h:
            wv = wv[..., :h] + wv[..., h:2 * h]
            h //= 2
        wv = wv[..., 0]
        buf[part_off + t * stride + first + np.arange(nt)] = (wv[:, 0] + wv[:, 1]) + (wv[:, 2] + wv[:, 3])
    return nt


def selpat_final_emulate(buf, part_off, nparts, m, out_off, fault=None):
    """k_selpat_final: per column lane k sums the parts k, k + 256, ... in order, then a halving tree over the 256 lanes.
    "first 256 parts": one trip only"""
    trips = 1 if fault == "first 256 parts" else -(-nparts // 256)
    for t in range(m):
        col = np.zeros(trips * 256)
        lim = min(nparts, trips * 256)
        col[:lim] = buf[part_off + t * nparts:part_off + t * nparts + lim]
        v = np.zeros(256)
        for row in col.reshape(trips, 256):
            v = v + row
        h = 128
        while h:
            v = v[:h] + v[h:2 * h]
            h //= 2
        buf[out_off + t] = v[0]
    return buf


def selpat_entries_emulate(tb, rows, cols, count, lu, xC, buf, s_off, out_off, outside, fault=None):
    """k_selpat_entries: out[k] = Sigma(rows[k], cols[k]) by the search of the walk, NaN outside the pattern; returns the counter.
    Faults: "no end guard" -- the search's result is compared without b < nb (what lies behind the supernode's rows in Lsi is read;
    behind the end of Lsi: not found); "diagonal row searched"; "triangle swapped" -- LU i < j is read from the first arena;
    "counter reset" -- the counter is overwritten with this launch's count"""
    nout = 0
    for k in range(count):
        i, j = int(rows[k]), int(cols[k])
        col, row = min(i, j), max(i, j)
        s = int(tb.SuperMap[col])
        c0, c1 = int(tb.Super[s]), int(tb.Super[s + 1])
        nsrow, nscol = tb.nsrow(s), c1 - c0
        nb = nsrow - nscol
        si, found = row - c0, True
        if row >= c1:
            start = int(tb.Lsip[s]) + nscol
            b = int(np.searchsorted(tb.Lsi[start:start + nb], row))
            if fault == "no end guard":
                found = start + b < len(tb.Lsi) and int(tb.Lsi[start + b]) == row
            else:
                found = b < nb and int(tb.Lsi[start + b]) == row
            si = (0 if fault == "diagonal row searched" else nscol) + b
        if not found:
            buf[out_off + k] = np.nan
            nout += 1
            continue
        off = int(tb.Xp[s]) + (col - c0) * nsrow + si
        second = lu and i < j and fault != "triangle swapped"
        buf[out_off + k] = buf[s_off + off + (xC if second else 0)]
    return nout if fault == "counter reset" else outside + nout
