"""Extended-precision references and per-element error bounds for the single-launch kernel tests (tests/test_kernels.py).

References are computed in np.longdouble (64-bit mantissa on x86-64: 11 more bits than fp64), so the reference's own
rounding is far below the bounds.  Every bound is per ELEMENT, of the form the algorithm satisfies in fp64
(u = 2^-53, SAFETY = small constant for the fused / reordered summations):
    GEMM / update  |C^ - C|       <= SAFETY (K + 2) u (|C0| + |Y| |X|^T)
    POTRF          |A - L^ L^T|   <= SAFETY (b + 2) u |L^| |L^T|
    GETRF          |PA - L^ U^|   <= SAFETY (b + 2) u |L^| |U^|
    TRSM           |X^ D^T - B|   <= SAFETY (b + 2) u |X^| |D^T|
    solve sweeps   |sum of an equation's terms - its right-hand side| <= SAFETY (terms) u (sum of the terms' magnitudes)
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
    sum of their magnitudes (|rhs| among them where rhs is itself a summand).  Only the columns `cols` are checked (the others may hold a planted NaN)."""
    total, mag = np.asarray(total, dtype=LD)[:, cols], np.asarray(mag, dtype=LD)[:, cols]
    rhs = np.asarray(rhs, dtype=LD)[:, cols]
    if not np.all(np.isfinite(total)):
        raise AssertionError(f"{what}: non-finite stored results at {np.argwhere(~np.isfinite(total))[:8].tolist()}")
    err = np.abs(total - rhs)
    bound = SAFETY * np.asarray(nterms, dtype=LD).reshape(-1, 1) * U * mag
    viol = err > bound
    if viol.any():
        k = tuple(np.argwhere(viol)[0])
        raise AssertionError(f"{what}: {int(viol.sum())} of {viol.size} equations beyond the bound, first at {list(k)} "
                             f"(err {float(err[k]):.3e}, bound {float(bound[k]):.3e})")
