"""sf_lu_plan_solve_transposed / sf_lu_plan_solve_many_transposed (LUPlan.solve / solve_many with trans=True): x = A^-T b with the
resident LU factor, column by column against tests/lu_trans_ref.lu_solve_t on the plan's OWN downloaded factor and pivots (same
inputs, so the comparison isolates the sweeps from the factor's conditioning).  The reference is pinned on the CPU in
tests/test_lu_trans_ref.py."""
import numpy as np
import pytest

from util import sf, gen, nd_perm_py, small_cases
from test_lu_pivot import pivot_cases, _dense_csc
from lu_selinv_ref import device_panels
from lu_trans_ref import lu_solve_t
import refine_ref as RR

pytestmark = pytest.mark.gpu

W = 16
KS = (1, 3, W, W + 1, 2 * W + 5)
ULP = 1.1102230246251565e-16


def _plan(S, tol=0.0):
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, None if S.symmetric else S.Ux)
    if tol > 0:
        plan.set_pivoting(tol)
    plan.factorize()
    return plan


class _Ref:
    """lu_solve_t on one plan's factor (the panels are unpacked once)"""

    def __init__(self, S, plan, pivoting):
        self.S, self.Lsx = S, plan.get_factor().copy()
        self.piv = plan.get_pivots() if pivoting else None
        self.panels = device_panels(S, self.Lsx)

    def __call__(self, b):
        self.b = b
        return lu_solve_t(self.S, self.Lsx, self.piv, b, self.panels)

    def spread(self, rng, want):
        """how far the REFERENCE's solution of the last right-hand sides moves when every entry of the factor moves by one ulp at
        random, per column, relative to the column's largest entry (the yardstick of tests/test_lu_pivot.py and
        test_solve_many.py::test_lu_with_pivoting)"""
        out = np.zeros(want.shape[1])
        for _ in range(5):
            moved = self.Lsx * (1.0 + rng.integers(-1, 2, self.Lsx.size) * ULP)
            d = np.abs(lu_solve_t(self.S, moved, self.piv, self.b) - want)
            out = np.maximum(out, d.max(axis=0) / np.abs(want).max(axis=0))
        return out


def _both_entry_points(plan, ref, n, rng):
    """(B, X, reference) of the single-column entry point, then of the blocked one for every k.  One block of right-hand sides and
    ONE reference solve serve all of them: the single column is its first, the block of k its first k."""
    Bfull = rng.standard_normal((n, max(KS)))
    want = ref(Bfull)
    b = np.ascontiguousarray(Bfull[:, 0])
    yield b, plan.solve(b, trans=True), want[:, 0], want
    for k in KS:
        B = Bfull[:, :k]
        X = plan.solve_many(B, trans=True)
        assert X.shape == (n, k) and X.dtype == np.float64
        yield B, X, want[:, :k], want


def _check_close(plan, ref, n, rng, rtol, atol_rel):
    for B, X, want, _ in _both_entry_points(plan, ref, n, rng):
        for j in range(1 if B.ndim == 1 else B.shape[1]):
            x, w = (X, want) if B.ndim == 1 else (X[:, j], want[:, j])
            err = np.abs(x - w).max() / np.abs(w).max()
            assert np.allclose(x, w, rtol=rtol, atol=atol_rel * np.abs(w).max()), (B.shape, j, err)


def _check_spread(plan, ref, n, rng, name):
    """err <= max(1e-12, 8 x spread); the blocked entry point also gets what the one-column device solve itself is off by on that
    column, as in test_solve_many.py::test_lu_with_pivoting"""
    spread = None
    for B, X, want, want_full in _both_entry_points(plan, ref, n, rng):
        if spread is None:
            spread = ref.spread(rng, want_full)
            print(name, "max spread", spread.max())
        if B.ndim == 1:
            err = float(np.abs(X - want).max() / np.abs(want).max())
            print(name, "single", "err", err, "spread", spread[0])
            assert err <= max(1e-12, 8.0 * spread[0]), (name, err, spread[0])
            continue
        for j in range(B.shape[1]):
            wmax = np.abs(want[:, j]).max()
            err = float(np.abs(X[:, j] - want[:, j]).max() / wmax)
            bound = max(1e-12, 8.0 * spread[j])
            if err > bound:
                err1 = float(np.abs(plan.solve(np.ascontiguousarray(B[:, j]), trans=True) - want[:, j]).max() / wmax)
                bound = max(bound, 8.0 * err1)
            assert err <= bound, (name, B.shape[1], j, err, spread[j])


def _stencil(N, seed=5):
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=seed)
    return sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 4 << 30, "lu", False)


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_small_cases_as_lu(case):
    """symmetric inputs through an LU plan (U aliases L): the narrow-supernode kernels and the general kernels without BIG.
    Also without a reference: the backward error of A^T x = b in longdouble."""
    name, n, Cp, Ci, Cx, perm, slot = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", True)
    plan = _plan(S)
    rng = np.random.default_rng(1)
    _check_close(plan, _Ref(S, plan, False), n, rng, 1e-12, 1e-13)
    A, _ = RR.dense_ld(n, *RR.matrix_coo(S))
    m = np.count_nonzero(A, axis=0)              # entries per row of A^T
    b = rng.standard_normal(n)
    _, _, berr, _ = RR.residual_ld(A.T, plan.solve(b, trans=True), b)
    print(name, "berr", berr, "floor", RR.floor(m))
    assert berr <= 8 * RR.floor(m), (name, berr)
    plan.close()


@pytest.mark.parametrize("N", [6, 8, 10, 12])
def test_unsymmetric_stencils(N):
    S = _stencil(N)
    plan = _plan(S)
    rng = np.random.default_rng(2)
    _check_close(plan, _Ref(S, plan, False), S.n, rng, 1e-12, 1e-13)
    A, _ = RR.dense_ld(S.n, *RR.matrix_coo(S))
    m = np.count_nonzero(A, axis=0)
    b = rng.standard_normal(S.n)
    _, _, berr, _ = RR.residual_ld(A.T, plan.solve(b, trans=True), b)
    print(N, "berr", berr, "floor", RR.floor(m))
    assert berr <= 8 * RR.floor(m), (N, berr)
    plan.close()


def test_wide_supernodes_34cubed():
    """a supernode wider than 1024 columns: BIG tasks, far tiles of several row groups, the row-major diagonal copies made from the
    L panels.  solve / solve_transposed / solve on one plan: neither sees the other's copies.  And y^T (A^-1 b) = (A^-T y)^T b."""
    S = _stencil(34)
    assert np.diff(S.Super).max() > 1024
    plan = _plan(S)
    n = S.n
    rng = np.random.default_rng(3)
    _check_close(plan, _Ref(S, plan, False), n, rng, 1e-11, 1e-12)
    b, y = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    x1 = plan.solve(b)
    xt = plan.solve(y, trans=True)
    x2 = plan.solve(b)
    assert np.allclose(x1, x2, rtol=1e-13, atol=1e-13 * np.abs(x1).max())
    lhs, rhs = float(y @ x1), float(xt @ b)
    print("y'(A^-1 b)", lhs, "(A^-T y)'b", rhs)
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))
    # the blocked entry points the same way
    B = rng.uniform(0.5, 1.5, (n, 3))
    X1 = plan.solve_many(B)
    plan.solve_many(B, trans=True)
    X2 = plan.solve_many(B)
    assert np.allclose(X1, X2, rtol=1e-13, atol=1e-13 * np.abs(X1).max())
    plan.close()


def _edge_cases():
    rng = np.random.default_rng(12)
    c = [("dense_700", *_dense_csc(rng.uniform(-1, 1, (700, 700)) + 20 * np.eye(700)), None)]
    c += [p[:6] for p in pivot_cases() if p[0].startswith("blockdiag_700_130_577_65")]
    return c


@pytest.mark.parametrize("case", _edge_cases(), ids=lambda c: c[0])
def test_edge_widths_without_pivoting(case):
    """one dense supernode of 700 columns (its last step has 188, its last wave 60) and panels of 700, 130, 577 and 65 columns in
    one level; no interchanges.  Dense triangles of this size amplify the rounding of another summation order by their own
    condition: the bound is the measured one-ulp spread of the reference."""
    name, n, Cp, Ci, Cx, perm = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    assert sorted(np.diff(S.Super).tolist()) == sorted(int(k) for k in name.split("_")[1:] if k.isdigit())
    plan = _plan(S)
    _check_spread(plan, _Ref(S, plan, False), n, np.random.default_rng(4), name)
    plan.close()


PIVOTED = ("dense_200_tol01", "zero_diag_12", "general_14_tol03", "blockdiag_700_130_577_65_tol03")


@pytest.mark.parametrize("case", [c for c in pivot_cases() if c[0] in PIVOTED], ids=lambda c: c[0])
def test_with_pivoting(case):
    name, n, Cp, Ci, Cx, perm, tol, vtol = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    plan = _plan(S, tol)
    assert np.count_nonzero(plan.get_pivots() != np.arange(n)) > 0
    _check_spread(plan, _Ref(S, plan, True), n, np.random.default_rng(5), name)
    plan.close()


def test_symmetric_input_transposed_is_the_plain_solve():
    N = 12
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    S = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", True)
    plan = _plan(S)
    b = np.random.default_rng(6).standard_normal(n)
    x, xt = plan.solve(b), plan.solve(b, trans=True)
    assert np.allclose(xt, x, rtol=1e-12, atol=1e-12 * np.abs(x).max())
    plan.close()


def test_column_independence():
    """a NaN column stays in its column.  Bit for bit on a front of one step (dense_200 with its interchanges: one diagonal task,
    no tile adds to x, so the summation order is fixed); on a sparse matrix the tiles' atomics land in an order that differs from
    run to run, so there the clean columns are compared to rounding, as test_solve_many.py::test_column_independence does."""
    name, n, Cp, Ci, Cx, perm, tol, _ = [c for c in pivot_cases() if c[0] == "dense_200_tol01"][0]
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    plan = _plan(S, tol)
    B = np.random.default_rng(7).standard_normal((n, W))
    clean = plan.solve_many(B, trans=True)
    Bn = B.copy()
    Bn[n // 2, 3] = np.nan
    X = plan.solve(Bn, trans=True)               # a 2-D b takes the blocked path
    assert X.shape == (n, W)
    assert not np.isfinite(X[:, 3]).all()
    keep = [j for j in range(W) if j != 3]
    assert np.array_equal(X[:, keep], clean[:, keep])
    plan.close()
    S = _stencil(12)
    plan = _plan(S)
    n = S.n
    B = np.random.default_rng(8).standard_normal((n, W + 4))
    clean = plan.solve_many(B, trans=True)
    Bn = B.copy()
    Bn[n // 2, 3] = np.nan
    Bn[7, W + 1] = np.inf
    Bn[:, 5] = 0.0
    X = plan.solve_many(Bn, trans=True)
    assert np.all(X[:, 5] == 0.0)
    assert not np.isfinite(X[:, 3]).all() and not np.isfinite(X[:, W + 1]).all()
    for j in range(W + 4):
        if j not in (3, 5, W + 1):
            assert np.allclose(X[:, j], clean[:, j], rtol=1e-13, atol=1e-13 * np.abs(clean[:, j]).max()), j
    plan.close()


def test_layouts_and_stats():
    import ctypes as C
    S = _stencil(8)
    plan = _plan(S)
    n, k = S.n, W + 2
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    B = np.random.default_rng(9).standard_normal((n, k))
    ref = plan.solve_many(np.asfortranarray(B), trans=True)
    same = lambda X: np.allclose(X, ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
    assert same(plan.solve_many(np.ascontiguousarray(B), trans=True))
    ldb, ldx = n + 5, n + 11
    Bp = np.full((ldb, k), 7.0, order="F")
    Bp[:n] = B
    Xp = np.full((ldx, k), -3.0, order="F")
    assert sf.lib.sf_lu_plan_solve_many_transposed(plan._h, k, dp(Bp), ldb, dp(Xp), ldx) == 0
    assert same(Xp[:n]) and np.all(Xp[n:] == -3.0)
    x1 = np.full(ldx, -3.0)
    assert sf.lib.sf_lu_plan_solve_many_transposed(plan._h, 1, dp(Bp), ldb, dp(x1), ldx) == 0       # one column of the padded block
    assert same(np.column_stack([x1[:n], ref[:, 1:]])) and np.all(x1[n:] == -3.0)
    Bi = np.asfortranarray(B.copy())
    assert sf.lib.sf_lu_plan_solve_many_transposed(plan._h, k, dp(Bi), n, dp(Bi), n) == 0      # in place
    assert same(Bi)
    assert plan.solve_many(np.empty((n, 0)), trans=True).shape == (n, 0)
    assert plan.stat("last_solve_many_ms") > 0
    plan.solve(B[:, 0].copy(), trans=True)
    assert plan.stat("last_solve_ms") > 0
    # a plan whose last factorization failed is refused, as refine refuses it
    plan.set_values(S.Lx * 0.0, S.Ux * 0.0)
    with pytest.raises(sf.SparseFrameError):
        plan.factorize()
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
        plan.solve(B[:, 0].copy(), trans=True)
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
        plan.solve_many(B, trans=True)
    plan.close()
    # a Cholesky plan has no transposed entry point
    n, Cp, Ci, Cx = gen.laplacian_lower(6, 6, 6)
    Sc = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(6, 6, 6), 1 << 30)
    cp = sf.CholPlan(Sc)
    cp.set_values(Sc.Lx)
    cp.factorize()
    x = np.ones(n)
    assert sf.lib.sf_lu_plan_solve_transposed(cp._h, dp(x), dp(x)) == 1
    cp.close()
