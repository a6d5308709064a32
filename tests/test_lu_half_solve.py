"""sf_lu_plan_solve_half (LUPlan.half_solve): the four halves of the solves with a resident LU factor -- F B ("L"), U^-1 B ("U"),
U^-T B ("Ut"), F^T B ("Lt") -- column by column against tests/lu_half_ref.py on the plan's OWN downloaded factor and pivots (same
inputs, so the comparison isolates the sweeps from the factor's conditioning).  The reference is pinned on the CPU in
tests/test_lu_half_ref.py.  Tolerances: those of tests/test_lu_transposed.py, whose kernels these are."""
import ctypes as C

import numpy as np
import pytest

import lu_half_ref as R
from test_lu_pivot import pivot_cases
from util import sf, gen, nd_perm_py, small_cases

pytestmark = pytest.mark.gpu

W = 16
KS = (1, 3, W, W + 1)
WHICH = ("L", "U", "Ut", "Lt")
ULP = 1.1102230246251565e-16
SF_OK, SF_ERR_ARG = 0, 1


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _plan(S, tol=0.0):
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, None if S.symmetric else S.Ux)
    if tol > 0:
        plan.set_pivoting(tol)
    plan.factorize()
    return plan


def _factor(S, plan, pivoting=False):
    return R.Factor(S, plan.get_factor().copy(), plan.get_pivots() if pivoting else None)


def _stencil(N, seed=5):
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=seed)
    return sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 4 << 30, "lu", False)


def _calls(plan, Bfull, which):
    """(k, X as (n, k)) of the 1-D call and of the blocked one for every k: one block of right-hand sides serves all of them"""
    x = plan.half_solve(np.ascontiguousarray(Bfull[:, 0]), which)
    assert x.shape == (Bfull.shape[0],) and x.dtype == np.float64
    yield 0, x.reshape(-1, 1)
    for k in KS:
        X = plan.half_solve(Bfull[:, :k], which)
        assert X.shape == (Bfull.shape[0], k) and X.dtype == np.float64
        yield k, X


def _check_close(plan, F, n, rng, rtol, atol_rel, name):
    Bfull = rng.standard_normal((n, max(KS)))
    for which in WHICH:
        want = R.half(F, Bfull, which)          # ONE reference sweep per half
        for k, X in _calls(plan, Bfull, which):
            for j in range(X.shape[1]):
                w = want[:, j]
                err = np.abs(X[:, j] - w).max() / np.abs(w).max()
                assert np.allclose(X[:, j], w, rtol=rtol, atol=atol_rel * np.abs(w).max()), (name, which, k, j, err)


def _check_spread(plan, S, F, n, rng, name):
    """err <= max(1e-12, 8 x spread), spread = how far the REFERENCE's result moves when every entry of the factor moves by one ulp
    at random, per column, relative to the column's largest entry; the blocked entry point also gets what the one-column device
    sweep itself is off by on that column -- tests/test_lu_transposed.py::_check_spread"""
    Bfull = rng.standard_normal((n, max(KS)))
    Lsx = plan.get_factor().copy()
    moved = [R.Factor(S, Lsx * (1.0 + rng.integers(-1, 2, Lsx.size) * ULP), F.piv) for _ in range(5)]
    for which in WHICH:
        want = R.half(F, Bfull, which)
        wmax = np.abs(want).max(axis=0)
        spread = np.zeros(Bfull.shape[1])
        for Fm in moved:
            spread = np.maximum(spread, np.abs(R.half(Fm, Bfull, which) - want).max(axis=0) / wmax)
        print(name, which, "max spread", spread.max())
        for k, X in _calls(plan, Bfull, which):
            for j in range(X.shape[1]):
                err = float(np.abs(X[:, j] - want[:, j]).max() / wmax[j])
                bound = max(1e-12, 8.0 * spread[j])
                if k > 0 and err > bound:
                    x1 = plan.half_solve(np.ascontiguousarray(Bfull[:, j]), which)
                    bound = max(bound, 8.0 * float(np.abs(x1 - want[:, j]).max() / wmax[j]))
                print(name, which, "k", k, "col", j, "err", err, "bound", bound)
                assert err <= bound, (name, which, k, j, err, spread[j])


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_small_cases_as_lu(case):
    name, n, Cp, Ci, Cx, perm, slot = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", True)
    plan = _plan(S)
    _check_close(plan, _factor(S, plan), n, np.random.default_rng(1), 1e-12, 1e-13, name)
    plan.close()


@pytest.mark.parametrize("N", [6, 10])
def test_unsymmetric_stencils(N):
    S = _stencil(N)
    plan = _plan(S)
    _check_close(plan, _factor(S, plan), S.n, np.random.default_rng(2), 1e-12, 1e-13, f"stencil_{N}")
    plan.close()


@pytest.mark.parametrize("case", pivot_cases(), ids=lambda c: c[0])
def test_with_pivoting(case):
    name, n, Cp, Ci, Cx, perm, tol, _ = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    plan = _plan(S, tol)
    assert np.count_nonzero(plan.get_pivots() != np.arange(n)) > 0
    _check_spread(plan, S, _factor(S, plan, True), n, np.random.default_rng(5), name)
    plan.close()


@pytest.mark.parametrize("pivoting", [False, True], ids=["nopivot", "pivot"])
def test_compositions(pivoting):
    """"L" then "U" is solve_many, "Ut" then "Lt" is solve_many(trans=True): the same kernels in the same order on the same numbers
    (the block between the halves crosses to the host and back unchanged).  On a sparse matrix the tiles' atomics land in an order
    that differs from run to run, so there the two agree to 1e-13, the tolerance tests/test_lu_transposed.py puts between two runs
    of one sweep; on a front of one step (dense_200 with its interchanges) nothing is reordered and they agree bit for bit."""
    if pivoting:
        name, n, Cp, Ci, Cx, perm, tol, _ = [c for c in pivot_cases() if c[0] == "dense_200_tol01"][0]
        S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    else:
        S, tol = _stencil(10), 0.0
    plan = _plan(S, tol)
    B = np.random.default_rng(6).standard_normal((S.n, W + 3))
    b = np.ascontiguousarray(B[:, 0])
    for first, second, trans in (("L", "U", False), ("Ut", "Lt", True)):
        for rhs, want in ((B, plan.solve_many(B, trans=trans)), (b, plan.solve(b, trans=trans))):
            got = plan.half_solve(plan.half_solve(rhs, first), second)
            if pivoting:
                assert np.array_equal(got, want), (first, second, np.abs(got - want).max())
            else:
                assert np.allclose(got, want, rtol=1e-13, atol=1e-13 * np.abs(want).max()), (first, second, np.abs(got - want).max())
    assert plan.stat("last_half_ms") > 0
    plan.close()


def test_wide_supernodes_34cubed():
    """a supernode wider than 1024 columns: BIG tasks and the row-major diagonal copies, which BOTH backward halves make for
    themselves -- "U" from the U^T panels, "Lt" from the L panels.  A fresh plan is called with "U", then "Lt", then solve, then "U"
    again: a half that read the copies the call before it left behind would be wrong by O(1).  Then new values on the same plan."""
    S = _stencil(34)
    assert np.diff(S.Super).max() > 1024
    n = S.n
    rng = np.random.default_rng(3)
    B = rng.uniform(0.5, 1.5, (n, 3))
    b = np.ascontiguousarray(B[:, 0])
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, S.Ux)
    plan.factorize()
    wantU = wantLt = None
    for scale in (1.0, 2.0):
        if scale != 1.0:
            # 2 A = L (2 U) exactly (a power of two): F and "Lt" keep their values, "U" halves -- no second reference sweep
            plan.set_values(scale * S.Lx, scale * S.Ux)
            plan.factorize()
            wantU = wantU / scale
        got = [plan.half_solve(B, "U"), plan.half_solve(B, "Lt")]
        x = plan.solve(b)
        got += [plan.half_solve(B, "U"), plan.half_solve(b, "Lt"), plan.half_solve(b, "U")]
        if wantU is None:
            F = _factor(S, plan)
            wantU, wantLt = R.half(F, B, "U"), R.half(F, B, "Lt")
        for X, want, what in ((got[0], wantU, "U first"), (got[1], wantLt, "Lt after U"), (got[2], wantU, "U after solve"),
                              (got[3], wantLt[:, 0], "Lt one column"), (got[4], wantU[:, 0], "U one column after Lt")):
            err = float(np.abs(X - want).max() / np.abs(want).max())
            print(scale, what, "err", err)
            assert np.allclose(X, want, rtol=1e-11, atol=1e-12 * np.abs(want).max()), (scale, what, err)
        # the solve in between is "L" then "U"
        xh = plan.half_solve(plan.half_solve(b, "L"), "U")
        assert np.allclose(x, xh, rtol=1e-12, atol=1e-12 * np.abs(xh).max())
    plan.close()


def test_layouts_in_place_and_stats():
    S = _stencil(8)
    plan = _plan(S)
    n, k = S.n, W + 2
    F = _factor(S, plan)
    B = np.random.default_rng(9).standard_normal((n, k))
    lib = sf.lib
    for which, code in (("L", 0), ("U", 1), ("Ut", 2), ("Lt", 3)):
        ref = R.half(F, B, which)
        same = lambda X: np.allclose(X, ref, rtol=1e-12, atol=1e-13 * np.abs(ref).max())
        assert same(plan.half_solve(np.asfortranarray(B), which)) and same(plan.half_solve(np.ascontiguousarray(B), which))
        wide = np.random.default_rng(10).standard_normal((n, 2 * k))
        wide[:, ::2] = B
        assert same(plan.half_solve(wide[:, ::2], which))                   # not contiguous in either order
        ldb, ldx = n + 5, n + 11
        Bp = np.full((ldb, k), 7.0, order="F")
        Bp[:n] = B
        Xp = np.full((ldx, k), -3.0, order="F")
        assert lib.sf_lu_plan_solve_half(plan._h, code, k, _dp(Bp), ldb, _dp(Xp), ldx) == SF_OK
        assert same(Xp[:n]) and np.all(Xp[n:] == -3.0) and np.all(Bp[n:] == 7.0)
        x1 = np.full(ldx, -3.0)
        assert lib.sf_lu_plan_solve_half(plan._h, code, 1, _dp(Bp), ldb, _dp(x1), ldx) == SF_OK        # one column of the padded block
        assert same(np.column_stack([x1[:n], ref[:, 1:]])) and np.all(x1[n:] == -3.0)
        Bq = Bp.copy(order="F")
        assert lib.sf_lu_plan_solve_half(plan._h, code, k, _dp(Bq), ldb, _dp(Bq), ldb) == SF_OK        # in place, padded
        assert same(Bq[:n]) and np.all(Bq[n:] == 7.0)
        Bi = np.asfortranarray(B.copy())
        assert lib.sf_lu_plan_solve_half(plan._h, code, k, _dp(Bi), n, _dp(Bi), n) == SF_OK        # in place
        assert same(Bi)
        bi = B[:, 0].copy()
        assert lib.sf_lu_plan_solve_half(plan._h, code, 1, _dp(bi), n, _dp(bi), n) == SF_OK
        assert np.allclose(bi, ref[:, 0], rtol=1e-12, atol=1e-13 * np.abs(ref[:, 0]).max())
        assert lib.sf_lu_plan_solve_half(plan._h, code, k, _dp(Bi), n + 1, _dp(Bi), n) == SF_ERR_ARG
        assert plan.stat("last_half_ms") > 0
        assert plan.half_solve(np.empty((n, 0)), which).shape == (n, 0)
        assert lib.sf_lu_plan_solve_half(plan._h, code, 0, _dp(Bi), n, _dp(Bi), n) == SF_OK
    with pytest.raises(ValueError):
        plan.half_solve(B, "LT")
    with pytest.raises(ValueError):
        plan.half_solve(np.ones((n + 1, 2)))
    plan.close()


def _refused(plan, n):
    B = np.ones((n, 3), order="F")
    X = np.full((n, 3), 7.0, order="F")
    rc = [sf.lib.sf_lu_plan_solve_half(plan._h, which, k, _dp(B), n, _dp(X), n) for which in range(4) for k in (3, 1, 0)]
    return rc == [SF_ERR_ARG] * 12 and bool(np.all(X == 7.0))


def test_plan_lifecycle():
    S = _stencil(8)
    n = S.n
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, S.Ux)
    assert _refused(plan, n)                                 # before any factorization
    plan.factorize()
    B = np.random.default_rng(11).standard_normal((n, 3))
    X = plan.half_solve(B, "Ut")
    # a failed factorization: refused until one succeeds, and the plan stays usable
    plan.set_values(S.Lx * 0.0, S.Ux * 0.0)
    with pytest.raises(sf.SparseFrameError):
        plan.factorize()
    assert _refused(plan, n)
    plan.set_values(S.Lx, S.Ux)
    assert _refused(plan, n)
    plan.factorize()
    X2 = plan.half_solve(B, "Ut")
    assert np.allclose(X2, X, rtol=1e-13, atol=1e-13 * np.abs(X).max())
    plan.close()
    for which in WHICH:
        with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
            plan.half_solve(B, which)                        # after close(): no handle
    # a Cholesky plan is refused at the LU entry point
    n, Cp, Ci, Cx = gen.laplacian_lower(6, 6, 6)
    Sc = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(6, 6, 6), 1 << 30)
    cp = sf.CholPlan(Sc)
    cp.set_values(Sc.Lx)
    cp.factorize()
    assert _refused(cp, n)
    cp.close()
