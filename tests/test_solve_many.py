"""sf_chol_plan_solve_many / sf_lu_plan_solve_many (CholPlan.solve_many, LUPlan.solve_many): the blocked multi-right-hand-side
device solve with the resident factor, column by column against the CPU oracle's solve."""
import ctypes as C

import numpy as np
import pytest

from util import sf, gen, nd_perm_py, small_cases
from test_lu_pivot import pivot_cases

pytestmark = pytest.mark.gpu

W = 16
EXPERIMENT_KNOBS = ("SF_SOLVE_BWD_AHEAD", "SF_SOLVE_BWD_FUSED", "SF_SOLVE_DIAGT", "SF_SOLVE_FAR_GROUPS", "SF_SOLVE_FAR_WGS",
                    "SF_SOLVE_FWD_AHEAD", "SF_SOLVE_FWD_FAR_FIRST")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _chol_plan(sym):
    plan = sf.CholPlan(sym, device=0)
    plan.set_values(sym.Lx)
    plan.factorize()
    return plan, plan.get_factor()


def _check_columns(X, B, solve1, rtol, atol_rel):
    for j in range(B.shape[1]):
        want = solve1(B[:, j])
        assert np.allclose(X[:, j], want, rtol=rtol, atol=atol_rel * np.abs(want).max()), j


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_small_cases_cholesky(oracle, case):
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    plan, Lsx = _chol_plan(sym)
    rng = np.random.default_rng(1)
    assert plan.stat("solve_many_width") == W
    for k in (1, 3, W, W + 1, 2 * W + 5):
        B = rng.standard_normal((n, k))
        X = plan.solve_many(B)
        assert X.shape == (n, k) and X.dtype == np.float64
        _check_columns(X, B, lambda b: oracle.chol_solve(sym, Lsx, b), 1e-12, 1e-13)
    plan.close()


@pytest.mark.parametrize("knobs", [
    {"SF_SOLVE_FAR_WGS": "1", "SF_SOLVE_FAR_GROUPS": "64"},
    {"SF_SOLVE_FAR_WGS": "1", "SF_SOLVE_FAR_GROUPS": "3", "SF_SOLVE_FWD_FAR_FIRST": "0"},
    {"SF_SOLVE_BWD_AHEAD": "0", "SF_SOLVE_FWD_AHEAD": "0", "SF_SOLVE_DIAGT": "0"},
    {"SF_SOLVE_BWD_FUSED": "0"}], ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("method", ["cholesky", "lu"])
def test_wide_supernodes_schedules(oracle, monkeypatch, knobs, method):
    """supernodes of several 256-column steps (BIG tasks, far tiles, row-major diagonal copies) under the schedule variants"""
    if any(k in EXPERIMENT_KNOBS for k in knobs) and not sf.lib.sf_build_experiments():
        pytest.skip("A/B switch compiled out of this build (make -C sparse-matrix-factorization-library_amd/csrc EXP=1)")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    N = 34
    if method == "lu":
        n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
        sym = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 4 << 30, "lu", False)
        plan = sf.LUPlan(sym)
        plan.set_values(sym.Lx, sym.Ux)
    else:
        n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 4 << 30)
        plan = sf.CholPlan(sym)
        plan.set_values(sym.Lx)
    assert np.diff(sym.Super).max() > 1024
    plan.factorize()
    Lsx = plan.get_factor()
    B = np.random.default_rng(2).standard_normal((n, W + 3))
    X = plan.solve_many(B)
    ref = oracle.lu_solve if method == "lu" else oracle.chol_solve
    _check_columns(X, B, lambda b: ref(sym, Lsx, b), 1e-11, 1e-12)
    plan.close()


def test_wide_supernodes_default_schedule(oracle):
    """the release build's schedule on the wide-supernode matrix (the knob variants above skip without EXP=1)"""
    N = 34
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 4 << 30)
    assert np.diff(sym.Super).max() > 1024
    plan, Lsx = _chol_plan(sym)
    B = np.random.default_rng(3).standard_normal((n, W + 3))
    X = plan.solve_many(B)
    _check_columns(X, B, lambda b: oracle.chol_solve(sym, Lsx, b), 1e-11, 1e-12)
    # and against the one-column device solve
    for j in (0, W, W + 2):
        assert np.allclose(X[:, j], plan.solve(B[:, j]), rtol=1e-12, atol=1e-13 * np.abs(X[:, j]).max())
    plan.close()


@pytest.mark.parametrize("case", [c for c in pivot_cases() if c[0] in ("dense_200_tol01", "zero_diag_12", "general_14_tol03")],
                         ids=lambda c: c[0])
def test_lu_with_pivoting(oracle, case):
    name, n, Cp, Ci, Cx, perm, tol, vtol = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, S.Ux)
    plan.set_pivoting(tol)
    plan.factorize()
    piv = plan.get_pivots()
    assert np.count_nonzero(piv != np.arange(n)) > 0
    Lsx = plan.get_factor()
    rng = np.random.default_rng(4)
    B = rng.standard_normal((n, W + 1))
    X = plan.solve_many(B)
    for j in range(B.shape[1]):
        want = oracle.lu_solve_pivot(S, Lsx, piv, B[:, j])
        spread = 0.0
        for _ in range(5):
            moved = Lsx * (1.0 + rng.integers(-1, 2, Lsx.size) * 1.1102230246251565e-16)
            spread = max(spread, float(np.max(np.abs(oracle.lu_solve_pivot(S, moved, piv, B[:, j]) - want)) / np.abs(want).max()))
        err = float(np.max(np.abs(X[:, j] - want)) / np.abs(want).max())
        # the bound of test_lu_pivot's one-column solve, or what that device solve itself is off by on this column (a random
        # right-hand side on zero_diag_12 meets multipliers of 1e6: the rounding of any summation order shows)
        err1 = float(np.max(np.abs(plan.solve(np.ascontiguousarray(B[:, j])) - want)) / np.abs(want).max())
        assert err <= max(1e-12, 8.0 * spread, 8.0 * err1), (name, j, err, spread, err1)
    plan.close()


def test_column_independence():
    N = 16
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    plan, _ = _chol_plan(sym)
    B = np.random.default_rng(5).standard_normal((n, W + 4))
    B[n // 2, 3] = np.nan
    B[7, W + 1] = np.inf
    B[:, 5] = 0.0
    X = plan.solve_many(B)
    assert np.all(X[:, 5] == 0.0)
    for j in range(B.shape[1]):
        if j in (3, W + 1):
            continue
        assert np.isfinite(X[:, j]).all(), j
        want = plan.solve(np.ascontiguousarray(B[:, j]))
        assert np.allclose(X[:, j], want, rtol=1e-13, atol=1e-13 * max(np.abs(want).max(), 1e-300)), j
    assert not np.isfinite(X[:, 3]).all() and not np.isfinite(X[:, W + 1]).all()
    plan.close()


def test_layouts():
    N = 12
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    plan, _ = _chol_plan(sym)
    k = W + 2
    B = np.random.default_rng(6).standard_normal((n, k))
    ref = plan.solve_many(np.asfortranarray(B))
    # (the sweeps scatter with atomics: two runs agree to rounding, not bit for bit)
    same = lambda X: np.allclose(X, ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
    assert same(plan.solve_many(np.ascontiguousarray(B)))        # C order
    assert same(plan.solve(B))                                   # 2-D solve() goes to solve_many
    # ldb > n, ldx > n through the flat ABI
    ldb, ldx = n + 5, n + 11
    Bp = np.full((ldb, k), 7.0, order="F")
    Bp[:n] = B
    Xp = np.full((ldx, k), -3.0, order="F")
    assert sf.lib.sf_chol_plan_solve_many(plan._h, k, _dp(Bp), ldb, _dp(Xp), ldx) == 0
    assert same(Xp[:n])
    assert np.all(Xp[n:] == -3.0)
    x1 = np.full(ldx, -3.0)
    assert sf.lib.sf_chol_plan_solve_many(plan._h, 1, _dp(Bp), ldb, _dp(x1), ldx) == 0       # one column of the padded block
    assert same(np.column_stack([x1[:n], ref[:, 1:]])) and np.all(x1[n:] == -3.0)
    # in place, X = B
    Bi = np.asfortranarray(B.copy())
    assert sf.lib.sf_chol_plan_solve_many(plan._h, k, _dp(Bi), n, _dp(Bi), n) == 0
    assert same(Bi)
    # nrhs == 0 and a wrong first dimension
    assert plan.solve_many(np.empty((n, 0))).shape == (n, 0)
    with pytest.raises(ValueError):
        plan.solve_many(np.ones((n + 1, 2)))
    plan.close()


def test_plan_lifecycle(oracle):
    N = 14
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    plan, Lsx = _chol_plan(sym)
    bytes_before = plan.stat("bytes_device")
    rng = np.random.default_rng(7)
    for k in (2, 40, 1, W):
        B = rng.standard_normal((n, k))
        X = plan.solve_many(B)
        _check_columns(X, B, lambda b: oracle.chol_solve(sym, Lsx, b), 1e-12, 1e-13)
        b = rng.standard_normal(n)
        assert np.allclose(plan.solve(b), oracle.chol_solve(sym, Lsx, b), rtol=1e-12, atol=1e-13)
    assert plan.stat("last_solve_many_ms") > 0
    assert plan.stat("bytes_solve_many") > 0
    assert plan.stat("bytes_device") == bytes_before
    # new values, the same plan
    plan.set_values(sym.Lx * 2.0)
    plan.factorize()
    Lsx2 = plan.get_factor()
    B = rng.standard_normal((n, W + 3))
    X = plan.solve_many(B)
    _check_columns(X, B, lambda b: oracle.chol_solve(sym, Lsx2, b), 1e-12, 1e-13)
    plan.close()


def test_residual_48cubed():
    N = 48
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), sf.REFERENCE_SLOT_1GPU)
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx)
    plan.factorize()
    B = np.random.default_rng(8).uniform(0.5, 1.5, (n, W))
    X = plan.solve_many(B)
    Lp, Li, Lx = sym.Lp, sym.Li, sym.Lx
    cols = np.repeat(np.arange(n), np.diff(Lp))
    off = Li != cols
    colsum = np.zeros(n)
    np.add.at(colsum, cols, np.abs(Lx))
    np.add.at(colsum, Li[off], np.abs(Lx[off]))
    for j in range(W):
        b, x = B[:, j], X[:, j]
        r = -b.copy()
        np.add.at(r, Li, Lx * x[cols])
        np.add.at(r, cols[off], Lx[off] * x[Li[off]])
        res = np.abs(r).max() / (colsum.max() * np.abs(x).max() + np.abs(b).max())
        assert res <= 1e-13, (j, res)
    plan.close()


def test_out_of_core_plan_refused():
    N = 12
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    S = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    total = int((np.diff(S.Super) * np.diff(S.Lsip)).sum())
    g, ng, ge, te, nd, fits = sf.ooc_partition(S, int(total * 0.6))
    assert ng >= 2
    plan = sf.CholPlan(S, ooc_group=g, ooc_ngroups=ng)
    with pytest.raises(Exception):
        plan.solve_many(np.ones((n, 2)))
    plan.close()
