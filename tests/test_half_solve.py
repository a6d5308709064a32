"""sf_chol_plan_solve_half / sf_chol_plan_quadform (CholPlan.solve_half, CholPlan.quadform): the two halves of the device solve on
their own and the quadratic form b^T A^-1 b, against the numpy sweeps of tests/sample_ref.py over the plan's own factor."""
import ctypes as C

import numpy as np
import pytest

import sample_ref
from util import sf, gen, nd_perm_py, small_cases

pytestmark = pytest.mark.gpu

W = 16
SF_OK, SF_ERR_ARG = 0, 1


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _chol_plan(sym):
    plan = sf.CholPlan(sym, device=0)
    plan.set_values(sym.Lx)
    plan.factorize()
    return plan, plan.get_factor()


def _close(got, want, rtol=1e-12, atol_rel=1e-13):
    return np.allclose(got, want, rtol=rtol, atol=atol_rel * max(np.abs(want).max(), 1e-300))


def _lap(N, perm=True):
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    return sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N) if perm else None, 4 << 30)


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_small_cases(case):
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    plan, Lsx = _chol_plan(sym)
    B = np.random.default_rng(1).standard_normal((n, W + 1))
    for which in ("L", "Lt"):
        want = sample_ref.half_solve(sym, Lsx, B, which)
        got = {}
        for k in (1, 3, W, W + 1):
            X = plan.solve_half(B[:, :k], which)
            assert X.shape == (n, k) and X.dtype == np.float64
            assert _close(X, want[:, :k]), (which, k, float(np.abs(X - want[:, :k]).max()))
            got[k] = X
        # the one-column kernels and the 16-wide ones agree; a 1-D right-hand side is the one-column call
        assert _close(got[1][:, 0], got[3][:, 0]), which
        x = plan.solve_half(B[:, 0], which)
        assert x.shape == (n,) and _close(x, got[3][:, 0]), which
    # the two halves one after the other are the whole solve
    Y = plan.solve_half(plan.solve_half(B, "L"), "Lt")
    assert _close(Y, plan.solve_many(B))
    plan.close()


def test_wide_supernodes_backward_half_first(oracle):
    """34^3: a supernode wider than 1024 columns (BIG tasks, far tiles, the row-major copies of the diagonal blocks).  The first
    solve-type call of a FRESH plan is the backward half, which has to make those copies itself -- and make them again after a
    refactorization"""
    N = 34
    sym = _lap(N)
    n = sym.n
    assert np.diff(sym.Super).max() > 1024
    plan, Lsx = _chol_plan(sym)
    rng = np.random.default_rng(2)
    B = rng.standard_normal((n, W + 3))
    X = plan.solve_half(B, "Lt")
    assert _close(X, sample_ref.half_solve(sym, Lsx, B, "Lt"), 1e-11, 1e-12)
    Y = plan.solve_half(B, "L")
    assert _close(Y, sample_ref.half_solve(sym, Lsx, B, "L"), 1e-11, 1e-12)
    b = np.ascontiguousarray(B[:, 2])
    assert _close(plan.solve(b), oracle.chol_solve(sym, Lsx, b), 1e-11, 1e-12)
    # new values, the same plan: the copies of the old factor's diagonal blocks must not be used
    plan.set_values(2.0 * sym.Lx)
    plan.factorize()
    Lsx2 = plan.get_factor()
    X2 = plan.solve_half(B, "Lt")
    assert _close(X2, sample_ref.half_solve(sym, Lsx2, B, "Lt"), 1e-11, 1e-12)
    x1 = plan.solve_half(b, "Lt")
    assert _close(x1, X2[:, 2], 1e-11, 1e-12)
    plan.close()


def test_quadform():
    sym = _lap(16)
    n = sym.n
    plan, Lsx = _chol_plan(sym)
    rng = np.random.default_rng(3)
    for k in (1, W, W + 5):
        B = rng.standard_normal((n, k))
        q = plan.quadform(B)
        assert q.shape == (k,) and q.dtype == np.float64
        via_solve = np.einsum("ij,ij->j", B, plan.solve_many(B))
        via_ref = (sample_ref.half_solve(sym, Lsx, B, "L") ** 2).sum(axis=0)
        assert np.allclose(q, via_solve, rtol=1e-11, atol=0.0), (k, q, via_solve)
        assert np.allclose(q, via_ref, rtol=1e-11, atol=0.0), (k, q, via_ref)
    b = rng.standard_normal(n)
    q1 = plan.quadform(b)
    assert isinstance(q1, float)
    assert np.isclose(q1, float(b @ plan.solve(b)), rtol=1e-11, atol=0.0)
    assert np.isclose(q1, plan.quadform(b.reshape(-1, 1))[0], rtol=1e-13, atol=0.0)
    # columns do not leak into each other
    B = rng.standard_normal((n, W + 5))
    clean = plan.quadform(B)
    B[n // 2, 3] = np.nan
    B[:, 5] = 0.0
    B[7, W + 1] = np.inf
    q = plan.quadform(B)
    assert not np.isfinite(q[3]) and not np.isfinite(q[W + 1])
    assert q[5] == 0.0
    keep = [j for j in range(W + 5) if j not in (3, 5, W + 1)]
    assert np.isfinite(q[keep]).all() and np.allclose(q[keep], clean[keep], rtol=1e-13, atol=0.0)
    assert plan.quadform(np.zeros(n)) == 0.0
    assert plan.stat("last_quadform_ms") > 0
    plan.close()


def test_quadform_bitwise_repeatable():
    """the reduction itself has a fixed order: the same block gives the same bits (the sweep before it scatters with atomics, so this
    is checked where the sweep has nothing to reorder: a diagonal matrix)"""
    n = 5000
    d = np.linspace(1.0, 3.0, n)
    sym = sf.analyze(n, np.arange(n + 1), np.arange(n), d, None, 1 << 30)
    plan, _ = _chol_plan(sym)
    B = np.random.default_rng(4).standard_normal((n, W))
    q = plan.quadform(B)
    assert np.allclose(q, (B * B / d[:, None]).sum(axis=0), rtol=1e-13, atol=0.0)
    for _ in range(3):
        assert np.array_equal(plan.quadform(B), q)
    assert np.isclose(plan.quadform(B[:, 0].copy()), q[0], rtol=1e-13, atol=0.0)
    plan.close()


def test_layouts():
    sym = _lap(12)
    n = sym.n
    plan, _ = _chol_plan(sym)
    lib = sf.lib
    k = W + 2
    B = np.random.default_rng(6).standard_normal((n, k))
    for which, w in (("L", 0), ("Lt", 1)):
        ref = plan.solve_half(np.asfortranarray(B), which)
        # (the sweeps scatter with atomics: two runs agree to rounding, not bit for bit)
        same = lambda X: np.allclose(X, ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
        assert same(plan.solve_half(np.ascontiguousarray(B), which))        # C order
        # ldb > n, ldx > n through the flat ABI
        ldb, ldx = n + 5, n + 11
        Bp = np.full((ldb, k), 7.0, order="F")
        Bp[:n] = B
        Xp = np.full((ldx, k), -3.0, order="F")
        assert lib.sf_chol_plan_solve_half(plan._h, w, k, _dp(Bp), ldb, _dp(Xp), ldx) == SF_OK
        assert same(Xp[:n]) and np.all(Xp[n:] == -3.0) and np.all(Bp[n:] == 7.0)
        x1 = np.full(ldx, -3.0)
        assert lib.sf_chol_plan_solve_half(plan._h, w, 1, _dp(Bp), ldb, _dp(x1), ldx) == SF_OK       # one column: the other kernels
        assert same(np.column_stack([x1[:n], ref[:, 1:]])) and np.all(x1[n:] == -3.0)
        # in place, X = B (refused with different leading dimensions)
        Bi = np.asfortranarray(B.copy())
        assert lib.sf_chol_plan_solve_half(plan._h, w, k, _dp(Bi), n, _dp(Bi), n) == SF_OK
        assert same(Bi)
        Bq = Bp.copy(order="F")
        assert lib.sf_chol_plan_solve_half(plan._h, w, k, _dp(Bq), ldb, _dp(Bq), ldb) == SF_OK        # in place, padded
        assert same(Bq[:n]) and np.all(Bq[n:] == 7.0)
        assert lib.sf_chol_plan_solve_half(plan._h, w, k, _dp(Bp), ldb, _dp(Bp), ldb + 1) == SF_ERR_ARG
        # nrhs == 0 and a wrong first dimension
        assert lib.sf_chol_plan_solve_half(plan._h, w, 0, _dp(Bp), ldb, _dp(Xp), ldx) == SF_OK
        assert plan.solve_half(np.empty((n, 0)), which).shape == (n, 0)
        with pytest.raises(ValueError):
            plan.solve_half(np.ones((n + 1, 2)), which)
        with pytest.raises(ValueError):
            plan.solve_half(np.ones(n - 1), which)
    with pytest.raises(ValueError):
        plan.solve_half(B, "U")
    # quadform: leading dimension, C order, no columns, a wrong first dimension
    qref = plan.quadform(np.asfortranarray(B))
    assert np.allclose(plan.quadform(np.ascontiguousarray(B)), qref, rtol=1e-13, atol=0.0)
    ldb = n + 5
    Bp = np.full((ldb, k), 7.0, order="F")
    Bp[:n] = B
    q = np.full(k + 2, -3.0)
    assert lib.sf_chol_plan_quadform(plan._h, k, _dp(Bp), ldb, _dp(q)) == SF_OK
    assert np.allclose(q[:k], qref, rtol=1e-13, atol=0.0) and np.all(q[k:] == -3.0)
    assert lib.sf_chol_plan_quadform(plan._h, 0, _dp(Bp), ldb, _dp(q)) == SF_OK and np.all(q[k:] == -3.0)
    q1 = np.full(2, -3.0)
    assert lib.sf_chol_plan_quadform(plan._h, 1, _dp(Bp), ldb, _dp(q1)) == SF_OK        # one column of the padded block
    assert np.allclose(q1[0], qref[0], rtol=1e-13, atol=0.0) and q1[1] == -3.0
    assert plan.quadform(np.empty((n, 0))).shape == (0,)
    with pytest.raises(ValueError):
        plan.quadform(np.ones((n + 1, 2)))
    plan.close()


def _all_calls(h, n):
    """the return codes of the five kinds of call on the handle h"""
    B = np.ones((n, 3), order="F")
    X = np.empty_like(B)
    q = np.empty(3)
    lib = sf.lib
    return [lib.sf_chol_plan_solve_half(h, 0, 3, _dp(B), n, _dp(X), n), lib.sf_chol_plan_solve_half(h, 1, 1, _dp(B), n, _dp(X), n),
            lib.sf_chol_plan_quadform(h, 3, _dp(B), n, _dp(q)), lib.sf_chol_plan_quadform(h, 1, _dp(B), n, _dp(q)),
            lib.sf_chol_plan_sample(h, 3, 1, 0, _dp(X), n, None, 0)]


def test_refusals():
    N = 8
    # an LU plan
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
    S = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", False)
    lu = sf.LUPlan(S)
    lu.set_values(S.Lx, S.Ux)
    lu.factorize()
    assert _all_calls(lu._h, n) == [SF_ERR_ARG] * 5
    b = np.ones(n)
    assert np.isfinite(lu.solve(b)).all()
    lu.close()
    # an out-of-core plan
    N = 12
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    S = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    total = int((np.diff(S.Super) * np.diff(S.Lsip)).sum())
    g, ng, ge, te, nd, fits = sf.ooc_partition(S, int(total * 0.6))
    assert ng >= 2
    ooc = sf.CholPlan(S, ooc_group=g, ooc_ngroups=ng)
    assert _all_calls(ooc._h, n) == [SF_ERR_ARG] * 5
    for call in (lambda: ooc.solve_half(np.ones((n, 2))), lambda: ooc.quadform(np.ones(n)), lambda: ooc.sample(2)):
        with pytest.raises(sf.SparseFrameError):
            call()
    ooc.close()


def test_plan_lifecycle():
    sym = _lap(14)
    n = sym.n
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx)
    assert _all_calls(plan._h, n) == [SF_ERR_ARG] * 5            # before any factorization
    plan.factorize()
    Lsx = plan.get_factor()
    bytes_before = plan.stat("bytes_device")
    assert plan.stat("bytes_solve_many") == 0
    rng = np.random.default_rng(7)
    b = rng.standard_normal(n)
    assert _close(plan.solve_half(b, "Lt"), sample_ref.half_solve(sym, Lsx, b, "Lt"))
    assert plan.stat("last_half_ms") > 0
    assert plan.stat("bytes_solve_many") == 0                      # one column: no 16-wide block
    assert plan.quadform(b) > 0 and plan.stat("last_quadform_ms") > 0
    assert plan.stat("bytes_solve_many") == 0
    B = rng.standard_normal((n, 3))
    assert _close(plan.solve_half(B, "L"), sample_ref.half_solve(sym, Lsx, B, "L"))
    assert plan.stat("last_half_ms") > 0
    assert plan.stat("bytes_solve_many") == 2 * n * W * 8
    assert plan.sample(3, seed=1).shape == (n, 3) and plan.stat("last_sample_ms") > 0
    assert plan.stat("bytes_device") == bytes_before
    x0 = plan.solve(b)
    # a failed factorization (non-positive pivot): refused until one succeeds, and the plan stays usable
    bad = sym.Lx.copy()
    cols = np.repeat(np.arange(n), np.diff(sym.Lp))
    bad[(sym.Li == cols) & (cols == n // 2)] = -1.0
    plan.set_values(bad)
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_NOT_POSDEF"):
        plan.factorize()
    assert _all_calls(plan._h, n) == [SF_ERR_ARG] * 5
    plan.set_values(sym.Lx)
    assert _all_calls(plan._h, n) == [SF_ERR_ARG] * 5            # still no successful factorization
    plan.factorize()
    assert _all_calls(plan._h, n) == [SF_OK] * 5
    assert _close(plan.solve(b), x0)
    assert _close(plan.solve_half(plan.solve_half(b, "L"), "Lt"), x0)
    assert plan.stat("bytes_device") == bytes_before
    plan.close()
