"""Device residual and iterative refinement (sf_chol_plan_residual / sf_chol_plan_refine and the LU entry points) against
longdouble references (tests/refine_ref.py) and against the hand-rolled host loop the other tests use."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import scipy.sparse as sp

import kernel_ref as kr
import refine_ref as rr
from util import sf, gen, nd_perm_py, small_cases

pytestmark = pytest.mark.gpu

SQRT_EPS = 1.4901161193847656e-08
RESID_NAMES = ("lap3d_8_nd", "arrow_300_1", "band_500", "blockdiag", "dense_70", "one_by_one", "diagonal_5")


@pytest.fixture(scope="module", autouse=True)
def _needs_longdouble():
    if not kr.have_longdouble():
        pytest.skip("np.longdouble has no 64-bit mantissa on this platform: no extended-precision reference")


def _resid_cases():
    cases = [(c[0], "cholesky") + c[1:6] for c in small_cases() if c[0] in RESID_NAMES]
    assert len(cases) == len(RESID_NAMES)
    cases.append(("lu_stencil_6_drop", "lu") + gen.unsymmetric_stencil(6, 6, 6, drop=0.05) + (nd_perm_py(6, 6, 6),))
    cases.append(("lu_sym_lap3d_6", "lu_sym") + gen.laplacian_lower(6, 6, 6) + (nd_perm_py(6, 6, 6),))
    return cases


def _analyze(kind, n, Cp, Ci, Cx, perm):
    if kind == "cholesky":
        return sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30)
    return sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", kind == "lu_sym")


def _plan(kind, S, Lx=None, Ux=None):
    if kind == "cholesky":
        plan = sf.CholPlan(S)
        plan.set_values(S.Lx if Lx is None else Lx)
    else:
        plan = sf.LUPlan(S)
        plan.set_values(S.Lx if Lx is None else Lx, None if kind == "lu_sym" else (S.Ux if Ux is None else Ux))
    return plan


def _csr(n, coo):
    rows, cols, vals = coo
    return sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()


def _check_residual(plan, A, m, x, b, what):
    """one residual call against longdouble: every r_i, every w_i, berr and nerr; a second call gives the same bits"""
    r, berr, nerr = plan.residual(b, x)
    w = plan.residual_weights()
    r_ld, w_ld, berr_ld, nerr_ld = rr.residual_ld(A, x, b)
    floor = rr.floor(m)
    print(f"{what}: n={len(x)} max m={int(np.max(m))} berr={berr:.3e} (ld {berr_ld:.3e}) nerr={nerr:.3e} (ld {nerr_ld:.3e}) floor={floor:.3e}")
    kr.assert_within(r, r_ld, kr.SAFETY * (m + 2) * kr.U * w_ld, what + " r")
    kr.assert_within(w, w_ld, (m + 2) * kr.U * w_ld, what + " w")
    assert abs(berr - berr_ld) <= floor, (what, berr, berr_ld)
    assert abs(nerr - nerr_ld) <= floor, (what, nerr, nerr_ld)
    r2, berr2, nerr2 = plan.residual(b, x)
    assert np.array_equal(kr.bits(r), kr.bits(r2)) and np.array_equal(kr.bits(w), kr.bits(plan.residual_weights())), what
    assert berr == berr2 and nerr == nerr2, what


@pytest.mark.parametrize("case", _resid_cases(), ids=lambda c: c[0])
def test_residual_against_longdouble(case):
    """works before any factorization (set_values only); x and b scaled over 1e-6 .. 1e6"""
    name, kind, n, Cp, Ci, Cx, perm = case
    S = _analyze(kind, n, Cp, Ci, Cx, perm)
    A, m = rr.dense_ld(n, *rr.matrix_coo(S))
    rng = np.random.default_rng(17)
    x = rng.standard_normal(n) * kr.scalings(rng, n)
    b = rng.standard_normal(n) * kr.scalings(rng, n)
    plan = _plan(kind, S)
    _check_residual(plan, A, m, x, b, name)
    if n > 1:       # a zero row of (|A| |x| + |b|) is skipped: x = 0 and b = e_0 leave every other row at w = 0, r = 0 exactly
        e0 = np.zeros(n)
        e0[0] = 1.0
        r, berr, nerr = plan.residual(e0, np.zeros(n))
        assert np.array_equal(r, e0) and berr == 1.0 and nerr == 1.0
    plan.close()


def _with_duplicates(Cp, Ci, Cx, rng, count):
    """`count` entries given twice, the extra copy FIRST in its column and with a wrong value"""
    picks = np.sort(rng.choice(len(Ci), count, replace=False))
    col = np.searchsorted(Cp, picks, side="right") - 1
    Ci2 = np.insert(Ci, picks, Ci[picks])
    Cx2 = np.insert(Cx, picks, Cx[picks] * 3.0 + 1.0)
    Cp2 = Cp + np.concatenate([[0], np.cumsum(np.bincount(col, minlength=len(Cp) - 1))])
    return np.ascontiguousarray(Cp2, dtype=np.int64), np.ascontiguousarray(Ci2, dtype=np.int64), Cx2


@pytest.mark.parametrize("kind", ["cholesky", "lu_sym", "lu"])
def test_value_given_twice_counts_as_the_last_one(kind):
    """as loadA: the residual of the structure with duplicates (first copies wrong) equals the one of the clean matrix"""
    N = 6
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=3) if kind == "lu" else gen.laplacian_lower(N, N, N)
    S = _analyze(kind, n, Cp, Ci, Cx, nd_perm_py(N, N, N))
    A, m = rr.dense_ld(n, *rr.matrix_coo(S))
    rng = np.random.default_rng(7)
    keys = ("n", "nsuper", "Super", "SuperMap", "Lsip", "Lsi", "Lsxp", "xsize", "lu", "symmetric")
    dup = types.SimpleNamespace(**{k: getattr(S, k) for k in keys if kind != "cholesky" or k not in ("lu", "symmetric")})
    dup.Lp, dup.Li, Lx = _with_duplicates(S.Lp, S.Li, S.Lx, rng, 200)
    Ux = None
    if kind == "lu":
        dup.Up, dup.Ui, Ux = _with_duplicates(S.Up, S.Ui, S.Ux, rng, 200)
    # (the reference reads the same arrays: its last-occurrence rule must reproduce the clean matrix)
    dupv = types.SimpleNamespace(n=n, lu=int(kind != "cholesky"), symmetric=int(kind != "lu"), Lp=dup.Lp, Li=dup.Li, Lx=Lx,
                                 Up=getattr(dup, "Up", None), Ui=getattr(dup, "Ui", None), Ux=Ux)
    A2, m2 = rr.dense_ld(n, *rr.matrix_coo(dupv))
    assert np.array_equal(A, A2) and np.array_equal(m, m2)
    x = rng.standard_normal(n) * kr.scalings(rng, n)
    b = rng.standard_normal(n) * kr.scalings(rng, n)
    plan = _plan(kind, dup, Lx, Ux)
    _check_residual(plan, A, m, x, b, "duplicates_" + kind)
    plan.close()


def _fresh_cases():
    return [("lap3d_8_nd", "cholesky") + gen.laplacian_lower(8, 8, 8) + (nd_perm_py(8, 8, 8),),
            ("lu_stencil_12", "lu") + gen.unsymmetric_stencil(12, 12, 12, seed=9) + (nd_perm_py(12, 12, 12),)]


@pytest.mark.parametrize("case", _fresh_cases(), ids=lambda c: c[0])
def test_refine_with_a_fresh_factor(case):
    name, kind, n, Cp, Ci, Cx, perm = case
    S = _analyze(kind, n, Cp, Ci, Cx, perm)
    A, m = rr.dense_ld(n, *rr.matrix_coo(S))
    floor = rr.floor(m)
    b = 1.0 + np.arange(n) / n
    plan = _plan(kind, S)
    plan.factorize()
    x, info = plan.refine(b, return_info=True)
    berr_ld = rr.residual_ld(A, x, b)[2]
    print(f"{name}: iters={info['iters']} berr0={info['berr0']:.3e} berr={info['berr']:.3e} host longdouble berr={berr_ld:.3e} floor={floor:.3e}")
    assert info["berr"] <= floor and berr_ld <= floor
    assert info["iters"] <= 2
    assert info["iters"] == plan.stat("last_refine_iters") and info["berr"] == plan.stat("last_refine_berr")
    assert plan.stat("last_refine_ms") > 0
    x0, info0 = plan.refine(b, max_iter=0, return_info=True)
    xs = plan.solve(b)
    assert info0["iters"] == 0 and info0["berr"] == info0["berr0"]
    assert np.max(np.abs(x0 - xs)) <= 1e-12 * np.max(np.abs(xs))
    assert abs(info0["berr"] - rr.residual_ld(A, x0, b)[2]) <= floor
    plan.close()


@pytest.fixture(scope="module")
def lap8():
    n, Cp, Ci, Cx = gen.laplacian_lower(8, 8, 8)
    S = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(8, 8, 8), 1 << 30)
    return S


def test_refine_with_a_stale_factor(lap8):
    """factorize, then set_values with every value moved by 1e-3 relative: refine converges towards the NEW matrix with the old
    factor (an exact-LU version of this iteration on the CPU: berr0 = 7.8e-4, below 4e-16 at step 5).  Also the test that the
    kernel reads the values through the position map: a copy taken at set-up would leave berr at 1e-3."""
    S = lap8
    n = S.n
    plan = _plan("cholesky", S)
    plan.factorize()
    x_old = plan.refine(1.0 + np.arange(n) / n)             # (the row form is built here, before the values change)
    Lx2 = S.Lx * (1.0 + 1e-3 * np.random.default_rng(5).uniform(-1, 1, S.Lx.size))
    plan.set_values(Lx2)
    A, m = rr.dense_ld(n, *rr.matrix_coo(S, Lx=Lx2))
    floor = rr.floor(m)
    b = 1.0 + np.arange(n) / n
    x, info = plan.refine(b, max_iter=10, return_info=True)
    berr_ld = rr.residual_ld(A, x, b)[2]
    print(f"stale: iters={info['iters']} berr0={info['berr0']:.3e} berr={info['berr']:.3e} host longdouble berr={berr_ld:.3e} floor={floor:.3e}")
    assert info["berr0"] >= 1e-5
    assert berr_ld <= floor and info["berr"] <= floor
    assert 3 <= info["iters"] <= 10
    assert not np.array_equal(x, x_old)
    plan.close()


def test_divergence_keeps_the_best_iterate(lap8):
    """values 3 A with the factor of A: the first correction overshoots (x1 = x0 + (I - 3) x0-ish), berr gets worse, the loop
    stops on stagnation and hands back x0"""
    S = lap8
    n = S.n
    plan = _plan("cholesky", S)
    plan.factorize()
    plan.set_values(3.0 * S.Lx)
    b = 1.0 + np.arange(n) / n
    x, info = plan.refine(b, max_iter=10, return_info=True)
    xs = plan.solve(b)
    A, m = rr.dense_ld(n, *rr.matrix_coo(S, Lx=3.0 * S.Lx))
    print(f"divergence: iters={info['iters']} berr0={info['berr0']:.3e} berr={info['berr']:.3e}")
    assert info["iters"] == 1 and info["berr"] == info["berr0"]
    assert np.max(np.abs(x - xs)) <= 1e-12 * np.max(np.abs(xs))
    assert abs(info["berr"] - rr.residual_ld(A, x, b)[2]) <= rr.floor(m)
    plan.close()


def _zero_diag_12():
    """the zero-diagonal 12^3 case of tests/test_lu_pivot.py"""
    N = 12
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=9)
    perm = nd_perm_py(N, N, N)
    S0 = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    widths = np.diff(S0.Super)
    leaves = [s for s in range(S0.nsuper) if widths[s] >= 4][::2]
    Cx = Cx.copy()
    cols = np.repeat(np.arange(n), np.diff(Cp))
    for s in leaves:
        g = S0.Perm[S0.Super[s]]
        Cx[(Ci == g) & (cols == g)] = 0.0
    return n, Cp, Ci, Cx, perm


def _pivot_cases():
    return [("general_10_tol1", gen.unsymmetric_general(10, 10, 10, seed=21) + (nd_perm_py(10, 10, 10),), 1.0, 0.0),
            ("zero_diag_12_tol01", _zero_diag_12(), 0.1, SQRT_EPS),
            ("zero_diag_12_perturbed", _zero_diag_12(), 0.0, SQRT_EPS)]


def _scaled_residual(A, x, b):
    r = A @ x - b
    return float(np.abs(r).max() / (abs(A).sum(axis=0).max() * np.abs(x).max() + np.abs(b).max()))


@pytest.mark.parametrize("case", _pivot_cases(), ids=lambda c: c[0])
def test_refine_pivoted_lu(case):
    """the project's bar (scaled residual <= 1e-10) after refine(max_iter=5), and the device loop of k steps is no worse than the
    hand-rolled host loop with k - 1 (both judged in longdouble on the host, never by the code under test alone)"""
    name, (n, Cp, Ci, Cx, perm), tol, perturb = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    coo = rr.matrix_coo(S)
    A, m = rr.dense_ld(n, *coo)
    A64 = _csr(n, coo)
    floor = rr.floor(m)
    b = 1.0 + np.arange(n) / n
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, S.Ux)
    plan.set_pivoting(tol, perturb)
    plan.factorize()
    if name.endswith("perturbed"):
        assert plan.stat("perturbed_pivots") > 0
    x, info = plan.refine(b, max_iter=5, return_info=True)
    k = info["iters"]
    res = _scaled_residual(A64, x, b)
    berr_ld = rr.residual_ld(A, x, b)[2]
    xs = rr.host_refine(plan, A64, b, max(k - 1, 0))
    host = [rr.residual_ld(A, xi, b)[2] for xi in xs]
    print(f"{name}: iters={k} berr0={info['berr0']:.3e} berr={info['berr']:.3e} host longdouble berr={berr_ld:.3e} scaled residual={res:.3e} "
          f"host loop berr by step={['%.3e' % h for h in host]} floor={floor:.3e} perturbed={plan.stat('perturbed_pivots'):.0f}")
    assert res <= 1e-10
    assert abs(info["berr"] - berr_ld) <= floor
    assert berr_ld <= max(floor, host[-1])
    plan.close()


def test_non_finite_input(lap8):
    S = lap8
    n = S.n
    plan = _plan("cholesky", S)
    plan.factorize()
    b = 1.0 + np.arange(n) / n
    b[n // 3] = np.nan
    x, info = plan.refine(b, return_info=True)          # SF_OK: no exception
    assert not math.isfinite(info["berr"]) and info["iters"] == 0
    good = 1.0 + np.arange(n) / n
    x = plan.solve(good)
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[5] = bad
        r, berr, nerr = plan.residual(good, xb)
        assert not math.isfinite(berr) and not math.isfinite(nerr)
    r, berr, nerr = plan.residual(good, x)
    assert math.isfinite(berr) and math.isfinite(nerr)
    plan.close()


def test_aliasing_and_state(lap8):
    S = lap8
    n = S.n
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    b = 1.0 + np.arange(n) / n
    plan = sf.CholPlan(S)
    berr = C.c_double()
    out = np.empty(n)
    plan.set_values(S.Lx)
    assert sf.lib.sf_chol_plan_refine(plan._h, dp(b), dp(out), 2, 0.0, C.byref(berr)) == 1       # before any factorization
    plan.factorize()
    val0, xs0 = plan.validate(), plan.solve(b)
    bytes_device = plan.stat("bytes_device")
    assert plan.stat("bytes_refine") == 0
    want = plan.refine(b)
    buf = b.copy()
    assert sf.lib.sf_chol_plan_refine(plan._h, dp(buf), dp(buf), 5, 0.0, C.byref(berr)) == 0     # x_host is b_host
    assert np.max(np.abs(buf - want)) <= 1e-12 * np.max(np.abs(want))
    val1, xs1 = plan.validate(), plan.solve(b)
    assert abs(val1 - val0) <= 1e-12 and np.max(np.abs(xs1 - xs0)) <= 1e-12 * np.max(np.abs(xs0))
    assert plan.stat("bytes_device") == bytes_device and plan.stat("bytes_refine") > 0
    # a failed factorization (non-positive pivot): refused until one succeeds
    bad = S.Lx.copy()
    cols = np.repeat(np.arange(n), np.diff(S.Lp))
    bad[(S.Li == cols) & (cols == n // 2)] = -1.0
    plan.set_values(bad)
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_NOT_POSDEF"):
        plan.factorize()
    assert sf.lib.sf_chol_plan_refine(plan._h, dp(b), dp(out), 2, 0.0, C.byref(berr)) == 1
    plan.residual(b, xs0)                                                                       # (residual needs the values only)
    plan.set_values(S.Lx)
    assert sf.lib.sf_chol_plan_refine(plan._h, dp(b), dp(out), 2, 0.0, C.byref(berr)) == 1       # still no successful factorization
    plan.factorize()
    x = plan.refine(b)
    assert np.max(np.abs(x - want)) <= 1e-12 * np.max(np.abs(want))
    plan.close()
