"""sf_lu_plan_gram / _gram_device (LUPlan.cross_gram, .cross_gram_device, .schur_complement, .solve_saddle): G = C^T A^-1 B = Z^T Y
with Z = U^-T C and Y = F B, against tests/lu_half_ref.py over the plan's own factor (and pivots).

The acceptance bound is componentwise, |G - Gref|_ij <= tol (|Z|^T |Y|)_ij with Z, Y from the numpy sweeps: tol = 1e-12 on the
small cases and 1e-11 at 34^3, the half solves' own tolerances at those sizes (tests/test_lu_half_solve.py) carried through a dot
product.  With pivoting on an entry also gets 8 x its spread: how far the REFERENCE's G_ij moves when every entry of the factor
moves by one ulp at random (5 draws), the yardstick of tests/test_lu_transposed.py.

The reductions have a fixed order, but the forward sweeps before them (sf_solve.hip, not part of this feature) add the tiles'
contributions to a row with floating-point atomics in the order the workgroups arrive; "the same bits as another call" can hold
only where a sweep has nothing to reorder."""
import ctypes as C

import numpy as np
import pytest
import torch

import lu_half_ref as R
import refine_ref as RR
from test_lu_pivot import pivot_cases
from util import sf, gen, nd_perm_py, small_cases

pytestmark = pytest.mark.gpu

W = 16
DEV = "cuda:0"
SF_OK, SF_ERR_ARG = 0, 1
SHAPES = ((1, 1), (1, 3), (3, 1), (W, W), (W + 1, 2 * W + 1), (2 * W + 1, 5))
MMAX, KMAX = 2 * W + 1, 2 * W + 1
ULP = 1.1102230246251565e-16


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


def _identity(n):
    return sf.analyze(n, np.arange(n + 1), np.arange(n), np.ones(n), None, 1 << 30, "lu", True)


def _slabs(n):
    """the grid rule of DESIGN 8h: slabs of about 2048 rows, a whole number of 64-row stretches each, 256 at most"""
    want = min(256, max(1, (n + 2047) // 2048))
    rows = (((n + want - 1) // want + 63) // 64) * 64
    return (n + rows - 1) // rows


def _dev(A):
    """the (n, k) host array as a column-major device tensor"""
    return torch.from_numpy(np.ascontiguousarray(A.T)).to(DEV).t()


def _check(G, Gref, Z, Y, tol, what, extra=None):
    ok, ratio = R.within(G, Gref, Z, Y, tol, extra)
    print(f"{what}: max |G - Gref| / bound = {ratio:.3e} (tol {tol:.0e})")
    assert ok, (what, ratio)


def _all_shapes(plan, F, n, rng, tol, name, spread_of=None):
    """every shape against ONE reference (the leading columns of one C and one B)"""
    Cf, Bf = rng.standard_normal((n, MMAX)), rng.standard_normal((n, KMAX))
    Gref, Z, Y = R.cross_gram_ref(F, Cf, Bf)
    extra = 8.0 * spread_of(Cf, Bf, Gref) if spread_of else None
    for m, k in SHAPES:
        G = plan.cross_gram(Cf[:, :m], Bf[:, :k])
        assert G.shape == (m, k) and G.dtype == np.float64
        _check(G, Gref[:m, :k], Z[:, :m], Y[:, :k], tol, f"{name} ({m}, {k})", None if extra is None else extra[:m, :k])
    g = plan.cross_gram(np.ascontiguousarray(Cf[:, 0]), np.ascontiguousarray(Bf[:, 0]))
    assert isinstance(g, float)
    _check(np.array([[g]]), Gref[:1, :1], Z[:, :1], Y[:, :1], tol, f"{name} 1-D", None if extra is None else extra[:1, :1])
    return Cf, Bf, Gref, Z, Y


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_small_cases_as_lu(case):
    name, n, Cp, Ci, Cx, perm, slot = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", True)
    plan = _plan(S)
    _all_shapes(plan, _factor(S, plan), n, np.random.default_rng(1), 1e-12, name)
    plan.close()


@pytest.mark.parametrize("N", [6, 10])
def test_unsymmetric_stencils(N):
    S = _stencil(N)
    plan = _plan(S)
    Cf, Bf, Gref, _, _ = _all_shapes(plan, _factor(S, plan), S.n, np.random.default_rng(2), 1e-12, f"stencil_{N}")
    # route agreement: C^T (A^-1 B) with the full solve, 1e-11 of max |G|
    G = plan.cross_gram(Cf, Bf)
    route = Cf.T @ plan.solve_many(Bf)
    err = float(np.abs(G - route).max() / np.abs(route).max())
    print("route agreement", err)
    assert err <= 1e-11
    # and G is not symmetric, even for C = B
    Gbb = plan.cross_gram(Bf, Bf)
    assert np.abs(Gbb - Gbb.T).max() > 1e-6 * np.abs(Gbb).max()
    plan.close()


@pytest.mark.parametrize("case", pivot_cases(), ids=lambda c: c[0])
def test_with_pivoting(case):
    name, n, Cp, Ci, Cx, perm, tol, _ = case
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    plan = _plan(S, tol)
    assert np.count_nonzero(plan.get_pivots() != np.arange(n)) > 0
    F = _factor(S, plan, True)
    Lsx = plan.get_factor().copy()
    rng = np.random.default_rng(5)

    def spread_of(Cf, Bf, Gref):
        out = np.zeros_like(Gref)
        for _ in range(5):
            Fm = R.Factor(S, Lsx * (1.0 + rng.integers(-1, 2, Lsx.size) * ULP), F.piv)
            out = np.maximum(out, np.abs(R.cross_gram_ref(Fm, Cf, Bf)[0] - Gref))
        print(name, "max spread / max |G|", out.max() / np.abs(Gref).max())
        return out

    _all_shapes(plan, F, n, rng, 1e-12, name, spread_of)
    plan.close()


@pytest.mark.parametrize("n", [4099, 3])
def test_exact_on_the_identity(n):
    """A = I, small-integer C and B: every intermediate is a small integer, so the result is exact -- a row dropped or counted twice
    at the tail, at a slab boundary or between the waves' groups changes it.  4099 is prime: two slabs, a tail that is no multiple
    of 4 rows.  The sweeps have nothing to reorder here, so calls repeat bit for bit and a NaN keeps to its column or row bit for bit"""
    S = _identity(n)
    plan = _plan(S)
    rng = np.random.default_rng(2)
    m, k = 2 * W + 1, W + 1
    Cf = rng.integers(-8, 9, size=(n, m)).astype(np.float64)
    Bf = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
    G = plan.cross_gram(Cf, Bf)
    assert np.array_equal(G, Cf.T @ Bf)
    assert plan.stat("last_gram_parts") == _slabs(n) and (_slabs(n) >= 2 if n == 4099 else _slabs(n) == 1)
    for mm, kk in SHAPES:
        if mm <= m and kk <= k:
            assert np.array_equal(plan.cross_gram(Cf[:, :mm], Bf[:, :kk]), (Cf.T @ Bf)[:mm, :kk]), (mm, kk)
    for _ in range(2):
        assert np.array_equal(plan.cross_gram(Cf, Bf), G)
    c, b = np.ascontiguousarray(Cf[:, 5]), np.ascontiguousarray(Bf[:, 7])
    assert plan.cross_gram(c, b) == float(c @ b) == G[5, 7]
    assert plan.stat("last_gram_parts") == 0                 # the one-column path
    # containment, bit for bit
    j, i = 9, 20
    Bn = Bf.copy()
    Bn[n // 2, j] = np.nan
    Gn = plan.cross_gram(Cf, Bn)
    keep = np.arange(k) != j
    assert np.isnan(Gn[:, j]).all() and np.array_equal(Gn[:, keep], G[:, keep])
    Cn = Cf.copy()
    Cn[n - 1, i] = np.nan
    Gn = plan.cross_gram(Cn, Bf)
    keep = np.arange(m) != i
    assert np.isnan(Gn[i, :]).all() and np.array_equal(Gn[keep, :], G[keep, :])
    Cn[n - 1, i] = np.inf
    Gn = plan.cross_gram(Cn, Bf)
    assert not np.isfinite(Gn[i, :]).any() and np.array_equal(Gn[keep, :], G[keep, :])
    plan.close()


def _root_path_rows(S):
    """(the columns of the supernodes on the longest path of the elimination tree, from a leaf to the root; supernodes on it)"""
    Super, SuperMap, Lsip, Lsi = (np.asarray(getattr(S, key)) for key in ("Super", "SuperMap", "Lsip", "Lsi"))
    ncol, nrow = np.diff(Super), np.diff(Lsip)
    # the parent: the supernode of the first row below the diagonal block
    parent = [int(SuperMap[Lsi[Lsip[s] + ncol[s]]]) if nrow[s] > ncol[s] else -1 for s in range(int(S.nsuper))]

    def path(s):
        out = []
        while s >= 0:
            out.append(s)
            s = parent[s]
        return out

    best = max((path(s) for s in range(int(S.nsuper))), key=len)
    return np.concatenate([np.arange(Super[s], Super[s + 1]) for s in best]), len(best)


def test_containment_on_the_16cubed_stencil():
    """a NaN in column j of B changes column j of G only, a NaN in column i of C row i only -- compared bit for bit with the clean
    call on the same plan.

    "The same bits as another call" presupposes that the clean columns' own sweeps repeat, and on this matrix they repeat only
    where they have nothing to reorder: the row tiles of the supernodes of one level add to their ancestors' rows with
    floating-point atomics in the order the workgroups arrive (sf_solve.hip, not part of this feature).  So the blocks of the
    bit-for-bit part are supported on ONE path of the elimination tree, the longest: a leaf supernode and all its ancestors up to
    the root (17 supernodes with 3,925 of the 4,096 rows; what is left out are the other 49 small leaves).  On every level one
    supernode has something to add, all others add exact zeros, and x + 0 is x in any order.  The path goes through everything
    the feature runs here -- narrow and wide panels, row tiles and their atomics on every level, two slabs, a padded last chunk
    on both sides -- and both NaNs start in the leaf and travel the whole path.
    Blocks that are dense in the rows are checked against the componentwise bound only; their bits were first asserted too and
    differ from call to call (measured on an MI355X: 100 - 144 of the 608 entries outside column 20 with the NaN in B, 108 - 143
    of the 594 outside row 17 with the NaN in C, every one within 1e-16 (|Z|^T |Y|)_ij of the reference; two clean calls differ
    the same way, as tests/test_gram.py records for the Cholesky twin)."""
    S = _stencil(16)
    n = S.n
    plan = _plan(S)
    F = _factor(S, plan)
    rng = np.random.default_rng(4)
    m, k, i, j = W + 3, 2 * W + 1, 17, 20
    keep, keepi = np.arange(k) != j, np.arange(m) != i
    path, depth = _root_path_rows(S)
    assert depth >= 8 and n // 2 <= len(path) < n           # many levels, most of the rows
    mask = np.zeros((n, 1))
    mask[path] = 1.0
    for dense in (False, True):
        what = "dense" if dense else "root path"
        Cf, Bf = rng.standard_normal((n, m)), rng.standard_normal((n, k))
        if not dense:
            Cf, Bf = Cf * mask, Bf * mask
        Gref, Z, Y = R.cross_gram_ref(F, Cf, Bf)
        clean = plan.cross_gram(Cf, Bf)
        _check(clean, Gref, Z, Y, 1e-12, f"16^3 {what}, clean")
        assert np.count_nonzero(clean) == m * k
        again = plan.cross_gram(Cf, Bf)
        Bn = Bf.copy()
        Bn[path[1], j] = np.nan                             # in the leaf: it travels the whole path
        G = plan.cross_gram(Cf, Bn)
        assert np.isnan(G[:, j]).all() and np.isfinite(G[:, keep]).all()
        _check(G[:, keep], Gref[:, keep], Z, Y[:, keep], 1e-12, f"16^3 {what}, NaN in B, outside its column")
        Cn = Cf.copy()
        Cn[path[2], i] = np.nan
        G2 = plan.cross_gram(Cn, Bf)
        assert np.isnan(G2[i, :]).all() and np.isfinite(G2[keepi, :]).all()
        _check(G2[keepi, :], Gref[keepi, :], Z[:, keepi], Y, 1e-12, f"16^3 {what}, NaN in C, outside its row")
        Cn[path[2], i] = np.inf
        G3 = plan.cross_gram(Cn, Bf)
        assert not np.isfinite(G3[i, :]).any() and np.isfinite(G3[keepi, :]).all()
        diffs = (int((again != clean).sum()), int((G[:, keep] != clean[:, keep]).sum()), int((G2[keepi, :] != clean[keepi, :]).sum()),
                 int((G3[keepi, :] != clean[keepi, :]).sum()))
        print(f"16^3 {what}: entries whose bits differ from the clean call -- a second clean call {diffs[0]} of {m * k}, NaN in column "
              f"{j} of B {diffs[1]} of {m * (k - 1)}, NaN in column {i} of C {diffs[2]} of {(m - 1) * k}, Inf there {diffs[3]}")
        if not dense:
            assert diffs == (0, 0, 0, 0), diffs
    plan.close()


def test_wide_supernodes_34cubed():
    S = _stencil(34)
    n = S.n
    assert np.diff(S.Super).max() > 1024
    plan = _plan(S)
    rng = np.random.default_rng(3)
    m, k = W + 3, 5
    Cf, Bf = rng.standard_normal((n, m)), rng.standard_normal((n, k))
    Gref, Z, Y = R.cross_gram_ref(_factor(S, plan), Cf, Bf)
    G = plan.cross_gram(Cf, Bf)
    _check(G, Gref, Z, Y, 1e-11, "34^3 (19, 5)")
    assert plan.stat("last_gram_parts") == _slabs(n) >= 2 and plan.stat("last_gram_ms") > 0
    # new values, the same plan: A doubled halves the result (L stays, U doubles: Z halves)
    plan.set_values(2.0 * S.Lx, 2.0 * S.Ux)
    plan.factorize()
    _check(plan.cross_gram(Cf, Bf), 0.5 * G, 0.5 * Z, Y, 1e-11, "34^3 (19, 5), 2 A against half the first")
    plan.close()


def test_device_entry():
    N = 10
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
    perm = np.asarray(nd_perm_py(N, N, N), dtype=np.int64)
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    plan = _plan(S)
    m, k = W + 1, 2 * W + 1
    rng = np.random.default_rng(6)
    Cf, Bf = rng.standard_normal((n, m)), rng.standard_normal((n, k))
    Gref, Z, Y = R.cross_gram_ref(_factor(S, plan), Cf, Bf)
    Cd, Bd = _dev(Cf), _dev(Bf)
    with pytest.raises(sf.SparseFrameError):
        plan.cross_gram_device(Cd, Bd, perm_in=True)            # a flag without an ordering
    for mm, kk in ((1, 1), (1, 3), (3, 1), (m, k)):
        Gd = plan.cross_gram_device(Cd[:, :mm], Bd[:, :kk])
        assert tuple(Gd.shape) == (mm, kk) and Gd.dtype == torch.float64
        _check(Gd.cpu().numpy(), Gref[:mm, :kk], Z[:, :mm], Y[:, :kk], 1e-12, f"cross_gram_device ({mm}, {kk})")
    g1 = plan.cross_gram_device(Cd[:, 0].contiguous(), Bd[:, 0].contiguous())
    assert tuple(g1.shape) == (1, 1)
    _check(g1.cpu().numpy(), Gref[:1, :1], Z[:, :1], Y[:, :1], 1e-12, "cross_gram_device 1-D")
    # the caller's numbering, both inputs: row perm[i] of a block is row i of the permuted system
    plan.set_ordering(perm)
    Co, Bo = np.empty_like(Cf), np.empty_like(Bf)
    Co[perm], Bo[perm] = Cf, Bf
    for mm, kk in ((1, 1), (m, k)):
        G = plan.cross_gram_device(_dev(Co[:, :mm]), _dev(Bo[:, :kk]), perm_in=True).cpu().numpy()
        _check(G, Gref[:mm, :kk], Z[:, :mm], Y[:, :kk], 1e-12, f"cross_gram_device perm_in ({mm}, {kk})")
    _check(plan.cross_gram_device(Cd, Bd).cpu().numpy(), Gref, Z, Y, 1e-12, "cross_gram_device, ordering set, no flag")
    # out= is honoured, with a leading dimension of its own; what lies between its columns is not touched
    ldg = m + 5
    buf = torch.full((k, ldg), -7.25, dtype=torch.float64, device=DEV)
    out = buf.t()[:m]
    assert plan.cross_gram_device(Cd, Bd, out=out) is out
    whole = buf.t().cpu().numpy()
    _check(whole[:m], Gref, Z, Y, 1e-12, "cross_gram_device out=")
    assert np.all(whole[m:] == -7.25)
    # refused: the wrong device, too short a tensor, a result of the wrong shape or one that overlaps an input
    with pytest.raises(ValueError):
        plan.cross_gram_device(torch.from_numpy(Cf), Bd)
    with pytest.raises(ValueError):
        plan.cross_gram_device(Cd, _dev(Bf[:n - 1]))
    with pytest.raises(ValueError):
        plan.cross_gram_device(Cd, Bd, out=torch.empty((k, m), dtype=torch.float64, device=DEV).t()[:, :k - 1])
    before_b, before_c = Bd.clone(), Cd.clone()
    with pytest.raises(sf.SparseFrameError):
        plan.cross_gram_device(Cd, Bd, out=Bd[:m])              # column-major (m, k) with the block's leading dimension: inside B
    with pytest.raises(sf.SparseFrameError):
        plan.cross_gram_device(Cd, Bd[:, :m], out=Cd[:m])                   # ... inside C
    assert torch.equal(Bd, before_b) and torch.equal(Cd, before_c)
    lib = sf.lib
    Gd = torch.empty((m, k), dtype=torch.float64, device=DEV)
    args = (m, Cd.data_ptr(), n, k, Bd.data_ptr(), n, Gd.data_ptr(), m)
    assert lib.sf_lu_plan_gram_device(plan._h, 2, *args) == SF_ERR_ARG      # SF_DEV_PERM_OUT
    assert lib.sf_lu_plan_gram_device(plan._h, 0, 0, Cd.data_ptr(), n, k, Bd.data_ptr(), n, Gd.data_ptr(), 1) == SF_OK
    assert lib.sf_lu_plan_gram_device(plan._h, 0, m, Cd.data_ptr(), n, 0, Bd.data_ptr(), n, Gd.data_ptr(), m) == SF_OK
    plan.close()


def test_layouts():
    S = _stencil(8)
    n = S.n
    plan = _plan(S)
    m, k = 3, W + 2
    rng = np.random.default_rng(7)
    Cf, Bf = rng.standard_normal((n, m)), rng.standard_normal((n, k))
    Gref, Z, Y = R.cross_gram_ref(_factor(S, plan), Cf, Bf)
    _check(plan.cross_gram(np.ascontiguousarray(Cf), np.asfortranarray(Bf)), Gref, Z, Y, 1e-12, "C order / Fortran order")
    ldc, ldb, ldg = n + 3, n + 5, m + 3
    Cp_ = np.full((ldc, m), 5.0, order="F")
    Cp_[:n] = Cf
    Bp = np.full((ldb, k), 7.0, order="F")
    Bp[:n] = Bf
    Gp = np.full((ldg, k + 1), -3.0, order="F")
    lib = sf.lib
    assert lib.sf_lu_plan_gram(plan._h, m, _dp(Cp_), ldc, k, _dp(Bp), ldb, _dp(Gp), ldg) == SF_OK
    _check(Gp[:m, :k], Gref, Z, Y, 1e-12, "ldc > n, ldb > n, ldg > m")
    assert np.all(Gp[m:] == -3.0) and np.all(Gp[:, k] == -3.0) and np.all(Bp[n:] == 7.0) and np.all(Cp_[n:] == 5.0)
    assert lib.sf_lu_plan_gram(plan._h, 0, _dp(Cp_), ldc, k, _dp(Bp), ldb, _dp(Gp), ldg) == SF_OK and np.all(Gp[m:] == -3.0)
    assert lib.sf_lu_plan_gram(plan._h, m, _dp(Cp_), ldc, 0, _dp(Bp), ldb, _dp(Gp), ldg) == SF_OK
    _check(Gp[:m, :k], Gref, Z, Y, 1e-12, "untouched by the empty calls")
    assert lib.sf_lu_plan_gram(plan._h, 1, _dp(Cp_), ldc, 1, _dp(Bp), ldb, _dp(Gp), ldg) == SF_OK
    _check(Gp[:1, :1], Gref[:1, :1], Z[:, :1], Y[:, :1], 1e-12, "one column through the ABI")
    assert np.all(Gp[m:] == -3.0)
    # C == B is allowed: both are read only
    Gs = np.zeros((k, k), order="F")
    assert lib.sf_lu_plan_gram(plan._h, k, _dp(Bp), ldb, k, _dp(Bp), ldb, _dp(Gs), k) == SF_OK
    Gbb, Zb, Yb = R.cross_gram_ref(_factor(S, plan), Bf, Bf)
    _check(Gs, Gbb, Zb, Yb, 1e-12, "C is B")
    assert plan.cross_gram(np.empty((n, 0)), Bf).shape == (0, k)
    with pytest.raises(ValueError):
        plan.cross_gram(np.ones((n + 1, 2)), Bf)
    with pytest.raises(ValueError):
        plan.cross_gram(Cf, np.ones((n, 1025)))
    plan.close()


@pytest.mark.parametrize("with_D", [False, True], ids=["D=None", "D!=0"])
@pytest.mark.parametrize("k", [1, 3, 17])
def test_schur_complement_and_saddle_solve(k, with_D):
    S = _stencil(10)
    n = S.n
    plan = _plan(S)
    rng = np.random.default_rng(8)
    B, Cc = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    f, g = rng.standard_normal(n), rng.standard_normal(k)
    D = rng.standard_normal((k, k)) + 2.0 * np.eye(k) if with_D else None
    x, y = plan.solve_saddle(B, Cc, f, g, D)
    assert x.shape == (n,) and y.shape == (k,)
    A, _ = RR.dense_ld(n, *RR.matrix_coo(S))
    res = R.saddle_residual(A, B, Cc, D, x, y, f, g)
    print(f"saddle residual (longdouble, k={k}): {res:.3e}")
    assert res <= 1e-10
    # schur_complement(C, B, D) = D - cross_gram(C, B)
    D2 = rng.standard_normal((k, k))
    G = plan.cross_gram(Cc, B)
    assert np.allclose(plan.schur_complement(Cc, B, D2), D2 - G, rtol=1e-13, atol=1e-13 * np.abs(G).max())
    if not with_D:
        with pytest.raises(ValueError, match="singular Schur complement"):
            plan.solve_saddle(B, np.zeros((n, k)), f, g)
        # ... which D makes up for
        x, y = plan.solve_saddle(B, np.zeros((n, k)), f, g, np.eye(k))
        assert R.saddle_residual(A, B, np.zeros((n, k)), np.eye(k), x, y, f, g) <= 1e-10
        if k > 1:
            Cs = Cc.copy()
            Cs[:, 1] = Cs[:, 0]                                  # two equal rows of S: a pivot of a few ulps, not an exact zero
            with pytest.raises(ValueError, match="singular Schur complement"):
                plan.solve_saddle(B, Cs, f, g)
    plan.close()


def _both_calls(plan, n):
    B = np.ones((n, 3), order="F")
    Cc = np.ones((n, 2), order="F")
    G = np.full((2, 3), 7.0, order="F")
    Bd, Cd = _dev(B), _dev(Cc)
    Gd = torch.full((3, 2), 7.0, dtype=torch.float64, device=DEV).t()
    lib = sf.lib
    rc = [lib.sf_lu_plan_gram(plan._h, 2, _dp(Cc), n, 3, _dp(B), n, _dp(G), 2), lib.sf_lu_plan_gram(plan._h, 1, _dp(Cc), n, 1, _dp(B), n, _dp(G), 2),
          lib.sf_lu_plan_gram_device(plan._h, 0, 2, Cd.data_ptr(), n, 3, Bd.data_ptr(), n, Gd.data_ptr(), 2)]
    untouched = bool(np.all(G == 7.0)) and bool((Gd == 7.0).all())
    return rc, untouched


def test_store_stats_and_lifecycle():
    S = _stencil(14)
    n = S.n
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, S.Ux)
    assert _both_calls(plan, n) == ([SF_ERR_ARG] * 3, True)         # before any factorization
    plan.factorize()
    F = _factor(S, plan)
    bytes_before = plan.stat("bytes_device")
    assert plan.stat("bytes_gram") == 0
    rng = np.random.default_rng(9)
    Cf, Bf = rng.standard_normal((n, 2 * W + 1)), rng.standard_normal((n, 3 * W + 1))
    Gref, Z, Y = R.cross_gram_ref(F, Cf, Bf)

    def call(m, k, what):
        _check(plan.cross_gram(Cf[:, :m], Bf[:, :k]), Gref[:m, :k], Z[:, :m], Y[:, :k], 1e-12, what)
        return plan.stat("bytes_gram")

    g = plan.cross_gram(Cf[:, 0].copy(), Bf[:, 0].copy())
    assert isinstance(g, float) and plan.stat("last_gram_ms") > 0
    assert plan.stat("bytes_gram") == 0 and plan.stat("last_gram_parts") == 0      # one column: no store
    b1 = call(W + 1, 2 * W + 1, "a large call (17, 33)")
    assert b1 >= 5 * n * W * 8 and plan.stat("last_gram_parts") == _slabs(n) and plan.stat("last_gram_ms") > 0
    assert call(3, 5, "a small call (3, 5)") == b1                  # reused
    assert call(W, 2 * W, "(16, 32)") == b1
    b2 = call(W + 1, 3 * W + 1, "more columns of B (17, 49)")
    assert b2 > b1 and b2 >= 6 * n * W * 8                          # grown
    b3 = call(2 * W + 1, 3, "more columns of C (33, 3)")
    assert b3 > b2 and b3 >= 7 * n * W * 8                          # grown on the other side; the Y side keeps its room
    assert call(W + 1, 3 * W + 1, "(17, 49) again") == b3
    assert plan.stat("bytes_device") == bytes_before
    # a failed factorization: refused until one succeeds, and the plan stays usable
    plan.set_values(S.Lx * 0.0, S.Ux * 0.0)
    with pytest.raises(sf.SparseFrameError):
        plan.factorize()
    assert _both_calls(plan, n) == ([SF_ERR_ARG] * 3, True)
    plan.set_values(S.Lx, S.Ux)
    assert _both_calls(plan, n) == ([SF_ERR_ARG] * 3, True)         # still no successful factorization
    plan.factorize()
    assert _both_calls(plan, n)[0] == [SF_OK] * 3
    assert call(2 * W + 1, 3 * W + 1, "(33, 49) after the refactorization") == b3
    # close() frees the store.  With 1024 + 1024 columns it is larger than half of everything else the plan holds on the device, so
    # the device's free memory cannot grow by the store and half of the rest unless the store is among what is freed
    Gw = plan.cross_gram(rng.standard_normal((n, 1024)), rng.standard_normal((n, 1024)))
    assert Gw.shape == (1024, 1024) and np.isfinite(Gw).all()
    bw, rest = plan.stat("bytes_gram"), plan.stat("bytes_device") + plan.stat("bytes_solve_many")
    print("bytes_gram", bw, "the rest", rest)
    assert bw >= 128 * n * W * 8 and bw > 0.5 * rest + (8 << 20)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    plan.close()
    grown = torch.cuda.mem_get_info(0)[0] - free_before
    print("freed by close()", grown)
    assert grown >= bw + 0.5 * rest
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
        plan.cross_gram(Cf, Bf)                                     # after close(): no handle


def test_alias_against_the_cholesky_gram():
    """cross_gram(B, B) on a symmetric matrix as LU is B^T A^-1 B, what CholPlan.gram(B) computes from another factorization of the
    same matrix: 1e-11 of max |G|"""
    N = 12
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    perm = nd_perm_py(N, N, N)
    Sl = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", True)
    Sc = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30)
    lu = _plan(Sl)
    ch = sf.CholPlan(Sc)
    ch.set_values(Sc.Lx)
    ch.factorize()
    B = np.random.default_rng(10).standard_normal((n, W + 3))
    G, Gc = lu.cross_gram(B, B), ch.gram(B)
    err = float(np.abs(G - Gc).max() / np.abs(Gc).max())
    print("cross_gram(B, B) against CholPlan.gram(B):", err)
    assert err <= 1e-11
    lu.close()
    ch.close()


def test_refusals():
    """a Cholesky plan at the LU entry points"""
    N = 8
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    Sc = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    ch = sf.CholPlan(Sc)
    ch.set_values(Sc.Lx)
    ch.factorize()
    assert _both_calls(ch, n) == ([SF_ERR_ARG] * 3, True)
    ch.close()
