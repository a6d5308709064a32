"""sf_chol_plan_gram / _gram_device (CholPlan.gram, .gram_device, .schur, .solve_bordered): the dense Schur complement of a border,
G = B^T A^-1 B = Y^T Y with Y = L^-1 B, against tests/gram_ref.py over the plan's own factor.

The acceptance bound is componentwise, |G - Gref|_ij <= tol (|Y|^T |Y|)_ij with Y from the numpy sweeps: tol = 1e-12 on the small
cases and 1e-11 at 34^3, the half solves' own tolerances at those sizes (tests/test_half_solve.py) carried through a dot product.

Bit-for-bit statements are made where they can hold.  The reduction Y^T Y has a fixed order, but the forward sweep before it
(sf_solve.hip, not part of this feature) adds the tiles' contributions to a row with floating-point atomics, in the order the
workgroups happen to arrive: two sweeps of the same block differ in the last bit of some entries.  Measured on the 16^3
Laplacian, k = 33: 6,000 - 7,200 of the 135,168 entries of Y and 640 - 700 of the 1,089 entries of G differ between two calls,
by at most 1.2e-16 relative to max |G|; on band_500 two one-column calls differed by one ulp (201.39904796825795 against
...797).  So "the same bits as another call" (gram against quadform, a NaN column against the clean run, call against call) is
asserted where the sweep has nothing to reorder -- no supernode with rows below its diagonal block -- and against the
componentwise bound elsewhere; symmetry, which is a property of one call, is asserted bit for bit everywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import gram_ref
from util import sf, gen, small_cases

pytestmark = pytest.mark.gpu

W = 16
DEV = "cuda:0"
SF_OK, SF_ERR_ARG = 0, 1
KS = (1, 3, W, W + 1, 2 * W + 1)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _chol_plan(sym):
    plan = sf.CholPlan(sym, device=0)
    plan.set_values(sym.Lx)
    plan.factorize()
    return plan, plan.get_factor()


def _lap(N):
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    return sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 4 << 30)


def _identity(n):
    return sf.analyze(n, np.arange(n + 1), np.arange(n), np.ones(n), None, 1 << 30)


def _no_scatter(sym):
    """no supernode has rows below its diagonal block: the forward sweep adds nothing with atomics, so it repeats bit for bit"""
    return bool(np.all(np.diff(sym.Lsip) == np.diff(sym.Super)))


def _dev(A):
    """the (n, k) host array as a column-major device tensor"""
    return torch.from_numpy(np.ascontiguousarray(A.T)).to(DEV).t()


def _check(G, Gref, Y, tol, what):
    ok, ratio = gram_ref.within(G, Gref, Y, tol)
    print(f"{what}: max |G - Gref| / (|Y|^T |Y|) = {ratio:.3e} (tol {tol:.0e})")
    assert ok, (what, ratio)


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_small_cases(case):
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    plan, Lsx = _chol_plan(sym)
    B = np.random.default_rng(1).standard_normal((n, KS[-1]))
    Gref, Y = gram_ref.gram(sym, Lsx, B)
    got = {}
    for k in KS:
        G = plan.gram(B[:, :k])
        assert G.shape == (k, k) and G.dtype == np.float64
        _check(G, Gref[:k, :k], Y[:, :k], 1e-12, f"{name} k={k}")
        assert np.array_equal(G, G.T), k
        got[k] = G
    # one column is quadform's own path -- the same bits where the sweep scatters nothing, two runs of one code path elsewhere;
    # the diagonal is quadform's in general
    b = np.ascontiguousarray(B[:, 0])
    g1, q1 = plan.gram(b), plan.quadform(b)
    assert isinstance(g1, float)
    if _no_scatter(sym):
        assert g1 == q1 and g1 == got[1][0, 0], (g1, q1, got[1][0, 0])
    else:
        assert np.isclose(g1, q1, rtol=1e-13, atol=0.0) and np.isclose(g1, got[1][0, 0], rtol=1e-13, atol=0.0), (g1, q1, got[1][0, 0])
    q = plan.quadform(B[:, :W + 1])
    assert np.allclose(np.diag(got[W + 1]), q, rtol=1e-13, atol=0.0), (np.diag(got[W + 1]), q)
    plan.close()


@pytest.mark.parametrize("n", [4099, 3])
def test_exact_on_the_identity(n):
    """A = I, integer B: every intermediate is a small integer, so the result is exact -- a row dropped or counted twice at the
    tail, at a slab boundary or between the waves' groups changes it.  4099 is prime: no multiple of 4, of 64 or of a slab"""
    sym = _identity(n)
    plan, _ = _chol_plan(sym)
    k = 2 * W + 1
    B = np.random.default_rng(2).integers(-8, 9, size=(n, k)).astype(np.float64)
    G = plan.gram(B)
    assert np.array_equal(G, B.T @ B)
    if n >= 4096:
        assert plan.stat("last_gram_parts") >= 2
    else:
        assert plan.stat("last_gram_parts") == 1
    # the reduction has a fixed order: the same bits on every call (the sweep has nothing to reorder here)
    assert _no_scatter(sym)
    for _ in range(2):
        assert np.array_equal(plan.gram(B), G)
    # one column: exactly quadform's value; a NaN column: every entry outside its row and column keeps its bits
    b = np.ascontiguousarray(B[:, 5])
    assert plan.gram(b) == plan.quadform(b) == float(b @ b) == G[5, 5]
    j = 20
    Bn = B.copy()
    Bn[n // 2, j] = np.nan
    Gn = plan.gram(Bn)
    keep = np.arange(k) != j
    assert np.isnan(Gn[j, :]).all() and np.isnan(Gn[:, j]).all()
    assert np.array_equal(Gn[np.ix_(keep, keep)], G[np.ix_(keep, keep)])
    plan.close()


def test_wide_supernodes():
    N = 34
    sym = _lap(N)
    n = sym.n
    assert np.diff(sym.Super).max() > 1024
    plan, Lsx = _chol_plan(sym)
    k = W + 3
    B = np.random.default_rng(3).standard_normal((n, k))
    Gref, Y = gram_ref.gram(sym, Lsx, B)
    G = plan.gram(B)
    _check(G, Gref, Y, 1e-11, "34^3 k=19")
    assert np.array_equal(G, G.T)
    assert plan.stat("last_gram_parts") >= 2 and plan.stat("last_gram_ms") > 0
    # new values, the same plan: A doubled halves the result
    plan.set_values(2.0 * sym.Lx)
    plan.factorize()
    G2 = plan.gram(B)
    _check(G2, 0.5 * G, Y / np.sqrt(2.0), 1e-11, "34^3 k=19, 2 A against half the first")
    plan.close()


def test_column_containment():
    """a NaN in column 20 of B reaches row 20 and column 20 of G and nothing else: there all is NaN, everywhere else the NaN run
    is as good as the clean one.  Bit-identity with the clean run is asserted in test_exact_on_the_identity -- here two clean
    runs already differ in the last bit of some 650 of the 1,089 entries (see the top of the file), and a first version of this
    test that compared bits counted 618 differing entries outside row and column 20"""
    sym = _lap(16)
    n = sym.n
    plan, Lsx = _chol_plan(sym)
    k, j = 2 * W + 1, 20
    B = np.random.default_rng(4).standard_normal((n, k))
    Gref, Y = gram_ref.gram(sym, Lsx, B)
    clean = plan.gram(B)
    _check(clean, Gref, Y, 1e-12, "16^3 k=33, clean")
    Bn = B.copy()
    Bn[:, j] = np.nan
    G = plan.gram(Bn)
    keep = np.arange(k) != j
    assert np.isnan(G[j, :]).all() and np.isnan(G[:, j]).all()
    sub = np.ix_(keep, keep)
    assert np.isfinite(G[sub]).all()
    _check(G[sub], Gref[sub], Y[:, keep], 1e-12, "16^3 k=33, column 20 NaN, outside row / column 20")
    diff = int((G[sub] != clean[sub]).sum())
    print(f"entries outside row / column {j} whose bits differ from the clean run: {diff} of {(k - 1) ** 2}")
    # an Inf behaves the same
    Bn[:, j] = B[:, j]
    Bn[7, j] = np.inf
    G = plan.gram(Bn)
    assert not np.isfinite(G[j, :]).any() and not np.isfinite(G[:, j]).any() and np.isfinite(G[sub]).all()
    _check(G[sub], Gref[sub], Y[:, keep], 1e-12, "16^3 k=33, an Inf in column 20, outside row / column 20")
    plan.close()


def test_symmetry_bitwise():
    sym = _lap(16)
    plan, _ = _chol_plan(sym)
    B = np.random.default_rng(5).standard_normal((sym.n, 2 * W + 1))
    for _ in range(2):
        G = plan.gram(B)
        assert np.array_equal(G, G.T)
    plan.close()


def test_device_entry():
    N = 12
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    perm = np.asarray(sf.grid_nd_perm(N, N, N), dtype=np.int64)
    sym = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30)
    plan, Lsx = _chol_plan(sym)
    k = 2 * W + 1
    B = np.random.default_rng(6).standard_normal((n, k))
    Gref, Y = gram_ref.gram(sym, Lsx, B)
    Bd = _dev(B)
    with pytest.raises(sf.SparseFrameError):
        plan.gram_device(Bd, perm_in=True)                  # a flag without an ordering
    for kk in (1, 3, k):
        Gd = plan.gram_device(Bd[:, :kk])
        assert tuple(Gd.shape) == (kk, kk) and Gd.dtype == torch.float64
        G = Gd.cpu().numpy()
        _check(G, Gref[:kk, :kk], Y[:, :kk], 1e-12, f"gram_device k={kk}")
        assert np.array_equal(G, G.T)
        _check(G, plan.gram(B[:, :kk]), Y[:, :kk], 1e-12, f"gram_device against gram k={kk}")
    g1 = plan.gram_device(Bd[:, 0].contiguous())
    assert tuple(g1.shape) == (1, 1)
    _check(g1.cpu().numpy(), Gref[:1, :1], Y[:, :1], 1e-12, "gram_device 1-D")
    # the caller's numbering: row perm[i] of the block is row i of the permuted system
    plan.set_ordering(perm)
    Bo = np.empty_like(B)
    Bo[perm] = B
    assert np.array_equal(Bo[perm], B)
    for kk in (1, k):
        G = plan.gram_device(_dev(Bo[:, :kk]), perm_in=True).cpu().numpy()
        _check(G, Gref[:kk, :kk], Y[:, :kk], 1e-12, f"gram_device perm_in k={kk}")
    # out= is honoured, with a leading dimension of its own; what lies between its columns is not touched
    ldg = k + 5
    buf = torch.full((k, ldg), -7.25, dtype=torch.float64, device=DEV)
    out = buf.t()[:k]
    assert plan.gram_device(Bd, out=out) is out
    whole = buf.t().cpu().numpy()
    _check(whole[:k], Gref, Y, 1e-12, "gram_device out=")
    assert np.all(whole[k:] == -7.25)
    # refused: the wrong device, too short a tensor, a result that overlaps the block.  (No call here hands the library a pointer
    # that is not the device's, or a block that ends past its allocation: see tests/test_device_io.py)
    with pytest.raises(ValueError):
        plan.gram_device(torch.from_numpy(B))
    with pytest.raises(ValueError):
        plan.gram_device(_dev(B[:n - 1]))
    with pytest.raises(ValueError):
        plan.gram_device(Bd, out=torch.empty((k - 1, k - 1), dtype=torch.float64, device=DEV).t())
    before = Bd.clone()
    with pytest.raises(sf.SparseFrameError):
        plan.gram_device(Bd, out=Bd[:k])                    # column-major (k, k) with the block's leading dimension: inside B
    assert torch.equal(Bd, before)
    lib = sf.lib
    Gd = torch.empty((k, k), dtype=torch.float64, device=DEV)
    assert lib.sf_chol_plan_gram_device(plan._h, 2, k, Bd.data_ptr(), n, Gd.data_ptr(), k) == SF_ERR_ARG      # SF_DEV_PERM_OUT
    assert lib.sf_chol_plan_gram_device(plan._h, 0, 0, Bd.data_ptr(), n, Gd.data_ptr(), 1) == SF_OK
    plan.close()


def test_layouts():
    sym = _lap(12)
    n = sym.n
    plan, Lsx = _chol_plan(sym)
    k = W + 2
    B = np.random.default_rng(7).standard_normal((n, k))
    Gref, Y = gram_ref.gram(sym, Lsx, B)
    _check(plan.gram(np.ascontiguousarray(B)), Gref, Y, 1e-12, "C order")
    ldb, ldg = n + 5, k + 3
    Bp = np.full((ldb, k), 7.0, order="F")
    Bp[:n] = B
    Gp = np.full((ldg, k + 1), -3.0, order="F")
    lib = sf.lib
    assert lib.sf_chol_plan_gram(plan._h, k, _dp(Bp), ldb, _dp(Gp), ldg) == SF_OK
    _check(Gp[:k, :k], Gref, Y, 1e-12, "ldb > n, ldg > k")
    assert np.all(Gp[k:] == -3.0) and np.all(Gp[:, k] == -3.0) and np.all(Bp[n:] == 7.0)
    assert lib.sf_chol_plan_gram(plan._h, 0, _dp(Bp), ldb, _dp(Gp), ldg) == SF_OK and np.all(Gp[k:] == -3.0)
    assert lib.sf_chol_plan_gram(plan._h, 1, _dp(Bp), ldb, _dp(Gp), ldg) == SF_OK
    assert Gp[0, 0] == plan.quadform(B[:, 0].copy()) and np.all(Gp[k:] == -3.0)
    assert plan.gram(np.empty((n, 0))).shape == (0, 0)
    with pytest.raises(ValueError):
        plan.gram(np.ones((n + 1, 2)))
    with pytest.raises(ValueError):
        plan.gram(np.ones((n, 1025)))
    plan.close()


@pytest.mark.parametrize("with_C", [False, True], ids=["C=0", "C=I"])
def test_schur_and_bordered_solve(with_C):
    sym = _lap(16)
    n, k = sym.n, 5
    plan, _ = _chol_plan(sym)
    rng = np.random.default_rng(8)
    B = rng.standard_normal((n, k))
    f, g = rng.standard_normal(n), rng.standard_normal(k)
    C_ = np.eye(k) if with_C else None
    x, y = plan.solve_bordered(B, f, g, C_)
    assert x.shape == (n,) and y.shape == (k,)
    res = gram_ref.bordered_residual(sym, B, C_, x, y, f, g)
    print(f"bordered residual: {res:.3e}")
    assert res <= 1e-10
    # schur(B, D) = D - gram(B); with D = -C it is minus the matrix solve_bordered factors
    D = rng.standard_normal((k, k))
    G = plan.gram(B)
    assert np.allclose(plan.schur(B, D), D - G, rtol=1e-13, atol=1e-13 * np.abs(G).max())
    if not with_C:
        Bs = B.copy()
        Bs[:, 3] = Bs[:, 1]
        with pytest.raises(ValueError, match="rank-deficient"):
            plan.solve_bordered(Bs, f, g)
        # ... which C makes up for
        x, y = plan.solve_bordered(Bs, f, g, np.eye(k))
        assert gram_ref.bordered_residual(sym, Bs, np.eye(k), x, y, f, g) <= 1e-10
    plan.close()


def _both_calls(plan, n):
    B = np.ones((n, 3), order="F")
    G = np.full((3, 3), 7.0, order="F")
    Bd = _dev(B)
    Gd = torch.full((3, 3), 7.0, dtype=torch.float64, device=DEV)
    lib = sf.lib
    rc = [lib.sf_chol_plan_gram(plan._h, 3, _dp(B), n, _dp(G), 3), lib.sf_chol_plan_gram(plan._h, 1, _dp(B), n, _dp(G), 3),
          lib.sf_chol_plan_gram_device(plan._h, 0, 3, Bd.data_ptr(), n, Gd.data_ptr(), 3)]
    untouched = bool(np.all(G == 7.0)) and bool((Gd == 7.0).all())
    return rc, untouched


def test_plan_lifecycle():
    sym = _lap(14)
    n = sym.n
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx)
    assert _both_calls(plan, n) == ([SF_ERR_ARG] * 3, True)         # before any factorization
    plan.factorize()
    Lsx = plan.get_factor()
    bytes_before = plan.stat("bytes_device")
    assert plan.stat("bytes_gram") == 0
    rng = np.random.default_rng(9)
    B = rng.standard_normal((n, 2 * W + 1))
    Gref, Y = gram_ref.gram(sym, Lsx, B)
    assert plan.gram(B[:, 0].copy()) > 0 and plan.stat("last_gram_ms") > 0
    assert plan.stat("bytes_gram") == 0 and plan.stat("last_gram_parts") == 0      # one column: no store
    _check(plan.gram(B[:, :3]), Gref[:3, :3], Y[:, :3], 1e-12, "k=3")
    b1 = plan.stat("bytes_gram")
    assert b1 >= n * W * 8 and plan.stat("last_gram_parts") >= 1 and plan.stat("last_gram_ms") > 0
    _check(plan.gram(B[:, :W]), Gref[:W, :W], Y[:, :W], 1e-12, "k=16")
    assert plan.stat("bytes_gram") == b1                            # still one chunk
    _check(plan.gram(B[:, :W + 1]), Gref[:W + 1, :W + 1], Y[:, :W + 1], 1e-12, "k=17")
    b2 = plan.stat("bytes_gram")
    assert b2 > b1 and b2 >= 2 * n * W * 8                          # two chunks: the store has grown
    _check(plan.gram(B), Gref, Y, 1e-12, "k=33")
    b3 = plan.stat("bytes_gram")
    assert b3 > b2 and b3 >= 3 * n * W * 8
    _check(plan.gram(B[:, :5]), Gref[:5, :5], Y[:, :5], 1e-12, "k=5 after k=33")
    assert plan.stat("bytes_gram") == b3                            # a smaller block reuses it
    assert plan.stat("bytes_device") == bytes_before
    # a failed factorization (non-positive pivot): refused until one succeeds, and the plan stays usable
    bad = sym.Lx.copy()
    cols = np.repeat(np.arange(n), np.diff(sym.Lp))
    bad[(sym.Li == cols) & (cols == n // 2)] = -1.0
    plan.set_values(bad)
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_NOT_POSDEF"):
        plan.factorize()
    assert _both_calls(plan, n) == ([SF_ERR_ARG] * 3, True)
    plan.set_values(sym.Lx)
    assert _both_calls(plan, n) == ([SF_ERR_ARG] * 3, True)         # still no successful factorization
    plan.factorize()
    assert _both_calls(plan, n)[0] == [SF_OK] * 3
    _check(plan.gram(B), Gref, Y, 1e-12, "k=33 after the refactorization")
    assert plan.stat("bytes_gram") == b3 and plan.stat("bytes_device") == bytes_before
    # close() frees the store: with 1024 columns it is several times everything else the plan holds, so the device's free memory
    # cannot grow by its size unless it is among what is freed
    Gw = plan.gram(rng.standard_normal((n, 1024)))
    assert np.array_equal(Gw, Gw.T) and np.isfinite(Gw).all()
    bw = plan.stat("bytes_gram")
    assert bw >= 64 * n * W * 8 and bw > 4 * (plan.stat("bytes_device") + plan.stat("bytes_solve_many"))
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    plan.close()
    assert torch.cuda.mem_get_info(0)[0] >= free_before + bw


def test_refusals():
    """an LU plan and an out-of-core plan (tests/test_half_solve.py::test_refusals)"""
    from util import nd_perm_py
    N = 8
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
    S = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", False)
    lu = sf.LUPlan(S)
    lu.set_values(S.Lx, S.Ux)
    lu.factorize()
    assert _both_calls(lu, n) == ([SF_ERR_ARG] * 3, True)
    lu.close()
    N = 12
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    S = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    total = int((np.diff(S.Super) * np.diff(S.Lsip)).sum())
    g, ng, ge, te, nd, fits = sf.ooc_partition(S, int(total * 0.6))
    assert ng >= 2
    ooc = sf.CholPlan(S, ooc_group=g, ooc_ngroups=ng)
    assert _both_calls(ooc, n) == ([SF_ERR_ARG] * 3, True)
    with pytest.raises(sf.SparseFrameError):
        ooc.gram(np.ones((n, 2)))
    ooc.close()
