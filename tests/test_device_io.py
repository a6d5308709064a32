"""The device-pointer entry points on torch tensors (CholPlan / LUPlan .set_ordering, .solve_device, .permute_device,
.sample_device, .set_values_device, .set_value_map, .set_values_mapped_device): the data-movement kernels bit for bit through
permute_device, the solves against the host-array calls of the same plan.

No test hands these calls a host pointer: the pointer check exists so that one cannot reach a kernel, and a test of it that
failed would fault the device it runs on."""
import types

import numpy as np
import pytest
import torch

from test_lu_pivot import pivot_cases
from util import sf, gen, nd_perm_py, small_cases

pytestmark = pytest.mark.gpu

W = 16
WIDTHS = (1, 3, W, W + 1)
DEV = "cuda:0"
SENTINEL = -7.25


def _close(got, want, rtol=1e-12, atol_rel=1e-13):
    """tests/test_half_solve.py::_close"""
    return np.allclose(got, want, rtol=rtol, atol=atol_rel * max(np.abs(want).max(), 1e-300))


def _cases():
    n, Cp, Ci, Cx = gen.laplacian_lower(7, 7, 7)
    return small_cases() + [("lap3d_7_gridnd", n, Cp, Ci, Cx, sf.grid_nd_perm(7, 7, 7), 1 << 30)]


def _colmajor(A, ld, fill=SENTINEL):
    """the (n, k) host array as a column-major device tensor with leading dimension ld, and the (ld, k) buffer under it"""
    n, k = A.shape
    buf = torch.full((k, ld), fill, dtype=torch.float64, device=DEV)
    T = buf.t()[:n]
    T.copy_(torch.from_numpy(np.ascontiguousarray(A)).to(DEV))
    assert T.stride() == (1, ld) or n <= 1 or k <= 1
    return T, buf.t()


def _empty(n, k, ld):
    buf = torch.full((k, ld), SENTINEL, dtype=torch.float64, device=DEV)
    return buf.t()[:n], buf.t()


def _host(T):
    return T.cpu().numpy()


def _perm_of(perm, n):
    return np.arange(n, dtype=np.int64) if perm is None else np.asarray(perm, dtype=np.int64)


def _unperm(A, perm):
    """the array whose rows perm[i] are the rows i of A: A in the caller's numbering"""
    out = np.empty_like(A)
    out[perm] = A
    return out


def _plan(case, factorize=True):
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    plan = sf.CholPlan(sym, device=0)
    if factorize:
        plan.set_values(sym.Lx)
        plan.factorize()
    return sym, plan, _perm_of(perm, n)


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_permute_device_bitwise(case):
    """load / store and pack / unpack with and without the ordering, nothing in between: exact"""
    sym, plan, perm = _plan(case, factorize=False)          # needs no values and no factor
    n = sym.n
    B = np.random.default_rng(1).standard_normal((n, W + 1))
    with pytest.raises(sf.SparseFrameError):
        plan.permute_device(_colmajor(B[:, :3], n)[0])      # no ordering yet
    plan.set_ordering(perm)
    assert plan.stat("bytes_ordering") == 4 * max(n, 1)
    for k in WIDTHS:
        for ldb, ldx in ((n, n), (n + 5, n + 5), (n, n + 5)):
            Bd, _ = _colmajor(B[:, :k], ldb)
            for inverse in (False, True):
                out, whole = _empty(n, k, ldx)
                got = plan.permute_device(Bd, out=out, inverse=inverse)
                assert got is out
                want = _unperm(B[:, :k], perm) if inverse else B[perm, :k]
                assert np.array_equal(_host(out), want), (k, ldb, ldx, inverse)
                assert np.all(_host(whole)[n:] == SENTINEL), (k, ldx, inverse)      # the rows between n and ld are not touched
                assert np.array_equal(_host(Bd), B[:, :k])
    # 1-D, and an output the call allocates
    b = torch.from_numpy(B[:, 0].copy()).to(DEV)
    x = plan.permute_device(b)
    assert tuple(x.shape) == (n,) and np.array_equal(_host(x), B[perm, 0])
    X = plan.permute_device(_colmajor(B, n)[0])
    assert tuple(X.shape) == (n, W + 1) and (n <= 1 or X.stride(0) == 1) and np.array_equal(_host(X), B[perm])
    # a C-contiguous input is taken by copy
    Xc = plan.permute_device(torch.from_numpy(B).to(DEV), inverse=True)
    assert np.array_equal(_host(Xc), _unperm(B, perm))
    # not in place; a non-permutation is refused and the stored ordering stays
    Bd, _ = _colmajor(B, n)
    with pytest.raises(sf.SparseFrameError):
        plan.permute_device(Bd, out=Bd)
    if n > 1:
        bad = perm.copy()
        bad[0] = bad[1]
        with pytest.raises(sf.SparseFrameError):
            plan.set_ordering(bad)
        bad[0] = n
        with pytest.raises(sf.SparseFrameError):
            plan.set_ordering(bad)
        assert np.array_equal(_host(plan.permute_device(b)), B[perm, 0])
    plan.set_ordering(None)
    assert np.array_equal(_host(plan.permute_device(b)), B[:, 0])
    plan.close()


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_solve_device(case):
    sym, plan, perm = _plan(case)
    n = sym.n
    B = np.random.default_rng(2).standard_normal((n, W + 1))
    want = {"solve": plan.solve_many(B), "half_L": plan.solve_half(B, "L"), "half_Lt": plan.solve_half(B, "Lt")}
    Bo = _unperm(B, perm)
    # flags without an ordering are refused
    with pytest.raises(sf.SparseFrameError):
        plan.solve_device(_colmajor(B, n)[0], perm_in=True)
    with pytest.raises(sf.SparseFrameError):
        plan.solve_device(_colmajor(B, n)[0], perm_out=True)
    plan.set_ordering(perm)
    for op in ("solve", "half_L", "half_Lt"):
        for k in WIDTHS:
            for ld in (n, n + 5):
                Bd, _ = _colmajor(B[:, :k], ld)
                out, whole = _empty(n, k, ld)
                plan.solve_device(Bd, out=out, op=op)
                X = _host(out)
                assert _close(X, want[op][:, :k]), (op, k, ld, float(np.abs(X - want[op][:, :k]).max()))
                assert np.all(_host(whole)[n:] == SENTINEL) and np.array_equal(_host(Bd), B[:, :k])
                stat = "last_half_ms" if op != "solve" else ("last_solve_ms" if k == 1 else "last_solve_many_ms")
                assert plan.stat(stat) > 0
            # the four combinations of the flags against the numpy-permuted host call, and in place
            for pin in (False, True):
                for pout in (False, True):
                    Bd, whole = _colmajor((Bo if pin else B)[:, :k], n + 5)
                    X = plan.solve_device(Bd, op=op, perm_in=pin, perm_out=pout)
                    got = _host(X)[perm] if pout else _host(X)
                    assert _close(got, want[op][:, :k]), (op, k, pin, pout)
                    Y = plan.solve_device(Bd, out=Bd, op=op, perm_in=pin, perm_out=pout)
                    assert Y is Bd
                    got = _host(Bd)[perm] if pout else _host(Bd)
                    assert _close(got, want[op][:, :k]), (op, k, pin, pout, "in place")
                    assert np.all(_host(whole)[n:] == SENTINEL)
    # 1-D right-hand side
    x = plan.solve_device(torch.from_numpy(Bo[:, 0].copy()).to(DEV), perm_in=True, perm_out=True)
    assert tuple(x.shape) == (n,) and _close(_host(x)[perm], want["solve"][:, 0])
    plan.close()


def test_caller_numbering_residual():
    """solve the caller's own system: |A x - b| from the UNPERMUTED matrix, the bound of the validate tests (test_edge_cases)"""
    name, n, Cp, Ci, Cx, perm, slot = _cases()[-1]
    sym, plan, perm = _plan(_cases()[-1])
    plan.set_ordering(perm)
    A = types.SimpleNamespace(n=n, Lp=np.asarray(Cp), Li=np.asarray(Ci), Lx=np.asarray(Cx, dtype=np.float64))
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n)
    x = _host(plan.solve_device(torch.from_numpy(b).to(DEV), perm_in=True, perm_out=True))
    res = sf.validate_solution(A, x, b)
    print(f"caller-numbering residual (1 column) = {res:.3e}")
    assert res <= 1e-13
    B = rng.standard_normal((n, W + 1))
    X = _host(plan.solve_device(_colmajor(B, n + 5)[0], perm_in=True, perm_out=True))
    for j in range(W + 1):
        res = sf.validate_solution(A, X[:, j], B[:, j])
        assert res <= 1e-13, (j, res)
    plan.close()


def test_column_independence():
    """a NaN in one column stays in that column (tests/test_solve_many.py::test_column_independence)"""
    sym, plan, perm = _plan(_cases()[-1])
    n = sym.n
    plan.set_ordering(perm)
    B = np.random.default_rng(5).standard_normal((n, W + 4))
    B[n // 2, 3] = np.nan
    B[7, W + 1] = np.inf
    B[:, 5] = 0.0
    X = _host(plan.solve_device(_colmajor(B, n + 5)[0], perm_in=True, perm_out=True))[perm]
    Bp = B[perm]
    assert np.all(X[:, 5] == 0.0)
    for j in range(B.shape[1]):
        if j in (3, W + 1):
            continue
        assert np.isfinite(X[:, j]).all(), j
        want = plan.solve(np.ascontiguousarray(Bp[:, j]))
        assert np.allclose(X[:, j], want, rtol=1e-13, atol=1e-13 * max(np.abs(want).max(), 1e-300)), j
    assert not np.isfinite(X[:, 3]).all() and not np.isfinite(X[:, W + 1]).all()
    plan.close()


def _lu_plan(n, Cp, Ci, Cx, perm, tol=0.0):
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, S.Ux)
    if tol:
        plan.set_pivoting(tol)
    plan.factorize()
    return S, plan


def test_lu_solve_device():
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(7, 7, 7, seed=5)
    perm = nd_perm_py(7, 7, 7)
    S, plan = _lu_plan(n, Cp, Ci, Cx, perm)
    plan.set_ordering(perm)
    B = np.random.default_rng(6).standard_normal((n, W + 1))
    Bo = _unperm(B, perm)
    for op, trans in (("solve", False), ("trans", True)):
        want = plan.solve_many(B, trans)
        for k in WIDTHS:
            for ld in (n, n + 5):
                X = _host(plan.solve_device(_colmajor(B[:, :k], ld)[0], op=op))
                assert _close(X, want[:, :k]), (op, k, ld)
            Bd, _ = _colmajor(Bo[:, :k], n + 5)
            plan.solve_device(Bd, out=Bd, op=op, perm_in=True, perm_out=True)
            assert _close(_host(Bd)[perm], want[:, :k]), (op, k, "caller's numbering, in place")
    with pytest.raises(ValueError):
        plan.solve_device(_colmajor(B, n)[0], op="half_L")
    assert not hasattr(plan, "sample_device")
    plan.close()


@pytest.mark.parametrize("case", [c for c in pivot_cases() if c[0] in ("dense_200_tol01", "zero_diag_12", "general_14_tol03")],
                         ids=lambda c: c[0])
def test_lu_solve_device_pivoting(oracle, case):
    """pivoting on: the bound of tests/test_solve_many.py::test_lu_with_pivoting, for the plain and (against the host call, which
    tests/test_lu_transposed.py holds to its own oracle) the transposed solve"""
    name, n, Cp, Ci, Cx, perm, tol, vtol = case
    S, plan = _lu_plan(n, Cp, Ci, Cx, perm, tol)
    piv = plan.get_pivots()
    assert np.count_nonzero(piv != np.arange(n)) > 0
    Lsx = plan.get_factor()
    rng = np.random.default_rng(4)
    B = rng.standard_normal((n, W + 1))
    X = _host(plan.solve_device(_colmajor(B, n + 5)[0]))
    XT = _host(plan.solve_device(_colmajor(B, n + 5)[0], op="trans"))
    XT_host = plan.solve_many(B, True)
    for j in range(B.shape[1]):
        want = oracle.lu_solve_pivot(S, Lsx, piv, B[:, j])
        spread = 0.0
        for _ in range(5):
            moved = Lsx * (1.0 + rng.integers(-1, 2, Lsx.size) * 1.1102230246251565e-16)
            spread = max(spread, float(np.max(np.abs(oracle.lu_solve_pivot(S, moved, piv, B[:, j]) - want)) / np.abs(want).max()))
        err = float(np.max(np.abs(X[:, j] - want)) / np.abs(want).max())
        err1 = float(np.max(np.abs(plan.solve(np.ascontiguousarray(B[:, j])) - want)) / np.abs(want).max())
        print(f"{name} column {j}: err {err:.3e} spread {spread:.3e} err1 {err1:.3e}")
        assert err <= max(1e-12, 8.0 * spread, 8.0 * err1), (name, j, err, spread, err1)
        x1 = _host(plan.solve_device(torch.from_numpy(B[:, j].copy()).to(DEV)))
        assert float(np.max(np.abs(x1 - want)) / np.abs(want).max()) <= max(1e-12, 8.0 * spread, 8.0 * err1), (name, j, "one column")
        errT = float(np.max(np.abs(XT[:, j] - XT_host[:, j])) / np.abs(XT_host[:, j]).max())
        assert errT <= max(1e-12, 8.0 * spread, 8.0 * err1), (name, j, errT)
    plan.close()


@pytest.mark.parametrize("case", [c for c in _cases() if c[0] in ("lap2d_8x8_nd", "band_500", "one_by_one", "lap3d_7_gridnd")],
                         ids=lambda c: c[0])
def test_values_from_device(case):
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    Cx = np.asarray(Cx, dtype=np.float64)
    Ax = Cx * (1.0 + 0.25 * np.random.default_rng(7).uniform(size=len(Cx)))        # other values on the same pattern
    Lx = sf.analyze(n, Cp, Ci, Ax, perm, slot).Lx
    rng = np.random.default_rng(8)
    b, x = rng.standard_normal(n), rng.standard_normal(n)
    B = rng.standard_normal((n, 3))
    host = sf.CholPlan(sym, device=0)
    host.set_values(Lx)
    r_want = host.residual(b, x)
    host.factorize()
    X_want = host.solve_many(B)
    nsrc, mapL, mapU = sym.value_map()
    for how in ("device", "mapped"):
        plan = sf.CholPlan(sym, device=0)
        plan.set_values(sym.Lx)
        plan.factorize()
        plan.selinv()
        assert plan.stat("selinv_valid") == 1
        if how == "device":
            plan.set_values_device(torch.from_numpy(Lx).to(DEV))
        else:
            bad = mapL.copy()
            bad[0] = nsrc
            with pytest.raises(sf.SparseFrameError):
                plan.set_value_map(nsrc, bad)
            bad[0] = -2
            with pytest.raises(sf.SparseFrameError):
                plan.set_value_map(nsrc, bad)
            with pytest.raises(ValueError):
                plan.set_values_mapped_device(torch.from_numpy(Ax).to(DEV))       # no map yet
            plan.set_value_map(nsrc, mapL, mapU)
            assert plan.stat("bytes_ordering") == 8 * max(sym.nnz, 1)
            plan.set_values_mapped_device(torch.from_numpy(Ax).to(DEV))
        assert plan.stat("selinv_valid") == 0
        r = plan.residual(b, x)
        assert np.array_equal(r[0], r_want[0]) and r[1] == r_want[1] and r[2] == r_want[2], how     # a fixed summation order: same bits
        plan.factorize()
        assert _close(plan.solve_many(B), X_want), how
        assert _close(_host(plan.solve_device(_colmajor(B, n)[0])), X_want), how
        plan.close()
    host.close()


def test_lu_values_from_device():
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(6, 5, 4, seed=3)
    perm = nd_perm_py(6, 5, 4)
    S = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
    Cx = np.asarray(Cx, dtype=np.float64)
    rng = np.random.default_rng(9)
    b, x = rng.standard_normal(n), rng.standard_normal(n)
    B = rng.standard_normal((n, 3))
    host = sf.LUPlan(S)
    host.set_values(S.Lx, S.Ux)
    r_want = host.residual(b, x)
    host.factorize()
    X_want = host.solve_many(B)
    nsrc, mapL, mapU = S.value_map()
    for how in ("device", "mapped"):
        plan = sf.LUPlan(S)
        if how == "device":
            plan.set_values_device(torch.from_numpy(S.Lx).to(DEV), torch.from_numpy(S.Ux).to(DEV))
        else:
            plan.set_value_map(nsrc, mapL, mapU)
            plan.set_values_mapped_device(torch.from_numpy(Cx).to(DEV))
        r = plan.residual(b, x)
        assert np.array_equal(r[0], r_want[0]) and r[1] == r_want[1], how
        plan.factorize()
        assert _close(plan.solve_many(B), X_want), how
        plan.close()
    host.close()


def test_sample_device():
    sym, plan, perm = _plan(_cases()[-1])
    n = sym.n
    plan.set_ordering(perm)
    K = W + 1
    want = plan.sample(K, seed=5, first=3)
    X = plan.sample_device(K, seed=5, first=3)
    assert tuple(X.shape) == (n, K) and _close(_host(X), want)
    assert plan.stat("last_sample_ms") > 0
    out, whole = _empty(n, K, n + 5)
    plan.sample_device(K, seed=5, first=3, out=out, perm_out=True)
    assert _close(_host(out)[perm], want) and np.all(_host(whole)[n:] == SENTINEL)
    # however a run is cut into calls: 17 in one call against 16 + 1
    A = _host(plan.sample_device(W, seed=5, first=3))
    Bb = _host(plan.sample_device(1, seed=5, first=3 + W))
    assert np.array_equal(np.hstack([A, Bb]), _host(X))
    plan.close()


def test_lifecycle():
    """the first solve-type call of a fresh plan is the backward half on device memory; again after new values from the device"""
    case = _cases()[-1]
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    B = np.random.default_rng(10).standard_normal((n, W + 1))
    ref = sf.CholPlan(sym, device=0)
    ref.set_values(sym.Lx)
    ref.factorize()
    want1 = ref.solve_half(B, "Lt")
    ref.set_values(2.0 * sym.Lx)
    ref.factorize()
    want2 = ref.solve_half(B, "Lt")
    ref.close()

    plan = sf.CholPlan(sym, device=0)
    plan.set_values(sym.Lx)
    Bd, _ = _colmajor(B, n)
    with pytest.raises(sf.SparseFrameError):
        plan.solve_device(Bd)                       # no factorization yet
    plan.factorize()
    assert plan.stat("bytes_solve_many") == 0
    assert _close(_host(plan.solve_device(Bd, op="half_Lt")), want1)
    assert plan.stat("bytes_solve_many") == 2 * n * W * 8
    plan.set_values_device(torch.from_numpy(2.0 * sym.Lx).to(DEV))
    plan.factorize()
    assert _close(_host(plan.solve_device(Bd, op="half_Lt")), want2)
    assert _close(_host(plan.solve_device(Bd[:, 0].contiguous(), op="half_Lt")), want2[:, 0])
    # a factorization that failed: refused until one succeeds
    neg = sym.Lx.copy()
    neg[sym.Li == np.repeat(np.arange(n), np.diff(sym.Lp))] = -1.0        # a negative diagonal
    plan.set_values_device(torch.from_numpy(neg).to(DEV))
    with pytest.raises(sf.SparseFrameError):
        plan.factorize()
    with pytest.raises(sf.SparseFrameError):
        plan.solve_device(Bd)
    with pytest.raises(sf.SparseFrameError):
        plan.sample_device(3)
    plan.set_values(sym.Lx)
    plan.factorize()
    assert _close(_host(plan.solve_device(Bd, op="half_Lt")), want1)
    plan.close()
