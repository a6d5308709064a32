"""sf_chol_plan_sample (CholPlan.sample): x = L^-T z with standard normals z generated on the device -- the stream against its numpy
statement (tests/sample_ref.py), the sweep against the numpy half solve, and the distribution against the selected inverse."""
import ctypes as C

import numpy as np
import pytest

import sample_ref
from util import sf, gen

pytestmark = pytest.mark.gpu

W = 16
SF_OK = 0


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _chol_plan(sym):
    plan = sf.CholPlan(sym, device=0)
    plan.set_values(sym.Lx)
    plan.factorize()
    return plan, plan.get_factor()


@pytest.fixture(scope="module")
def lap16():
    """the 16^3 plan, its factor, and the first 40 samples of stream 5 with their normals"""
    N = 16
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    plan, Lsx = _chol_plan(sym)
    X, Z = plan.sample(40, seed=5, return_z=True)       # (the first solve-type call of the plan)
    yield sym, plan, Lsx, X, Z
    plan.close()


def test_stream_and_sweep(lap16):
    sym, plan, Lsx, X, Z = lap16
    n = sym.n
    assert X.shape == (n, 40) and Z.shape == (n, 40)
    # device and numpy log / cos / sin / sqrt each within about 1e-14 of the exact value for |z| <= 8.6; a wrong stream is off by O(1)
    want = sample_ref.normals(5, n, 0, 40)
    err = float(np.abs(Z - want).max())
    print(f"max |Z - reference normals| = {err:.3e}")
    assert err <= 1e-13
    ref = sample_ref.half_solve(sym, Lsx, Z, "Lt")
    assert np.allclose(X, ref, rtol=1e-12, atol=1e-13 * np.abs(ref).max())
    assert plan.stat("last_sample_ms") > 0


def test_chunk_independence(lap16):
    sym, plan, Lsx, X, Z = lap16
    # an odd first sample: every Box-Muller pair lies across two columns of the chunk
    X5, Z5 = plan.sample(5, seed=5, first=17, return_z=True)
    assert np.array_equal(Z5, Z[:, 17:22])
    tol = 1e-13 * np.abs(X).max()           # (the sweeps scatter with atomics: equal to rounding)
    assert np.abs(X5 - X[:, 17:22]).max() <= tol
    X16, Z16 = plan.sample(W, seed=5, first=W + 2, return_z=True)
    assert np.array_equal(Z16, Z[:, W + 2:2 * W + 2])
    assert np.abs(X16 - X[:, W + 2:2 * W + 2]).max() <= tol
    # another seed is another stream; without Z the same samples
    _, Z6 = plan.sample(5, seed=6, first=17, return_z=True)
    assert np.abs(Z6 - Z5).max() > 0.1
    Xn = plan.sample(40, seed=5)
    assert isinstance(Xn, np.ndarray) and np.abs(Xn - X).max() <= tol
    # 64-bit seeds and sample numbers
    seed, first = (1 << 63) + 12345, (1 << 40) + 3
    _, Zb = plan.sample(3, seed=seed, first=first, return_z=True)
    assert np.abs(Zb - sample_ref.normals(seed, sym.n, first, 3)).max() <= 1e-13
    assert plan.sample(0, seed=5).shape == (sym.n, 0)


def test_flat_abi_leading_dimensions(lap16):
    sym, plan, Lsx, X, Z = lap16
    n = sym.n
    k = W + 3
    ldx, ldz = n + 7, n + 3
    Xp = np.full((ldx, k), -3.0, order="F")
    Zp = np.full((ldz, k), 7.0, order="F")
    assert sf.lib.sf_chol_plan_sample(plan._h, k, 5, 0, _dp(Xp), ldx, _dp(Zp), ldz) == SF_OK
    assert np.array_equal(Zp[:n], Z[:, :k]) and np.all(Zp[n:] == 7.0)
    assert np.abs(Xp[:n] - X[:, :k]).max() <= 1e-13 * np.abs(X).max() and np.all(Xp[n:] == -3.0)
    Xq = np.full((ldx, k), -3.0, order="F")
    assert sf.lib.sf_chol_plan_sample(plan._h, k, 5, 0, _dp(Xq), ldx, None, 0) == SF_OK
    assert np.abs(Xq[:n] - X[:, :k]).max() <= 1e-13 * np.abs(X).max() and np.all(Xq[n:] == -3.0)
    assert sf.lib.sf_chol_plan_sample(plan._h, 0, 5, 0, _dp(Xq), ldx, None, 0) == SF_OK
    x1, z1 = np.full(ldx, -3.0), np.full(ldz, 7.0)
    assert sf.lib.sf_chol_plan_sample(plan._h, 1, 5, 0, _dp(x1), ldx, _dp(z1), ldz) == SF_OK        # one sample
    assert np.array_equal(z1[:n], Z[:, 0]) and np.all(z1[n:] == 7.0)
    assert np.abs(x1[:n] - X[:, 0]).max() <= 1e-13 * np.abs(X).max() and np.all(x1[n:] == -3.0)


def test_distribution_against_selinv():
    """Cov(x) = A^-1: the per-row second moment of 4096 samples against diag(A^-1) from the selected inverse.  A second moment of
    4096 normals has relative standard deviation sqrt(2 / 4096); the largest of the 216 deviations is capped at five of them (the
    numpy reference alone gives 3.07 for this matrix, seed and count)"""
    n, Cp, Ci, Cx = gen.laplacian_lower(6, 6, 6, diag=6.1)
    sym = sf.analyze(n, Cp, Ci, Cx, None, 1 << 30)
    plan, _ = _chol_plan(sym)
    K = 4096
    X = plan.sample(K, seed=11)
    plan.selinv()
    var = plan.selinv_diag()
    m2 = (X * X).mean(axis=1)
    dev = float(np.abs(m2 / var - 1.0).max() / np.sqrt(2.0 / K))
    print(f"largest deviation of a row's second moment: {dev:.3f} sigma")
    assert dev <= 5.0
    plan.close()
