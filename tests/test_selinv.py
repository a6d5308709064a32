"""sf_chol_plan_selinv / _get_selinv_range / _selinv_diag / _logdet (CholPlan.selinv, get_selinv, selinv_diag, logdet): the
selected inverse of a resident Cholesky factor against dense inverses, against solve_many columns on a matrix with supernodes of
several 512-column units, and against the closed forms of the Dirichlet Laplacian at full size."""
import ctypes as C

import numpy as np
import pytest

from util import sf, gen, dense_reference_factor, panel_entries_from_dense, rel_err
from selinv_ref import flops as ref_flops, UW
from test_selinv_abi import selinv_cases

pytestmark = pytest.mark.gpu


def _plan(sym):
    plan = sf.CholPlan(sym, device=0)
    plan.set_values(sym.Lx)
    plan.factorize()
    return plan


def arena_diag(sym, S):
    cols = np.arange(sym.n)
    s = sym.SuperMap[cols]
    nsrow = np.diff(sym.Lsip)[s]
    return S[sym.Lsxp[s] + (cols - sym.Super[s]) * (nsrow + 1)]


def laplacian_eigs(N):
    c = 2.0 * np.cos(np.arange(1, N + 1) * np.pi / (N + 1))
    return 6.0 - c[:, None, None] - c[None, :, None] - c[None, None, :]


@pytest.mark.parametrize("case", selinv_cases(), ids=lambda c: c[0])
def test_dense_reference(case):
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    plan = _plan(sym)
    assert plan.stat("selinv_valid") == 0
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    assert plan.stat("flops_selinv") == pytest.approx(ref_flops(sym), rel=1e-12)
    A, _ = dense_reference_factor(sym)
    S = plan.get_selinv()
    assert rel_err(S, panel_entries_from_dense(sym, np.linalg.inv(A))) <= 1e-11, name
    assert np.array_equal(plan.selinv_diag(), arena_diag(sym, S))
    sign, ld = np.linalg.slogdet(A)
    assert sign > 0 and abs(plan.logdet() - ld) <= 1e-11 * max(1.0, abs(ld))
    plan.close()


def test_wide_supernodes_against_solve_many():
    N = 34
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    ncol = np.diff(sym.Super)
    assert ncol.max() > 1024
    plan = _plan(sym)
    plan.selinv()
    S = plan.get_selinv()
    cols = []
    for s in np.argsort(-ncol)[:4]:                    # the widest supernodes: first, last and unit-boundary columns
        c0, c1 = sym.Super[s], sym.Super[s + 1]
        cols += [c0, c1 - 1] + [c0 + k for k in range(UW, c1 - c0, UW)] + [c0 + k - 1 for k in range(UW, c1 - c0, UW)]
    below = np.nonzero(ncol < np.diff(sym.Lsip))[0]
    parents = sym.SuperMap[sym.Lsi[sym.Lsip[below] + ncol[below]]]
    leaves = np.setdiff1d(np.arange(sym.nsuper), parents)
    rng = np.random.default_rng(4)
    cols += [int(sym.Super[s]) for s in rng.choice(leaves, 48 - len(cols), replace=False)]
    cols = np.array(sorted(set(int(c) for c in cols)))
    E = np.zeros((n, len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    X = plan.solve_many(E)
    for k, j in enumerate(cols):
        s = sym.SuperMap[j]
        nsrow = sym.Lsip[s + 1] - sym.Lsip[s]
        c = j - sym.Super[s]
        rows = sym.Lsi[sym.Lsip[s]:sym.Lsip[s + 1]]
        got = S[sym.Lsxp[s] + c * nsrow: sym.Lsxp[s] + (c + 1) * nsrow]
        want = X[rows, k]
        assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want)), j
    assert np.array_equal(plan.selinv_diag(), arena_diag(sym, S))
    logdet = float(np.sum(np.log(laplacian_eigs(N))))
    assert abs(plan.logdet() - logdet) <= 1e-11 * abs(logdet)
    plan.close()


def test_nothing_else_changes():
    N = 16
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    plan = _plan(sym)
    b = 1.0 + np.arange(n) / n
    F0, x0, x0b = plan.get_factor().copy(), plan.solve(b), plan.solve(b)
    plan.selinv()
    S1 = plan.get_selinv().copy()
    assert np.array_equal(plan.get_factor(), F0)
    # the device solve's forward sweep adds into x with atomics, so two solves of one factor may differ in the last bits: the solve
    # after selinv() must stay within that run-to-run spread (floor: 8 ulp of the largest entry)
    spread = max(float(np.max(np.abs(x0b - x0))), 8 * np.finfo(float).eps * float(np.max(np.abs(x0))))
    assert float(np.max(np.abs(plan.solve(b) - x0))) <= spread
    plan.selinv()
    assert np.array_equal(plan.get_selinv(), S1)
    plan.set_values(4.0 * sym.Lx)
    assert plan.stat("selinv_valid") == 0
    with pytest.raises(sf.SparseFrameError):
        plan.get_selinv()
    with pytest.raises(sf.SparseFrameError):
        plan.selinv()                           # the resident factor is not one of the current values
    with pytest.raises(sf.SparseFrameError):
        plan.logdet()
    plan.factorize()
    assert plan.stat("selinv_valid") == 0
    with pytest.raises(sf.SparseFrameError):
        plan.selinv_diag()
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    assert rel_err(plan.get_selinv(), S1 / 4.0) <= 1e-14
    plan.close()


def _closed_form_entry(N, lam, p, q):
    """A^-1(p, q) = sum_lambda v(p) v(q) / lambda over the sine eigenvectors (grid ids in the original ordering)"""
    k = np.arange(1, N + 1)
    f = []
    for a, b in ((p % N, q % N), ((p // N) % N, (q // N) % N), (p // (N * N), q // (N * N))):
        f.append(np.sin(k * np.pi * (a + 1) / (N + 1)) * np.sin(k * np.pi * (b + 1) / (N + 1)) * 2.0 / (N + 1))
    return float(np.einsum("i,j,k,ijk->", f[0], f[1], f[2], 1.0 / lam))


def test_full_size_128cubed_closed_forms():
    N = 128
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N, 3, 1), sf.REFERENCE_SLOT_1GPU)
    plan = _plan(sym)
    plan.selinv()
    lam = laplacian_eigs(N)
    d = plan.selinv_diag()
    assert abs(d.sum() - float(np.sum(1.0 / lam))) <= 1e-10 * float(np.sum(1.0 / lam))
    perm = np.asarray(sym.Perm)
    rng = np.random.default_rng(128)
    for j in rng.choice(n, 16, replace=False):
        want = _closed_form_entry(N, lam, perm[j], perm[j])
        assert abs(d[j] - want) <= 1e-10 * abs(want), j
    nscol, nsrow = np.diff(sym.Super), np.diff(sym.Lsip)
    has_below = np.nonzero(nsrow > nscol)[0]
    out = np.zeros(1)
    for s in rng.choice(has_below, 16, replace=False):
        c = int(rng.integers(nscol[s]))
        r = int(rng.integers(nscol[s], nsrow[s]))
        e = int(sym.Lsxp[s] + c * nsrow[s] + r)
        sf.lib.sf_chol_plan_get_selinv_range(plan._h, e, e + 1, out.ctypes.data_as(C.POINTER(C.c_double)))
        i, j = int(sym.Lsi[sym.Lsip[s] + r]), int(sym.Super[s] + c)
        want = _closed_form_entry(N, lam, perm[i], perm[j])
        assert abs(out[0] - want) <= 1e-10 * abs(d[j]), (s, r, c)
    logdet = float(np.sum(np.log(lam)))
    assert abs(plan.logdet() - logdet) <= 1e-11 * abs(logdet)
    plan.close()
