"""sf_lu_plan_selinv / _get_selinv_range / _selinv_diag / _logdet (LUPlan.selinv, get_selinv, selinv_diag, logdet): the selected
inverse of a resident no-pivot LU factor against dense inverses and against solve_many columns on a matrix with a supernode of
more than one 512-column unit that has rows below it; the state rules; the sign of the determinant under row interchanges."""
import ctypes as C

import numpy as np
import pytest

from util import sf, gen, nd_perm_py, rel_err
from lu_selinv_ref import flops as ref_flops, UW
from test_lu import reference_layout_from_dense
from test_lu_selinv_abi import lu_selinv_cases, dense_permuted

pytestmark = pytest.mark.gpu

SF_ERR_ARG = 1


def _plan(sym, symm=False):
    plan = sf.LUPlan(sym, device=0)
    plan.set_values(sym.Lx, None if symm else sym.Ux)
    plan.factorize()
    return plan


def packed_diag(sym, S):
    """the diagonal entries of Sigma in the packed layout: panel s, column c, row c"""
    cols = np.arange(sym.n)
    s = sym.SuperMap[cols]
    lda = 2 * np.diff(sym.Lsip)[s] - np.diff(sym.Super)[s]
    return S[sym.Lsxp[s] + (cols - sym.Super[s]) * (lda + 1)]


def permutation_sign(p):
    p = np.asarray(p)
    seen = np.zeros(len(p), dtype=bool)
    cycles = 0
    for j in range(len(p)):
        if not seen[j]:
            cycles += 1
            k = j
            while not seen[k]:
                seen[k] = True
                k = p[k]
    return -1 if (len(p) - cycles) % 2 else 1


@pytest.mark.parametrize("case", lu_selinv_cases(), ids=lambda c: c[0])
def test_dense_reference(case):
    name, n, Cp, Ci, Cx, perm, slot, symm = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", symm)
    plan = _plan(sym, symm)
    assert plan.stat("selinv_valid") == 0
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    assert plan.stat("flops_selinv") == pytest.approx(ref_flops(sym), rel=1e-12)
    Ap = dense_permuted(sym, n, Cp, Ci, Cx, symm)
    S = plan.get_selinv()
    err = rel_err(S, reference_layout_from_dense(sym, np.linalg.inv(Ap)))
    print(name, "rel_err", err)
    assert err <= 1e-11, name
    assert np.array_equal(plan.selinv_diag(), packed_diag(sym, S))
    want_sign, want_ld = np.linalg.slogdet(Ap)
    ld, sign = plan.logdet()
    print(name, "logdet", ld, want_ld, sign, want_sign)
    assert sign == want_sign and abs(ld - want_ld) <= 1e-11 * max(1.0, abs(want_ld))
    plan.close()


def test_wide_supernode_with_rows_below_against_solve_many():
    dims = (38, 19, 19)         # the smallest 2:1:1 grid whose analysis has a supernode of more than 512 columns with rows below it
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(*dims, extra_per_row=0, seed=3)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(*dims), 1 << 30, "lu", False)
    ncol, nsrow = np.diff(sym.Super), np.diff(sym.Lsip)
    assert np.any((ncol > UW) & (nsrow > ncol))
    plan = _plan(sym)
    plan.selinv()
    S = plan.get_selinv()
    cols = []
    for s in np.argsort(-ncol)[:4]:                    # the widest supernodes: first, last and unit-boundary columns
        c0, c1 = sym.Super[s], sym.Super[s + 1]
        cols += [c0, c1 - 1] + [c0 + k for k in range(UW, c1 - c0, UW)] + [c0 + k - 1 for k in range(UW, c1 - c0, UW)]
    below = np.nonzero(ncol < nsrow)[0]
    parents = sym.SuperMap[sym.Lsi[sym.Lsip[below] + ncol[below]]]
    leaves = np.setdiff1d(np.arange(sym.nsuper), parents)
    rng = np.random.default_rng(4)
    cols += [int(sym.Super[s]) for s in rng.choice(leaves, 48 - len(cols), replace=False)]
    cols = np.array(sorted(set(int(c) for c in cols)))
    assert len(cols) <= 48
    E = np.zeros((n, len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    X = plan.solve_many(E)                               # X[:, k] = column cols[k] of A^-1
    colmax = np.max(np.abs(X), axis=0)
    kof = np.full(n, -1)
    kof[cols] = np.arange(len(cols))
    n_rc, n_cr, worst = 0, 0, 0.0
    for s in range(sym.nsuper):
        nc, nr = int(ncol[s]), int(nsrow[s])
        lda = 2 * nr - nc
        rows = sym.Lsi[sym.Lsip[s]:sym.Lsip[s + 1]]
        P = S[sym.Lsxp[s]:sym.Lsxp[s + 1]].reshape(nc, lda)           # [column][packed row]
        for c in np.nonzero(kof[sym.Super[s]:sym.Super[s + 1]] >= 0)[0]:      # Sigma(rows, j): diagonal block and Sigma(R,C)
            k = kof[sym.Super[s] + c]
            d = np.max(np.abs(P[c, :nr] - X[rows, k])) / colmax[k]
            worst = max(worst, d)
            assert d <= 1e-11, (s, c)
            n_rc += nr > nc
        for x in np.nonzero(kof[rows[nc:]] >= 0)[0]:                          # Sigma(C, g)^T for the rows g below that are in T
            k = kof[rows[nc + x]]
            d = np.max(np.abs(P[:, nr + x] - X[sym.Super[s]:sym.Super[s + 1], k])) / colmax[k]
            worst = max(worst, d)
            assert d <= 1e-11, (s, x)
            n_cr += 1
    print("compared", n_rc, n_cr, "worst", worst)
    assert n_rc > 1 and n_cr > 1
    assert np.array_equal(plan.selinv_diag(), packed_diag(sym, S))
    plan.close()


def test_state():
    N = 12
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=6)
    sym = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", False)
    plan = _plan(sym)
    F0 = plan.get_factor().copy()
    ld0, sign0 = plan.logdet()
    plan.selinv()
    S1 = plan.get_selinv().copy()
    assert np.array_equal(plan.get_factor(), F0)
    plan.selinv()
    assert np.array_equal(plan.get_selinv(), S1)
    plan.set_values(4.0 * sym.Lx, 4.0 * sym.Ux)
    assert plan.stat("selinv_valid") == 0
    for call in (plan.get_selinv, plan.selinv_diag, plan.selinv, plan.logdet):
        with pytest.raises(sf.SparseFrameError):
            call()
    plan.factorize()
    assert plan.stat("selinv_valid") == 0
    with pytest.raises(sf.SparseFrameError):
        plan.selinv_diag()
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    assert rel_err(plan.get_selinv(), S1 / 4.0) <= 1e-14
    ld1, sign1 = plan.logdet()
    assert sign1 == sign0 and abs(ld1 - (ld0 + n * np.log(4.0))) <= 1e-11 * abs(ld1)
    plan.close()


def test_pivoting():
    N = 12
    n, Cp, Ci, Cx0 = gen.unsymmetric_stencil(N, N, N, seed=9)
    perm = nd_perm_py(N, N, N)
    parities = []
    for seed in range(6):
        _, _, _, Cx = gen.weaken_diagonal(n, Cp, Ci, Cx0, seed=70 + seed)
        sym = sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)
        plan = sf.LUPlan(sym)
        plan.set_values(sym.Lx, sym.Ux)
        plan.set_pivoting(tol=1.0)
        plan.factorize()
        with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
            plan.selinv()
        piv = plan.get_pivots()
        parities.append((permutation_sign(piv), bool(np.any(piv != np.arange(n)))))
        want_sign, want_ld = np.linalg.slogdet(dense_permuted(sym, n, Cp, Ci, Cx, False))
        ld, sign = plan.logdet()
        print("seed", seed, "parity", parities[-1], "logdet", ld, want_ld, sign, want_sign)
        assert sign == want_sign and abs(ld - want_ld) <= 1e-11 * max(1.0, abs(want_ld))
        plan.close()
    assert any(sg < 0 for sg, moved in parities)
    assert any(sg > 0 and moved for sg, moved in parities)
    # no threshold, perturbation only: accepted
    sym = sf.analyze(n, Cp, Ci, Cx0, perm, 1 << 30, "lu", False)
    plan = sf.LUPlan(sym)
    plan.set_values(sym.Lx, sym.Ux)
    plan.set_pivoting(tol=0.0, perturb=1e-8)
    plan.factorize()
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    plan.close()


def test_cholesky_plan_refused():
    N = 6
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    plan = sf.CholPlan(sym, device=0)
    plan.set_values(sym.Lx)
    plan.factorize()
    out = np.zeros(1)
    sign = C.c_int(0)
    assert sf.lib.sf_lu_plan_selinv(plan._h) == SF_ERR_ARG
    assert sf.lib.sf_lu_plan_logdet(plan._h, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sign)) == SF_ERR_ARG
    plan.close()
