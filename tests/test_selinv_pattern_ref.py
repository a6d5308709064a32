"""selinv_pattern_ref (the numpy restatement of sf_*_plan_selinv_values / _trace / _entries) over arenas produced by selinv_ref /
lu_selinv_ref, against np.linalg.inv of the permuted dense matrix; and the trace as the derivative of the log-determinant against
a finite difference of slogdet."""
import functools

import numpy as np
import pytest

import selinv_pattern_ref as spr
from util import sf, gen, dense_reference_factor, panel_entries_from_dense
from selinv_ref import selinv_ref
from lu_selinv_ref import lu_selinv_ref
from test_selinv_abi import selinv_cases
from test_lu import dense_lu_nopiv, reference_layout_from_dense
from test_lu_selinv_abi import lu_selinv_cases, dense_permuted

TOL = 1e-11         # what test_selinv_abi / test_lu_selinv_abi ask of the reference arenas themselves
EPS = np.finfo(float).eps


@functools.lru_cache(maxsize=None)
def chol_setup(k):
    name, n, Cp, Ci, Cx, perm, slot = selinv_cases()[k]
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    A, L = dense_reference_factor(sym)
    return sym, A, selinv_ref(sym, panel_entries_from_dense(sym, L))


@functools.lru_cache(maxsize=None)
def lu_setup(k):
    name, n, Cp, Ci, Cx, perm, slot, symm = lu_selinv_cases()[k]
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", symm)
    Ap = dense_permuted(sym, n, Cp, Ci, Cx, symm)
    return sym, Ap, lu_selinv_ref(sym, reference_layout_from_dense(sym, dense_lu_nopiv(Ap))), symm


def _col_of(Lp):
    return np.repeat(np.arange(len(Lp) - 1), np.diff(Lp))


def chol_dense_M(sym, V):
    M = np.zeros((sym.n, sym.n))
    j = _col_of(sym.Lp)
    M[sym.Li, j] = V
    M[j, sym.Li] = V
    return M


def lu_dense_M(sym, symm, VL, VU):
    """what set_values(VL, VU) assembles: L's entries below the diagonal, U's by row; U aliasing L: both triangles from VL"""
    M = np.zeros((sym.n, sym.n))
    j = _col_of(sym.Lp)
    if symm:
        M[sym.Li, j] = VL
        M[j, sym.Li] = VL
        return M
    off = sym.Li != j
    M[sym.Li[off], j[off]] = VL[off]
    M[_col_of(sym.Up), sym.Ui] = VU
    return M


def _close(got, want, scale):
    return np.max(np.abs(np.asarray(got) - np.asarray(want))) <= TOL * scale


@pytest.mark.parametrize("k", range(len(selinv_cases())), ids=[c[0] for c in selinv_cases()])
def test_cholesky_against_dense_inverse(k):
    sym, A, S = chol_setup(k)
    Sig = np.linalg.inv(A)
    smax = np.max(np.abs(Sig))
    j = _col_of(sym.Lp)
    assert _close(spr.chol_values(sym, S), Sig[sym.Li, j], smax)
    rng = np.random.default_rng(k)
    V = rng.uniform(-1, 1, (len(sym.Li), 3))
    terms = spr.chol_trace_terms(sym, S, V)
    for t in range(3):
        M = chol_dense_M(sym, V[:, t])
        assert abs(terms[:, t].sum() - np.trace(Sig @ M)) <= TOL * np.sum(np.abs(Sig) * np.abs(M))
    # every position of the pattern, both triangles, and the pairs that are not in it
    rr, cc = spr.pattern_pairs(sym)
    got, outside = spr.entries(sym, S, np.concatenate([rr, cc]), np.concatenate([cc, rr]))
    assert outside == 0 and _close(got, np.concatenate([Sig[rr, cc], Sig[cc, rr]]), smax)
    inpat = np.zeros((sym.n, sym.n), dtype=bool)
    inpat[rr, cc] = inpat[cc, rr] = True
    oi, oj = np.nonzero(~inpat)
    got, outside = spr.entries(sym, S, oi, oj)
    assert outside == len(oi) and np.all(np.isnan(got))


@pytest.mark.parametrize("k", range(len(lu_selinv_cases())), ids=[c[0] for c in lu_selinv_cases()])
def test_lu_against_dense_inverse(k):
    sym, Ap, S, symm = lu_setup(k)
    Sig = np.linalg.inv(Ap)
    smax = np.max(np.abs(Sig))
    j = _col_of(sym.Lp)
    SL, SU = spr.lu_values(sym, S, symm)
    TL, TU = spr.lu_values(sym, S, symm, transposed=True)
    assert _close(SL, Sig[sym.Li, j], smax) and _close(TL, Sig[j, sym.Li], smax)
    assert np.array_equal(SL[sym.Li == j], TL[sym.Li == j])         # the L diagonal positions: Sigma_jj
    if symm:
        assert SU is None and TU is None
    else:
        ju = _col_of(sym.Up)
        assert _close(SU, Sig[ju, sym.Ui], smax) and _close(TU, Sig[sym.Ui, ju], smax)
    rng = np.random.default_rng(100 + k)
    VL = rng.uniform(-1, 1, (len(sym.Li), 2))
    VU = None if symm else rng.uniform(-1, 1, (len(sym.Ui), 2))
    terms = spr.lu_trace_terms(sym, S, symm, VL, VU)
    for t in range(2):
        M = lu_dense_M(sym, symm, VL[:, t], None if symm else VU[:, t])
        assert abs(terms[:, t].sum() - np.trace(Sig @ M)) <= TOL * np.sum(np.abs(Sig.T) * np.abs(M))
    rr, cc = spr.pattern_pairs(sym)
    got, outside = spr.entries(sym, S, np.concatenate([rr, cc]), np.concatenate([cc, rr]), lu=True)
    assert outside == 0 and _close(got, np.concatenate([Sig[rr, cc], Sig[cc, rr]]), smax)
    inpat = np.zeros((sym.n, sym.n), dtype=bool)
    inpat[rr, cc] = inpat[cc, rr] = True
    oi, oj = np.nonzero(~inpat)
    got, outside = spr.entries(sym, S, oi, oj, lu=True)
    assert outside == len(oi) and np.all(np.isnan(got))


def test_live_mask_and_duplicates():
    """an entry given again later in its column is not part of the assembled matrix: its value has the Sigma of its (i, j), its
    trace term is not there"""
    Lp, Li = np.array([0, 3, 5]), np.array([1, 0, 1, 1, 1])
    assert spr.live_mask(Lp, Li).tolist() == [False, True, True, False, True]
    assert spr.live_mask(Lp, Li, skip_diag=True).tolist() == [False, False, True, False, False]


def _fd_check(f, grad, n, rho, kappa):
    """forward difference of f at 0 against grad.  |f''| <= M2 = n (rho / (1 - h rho))^2 on [0, h] for f = log|det(A + theta D)|,
    rho = |A^-1 D|_2 (f'' = -tr((A(theta)^-1 D)^2), at most n times the squared spectral norm).  slogdet is a backward-stable LU:
    it returns the determinant of A + dA with |dA| <= n eps |A|, which moves log|det| by at most |tr(A^-1 dA)| <= ef = n^2 eps kappa.
    (f(h) - f(0)) / h - f'(0) is then at most h M2 / 2 + 2 ef / h, smallest at h = 2 sqrt(ef / M2)."""
    ef = n * n * EPS * kappa
    h = 2.0 * np.sqrt(ef / (n * rho * rho))
    assert h * rho < 0.5
    M2 = n * (rho / (1.0 - h * rho)) ** 2
    tol = h * M2 / 2.0 + 2.0 * ef / h
    fd = (f(h) - f(0.0)) / h
    print("h", h, "tol", tol, "fd", fd, "grad", grad, "diff", abs(fd - grad))
    assert tol < 1e-3 * max(abs(grad), 1.0)           # (the check can tell a missing factor 2 or a dropped entry)
    assert abs(fd - grad) <= tol


def test_logdet_grad_finite_difference_spd():
    k = [c[0] for c in selinv_cases()].index("lap3d_4_nd")
    sym, A, S = chol_setup(k)
    dA = np.random.default_rng(1).uniform(-1, 1, len(sym.Li))
    D = chol_dense_M(sym, dA)
    grad = float(spr.chol_trace_terms(sym, S, dA).sum())
    rho = np.linalg.norm(np.linalg.solve(A, D), 2)
    _fd_check(lambda th: np.linalg.slogdet(A + th * D)[1], grad, sym.n, rho, np.linalg.cond(A))


def test_logdet_grad_finite_difference_unsymmetric():
    k = [c[0] for c in lu_selinv_cases()].index("st3d_5_nd")
    sym, Ap, S, symm = lu_setup(k)
    assert not symm
    rng = np.random.default_rng(2)
    dL, dU = rng.uniform(-1, 1, len(sym.Li)), rng.uniform(-1, 1, len(sym.Ui))
    D = lu_dense_M(sym, False, dL, dU)
    grad = float(spr.lu_trace_terms(sym, S, False, dL, dU).sum())
    rho = np.linalg.norm(np.linalg.solve(Ap, D), 2)
    _fd_check(lambda th: np.linalg.slogdet(Ap + th * D)[1], grad, sym.n, rho, np.linalg.cond(Ap))
