"""sf_chol_plan_rowdel / _rowadd (CholPlan.rowdel, rowadd): row and column j of the resident factor become the identity's, or
take new values, in place (csrc/sf_rowmod.hip).  The factor is read back with get_factor and checked against the plan's
own refactorization of the target matrix (existing code, not the code under test) and against tests/rowmod_ref.py.

Backward error |L'L'^T - A'|_F / |A'|_F (longdouble) of a modified factor is held to 8 x that of the refactorization, the margin
of tests/test_updown.py.  Measured ratios are printed as ROWMOD_RATIO lines and recorded in DESIGN 8q.  The cases are those of
tests/test_rowmod_ref.py (arrow_900_200 is dropped there, where the emulation alone misses the margin: rowadd of a row behind a
long sweep; tools/rowmod_accuracy.py measures that case on the device)."""
import ctypes as C
import functools

import numpy as np
import pytest

import kernel_ref as kr
import rowmod_ref as rr
import updown_ref as ur
from test_rowmod_ref import CASES, MARGIN, NAMES
from util import sf

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def setup(name):
    _, n, Cp, Ci, Cx, perm, slot = CASES[NAMES.index(name)]
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    perm = np.arange(n) if perm is None else np.asarray(perm)
    return sym, ur.Structure(sym), ur.dense_matrix(sym), perm


def values_of(sym, A):
    """Lx of A on the plan's pattern; deleted(A, j) keeps that pattern (explicit zeros in row and column j)"""
    return ur.values_of(sym, A)


def fresh(sym, A=None):
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx if A is None else values_of(sym, A))
    plan.factorize()
    return plan


@functools.lru_cache(maxsize=None)
def factor_of(name, j=None):
    """(factor, backward error) of the plan's own factorization of A (j None) or of A with row j deleted"""
    sym, st, A, _ = setup(name)
    A1 = A if j is None else rr.deleted(A, j)
    plan = fresh(sym, A1)
    L = plan.get_factor().copy()
    ld = plan.logdet()
    plan.close()
    e = ur.backward_error(st, L, A1)
    return L, (e if e > 0 else kr.U * st.n), ld


def report(what, ratio):
    print(f"ROWMOD_RATIO {what}: backward error / refactorization's = {ratio:.3g}")
    return ratio


touched_mask = rr.write_set


def schur(A, j):
    """the Schur complement of variable j against ALL the others, a_jj - a_j^T A_oo^-1 a_j = 1 / (A^-1)_jj = det A / det A', from
    numpy on the dense matrix (for the last row this is a22 - a12^T A11^-1 a12 with the leading block; for an earlier one the
    trailing variables take part too, which is why L33 changes)"""
    o = np.arange(A.shape[0]) != j
    return A[j, j] - A[j, o] @ np.linalg.solve(A[np.ix_(o, o)], A[o, j])


def cases_and_rows():
    out = []
    for name in NAMES:
        sym, st, _, _ = setup(name)
        out += [(name, j) for j in rr.rows_to_try(st, NAMES.index(name))]
    out += [("dense_70", 0), ("dense_70", 69)]                  # check 9: no sweep / no update
    return sorted(set(out), key=lambda c: (NAMES.index(c[0]), c[1]))


ROWS = cases_and_rows()


@pytest.mark.parametrize("name,j", ROWS)
def test_rowdel_against_refactorization(name, j):
    sym, st, A, perm = setup(name)
    A1 = rr.deleted(A, j)
    plan = fresh(sym)
    L0 = plan.get_factor().copy()
    ld0 = plan.logdet()
    what = plan.rowmod_path(j)
    assert what == rr.lists(st, j)
    plan.set_values(values_of(sym, A1))
    plan.rowdel(j)
    L1 = plan.get_factor().copy()
    assert plan.stat("selinv_valid") == 0 and plan.stat("update_path_supernodes") == len(what["update"])
    assert plan.stat("rowmod_row_tasks") == len(what["rows"]) + (1 if rr.locate(st, j)[1] else 0)
    assert plan.stat("rowmod_sweep_supernodes") == 0
    # every launch of the call against the rotations' alone: the column, and the row tasks' launch where there are any
    assert plan.stat("rowmod_launches") == plan.stat("update_launches") + (2 if plan.stat("rowmod_row_tasks") else 1)
    off = ~touched_mask(st, j, what)
    assert np.array_equal(kr.bits(L1)[off], kr.bits(L0)[off])
    _, e_ref, _ = factor_of(name, j)
    assert report(f"{name} j={j} rowdel", ur.backward_error(st, L1, A1) / e_ref) <= MARGIN
    emu, _ = rr.rowdel_emulate(st, L0, j)
    low = st.lower_mask()
    assert np.max(np.abs(emu - L1)[low]) <= 8.0 * sym.n * kr.U * np.max(np.abs(L1[low]))
    want = ld0 - np.log(schur(A, j))
    assert abs(plan.logdet() - want) <= 1e-11 * max(1.0, abs(want))
    e = np.zeros(sym.n)
    e[j] = 1.0
    assert plan.solve(e)[j] == 1.0
    plan.close()


@pytest.mark.parametrize("name,j", ROWS)
def test_rowadd_against_refactorization(name, j):
    sym, st, A, perm = setup(name)
    A1 = rr.deleted(A, j)
    plan = fresh(sym, A1)
    L0 = plan.get_factor().copy()
    ld0 = plan.logdet()
    idx, vals = rr.column_of(st, A, j)
    what = plan.rowmod_path(j, idx)
    assert what == rr.lists(st, j, idx)
    plan.set_values(sym.Lx)
    plan.rowadd(j, idx, vals)
    L1 = plan.get_factor().copy()
    assert plan.stat("selinv_valid") == 0 and plan.stat("rowmod_not_deleted") == 0
    assert plan.stat("rowmod_sweep_supernodes") == len(what["sweep"]) and plan.stat("update_path_supernodes") == len(what["update"])
    off = ~touched_mask(st, j, what)
    assert np.array_equal(kr.bits(L1)[off], kr.bits(L0)[off])
    _, e_ref, _ = factor_of(name)
    assert report(f"{name} j={j} rowadd", ur.backward_error(st, L1, A) / e_ref) <= MARGIN
    emu, failed, _ = rr.rowadd_emulate(st, L0, j, idx, vals)
    low = st.lower_mask()
    assert not failed and np.max(np.abs(emu - L1)[low]) <= 8.0 * sym.n * 2 * kr.U * np.max(np.abs(L1[low]))
    want = ld0 + np.log(schur(A, j))
    assert abs(plan.logdet() - want) <= 1e-11 * max(1.0, abs(want))
    b = np.random.default_rng(1).uniform(-1, 1, sym.n)
    ref = fresh(sym)
    xs = ref.solve(b)
    ref.close()
    assert np.max(np.abs(plan.solve(b) - xs)) <= 1e-12 * np.max(np.abs(xs))
    plan.close()


@pytest.mark.parametrize("name,j", ROWS)
def test_rowdel_then_rowadd_returns_the_factor(name, j):
    """check 3, with the bound of test_updown's round trip: the backward error against A within the margin of the factorization's"""
    sym, st, A, perm = setup(name)
    plan = fresh(sym)
    idx, vals = rr.column_of(st, A, j)
    plan.rowdel(j)
    plan.rowadd(j, idx, vals)
    L2 = plan.get_factor().copy()
    plan.close()
    L0, e0, _ = factor_of(name)
    assert report(f"{name} j={j} del-add", ur.backward_error(st, L2, A) / e0) <= MARGIN
    low = st.lower_mask()
    assert np.max(np.abs(L2 - L0)[low]) <= 4 * 8.0 * sym.n * 2 * kr.U * np.max(np.abs(L0[low]))


@pytest.mark.parametrize("name", ["lap3d_8_nd", "lap2d_30x17_nd"])
def test_perm_in_gives_the_same_bits(name):
    sym, st, A, perm = setup(name)
    j = rr.rows_to_try(st, 3)[-1]
    idx, vals = rr.column_of(st, A, j)
    facs = []
    for how in ("plan", "perm_in"):
        plan = fresh(sym)
        plan.set_ordering(perm)
        if how == "plan":
            plan.rowdel(j)
            facs.append(plan.get_factor().copy())
            plan.rowadd(j, idx[::-1], vals[::-1])
        else:
            assert plan.rowmod_path(int(perm[j]), perm[idx], perm_in=True) == plan.rowmod_path(j, idx)
            plan.rowdel(int(perm[j]), perm_in=True)                 # caller's numbering: row perm[i] is row i of the plan
            facs.append(plan.get_factor().copy())
            plan.rowadd(int(perm[j]), perm[idx], vals, perm_in=True)
        facs.append(plan.get_factor().copy())
        plan.close()
    assert np.array_equal(kr.bits(facs[0]), kr.bits(facs[2])) and np.array_equal(kr.bits(facs[1]), kr.bits(facs[3]))


@pytest.mark.parametrize("name", ["lap3d_8_nd", "band_dense_1000_150"])
def test_two_rows_in_either_order(name):
    sym, st, A, perm = setup(name)
    j1, j2 = sorted(rr.rows_to_try(st, 5)[-2:])
    if j1 == j2:
        j2 = j1 + 1
    b = np.random.default_rng(2).uniform(-1, 1, sym.n)
    xs = []
    for order in ([j1, j2], [j2, j1]):
        plan = fresh(sym)
        plan.rowdel(order)
        xs.append(plan.solve(b))
        plan.close()
    A2 = rr.deleted(rr.deleted(A, j1), j2)
    want = np.linalg.solve(A2, b)
    assert np.max(np.abs(xs[0] - xs[1])) <= 1e-12 * np.max(np.abs(xs[0]))
    assert np.max(np.abs(xs[0] - want)) <= 1e-10 * np.max(np.abs(want))


@pytest.mark.parametrize("name", ["lap3d_8_nd", "dense_70", "blockdiag_dense"])
def test_indefinite_rowadd(name):
    sym, st, A, perm = setup(name)
    j = sym.n // 2
    plan = fresh(sym)
    plan.rowdel(j)
    idx, vals = rr.column_of(st, A, j)
    small = vals.copy()
    small[idx == j] = A[j, j] - 2.0 / np.linalg.inv(A)[j, j]          # d = -(the Schur complement)
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_NOT_POSDEF"):
        plan.rowadd(j, idx, small)
    b = np.ones(sym.n)
    for call in (lambda: plan.solve(b), plan.logdet, plan.selinv, lambda: plan.rowdel(j), lambda: plan.rowadd(j, idx, vals)):
        with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
            call()
    plan.factorize()
    x = plan.solve(b)
    assert np.max(np.abs(A @ x - b)) <= 1e-10 * np.max(np.abs(x)) * np.max(np.abs(A))
    plan.rowdel(j)
    plan.rowadd(j, idx, vals)
    plan.close()


def test_refusals_leave_the_factor_alone():
    sym, st, A, perm = setup("lap3d_8_nd")
    plan = fresh(sym)
    L0 = plan.get_factor().copy()
    n = sym.n
    j = rr.rows_to_try(st, 0)[1]
    idx, vals = rr.column_of(st, A, j)
    lib = sf.lib
    lp, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))

    def add(row, Ai, Ax, flags=0):
        Ai, Ax = np.ascontiguousarray(Ai, dtype=np.int64), np.ascontiguousarray(Ax, dtype=np.float64)
        return lib.sf_chol_plan_rowadd(plan._h, row, len(Ai), lp(Ai), dp(Ax), flags)

    assert lib.sf_chol_plan_rowdel(plan._h, -1, 0) == 1 and lib.sf_chol_plan_rowdel(plan._h, n, 0) == 1
    assert lib.sf_chol_plan_rowdel(plan._h, j, 2) == 1 and lib.sf_chol_plan_rowdel(plan._h, j, 1) == 1      # flag; no ordering
    assert add(-1, idx, vals) == 1 and add(n, idx, vals) == 1                   # a row outside [0, n)
    assert add(j, np.append(idx, idx[0]), np.append(vals, 1.0)) == 1            # an index twice
    assert add(j, idx[idx != j], vals[idx != j]) == 1                           # a missing diagonal
    assert add(j, [], []) == 1
    assert add(j, idx, vals, flags=2) == 1 and add(j, idx, vals, flags=1) == 1
    outside = next(i for i in range(n) if not rr.admissible_index(st, j, i))
    assert add(j, np.append(idx, outside), np.append(vals, 1.0)) == 1 and plan.stat("rowmod_bad_index") == len(idx)
    assert plan.stat("bytes_update") == 0                                       # nothing was allocated for any of these
    assert add(j, idx, vals) == 1 and plan.stat("rowmod_not_deleted") == 1      # the row is not the identity's
    assert plan.stat("rowmod_bad_index") == -1                                  # (every call starts the two stats afresh)
    assert plan.stat("bytes_update") >= n * 16 * 8                              # (the check works in the update's block)
    assert np.array_equal(kr.bits(plan.get_factor()), kr.bits(L0))
    # ... and a row that is deleted but whose column is not: the other half of the check
    plan.rowdel(j)
    assert plan.stat("rowmod_not_deleted") == 0
    L1 = plan.get_factor().copy()
    j2 = int(st.rows(rr.locate(st, j)[0])[-1])
    if j2 != j:
        i2, v2 = rr.column_of(st, A, j2)
        assert add(j2, i2, v2) == 1 and plan.stat("rowmod_not_deleted") == 1
    assert np.array_equal(kr.bits(plan.get_factor()), kr.bits(L1))
    assert add(j, idx, vals) == 0 and plan.stat("rowmod_not_deleted") == 0 and plan.stat("rowmod_bad_index") == -1
    plan.close()
    # no successful factorization: refused
    p2 = sf.CholPlan(sym)
    p2.set_values(sym.Lx)
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
        p2.rowdel(0)
    p2.close()
    # a sharded and a mapped plan: refused, and what they hold stays bit for bit
    owner, _, _ = sf.subtree_partition(sym, 2)
    for make in (lambda: sf.CholPlan(sym, phase=sf.phases_for_rank(owner, 0), load_top=True),
                 lambda: sf.CholPlan(sym, owner=owner, rank=0, nranks=2)):
        p3 = make()
        p3.set_values(sym.Lx)
        p3.factorize_phase(0)
        before = p3.get_factor().copy()
        with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
            p3.rowdel(0)
        with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
            p3.rowadd(0, [0], [1.0])
        assert np.array_equal(kr.bits(p3.get_factor()), kr.bits(before)) and p3.stat("bytes_update") == 0
        p3.close()


def test_selinv_recomputes_after_rowdel():
    sym, st, A, perm = setup("lap3d_4_nd")
    j = sym.n // 3
    plan = fresh(sym)
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    A1 = rr.deleted(A, j)
    plan.set_values(values_of(sym, A1))
    plan.rowdel(j)
    assert plan.stat("selinv_valid") == 0
    with pytest.raises(sf.SparseFrameError):
        plan.selinv_diag()
    plan.selinv()
    want = np.diag(np.linalg.inv(A1))
    assert np.max(np.abs(plan.selinv_diag() - want)) <= 1e-11 * np.max(np.abs(want))
    plan.sync()                                                 # must not hand the plan back to its last factorization
    want = np.linalg.slogdet(A1)[1]
    assert abs(plan.logdet() - want) <= 1e-11 * max(1.0, abs(want))
    plan.close()


def test_dense_70_ends_have_nothing_to_sweep_or_update():
    sym, st, A, perm = setup("dense_70")
    plan = fresh(sym)
    assert plan.rowmod_path(0, rr.column_of(st, A, 0)[0])["sweep"] == [] and plan.rowmod_path(0)["rows"] == []
    assert plan.rowmod_path(sym.n - 1)["update"] == []
    plan.rowdel(sym.n - 1)
    assert plan.stat("rowmod_launches") == 2 and plan.stat("update_launches") == 0      # the row, the column; no rotation
    plan.close()
