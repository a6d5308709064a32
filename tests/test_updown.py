"""sf_chol_plan_update / _update_device (CholPlan.update, update_device): the resident factor of A becomes that of A +- W W^T in place
(csrc/sf_updown.hip).  The factor is read back with get_factor and checked against the plan's own refactorization of A'
(existing code, not the code under test) and against tests/updown_ref.py.  Diagonal bumps and vectors on existing edges of A run on
the plan of the case's own analysis (its ordering, its relaxed supernodes, fill outside A's pattern); only whole-column cliques, whose
products need places on the fill, run on a plan made for the pattern of L (setup).

Backward error |L'L'^T - A'|_F / |A'|_F (longdouble) of an updated factor is held to 8 x that of the refactorization of A': an
updated entry passes through up to k extra rotations per preceding path column on top of the factorization's own rounding, which
enters as its square root at these sizes.  Measured worst ratios are printed as UPDOWN_RATIO lines and recorded in DESIGN 8o."""
import functools

import numpy as np
import pytest

import kernel_ref as kr
import updown_ref as ur
from util import sf, small_cases, wide_cases

pytestmark = pytest.mark.gpu

WANT = ("blockdiag_dense", "band_dense_1000_150", "arrow_900_200", "lap3d_8_nd", "lap2d_30x17_nd", "blockdiag", "dense_70", "diagonal_5",
        "lap3d_4_nd")
CASES = [c for c in small_cases() + wide_cases() if c[0] in WANT]
NAMES = [c[0] for c in CASES]
MARGIN = 8.0


@functools.lru_cache(maxsize=None)
def setup(name, full=False):
    """(sym, structure, dense permuted A, the case's ordering).  full=False: the plan of the case's own analysis -- its ordering, its
    relaxed supernodes, A's own pattern with the fill outside it: diagonal bumps and vectors on existing edges of A keep A' inside
    that pattern, so set_values + factorize of the same plan is the reference.  full=True, for the clique columns only: the plan is
    made for the permuted matrix with the whole pattern of L as its own (explicit zeros on the fill), so that A +- W W^T has a
    place for every entry a whole column of L adds; this analysis amalgamates more (fewer, wider supernodes)."""
    _, n, Cp, Ci, Cx, perm, slot = CASES[NAMES.index(name)]
    sym0 = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    A = ur.dense_matrix(sym0)
    perm = np.arange(n) if perm is None else np.asarray(perm)
    if not full:
        return sym0, ur.Structure(sym0), A, perm
    st0 = ur.Structure(sym0)
    rows, cols = np.nonzero(st0.dense(np.ones(sym0.xsize)))
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    Lp = np.zeros(n + 1, dtype=np.int64)
    np.add.at(Lp, cols + 1, 1)
    sym = sf.analyze(n, np.cumsum(Lp), rows.astype(np.int64), A[rows, cols], None, slot)
    return sym, ur.Structure(sym), A, np.arange(n)


def fresh(sym, A=None):
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx if A is None else ur.values_of(sym, A))
    plan.factorize()
    return plan


def make_w(sym, st, k, kind, seed):
    """k admissible columns.  bump: diagonal entries; edge: alpha (e_i - e_j) on existing edges; clique: a whole column of the
    pattern (every product w_i w_j then has a place in the plan's values).  The columns start in leaves (the first ones), in root
    supernodes (the last one) and anywhere between"""
    n, Lp, Li = sym.n, np.asarray(sym.Lp), np.asarray(sym.Li)
    rng = np.random.default_rng(seed)
    roots = [s for s in range(st.nsuper) if st.parent(s) < 0]
    starts = [0, roots[-1]] + [int(s) for s in rng.integers(st.nsuper, size=max(k - 2, 0))]
    W = np.zeros((n, k))
    for t in range(k):
        s = starts[t % len(starts)] if t < len(starts) else starts[t]
        j = int(st.Super[s]) + int(rng.integers(st.nscol(s)))
        r = np.sort(Li[Lp[j]:Lp[j + 1]])
        assert r[0] == j and st.admissible(r)
        if kind == "bump" or len(r) == 1:
            W[r[0], t] = rng.uniform(0.5, 1.5)
        elif kind == "edge":
            W[[r[0], r[int(rng.integers(1, len(r)))]], t] = np.array([1.0, -1.0]) * rng.uniform(0.5, 1.5)
        else:
            W[r, t] = rng.uniform(-1.0, 1.0, len(r))
    return W


def report(name, ratio):
    print(f"UPDOWN_RATIO {name}: backward error / refactorization's = {ratio:.3g}")
    return ratio


def reference_error(sym, st, A1):
    """backward error of the plan's own refactorization of A' (u n when that is exactly 0), and that factor"""
    ref = fresh(sym, A1)
    Lr = ref.get_factor().copy()
    ref.close()
    e = ur.backward_error(st, Lr, A1)
    return (e if e > 0 else kr.U * st.n), Lr


def check_untouched(st, before, after, path):
    off = ~st.panel_mask(path) | ~st.lower_mask()
    assert np.array_equal(kr.bits(after)[off], kr.bits(before)[off])


@pytest.mark.parametrize("name", [n for n in NAMES if n != "lap3d_4_nd"])
@pytest.mark.parametrize("k,kind", [(1, "bump"), (2, "edge"), (16, "clique"), (17, "edge")])
def test_update_against_refactorization(name, k, kind):
    sym, st, A, perm = setup(name, kind == "clique")
    W = make_w(sym, st, k, kind, 100 * NAMES.index(name) + k)
    plan = fresh(sym)
    L0 = plan.get_factor().copy()
    ld0 = plan.logdet()
    G = np.atleast_2d(plan.gram(W))
    path = plan.update_path(W)
    assert path.tolist() == st.path([np.flatnonzero(W[:, t]) for t in range(k)])
    A1 = A + W @ W.T
    plan.set_values(ur.values_of(sym, A1))
    plan.update(W)
    L1 = plan.get_factor().copy()
    assert plan.stat("update_path_supernodes") == len(path) and plan.stat("bytes_update") >= sym.n * 16 * 8
    assert plan.stat("update_path_columns") == sum(st.nscol(s) for s in path) and plan.stat("selinv_valid") == 0
    check_untouched(st, L0, L1, path)                                                        # check 1
    e_ref, Lr = reference_error(sym, st, A1)
    ratio = report(f"{name} k={k} {kind}", ur.backward_error(st, L1, A1) / e_ref)            # check 2
    assert ratio <= MARGIN
    want = ld0 + np.linalg.slogdet(np.eye(k) + G)[1]                                         # check 3
    assert abs(plan.logdet() - want) <= 1e-11 * max(1.0, abs(want))
    # the emulation agrees: every entry went through at most n k rotations of a few roundings each
    emu, failed, _ = ur.update_emulate(st, L0, W, +1)
    assert not failed
    low = st.lower_mask()
    assert np.max(np.abs(emu - L1)[low]) <= 8.0 * sym.n * k * kr.U * np.max(np.abs(L1[low]))
    # check 4: refine and solve with the updated factor against the refactorized plan
    b = np.random.default_rng(1).uniform(-1, 1, sym.n)
    x, info = plan.refine(b, max_iter=2, return_info=True)
    ref = fresh(sym, A1)
    xr, info_r = ref.refine(b, max_iter=2, return_info=True)
    assert info["berr0"] <= MARGIN * max(info_r["berr0"], kr.U)
    xs = ref.solve(b)
    assert np.max(np.abs(plan.solve(b) - xs)) <= 1e-12 * np.max(np.abs(xs))
    ref.close()
    plan.close()


@pytest.mark.parametrize("name", [n for n in NAMES if n != "lap3d_4_nd"])
@pytest.mark.parametrize("k,kind", [(1, "bump"), (4, "edge"), (16, "edge"), (17, "clique")])
def test_update_then_downdate_returns_the_factor(name, k, kind):
    """check 5, with its precondition max_t |L^-1 w_t|^2 <= 1/2 (L the factor of A) taken from quadform before the calls"""
    sym, st, A, perm = setup(name, kind == "clique")
    plan = fresh(sym)
    L0 = plan.get_factor().copy()
    e0 = ur.backward_error(st, L0, A)
    e0 = e0 if e0 > 0 else kr.U * st.n
    W = make_w(sym, st, k, kind, 7 + k)
    W = W * min(1.0, np.sqrt(0.5 / np.max(np.atleast_1d(plan.quadform(W)))) * 0.999)
    assert np.max(np.atleast_1d(plan.quadform(W))) <= 0.5
    path = plan.update_path(W)
    plan.update(W)
    L1 = plan.get_factor().copy()
    plan.update(W, downdate=True)
    L2 = plan.get_factor().copy()
    check_untouched(st, L1, L2, path)
    assert report(f"{name} k={k} {kind} up-down", ur.backward_error(st, L2, A) / e0) <= MARGIN
    # a downdate on its own: sum_t |L^-1 w_t|^2 <= 1/2 bounds the largest eigenvalue of W^T A^-1 W, so A - W W^T is definite
    W = W * np.sqrt(0.5 / max(np.sum(np.atleast_1d(plan.quadform(W))), 0.5)) * 0.999
    A1 = A - W @ W.T
    plan.update(W, downdate=True)
    e_ref, _ = reference_error(sym, st, A1)
    assert report(f"{name} k={k} {kind} down", ur.backward_error(st, plan.get_factor(), A1) / e_ref) <= MARGIN
    plan.close()


@pytest.mark.parametrize("name", ["lap3d_8_nd", "lap2d_30x17_nd"])
def test_perm_in_and_device_entry_point(name):
    import torch
    sym, st, A, perm = setup(name)
    W = make_w(sym, st, 5, "edge", 3)
    Wp = np.concatenate([[0], np.cumsum([np.count_nonzero(W[:, t]) for t in range(5)])])
    Wi = np.concatenate([np.flatnonzero(W[:, t])[::-1] for t in range(5)])          # rows in descending order
    Wx = np.concatenate([W[np.flatnonzero(W[:, t])[::-1], t] for t in range(5)])
    facs = []
    for how in ("dense", "triple", "perm_in", "device", "device_perm_in"):
        plan = fresh(sym)
        plan.set_ordering(perm)
        if how == "dense":
            plan.update(W)
        elif how == "triple":
            plan.update((Wp, Wi, Wx))
        elif how == "perm_in":
            plan.update((Wp, perm[Wi], Wx), perm_in=True)       # caller's numbering: row perm[i] is row i of the plan
            assert plan.update_path((Wp, perm[Wi], None), perm_in=True).tolist() == plan.update_path(W).tolist()
        else:
            d = torch.tensor(Wx, dtype=torch.float64, device="cuda:0")
            plan.update_device(Wp, perm[Wi] if how.endswith("perm_in") else Wi, d, perm_in=how.endswith("perm_in"))
        facs.append(plan.get_factor().copy())
        plan.close()
    for f in facs[1:]:
        assert np.array_equal(kr.bits(f), kr.bits(facs[0]))


@pytest.mark.parametrize("name", ["lap3d_8_nd", "dense_70", "blockdiag_dense"])
def test_indefinite_downdate(name):
    sym, st, A, perm = setup(name)
    plan = fresh(sym)
    j = sym.n // 2
    W = np.zeros(sym.n)
    W[j] = 2.0 * np.sqrt(A[j, j])
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_NOT_POSDEF"):
        plan.update(W, downdate=True)
    b = np.ones(sym.n)
    for call in (lambda: plan.solve(b), lambda: plan.solve_many(np.ones((sym.n, 2))), plan.logdet, lambda: plan.solve_half(b),
                 lambda: plan.refine(b), plan.selinv, lambda: plan.update(W), lambda: plan.sample(1)):
        with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
            call()
    plan.factorize()
    x = plan.solve(b)
    assert np.max(np.abs(A @ x - b)) <= 1e-10 * np.max(np.abs(x)) * np.max(np.abs(A))
    plan.update(0.25 * W)
    plan.close()


def test_refusals_leave_the_factor_alone():
    sym, st, A, perm = setup("lap3d_8_nd")
    plan = fresh(sym)
    L0 = plan.get_factor().copy()
    n = sym.n
    s0 = next(s for s in range(st.nsuper) if st.parent(s) >= 0)
    outside = int(np.setdiff1d(np.arange(st.Super[s0 + 1], n), st.rows(s0))[0])
    good = (np.array([0, 1]), np.array([0]), np.array([1.0]))
    lib = sf.lib
    import ctypes as C
    lp, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))

    def raw(sign, k, Wp, Wi, Wx, flags=0):
        Wp, Wi, Wx = np.ascontiguousarray(Wp, dtype=np.int64), np.ascontiguousarray(Wi, dtype=np.int64), np.ascontiguousarray(Wx, dtype=np.float64)
        return lib.sf_chol_plan_update(plan._h, sign, k, lp(Wp), lp(Wi), dp(Wx), flags)

    assert raw(0, 1, *good) == 1 and raw(2, 1, *good) == 1                      # sign
    assert raw(1, -1, *good) == 1                                               # k < 0
    assert raw(1, 1, [0, 1], [n], [1.0]) == 1 and raw(1, 1, [0, 1], [-1], [1.0]) == 1
    assert raw(1, 1, [0, 2], [3, 3], [1.0, 1.0]) == 1                           # a duplicate row
    assert raw(1, 1, *good, flags=2) == 1                                       # an unknown flag
    assert raw(1, 1, *good, flags=1) == 1                                       # PERM_IN without an ordering
    bad = ([0, 1, 3], [0, int(st.Super[s0]), outside], [1.0, 1.0, 1.0])
    assert raw(1, 2, *bad) == 1 and plan.stat("update_bad_column") == 1
    # ... in the second chunk too: all columns are checked before the first launch
    Wp = np.concatenate([np.arange(17), [18]])
    assert raw(1, 17, Wp, [0] * 16 + [int(st.Super[s0]), outside], np.ones(18)) == 1 and plan.stat("update_bad_column") == 16
    assert raw(1, 0, [0], [], []) == 0                                          # k = 0 changes nothing
    assert np.array_equal(kr.bits(plan.get_factor()), kr.bits(L0))
    assert plan.stat("bytes_update") == 0
    plan.close()
    # no successful factorization: refused
    p2 = sf.CholPlan(sym)
    p2.set_values(sym.Lx)
    with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
        p2.update(good)
    p2.close()
    # a sharded, a mapped and an out-of-core plan: refused, and what they hold stays bit for bit
    owner, _, _ = sf.subtree_partition(sym, 2)
    for make, reads in ((lambda: sf.CholPlan(sym, phase=sf.phases_for_rank(owner, 0), load_top=True), True),
                        (lambda: sf.CholPlan(sym, owner=owner, rank=0, nranks=2), True)):
        p3 = make()
        p3.set_values(sym.Lx)
        p3.factorize_phase(0)
        before = p3.get_factor().copy()
        for down in (False, True):
            with pytest.raises(sf.SparseFrameError, match="SF_ERR_ARG"):
                p3.update(good, downdate=down)
        assert np.array_equal(kr.bits(p3.get_factor()), kr.bits(before)) and p3.stat("bytes_update") == 0
        p3.close()
    lsym = sf.analyze(n, *CASES[NAMES.index("lap3d_8_nd")][2:6], 1 << 30, "lu", True)
    lu = sf.LUPlan(lsym)
    Wp, Wi, Wx = (np.ascontiguousarray(a) for a in (np.array([0, 1]), np.array([0]), np.array([1.0])))
    assert lib.sf_chol_plan_update(lu._h, 1, 1, lp(Wp), lp(Wi), dp(Wx), 0) == 1
    lu.close()


def test_sync_after_an_update_keeps_the_factor_current():
    """CholPlan.sync() after a successful update must not hand the plan back to the generation of its last factorization"""
    sym, st, A, perm = setup("lap2d_30x17_nd")
    plan = fresh(sym)
    W = make_w(sym, st, 2, "edge", 4)
    A1 = A + W @ W.T
    plan.set_values(ur.values_of(sym, A1))
    plan.update(W)
    plan.sync()
    want = np.linalg.slogdet(A1)[1]
    assert abs(plan.logdet() - want) <= 1e-11 * max(1.0, abs(want))
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    plan.update(W, downdate=True)
    plan.sync()
    plan.set_values(sym.Lx)         # (the values of A again: the generation moves, the factor stays usable for the solves)
    x = plan.solve(np.ones(sym.n))
    assert np.max(np.abs(A @ x - 1.0)) <= 1e-10 * np.max(np.abs(x)) * np.max(np.abs(A))
    plan.close()


def test_selinv_recomputes_against_the_updated_matrix():
    sym, st, A, perm = setup("lap3d_4_nd")
    plan = fresh(sym)
    plan.selinv()
    assert plan.stat("selinv_valid") == 1
    W = make_w(sym, st, 3, "edge", 11)
    plan.set_values(ur.values_of(sym, A + W @ W.T))
    plan.update(W)
    assert plan.stat("selinv_valid") == 0
    with pytest.raises(sf.SparseFrameError):
        plan.selinv_diag()
    plan.selinv()
    want = np.diag(np.linalg.inv(A + W @ W.T))
    assert np.max(np.abs(plan.selinv_diag() - want)) <= 1e-11 * np.max(np.abs(want))
    kappa = plan.condest()
    assert 0.3 * np.linalg.cond(A + W @ W.T, 1) <= kappa * 3.0
    plan.close()
