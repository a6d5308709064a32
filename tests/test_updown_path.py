"""The path of a rank-k update and the admissibility rule (csrc/sf_updown_path.cpp) through sf_chol_plan_update_path on
schedule-only plans: no device anywhere in this file."""
import ctypes as C
import functools

import numpy as np
import pytest

import updown_ref as ur
from util import sf, small_cases, wide_cases

lib = sf._lib.lib
CASES = small_cases() + wide_cases()
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def setup(name):
    _, n, Cp, Ci, Cx, perm, slot = CASES[NAMES.index(name)]
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    return sym, ur.Structure(sym), sf.Schedule(sym, np.zeros(sym.nsuper, dtype=np.int32), 0, 1)


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _raw(sch, k, Wp, Wi, flags=0, supers=True):
    """(rc, count, supers, bad) of one raw call"""
    Wp, Wi = np.ascontiguousarray(Wp, dtype=np.int64), np.ascontiguousarray(Wi, dtype=np.int64)
    count, bad = np.full(1, -7, dtype=np.int64), np.full(1, -7, dtype=np.int64)
    out = np.full(max(sch.nsuper, 1), -1, dtype=np.int64)
    rc = lib.sf_chol_plan_update_path(sch._h, k, _lp(Wp), _lp(Wi), flags, _lp(count), _lp(out) if supers else None, _lp(bad))
    return rc, int(count[0]), out, int(bad[0])


def _columns(st, rng):
    """admissible columns of every kind: a diagonal entry, an existing edge, a full clique, starts in leaves and in roots"""
    cols = []
    roots = [s for s in range(st.nsuper) if st.parent(s) < 0]
    leaves = sorted(set(range(st.nsuper)) - {st.parent(s) for s in range(st.nsuper)})
    for s in {leaves[0], leaves[-1], roots[0], roots[-1], int(rng.integers(st.nsuper))}:
        r = st.clique(s)
        cols.append(r[:1])                                  # a diagonal entry
        if len(r) > 1:
            cols.append(np.array([r[0], r[-1]]))            # an existing edge: first column, last row
            cols.append(rng.permutation(r))                 # the whole clique, rows in any order
        j = int(st.Super[s]) + st.nscol(s) // 2             # from the middle of the supernode
        cols.append(st.clique(s, j))
    return cols


@pytest.mark.parametrize("name", NAMES)
def test_containment_and_order(name):
    """below(s) is contained in cols(parent) + below(parent), relaxed supernodes included; the rows below are ascending and the
    parent has a larger number: what the rule and the ascending order of the path rest on"""
    _, st, _ = setup(name)
    for s in range(st.nsuper):
        assert np.array_equal(st.rows(s)[:st.nscol(s)], np.arange(st.Super[s], st.Super[s + 1]))
        b = st.below(s)
        assert np.all(np.diff(b) > 0) and (len(b) == 0 or b[0] >= st.Super[s + 1])
        p = st.parent(s)
        if p >= 0:
            assert p > s
            assert np.all(np.isin(b, st.rows(p))), (name, s, p)


@pytest.mark.parametrize("name", NAMES)
def test_path_is_the_ancestor_walk(name):
    sym, st, sch = setup(name)
    rng = np.random.default_rng(NAMES.index(name))
    cols = _columns(st, rng)
    for c in cols:
        assert st.admissible(c)
    for group in [[c] for c in cols] + [cols, cols[::-1], cols[:2] + [np.zeros(0, dtype=np.int64)] + cols[2:4]]:
        Wp = np.concatenate([[0], np.cumsum([len(c) for c in group])])
        Wi = np.concatenate(group) if len(group) else np.zeros(0)
        rc, count, out, bad = _raw(sch, len(group), Wp, Wi)
        want = st.path(group)
        assert (rc, bad, count) == (0, -1, len(want))
        assert out[:count].tolist() == want
        assert np.all(np.diff(out[:count]) > 0)
        assert _raw(sch, len(group), Wp, Wi, supers=False)[:2] == (0, len(want))       # supers may be NULL
        got = sch.update_path((Wp, Wi, None))
        assert got.tolist() == want


def test_forest_two_trees():
    sym, st, sch = setup("blockdiag")
    roots = [s for s in range(st.nsuper) if st.parent(s) < 0]
    assert len(roots) >= 3
    tree = lambda s: s if st.parent(s) < 0 else tree(st.parent(s))      # noqa: E731
    a = 0
    b = next(s for s in range(st.nsuper) if tree(s) != tree(a))
    cols = [st.clique(a)[:1], st.clique(b)[:1]]
    W = np.zeros((sym.n, 2))
    W[cols[0], 0] = 1.0
    W[cols[1], 1] = 2.0
    got = sch.update_path(W).tolist()
    assert got == st.path(cols)
    assert {tree(s) for s in got} == {tree(a), tree(b)}
    assert got == sorted(set(st.path(cols[:1])) | set(st.path(cols[1:])))


@pytest.mark.parametrize("name", ["lap3d_8_nd", "lap2d_30x17_nd", "arrow_900_200", "band_500"])
def test_bad_column_is_reported(name):
    sym, st, sch = setup(name)
    # a row that is neither a column of s0 nor below it: from a leaf with a parent, a row of no ancestor at all or of a far one
    s0 = next(s for s in range(st.nsuper) if st.parent(s) >= 0 and len(np.setdiff1d(np.arange(st.Super[s + 1], sym.n), st.rows(s))))
    outside = int(np.setdiff1d(np.arange(st.Super[s0 + 1], sym.n), st.rows(s0))[0])
    good, bad_col = st.clique(s0)[:2], np.array([outside, int(st.Super[s0])])
    assert not st.admissible(bad_col)
    for group, want in (([bad_col], 0), ([good, bad_col], 1), ([good, good[:1], bad_col, bad_col], 2), ([good] * 17 + [bad_col], 17)):
        Wp = np.concatenate([[0], np.cumsum([len(c) for c in group])])
        rc, count, out, bad = _raw(sch, len(group), Wp, np.concatenate(group))
        assert (rc, count, bad) == (1, 0, want)
        assert np.all(out == -1)
        assert sch.update_path((Wp, np.concatenate(group), None), return_bad=True) == (None, want)
    with pytest.raises(sf.SparseFrameError):
        sch.update_path((np.array([0, 2]), bad_col, None))


def test_refusals_without_a_device():
    sym, st, sch = setup("lap3d_4_nd")
    n = sym.n
    ok = (1, [0, 1], [0])
    assert _raw(sch, *ok)[0] == 0
    assert _raw(sch, 0, [0], [])[:2] == (0, 0)                                  # k = 0: the empty path
    assert _raw(sch, -1, [0], [])[0] == 1                                       # k < 0
    assert _raw(sch, 1, [0, 1], [n])[0] == 1 and _raw(sch, 1, [0, 1], [-1])[0] == 1     # a row out of range
    assert _raw(sch, 1, [0, 2], [0, 0])[0] == 1                                 # a row twice in a column
    assert _raw(sch, 2, [0, 1, 2], [0, 0])[0] == 0                              # ... but once in each of two columns is fine
    assert _raw(sch, 1, [0, 1], [0], flags=2)[0] == 1 and _raw(sch, 1, [0, 1], [0], flags=4)[0] == 1   # unknown flag bits
    assert _raw(sch, 1, [0, 1], [0], flags=1)[0] == 1                           # SF_DEV_PERM_IN without an ordering
    assert _raw(sch, 1, [1, 0], [0])[0] == 1                                    # offsets that go down
    count = np.zeros(1, dtype=np.int64)
    assert lib.sf_chol_plan_update_path(None, 0, _lp(np.zeros(1, dtype=np.int64)), None, 0, _lp(count), None, None) == 1
    assert lib.sf_chol_plan_update_path(sch._h, 0, None, None, 0, _lp(count), None, None) == 1
    assert lib.sf_chol_plan_update_path(sch._h, 0, _lp(np.zeros(1, dtype=np.int64)), None, 0, None, None, None) == 1
    # an LU schedule is refused; so is the update itself on a plan without a device
    lsym = sf.analyze(n, *CASES[NAMES.index("lap3d_4_nd")][2:5], CASES[NAMES.index("lap3d_4_nd")][5], 1 << 30, "lu", True)
    lsch = sf.Schedule(lsym, np.zeros(lsym.nsuper, dtype=np.int32), 0, 1, lu=True)
    assert _raw(lsch, *ok)[0] == 1
    Wp, Wi, Wx = np.array([0, 1]), np.array([0]), np.array([1.0])
    for sign in (1, -1):
        assert lib.sf_chol_plan_update(sch._h, sign, 1, _lp(Wp), _lp(Wi), Wx.ctypes.data_as(C.POINTER(C.c_double)), 0) == 1
    ooc = sf.Schedule(sym, None, 0, 1, ooc_group=np.zeros(sym.nsuper, dtype=np.int32), ooc_ngroups=1)
    assert _raw(ooc, *ok)[0] == 0                                               # the path needs the structure only


def test_mapped_rank_schedules_answer_too():
    """a rank's part of a mapped factorization has the whole structure: the same path on every rank"""
    name = "lap3d_8_nd"
    sym, st, sch = setup(name)
    owner, _, _ = sf.subtree_partition(sym, 2)
    col = st.clique(0)[:1]
    want = st.path([col])
    for rank in range(2):
        part = sf.Schedule(sym, owner, rank, 2)
        assert _raw(part, 1, [0, 1], col)[2][:len(want)].tolist() == want
