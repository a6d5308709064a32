"""What a row deletion / addition touches (csrc/sf_rowmod_path.cpp) through sf_chol_plan_rowmod_path on schedule-only
plans: no device anywhere in this file.  The reference is the brute force of tests/rowmod_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import rowmod_ref as rr
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


def _raw(sch, row, Ai, flags=0, lists=True):
    """(rc, (nrows, nsweep, nupdate), the four lists, bad) of one raw call"""
    Ai = np.ascontiguousarray(Ai, dtype=np.int64)
    cnt, bad = np.full(3, -7, dtype=np.int64), np.full(1, -7, dtype=np.int64)
    out = np.full((4, max(sch.nsuper, 1)), -1, dtype=np.int64)
    ptr = (lambda a: _lp(a)) if lists else (lambda a: None)
    rc = lib.sf_chol_plan_rowmod_path(sch._h, row, len(Ai), _lp(Ai) if len(Ai) else None, flags, _lp(cnt[0:]), ptr(out[0]), ptr(out[1]),
                                      _lp(cnt[1:]), ptr(out[2]), _lp(cnt[2:]), ptr(out[3]), _lp(bad))
    return rc, tuple(int(v) for v in cnt), out, int(bad[0])


def _rows(st, name):
    return rr.rows_to_try(st, NAMES.index(name)) if st.n > 1 else [0]


def _own_column(sym, j):
    """the pattern of A's column and row j in the plan's numbering"""
    Lp, Li = np.asarray(sym.Lp), np.asarray(sym.Li)
    col = np.repeat(np.arange(sym.n), np.diff(Lp))
    return np.union1d(Li[Lp[j]:Lp[j + 1]], col[Li == j])


@pytest.mark.parametrize("name", NAMES)
def test_lists_are_the_reference(name):
    sym, st, sch = setup(name)
    for j in _rows(st, name):
        s, c = rr.locate(st, j)
        own = _own_column(sym, j)
        before = [i for i in range(j) if rr.admissible_index(st, j, i)]
        for idx in (None, own, own[::-1], np.array(before + [j], dtype=np.int64)):
            want = rr.lists(st, j, idx)
            rc, cnt, out, bad = _raw(sch, j, [] if idx is None else idx)
            assert (rc, bad) == (0, -1)
            assert cnt == (len(want["rows"]), len(want["sweep"]), len(want["update"]))
            assert list(zip(out[0, :cnt[0]].tolist(), out[1, :cnt[0]].tolist())) == want["rows"]
            assert out[2, :cnt[1]].tolist() == want["sweep"] and out[3, :cnt[2]].tolist() == want["update"]
            assert _raw(sch, j, [] if idx is None else idx, lists=False)[:2] == (0, cnt)        # the lists may be NULL
            got = sch.rowmod_path(j, idx)
            assert got == want
            # every sweep supernode has the row below it; the sweep is ascending and ends before s
            for p in want["sweep"]:
                assert j in st.below(p)
            sweep = out[2, :cnt[1]]
            assert np.all(np.diff(sweep) > 0) and (len(sweep) == 0 or sweep[-1] < s)
            # the panels that hold the row: ascending, before s, and the position names it
            for p, pos in want["rows"]:
                assert p < s and pos >= st.nscol(p) and st.rows(p)[pos] == j
            # the update's path is that of w = L(j + 1:, j)
            w = st.rows(s)[c + 1:]
            assert want["update"] == (sch.update_path((np.array([0, len(w)]), w, None)).tolist() if len(w) else [])
        if idx is None:
            assert cnt[1] == 0


@pytest.mark.parametrize("name", NAMES)
def test_index_outside_the_rule_is_refused(name):
    sym, st, sch = setup(name)
    for j in _rows(st, name):
        own = _own_column(sym, j)
        outside = [i for i in range(sym.n) if not rr.admissible_index(st, j, i)]
        if not outside:
            continue
        for bad_i in (outside[0], outside[-1]):
            for pos in (0, len(own)):
                idx = np.insert(own, pos, bad_i)
                rc, cnt, out, bad = _raw(sch, j, idx)
                assert (rc, cnt, bad) == (1, (0, 0, 0), pos)
                assert np.all(out == -1)
        with pytest.raises(sf.SparseFrameError):
            sch.rowmod_path(j, [outside[0], j])


def test_some_case_has_something_to_refuse():
    assert any(not rr.admissible_index(setup(n)[1], 0, i) for n in ("lap3d_8_nd", "arrow_900_200") for i in range(setup(n)[0].n))


def test_refusals_without_a_device():
    sym, st, sch = setup("lap3d_4_nd")
    n = sym.n
    assert _raw(sch, 0, [0])[0] == 0
    assert _raw(sch, -1, [])[0] == 1 and _raw(sch, n, [])[0] == 1               # a row out of range
    assert _raw(sch, 0, [n])[0] == 1 and _raw(sch, 0, [-1])[0] == 1             # an index out of range
    assert _raw(sch, 0, [0, 0])[0] == 1                                         # an index twice
    own = _own_column(sym, 3)
    assert _raw(sch, 3, np.concatenate([own, own[:1]]))[0] == 1
    assert _raw(sch, 0, [0], flags=2)[0] == 1 and _raw(sch, 0, [0], flags=4)[0] == 1    # unknown flag bits
    assert _raw(sch, 0, [0], flags=1)[0] == 1                                   # SF_DEV_PERM_IN without an ordering
    assert lib.sf_chol_plan_rowmod_path(None, 0, 0, None, 0, *[None] * 8) == 1
    assert lib.sf_chol_plan_rowmod_path(sch._h, 0, 0, None, 0, *[None] * 8) == 0        # every output may be NULL
    assert lib.sf_chol_plan_rowmod_path(sch._h, 0, 1, None, 0, *[None] * 8) == 1        # indices announced, none given
    assert lib.sf_chol_plan_rowmod_path(sch._h, 0, -1, None, 0, *[None] * 8) == 1
    # an LU schedule is refused; so are the two calls themselves on a plan without a device
    lsym = sf.analyze(n, *CASES[NAMES.index("lap3d_4_nd")][2:5], CASES[NAMES.index("lap3d_4_nd")][5], 1 << 30, "lu", True)
    lsch = sf.Schedule(lsym, np.zeros(lsym.nsuper, dtype=np.int32), 0, 1, lu=True)
    assert _raw(lsch, 0, [0])[0] == 1
    Ai, Ax = np.array([0], dtype=np.int64), np.array([4.0])
    assert lib.sf_chol_plan_rowdel(sch._h, 0, 0) == 1
    assert lib.sf_chol_plan_rowadd(sch._h, 0, 1, _lp(Ai), Ax.ctypes.data_as(C.POINTER(C.c_double)), 0) == 1
    ooc = sf.Schedule(sym, None, 0, 1, ooc_group=np.zeros(sym.nsuper, dtype=np.int32), ooc_ngroups=1)
    assert _raw(ooc, 0, [0])[0] == 0                                            # the lists need the structure only
