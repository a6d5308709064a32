"""The numpy emulation of the update / downdate launches (tests/updown_ref.py) against a longdouble dense Cholesky of A +- W W^T: what
the GPU tests (tests/test_updown.py, tests/test_kernels_updown.py) compare the kernels with is itself right.  CPU only."""
import functools

import numpy as np
import pytest

import kernel_ref as kr
import updown_ref as ur
from util import sf, small_cases, wide_cases

CASES = [c for c in small_cases() + wide_cases() if c[1] > 1]
NAMES = [c[0] for c in CASES]
pytestmark = pytest.mark.skipif(not kr.have_longdouble(), reason="needs an 80-bit long double")


@functools.lru_cache(maxsize=None)
def setup(name):
    _, n, Cp, Ci, Cx, perm, slot = CASES[NAMES.index(name)]
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    st = ur.Structure(sym)
    A = ur.dense_matrix(sym)
    return sym, st, A, ur.chol_panels(sym, st, A)


def _w(st, n, name):
    """two admissible columns: the clique of a leaf's first column and an edge / diagonal bump further up its chain"""
    rng = np.random.default_rng(NAMES.index(name))
    W = np.zeros((n, 2))
    r = st.clique(0)
    W[r, 0] = rng.uniform(0.5, 1.0, len(r))
    p = st.parent(0)
    r = st.clique(p if p >= 0 else 0, count=2)
    W[r, 1] = rng.uniform(0.5, 1.0, len(r)) * np.array([1.0, -1.0])[:len(r)]
    return W


def _tol(st, k):
    """every entry passes through at most n k rotations of a few roundings each, relative to the panel's scale: 8 n k u"""
    return 8.0 * st.n * k * kr.U


@pytest.mark.parametrize("name", NAMES)
def test_emulation_against_longdouble_factor(name):
    sym, st, A, L0 = setup(name)
    W = _w(st, sym.n, name)
    low = st.lower_mask()
    scale = np.max(np.abs(L0))
    up, failed, path = ur.update_emulate(st, L0, W, +1)
    assert not failed
    want = ur.chol_panels(sym, st, A + W @ W.T)
    assert np.max(np.abs(up - want)[low]) <= _tol(st, 2) * max(scale, np.max(np.abs(want)))
    # panels off the path, and the strict upper parts of the diagonal blocks, keep their bits
    off = ~st.panel_mask(path) | ~low
    assert np.array_equal(kr.bits(up)[off], kr.bits(L0)[off])
    # and back down again
    down, failed, path2 = ur.update_emulate(st, up, W, -1)
    assert not failed and path2 == path
    assert np.max(np.abs(down - L0)[low]) <= 4 * _tol(st, 2) * scale
    assert np.array_equal(kr.bits(down)[off], kr.bits(L0)[off])


@pytest.mark.parametrize("name", ["lap3d_4_nd", "blockdiag", "dense_70", "diagonal_5"])
def test_chunks_commute(name):
    """17 columns run as 16 + 1: the same A' as the dense factorization of A + W W^T"""
    sym, st, A, L0 = setup(name)
    rng = np.random.default_rng(5)
    W = np.zeros((sym.n, 17))
    for t in range(17):
        s = int(rng.integers(st.nsuper))
        r = st.clique(s, count=int(rng.integers(1, 4)))
        W[r, t] = rng.uniform(-1, 1, len(r))
    up, failed, _ = ur.update_emulate(st, L0, W, +1)
    assert not failed
    want = ur.chol_panels(sym, st, A + W @ W.T)
    low = st.lower_mask()
    assert np.max(np.abs(up - want)[low]) <= _tol(st, 17) * np.max(np.abs(want))


@pytest.mark.parametrize("name", NAMES)
def test_inadmissible_column_is_rejected(name):
    sym, st, A, L0 = setup(name)
    cand = [(s, np.setdiff1d(np.arange(st.Super[s + 1], sym.n), st.rows(s))) for s in range(st.nsuper)]
    cand = [(s, o) for s, o in cand if len(o)]
    if not cand:        # every column sees every later row (one dense supernode, a diagonal matrix's lone columns): nothing to reject
        assert all(st.admissible(st.clique(s)) for s in range(st.nsuper))
        return
    s, outside = cand[0]
    W = np.zeros(sym.n)
    W[[int(st.Super[s]), int(outside[0])]] = 1.0
    assert not st.admissible(np.flatnonzero(W))
    with pytest.raises(ValueError):
        ur.update_emulate(st, L0, W, +1)


@pytest.mark.parametrize("name", NAMES)
def test_indefinite_downdate_raises_the_flag(name):
    sym, st, A, L0 = setup(name)
    j = sym.n // 2
    W = np.zeros(sym.n)
    W[j] = 2.0 * np.sqrt(A[j, j])
    _, failed, _ = ur.update_emulate(st, L0, W, -1)
    assert failed
    # the same column as an update is fine, and a downdate that keeps A' definite does not raise it
    assert not ur.update_emulate(st, L0, W, +1)[1]
    assert not ur.update_emulate(st, L0, 5e-4 * W, -1)[1]


def test_zero_column_is_the_identity_bit_for_bit():
    """c = 1, s = 0 exactly: what lets the kernels run a chunk's zero columns and the supernodes a column does not reach"""
    sym, st, A, L0 = setup("lap3d_8_nd")
    W = np.zeros((sym.n, 2))
    W[st.clique(0), 0] = 0.75
    one, _, path = ur.update_emulate(st, L0, W[:, :1], +1)
    two, _, _ = ur.update_emulate(st, L0, W, +1)
    assert np.array_equal(kr.bits(one), kr.bits(two))
    for sign in (+1, -1):
        same, failed, _ = ur.update_emulate(st, L0, np.zeros((sym.n, 1)), sign)
        assert not failed and np.array_equal(kr.bits(same), kr.bits(L0))
