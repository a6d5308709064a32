"""tests/sample_ref.py against independent statements: the Philox4x32-10 known answers, the stream's independence of how it is cut,
the moments of the normals, and the supernodal half solves against dense triangular solves."""
import numpy as np
import pytest
import scipy.linalg

import sample_ref
from util import sf, small_cases, dense_reference_factor

KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = tuple(int(r) for r in sample_ref.philox4x32_10(counter, key))
    assert got == want, [f"{r:08x}" for r in got]


def test_philox_vectorised_matches_scalar():
    c = np.arange(5, dtype=np.uint64) * np.uint64(0x01234567)
    r = sample_ref.philox4x32_10((c, 3, c[::-1], 0), (11, 12))
    for j in range(5):
        one = sample_ref.philox4x32_10((int(c[j]), 3, int(c[4 - j]), 0), (11, 12))
        assert [int(w[j]) for w in r] == [int(w) for w in one]


def test_normals_do_not_depend_on_the_cut():
    whole = sample_ref.normals(7, 1000, 0, 40)
    assert np.array_equal(sample_ref.normals(7, 1000, 17, 5), whole[:, 17:22])       # an odd first sample: pairs split across the cut
    assert np.array_equal(sample_ref.normals(7, 1000, 16, 16), whole[:, 16:32])
    assert np.array_equal(sample_ref.normals(7, 300, 0, 40), whole[:300])
    assert sample_ref.normals(7, 10, 3, 0).shape == (10, 0)
    assert not np.array_equal(sample_ref.normals(8, 1000, 0, 40), whole)
    assert np.isfinite(whole).all()


def test_normals_moments():
    """N = 1,149,984 normals, every statistic capped at five of its standard deviations"""
    n, k = 35937, 32
    Z = sample_ref.normals(20261019, n, 0, k)
    N = Z.size
    mean = abs(Z.mean()) * np.sqrt(N)
    var = abs(Z.var() - 1.0) / np.sqrt(2.0 / N)
    Cc = np.corrcoef(Z.T)
    np.fill_diagonal(Cc, 0.0)
    corr = np.abs(Cc).max() * np.sqrt(n)
    print(f"mean {mean:.3f} var {var:.3f} corr {corr:.3f} (sigmas)")
    assert mean <= 5.0 and var <= 5.0 and corr <= 5.0, (mean, var, corr)


@pytest.mark.parametrize("case", small_cases(), ids=lambda c: c[0])
def test_half_solve_against_dense(oracle, case):
    name, n, Cp, Ci, Cx, perm, slot = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    Lsx, info, _ = oracle.chol_factorize(sym)
    assert info == 0
    _, L = dense_reference_factor(sym)
    B = np.random.default_rng(1).standard_normal((n, 3))
    close = lambda got, want: np.allclose(got, want, rtol=1e-12, atol=1e-13 * np.abs(want).max())
    Y = sample_ref.half_solve(sym, Lsx, B, "L")
    assert close(Y, scipy.linalg.solve_triangular(L, B, lower=True))
    assert close(sample_ref.half_solve(sym, Lsx, B, "Lt"), scipy.linalg.solve_triangular(L, B, lower=True, trans="T"))
    # one vector, and the two halves one after the other: the whole solve
    assert close(sample_ref.half_solve(sym, Lsx, B[:, 1], "L"), Y[:, 1])
    x = sample_ref.half_solve(sym, Lsx, Y[:, 1], "Lt")
    assert close(x, oracle.chol_solve(sym, Lsx, np.ascontiguousarray(B[:, 1])))
