"""The C ABI of the LU plans' half solves and of C^T A^-1 B without a device (sf_lu_plan_solve_half, sf_lu_plan_gram,
sf_lu_plan_gram_device): exported symbols, the constants against the header, the refusals that are decided before anything touches
a device, the resource usage of the kernels of sf_gram_lu.hip, and LUPlan's own argument checks."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from test_half_abi import LIB, ROOT, _dp, _resource_usage, _schedule
from util import sf, gen

SF_OK, SF_ERR_ARG = 0, 1
SYMBOLS = ("sf_lu_plan_solve_half", "sf_lu_plan_gram", "sf_lu_plan_gram_device")
HALVES = {"L": 0, "U": 1, "UT": 2, "LT": 3}
MAX_K = 1024
FILL = 7.0
NAMES = ("half_solve", "cross_gram", "cross_gram_device", "schur_complement", "solve_saddle")


def _addr(a):
    """a host array's address where a device address is expected: every call here is refused before any pointer is looked at"""
    return C.c_void_p(a.ctypes.data)


def test_symbols_exported():
    nm = subprocess.run(["nm", "-D", LIB], stdout=subprocess.PIPE, text=True).stdout
    for name in SYMBOLS:
        assert f" T {name}" in nm, name


def test_constants_match_the_header():
    with open(os.path.join(ROOT, "include", "sparseframe_flat.h")) as fh:
        hdr = fh.read()
    for name, value in HALVES.items():
        assert f"#define SF_LU_HALF_{name:<2} {value} " in hdr, name
    assert f"#define SF_GRAM_MAX_K {MAX_K}\n" in hdr
    assert sf.LUPlan.GRAM_MAX_K == MAX_K
    assert sf.LUPlan._HALVES == {"L": 0, "U": 1, "Ut": 2, "Lt": 3}


def _all_refused(h, n):
    ld = max(n, 1)
    B = np.ones((ld, 3), order="F")
    Cc = np.ones((ld, 2), order="F")
    X = np.full((ld, 3), FILL, order="F")
    G = np.full((2, 3), FILL, order="F")
    lib = sf.lib
    for which in HALVES.values():
        for k in (3, 1, 0):         # ... even with nothing to solve
            assert lib.sf_lu_plan_solve_half(h, which, k, _dp(B), ld, _dp(X), ld) == SF_ERR_ARG
    for m, k in ((2, 3), (1, 1), (1, 3), (0, 3), (2, 0)):
        assert lib.sf_lu_plan_gram(h, m, _dp(Cc), ld, k, _dp(B), ld, _dp(G), 2) == SF_ERR_ARG
        for flags in (0, 1):
            assert lib.sf_lu_plan_gram_device(h, flags, m, _addr(Cc), ld, k, _addr(B), ld, _addr(G), 2) == SF_ERR_ARG
    assert np.all(X == FILL) and np.all(G == FILL) and np.all(B == 1.0) and np.all(Cc == 1.0)


def test_null_plan():
    _all_refused(None, 4)


def test_bad_arguments():
    """what is wrong with the arguments alone is said before the plan is looked at (an LU schedule: refused anyway, so nothing is
    ever written)"""
    sym, sch = _schedule(lu=True)
    n, h, lib = sym.n, sch._h, sf.lib
    B = np.ones((n, 3), order="F")
    Cc = np.ones((n, 2), order="F")
    X = np.full((n, 3), FILL, order="F")
    G = np.full((2, 3), FILL, order="F")
    wide = np.ones((1, 1))          # (never read: the size is refused first)
    half, gram, gdev = lib.sf_lu_plan_solve_half, lib.sf_lu_plan_gram, lib.sf_lu_plan_gram_device
    assert half(h, 0, 3, None, n, _dp(X), n) == SF_ERR_ARG
    assert half(h, 0, 3, _dp(B), n, None, n) == SF_ERR_ARG
    for which in (4, -1, 17):
        assert half(h, which, 3, _dp(B), n, _dp(X), n) == SF_ERR_ARG
    assert half(h, 1, -1, _dp(B), n, _dp(X), n) == SF_ERR_ARG
    assert half(h, 2, 3, _dp(B), n - 1, _dp(X), n) == SF_ERR_ARG
    assert half(h, 3, 3, _dp(B), n, _dp(X), n - 1) == SF_ERR_ARG
    assert half(h, 0, 3, _dp(X), n + 1, _dp(X), n) == SF_ERR_ARG            # in place needs ldx == ldb
    assert gram(h, 2, None, n, 3, _dp(B), n, _dp(G), 2) == SF_ERR_ARG
    assert gram(h, 2, _dp(Cc), n, 3, None, n, _dp(G), 2) == SF_ERR_ARG
    assert gram(h, 2, _dp(Cc), n, 3, _dp(B), n, None, 2) == SF_ERR_ARG
    assert gram(h, -1, _dp(Cc), n, 3, _dp(B), n, _dp(G), 2) == SF_ERR_ARG
    assert gram(h, 2, _dp(Cc), n, -1, _dp(B), n, _dp(G), 2) == SF_ERR_ARG
    assert gram(h, MAX_K + 1, _dp(wide), n, 3, _dp(B), n, _dp(G), MAX_K + 1) == SF_ERR_ARG
    assert gram(h, 2, _dp(Cc), n, MAX_K + 1, _dp(wide), n, _dp(G), 2) == SF_ERR_ARG
    assert gram(h, 2, _dp(Cc), n - 1, 3, _dp(B), n, _dp(G), 2) == SF_ERR_ARG
    assert gram(h, 2, _dp(Cc), n, 3, _dp(B), n - 1, _dp(G), 2) == SF_ERR_ARG
    assert gram(h, 2, _dp(Cc), n, 3, _dp(B), n, _dp(G), 1) == SF_ERR_ARG
    assert gdev(h, 0, 2, None, n, 3, _addr(B), n, _addr(G), 2) == SF_ERR_ARG
    assert gdev(h, 0, 2, _addr(Cc), n, 3, None, n, _addr(G), 2) == SF_ERR_ARG
    assert gdev(h, 0, 2, _addr(Cc), n, 3, _addr(B), n, None, 2) == SF_ERR_ARG
    assert gdev(h, 0, -1, _addr(Cc), n, 3, _addr(B), n, _addr(G), 2) == SF_ERR_ARG
    assert gdev(h, 0, 2, _addr(Cc), n, MAX_K + 1, _addr(wide), n, _addr(G), 2) == SF_ERR_ARG
    assert gdev(h, 0, 2, _addr(Cc), n - 1, 3, _addr(B), n, _addr(G), 2) == SF_ERR_ARG
    assert gdev(h, 0, 2, _addr(Cc), n, 3, _addr(B), n - 1, _addr(G), 2) == SF_ERR_ARG
    assert gdev(h, 0, 2, _addr(Cc), n, 3, _addr(B), n, _addr(G), 1) == SF_ERR_ARG
    for flags in (2, 3, 4, -1):     # SF_DEV_PERM_OUT and anything else that is not SF_DEV_PERM_IN
        assert gdev(h, flags, 2, _addr(Cc), n, 3, _addr(B), n, _addr(G), 2) == SF_ERR_ARG
    assert np.all(X == FILL) and np.all(G == FILL)
    sch.close()


@pytest.mark.parametrize("lu", [True, False], ids=["lu", "cholesky"])
def test_schedule_only_plans_refused(lu):
    """an LU schedule has no device side; a Cholesky handle is refused at the LU entry points whatever it is"""
    sym, sch = _schedule(lu)
    _all_refused(sch._h, sym.n)
    sch.close()


def test_out_of_core_schedule_refused():
    sym, sch = _schedule(ooc=True)
    _all_refused(sch._h, sym.n)
    sch.close()


@pytest.mark.parametrize("rank", [0, 1])
def test_mapped_schedules_refused(rank):
    """rank `rank`'s part of a two-rank factorization (partial, mapped), LU and Cholesky"""
    from util import nd_perm_py
    N = 8
    for lu in (True, False):
        if lu:
            n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
            sym = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", False)
        else:
            n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
            sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
        owner, _, _ = sf.subtree_partition(sym, 2, 0.75)
        sch = sf.Schedule(sym, owner, rank, 2, lu=lu)
        _all_refused(sch._h, sym.n)
        sch.close()


def test_kernels_use_no_scratch(tmp_path):
    t = _resource_usage("sf_gram_lu.hip", tmp_path)
    assert sum("k_gram2_part" in k for k in t) == 1 and sum("k_gram2_final" in k for k in t) == 1, sorted(t)
    assert sum("k_dot_part" in k for k in t) == 1 and sum("k_dot_final" in k for k in t) == 1, sorted(t)
    assert len(t) == 4, sorted(t)           # no sweep, pack or load kernel of its own
    assert all(v["ScratchSize"] == 0 for v in t.values()), t
    # the shared row walk moved to a header: sf_gram.hip still compiles to its two kernels (tests/test_gram_abi.py has the rest)
    g = _resource_usage("sf_gram.hip", tmp_path)
    assert len(g) == 2 and all(v["ScratchSize"] == 0 for v in g.values()), g


def _bare_plan(n):
    """an LUPlan with no handle: whatever reaches the library fails there with SparseFrameError, not with ValueError / TypeError"""
    plan = sf.LUPlan.__new__(sf.LUPlan)
    plan.n, plan.device, plan._h = n, 0, None
    return plan


def test_python_argument_checks():
    """LUPlan's own checks come before the library is called; a Cholesky plan has none of the five"""
    for name in NAMES:
        assert hasattr(sf.LUPlan, name) and not hasattr(sf.CholPlan, name), name
    n = 6
    plan = _bare_plan(n)
    ok = np.ones((n, 2))
    for bad in (np.ones((n + 1, 2)), np.ones(n - 1), np.ones((n, 2, 2))):
        with pytest.raises(ValueError):
            plan.half_solve(bad)
        with pytest.raises(ValueError):
            plan.cross_gram(bad, ok)
        with pytest.raises(ValueError):
            plan.cross_gram(ok, bad)
    for which in ("l", "LT", "Ltt", 0, None):
        with pytest.raises(ValueError):
            plan.half_solve(ok, which)
    with pytest.raises(ValueError):
        plan.cross_gram(np.ones((n, MAX_K + 1)), ok)
    with pytest.raises(ValueError):
        plan.cross_gram(ok, np.ones((n, MAX_K + 1)))
    assert plan.half_solve(np.empty((n, 0))).shape == (n, 0)                    # no columns: no call
    assert plan.cross_gram(np.empty((n, 0)), ok).shape == (0, 2)
    assert plan.cross_gram(ok, np.empty((n, 0))).shape == (2, 0)
    for call in (lambda: plan.half_solve(ok, "Ut"), lambda: plan.cross_gram(ok, np.ones((n, 3))), lambda: plan.cross_gram(np.ones(n), np.ones(n))):
        with pytest.raises(sf.SparseFrameError):
            call()                                                              # (a well-formed call does reach the library)
    with pytest.raises(ValueError):
        plan.schur_complement(ok, np.ones((n, 3)), np.ones((3, 2)))
    with pytest.raises(ValueError):
        plan.schur_complement(np.ones((n + 1, 2)), ok, np.ones((2, 2)))
    B, Cc, f, g = np.ones((n, 2)), np.ones((n, 2)), np.ones(n), np.ones(2)
    for args in ((B, Cc, np.ones(n + 1), g), (B, Cc, f, np.ones(3)), (np.ones(n), np.ones(n), f, np.ones(1)), (np.ones((n + 1, 2)), Cc, f, g),
                 (B, np.ones((n, 3)), f, g), (B, Cc, f, g, np.ones((3, 3))), (np.ones((n, MAX_K)), np.ones((n, MAX_K)), f, np.ones(MAX_K))):
        with pytest.raises(ValueError):
            plan.solve_saddle(*args)
    # cross_gram_device: not a tensor, the wrong type, the wrong place, the wrong shape -- judged on the tensor's attributes alone
    with pytest.raises(TypeError):
        plan.cross_gram_device(np.ones((n, 2)), np.ones((n, 2)))

    def fake(shape, strides, dtype="torch.float64", cuda=True, index=0):
        return types.SimpleNamespace(data_ptr=lambda: 4096, dtype=dtype, shape=shape, stride=lambda: strides, is_cuda=cuda,
                                     device=types.SimpleNamespace(index=index))

    good = fake((n, 2), (1, n))
    with pytest.raises(TypeError):
        plan.cross_gram_device(fake((n, 2), (1, n), dtype="torch.float32"), good)
    for bad in (fake((n, 2), (1, n), cuda=False), fake((n, 2), (1, n), index=1), fake((n - 1, 2), (1, n - 1)), fake((n, 2, 2), (1, n, 2 * n)),
                fake((n, MAX_K + 1), (1, n))):
        with pytest.raises(ValueError):
            plan.cross_gram_device(bad, good)
        with pytest.raises(ValueError):
            plan.cross_gram_device(good, bad)
    three = fake((n, 3), (1, n))
    for bad_out in (fake((3, 2), (1, 3)), fake((2, 2), (1, 2)), fake((2, 3), (3, 1)), fake((2,), (1,)), fake((2, 3), (1, 2), index=1)):
        with pytest.raises(ValueError):
            plan.cross_gram_device(good, three, out=bad_out)
