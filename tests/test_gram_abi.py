"""The Gram matrix's C ABI without a device (sf_chol_plan_gram, sf_chol_plan_gram_device): exported symbols, the refusals that are
decided before anything touches a device, the resource usage of the kernels of sf_gram.hip, and CholPlan's own argument checks."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from test_half_abi import LIB, ROOT, _dp, _resource_usage, _schedule
from util import sf, gen

SF_OK, SF_ERR_ARG = 0, 1
SYMBOLS = ("sf_chol_plan_gram", "sf_chol_plan_gram_device")
MAX_K = 1024
FILL = 7.0


def _addr(a):
    """a host array's address where a device address is expected: every call here is refused before any pointer is looked at"""
    return C.c_void_p(a.ctypes.data)


def test_symbols_exported():
    nm = subprocess.run(["nm", "-D", LIB], stdout=subprocess.PIPE, text=True).stdout
    for name in SYMBOLS:
        assert f" T {name}" in nm, name


def test_max_k_matches_the_header():
    with open(os.path.join(ROOT, "include", "sparseframe_flat.h")) as fh:
        hdr = fh.read()
    assert f"#define SF_GRAM_MAX_K {MAX_K}\n" in hdr
    assert sf.CholPlan.GRAM_MAX_K == MAX_K


def _all_refused(h, n):
    ld = max(n, 1)
    B = np.ones((ld, 3), order="F")
    G = np.full((3, 3), FILL, order="F")
    lib = sf.lib
    for k in (3, 1, 0):             # ... even with nothing to compute
        assert lib.sf_chol_plan_gram(h, k, _dp(B), ld, _dp(G), 3) == SF_ERR_ARG
        for flags in (0, 1):
            assert lib.sf_chol_plan_gram_device(h, flags, k, _addr(B), ld, _addr(G), 3) == SF_ERR_ARG
    assert np.all(G == FILL) and np.all(B == 1.0)


def test_null_plan():
    _all_refused(None, 4)


def test_bad_arguments():
    """what is wrong with the arguments alone is said before the plan is looked at"""
    sym, sch = _schedule()
    n, h, lib = sym.n, sch._h, sf.lib
    B = np.ones((n, 3), order="F")
    G = np.full((3, 3), FILL, order="F")
    wide = np.ones((1, 1))          # (never read: k is refused first)
    assert lib.sf_chol_plan_gram(h, 3, None, n, _dp(G), 3) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram(h, 3, _dp(B), n, None, 3) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram(h, -1, _dp(B), n, _dp(G), 3) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram(h, MAX_K + 1, _dp(wide), n, _dp(G), MAX_K + 1) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram(h, 3, _dp(B), n - 1, _dp(G), 3) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram(h, 3, _dp(B), n, _dp(G), 2) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram_device(h, 0, 3, None, n, _addr(G), 3) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram_device(h, 0, 3, _addr(B), n, None, 3) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram_device(h, 0, -1, _addr(B), n, _addr(G), 3) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram_device(h, 0, MAX_K + 1, _addr(wide), n, _addr(G), MAX_K + 1) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram_device(h, 0, 3, _addr(B), n - 1, _addr(G), 3) == SF_ERR_ARG
    assert lib.sf_chol_plan_gram_device(h, 0, 3, _addr(B), n, _addr(G), 2) == SF_ERR_ARG
    for flags in (2, 3, 4, -1):     # SF_DEV_PERM_OUT and anything else that is not SF_DEV_PERM_IN
        assert lib.sf_chol_plan_gram_device(h, flags, 3, _addr(B), n, _addr(G), 3) == SF_ERR_ARG
    assert np.all(G == FILL)
    sch.close()


@pytest.mark.parametrize("lu", [False, True], ids=["cholesky", "lu"])
def test_schedule_only_plans_refused(lu):
    sym, sch = _schedule(lu)
    _all_refused(sch._h, sym.n)
    sch.close()


def test_out_of_core_schedule_refused():
    sym, sch = _schedule(ooc=True)
    _all_refused(sch._h, sym.n)
    sch.close()


@pytest.mark.parametrize("rank", [0, 1])
def test_mapped_schedules_refused(rank):
    N = 8
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    owner, _, _ = sf.subtree_partition(sym, 2, 0.75)
    sch = sf.Schedule(sym, owner, rank, 2)
    _all_refused(sch._h, sym.n)
    sch.close()


def test_kernels_use_no_scratch(tmp_path):
    t = _resource_usage("sf_gram.hip", tmp_path)
    assert sum("k_gram_part" in k for k in t) == 1 and sum("k_gram_final" in k for k in t) == 1, sorted(t)
    assert len(t) == 2, sorted(t)           # no sweep, pack or one-column kernel of its own
    assert all(v["ScratchSize"] == 0 for v in t.values()), t


def _bare_plan(n):
    """a CholPlan with no handle: whatever reaches the library fails there with SparseFrameError, not with ValueError / TypeError"""
    plan = sf.CholPlan.__new__(sf.CholPlan)
    plan.n, plan.device, plan._h = n, 0, None
    return plan


def test_python_argument_checks():
    """CholPlan's own checks come before the library is called; an LU plan has none of the four"""
    for name in ("gram", "gram_device", "schur", "solve_bordered"):
        assert hasattr(sf.CholPlan, name) and not hasattr(sf.LUPlan, name), name
    n = 6
    plan = _bare_plan(n)
    for bad in (np.ones((n + 1, 2)), np.ones(n - 1), np.ones((n, 2, 2)), np.ones((n, MAX_K + 1))):
        with pytest.raises(ValueError):
            plan.gram(bad)
    assert plan.gram(np.empty((n, 0))).shape == (0, 0)              # no columns: no call
    with pytest.raises(sf.SparseFrameError):
        plan.gram(np.ones((n, 2)))                                  # (a well-formed call does reach the library)
    with pytest.raises(ValueError):
        plan.schur(np.ones((n, 2)), np.ones((3, 3)))
    with pytest.raises(ValueError):
        plan.schur(np.ones((n + 1, 2)), np.ones((2, 2)))
    B, f, g = np.ones((n, 2)), np.ones(n), np.ones(2)
    for args in ((B, np.ones(n + 1), g), (B, f, np.ones(3)), (np.ones(n), f, np.ones(1)), (np.ones((n + 1, 2)), f, g),
                 (B, f, g, np.ones((3, 3))), (np.ones((n, MAX_K)), f, np.ones(MAX_K))):
        with pytest.raises(ValueError):
            plan.solve_bordered(*args)
    # gram_device: not a tensor, the wrong type, the wrong place, the wrong shape -- judged on the tensor's attributes alone
    with pytest.raises(TypeError):
        plan.gram_device(np.ones((n, 2)))

    def fake(shape, strides, dtype="torch.float64", cuda=True, index=0):
        return types.SimpleNamespace(data_ptr=lambda: 4096, dtype=dtype, shape=shape, stride=lambda: strides, is_cuda=cuda,
                                     device=types.SimpleNamespace(index=index))

    with pytest.raises(TypeError):
        plan.gram_device(fake((n, 2), (1, n), dtype="torch.float32"))
    for bad in (fake((n, 2), (1, n), cuda=False), fake((n, 2), (1, n), index=1), fake((n - 1, 2), (1, n - 1)), fake((n, 2, 2), (1, n, 2 * n)),
                fake((n, MAX_K + 1), (1, n))):
        with pytest.raises(ValueError):
            plan.gram_device(bad)
    good = fake((n, 2), (1, n))
    for bad_out in (fake((3, 3), (1, 3)), fake((2, 2), (2, 1)), fake((2,), (1,)), fake((2, 2), (1, 2), index=1)):
        with pytest.raises(ValueError):
            plan.gram_device(good, out=bad_out)
