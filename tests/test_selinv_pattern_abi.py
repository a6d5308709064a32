"""The C ABI of Sigma on the pattern, its traces and its entries without a device (sf_*_plan_selinv_values[_t][_device], _selinv_trace
[_device], _selinv_entries): exported symbols, the constants against the header, every refusal that is decided before anything
touches a device -- with all outputs left as they were --, the resource usage of the kernels of sf_selinv_pattern.hip, and the
plans' own argument checks."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from test_half_abi import LIB, ROOT, _dp, _resource_usage, _schedule
from util import sf, gen

_lib = sf._lib

SF_OK, SF_ERR_ARG = 0, 1
CHOL = ("sf_chol_plan_selinv_values", "sf_chol_plan_selinv_values_device", "sf_chol_plan_selinv_trace", "sf_chol_plan_selinv_trace_device",
        "sf_chol_plan_selinv_entries")
LU = ("sf_lu_plan_selinv_values", "sf_lu_plan_selinv_values_device", "sf_lu_plan_selinv_values_t", "sf_lu_plan_selinv_values_t_device",
      "sf_lu_plan_selinv_trace", "sf_lu_plan_selinv_trace_device", "sf_lu_plan_selinv_entries")
MAX_M = 64
FILL = 7.0
NAMES = ("selinv_values", "selinv_values_device", "selinv_trace", "selinv_trace_device", "selinv_entries", "logdet_grad")


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _addr(a):
    """a host array's address where a device address is expected: every call here is refused before any pointer is looked at"""
    return C.c_void_p(a.ctypes.data)


def test_symbols_exported():
    nm = subprocess.run(["nm", "-D", LIB], stdout=subprocess.PIPE, text=True).stdout
    for name in CHOL + LU:
        assert f" T {name}" in nm, name
        assert getattr(_lib.lu_lib, name) is not None, name       # ... and reachable through the LU struct library, which links it


def test_constants_match_the_header():
    with open(os.path.join(ROOT, "include", "sparseframe_flat.h")) as fh:
        hdr = fh.read()
    assert "#define SF_SEL_MAPPED 1 " in hdr and f"#define SF_SEL_MAX_M {MAX_M}\n" in hdr
    assert sf.api.SEL_MAX_M == MAX_M
    sym, sch = _schedule()
    assert sch.stat("selinv_pattern_max_m") == MAX_M and 1 <= sch.stat("selinv_pattern_chunk") <= MAX_M
    assert sch.stat("selinv_pattern_tile") % 256 == 0 and sch.stat("selinv_entries_chunk") >= 1
    assert sch.stat("bytes_selinv_pattern") == 0 and sch.stat("last_selinv_outside") == 0
    sch.close()
    for name in CHOL + LU:
        assert f"int {name}(" in hdr, name


class Outputs:
    """every output a call could write, prefilled"""

    def __init__(self, nnz, unz, m=3):
        self.L, self.U = np.full(max(nnz, 1), FILL), np.full(max(unz, 1), FILL)
        self.t = np.full(MAX_M, FILL)
        self.e = np.full(4, FILL)
        self.outside = np.full(1, 77, dtype=np.int64)

    def untouched(self):
        return bool(np.all(self.L == FILL) and np.all(self.U == FILL) and np.all(self.t == FILL) and np.all(self.e == FILL)
                    and self.outside[0] == 77)


def _all_refused(h, nnz, unz, n):
    """every entry point of both kinds, host and device forms, with well-formed arguments"""
    lib = sf.lib
    o = Outputs(nnz, unz)
    ldl, ldu = max(nnz, 1), max(unz, 1)
    VL, VU = np.ones((ldl, 3), order="F"), np.ones((ldu, 3), order="F")
    rows, cols = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    assert lib.sf_chol_plan_selinv_values(h, _dp(o.L)) == SF_ERR_ARG
    assert lib.sf_chol_plan_selinv_values_device(h, _addr(o.L)) == SF_ERR_ARG
    for fn in (lib.sf_lu_plan_selinv_values, lib.sf_lu_plan_selinv_values_t):
        assert fn(h, _dp(o.L), _dp(o.U)) == SF_ERR_ARG
        assert fn(h, _dp(o.L), None) == SF_ERR_ARG
    for fn in (lib.sf_lu_plan_selinv_values_device, lib.sf_lu_plan_selinv_values_t_device):
        assert fn(h, _addr(o.L), _addr(o.U)) == SF_ERR_ARG
        assert fn(h, _addr(o.L), None) == SF_ERR_ARG
    for m in (3, 1, 0):         # ... even with nothing to sum
        for flags in (0, 1):
            assert lib.sf_chol_plan_selinv_trace(h, m, _dp(VL), ldl, flags, _dp(o.t)) == SF_ERR_ARG
            assert lib.sf_chol_plan_selinv_trace_device(h, m, _addr(VL), ldl, flags, _addr(o.t)) == SF_ERR_ARG
            assert lib.sf_lu_plan_selinv_trace(h, m, _dp(VL), ldl, _dp(VU), ldu, flags, _dp(o.t)) == SF_ERR_ARG
            assert lib.sf_lu_plan_selinv_trace(h, m, _dp(VL), ldl, None, 0, flags, _dp(o.t)) == SF_ERR_ARG
            assert lib.sf_lu_plan_selinv_trace_device(h, m, _addr(VL), ldl, _addr(VU), ldu, flags, _addr(o.t)) == SF_ERR_ARG
    for count in (4, 1, 0):
        for fn in (lib.sf_chol_plan_selinv_entries, lib.sf_lu_plan_selinv_entries):
            assert fn(h, count, _lp(rows), _lp(cols), _dp(o.e), _lp(o.outside)) == SF_ERR_ARG
            assert fn(h, count, _lp(rows), _lp(cols), _dp(o.e), None) == SF_ERR_ARG
    assert o.untouched()
    assert np.all(VL == 1.0) and np.all(VU == 1.0)


def test_null_plan():
    _all_refused(None, 5, 5, 4)


def _counts(sym, lu):
    return len(sym.Li), (len(sym.Ui) if lu else 0)


@pytest.mark.parametrize("lu", [False, True], ids=["cholesky", "lu"])
def test_schedule_only_plans_refused(lu):
    """a schedule has no device side and no arena: refused at the entry points of its own kind and of the other one"""
    sym, sch = _schedule(lu)
    _all_refused(sch._h, *_counts(sym, lu), sym.n)
    sch.close()


def test_out_of_core_schedule_refused():
    sym, sch = _schedule(ooc=True)
    _all_refused(sch._h, *_counts(sym, False), sym.n)
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
        _all_refused(sch._h, *_counts(sym, lu), sym.n)
        sch.close()


@pytest.mark.parametrize("lu", [False, True], ids=["cholesky", "lu"])
def test_bad_arguments(lu):
    """NULL pointers, negative counts, m above the limit, short leading dimensions, unknown flags, indices outside [0, n): each is
    SF_ERR_ARG with nothing written (on a schedule, which is refused anyway -- so nothing is ever written here either way)"""
    sym, sch = _schedule(lu)
    h, lib, n = sch._h, sf.lib, sym.n
    nnz, unz = _counts(sym, lu)
    o = Outputs(nnz, unz)
    VL, VU = np.ones((nnz, 3), order="F"), np.ones((max(unz, 1), 3), order="F")
    wide = np.ones((1, 1))          # (never read: the count is refused first)
    rows, cols = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    if lu:
        trace = lambda m, vl, ldl, vu, ldu, flags, out: lib.sf_lu_plan_selinv_trace(h, m, vl, ldl, vu, ldu, flags, out)
        assert lib.sf_lu_plan_selinv_values(h, None, _dp(o.U)) == SF_ERR_ARG
        assert lib.sf_lu_plan_selinv_values(h, _dp(o.L), None) == SF_ERR_ARG
        assert lib.sf_lu_plan_selinv_values_t(h, None, _dp(o.U)) == SF_ERR_ARG
        assert lib.sf_lu_plan_selinv_values_device(h, None, _addr(o.U)) == SF_ERR_ARG
        assert trace(3, _dp(VL), nnz, None, unz, 0, _dp(o.t)) == SF_ERR_ARG             # its own U structure needs VU
        assert trace(3, _dp(VL), nnz, _dp(VU), unz - 1, 0, _dp(o.t)) == SF_ERR_ARG
        assert trace(3, _dp(VL), nnz, _dp(VU), unz, 1, _dp(o.t)) == SF_ERR_ARG          # mapped: one array, VU must be NULL
        entries = lib.sf_lu_plan_selinv_entries
    else:
        trace = lambda m, vl, ldl, vu, ldu, flags, out: lib.sf_chol_plan_selinv_trace(h, m, vl, ldl, flags, out)
        assert lib.sf_chol_plan_selinv_values(h, None) == SF_ERR_ARG
        assert lib.sf_chol_plan_selinv_values_device(h, None) == SF_ERR_ARG
        entries = lib.sf_chol_plan_selinv_entries
    assert trace(3, None, nnz, _dp(VU), unz, 0, _dp(o.t)) == SF_ERR_ARG
    assert trace(3, _dp(VL), nnz, _dp(VU), unz, 0, None) == SF_ERR_ARG
    assert trace(-1, _dp(VL), nnz, _dp(VU), unz, 0, _dp(o.t)) == SF_ERR_ARG
    assert trace(MAX_M + 1, _dp(wide), nnz, _dp(wide), unz, 0, _dp(o.t)) == SF_ERR_ARG
    assert trace(3, _dp(VL), nnz - 1, _dp(VU), unz, 0, _dp(o.t)) == SF_ERR_ARG
    for flags in (2, 3, -1, 1 << 8):
        assert trace(3, _dp(VL), nnz, _dp(VU), unz, flags, _dp(o.t)) == SF_ERR_ARG
    assert trace(3, _dp(VL), nnz, None, 0, 1, _dp(o.t)) == SF_ERR_ARG                   # mapped without a stored map
    assert entries(h, -1, _lp(rows), _lp(cols), _dp(o.e), _lp(o.outside)) == SF_ERR_ARG
    assert entries(h, 4, None, _lp(cols), _dp(o.e), _lp(o.outside)) == SF_ERR_ARG
    assert entries(h, 4, _lp(rows), None, _dp(o.e), _lp(o.outside)) == SF_ERR_ARG
    assert entries(h, 4, _lp(rows), _lp(cols), None, _lp(o.outside)) == SF_ERR_ARG
    for bad in (n, -1):
        r2 = rows.copy()
        r2[3] = bad
        assert entries(h, 4, _lp(r2), _lp(cols), _dp(o.e), _lp(o.outside)) == SF_ERR_ARG
        assert entries(h, 4, _lp(rows), _lp(r2), _dp(o.e), _lp(o.outside)) == SF_ERR_ARG
    assert o.untouched()
    sch.close()


def test_kernels_use_no_scratch(tmp_path):
    t = _resource_usage("sf_selinv_pattern.hip", tmp_path)
    assert sum("k_selpat_part" in k for k in t) == 2, sorted(t)            # plain and mapped
    for name in ("k_selpat_final", "k_selpat_gather", "k_selpat_build", "k_selpat_entries"):
        assert sum(name in k for k in t) == 1, (name, sorted(t))
    assert len(t) == 6, sorted(t)           # no sweep, no factorization or selected-inversion kernel of its own
    assert all(v["ScratchSize"] == 0 for v in t.values()), t


def _bare_plan(cls, n, nnz, unz=0, alias=False):
    """a plan with no handle: whatever reaches the library fails there with SparseFrameError, not with ValueError / TypeError"""
    plan = cls.__new__(cls)
    plan.n, plan.device, plan._h, plan._nnz, plan._unz, plan._alias = n, 0, None, nnz, unz, alias
    return plan


def test_python_argument_checks():
    for name in NAMES:
        assert hasattr(sf.CholPlan, name) and hasattr(sf.LUPlan, name), name
    n, nnz, unz = 6, 11, 9
    chol = _bare_plan(sf.CholPlan, n, nnz)
    lu = _bare_plan(sf.LUPlan, n, nnz, unz)
    sym_lu = _bare_plan(sf.LUPlan, n, nnz, 0, alias=True)
    ok, oku = np.ones((nnz, 2)), np.ones((unz, 2))
    for bad in (np.ones((nnz + 1, 2)), np.ones(nnz - 1), np.ones((nnz, 2, 2)), np.ones((nnz, MAX_M + 1))):
        with pytest.raises(ValueError):
            chol.selinv_trace(bad)
        with pytest.raises(ValueError):
            chol.logdet_grad(bad)
        with pytest.raises(ValueError):
            lu.selinv_trace(bad, oku)
        with pytest.raises(ValueError):
            sym_lu.selinv_trace(bad)
    for bad in (np.ones((unz + 1, 2)), np.ones((unz, 3)), np.ones(unz), None):
        with pytest.raises(ValueError):
            lu.selinv_trace(ok, bad)
    with pytest.raises(ValueError):
        chol.selinv_trace(ok, oku)                  # VU is an LU plan's
    with pytest.raises(ValueError):
        sym_lu.selinv_trace(ok, oku)                # ... with its own U structure
    with pytest.raises(ValueError):
        chol.selinv_trace(ok, mapped=True)          # no value map
    with pytest.raises(ValueError):
        chol.selinv_values(transposed=True)
    for rows, cols in ((np.zeros(3), np.zeros(4)), (np.zeros((2, 2)), np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            chol.selinv_entries(rows, cols)
    assert chol.selinv_trace(np.empty((nnz, 0))).shape == (0,)             # no columns: no call
    # well-formed calls do reach the library: any memory order, a padded leading dimension, one column
    big = np.ones((nnz + 3, 2), order="F")
    for V in (ok, np.asfortranarray(ok), big[:nnz], np.ones(nnz), np.ones((nnz, MAX_M))):
        with pytest.raises(sf.SparseFrameError):
            chol.selinv_trace(V)
    for call in (chol.selinv_values, lu.selinv_values, sym_lu.selinv_values, lambda: lu.selinv_trace(ok, oku), lambda: sym_lu.logdet_grad(ok),
                 lambda: chol.selinv_entries([0, 1], [1, 0]), lambda: lu.selinv_values(transposed=True)):
        with pytest.raises(sf.SparseFrameError):
            call()
    # the device forms: judged on the tensor's attributes alone
    with pytest.raises(TypeError):
        chol.selinv_trace_device(np.ones((nnz, 2)))
    with pytest.raises(TypeError):
        chol.selinv_values_device(np.ones(nnz))

    def fake(shape, strides, dtype="torch.float64", cuda=True, index=0):
        return types.SimpleNamespace(data_ptr=lambda: 4096, dtype=dtype, shape=shape, stride=lambda: strides, is_cuda=cuda,
                                     device=types.SimpleNamespace(index=index))

    good = fake((nnz, 2), (1, nnz))
    with pytest.raises(TypeError):
        chol.selinv_trace_device(fake((nnz, 2), (1, nnz), dtype="torch.float32"))
    for bad in (fake((nnz, 2), (1, nnz), cuda=False), fake((nnz, 2), (1, nnz), index=1), fake((nnz - 1, 2), (1, nnz - 1)),
                fake((nnz, 2, 2), (1, nnz, 2 * nnz)), fake((nnz, MAX_M + 1), (1, nnz))):
        with pytest.raises(ValueError):
            chol.selinv_trace_device(bad, out=fake((2,), (1,)))
    for bad_out in (fake((3,), (1,)), fake((2, 1), (1, 2)), fake((2,), (1,), index=1), fake((2,), (1,), cuda=False)):
        with pytest.raises(ValueError):
            chol.selinv_trace_device(good, out=bad_out)
    with pytest.raises(ValueError):
        lu.selinv_trace_device(good, out=fake((2,), (1,)))                 # VU missing
    with pytest.raises(ValueError):
        chol.selinv_values_device(fake((nnz - 1,), (1,)))
    with pytest.raises(ValueError):
        chol.selinv_values_device(fake((nnz, 1), (1, nnz)))
    with pytest.raises(ValueError):
        lu.selinv_values_device(fake((nnz,), (1,)))                         # outU missing
    with pytest.raises(ValueError):
        chol.selinv_values_device(fake((nnz,), (1,)), fake((unz,), (1,)))
