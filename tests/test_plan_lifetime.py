"""Plans give back what they took: every feature that allocates device state on first use is exercised on a small plan, and the
library's counters of live device blocks and live pinned blocks (sf_debug_live_blocks, kept by the allocator seam of
sf_device_mem.h) must be back where they started once the plan is closed.  The shapes are the smallest on which every path
allocates; the numbers the calls return are other tests' business."""
import ctypes as C

import numpy as np
import pytest

from util import sf, gen, nd_perm_py

lib = sf._lib.lib
pytestmark = pytest.mark.gpu

SF_ERR_ARG = 1


def _live():
    return int(lib.sf_debug_live_blocks(0)), int(lib.sf_debug_live_blocks(1))


class _Returned:
    """with _Returned() as c: ... c.held() inside asserts that device blocks are held; on the way out both counters are back"""

    def __enter__(self):
        self.start = _live()
        return self

    def held(self):
        now = _live()
        assert now[0] > self.start[0], (self.start, now)
        return now

    def __exit__(self, et, ev, tb):
        if et is None:
            assert _live() == self.start, (self.start, _live())
        return False


def _chol(N=8):
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    perm = sf.grid_nd_perm(N, N, N)
    return n, Cx, perm, sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30)


def _lu_own_u(N=8):
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
    perm = nd_perm_py(N, N, N)
    return n, Cx, perm, sf.analyze(n, Cp, Ci, Cx, perm, 1 << 30, "lu", False)


def _pattern_reads(plan, S, n, rng, own_u):
    """selinv and everything that reads it: the arena and scratch, the diagonal, positions and marks, parts, the pair stage"""
    plan.selinv()
    plan.selinv_diag()
    plan.selinv_values()
    V = rng.standard_normal((len(S.Lx), 3))
    if own_u:
        plan.selinv_trace(V, rng.standard_normal((len(S.Ux), 3)))
    else:
        plan.selinv_trace(V)
    vals, outside = plan.selinv_entries(np.arange(n), np.arange(n))
    assert outside == 0 and np.all(np.isfinite(vals))
    plan.logdet()


def test_cholesky_plan_returns_everything():
    import torch
    n, Cx, perm, S = _chol()
    rng = np.random.default_rng(0)
    b = rng.standard_normal(n)
    with _Returned() as c:
        plan = sf.CholPlan(S)
        plan.set_values(S.Lx)
        plan.factorize()
        c.held()
        x = plan.solve(b)
        plan.solve_many(rng.standard_normal((n, 17)))
        plan.solve_half(b)
        plan.quadform(b)
        plan.gram(rng.standard_normal((n, 5)))
        before = plan.stat("bytes_gram")
        plan.gram(rng.standard_normal((n, 33)))         # grows the store once
        assert plan.stat("bytes_gram") > before
        plan.sample(3, seed=1)
        plan.set_ordering(perm)
        nsrc, mapL, mapU = S.value_map()
        plan.set_value_map(nsrc, mapL, mapU)
        plan.set_values_mapped_device(torch.tensor(Cx[:nsrc], dtype=torch.float64, device="cuda:0"))
        plan.factorize()
        plan.solve_device(torch.tensor(b, dtype=torch.float64, device="cuda:0"), perm_in=True, perm_out=True)
        plan.validate()
        plan.residual(b, x)
        plan.refine(b)
        plan.condest()
        _pattern_reads(plan, S, n, rng, False)
        plan.factorize_to_host(S.Lx)                    # the rings, the download streams and their events
        assert _live()[1] > c.start[1]
        hashes = C.POINTER(C.c_uint64)()
        lib.sf_plan_panel_hashes.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint64))]
        lib.sf_plan_panel_hashes.restype = C.c_int
        assert lib.sf_plan_panel_hashes(plan._h, C.byref(hashes)) == 0
        held = c.held()
        plan.solve(b)                                   # nothing of the above allocates a second time
        plan.gram(rng.standard_normal((n, 33)))
        plan.selinv()
        assert _live() == held
        plan.close()


def test_lu_plan_with_its_own_u_returns_everything():
    import torch
    n, Cx, perm, S = _lu_own_u()
    rng = np.random.default_rng(1)
    b = rng.standard_normal(n)
    with _Returned() as c:
        plan = sf.LUPlan(S)
        plan.set_values(S.Lx, S.Ux)
        plan.factorize()
        c.held()
        x = plan.solve(b)
        plan.solve(b, trans=True)
        plan.solve_many(rng.standard_normal((n, 17)))
        plan.solve_many(rng.standard_normal((n, 17)), trans=True)
        plan.half_solve(b, "L")
        plan.cross_gram(rng.standard_normal((n, 5)), rng.standard_normal((n, 5)))
        plan.cross_gram(rng.standard_normal((n, 33)), rng.standard_normal((n, 17)))     # grows the store
        plan.get_factor()                               # d_pack
        plan.set_ordering(perm)
        nsrc, mapL, mapU = S.value_map()
        plan.set_value_map(nsrc, mapL, mapU)
        plan.set_values_mapped_device(torch.tensor(Cx[:nsrc], dtype=torch.float64, device="cuda:0"))     # the max |a_ij| parts
        plan.factorize()
        plan.solve_device(torch.tensor(b, dtype=torch.float64, device="cuda:0"), perm_in=True, perm_out=True)
        plan.validate()
        plan.residual(b, x)
        plan.refine(b)
        plan.condest()
        _pattern_reads(plan, S, n, rng, True)
        plan.get_selinv()                               # the pack temporary
        plan.factorize_to_host(S.Lx, S.Ux)
        assert _live()[1] > c.start[1]
        c.held()
        plan.close()
    with _Returned() as c:                              # pivoting: the pivot records, nothing else
        plan = sf.LUPlan(S)
        plan.set_pivoting(0.1)
        plan.set_values(S.Lx, S.Ux)
        plan.factorize()
        plan.solve(b)
        c.held()
        plan.close()


def test_lu_plan_on_a_symmetric_structure_returns_everything():
    N = 8
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    S = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30, "lu", True)
    with _Returned() as c:
        plan = sf.LUPlan(S)                             # U aliases L
        plan.set_values(S.Lx)
        plan.factorize()
        plan.selinv()
        plan.selinv_values()
        c.held()
        plan.close()


def test_out_of_core_plan_returns_everything():
    n, _, _, S = _chol(12)
    total = int((np.diff(S.Super) * np.diff(S.Lsip)).sum())
    g, ng, ge, te, nd, fits = sf.ooc_partition(S, int(total * 0.6))
    assert ng >= 2
    with _Returned() as c:
        plan = sf.CholPlan(S, ooc_group=g, ooc_ngroups=ng)
        c.held()
        plan.factorize_to_host(S.Lx)
        assert _live()[1] > c.start[1]
        plan.close()


def test_refused_creation_returns_everything():
    """a structure validate_structure refuses (tests/test_kernels.py::_defects, "beyond n"): by then the helper thread has
    allocated the factor and uploaded the structure"""
    n, _, _, S = _chol()
    j = int(S.Super[S.nsuper - 1])
    p = int(S.Lp[j + 1])
    Li = np.insert(S.Li, p, n)
    Lp = S.Lp.copy()
    Lp[j + 1:] += 1
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (S.Super, S.SuperMap, S.Lsip, S.Lsi, S.Lsxp, Lp, Li)]
    with _Returned():
        h = C.c_void_p()
        rc = lib.sf_chol_plan_create(C.byref(h), 0, S.n, S.nsuper, *[a.ctypes.data_as(C.POINTER(C.c_int64)) for a in arrs])
        assert rc == SF_ERR_ARG and h.value is None


def test_struct_path_returns_everything():
    """the factor is the pool's: lent to the plan, neither freed nor counted by it"""
    N = 8
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    with _Returned():
        common = sf.CommonInfo(dev_slot_size=1 << 30)
        mi = sf.MatrixInfo()
        mi.set_csc(n, Cp, Ci, Cx)
        mi.set_perm(sf.grid_nd_perm(N, N, N))
        mi.analyze(common)
        mi.factorize(common)
        mi.cleanup()
        common.close()
