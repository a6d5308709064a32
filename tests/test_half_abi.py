"""The half solves', the quadratic form's and the sampler's C ABI without a device: exported symbols, the refusals that are decided
before anything touches a device, and the resource usage of the kernels of sf_sample.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from util import sf, gen, nd_perm_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "csrc")
LIB = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "libsparseframe_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SF_OK, SF_ERR_ARG = 0, 1
SYMBOLS = ("sf_chol_plan_solve_half", "sf_chol_plan_quadform", "sf_chol_plan_sample")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_symbols_exported():
    nm = subprocess.run(["nm", "-D", LIB], stdout=subprocess.PIPE, text=True).stdout
    for name in SYMBOLS:
        assert f" T {name}" in nm, name


def _all_refused(h, n):
    ld = max(n, 1)
    B = np.ones((ld, 3), order="F")
    X = np.full((ld, 3), 7.0, order="F")
    Z = np.full((ld, 3), 7.0, order="F")
    q = np.full(3, 7.0)
    lib = sf.lib
    for which in (0, 1):
        for k in (3, 1, 0):         # ... even with nothing to solve
            assert lib.sf_chol_plan_solve_half(h, which, k, _dp(B), ld, _dp(X), ld) == SF_ERR_ARG
    for k in (3, 1, 0):
        assert lib.sf_chol_plan_quadform(h, k, _dp(B), ld, _dp(q)) == SF_ERR_ARG
        assert lib.sf_chol_plan_sample(h, k, 5, 0, _dp(X), ld, _dp(Z), ld) == SF_ERR_ARG
        assert lib.sf_chol_plan_sample(h, k, 5, 0, _dp(X), ld, None, 0) == SF_ERR_ARG
    assert np.all(X == 7.0) and np.all(Z == 7.0) and np.all(q == 7.0)


def _schedule(lu=False, ooc=False):
    N = 8
    if lu:
        n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
        sym = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", False)
    else:
        n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    if ooc:
        return sym, sf.Schedule(sym, None, 0, 1, ooc_group=np.zeros(sym.nsuper, dtype=np.int32), ooc_ngroups=1)
    return sym, sf.Schedule(sym, np.zeros(sym.nsuper, dtype=np.int32), 0, 1, lu=lu)


def test_null_plan():
    _all_refused(None, 4)


def test_bad_arguments():
    """what is wrong with the arguments alone is said before the plan is looked at"""
    sym, sch = _schedule()
    n, h, lib = sym.n, sch._h, sf.lib
    B = np.ones((n, 3), order="F")
    X = np.empty_like(B)
    q = np.empty(3)
    assert lib.sf_chol_plan_solve_half(h, 0, 3, None, n, _dp(X), n) == SF_ERR_ARG
    assert lib.sf_chol_plan_solve_half(h, 0, 3, _dp(B), n, None, n) == SF_ERR_ARG
    assert lib.sf_chol_plan_solve_half(h, 2, 3, _dp(B), n, _dp(X), n) == SF_ERR_ARG
    assert lib.sf_chol_plan_solve_half(h, -1, 3, _dp(B), n, _dp(X), n) == SF_ERR_ARG
    assert lib.sf_chol_plan_solve_half(h, 0, -1, _dp(B), n, _dp(X), n) == SF_ERR_ARG
    assert lib.sf_chol_plan_solve_half(h, 1, 3, _dp(B), n - 1, _dp(X), n) == SF_ERR_ARG
    assert lib.sf_chol_plan_solve_half(h, 1, 3, _dp(B), n, _dp(X), n - 1) == SF_ERR_ARG
    assert lib.sf_chol_plan_quadform(h, 3, None, n, _dp(q)) == SF_ERR_ARG
    assert lib.sf_chol_plan_quadform(h, 3, _dp(B), n, None) == SF_ERR_ARG
    assert lib.sf_chol_plan_quadform(h, 3, _dp(B), n - 1, _dp(q)) == SF_ERR_ARG
    assert lib.sf_chol_plan_sample(h, 3, 0, 0, None, n, None, 0) == SF_ERR_ARG
    assert lib.sf_chol_plan_sample(h, 3, 0, 0, _dp(X), n - 1, None, 0) == SF_ERR_ARG
    assert lib.sf_chol_plan_sample(h, 3, 0, 0, _dp(X), n, _dp(B), n - 1) == SF_ERR_ARG
    assert lib.sf_chol_plan_sample(h, -1, 0, 0, _dp(X), n, None, 0) == SF_ERR_ARG
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


def test_python_argument_checks():
    """CholPlan's own checks come before the library is called; an LU plan has none of the three"""
    for name in ("solve_half", "quadform", "sample"):
        assert hasattr(sf.CholPlan, name) and not hasattr(sf.LUPlan, name), name


def _resource_usage(src, tmp_path):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-c", "-O3", "-std=c++17", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, src), "-o",
                        str(tmp_path / (src + ".o"))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:]
    out = {}
    name = None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_kernels_use_no_scratch(tmp_path):
    t = _resource_usage("sf_sample.hip", tmp_path)
    assert sum("k_sample_fill" in k for k in t) == 1, sorted(t)
    assert sum("k_quadform_part" in k for k in t) == 2 and sum("k_quadform_final" in k for k in t) == 2, sorted(t)     # widths 1 and 16
    assert len(t) == 5, sorted(t)           # no sweep kernel of its own: those are sf_solve.hip's
    assert all(v["ScratchSize"] == 0 for v in t.values()), t
