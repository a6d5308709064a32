"""LU selected inversion's C ABI without a device: exported symbols, argument checks that run before anything touches a device,
zero scratch for the kernels of sf_selinv_lu.hip, and the numpy reference of the algorithm and its two-arena indexing
(lu_selinv_ref) against dense inverses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from util import sf, gen, nd_perm_py, rel_err
from lu_selinv_ref import lu_selinv_ref, units, UW
from test_lu import lu_cases, lu_wide_cases, dense_lu_nopiv, reference_layout_from_dense, _dense_unsym_csc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "libsparseframe_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SF_ERR_ARG = 1
SYMBOLS = ("sf_lu_plan_selinv", "sf_lu_plan_get_selinv_range", "sf_lu_plan_selinv_diag", "sf_lu_plan_logdet")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def unsym_block_case(sizes, seed=5):
    """block-diagonal dense unsymmetric strictly diagonally dominant blocks: one supernode of exactly k columns per block"""
    rng = np.random.default_rng(seed)
    n_ = sum(sizes)
    A = np.zeros((n_, n_))
    o = 0
    for k in sizes:
        B = rng.uniform(-1, 1, (k, k))
        B[np.arange(k), np.arange(k)] = np.abs(B).sum(axis=1) + 1.0
        A[o:o + k, o:o + k] = B
        o += k
    return ("unsym_blocks_" + "_".join(map(str, sizes)),) + _dense_unsym_csc(A) + (None, 1 << 30, False)


def lu_selinv_cases():
    """(name, n, Cp, Ci, Cx, perm, devSlotSize, symmetric) -- shared by the CPU and the GPU tests"""
    band = [c for c in lu_wide_cases() if c[0] == "band_unsym_900_130"]
    assert len(band) == 1
    return lu_cases() + [unsym_block_case((64, 65)), unsym_block_case((512, 513, 3)), band[0] + (None, 1 << 30, False)]


def dense_permuted(sym, n, Cp, Ci, Cx, symm):
    A = gen.dense_from_lower(n, Cp, Ci, Cx) if symm else gen.dense_from_csc(n, Cp, Ci, Cx)
    return A[np.ix_(sym.Perm, sym.Perm)]


def test_symbols_exported():
    nm = subprocess.run(["nm", "-D", LIB], stdout=subprocess.PIPE, text=True).stdout
    for name in SYMBOLS:
        assert f" T {name}" in nm


def _all_refused(h, n, xsize):
    d = np.zeros(max(n, 1))
    out = np.zeros(max(xsize, 1))
    sign = C.c_int(7)
    assert sf.lib.sf_lu_plan_selinv(h) == SF_ERR_ARG
    assert sf.lib.sf_lu_plan_get_selinv_range(h, 0, xsize, _dp(out)) == SF_ERR_ARG
    assert sf.lib.sf_lu_plan_selinv_diag(h, _dp(d)) == SF_ERR_ARG
    assert sf.lib.sf_lu_plan_logdet(h, _dp(d), C.byref(sign)) == SF_ERR_ARG
    assert sf.lib.sf_lu_plan_logdet(h, _dp(d), None) == SF_ERR_ARG


def test_null_plan():
    _all_refused(None, 4, 4)


@pytest.mark.parametrize("lu", [True, False], ids=["lu", "cholesky"])
def test_schedule_only_plans_refused(lu):
    N = 8
    if lu:
        n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, seed=5)
        sym = sf.analyze(n, Cp, Ci, Cx, nd_perm_py(N, N, N), 1 << 30, "lu", False)
    else:
        n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)
    sch = sf.Schedule(sym, np.zeros(sym.nsuper, dtype=np.int32), 0, 1, lu=lu)
    _all_refused(sch._h, sym.n, sym.xsize)
    sch.close()


def test_lu_selinv_kernels_use_no_scratch(tmp_path):
    """sf_selinv_lu.hip compiled device-only for gfx950: every kernel in it reports zero scratch"""
    src = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "csrc", "sf_selinv_lu.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-c", "-O3", "-std=c++17", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "k.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:]
    scratch = {}
    name = None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    # small, trinv, finish, pack, diag, logdet part / final, and the shared GEMM plain / transposed / gathered
    assert len(scratch) == 10, sorted(scratch)
    assert sum("k_lu_selinv" in k for k in scratch) == 5 and sum("k_lu_logdet" in k for k in scratch) == 2
    assert sum("k_selinv_gemm" in k for k in scratch) == 3
    assert all(v == 0 for v in scratch.values()), scratch


@pytest.mark.parametrize("case", lu_selinv_cases(), ids=lambda c: c[0])
def test_reference_against_dense_inverse(case):
    name, n, Cp, Ci, Cx, perm, slot, symm = case
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", symm)
    Ap = dense_permuted(sym, n, Cp, Ci, Cx, symm)
    S = lu_selinv_ref(sym, reference_layout_from_dense(sym, dense_lu_nopiv(Ap)))
    want = reference_layout_from_dense(sym, np.linalg.inv(Ap))
    err = rel_err(S, want)
    print(name, "rel_err", err)
    assert err <= 1e-11, name


def test_unit_decomposition_covers_every_column():
    for name, n, Cp, Ci, Cx, perm, slot, symm in lu_selinv_cases():
        sym = sf.analyze(n, Cp, Ci, Cx, perm, slot, "lu", symm)
        seen = np.zeros(n, dtype=np.int64)
        for J, cb, w in units(sym):
            assert 1 <= w <= UW
            seen[sym.Super[J] + cb: sym.Super[J] + cb + w] += 1
        assert np.all(seen == 1), name
