"""Single-launch tests of the numeric kernels of csrc/sf_kernels.hip, of the fused step (csrc/sf_step.hip) and of the device
solve's kernels (csrc/sf_solve.hip) against extended-precision references.

Every other GPU test reaches the kernels through a whole plan, i.e. only at the shapes the symbolic analysis of a few
matrix families produces.  Here a test-only probe (tests/kernels/sf_kprobe.hip, built by the fixture below) runs ONE
launch of a release launcher on task lists the test builds itself, in a host image of the factor arena whose guards and
unread elements hold NaN (tests/kernel_ref.py).  Checked: per-element error bounds (operands scaled over 1e-6 .. 1e6),
the read footprint (no NaN reaches a stored result), the write footprint (everything else bit-identical), the stream-K
partition of k_gemm, pivot records, the load kernels, one step of the solve sweeps (diagonal tasks and row tiles in one
launch), and the plan's validation of the matrix row indices.
"""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import kernel_ref as kr
from util import ROOT, sf, gen

lib = sf._lib.lib
KDIR = os.path.join(ROOT, "tests", "kernels")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

GEMM_BM, GEMM_BK, SU_TM, SU_TN = 128, 16, 64, 32      # sf_kernels.h

GEMM_PROB = np.dtype([("y_off", "<i8"), ("x_off", "<i8"), ("c_off", "<i8"), ("src_rows", "<i8"), ("tgt_rows", "<i8"),
                      ("lda", "<i4"), ("ldc", "<i4"), ("M", "<i4"), ("N", "<i4"), ("K", "<i4"), ("tgt_first_col", "<i4"),
                      ("tgt_nscol", "<i4"), ("tgt_nbelow", "<i4"), ("strict", "<i4"), ("pad_", "<i4"), ("map_off", "<i8")])
GEMM_TASK = np.dtype([("prob", "<i4"), ("tm", "<u2"), ("tn", "<u2"), ("kt0", "<u4"), ("nkt", "<u4")])
POTRF_TASK = np.dtype([("panel", "<i8"), ("ld", "<i4"), ("diag", "<i4"), ("b", "<i4"), ("first_col", "<i4")])
STEP_TASK = np.dtype([("panel", "<i8"), ("xpanel", "<i8"), ("ld", "<i4"), ("J", "<i4"), ("diag", "<i4"), ("b", "<i4"), ("row0", "<i4"),
                      ("nrows", "<i4"), ("flag", "<i4"), ("mode", "<i4"), ("slot", "<i4"), ("next_b", "<i4"), ("first_col", "<i4"),
                      ("pad", "<i4")])
TRSM_TASK = np.dtype([("panel", "<i8"), ("dpanel", "<i8"), ("ld", "<i4"), ("diag", "<i4"), ("b", "<i4"), ("row0", "<i4"),
                      ("nrows", "<i4"), ("unit", "<i4"), ("first_col", "<i4"), ("pad", "<i4")])
SOLVE_TASK = np.dtype([("panel", "<i8"), ("rows", "<i8"), ("ld", "<i4"), ("diag", "<i4"), ("b", "<i4"), ("row0", "<i4"), ("nrows", "<i4"),
                       ("first_col", "<i4"), ("flag", "<i4"), ("expect", "<i4"), ("tdiag", "<i8")])
FILL_TILE = np.dtype([("xp", "<i8"), ("nsrow", "<i4"), ("r0", "<i4"), ("c0", "<i4"), ("cb", "<i4"), ("ce", "<i4")], align=True)
COND_SCALARS = np.dtype([("nrm", "<f8"), ("flags", "<i4"), ("j", "<i4")])
SEL_UNIT = np.dtype([("lx", "<i8"), ("rows", "<i8"), ("nsrow", "<i4"), ("ncol", "<i4"), ("cb", "<i4"), ("w", "<i4"), ("pair0", "<i4"),
                     ("npair", "<i4")])
SEL_PAIR = np.dtype([("map_off", "<i8"), ("i", "<i4"), ("pad_", "<i4")])


def _make(args, timeout):
    return subprocess.run(["make", "-C", KDIR, f"HIPCC={HIPCC}", "-j4"] + args, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=timeout)


def test_probe_compiles(tmp_path):
    """the probe builds against the release library's launchers (no GPU needed)"""
    r = _make([f"OUT={tmp_path / 'libsf_kprobe.so'}"], 300)
    assert r.returncode == 0, r.stdout
    nm = subprocess.run(["nm", "-D", str(tmp_path / "libsf_kprobe.so")], stdout=subprocess.PIPE, text=True).stdout
    for name in ("kp_gemm", "kp_update_small", "kp_potrf", "kp_getrf", "kp_trsm", "kp_step", "kp_build_loadmap", "kp_solve_fwd",
                 "kp_solve_bwd", "kp_pack_lu", "kp_lu_fill_u11", "kp_factor_hash", "kp_tsolve_bwd", "kp_condest_fill", "kp_condest_sign_norm",
                 "kp_condest_argmax_next", "kp_solve_many_pack", "kp_solve_many_unpack", "kp_selinv_small", "kp_lu_selinv_small",
                 "kp_selinv_trinv", "kp_selinv_gemm", "kp_selinv_sum", "kp_selinv_finish", "kp_selinv_diag", "kp_logdet", "kp_lu_selinv_pack",
                 "kp_residual", "kp_loadmap_drop", "kp_refine_resid", "kp_refine_norms", "kp_refine_update", "kp_gram_slabs", "kp_gram_row",
                 "kp_gram2_col", "kp_dot", "kp_quadform", "kp_sample_fill", "kp_dev_load1", "kp_dev_store1", "kp_dev_pack", "kp_dev_unpack",
                 "kp_dev_gather_values", "kp_dev_absmax", "kp_selpat_build", "kp_selpat_gather", "kp_selpat_part", "kp_selpat_final",
                 "kp_selpat_entries"):
        assert f" T {name}" in nm


def test_kernels_compile_with_two_lu_step_workgroups(tmp_path):
    """the documented build knob -DSF_LU_STEP_WGS=2 compiles (device side only)"""
    src = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "csrc", "sf_step.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-c", "-O1", "-std=c++17",
                        "-I" + os.path.join(ROOT, "include"), "-DSF_LU_STEP_WGS=2", src, "-o", str(tmp_path / "k.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]


def test_step_kernel_keeps_three_workgroups_per_cu(tmp_path):
    """k_step (csrc/sf_step.hip) compiled device-only with the library's flags: the compiler's resource remarks of both
    instantiations show 3 waves per SIMD = 3 workgroups per CU, no scratch for the Cholesky variant and no more
    than the 24 bytes / 5 spilled VGPRs the LU variant (168 VGPRs, the limit for that occupancy) has always had"""
    src = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "csrc", "sf_step.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-munsafe-fp-atomics",
                        "-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "k.s")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    res, cur = {}, None
    for line in r.stdout.splitlines():
        if "remark:" not in line:
            continue
        key, _, val = line.split("remark:", 1)[1].split("[-Rpass")[0].strip().rpartition(":")
        if key == "Function Name":
            cur = res.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    lu = [v for k, v in res.items() if "k_stepILb1E" in k]
    chol = [v for k, v in res.items() if "k_stepILb0E" in k]
    assert len(lu) == 1 and len(chol) == 1, sorted(res)
    lu, chol = lu[0], chol[0]
    print("k_step<true>:", lu, "\nk_step<false>:", chol)
    assert int(lu["Occupancy [waves/SIMD]"]) == 3 and int(chol["Occupancy [waves/SIMD]"]) == 3
    assert int(lu["LDS Size [bytes/block]"]) == 41480 and int(chol["LDS Size [bytes/block]"]) == 40968
    assert int(chol["ScratchSize [bytes/lane]"]) == 0 and int(chol["VGPRs Spill"]) == 0
    assert int(lu["ScratchSize [bytes/lane]"]) <= 24 and int(lu["VGPRs Spill"]) <= 5


# ---------------------------------------------------------------------------------------------------------------------
# the plan's validation of the row indices of the matrix (no GPU: schedule-only plans run the same checks)
# ---------------------------------------------------------------------------------------------------------------------
def _symbolic(N=10):
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    return sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30)


def _insert(Lp, Li, Lx, j, i, val, first):
    """(Lp, Li, Lx) with the entry (i, j) added at the start (first) or the end of column j"""
    p = int(Lp[j]) if first else int(Lp[j + 1])
    Li2 = np.insert(Li, p, i)
    Lx2 = np.insert(Lx, p, val)
    Lp2 = Lp.copy()
    Lp2[j + 1:] += 1
    return Lp2, Li2, Lx2


def _defects(sym):
    """(name, j, i): entries that have no place in column j's panel, chosen so that even unchecked code would write inside
    the factor storage"""
    Super, Lsip, Lsi = sym.Super, sym.Lsip, sym.Lsi
    out = []
    s = next(s for s in range(1, sym.nsuper) if Super[s] > 0)
    out.append(("above the first column", int(Super[s]), int(Super[s]) - 1))
    for s in range(sym.nsuper):
        nscol = Super[s + 1] - Super[s]
        rows = Lsi[Lsip[s] + nscol:Lsip[s + 1]]
        gaps = np.flatnonzero(np.diff(rows) > 1)
        if len(gaps):
            out.append(("between two listed rows", int(Super[s]), int(rows[gaps[0]]) + 1))
            break
    out.append(("beyond n", int(Super[sym.nsuper - 1]), int(sym.n)))
    return out


def _schedule_rc(sym, Lp, Li, nranks, lu=False):
    owner = np.zeros(sym.nsuper, dtype=np.int32)
    if nranks > 1:
        owner, _, _ = sf.subtree_partition(sym, nranks, 0.5)
        owner = np.ascontiguousarray(owner, dtype=np.int32)
    h = C.c_void_p()
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (sym.Super, sym.SuperMap, sym.Lsip, sym.Lsi, sym.Lsxp, Lp, Li)]
    lp = [a.ctypes.data_as(C.POINTER(C.c_long)) for a in arrs]
    if lu:
        rc = lib.sf_lu_plan_schedule_mapped(C.byref(h), sym.n, sym.nsuper, *lp, None, None,
                                            owner.ctypes.data_as(C.POINTER(C.c_int32)), 0, nranks)
    else:
        rc = lib.sf_chol_plan_schedule_mapped(C.byref(h), sym.n, sym.nsuper, *lp, owner.ctypes.data_as(C.POINTER(C.c_int32)), 0, nranks)
    ok = h.value is not None
    if ok:
        lib.sf_chol_plan_destroy(h)
    return rc, ok


@pytest.mark.parametrize("nranks", [1, 2])      # 1: the load-map path, 2: the masked search path
def test_plan_rejects_entries_without_a_place(nranks):
    sym = _symbolic()
    rc, ok = _schedule_rc(sym, sym.Lp, sym.Li, nranks)
    assert rc == 0 and ok
    for name, j, i in _defects(sym):
        for first in (True, False):
            Lp, Li, _ = _insert(sym.Lp, sym.Li, sym.Lx, j, i, 1.0, first)
            rc, ok = _schedule_rc(sym, Lp, Li, nranks)
            assert rc == 1 and not ok, (name, first, rc)        # SF_ERR_ARG, no plan
            rc, ok = _schedule_rc(sym, Lp, Li, nranks, lu=True)
            assert rc == 1 and not ok, ("lu", name, first, rc)


def test_plan_accepts_duplicate_entries():
    sym = _symbolic()
    j = int(sym.Super[1])
    Lp, Li, _ = _insert(sym.Lp, sym.Li, sym.Lx, j, j, 1.0, False)
    assert _schedule_rc(sym, Lp, Li, 1) == (0, True)


def _with_duplicates(Cp, Ci, Cx, rng, count):
    """(Cp, Ci, Cx) with `count` entries given twice, the extra copy FIRST in its column and with a wrong value"""
    picks = np.sort(rng.choice(len(Ci), count, replace=False))
    col = np.searchsorted(Cp, picks, side="right") - 1
    Ci2 = np.insert(Ci, picks, Ci[picks])
    Cx2 = np.insert(Cx, picks, Cx[picks] * 3.0 + 1.0)
    Cp2 = Cp + np.concatenate([[0], np.cumsum(np.bincount(col, minlength=len(Cp) - 1))])
    return np.ascontiguousarray(Cp2, dtype=np.int64), np.ascontiguousarray(Ci2, dtype=np.int64), Cx2


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cholesky", "lu_aliased", "lu_explicit_u"])
def test_duplicate_entries_last_one_wins(kind):
    """thousands of entries given twice, the first copy with a wrong value: the factor matches the one without duplicates
    to 1e-12 of its largest entry (the reference's sequential loadA keeps the last copy; a wrong winner is an O(1) change).
    LU with U aliasing L loads every entry into both panels; with an explicit U, U's entries are duplicated too."""
    rng = np.random.default_rng(7)
    N = 12
    if kind == "cholesky":
        sym = _symbolic(N)
        make = lambda S: sf.CholPlan(S, device=0)
    else:
        n, Cp, Ci, Cx = (gen.laplacian_lower(N, N, N) if kind == "lu_aliased" else gen.unsymmetric_stencil(N, N, N, seed=3))
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), 1 << 30, "lu", kind == "lu_aliased")
        make = lambda S: sf.LUPlan(S, device=0)
    explicit_u = kind == "lu_explicit_u"

    def run(S, Lx, Ux):
        plan = make(S)
        if kind == "cholesky":
            plan.set_values(Lx)
        else:
            plan.set_values(Lx, Ux)
        plan.factorize()
        out = plan.get_factor().copy()
        plan.close()
        return out

    want = run(sym, sym.Lx, sym.Ux if explicit_u else None)
    keys = ("n", "nsuper", "Super", "SuperMap", "Lsip", "Lsi", "Lsxp", "xsize", "lu", "symmetric")
    dup = types.SimpleNamespace(**{k: getattr(sym, k) for k in keys if kind != "cholesky" or k not in ("lu", "symmetric")})
    dup.Lp, dup.Li, Lx = _with_duplicates(sym.Lp, sym.Li, sym.Lx, rng, 3000)
    Ux = None
    if explicit_u:
        dup.Up, dup.Ui, Ux = _with_duplicates(sym.Up, sym.Ui, sym.Ux, rng, 3000)
    got = run(dup, Lx, Ux)
    # (the Schur updates add with atomics: the factor is not bit-reproducible from run to run)
    assert np.all(np.isfinite(got))
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


# ---------------------------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kp():
    if not kr.have_longdouble():
        pytest.skip("np.longdouble has no 64-bit mantissa on this platform: no extended-precision reference")
    r = _make([], 600)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(os.path.join(KDIR, "libsf_kprobe.so"))
    for name, dt in (("GemmProb", GEMM_PROB), ("GemmTask", GEMM_TASK), ("PotrfTask", POTRF_TASK), ("TrsmTask", TRSM_TASK), ("StepTask", STEP_TASK),
                     ("SolveTask", SOLVE_TASK), ("FillTile", FILL_TILE), ("CondScalars", COND_SCALARS), ("SelUnit", SEL_UNIT),
                     ("SelPair", SEL_PAIR)):
        assert L.kp_sizeof(name.encode()) == dt.itemsize, name
    vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int, C.c_double
    L.kp_gemm.argtypes = [vp, i64, vp, i32, vp, i32, vp, C.c_uint32, C.c_uint32, i32, vp, i64, i32, i32, i32]
    L.kp_update_small.argtypes = [vp, i64, vp, i32, vp, i32, vp, i64]
    L.kp_build_relmaps.argtypes = [vp, i32, vp, i64, vp, i64]
    L.kp_potrf.argtypes = [vp, i64, vp, i32, vp]
    L.kp_getrf.argtypes = [vp, i64, vp, i32, i64, vp, f64, f64, vp, vp, i64, vp]
    L.kp_trsm.argtypes = [vp, i64, vp, i32, vp, i64]
    L.kp_step.argtypes = [vp, i64, vp, i32, i32, vp, i32, i32, vp, i64, f64, f64, vp, vp, i64, vp]
    L.kp_solve_fwd.argtypes = [vp, i64, vp, i64, vp, i64, vp, i32, i32, i32, i32, i32, vp, i64, i32, vp]
    L.kp_solve_bwd.argtypes = [vp, i64, vp, i64, vp, i64, vp, i32, i32, i32, i32, i64, i32, vp]
    L.kp_tsolve_bwd.argtypes = [vp, i64, vp, i64, vp, i64, vp, i32, i32, i32, i32, vp, i64, i64, i32, vp]
    L.kp_condest_fill.argtypes = [vp, i64, i64, i32]
    L.kp_condest_sign_norm.argtypes = [vp, vp, i64, i64, i32, vp]
    L.kp_condest_argmax_next.argtypes = [vp, i64, i64, vp, i32, i32]
    L.kp_solve_many_pack.argtypes = [vp, i64, i64, i32, vp, i64]
    L.kp_solve_many_unpack.argtypes = [vp, i64, i64, i32, vp, i64]
    L.kp_pack_lu.argtypes = [vp, i64, i64, vp, vp, vp, vp, i32, vp, i64, i64, i64]
    L.kp_lu_fill_u11.argtypes = [vp, i64, i64, vp, i64]
    L.kp_factor_hash.argtypes = [vp, i64, i64, vp, vp, vp, vp, i32, i32, i64, vp]
    L.kp_build_loadmap.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp, i64, i32, vp]
    L.kp_load_mapped.argtypes = [vp, i64, vp, vp, i64]
    L.kp_load_panels.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, vp]
    return L


def P(a):
    return None if a is None else a.ctypes.data


def _ok(rc):
    assert rc == 0, f"HIP error {rc}"


# ---------------------------------------------------------------------------------------------------------------------
# GEMM: k_gemm modes 0 / 1, k_update_small
# ---------------------------------------------------------------------------------------------------------------------
def _gemm_tiles(M, N, K, prob=0, bm=GEMM_BM, bn=GEMM_BM, whole_k=True):
    """the tiles of the lower trapezoid, as the plan lists them (sf_plan_build.hip: GEMM and small-update task lists)"""
    nkt = (K + GEMM_BK - 1) // GEMM_BK
    t = [(prob, tm, tn, 0, nkt if whole_k else 0) for tm in range((M + bm - 1) // bm) for tn in range((N + bn - 1) // bn)
         if (tm + 1) * bm - 1 >= tn * bn]
    return np.array(t, dtype=GEMM_TASK)


def _kt_prefix(tasks):
    return np.concatenate([[0], np.cumsum(tasks["nkt"].astype(np.int64))]).astype(np.uint32)


class GemmCase:
    """one C -= Y X^T problem in an arena: Y rows [0, M), X rows (mode 0: own rows of the same panel; mode 1: Y's first N)"""

    def __init__(self, rng, M, N, K, strict, mode, skew):
        self.M, self.N, self.K, self.strict, self.mode = M, N, K, strict, mode
        ar = kr.Arena()
        sc = kr.scalings(rng, M + N)
        ry, rx = sc[:M], (sc[:N] if mode == 1 else sc[M:])
        Y = ry[:, None] * rng.uniform(-1, 1, (M, K))
        X = Y[:N] if mode == 1 else rx[:, None] * rng.uniform(-1, 1, (N, K))
        xrow = 0 if mode == 1 else M + 3               # mode 0: X rows below Y's, NaN rows between
        lda = xrow + N + 2 + (M + N + skew) % 2 if mode == 0 else M + 1 + skew   # odd lda when skewed
        if skew:
            lda |= 1
        src = ar.alloc(lda * (K + 1), align=2, skew=skew)
        self.prob = np.zeros(1, dtype=GEMM_PROB)
        pb = self.prob[0]
        pb["y_off"], pb["x_off"], pb["lda"], pb["M"], pb["N"], pb["K"], pb["strict"] = src, src + xrow, lda, M, N, K, strict
        if mode == 0:
            ldc = M + 1 + skew
            coff = ar.alloc(ldc * N, align=2, skew=skew)
            pb["c_off"], pb["ldc"] = coff, ldc
            rowmap = np.arange(M)
            colmap = np.arange(N)
            self.relmap = None
        else:
            # target supernode: columns [F, F + nc), rows below: a sorted set; the source rows are a random sorted subset
            F, nc = 1000, N + int(rng.integers(0, 40))
            nb = (M - N) + int(rng.integers(0, 60))
            below = np.sort(rng.choice(np.arange(F + nc, F + nc + 4 * nb + 8), nb, replace=False))
            rows = np.concatenate([np.sort(rng.choice(np.arange(F, F + nc), N, replace=False)),
                                   np.sort(rng.choice(below, M - N, replace=False))])
            Lsi = np.concatenate([np.full(3, -1), rows, np.full(2, -1), below]).astype(np.int32)
            ldc = nc + nb
            coff = ar.alloc(ldc * nc, skew=skew)
            pb["c_off"], pb["ldc"], pb["src_rows"], pb["tgt_rows"] = coff, ldc, 3, 3 + M + 2
            pb["tgt_first_col"], pb["tgt_nscol"], pb["tgt_nbelow"], pb["map_off"] = F, nc, nb, 5
            self.Lsi = Lsi
            rowmap = np.where(np.arange(M) < N, rows - F, nc + np.searchsorted(below, rows))
            colmap = rowmap[:N]
            self.relmap_want = np.concatenate([np.full(5, -7), rowmap, np.full(4, -7)]).astype(np.int32)
        self.arena = ar.image()
        a = self.arena
        srcv = a[src:src + lda * (K + 1)].reshape(K + 1, lda)      # [k][row]
        srcv[:K, :M] = Y.T
        if mode == 0:
            srcv[:K, xrow:xrow + N] = X.T
        C0 = ry[:, None] * rx[None, :] * rng.uniform(-1, 1, (M, N))
        self.ref, self.bound, self.mask = kr.gemm_ref(C0, Y, X, strict)
        self.C0 = C0
        # the target region holds finite sentinels (a stray atomic add into a NaN would leave it NaN, i.e. unnoticed)
        csize = ldc * (N if mode == 0 else nc)
        a[coff:coff + csize] = rng.uniform(-1, 1, csize)
        ci, cj = np.nonzero(self.mask)
        self.tgt = coff + rowmap[ci] + colmap[cj] * ldc      # arena index of every produced element
        a[self.tgt] = C0[ci, cj]
        self.before = a.copy()

    def check(self, after, what):
        written = np.zeros(len(after), dtype=bool)
        written[self.tgt] = True
        kr.assert_unchanged(self.before, after, written, what)
        ci, cj = np.nonzero(self.mask)
        kr.assert_within(after[self.tgt], self.ref[ci, cj], self.bound[ci, cj], what)


def _relmap(kp, case):
    rel = np.full(len(case.relmap_want), -7, dtype=np.int32)
    _ok(kp.kp_build_relmaps(P(case.prob), 1, P(case.Lsi), len(case.Lsi), P(rel), len(rel)))
    assert np.array_equal(rel, case.relmap_want), "k_build_relmaps against np.searchsorted"
    return rel


def _run_gemm(kp, case, tasks, u_lo=None, u_hi=None, ticket=1, whole=0, cap=0, relmap=None, arena=None):
    pre = _kt_prefix(tasks)
    a = (case.arena if arena is None else arena).copy()
    u_lo = 0 if u_lo is None else u_lo
    u_hi = int(pre[-1]) if u_hi is None else u_hi
    _ok(kp.kp_gemm(P(a), len(a), P(case.prob), len(case.prob), P(tasks), len(tasks), P(pre), u_lo, u_hi, case.mode,
                   P(relmap), 0 if relmap is None else len(relmap), ticket, whole, cap))
    return a


GEMM_M = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257]
GEMM_K = [1, 3, 4, 15, 16, 17, 63, 64, 65, 200]


def _gemm_shapes(seed):
    rng = np.random.default_rng(seed)
    out = []
    for M in GEMM_M:
        for K in GEMM_K:
            N = int(rng.choice([n for n in GEMM_M if n <= M]))
            out.append((M, N, K))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_gemm_shapes(kp, mode):
    rng = np.random.default_rng(11 + mode)
    for i, (M, N, K) in enumerate(_gemm_shapes(mode)):
        strict, skew = i % 2, (i // 2) % 2
        case = GemmCase(rng, M, N, K, strict, mode, skew)
        rel = _relmap(kp, case) if mode == 1 else None
        tasks = _gemm_tiles(M, N, K)
        out = _run_gemm(kp, case, tasks, relmap=rel, ticket=i % 3 != 0)
        case.check(out, f"k_gemm<{mode}> M={M} N={N} K={K} strict={strict} skew={skew}")


@pytest.mark.gpu
def test_update_small_shapes(kp):
    rng = np.random.default_rng(5)
    for i, (M, N, K) in enumerate(_gemm_shapes(2)):
        if K > 64:              # the plan routes K <= SU_MAXK only
            continue
        strict, skew = i % 2, (i // 3) % 2
        case = GemmCase(rng, M, N, K, strict, 1, skew)
        rel = _relmap(kp, case)
        tasks = _gemm_tiles(M, N, K, bm=SU_TM, bn=SU_TN, whole_k=False)
        a = case.arena.copy()
        _ok(kp.kp_update_small(P(a), len(a), P(case.prob), 1, P(tasks), len(tasks), P(rel), len(rel)))
        case.check(a, f"k_update_small M={M} N={N} K={K} strict={strict} skew={skew}")


# ---------------------------------------------------------------------------------------------------------------------
# the stream-K partition of k_gemm: many single-tile problems of different K onto ONE target (every unit adds in)
# ---------------------------------------------------------------------------------------------------------------------
class SharedTarget:
    def __init__(self, rng, Ks):
        self.mode = 0
        ar = kr.Arena()
        Kmax = max(Ks)
        M = N = 100
        lda = 2 * M + 5
        src = ar.alloc(lda * (Kmax + 1), skew=1)
        coff = ar.alloc(M * N + 3 * M, skew=1)
        a = ar.image()
        sc = kr.scalings(rng, 2 * M)
        Y = sc[:M, None] * rng.uniform(-1, 1, (M, Kmax))
        X = sc[M:, None] * rng.uniform(-1, 1, (N, Kmax))
        v = a[src:src + lda * (Kmax + 1)].reshape(Kmax + 1, lda)
        v[:Kmax, :M] = Y.T
        v[:Kmax, M + 2:M + 2 + N] = X.T
        ldc = M + 3
        C0 = sc[:M, None] * sc[None, M:] * rng.uniform(-1, 1, (M, N))
        self.mask = np.tril(np.ones((M, N), dtype=bool))
        ci, cj = np.nonzero(self.mask)
        self.tgt = coff + ci + cj * ldc
        a[coff:coff + M * N + 3 * M] = rng.uniform(-1, 1, M * N + 3 * M)      # finite sentinels, see GemmCase
        a[self.tgt] = C0[ci, cj]
        self.arena, self.before = a, a.copy()
        self.prob = np.zeros(len(Ks), dtype=GEMM_PROB)
        for p, K in enumerate(Ks):
            self.prob[p] = (src, src + M + 2, coff, 0, 0, lda, ldc, M, N, K, 0, 0, 0, 0, 0, 0)
        self.tasks = np.array([(p, 0, 0, 0, (K + 15) // 16) for p, K in enumerate(Ks)], dtype=GEMM_TASK)
        ref = C0.astype(kr.LD)
        absb = np.abs(C0).astype(kr.LD)
        for K in sorted(set(Ks)):
            cnt = Ks.count(K)
            ref = ref - cnt * kr.matmul_ld(Y[:, :K], X[:, :K].T)
            absb = absb + cnt * kr.matmul_ld(np.abs(Y[:, :K]), np.abs(X[:, :K]).T)
        self.ref = ref[ci, cj]
        self.bound = (kr.SAFETY * (sum(Ks) + len(Ks) + 2) * kr.U * absb)[ci, cj]

    def check(self, after, what):
        written = np.zeros(len(after), dtype=bool)
        written[self.tgt] = True
        kr.assert_unchanged(self.before, after, written, what)
        kr.assert_within(after[self.tgt], self.ref, self.bound, what)


def _windows(pre, rng):
    """cuts of [0, U): inside a tile, on a tile boundary, and a window wholly inside one tile"""
    U = int(pre[-1])
    long_tiles = [i for i in range(len(pre) - 1) if pre[i + 1] - pre[i] >= 3]
    cuts = {int(pre[len(pre) // 2])}                    # on a boundary
    if long_tiles:
        t = long_tiles[len(long_tiles) // 2]
        cuts |= {int(pre[t]) + 1, int(pre[t]) + 2}        # [pre[t] + 1, pre[t] + 2): inside one tile
    cuts.add(int(rng.integers(1, U)) if U > 1 else 0)
    cuts = sorted(c for c in cuts if 0 < c < U)[:3]
    return list(zip([0] + cuts, cuts + [U]))


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 5, 8, 9, 13, 64, 512])
def test_gemm_stream_k_partition(kp, G):
    rng = np.random.default_rng(G)
    for T in sorted({1, max(G - 1, 1), G, G + 1, 3 * G + 5}):
        # shares below the min_units floor (test_gemm_stream_k_shares_above_min_units covers the other side)
        Kset = [1, 17, 40] if G >= 64 else [5, 200, 420]
        Ks = [Kset[i % 3] for i in range(T)]
        case = SharedTarget(rng, Ks)
        pre = _kt_prefix(case.tasks)
        for ticket in (0, 1):
            out = _run_gemm(kp, case, case.tasks, ticket=ticket, cap=G)
            case.check(out, f"G={G} tiles={T} ticket={ticket}")
        a = case.arena.copy()
        wins = _windows(pre, rng)
        for lo, hi in wins:
            a = _run_gemm(kp, case, case.tasks, lo, hi, ticket=1, cap=G, arena=a)
        case.check(a, f"G={G} tiles={T} windows={wins}")


MIN_UNITS = 16          # SF_GEMM_MIN_UNITS_DEFAULT (sf_kernels.hip, next to k_gemm)


def _split_shares(pre, u_lo, u_hi, G):
    """restatement of k_gemm's partition (sf_kernels.hip, the head / tail branch): the per-workgroup share Ueq of the head
    [u_lo, first whole tile) and of the tail after the whole-tile rounds, for ranges that are not empty"""
    ntasks = len(pre) - 1
    t0 = int(np.searchsorted(pre, u_lo, side="right")) - 1
    if pre[t0] < u_lo:
        t0 += 1
    t1 = int(np.searchsorted(pre, u_hi, side="right")) - 1
    R = (t1 - t0) // G if t1 > t0 else 0
    head_end = int(pre[t0]) if R > 0 else u_hi
    tail_beg = int(pre[t0 + R * G]) if R > 0 else u_hi
    assert t1 <= ntasks
    return [(rb - ra + G - 1) // G for ra, rb in ((u_lo, head_end), (tail_beg, u_hi)) if rb > ra]


@pytest.mark.gpu
@pytest.mark.parametrize("G", [5, 9])
def test_gemm_stream_k_shares_above_min_units(kp, G):
    """shares longer than the min_units floor (U = Ueq, workgroups by XCD share): G - 1 long tiles, and a window over them"""
    rng = np.random.default_rng(100 + G)
    case = SharedTarget(rng, [420] * (G - 1))
    pre = _kt_prefix(case.tasks)
    U = int(pre[-1])
    assert max(_split_shares(pre, 0, U, G)) > MIN_UNITS
    for ticket in (0, 1):
        case.check(_run_gemm(kp, case, case.tasks, ticket=ticket, cap=G), f"G={G} long tiles ticket={ticket}")
    cut = int(pre[0]) + 5                      # inside the first tile
    assert max(_split_shares(pre, cut, U, G)) > MIN_UNITS
    a = _run_gemm(kp, case, case.tasks, 0, cut, ticket=1, cap=G)
    a = _run_gemm(kp, case, case.tasks, cut, U, ticket=1, cap=G, arena=a)
    case.check(a, f"G={G} long tiles, windows [0, {cut}) [{cut}, {U})")


@pytest.mark.gpu
def test_gemm_whole_tiles_bit_reproducible(kp):
    """whole_tiles = 1: one addition per element -- bit-identical over grid caps and the dynamic / static deals"""
    rng = np.random.default_rng(3)
    case = GemmCase(rng, 128 * 40 + 17, 128 * 3 + 5, 75, 0, 0, 1)
    tasks = _gemm_tiles(case.M, case.N, case.K)
    first = None
    for G in (1, 5, 8, 9, 13, 64, 512):
        for ticket in (0, 1):
            out = _run_gemm(kp, case, tasks, ticket=ticket, whole=1, cap=G)
            if first is None:
                case.check(out, "whole_tiles")
                first = out
            else:
                assert np.array_equal(kr.bits(out), kr.bits(first)), f"whole_tiles: G={G} ticket={ticket} differs"


# ---------------------------------------------------------------------------------------------------------------------
# POTRF / GETRF / TRSM blocks
# ---------------------------------------------------------------------------------------------------------------------
BLOCKS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64]


def _spd(rng, b):
    s = kr.scalings(rng, b, 1e-3, 1e3)
    Z = rng.uniform(-1, 1, (b, b))
    A = Z @ Z.T + b * np.eye(b)
    return s[:, None] * A * s[None, :]


def _potrf_launch(kp, mats, ld_extra=3):
    """one launch, one task per matrix; returns the factors and info"""
    ar = kr.Arena()
    offs, tasks = [], []
    for A in mats:
        b = A.shape[0]
        ld, diag = b + ld_extra, 2
        off = ar.alloc(ld * (b + diag + 1), skew=1)
        offs.append((off, ld, diag))
        tasks.append((off, ld, diag, b, 0))
    a = ar.image()
    written = np.zeros(len(a), dtype=bool)
    for A, (off, ld, diag) in zip(mats, offs):
        b = A.shape[0]
        r, c = np.tril_indices(b)
        idx = off + diag + r + (diag + c) * ld
        a[idx] = A[r, c]                                  # lower triangle incl. the diagonal; the rest stays NaN
        written[idx] = True
    before = a.copy()
    tasks = np.array(tasks, dtype=POTRF_TASK)
    info = np.zeros(1, dtype=np.int32)
    _ok(kp.kp_potrf(P(a), len(a), P(tasks), len(tasks), P(info)))
    kr.assert_unchanged(before, a, written, "k_potrf_block")
    out = []
    for A, (off, ld, diag) in zip(mats, offs):
        b = A.shape[0]
        v = a[off:off + ld * (b + diag + 1)].reshape(-1, ld).T      # [row][col]
        out.append(np.tril(v[diag:diag + b, diag:diag + b]))
    return out, int(info[0])


@pytest.mark.gpu
def test_potrf_blocks(kp):
    rng = np.random.default_rng(1)
    mats = [_spd(rng, b) for b in BLOCKS]
    Ls, info = _potrf_launch(kp, mats)
    assert info == 0
    for A, L in zip(mats, Ls):
        kr.potrf_check(A, L, f"potrf b={A.shape[0]}")
        ref = kr.chol_ld(A)
        # forward: the input is a diagonal scaling of a well-conditioned matrix, so the error of row i is small against row i
        rowmax = np.max(np.abs(ref), axis=1, keepdims=True)
        assert np.all(np.abs(L - ref) <= 64 * A.shape[0] * kr.U * rowmax), f"potrf b={A.shape[0]}: forward error"


@pytest.mark.gpu
@pytest.mark.parametrize("b", [9, 33, 64])
def test_potrf_reports_non_positive_pivots(kp, b):
    rng = np.random.default_rng(b)
    for j in (0, b // 2, b - 1, "nan"):
        A = _spd(rng, b)
        if j == "nan":
            A[b // 3, b // 3] = np.nan
        else:
            L = np.linalg.cholesky(A)
            A[j, j] -= 2 * L[j, j] ** 2          # the pivot of column j becomes -L_jj^2
        _, info = _potrf_launch(kp, [A])
        assert info & 1, f"b={b} bad column {j}"


def _getrf_input(rng, b, tol, eps):
    """a block whose pivot decisions have relative margins >= 1e-8 (regenerated until they do)"""
    for _ in range(50):
        s = kr.scalings(rng, b, 1e-2, 1e2)
        A = s[:, None] * rng.uniform(-1, 1, (b, b))
        if tol == 0:
            A += np.diag(2 * b * s)
        if eps > 0 and b > 2:
            A[b // 2, :] = 2 * A[b // 2 - 1, :]   # rank-deficient: the two rows stay exact multiples, one reduces to exact zeros
        pos, L, Uu, npert, margin = kr.getrf_rule(A, tol, eps)
        if margin >= 1e-8:
            return A, pos, L, Uu, npert
    pytest.fail("no input with clear pivot decisions")


@pytest.mark.gpu
@pytest.mark.parametrize("tol,eps", [(0.0, 0.0), (0.0, 1e-8), (0.1, 0.0), (1.0, 0.0), (0.1, 1e-8), (1.0, 1e-8)])
def test_getrf_blocks(kp, tol, eps):
    rng = np.random.default_rng(int(tol * 10) + (eps > 0))
    ar = kr.Arena()
    cases = []
    for bi, b in enumerate(BLOCKS):
        A, pos, L, Uu, npert = _getrf_input(rng, b, tol, eps)
        ld, diag = b + 5, 3
        off = ar.alloc(ld * (b + diag), skew=1)
        cases.append((A, pos, L, Uu, npert, b, ld, diag, off, 100 * bi))
    u_shift = ar.size + 7
    ar.size = u_shift + ar.size + kr.GUARD                    # the U^T panels at the same offsets + u_shift
    a = ar.image()
    written = np.zeros(len(a), dtype=bool)
    tasks = []
    for A, pos, L, Uu, npert, b, ld, diag, off, fc in cases:
        r, c = np.nonzero(np.ones((b, b), dtype=bool))
        lower = c < r
        iL = off + diag + r[lower] + (diag + c[lower]) * ld             # PL(diag + r, diag + c), c < r
        iU = off + u_shift + diag + c[~lower] + (diag + r[~lower]) * ld  # PU(diag + c, diag + r), c >= r
        a[iL] = A[r[lower], c[lower]]
        a[iU] = A[r[~lower], c[~lower]]
        written[iL] = written[iU] = True
        tasks.append((off, ld, diag, b, fc))
    tasks = np.array(tasks, dtype=POTRF_TASK)
    before = a.copy()
    npiv = 100 * len(BLOCKS) + 200
    pivpos = np.full(npiv, -5, dtype=np.int32) if tol > 0 else None
    pivinv = np.full(npiv, -5, dtype=np.int32) if tol > 0 else None
    info = np.zeros(1, dtype=np.int32)
    nper = np.zeros(1, dtype=np.int32)
    _ok(kp.kp_getrf(P(a), len(a), P(tasks), len(tasks), u_shift, P(info), tol, eps, P(pivpos), P(pivinv), npiv, P(nper)))
    assert info[0] == 0
    kr.assert_unchanged(before, a, written, "k_getrf_block")
    want_np = 0
    for A, pos, L, Uu, npert, b, ld, diag, off, fc in cases:
        want_np += len(npert)
        g0 = fc + diag
        if tol > 0:
            assert np.array_equal(pivpos[g0:g0 + b], g0 + pos), f"b={b}: pivpos"
            assert np.array_equal(pivinv[g0 + pos], g0 + np.arange(b)), f"b={b}: pivinv"
        F = np.empty((b, b))
        for R in range(b):                    # stored by position R
            for c in range(b):
                F[R, c] = a[off + diag + R + (diag + c) * ld] if c < R else a[off + u_shift + diag + c + (diag + R) * ld]
        Lh = np.tril(F, -1) + np.eye(b)
        Uh = np.triu(F)
        PA = np.empty_like(A)
        PA[pos] = A
        res = np.abs(PA.astype(kr.LD) - kr.matmul_ld(Lh, Uh))
        bound = kr.SAFETY * (b + 2) * kr.U * kr.matmul_ld(np.abs(Lh), np.abs(Uh))
        for j in npert:                       # a replaced pivot: the factorization is of PA + E, E at (j, j) in pivot order
            res[j, j] = 0
        assert np.all(np.isfinite(F)) and np.all(res <= bound), f"getrf b={b} tol={tol} eps={eps}: |PA - LU| beyond the bound"
    assert nper[0] == want_np
    assert want_np > 0 or eps == 0


@pytest.mark.gpu
def test_getrf_threshold_tie(kp):
    """|a_jj| == tol * max exactly (powers of two): the natural row keeps the pivot (the rule is >=, sf_kernels.h)"""
    rng = np.random.default_rng(4)
    b, tol = 16, 0.5
    A = rng.uniform(-0.25, 0.25, (b, b)) + np.diag(np.full(b, 4.0))
    A[0, 0], A[5, 0] = 1.0, -2.0
    pos, _, _, _, _ = kr.getrf_rule(A, tol, 0.0)
    assert pos[0] == 0
    ld, diag, fc = b + 1, 0, 0
    ar = kr.Arena()
    off = ar.alloc(ld * b)
    u_shift = ar.size
    ar.size = 2 * ar.size + kr.GUARD
    a = ar.image()
    r, c = np.nonzero(np.ones((b, b), dtype=bool))
    lo = c < r
    a[off + r[lo] + c[lo] * ld] = A[r[lo], c[lo]]
    a[off + u_shift + c[~lo] + r[~lo] * ld] = A[r[~lo], c[~lo]]
    tasks = np.array([(off, ld, diag, b, fc)], dtype=POTRF_TASK)
    pivpos, pivinv = np.full(b, -1, dtype=np.int32), np.full(b, -1, dtype=np.int32)
    info, nper = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    _ok(kp.kp_getrf(P(a), len(a), P(tasks), 1, u_shift, P(info), tol, 0.0, P(pivpos), P(pivinv), b, P(nper)))
    assert info[0] == 0
    assert np.array_equal(pivpos, pos), (pivpos, pos)


def _trsm_case(rng, ar, b, nrows, unit):
    ld = nrows + b + 9
    diag, row0 = 1, b + 4
    off = ar.alloc(ld * (diag + b + 1), skew=1)
    s = kr.scalings(rng, nrows)
    D = np.tril(rng.uniform(-1, 1, (b, b))) + np.diag(rng.uniform(1, 2, b) * rng.choice([-1, 1], b))
    if unit:
        D[np.diag_indices(b)] = 1.0
    B = s[:, None] * rng.uniform(-1, 1, (nrows, b))
    return dict(b=b, nrows=nrows, unit=unit, ld=ld, diag=diag, row0=row0, off=off, D=D, B=B)


def _trsm_fill(a, written, t, first_col, perm=None):
    b, ld, diag, off, row0, nrows = t["b"], t["ld"], t["diag"], t["off"], t["row0"], t["nrows"]
    r, c = np.tril_indices(b, 0 if not t["unit"] else -1)
    a[off + diag + r + (diag + c) * ld] = t["D"][r, c]       # upper triangle (and a unit diagonal) stay NaN
    rr, cc = np.nonzero(np.ones((nrows, b), dtype=bool))
    idx = off + row0 + rr + (diag + cc) * ld
    a[idx] = t["B"][rr, cc]
    written[idx] = True
    t["idx"] = idx.reshape(nrows, b)
    return (off, off, ld, diag, b, row0, nrows, t["unit"], first_col, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("pivot", [False, True])
def test_trsm_blocks(kp, pivot):
    rng = np.random.default_rng(17 + pivot)
    ar = kr.Arena()
    cases, k = [], 0
    for b in BLOCKS:
        for nrows in (1, 63, 64, 65, 255, 256):
            if (b + nrows) % 3 and b not in (1, 64):        # a spread of the (b, nrows) grid
                continue
            unit = 1 if pivot else k % 2
            cases.append(_trsm_case(rng, ar, b, nrows, unit))
            k += 1
    a = ar.image()
    written = np.zeros(len(a), dtype=bool)
    npiv = 100 * len(cases) + 100
    pivinv = np.arange(npiv, dtype=np.int32) if pivot else None
    tasks = []
    for i, t in enumerate(cases):
        fc = 100 * i
        tasks.append(_trsm_fill(a, written, t, fc))
        if pivot:
            g0 = fc + t["diag"]
            t["perm"] = rng.permutation(t["b"])
            pivinv[g0:g0 + t["b"]] = g0 + t["perm"]
    tasks = np.array(tasks, dtype=TRSM_TASK)
    before = a.copy()
    _ok(kp.kp_trsm(P(a), len(a), P(tasks), len(tasks), P(pivinv), npiv))
    kr.assert_unchanged(before, a, written, "k_trsm_block")
    for t in cases:
        b = t["b"]
        Xh = a[t["idx"]]
        B = t["B"][:, t["perm"]] if pivot else t["B"]
        D = t["D"].astype(kr.LD)
        assert np.all(np.isfinite(Xh)), f"trsm b={b} nrows={t['nrows']}: non-finite"
        res = np.abs(kr.matmul_ld(Xh, D.T) - B.astype(kr.LD))
        bound = kr.SAFETY * (b + 2) * kr.U * kr.matmul_ld(np.abs(Xh), np.abs(D.T))
        assert np.all(res <= bound), f"trsm b={b} nrows={t['nrows']} unit={t['unit']} pivot={pivot}: |X D^T - B| beyond the bound"


# ---------------------------------------------------------------------------------------------------------------------
# k_step<false>: the fused 64-column steps of one outer block (Cholesky)
# ---------------------------------------------------------------------------------------------------------------------
NB, OUTER_NB, ST_ROWS = 64, 512, 64
STEP_PANELS = [(1, 0), (17, 1), (64, 63), (65, 64), (130, 65), (512, 300), (100, 300)]     # (nscol, nsrow - nscol)


def _chol_step_launches(panels, J=0):
    """the task list of every fused step of the outer block [J, J + 512), one launch per step, as sf_plan_build.hip builds
    them for Cholesky (the block_fused branch of the panel schedule): the diagonal tasks first (their own J = diag, slot =
    index in the launch, a fresh flag each), then the 64-row tiles below each diagonal block, with next_b = the width of
    the future diagonal block of this outer block that the tile's rows are (0: rows below the block's columns)"""
    launches, nflags = [], 0
    for ti in range(OUTER_NB // NB):
        diag = J + ti * NB
        tasks, flag_of, slot_of = [], [], []
        for off, nscol, nsrow in panels:
            if diag >= nscol:
                flag_of.append(-1)
                slot_of.append(-1)
                continue
            b = min(NB, nscol - diag)
            flag_of.append(nflags)
            tasks.append((off, off, nsrow, diag, diag, b, diag, b, nflags, 0, len(tasks), 0, 0, 0))
            slot_of.append(len(tasks) - 1)
            nflags += 1
        for (off, nscol, nsrow), fl, sl in zip(panels, flag_of, slot_of):
            if fl < 0:
                continue
            b = min(NB, nscol - diag)
            for r in range(diag + b, nsrow, ST_ROWS):
                nr = min(ST_ROWS, nsrow - r)
                nb = min(NB, nscol - r) if r < min(nscol, J + OUTER_NB) else 0
                tasks.append((off, off, nsrow, J, diag, b, r, nr, fl, 0, sl, nb, 0, 0))
        if tasks:
            launches.append((np.array(tasks, dtype=STEP_TASK), len(slot_of) - slot_of.count(-1)))
    return launches, nflags


def _chol_step_case(rng, shapes, bad_col=None):
    ar = kr.Arena()
    panels = []
    for nscol, extra in shapes:
        nsrow = nscol + extra
        panels.append((ar.alloc(nsrow * nscol, skew=1), nscol, nsrow))
    a = ar.image()
    mats, upper = [], np.zeros(len(a), dtype=bool)
    for k, (off, nscol, nsrow) in enumerate(panels):
        s = kr.scalings(rng, nsrow, 1e-3, 1e3)
        Z = rng.uniform(-1, 1, (nsrow, nscol))
        B = Z @ Z[:nscol].T
        B[:nscol] += np.diag(np.full(nscol, float(nscol)))
        A = s[:, None] * B * s[None, :nscol]
        if bad_col is not None and k == len(panels) - 1:
            L = np.linalg.cholesky(A[:nscol])
            A[bad_col, bad_col] -= 2 * L[bad_col, bad_col] ** 2
        v = a[off:off + nsrow * nscol].reshape(nscol, nsrow).T        # [row][col], column-major panel
        r, c = np.nonzero(np.tril(np.ones((nsrow, nscol), dtype=bool)))
        v[r, c] = A[r, c]
        ru, cu = np.nonzero(np.triu(np.ones((nscol, nscol), dtype=bool), 1))
        # the diagonal block's upper triangle: finite garbage (not NaN, so that a product with an explicit zero cannot hide a
        # read that is then selected away -- only its use or a store there is an error); it must stay bit-identical
        v[ru, cu] = rng.uniform(-1e3, 1e3, len(ru))
        mats.append(A)
    return panels, mats, a


def _run_steps(kp, a, launches, nflags, flags, epoch):
    info = np.zeros(1, dtype=np.int32)
    for tasks, ndiag in launches:
        _ok(kp.kp_step(P(a), len(a), P(tasks), len(tasks), 0, P(flags), nflags, epoch, P(info), 1024 * ndiag, 0.0, 0.0,
                       None, None, 0, None))
    return int(info[0])


def _check_chol_panels(before, a, panels, mats, what):
    written = np.zeros(len(a), dtype=bool)
    for (off, nscol, nsrow), A in zip(panels, mats):
        idx = off + np.arange(nsrow * nscol).reshape(nscol, nsrow).T
        low = np.tril(np.ones((nsrow, nscol), dtype=bool))
        written[idx[low]] = True
        Lh = np.where(low, a[idx], 0.0)
        assert np.all(np.isfinite(Lh)), f"{what} nscol={nscol} nsrow={nsrow}: non-finite factor entries"
        res = np.abs(A.astype(kr.LD) - kr.matmul_ld(Lh, Lh[:nscol].T))
        bound = kr.SAFETY * (nscol + 2) * kr.U * kr.matmul_ld(np.abs(Lh), np.abs(Lh[:nscol]).T)
        viol = low & (res > bound)
        assert not viol.any(), f"{what} nscol={nscol} nsrow={nsrow}: |A - L L^T| beyond the bound at {np.argwhere(viol)[:4].tolist()}"
    kr.assert_unchanged(before, a, written, what)


@pytest.mark.gpu
def test_step_cholesky_outer_block(kp):
    """all eight fused steps of one outer block over panels of different shapes, then a refactorization with epoch + 1 on
    the same flags"""
    rng = np.random.default_rng(21)
    panels, mats, a = _chol_step_case(rng, STEP_PANELS)
    launches, nflags = _chol_step_launches(panels)
    flags = np.zeros(nflags, dtype=np.int32)
    before = a.copy()
    assert _run_steps(kp, a, launches, nflags, flags, 1) == 0
    assert np.all(flags == 1)
    _check_chol_panels(before, a, panels, mats, "k_step")
    panels2, mats2, a2 = _chol_step_case(np.random.default_rng(22), STEP_PANELS)
    assert panels2 == panels
    before2 = a2.copy()
    assert _run_steps(kp, a2, launches, nflags, flags, 2) == 0
    assert np.all(flags == 2)
    _check_chol_panels(before2, a2, panels, mats2, "k_step refactorization (epoch 2)")


@pytest.mark.gpu
@pytest.mark.parametrize("bad_col", [0, 70, 129])
def test_step_cholesky_not_positive_definite(kp, bad_col):
    rng = np.random.default_rng(bad_col)
    panels, mats, a = _chol_step_case(rng, [(64, 10), (130, 65)], bad_col=bad_col)
    launches, nflags = _chol_step_launches(panels)
    flags = np.zeros(nflags, dtype=np.int32)
    info = _run_steps(kp, a, launches, nflags, flags, 1)
    assert info & 1 and not info & 2, info        # bit 0: a pivot <= 0; bit 1 (a wait ran out) must not be set


# ---------------------------------------------------------------------------------------------------------------------
# the load kernels against a numpy scatter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("skip_diag", [0, 1])
def test_load_kernels(kp, skip_diag):
    sym = _symbolic(9)
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    i64 = lambda x: np.ascontiguousarray(x, dtype=np.int64)
    n, ns = int(sym.n), int(sym.nsuper)
    Lp, Li, Super, SuperMap, Lsip, Lsi, Lsxp = i64(sym.Lp), i32(sym.Li), i32(sym.Super), i32(sym.SuperMap), i64(sym.Lsip), i32(sym.Lsi), i64(sym.Lsxp)
    rng = np.random.default_rng(2)
    Lx = rng.uniform(-1, 1, len(Li))
    base = kr.GUARD + 1
    want = np.full(len(Li), -1, dtype=np.int64)
    for j in range(n):
        s = SuperMap[j]
        c0, c1 = Super[s], Super[s + 1]
        nsrow, nscol = Lsip[s + 1] - Lsip[s], c1 - c0
        rows = Lsi[Lsip[s]:Lsip[s + 1]]
        for p in range(Lp[j], Lp[j + 1]):
            i = Li[p]
            if skip_diag and i == j:
                continue
            want[p] = base + Lsxp[s] + (j - c0) * nsrow + int(np.searchsorted(rows, i))
    m = np.full(len(Li), -9, dtype=np.int64)
    _ok(kp.kp_build_loadmap(P(Lp), P(Li), n, P(Super), P(SuperMap), ns, P(Lsip), P(Lsi), P(Lsxp), base, skip_diag, P(m)))
    assert np.array_equal(m, want), "k_build_loadmap"
    size = base + int(Lsxp[-1]) + kr.GUARD
    arena = np.full(size, np.nan)
    arena[base:base + int(Lsxp[-1])] = 0.0
    exp = arena.copy()
    exp[want[want >= 0]] = Lx[want >= 0]
    a = arena.copy()
    _ok(kp.kp_load_mapped(P(a), len(a), P(Lx), P(m), len(Li)))
    assert np.array_equal(kr.bits(a), kr.bits(exp)), "k_load_mapped"
    # the searching kernel: offsets relative to the arena start (panel offsets shifted by base), a mask over supernodes
    mask = (rng.uniform(size=ns) < 0.6).astype(np.int8)
    sel = (want >= 0) & (mask[SuperMap[np.searchsorted(Lp, np.arange(len(Li)), side="right") - 1]] != 0)
    exp = arena.copy()
    exp[want[sel]] = Lx[sel]
    a = arena.copy()
    _ok(kp.kp_load_panels(P(a), len(a), P(Lp), P(Li), P(Lx), n, P(Super), P(SuperMap), ns, P(Lsip), P(Lsi), P(Lsxp + base),
                          skip_diag, P(mask)))
    assert np.array_equal(kr.bits(a), kr.bits(exp)), "k_load_panels"


# ---------------------------------------------------------------------------------------------------------------------
# the device solve (csrc/sf_solve.hip): one launch = one step of a sweep, the diagonal tasks and their row tiles together,
# so the hand-off inside the launch is part of what is checked.  Every supernode of a case is one panel whose step is its
# last column block (columns [diag, diag + b) of diag + b); the rows below it gather / scatter through Lsi into a tail of x
# that the panels share (their atomics meet there).  What the launch may not read holds NaN: the arena outside the
# triangle and the rows below, x outside the blocks and the gathered rows.
# Checked as equations on the stored results, every sum formed in longdouble from the operands the kernel had
# (kernel_ref.assert_equations: SAFETY u (number of terms) (sum of |terms|) per element; the tiles add with fp64 atomics in no
# fixed order, so nothing is compared bit for bit).  The diagonal solves are checked by their residual, as test_trsm_blocks
# checks X D^T = B, not by the distance to a longdouble solution: a bound of that form holds for the residual of a substitution
# whatever the triangle's condition, and for the solution itself only with the condition number as a factor.
#   forward  diagonal: sum_k M(i, k) y_k = x_i           M = the block as the sweep sees it (unit diagonal, pivot order)
#            rows    : x'_g = x_g - sum over the panels and k of L(r, k) y_k
#   backward         : sum_{c >= k} D(c, k) y_c + sum_r L(r, k) x_g(r) = x_k
# ---------------------------------------------------------------------------------------------------------------------
SV_ROWS, SVM_W = 64, 16
SOLVE_B = [1, 63, 64, 65, 200, 256]
SOLVE_BELOW = [0, 1, 64, 65]
SOLVE_FAR = 130                 # rows of a far tile: ONE task of three row groups (64, 64, 2)
SOLVE_TAIL = 200
SOLVE_NARROW = [(1, 100, False), (37, 0, False), (64, 1, False), (37, 64, False), (64, 100, False)]      # five tasks: two workgroups
SOLVE_NAN_COL = 5


def _solve_shapes(big):
    """(b, rows below, far) of a general launch.  The <false> instantiations have no barrier between the 64-column sub-blocks, so
    a DIAGONAL task of b > 64 is outside their contract: a step with such a panel is launched with big = 1 (sf_plan_build.hip:
    big |= b > NB; the forward launch and the fused backward launch hold the step's diagonal tasks and tiles together), and only
    big steps carry far tiles.  The one way <false> meets b > 64 is the two-launch backward form, whose first launch holds the row
    tiles alone: test_solve_bwd_tiles_alone."""
    shapes = [(b, below, False) for b in SOLVE_B if big or b <= NB for below in SOLVE_BELOW]
    if big:
        shapes += [(65, SOLVE_FAR, True), (256, SOLVE_FAR, True)]
    return shapes


def _solve_case(rng, shapes, width, narrow=False, pivot=False, nan_col=None):
    ar = kr.Arena()
    panels, lsi, col = [], [], 0
    for i, (b, below, far) in enumerate(shapes):
        diag = 0 if narrow else 1 + i % 3
        nscol, nsrow = diag + b, diag + b + below
        ld = nsrow if narrow else nsrow + 5             # the narrow kernels take ld = nsrow as the row count
        # (off-diagonal entries ~ 1 / sqrt(b): a random triangle's substitution otherwise grows exponentially with b)
        D = np.tril(rng.uniform(-1, 1, (b, b)), -1) * (2 / np.sqrt(b)) + np.diag(rng.uniform(1, 2, b) * rng.choice([-1, 1], b))
        Lb = kr.scalings(rng, below)[:, None] * rng.uniform(-1, 1, (below, b))
        pos = np.arange(b)
        if pivot:
            for s in range(0, b, NB):
                pos[s:s + NB] = s + rng.permutation(min(NB, b - s))
        panels.append(dict(b=b, below=below, far=far, diag=diag, nscol=nscol, nsrow=nsrow, ld=ld, off=ar.alloc(ld * nscol, skew=i % 2),
                           first_col=col, blk=slice(col + diag, col + nscol), D=D, Lb=Lb, pos=pos))
        col += nscol
    nx = col + SOLVE_TAIL
    x = np.full((nx, width), np.nan)
    pivpos = np.arange(nx, dtype=np.int32)
    for p in panels:
        p["gi"] = col + np.sort(rng.choice(SOLVE_TAIL, p["below"], replace=False))
        p["rows"] = len(lsi)
        lsi += list(range(p["first_col"], p["first_col"] + p["nscol"])) + p["gi"].tolist()
        x[p["blk"]] = kr.scalings(rng, p["b"])[:, None] * rng.uniform(-1, 1, (p["b"], width))
        pivpos[p["blk"]] = p["blk"].start + p["pos"]
    used = np.unique(np.concatenate([p["gi"] for p in panels]))
    x[used] = kr.scalings(rng, len(used))[:, None] * rng.uniform(-1, 1, (len(used), width))
    cols = np.arange(width)
    if nan_col is not None:
        x[:, nan_col] = np.nan
        cols = cols[cols != nan_col]
    return types.SimpleNamespace(ar=ar, panels=panels, lsi=np.array(lsi, dtype=np.int32), x=x, nx=nx, pivpos=pivpos, cols=cols)


def _solve_arena(case, unit):
    a = case.ar.image()
    for p in case.panels:
        b, ld, diag, off = p["b"], p["ld"], p["diag"], p["off"]
        r, c = np.tril_indices(b, -1 if unit else 0)            # the upper triangle (and a unit diagonal) stay NaN
        a[off + diag + r + (diag + c) * ld] = p["D"][r, c]
        rr, cc = np.indices((p["below"], b))
        a[off + p["nscol"] + rr + (diag + cc) * ld] = p["Lb"]
    return a


def _solve_tasks(case, backward, narrow=False, tdiag=False, tiles_only=False):
    """the launch's task list as the plan orders it (producers first) and the size of the row-major copies' scratch"""
    dg, tiles, nT = [], [], 0
    for i, p in enumerate(case.panels):
        if narrow:
            dg.append((p["off"], p["rows"], p["nsrow"], 0, p["b"], 0, 0, p["first_col"], 0, 0, 0))
            continue
        head = (p["off"], p["rows"], p["ld"], p["diag"], p["b"])
        flag = 2 * i + backward         # sync words of a (panel, step): [flag] forward "solved", [flag + 1] backward tile counter
        rows = p["below"] if p["far"] else SV_ROWS
        mine = [head + (p["nscol"] + r, min(rows, p["below"] - r), p["first_col"], flag, 0, 0) for r in range(0, p["below"], rows)]
        td = 0
        if tdiag and i % 2 == 0:        # every other panel: both address forms in one launch
            td, nT = 1 + nT, nT + p["b"] * p["b"]
        dg.append(head + (0, 0, p["first_col"], flag, len(mine), td))
        tiles += mine
    if tiles_only:
        dg = []
    return np.array(tiles + dg if backward else dg + tiles, dtype=SOLVE_TASK), nT


def _solve_run(kp, case, a, tasks, backward, width, big, small, unit=0, pivot=False, nT=0):
    x, before, info = case.x.copy(), a.copy(), np.full(1, -1, dtype=np.int32)
    nsync = 2 * len(case.panels) + 1
    if backward:
        _ok(kp.kp_solve_bwd(P(a), len(a), P(case.lsi), len(case.lsi), P(x), case.nx, P(tasks), len(tasks), width, big, small, nT, nsync,
                            P(info)))
    else:
        _ok(kp.kp_solve_fwd(P(a), len(a), P(case.lsi), len(case.lsi), P(x), case.nx, P(tasks), len(tasks), width, big, small, unit,
                            P(case.pivpos) if pivot else None, case.nx, nsync, P(info)))
    assert info[0] == 0, info
    assert np.array_equal(kr.bits(before), kr.bits(a)), "the factor arena changed"
    return x


def _solve_check_fwd(case, x1, unit, what):
    x0 = case.x
    written = np.zeros(x0.shape, dtype=bool)
    tail, mag, cnt = x0.astype(kr.LD), np.abs(x0).astype(kr.LD), np.zeros(case.nx, dtype=np.int64)
    for p in case.panels:
        b, yh = p["b"], x1[p["blk"]]
        S = np.tril(p["D"], -1) + np.eye(b) if unit else p["D"]
        M = S.copy()
        for s in range(0, b, NB):       # row l of a sub-block meets the diagonal block's row pos[l]; left of it, its own
            M[s:s + NB, s:s + NB] = S[p["pos"][s:s + NB], s:s + NB]
        kr.assert_equations(kr.matmul_ld(M, yh), x0[p["blk"]], (M != 0).sum(1), kr.matmul_ld(np.abs(M), np.abs(yh)), case.cols,
                            f"{what} diagonal b={b}")
        written[p["blk"]] = True
        written[p["gi"]] = True
        tail[p["gi"]] -= kr.matmul_ld(p["Lb"], yh)
        mag[p["gi"]] += kr.matmul_ld(np.abs(p["Lb"]), np.abs(yh))
        cnt[p["gi"]] += b
    g = np.flatnonzero(cnt)
    kr.assert_equations(x1[g], tail[g], cnt[g] + 1, mag[g], case.cols, f"{what} rows below")      # the products and x_g itself
    kr.assert_unchanged(x0, x1, written, what)


def _solve_check_bwd(case, x1, what):
    x0 = case.x
    written = np.zeros(x0.shape, dtype=bool)
    for p in case.panels:
        b, yh, xr, D, Lb = p["b"], x1[p["blk"]], x0[p["gi"]], p["D"], p["Lb"]
        kr.assert_equations(kr.matmul_ld(D.T, yh) + kr.matmul_ld(Lb.T, xr), x0[p["blk"]], b - np.arange(b) + p["below"],
                            kr.matmul_ld(np.abs(D.T), np.abs(yh)) + kr.matmul_ld(np.abs(Lb.T), np.abs(xr)), case.cols,
                            f"{what} b={b} below={p['below']}")
        written[p["blk"]] = True
    kr.assert_unchanged(x0, x1, written, what)


def _tsolve_run(kp, case, a, tasks, width, big, small, pivpos=None, nT=0):
    """one transposed backward launch (csrc/sf_solve_t.hip) on the L panels of `a`; pivpos: the interchange record, or None"""
    x, before, info = case.x.copy(), a.copy(), np.full(1, -1, dtype=np.int32)
    nsync = 2 * len(case.panels) + 1
    _ok(kp.kp_tsolve_bwd(P(a), len(a), P(case.lsi), len(case.lsi), P(x), case.nx, P(tasks), len(tasks), width, big, small, P(pivpos), case.nx,
                         nT, nsync, P(info)))
    assert info[0] == 0, info
    assert np.array_equal(kr.bits(before), kr.bits(a)), "the factor arena changed"
    return x


def _tsolve_check_bwd(case, x1, what):
    """The transposed backward launch is the adjoint of the forward launch with unit = 1 and the same interchanges: with M as
    _solve_check_fwd builds it (kernel_ref.tsolve_matrix) and z the stored x1[blk], column by column
        M^T z + Lb^T x0[gi] = x0[blk],   nterms = the nonzeros of M's column + the rows below,   mag = |M^T| |z| + |Lb^T| |x0[gi]|.
    Everything in x outside the blocks is bit-unchanged.  Returns the worst err / bound."""
    x0 = case.x
    written = np.zeros(x0.shape, dtype=bool)
    worst = 0.0
    for p in case.panels:
        b, z, xr, Lb = p["b"], x1[p["blk"]], x0[p["gi"]], p["Lb"]
        M = kr.tsolve_matrix(p["D"], p["pos"], NB)
        worst = max(worst, kr.assert_equations(kr.matmul_ld(M.T, z) + kr.matmul_ld(Lb.T, xr), x0[p["blk"]], (M != 0).sum(0) + p["below"],
                                               kr.matmul_ld(np.abs(M.T), np.abs(z)) + kr.matmul_ld(np.abs(Lb.T), np.abs(xr)), case.cols,
                                               f"{what} b={b} below={p['below']}"))
        written[p["blk"]] = True
    kr.assert_unchanged(x0, x1, written, what)
    return worst


def _solve_name(width, direction, big=None):
    return f"k_solve{'_many' if width > 1 else ''}" + (f"_small_{direction}" if big is None else f"_{direction}<{bool(big)}>")


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("width", [1, SVM_W])
def test_solve_fwd_step(kp, width, big, unit):
    case = _solve_case(np.random.default_rng(31 + 4 * big + unit), _solve_shapes(big), width)
    tasks, _ = _solve_tasks(case, 0)
    x1 = _solve_run(kp, case, _solve_arena(case, unit), tasks, 0, width, big, 0, unit=unit)
    _solve_check_fwd(case, x1, unit, f"{_solve_name(width, 'fwd', big)} unit={unit}")


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, SVM_W])
def test_solve_fwd_step_pivoting(kp, width):
    """LU with pivoting: x_blk is brought into pivot order sub-block by sub-block as the sweep reaches it"""
    case = _solve_case(np.random.default_rng(41), [(65, 65, False), (200, 64, False)], width, pivot=True)
    tasks, _ = _solve_tasks(case, 0)
    x1 = _solve_run(kp, case, _solve_arena(case, 1), tasks, 0, width, 1, 0, unit=1, pivot=True)
    _solve_check_fwd(case, x1, 1, f"{_solve_name(width, 'fwd', 1)} pivoting")


@pytest.mark.gpu
@pytest.mark.parametrize("tdiag", [False, True])
@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("width", [1, SVM_W])
def test_solve_bwd_step(kp, width, big, tdiag):
    case = _solve_case(np.random.default_rng(51 + 4 * big + tdiag), _solve_shapes(big), width)
    tasks, nT = _solve_tasks(case, 1, tdiag=tdiag)
    x1 = _solve_run(kp, case, _solve_arena(case, 0), tasks, 1, width, big, 0, nT=nT)
    _solve_check_bwd(case, x1, f"{_solve_name(width, 'bwd', big)} tdiag={tdiag}")


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, SVM_W])
def test_solve_bwd_tiles_alone(kp, width):
    """the two-launch backward form (solve_bwd_fused off) launches a step's row tiles alone with big = 0, whatever the step's
    width: <false> with b > 64, waves 1 - 3 at work.  x_blk' = x_blk - L^T x[rows]; nothing waits, the counters just count."""
    shapes = [(b, below, False) for b in (65, 200, 256) for below in (1, 64, 65)]
    case = _solve_case(np.random.default_rng(91), shapes, width)
    tasks, _ = _solve_tasks(case, 1, tiles_only=True)
    x1 = _solve_run(kp, case, _solve_arena(case, 0), tasks, 1, width, 0, 0)
    x0, what = case.x, f"{_solve_name(width, 'bwd', 0)} tiles alone"
    written = np.zeros(x0.shape, dtype=bool)
    for p in case.panels:
        xr, Lb = x0[p["gi"]], p["Lb"]
        kr.assert_equations(x1[p["blk"]], x0[p["blk"]].astype(kr.LD) - kr.matmul_ld(Lb.T, xr), np.full(p["b"], p["below"] + 1),
                            np.abs(x0[p["blk"]]) + kr.matmul_ld(np.abs(Lb.T), np.abs(xr)), case.cols, f"{what} b={p['b']} below={p['below']}")
        written[p["blk"]] = True
    kr.assert_unchanged(x0, x1, written, what)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["unit0", "unit1", "pivoting"])
@pytest.mark.parametrize("width", [1, SVM_W])
def test_solve_small_fwd(kp, width, mode):
    unit, pivot = int(mode != "unit0"), mode == "pivoting"
    case = _solve_case(np.random.default_rng(61 + unit), SOLVE_NARROW, width, narrow=True, pivot=pivot)
    tasks, _ = _solve_tasks(case, 0, narrow=True)
    x1 = _solve_run(kp, case, _solve_arena(case, unit), tasks, 0, width, 0, 1, unit=unit, pivot=pivot)
    _solve_check_fwd(case, x1, unit, f"{_solve_name(width, 'fwd')} {mode}")


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, SVM_W])
def test_solve_small_bwd(kp, width):
    case = _solve_case(np.random.default_rng(71), SOLVE_NARROW, width, narrow=True)
    tasks, _ = _solve_tasks(case, 1, narrow=True)
    x1 = _solve_run(kp, case, _solve_arena(case, 0), tasks, 1, width, 0, 1)
    _solve_check_bwd(case, x1, _solve_name(width, "bwd"))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["fwd", "bwd", "small_fwd", "small_bwd"])
def test_solve_many_columns_are_independent(kp, kernel):
    """one of the SVM_W right-hand sides is NaN throughout: every other column still meets its bound"""
    narrow, backward = kernel.startswith("small"), kernel.endswith("bwd")
    shapes = SOLVE_NARROW if narrow else [(64, 1, False), (65, 65, False), (256, SOLVE_FAR, True)]
    case = _solve_case(np.random.default_rng(81), shapes, SVM_W, narrow=narrow, nan_col=SOLVE_NAN_COL)
    tasks, nT = _solve_tasks(case, int(backward), narrow=narrow, tdiag=True)
    x1 = _solve_run(kp, case, _solve_arena(case, 0), tasks, int(backward), SVM_W, int(not narrow), int(narrow), nT=nT)
    if backward:
        _solve_check_bwd(case, x1, f"k_solve_many_{kernel} with a NaN column")
    else:
        _solve_check_fwd(case, x1, 0, f"k_solve_many_{kernel} with a NaN column")
