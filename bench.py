#!/usr/bin/env python3
"""bench.py -- numeric-factorization throughput of the MI355X-native supernodal Cholesky.

    python bench.py --gpus N --steps K --warmup W

N > 1 is one process per GPU.  Under a launcher (torch.distributed.run: WORLD_SIZE / RANK / LOCAL_RANK in the environment) this
process is one rank; WITHOUT one (no WORLD_SIZE) this process starts the N ranks itself (python -m torch.distributed.run
--nproc-per-node N bench.py ..., before anything touches the GPU) and relays rank 0's line.  WORLD_SIZE != N is an error, and the
line carries `ranks_seen` -- a sum of 1 over the communicator the factorization uses -- and exits non-zero unless it equals N:
a value can never come from fewer ranks than --gpus says.

Workload at N = 1 (BASELINE.json configs[1]): 3-D 7-point Laplacian 128^3, SPD, fp64, deterministic
geometric nested dissection, devSlotSize = the reference's formula for one 288 GiB device.
A "step" = one complete numeric factorization (assemble + every panel + every Schur update) with the
matrix values, the symbolic structure and the task tables already resident in HBM; the factor stays
in HBM.  value = F_struct * N / t  with  F_struct = sum_j ColCount_j^2  (SURVEY 8d).
N > 1 (default --mp subtree): ONE factorization sharded over the N GPUs by elimination-tree subtrees:
own subtrees on their GPU, then the top supernodes with their large GEMMs split over the ranks and every top panel
summed once over RCCL, block by block (sharded.py, mode "distributed").  --scale weak (default): the matrix rows per GPU
stay those of config 2 (n = N x 128^3: g = round(128 N^(1/3)) = 161, 203, 256 -- N = 8 IS BASELINE config 4, 256^3 over
8 GPUs); --scale weak-flops: the flops per GPU stay those of 128^3 (g = round(128 N^(1/6)): 144, 161, 181; also timed as
`secondary.weak_flops` in an N > 1 run with --full); --scale strong: the same 128^3 matrix on every N.  An explicit --grid is
used as given, whatever --scale says.  --mp subtree-replicated: top supernodes replicated, one all-reduce.
--mp replicas: one independent matrix per GPU (the reference's multi-matrix mode, SparseFrame.c:3375).

A plain run sets up, warms up, times the --steps steps and prints the headline line.  With --full the JSON line also carries
  roofline     : the Schur-update kernel (k_gemm<1>: fp64 MFMA GEMM + fused mapped scatter), executed
                 update flops / its summed launch time (HIP events on the plan's stream)
  cpu_baseline : the CPU oracle (a port of the reference's CPU path on OpenBLAS) on a bounded sample
and the device validate (config.residual_*), the host-buffer boundary (config.pcie_inclusive) and the other BASELINE
configs (secondary); --no-roofline / --no-pcie / --no-secondary / --cpu-grid trim what --full adds.

--dump-outputs DIR: after the timed steps, the factor of the last step (what get_factor() would hand a caller, reference
layout) as DIR/factor_sample.npy (float64): the whole factor when it holds at most DUMP_BLOCKS x DUMP_BLOCK entries,
otherwise DUMP_BLOCKS blocks of DUMP_BLOCK consecutive entries at seeded random block-aligned places, whose first indices
are DIR/factor_sample_offsets.npy (float64, exact).  The inputs are generated deterministically, so two builds run with the
same arguments can be compared output for output.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
T_PROCESS_START = time.time()

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X datasheet fp64 matrix; v_mfma_f64_16x16x4_f64 = 2048 flop / 64 cyc / SIMD


HBM_PEAK_GBS = 8000.0          # MI355X HBM3E peak (guide: 8 TB/s spec, ~6.3 TB/s achievable)

DUMP_BLOCK = 1024              # --dump-outputs: consecutive factor entries per sampled block
DUMP_BLOCKS = 4096             # blocks per sample: 32 MiB of float64 (+ 32 KiB of offsets)
DUMP_SEED = 20240611


def dump_factor(out_dir, xsize, read):
    """--dump-outputs: the factor (xsize doubles, reference layout) or a seeded block sample of it; read(b, e) returns
    entries [b, e) as float64"""
    import numpy as np
    nblk = xsize // DUMP_BLOCK
    if nblk <= DUMP_BLOCKS:
        starts = np.zeros(1, dtype=np.int64)
        sample = read(0, xsize)
    else:
        starts = np.sort(np.random.default_rng(DUMP_SEED).choice(nblk, DUMP_BLOCKS, replace=False)).astype(np.int64) * DUMP_BLOCK
        sample = np.concatenate([read(int(b), int(b) + DUMP_BLOCK) for b in starts])
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "factor_sample.npy"), np.ascontiguousarray(sample, dtype=np.float64))
    np.save(os.path.join(out_dir, "factor_sample_offsets.npy"), starts.astype(np.float64))


def plan_factor_range(sf, plan):
    """read(b, e) over a whole plan's device factor (sf_chol_plan_get_factor_range: bounds-checked D2H, LU packed on the device)"""
    import ctypes as C
    import numpy as np

    def read(b, e):
        buf = np.empty(max(e - b, 1), dtype=np.float64)
        rc = sf.lib.sf_chol_plan_get_factor_range(plan._h, C.c_int64(b), C.c_int64(e), buf.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != 0:
            raise RuntimeError(f"sf_chol_plan_get_factor_range({b}, {e}) failed: {rc}")
        return buf[:e - b]
    return read


def config1_case(sf, np):
    """BASELINE config 1 -- the 2-D 5-point Laplacian 100 x 100 through the reference's own stage functions, as its demo runs it
    (SparseFrame_analyze with the default ordering, SparseFrame_factorize on the GPU, SparseFrame_validate = solve + residual):
    plumbing, not performance; the times of the second call (cached plan)"""
    n, Cp, Ci, Cx = sf.gen.laplacian_lower(100, 100)
    common = sf.CommonInfo()
    out = {"workload": "2D 5-point Laplacian 100x100 through the struct entry points (SparseFrame_analyze / _factorize / _validate), "
                       "built-in nested-dissection ordering", "n": n}
    for call in range(2):
        mi = sf.MatrixInfo()
        mi.set_csc(n, Cp, Ci, Cx)
        mi.analyze(common)
        mi.factorize(common)
        res = mi.validate()
        out.update({"analyze_ms": round(1e3 * mi.c.analyzeTime, 3), "factorize_ms": round(1e3 * mi.c.factorizeTime, 3),
                    "solve_ms": round(1e3 * mi.c.solveTime, 3), "residual": res, "nsuper": int(mi.c.nsuper)})
        mi.cleanup()
    common.close()
    return out


def end_to_end_case(sf, np, N=128):
    """what a user of the reference's stage functions waits for on the headline matrix, everything included except reading the file:
    SparseFrame_analyze with NO ordering supplied (the built-in nested dissection stands in for METIS, as in Demo/demo.c's flow,
    C:3396-3423), the FIRST SparseFrame_factorize of the pattern on a fresh handler list (plan build + first touch of Lsx +
    overlapped copy-back), SparseFrame_validate (solve on the resident factor behind the full fingerprint check + residual),
    SparseFrame_cleanup_matrix.  The built-in ordering gives a smaller factor than the geometric one the headline prescribes."""
    n, Cp, Ci, Cx = sf.gen.laplacian_lower(N, N, N)
    t0 = time.perf_counter()
    common = sf.CommonInfo()
    t1 = time.perf_counter()
    mi = sf.MatrixInfo()
    mi.set_csc(n, Cp, Ci, Cx)
    t2 = time.perf_counter()
    mi.analyze(common)
    t3 = time.perf_counter()
    mi.factorize(common)
    t4 = time.perf_counter()
    res = mi.validate()
    t5 = time.perf_counter()
    xsize = int(mi.c.xsize)
    solve_s = float(mi.c.solveTime)
    mi.cleanup()
    t6 = time.perf_counter()
    common.close()
    return {"workload": f"3D 7-point Laplacian {N}^3 through SparseFrame_analyze (built-in ordering) / _factorize (first call) / _validate / "
                        "_cleanup_matrix", "n": int(n), "factor_doubles": xsize,
            "allocate_gpu_s": round(t1 - t0, 3), "set_matrix_s": round(t2 - t1, 3), "analyze_s": round(t3 - t2, 3),
            "factorize_first_call_s": round(t4 - t3, 3), "validate_s": round(t5 - t4, 3), "solve_inside_validate_s": round(solve_s, 3),
            "cleanup_s": round(t6 - t5, 3), "end_to_end_s": round(t6 - t1, 3), "residual": res}


def half_log_det(np, sym, Lsx):
    """sum of the logarithms of the Cholesky factor's diagonal, from the factor in the reference layout"""
    sm, Sup, Xp = np.asarray(sym.SuperMap), np.asarray(sym.Super), np.asarray(sym.Lsxp)[:-1]
    nsrow = np.diff(sym.Lsip)
    return float(np.log(Lsx[Xp[sm] + (np.arange(sym.n) - Sup[sm]) * (nsrow[sm] + 1)]).sum())


def out_of_core_case(sf, np, sym, fraction=0.55, in_core_log_det=None, inputs=None):
    """the headline matrix with the device budget lowered to `fraction` of its factor: top panels resident, subtree
    groups streamed through two buffers, the factor leaves for pageable host memory as it is finished -- the same entry point and
    destination as pcie_inclusive.plan_second_call_ms, which is the in-core figure to compare with"""
    ent = np.diff(sym.Super) * np.diff(sym.Lsip)
    total = int(ent.sum())
    group, ng, ge, te, need, fits = sf.ooc_partition(sym, int(total * fraction))
    plan = sf.CholPlan(sym, ooc_group=group, ooc_ngroups=ng)
    host = np.empty(max(sym.xsize, 1), dtype=np.float64)
    ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        plan.factorize_to_host(sym.Lx, host)
        ms.append((time.perf_counter() - t0) * 1e3)
    dev = plan.stat("bytes_device")
    plan.close()
    # the factor only exists on the host.  The parity of the out-of-core path is tests/test_out_of_core.py (oracle, SparseFrame's own
    # validate); here: log det against the in-core run's
    ld = half_log_det(np, sym, host)
    del host
    # ... and the reference's entry points under the same budget: SparseFrame_factorize decides for the out-of-core plan by itself,
    # SparseFrame_validate solves on the host (nothing is resident; threaded sweeps over Lsx, csrc/sf_host_solve.h)
    struct = None
    if inputs:
        overhead = (384 << 20) + 12 * int(sym.Lp[-1]) + 24 * len(sym.Lsi)
        old_budget = os.environ.get("SF_DEVICE_BUDGET_MB")
        os.environ["SF_DEVICE_BUDGET_MB"] = str((overhead + int(fraction * 8 * total)) >> 20)
        try:
            common = sf.CommonInfo(dev_slot_size=sf.REFERENCE_SLOT_1GPU)
            mi = sf.MatrixInfo()
            mi.set_csc(inputs["n"], inputs["Cp"], inputs["Ci"], inputs["Cx"])
            mi.set_perm(inputs["perm"])
            mi.analyze(common)
            mi.factorize(common)
            res = mi.validate()
            struct = {"factorize_first_call_ms": round(1e3 * mi.c.factorizeTime, 1), "validate_residual": res,
                      "host_solve_ms": round(1e3 * mi.c.solveTime, 1)}
            mi.cleanup()
            common.close()
        finally:
            if old_budget is None:
                os.environ.pop("SF_DEVICE_BUDGET_MB", None)
            else:
                os.environ["SF_DEVICE_BUDGET_MB"] = old_budget
    return {"struct_entry_points": struct, "workload": f"the headline matrix, device budget {fraction} x factor", "groups": int(ng), "fits_budget": bool(fits),
            "factor_bytes": 8 * total, "device_bytes": int(dev), "top_bytes": 8 * int(te), "group_buffer_bytes": 8 * int(ge),
            "first_call_ms": round(ms[0], 1), "second_call_ms": round(ms[1], 1),
            "GFLOPs_struct_second_call": round(sym.flops_struct / (ms[1] * 1e-3) / 1e9, 1),
            "log_det_half": ld, "log_det_half_in_core": in_core_log_det,
            "log_det_rel_difference": (abs(ld - in_core_log_det) / abs(in_core_log_det)) if in_core_log_det else None}


def hbm_roofline_whole_factorization(plan, sym, ms):
    """HBM roofline of a whole (scatter-bound, config 3) factorization: algorithmic bytes = memset + loadA
    (16 nnz + 8 xsize) + every panel read and written once by its factorization (16 xsize) + read once as an update source
    (8 xsize) + the fused scatter (16 B per scattered element); traffic from the committed PMC passes of this workload."""
    E = plan.stat("scatter_elems")
    alg = 8.0 * sym.xsize + 16.0 * sym.nnz + 8.0 * sym.xsize + 16.0 * sym.xsize + 8.0 * sym.xsize + 16.0 * E
    gbs = alg / (ms * 1e-3) / 1e9
    traffic, src = None, None
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic_config3.json")))
    if files:
        with open(files[-1]) as f:
            pm = json.load(f)
        # the factorization's kernels only: the profiled run also solves (k_solve_*) and validates (k_resid_*)
        fk = [v for k, v in pm.items() if isinstance(v, dict) and "hbm_bytes_total" in v
              and not (k.startswith("k_solve") or k.startswith("k_resid"))]
        nf = max(int(pm.get("_total", {}).get("factorizations_in_the_run", 1)), 1)
        traffic = sum(v["hbm_bytes_total"] for v in fk) / nf if fk else pm.get("_total", {}).get("hbm_bytes_per_factorization")
        src = "committed rocprofv3 --pmc passes (factorization kernels; solve and residual kernels excluded): " + os.path.basename(files[-1])
    return {"bound": "hbm", "kernel": "whole factorization (level-scheduled: latency-bound, see DESIGN 5)",
            "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
            "algorithmic_bytes": alg, "scatter_elems": E, "traffic": traffic, "traffic_source": src}


def mfma_roofline_schur(plan, ms, lu=False):
    """roofline object of the Schur-update GEMM (k_gemm<1>) from the plan's event-profiled last factorization: algorithmic flops of the
    updates with K > 64 (LU: both sides, L:2570-2577) over the summed duration of that kernel's launches (HIP events on the plan's stream)"""
    upd_ms = plan.stat("last_update_ms")
    big = plan.stat("flops_update") - plan.stat("flops_update_small")
    ach = big / (upd_ms * 1e-3) / 1e12 if upd_ms > 0 else 0.0
    traffic, src = None, None
    if lu:          # HBM bytes per launch of that kernel from the committed PMC passes of config 5 (not measurable live)
        import glob
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic_lu_config5.json")))
        if files:
            with open(files[-1]) as f:
                traffic = json.load(f).get("k_gemm<1>", {}).get("hbm_bytes_per_launch")
            src = "committed rocprofv3 --pmc passes (profiles/), NOT measured in this run: " + os.path.basename(files[-1])
    return {"bound": "mfma", "kernel": "k_gemm<1> (Schur update, fused scatter%s)" % (", L and U^T sides" if lu else ""),
            "achieved": round(ach, 3), "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / FP64_MFMA_PEAK_TFLOPS, 4),
            "traffic": traffic, "traffic_source": src, "kernel_ms": round(upd_ms, 3), "algorithmic_flops": big,
            "whole_factorization_exec_TFLOPs": round(plan.stat("flops_exec") / (ms * 1e-3) / 1e12, 2),
            "whole_factorization_frac": round(plan.stat("flops_exec") / (ms * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS, 4)}


def secondary_case(sf, np, kind, steps=3):
    """one more BASELINE config timed in the same run (driver-side numbers for configs 3 and 5):
    kind 'config3' = 2-D 1000x1000 21-point random SPD stencil (the HBM-/latency-bound extend-add config),
    kind 'config5' = unsymmetric 19-point stencil 79^3, LU with threshold pivoting inside the diagonal blocks (diagonally dominant:
    the natural pivots pass), kind 'config5_pivoting' = the same matrix with a fifth of its diagonal weakened so that rows really
    are interchanged."""
    t0 = time.time()
    if kind == "config3":
        M = 1000
        n, Cp, Ci, Cx = sf.gen.stencil_spd_lower(M, M)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(M, M, 1, 3, 2), sf.REFERENCE_SLOT_1GPU)
        plan = sf.CholPlan(sym)
        plan.set_values(sym.Lx)
        wl = "2D 1000x1000 grid, 21-point random SPD stencil (rng 12345), n = 1M, Cholesky fp64, geometric ND with 2-line separators"
    else:
        M = 79
        n, Cp, Ci, Cx = sf.gen.unsymmetric_stencil(M, M, M, extra_per_row=0, seed=2024, drop=0.05)
        weak = kind == "config5_pivoting"
        if weak:
            n, Cp, Ci, Cx = sf.gen.weaken_diagonal(n, Cp, Ci, Cx, fraction=0.2, factor=0.02, seed=77)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(M, M, M, 3, 1), sf.REFERENCE_SLOT_1GPU, "lu", False)
        plan = sf.LUPlan(sym)
        plan.set_values(sym.Lx, sym.Ux)
        plan.set_pivoting(0.1)
        wl = ("unsymmetric 3D 19-point stencil 79^3 (5% of the entries dropped one-sidedly; SURVEY 8d's one random long-range entry "
              "per row is not used: the factor of that matrix is ~0.6 n^2 doubles under any ordering (profiles/r03_config5_rescope.txt: "
              "26x the stand-in's at 30^3, 1.2 TB at n = 493k)), "
              + ("20% of the diagonal entries multiplied by 0.02 (those rows are NOT diagonally dominant: the threshold test fails "
                 "there and rows are interchanged)" if weak else "diagonally dominant (every natural pivot passes the threshold)")
              + ", LU fp64 with threshold partial pivoting (tol 0.1) inside the 64x64 diagonal blocks")
    t_setup = time.time() - t0
    plan.factorize()
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.factorize(sync=False)
    plan.sync()
    ms = (time.perf_counter() - t0) / steps * 1e3
    plan.set_profiling(True)
    plan.factorize(sync=True)
    plan.set_profiling(False)
    F = sym.flops_struct
    out = {"workload": wl, "n": int(n), "nnz_input": int(len(Ci)), "nsuper": int(sym.nsuper), "factor_doubles": int(sym.xsize),
           "F_struct": F, "ms_per_step": round(ms, 3), "GFLOPs": round(F / (ms * 1e-3) / 1e9, 1), "steps": steps,
           "launches": int(plan.stat("launches")), "levels": int(plan.stat("levels")), "setup_s": round(t_setup, 2),
           "kernel_ms": {"schur_gemm": round(plan.stat("last_update_ms"), 3), "schur_small": round(plan.stat("last_small_update_ms"), 3),
                         "fused_step": round(plan.stat("last_step_ms"), 3), "outer_gemm": round(plan.stat("last_outer_gemm_ms"), 3),
                         "potrf": round(plan.stat("last_potrf_ms"), 3), "trsm": round(plan.stat("last_trsm_ms"), 3),
                         "load": round(plan.stat("last_load_ms"), 3)}}
    x = plan.solve(1 + np.arange(n) / n)
    out["device_solve_ms"] = round(plan.stat("last_solve_ms"), 3)
    if kind == "config3":
        out["residual_device_solve"] = plan.validate()          # solve + residual on the device
        out["residual_host_check"] = sf.validate_solution(sym, x)
        out["roofline"] = hbm_roofline_whole_factorization(plan, sym, ms)
    else:
        out["roofline"] = mfma_roofline_schur(plan, ms, lu=True)
        out["pivot_tol"] = plan.stat("pivot_tol")
        out["perturbed_pivots"] = int(plan.stat("perturbed_pivots"))
        out["rows_interchanged"] = int(np.count_nonzero(plan.get_pivots() != np.arange(n)))
        # residual of the device solve against the permuted matrix (numpy, reference validate formula L:3702-3858)
        lc = np.repeat(np.arange(n), np.diff(sym.Lp))
        r = -(1 + np.arange(n) / n)
        np.add.at(r, sym.Li, sym.Lx * x[lc])
        ur = np.repeat(np.arange(n), np.diff(sym.Up))
        off = sym.Ui != ur
        np.add.at(r, ur[off], sym.Ux[off] * x[sym.Ui[off]])
        colsum = np.zeros(n)
        np.add.at(colsum, lc, np.abs(sym.Lx))
        np.add.at(colsum, sym.Ui[off], np.abs(sym.Ux[off]))
        out["residual_host_check"] = float(np.abs(r).max() / (colsum.max() * np.abs(x).max() + np.abs(r * 0 + 1 + np.arange(n) / n).max()))
        out["residual_device_solve"] = plan.validate()          # solve + residual on the device
        if kind == "config5_pivoting":
            # two steps of iterative refinement on the host residual (what a perturbed or growth-affected factor calls for)
            import scipy.sparse as sp
            A = (sp.coo_matrix((sym.Lx, (sym.Li, lc)), shape=(n, n)) + sp.coo_matrix((sym.Ux[off], (ur[off], sym.Ui[off])), shape=(n, n))).tocsr()
            bvec = 1 + np.arange(n) / n
            xr = x
            for _ in range(2):
                xr = xr + plan.solve(bvec - A @ xr)
            rr = A @ xr - bvec
            out["residual_after_2_refinements"] = float(np.abs(rr).max() / (colsum.max() * np.abs(xr).max() + np.abs(bvec).max()))
    plan.close()
    return out


def self_launch(ngpu):
    """--gpus N > 1 with no launcher in the environment: start the N ranks as children (one process per GPU,
    torch.distributed.run on 127.0.0.1 with a free port) and leave with their exit code.  Runs before torch is imported:
    the parent never touches a GPU, rank 0's JSON line reaches stdout through the inherited descriptors."""
    import subprocess
    # --standalone: the launcher opens its own rendezvous on a free port of 127.0.0.1 (no port picked here and closed again before
    # the ranks bind it -- ADVICE r3: that was a race)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           f"--nproc-per-node={ngpu}", os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, SF_BENCH_SELF_LAUNCHED="1")
    sys.stderr.write(f"[bench.py] --gpus {ngpu} without a launcher: starting {ngpu} ranks: {' '.join(cmd)}\n")
    sys.stderr.flush()
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--grid", type=int, default=0, help="N of the N^3 grid (default: 128 for cholesky = BASELINE config 2, 79 for lu = config 5)")
    ap.add_argument("--method", choices=["cholesky", "lu"], default="cholesky",
                    help="cholesky: 3-D 7-pt Laplacian (the headline workload); lu: unsymmetric 19-pt stencil, no-pivot LU")
    ap.add_argument("--cpu-grid", type=int, default=-1,
                    help="N of the CPU-baseline sample (0 = skip; default: the benchmarked matrix itself up to 128 -- the headline 128^3 "
                         "takes the CPU path ~35 s -- and a 56^3 sample for LU)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="N = 1 default workload: skip the extra lines for BASELINE configs 3 and 5 (out['secondary'])")
    ap.add_argument("--cpu-threads", type=int, default=0, help="BLAS threads of the CPU baseline (0 = min(cores,16))")
    ap.add_argument("--workload", choices=["lap3d", "stencil2d"], default="lap3d",
                    help="cholesky only: lap3d = N^3 7-point Laplacian (config 2); stencil2d = N x N grid, 21-point random SPD "
                         "stencil, 2-line separators (BASELINE config 3 at N = 1000)")
    ap.add_argument("--mp", choices=["subtree", "subtree-replicated", "replicas"], default="subtree",
                    help="N > 1: shard one matrix by elimination-tree subtrees (default: distributed top; "
                         "subtree-replicated: replicated top) or run one matrix per GPU")
    ap.add_argument("--scale", choices=["weak", "weak-flops", "strong"], default="weak",
                    help="N > 1 with --mp subtree* and no explicit --grid: weak = grid round(base * N^(1/3)) (matrix rows per GPU fixed; "
                         "128 -> 256 at N = 8 = BASELINE config 4), weak-flops = round(base * N^(1/6)) (flops per GPU fixed), "
                         "strong = base grid")
    ap.add_argument("--check", action="store_true", help="download the factor and check the residual on the host")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-pcie", action="store_true",
                    help="N = 1: skip the host-buffer boundary lines (values H2D + factorize + overlapped factor D2H at plan level and "
                         "through the struct entry point SparseFrame_factorize), reported in config.pcie_inclusive; never `value`")
    ap.add_argument("--pcie", action="store_true", help="(default now; kept for compatibility)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure and check everything else: roofline, device validate and residuals, "
                         "pcie_inclusive, the secondary configs, the CPU baseline (N > 1: the distributed solve and the weak-flops "
                         "case); off by default, the --no-* options and --cpu-grid trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's factor (or a seeded sample of it) as .npy files into DIR")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    ngpu = max(args.gpus, 1)
    if ngpu > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(ngpu)                                 # never returns: the N ranks are children of this process

    import numpy as np
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != ngpu:
        # one process can never stand in for N: a value is only printed by a job whose ranks match --gpus
        raise SystemExit(f"bench.py: --gpus {ngpu} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {ngpu} bench.py --gpus {ngpu} ...), or unset "
                         "WORLD_SIZE and let bench.py start its ranks itself")
    # rehearsal hooks (never set by the driver): SF_BENCH_BACKEND=gloo SF_BENCH_DEVICE=0 lets several ranks share
    # the single GPU of a test box to exercise the N > 1 code path end to end (gloo stages CUDA tensors via the host)
    backend = os.environ.get("SF_BENCH_BACKEND", "nccl")
    if "SF_BENCH_DEVICE" in os.environ:
        local_rank = int(os.environ["SF_BENCH_DEVICE"])
    # SF_FORCE_DISTRIBUTED=1 (rehearsal, never set by the driver): run the N > 1 code path -- nccl group, C-side RCCL communicator,
    # mapped plan, sf_chol_plan_factorize_distributed -- with ONE rank on the single GPU of a test box
    forced = os.environ.get("SF_FORCE_DISTRIBUTED") == "1" and world == 1
    if forced:
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1"); os.environ.setdefault("MASTER_PORT", "29571")
    if world > 1 or forced:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        import datetime
        tmo = datetime.timedelta(seconds=600)            # a rank that dies must not leave the others waiting for long
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)

    sf = importlib.import_module("sparse-matrix-factorization-library_amd")
    if sf.device_count() < 1:
        raise SystemExit("bench.py needs a HIP device: the numeric path has no CPU fallback")

    lu = args.method == "lu"
    N = args.grid or (79 if lu else (1000 if args.workload == "stencil2d" else 128))
    shard_one = (world > 1 or forced) and args.mp.startswith("subtree")
    if lu and shard_one and args.mp != "subtree":
        raise SystemExit("sharded LU supports --mp subtree (distributed top) only")
    scaled_grid = shard_one and world > 1 and not args.grid and (lu or args.workload == "lap3d")
    if scaled_grid and args.scale == "weak":
        N = int(round(N * world ** (1.0 / 3.0)))      # n = g^3: the matrix rows per GPU stay those of the base grid (256 at N = 8)
    elif scaled_grid and args.scale == "weak-flops":
        N = int(round(N * world ** (1.0 / 6.0)))      # F ~ g^6: the flops per GPU stay those of the base grid
    # devSlotSize is an input of the symbolic analysis (C:1402): the reference's own formula (C:82-87,199) for the number of
    # 288 GiB devices the job runs on (1: 8,694,792,192; 2: 17,390,632,960; 4 and 8: 34,781,265,920 = BASELINE config 4's)
    slot = int(sf.lib.sf_reference_slot_size(world if shard_one else 1, 288 << 30))
    t0 = time.time()

    inputs = {}

    def make(M, keep=False):
        if lu:   # BASELINE config 5 stand-in: n ~ 500k, nnz ~ 9M, structurally and numerically unsymmetric, diagonally dominant
            n_, Cp_, Ci_, Cx_ = sf.gen.unsymmetric_stencil(M, M, M, extra_per_row=0, seed=2024, drop=0.05)
            perm_ = sf.grid_nd_perm(M, M, M, 3, 1)
            sym_ = sf.analyze(n_, Cp_, Ci_, Cx_, perm_, slot, "lu", False)
        elif args.workload == "stencil2d":
            n_, Cp_, Ci_, Cx_ = sf.gen.stencil_spd_lower(M, M)
            perm_ = sf.grid_nd_perm(M, M, 1, 3, 2)
            sym_ = sf.analyze(n_, Cp_, Ci_, Cx_, perm_, slot)
        else:
            n_, Cp_, Ci_, Cx_ = sf.gen.laplacian_lower(M, M, M)
            perm_ = sf.grid_nd_perm(M, M, M, 3, 1)
            sym_ = sf.analyze(n_, Cp_, Ci_, Cx_, perm_, slot)
        if keep:
            inputs.update(n=n_, Cp=Cp_, Ci=Ci_, Cx=Cx_, perm=perm_)
        return n_, sym_, len(Ci_)

    n, sym, nnz_in = make(N, keep=True)
    t_analyze = time.time() - t0
    F_struct, F_exec = sym.flops_struct, sym.flops_exec

    t0 = time.time()
    sharded = None
    if shard_one:
        sharded = sf.ShardedCholesky(sym, rank, world, device=local_rank,
                                     mode="distributed" if args.mp == "subtree" else "replicated")
        if lu:
            sharded.set_values(sym.Lx, sym.Ux)
        else:
            sharded.set_values(sym.Lx)
        plan = sharded.engine.plan
    elif lu:
        plan = sf.LUPlan(sym, device=local_rank)
        plan.set_values(sym.Lx, sym.Ux)
        plan.set_pivoting(0.1)
    else:
        plan = sf.CholPlan(sym, device=local_rank)
        plan.set_values(sym.Lx)
    t_plan = time.time() - t0

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def step(sync):
        if sharded is not None:
            sharded.factorize()
        else:
            plan.factorize(sync=sync)

    for _ in range(args.warmup):
        step(True)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(False)
    plan.sync()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed / args.steps * 1e3
    units = 1 if sharded is not None else world       # matrices factorized per step by the whole job (--mp replicas: one per RANK)
    value = F_struct * units / (elapsed / args.steps) / 1e9

    # how many ranks took part: a sum of 1 over the communicator the factorization's own collectives use (the C library's RCCL
    # communicator when it is the one in charge, torch.distributed's otherwise).  Every rank gets the same number; unless it is
    # --gpus, nobody prints a value.
    collectives = getattr(sharded.engine, "comm_kind", "none") if sharded is not None else ("torch" if world > 1 else "none")
    ranks_seen = 1
    if world > 1 or forced:
        one = torch.ones(1, dtype=torch.float64, device=f"cuda:{local_rank}")
        comm = getattr(sharded.engine, "comm", None) if sharded is not None else None
        torch.cuda.synchronize()
        if comm is not None:
            comm.allreduce_sum(one.data_ptr(), 1, torch.cuda.current_stream(local_rank).cuda_stream)
        else:
            dist.all_reduce(one, op=dist.ReduceOp.SUM)
        torch.cuda.synchronize()
        ranks_seen = int(round(float(one.item()))) + int(os.environ.get("SF_TEST_RANKS_SEEN_DELTA", "0"))   # (test hook)
    if ranks_seen != ngpu:
        sys.stderr.write(f"bench.py: rank {rank}: --gpus {ngpu} but the communicator ({collectives}) counted {ranks_seen} ranks: no value\n")
        if world > 1 or forced:
            dist.destroy_process_group()
        raise SystemExit(3)

    if args.dump_outputs:
        # the factor of the last timed step, before anything below factorizes again; a sharded factor is gathered first
        # (every rank takes part), as --check does
        if sharded is not None:
            Lsx = sharded.gather_factor()
            if rank == 0:
                dump_factor(args.dump_outputs, int(sym.xsize), lambda b, e: Lsx[b:e])
            del Lsx
        elif rank == 0:
            dump_factor(args.dump_outputs, int(sym.xsize), plan_factor_range(sf, plan))

    out = {
        "metric": "numeric-factorization GFLOP/s (supernodal %s)" % ("LU, pivoting inside the diagonal blocks" if lu else "Cholesky"),
        "value": round(value, 2), "unit": "GFLOP/s", "n_gpus": ngpu, "ranks_seen": ranks_seen, "collectives": collectives,
        "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
        # N = 1 has no scaling rule (null); N > 1: "weak" = work per GPU fixed as N grows (rows per GPU, --scale weak), "strong" = total work fixed
        "scaling": None if ngpu == 1 else ("strong" if (sharded is not None and (args.scale == "strong" or not scaled_grid)) else "weak"),
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": (f"unsymmetric 3D 19-point stencil {N}^3 (5% of entries dropped one-sidedly), diagonally dominant, "
                                f"LU fp64 with threshold partial pivoting inside the 64x64 diagonal blocks, geometric ND, devSlotSize {slot}") if lu else
                               (f"2D {N}x{N} grid, 21-point random SPD stencil (rng 12345), Cholesky fp64, geometric ND with 2-line "
                                f"separators, devSlotSize {slot}") if args.workload == "stencil2d" else
                               f"3D 7-point Laplacian {N}^3 SPD Cholesky fp64, geometric ND, devSlotSize {slot}",
                   "n": n, "nnz_input": int(nnz_in), "nsuper": int(sym.nsuper), "factor_doubles": int(sym.xsize),
                   "F_struct": F_struct, "F_exec": F_exec,
                   "parallelism": (("elimination-tree subtrees sharded over the GPUs; top supernodes proportionally mapped (a top "
                                    "supernode lives on the ranks whose subtrees lie below it): large GEMMs split over that group, every "
                                    "top panel all-reduced once inside it (RCCL sub-communicators, issued by the C library on the "
                                    "plan's stream) block by block, 64-column chains replicated inside the group")
                                   if (sharded.mode == "distributed" and getattr(sharded.engine, "comm_kind", "") == "rccl-c") else
                                   ("elimination-tree subtrees sharded over the GPUs; top supernodes on every rank, their large GEMMs "
                                    "split over the ranks and every 512-column block all-reduced once by torch.distributed (the fall-back "
                                    "of the C-side RCCL path), 64-column chains replicated")
                                   if sharded.mode == "distributed" else
                                   ("elimination-tree subtrees sharded over the GPUs, one RCCL all-reduce of the top panels, "
                                    "top supernodes replicated")) if sharded is not None else
                                  ("1 matrix per GPU (independent)" if ngpu > 1 else "single GPU"),
                   "grid_rule": ((f"--scale {args.scale}: " + {"weak": "matrix rows per GPU fixed, grid = round(128 N^(1/3)); N = 8 is "
                                  "BASELINE config 4 (256^3 over 8 GPUs)", "weak-flops": "flops per GPU fixed, grid = round(128 N^(1/6))",
                                  "strong": "the N = 1 matrix on every N"}[args.scale]) if (shard_one and world > 1 and not args.grid)
                                 else ("explicit --grid" if args.grid else "BASELINE config")),
                   "sharding": sharded.plan_info() if sharded is not None else None,
                   "exec_GFLOPs": round(F_exec * units / (elapsed / args.steps) / 1e9, 2),
                   "host_analyze_s": round(t_analyze, 2), "plan_create_s": round(t_plan, 2),
                   "timed_region": "numeric factorization only (memset + assembly + panels + Schur updates) on resident inputs; the H2D of "
                                   "the matrix values (8 B x nnz_input) and the factor's D2H are excluded -- see pcie_inclusive"},
    }

    if args.full and rank == 0 and not args.no_roofline and sharded is None:
        plan.set_profiling(True)
        plan.factorize(sync=True)
        plan.set_profiling(False)
        upd_ms = plan.stat("last_update_ms")
        # k_gemm<1> does the Schur updates with K > 64; those of the small bottom-level supernodes run in k_update_small
        big_flops = plan.stat("flops_update") - plan.stat("flops_update_small")
        achieved = big_flops / (upd_ms * 1e-3) / 1e12 if upd_ms > 0 else 0.0
        # HBM traffic of that kernel: not measurable live (PMC counters need rocprofv3); taken from the committed
        # PMC passes of this exact workload when they exist (profiles/*_pmc_traffic_128cubed.json, bytes per launch)
        traffic = None
        files = []
        if (N == 128 and not lu and args.workload == "lap3d") or (N == 79 and lu):
            import glob
            files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic_lu_config5.json" if lu else "*_pmc_traffic_128cubed.json")))
            if files:
                with open(files[-1]) as f:
                    traffic = json.load(f).get("k_gemm<1>", {}).get("hbm_bytes_per_launch")
        out["roofline"] = {"bound": "mfma", "kernel": "k_gemm<1> (Schur update, fused scatter%s)" % (", L and U^T sides" if lu else ""),
                           "achieved": round(achieved, 3), "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                           "frac": round(achieved / FP64_MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                           "traffic_source": ("committed rocprofv3 --pmc passes (profiles/), NOT measured in this run: "
                                              + os.path.basename(files[-1])) if traffic is not None else None,
                           "traffic_note": "HBM bytes per launch of k_gemm<1> from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes "
                                           "(profiles/, FETCH_SIZE x2 after calibration); null when no committed pass matches",
                           "kernel_ms": round(upd_ms, 3), "panel_ms": round(plan.stat("last_panel_ms"), 3),
                           "load_ms": round(plan.stat("last_load_ms"), 3),
                           "potrf_ms": round(plan.stat("last_potrf_ms"), 3), "trsm_ms": round(plan.stat("last_trsm_ms"), 3),
                           "inner_gemm_ms": round(plan.stat("last_inner_gemm_ms"), 3),
                           "fused_step_ms": round(plan.stat("last_step_ms"), 3),
                           "outer_gemm_ms": round(plan.stat("last_outer_gemm_ms"), 3),
                           "flops_outer_gemm": plan.stat("flops_outer_gemm"),
                           "flops_panel_gemm": plan.stat("flops_panel_gemm"),
                           "flops_update": plan.stat("flops_update"),
                           "flops_update_small": plan.stat("flops_update_small"),
                           "small_update_ms": round(plan.stat("last_small_update_ms"), 3),
                           "launches": int(plan.stat("launches")), "levels": int(plan.stat("levels"))}
        if args.workload == "stencil2d" and not lu:
            # config 3 is the HBM-/latency-bound extend-add config: its roofline object is the HBM one of the whole factorization
            # (as in the default run's secondary.config3); the MFMA figures of its Schur GEMM stay available beside it
            hb = hbm_roofline_whole_factorization(plan, sym, ms_per_step)
            hb["schur_gemm_mfma"] = out["roofline"]
            out["roofline"] = hb

    if args.full and sharded is not None and sharded.mode == "distributed" and getattr(sharded.engine, "comm", None) is not None:
        # correctness of the multi-GPU run, outside the timed region: the distributed solve with the factor left on the ranks
        # (every rank takes part), then the reference's validate() residual on rank 0 (numpy over the analysed matrix)
        try:
            bvec = 1 + np.arange(n) / n
            t_s = time.perf_counter()
            xs = sharded.solve(bvec)
            solve_ms = (time.perf_counter() - t_s) * 1e3
            if rank == 0:
                if lu:
                    lc = np.repeat(np.arange(n), np.diff(sym.Lp))
                    rr = -bvec.copy()
                    np.add.at(rr, sym.Li, sym.Lx * xs[lc])
                    ur = np.repeat(np.arange(n), np.diff(sym.Up))
                    off = sym.Ui != ur
                    np.add.at(rr, ur[off], sym.Ux[off] * xs[sym.Ui[off]])
                    colsum = np.zeros(n)
                    np.add.at(colsum, lc, np.abs(sym.Lx))
                    np.add.at(colsum, sym.Ui[off], np.abs(sym.Ux[off]))
                    res = float(np.abs(rr).max() / (colsum.max() * np.abs(xs).max() + np.abs(bvec).max()))
                else:
                    res = sf.validate_solution(sym, xs)
                out["config"]["residual_distributed_solve"] = res
                out["config"]["distributed_solve_wall_ms"] = round(solve_ms, 3)
        except Exception as e:      # noqa: BLE001 -- the throughput line must not be lost to a failing check
            if rank == 0:
                out["config"]["residual_distributed_solve"] = f"failed: {e}"

    if args.full and rank == 0 and sharded is None:
        # the reference's validate() with nothing leaving the device but the scalar: solve with the resident factor and
        # residual kernels over the plan's copy of A (sf_chol_plan_validate); the numpy form of the same residual is the
        # host cross-check (Cholesky).  No oracle code and no 30 GB download involved.
        res_dev, xs = plan.validate(return_x=True)
        out["config"]["residual_device_solve"] = res_dev
        if not lu:
            out["config"]["residual_host_check"] = sf.validate_solution(sym, xs)
        out["config"]["device_solve_ms"] = round(plan.stat("last_solve_ms"), 3)

    if args.full and rank == 0 and sharded is None and not args.no_pcie:
        try:
            # Host-buffer boundary (never `value`): what the drop-in entry point costs.
            #  (a) plan level: values H2D + factorize + factor D2H into pageable memory, the download of finished blocks
            #      overlapped with the computation (sf_chol_plan_factorize_to_host); first call = fresh, never touched pages
            #  (b) the reference's own entry point SparseFrame_factorize over matrix_info_struct, twice on one handler list:
            #      the first call also builds and caches the device plan, the second finds it
            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                return (time.perf_counter() - t0) * 1e3

            # (the struct calls come first: their Lsx is the first 30 GB this process touches, as in a caller's own program)
            common = sf.CommonInfo(dev_slot_size=sf.REFERENCE_SLOT_1GPU)
            mi = (sf.LUMatrixInfo if lu else sf.MatrixInfo)()
            mi.set_csc(inputs["n"], inputs["Cp"], inputs["Ci"], inputs["Cx"], symmetric=not lu)
            mi.set_perm(inputs["perm"])
            mi.analyze(common)
            st = []
            for _ in range(2):
                mi.factorize(common)
                st.append(mi.c.factorizeTime * 1e3)
            pc = {}
            # the struct path's solve runs on the factor still resident in the handler's plan -- by default only after the fingerprint of
            # EVERY panel of the caller's Lsx has been compared with the device's (one threaded pass over the host array: that pass is
            # most of struct_solve_ms); sf_handlers_set_resident_solve(2) = the caller vouches for Lsx, nothing is compared
            res_struct = mi.validate()
            solve_verified_ms = 1e3 * mi.c.solveTime
            sf.lib.sf_handlers_set_resident_solve(2)
            mi.validate()
            solve_trusted_ms = 1e3 * mi.c.solveTime
            sf.lib.sf_handlers_set_resident_solve(1)
            pc.update({"struct_first_call_ms": round(st[0], 1), "struct_second_call_ms": round(st[1], 1),
                       # SURVEY 8(d) words the metric as F / wall time of SparseFrame_factorize WITH the upload of the symbolic structure:
                       # that is the first call of a pattern (plan build + first touch of Lsx + numeric + overlapped copy-back); the
                       # headline `value` is the plan-resident step (config.timed_region)
                       "GFLOPs_struct_first_call": round(F_struct / (st[0] * 1e-3) / 1e9, 1),
                       "GFLOPs_struct_second_call": round(F_struct / (st[1] * 1e-3) / 1e9, 1),
                       "struct_second_call_over_resident_step": round(st[1] / ms_per_step, 3),
                       "struct_residual": res_struct, "struct_solve_ms": round(solve_verified_ms, 3),
                       "struct_solve_trusted_ms": round(solve_trusted_ms, 3),
                       "fingerprint_fallbacks": int(sf.lib.sf_handlers_fingerprint_fallbacks()),     # verified solves that fell back to the host sweep: 0 expected
                       "note": "SparseFrame_factorize(common, gpu_info_list, matrix_info): pageable Lsx malloc'ed by SparseFrame_analyze; "
                               "call 1 = plan build + first touch of Lsx + factorize + overlapped copy-back, call 2 = cached plan"})
            mi.cleanup()
            common.close()
            host = np.empty(max(sym.xsize, 1), dtype=np.float64)      # untouched pages: the first call pays the first touch
            if lu:
                ms = [timed(lambda: plan.factorize_to_host(sym.Lx, sym.Ux, host)) for _ in range(2)]
            else:
                ms = [timed(lambda: plan.factorize_to_host(sym.Lx, host)) for _ in range(2)]
            if not lu:      # sum of log(diagonal of L): compared with the out-of-core run's below (secondary.out_of_core)
                pc["log_det_half"] = half_log_det(np, sym, host)
            del host
            pc.update({"plan_first_call_ms": round(ms[0], 1), "plan_second_call_ms": round(ms[1], 1),
                       "factor_bytes": int(sym.xsize) * 8,
                       "second_call_over_resident_step": round(ms[1] / ms_per_step, 3),
                       "GFLOPs_second_call": round(F_struct / (ms[1] * 1e-3) / 1e9, 1)})
            out["config"]["pcie_inclusive"] = pc
        except Exception as e:      # noqa: BLE001 -- the boundary measurement must not take the headline with it
            out["config"]["pcie_inclusive"] = {"error": f"{type(e).__name__}: {e}"}

    if args.check and sharded is not None:
        import oracle
        Lsx = sharded.gather_factor()
        if rank == 0:
            res, _ = (oracle.lu_residual if lu else oracle.chol_residual)(sym, Lsx)
            out["config"]["residual"] = res
        del Lsx
    elif args.check and rank == 0:
        import oracle
        Lsx = plan.get_factor()
        res, _ = (oracle.lu_residual if lu else oracle.chol_residual)(sym, Lsx)
        out["config"]["residual"] = res
        del Lsx

    if args.full and rank == 0 and ngpu == 1 and not args.no_secondary and not lu and args.workload == "lap3d" and args.grid in (0, 128):
        def guarded(fn, *a, **kw):
            # a secondary case that fails must not take the headline with it: its entry says what happened
            try:
                return fn(*a, **kw)
            except Exception as e:      # noqa: BLE001 -- reported, not swallowed
                return {"error": f"{type(e).__name__}: {e}"}

        out["secondary"] = {"config1": guarded(config1_case, sf, np), "config3": guarded(secondary_case, sf, np, "config3"),
                            "config5": guarded(secondary_case, sf, np, "config5"),
                            "config5_pivoting": guarded(secondary_case, sf, np, "config5_pivoting")}
        plan.close()            # (the 30 GB of the headline plan make room; nothing below uses it)
        plan = None
        out["secondary"]["out_of_core"] = guarded(out_of_core_case, sf, np, sym, in_core_log_det=out["config"].get("pcie_inclusive", {}).get("log_det_half"), inputs=inputs)
        out["secondary"]["end_to_end"] = guarded(end_to_end_case, sf, np, N)

    if args.cpu_grid < 0:
        args.cpu_grid = min(N, 128)
    if args.full and rank == 0 and ngpu == 1 and args.cpu_grid > 0:
        import oracle
        threads = args.cpu_threads or min(os.cpu_count() or 1, 16)   # reference: min(omp_max, 16), SparseFrame.c:3357
        binfo = oracle.blas_init("auto", threads=threads)
        M = min(args.cpu_grid, 56) if lu else (N if args.workload == "stencil2d" else args.cpu_grid)
        cpu_factorize = oracle.lu_factorize if lu else oracle.chol_factorize
        # warm-up (BLAS thread pool, allocator) on a small case of the same kind, then ONE timed factorization of the sample
        # (cpu-grid 128 = the headline matrix itself)
        if M > 56 and args.workload != "stencil2d":
            _, symw, _ = make(40)
            cpu_factorize(symw)
        n2, sym2, _ = make(M) if M != N else (n, sym, nnz_in)
        if M <= 56 or args.workload == "stencil2d":
            cpu_factorize(sym2)
        _, info, st = cpu_factorize(sym2)
        out["cpu_baseline"] = {"value": round(sym2.flops_struct / st["seconds"] / 1e9, 2), "unit": "GFLOP/s",
                               "cores": int(binfo["threads"]), "host_cores": int(os.cpu_count() or 0),
                               "seconds": round(st["seconds"], 2),
                               "same_matrix_as_value": bool(M == N),
                               # north_star's ratio: CPU-reference wall-clock over the GPU step's on THE SAME matrix (null for a sample)
                               "cpu_seconds_over_gpu_step": round(st["seconds"] / (ms_per_step * 1e-3), 1) if M == N else None,
                               "gpu_over_cpu_same_metric": round(value / (sym2.flops_struct / st["seconds"] / 1e9), 1),
                               "kind": "port",
                               "sample": f"{'unsymmetric 19-point stencil' if lu else ('2D 21-point stencil' if args.workload == 'stencil2d' else '3D 7-point Laplacian')} grid {M} (same generator and ordering), full numeric "
                                         f"factorization, F_struct {sym2.flops_struct:.3e}, {st['seconds']:.2f} s, "
                                         f"1 tree worker x {binfo['threads']} BLAS threads, "
                                         f"{os.path.basename(binfo['name'])}",
                               "info": int(info)}

    if sharded is not None:
        sharded.close()
    elif plan is not None:
        plan.close()

    if (args.full and shard_one and world > 1 and not args.no_secondary and not lu and args.workload == "lap3d" and args.mp == "subtree"
            and args.scale == "weak"):
        # the other weak-scaling rule (flops per GPU fixed: 144 / 161 / 181 for N = 2 / 4 / 8), timed after the headline case with a
        # few steps; every rank takes part.  A failure here is reported inside the object and never costs the headline line.
        base = args.grid or 128
        M2 = int(round(base * world ** (1.0 / 6.0)))
        sec = {"workload": f"3D 7-point Laplacian {M2}^3 SPD Cholesky fp64 sharded over {world} GPUs (flops per GPU fixed: "
                           f"grid = round({base} N^(1/6)))", "grid": M2}
        sh2 = None

        def all_ok(ok):
            """every rank learns whether ALL of them are fine (a MIN over the job's torch group): a rank that failed alone -- out of
            memory at the larger grid, a plan error -- must not leave the others inside the secondary case's collectives"""
            t_ = torch.tensor([1.0 if ok else 0.0], device=f"cuda:{local_rank}", dtype=torch.float64)
            dist.all_reduce(t_, op=dist.ReduceOp.MIN)
            return bool(t_.item() > 0.5)

        # the headline is safe first: rank 0 keeps it in a file next to stdout's line, so a hang in here can be told from a failed run
        if rank == 0:
            try:
                with open(os.environ.get("SF_BENCH_HEADLINE_COPY", "/tmp/sf_bench_headline.json"), "w") as f_:
                    json.dump(out, f_)
            except OSError:
                pass
        # time budget: the driver allows the whole command 600 s; the secondary case only starts while at least 150 s are left
        # (every rank uses rank 0's clock)
        used = torch.tensor([time.time() - T_PROCESS_START], device=f"cuda:{local_rank}", dtype=torch.float64)
        dist.broadcast(used, src=0)
        if float(used.item()) > 450.0:
            sec["skipped"] = f"{float(used.item()):.0f} s of the run already used"
        else:
            err = None
            try:
                _, sym2, _ = make(M2)
                sh2 = sf.ShardedCholesky(sym2, rank, world, device=local_rank, mode="distributed")
                sh2.set_values(sym2.Lx)
            except Exception as e:      # noqa: BLE001
                err = f"{type(e).__name__}: {e}"
            if not all_ok(err is None):
                sec["error"] = err or "setup failed on another rank"
            else:
                try:
                    k2 = max(1, min(args.steps, 3))
                    sh2.factorize()
                    barrier()
                    t0 = time.perf_counter()
                    for _ in range(k2):
                        sh2.factorize()
                    barrier()
                    el = torch.tensor([time.perf_counter() - t0], device=f"cuda:{local_rank}", dtype=torch.float64)
                    dist.all_reduce(el, op=dist.ReduceOp.MAX)
                    el = float(el.item())
                    sec.update({"n": int(sym2.n), "F_struct": sym2.flops_struct, "steps": k2, "ms_per_step": round(el / k2 * 1e3, 3),
                                "GFLOPs": round(sym2.flops_struct / (el / k2) / 1e9, 2),
                                "collectives": getattr(sh2.engine, "comm_kind", "engine")})
                    if getattr(sh2.engine, "comm", None) is not None:
                        xs = sh2.solve(1 + np.arange(sym2.n) / sym2.n)
                        if rank == 0:
                            sec["residual_distributed_solve"] = sf.validate_solution(sym2, xs)
                except Exception as e:      # noqa: BLE001 -- (a failure inside the C library's collectives is a dead communicator: see INTEGRATION.md)
                    sec["error"] = f"{type(e).__name__}: {e}"
            if sh2 is not None:
                sh2.close()
        out.setdefault("secondary", {})["weak_flops"] = sec

    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1 or forced:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
