"""GPU only: the LU plans' half solves and G = C^T A^-1 B (`LUPlan.half_solve`, `cross_gram`) next to the library's
existing kernels on ONE plan: LU config 5 (the unsymmetric 19-point stencil 79^3 of bench.py, n = 493,039), pivoting off and on.
Prints one JSON line; per pivot setting:
  half_<which>_<k>   device ms ("last_half_ms") of each half at 1 and 16 columns
  solve_<k>, solve_trans_<k>   `solve` / `solve_many` and their transposed twins at the same widths ("last_solve_ms",
                     "last_solve_many_ms"): the parent commit's kernels, the yardstick of the halves
and per m = k in --ks:
  cross_gram         device ms ("last_gram_ms": both forward sweeps and the reductions, copies excluded) and wall time
  half_L, half_Ut    device ms of the two forward halves at that width: cross_gram is expected to cost about their sum
  solve_many         device ms of `solve_many(B)`
  old_route          wall time of what a caller had to do before: X = solve_many(B) (which downloads n x k), then C.T @ X
  reduction_alone    k_gram2_part + k_gram2_final for every chunk column on a zeroed store of their own (sf::launch_gram2_col of the
                     library, null stream, one event pair)
  reduction_model    the bytes the reduction reads -- every tile reads 2 n 128 bytes -- and the time to stream them at HBM speed
The minimum and the median over --reps calls after one warm-up call each."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sf = __import__("sparse-matrix-factorization-library_amd")
gen = sf.gen

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0       # MI355X HBM3E: specification; what a streaming copy reaches


def stats(ts):
    return {"min_ms": round(float(min(ts)), 4), "median_ms": round(float(np.median(ts)), 4)}


def timed(call, stat, reps):
    """(device ms from `stat`, wall ms) of `call`, after one warm-up call"""
    call()
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(stat())
    return stats(dev), stats(wall)


def reduction_alone(n, W, m, k, reps):
    """every chunk column of the reduction on a zeroed store of its own"""
    so = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "libsparseframe_hip.so")
    nm = subprocess.run(["nm", "-D", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    sym = lambda part: [ln.split()[-1] for ln in nm.splitlines() if part in ln and " T " in ln]
    (col_name,), (slabs_name,) = sym("launch_gram2_col"), sym("gram_slabs")
    launch, slabs = getattr(sf.lib, col_name), getattr(sf.lib, slabs_name)
    launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    launch.restype = None
    slabs.argtypes = [C.c_int64, C.POINTER(C.c_int64)]
    slabs.restype = C.c_int
    hip = sf.lib            # (a symbol lookup on the library's handle reaches the one HIP runtime it is linked to)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    nz, ny = (m + W - 1) // W, (k + W - 1) // W
    rows = C.c_int64()
    ns = slabs(n, C.byref(rows))
    blk = n * W * 8
    sizes = (nz * blk, ny * blk, nz * ns * W * W * 8, m * k * 8)
    bufs = [C.c_void_p() for _ in sizes]
    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipSetDevice(0))
    for b, sz in zip(bufs, sizes):
        ok(hip.hipMalloc(C.byref(b), C.c_size_t(sz)))
        ok(hip.hipMemset(b, 0, C.c_size_t(sz)))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    ts = []
    for _ in range(reps + 1):
        ok(hip.hipEventRecord(e0, None))
        for b in range(ny):
            launch(bufs[0], C.c_void_p(bufs[1].value + b * blk), n, nz, b, m, k, bufs[2], bufs[3], m, None)
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        ts.append(ms.value)
    ok(hip.hipEventDestroy(e0))
    ok(hip.hipEventDestroy(e1))
    for b in bufs:
        ok(hip.hipFree(b))
    return dict(stats(ts[1:]), launches=2 * ny, slabs=ns, slab_rows=rows.value)


def one_setting(sym, n, tol, a, rng):
    plan = sf.LUPlan(sym)
    plan.set_values(sym.Lx, sym.Ux)
    if tol > 0:
        plan.set_pivoting(tol)
    plan.factorize()
    W = int(plan.stat("solve_many_width"))
    out = {"n": n, "width": W, "pivot_tol": tol, "rows_moved": int(np.count_nonzero(plan.get_pivots() != np.arange(n)))}
    half, many, one = (lambda: plan.stat("last_half_ms")), (lambda: plan.stat("last_solve_many_ms")), (lambda: plan.stat("last_solve_ms"))
    b = rng.standard_normal(n)
    B16 = np.asfortranarray(rng.standard_normal((n, W)))
    for which in ("L", "U", "Ut", "Lt"):
        out[f"half_{which}_1"], _ = timed(lambda: plan.half_solve(b, which), half, a.reps)
        out[f"half_{which}_{W}"], _ = timed(lambda: plan.half_solve(B16, which), half, a.reps)
    for trans, name in ((False, "solve"), (True, "solve_trans")):
        out[f"{name}_1"], _ = timed(lambda: plan.solve(b, trans=trans), one, a.reps)
        out[f"{name}_{W}"], _ = timed(lambda: plan.solve_many(B16, trans=trans), many, a.reps)
    x = plan.solve(b)
    y = plan.half_solve(plan.half_solve(b, "L"), "U")
    out["halves_vs_solve_rel_diff"] = float(np.abs(y - x).max() / np.abs(x).max())
    for k in a.ks:
        Cm, B = np.empty((n, k), order="F"), np.empty((n, k), order="F")
        for j in range(k):
            Cm[:, j], B[:, j] = rng.standard_normal(n), rng.standard_normal(n)
        r = {}
        r["cross_gram"], r["cross_gram_wall"] = timed(lambda: plan.cross_gram(Cm, B), lambda: plan.stat("last_gram_ms"), a.reps)
        r["parts"], r["bytes_gram"] = int(plan.stat("last_gram_parts")), int(plan.stat("bytes_gram"))
        r["half_L"], _ = timed(lambda: plan.half_solve(B, "L"), half, a.reps)
        r["half_Ut"], _ = timed(lambda: plan.half_solve(Cm, "Ut"), half, a.reps)
        r["beyond_the_two_halves_ms"] = round(r["cross_gram"]["min_ms"] - r["half_L"]["min_ms"] - r["half_Ut"]["min_ms"], 3)
        old = []
        for _ in range(a.reps_old):
            t0 = time.perf_counter()
            X = plan.solve_many(B)
            t1 = time.perf_counter()
            G_old = Cm.T @ X
            old.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        r["solve_many"] = {"device_ms": round(plan.stat("last_solve_many_ms"), 3)}
        r["old_route_wall"] = {"solve_many_with_copies_ms": round(min(t[0] for t in old), 3), "host_product_ms": round(min(t[1] for t in old), 3),
                               "total_min_ms": round(min(t[0] + t[1] for t in old), 3)}
        del X
        G = plan.cross_gram(Cm, B)
        r["cross_gram_vs_old_route_rel_diff"] = float(np.abs(G - G_old).max() / np.abs(G_old).max())
        nch = (k + W - 1) // W
        nbytes = 2 * nch * nch * n * W * 8
        if tol == 0:
            r["reduction_alone"] = reduction_alone(n, W, k, k, a.reps)
            r["reduction_model"] = {"bytes": nbytes, "stream_ms_at_hbm_peak": round(nbytes / (HBM_PEAK_GBS * 1e6), 3),
                                    "stream_ms_at_hbm_achievable": round(nbytes / (HBM_ACHIEVABLE_GBS * 1e6), 3)}
        out[f"k{k}"] = r
        print(f"gram_lu_timing: tol = {tol}, m = k = {k} done", file=sys.stderr, flush=True)
        del B, Cm
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=79)
    ap.add_argument("--ks", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--tols", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reps-old", type=int, default=2)
    a = ap.parse_args()
    if sf.device_count() < 1:
        raise SystemExit("gram_lu_timing: no HIP device")
    N = a.N
    n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, extra_per_row=0, seed=2024, drop=0.05)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N, 3, 1), sf.REFERENCE_SLOT_1GPU, "lu", False)
    rng = np.random.default_rng(2024)
    res = {"tool": "gram_lu_timing", "reps": a.reps}
    for tol in a.tols:
        res[f"lu_config5_{N}cubed_tol{tol:g}"] = one_setting(sym, n, tol, a, rng)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
