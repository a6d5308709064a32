"""GPU only: the Schur complement of a border, G = B^T A^-1 B (`CholPlan.gram`), next to the library's existing kernels
on ONE plan, 128^3 Cholesky, at k = 16, 64 and 256 columns.  Prints one JSON line; per k:
  gram             device ms of `gram` ("last_gram_ms": forward sweeps and reductions, copies excluded) and its wall time
  gram_padded      --pad P: the same call through the C entry point with B in an array of leading dimension n + P (the chunks' way
                   to the device is then a strided copy)
  solve_half_L     device ms of `solve_half(B, "L")` for the same k ("last_half_ms"): the same sweeps with an unpack kernel in place
                   of the reduction, so gram - solve_half_L is what the reduction costs beyond the unpack
  solve_many       device ms of `solve_many(B)` ("last_solve_many_ms"): both sweeps
  old_route        wall time of what a caller had to do before: X = solve_many(B) (which downloads the n x k block), then B.T @ X
  reduction_alone  k_gram_part + k_gram_final for every chunk row on a store of their own (sf::launch_gram_row of the library, on the
                   null stream between two events)
  reduction_model  the bytes the reduction reads -- tile (a, b) reads 2 n 128 bytes, a diagonal tile n 128 -- and the time to stream
                   them at HBM speed
The minimum and the median over --reps calls after one warm-up call each; the old route is timed --reps-old times."""
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


def reduction_alone(n, W, k, reps):
    """every chunk row of the reduction on a zeroed store of its own: sf::launch_gram_row, null stream, one event pair"""
    so = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "libsparseframe_hip.so")
    nm = subprocess.run(["nm", "-D", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    sym = lambda part: [ln.split()[-1] for ln in nm.splitlines() if part in ln and " T " in ln]
    (row_name,), (slabs_name,) = sym("launch_gram_row"), sym("gram_slabs")
    launch, slabs = getattr(sf.lib, row_name), getattr(sf.lib, slabs_name)
    launch.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    launch.restype = None
    slabs.argtypes = [C.c_int64, C.POINTER(C.c_int64)]
    slabs.restype = C.c_int
    hip = sf.lib            # (a symbol lookup on the library's handle reaches the one HIP runtime it is linked to)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    nch = (k + W - 1) // W
    rows = C.c_int64()
    ns = slabs(n, C.byref(rows))
    sizes = (nch * n * W * 8, nch * ns * W * W * 8, k * k * 8)
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
        for a in range(nch):
            launch(bufs[0], n, a, k, bufs[1], bufs[2], k, None)
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        ts.append(ms.value)
    ok(hip.hipEventDestroy(e0))
    ok(hip.hipEventDestroy(e1))
    for b in bufs:
        ok(hip.hipFree(b))
    return dict(stats(ts[1:]), launches=2 * nch, slabs=ns, slab_rows=rows.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--ks", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reps-old", type=int, default=2)
    ap.add_argument("--pad", type=int, default=0, help="also time the host call with ldb = n + PAD")
    a = ap.parse_args()
    if sf.device_count() < 1:
        raise SystemExit("gram_timing: no HIP device")
    N = a.N
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), sf.REFERENCE_SLOT_1GPU)
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx)
    plan.factorize()
    W = int(plan.stat("solve_many_width"))
    rng = np.random.default_rng(2024)
    out = {"n": n, "width": W}
    for k in a.ks:
        B = np.empty((n, k), order="F")
        for j in range(k):
            B[:, j] = rng.standard_normal(n)
        r = {}
        g_dev, g_wall = timed(lambda: plan.gram(B), lambda: plan.stat("last_gram_ms"), a.reps)
        r["gram"], r["gram_wall"] = g_dev, g_wall
        if a.pad:
            Bp = np.zeros((n + a.pad, k), order="F")
            Bp[:n] = B
            Gp = np.zeros((k, k), order="F")
            dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))

            def padded():
                sf._lib.check(sf.lib.sf_chol_plan_gram(plan._h, k, dp(Bp), n + a.pad, dp(Gp), k), "sf_chol_plan_gram")

            r["gram_padded"], r["gram_padded_wall"] = timed(padded, lambda: plan.stat("last_gram_ms"), a.reps)
            del Bp
        r["parts"] = int(plan.stat("last_gram_parts"))
        r["bytes_gram"] = int(plan.stat("bytes_gram"))
        r["solve_half_L"], _ = timed(lambda: plan.solve_half(B, "L"), lambda: plan.stat("last_half_ms"), a.reps)
        r["reduction_beyond_unpack_ms"] = round(g_dev["min_ms"] - r["solve_half_L"]["min_ms"], 3)
        old = []
        for _ in range(a.reps_old):
            t0 = time.perf_counter()
            X = plan.solve_many(B)
            t1 = time.perf_counter()
            G_old = B.T @ X
            old.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        r["solve_many"] = {"device_ms": round(plan.stat("last_solve_many_ms"), 3)}
        r["old_route_wall"] = {"solve_many_with_copies_ms": round(min(t[0] for t in old), 3), "host_product_ms": round(min(t[1] for t in old), 3),
                               "total_min_ms": round(min(t[0] + t[1] for t in old), 3)}
        del X
        # what the numbers are numbers of
        G = plan.gram(B)
        r["gram_vs_old_route_rel_diff"] = float(np.abs(G - G_old).max() / np.abs(G_old).max())
        r["symmetric_bitwise"] = bool(np.array_equal(G, G.T))
        nch = (k + W - 1) // W
        nbytes = (nch * nch) * n * W * 8          # nch diagonal tiles read n 128 bytes, nch (nch - 1) / 2 others twice that
        r["reduction_alone"] = reduction_alone(n, W, k, a.reps)
        r["reduction_model"] = {"bytes": nbytes, "flops": n * 2 * W * W * (nch * (nch + 1) // 2),
                                "stream_ms_at_hbm_peak": round(nbytes / (HBM_PEAK_GBS * 1e6), 3),
                                "stream_ms_at_hbm_achievable": round(nbytes / (HBM_ACHIEVABLE_GBS * 1e6), 3)}
        out[f"k{k}"] = r
        print(f"gram_timing: k = {k} done", file=sys.stderr, flush=True)
        del B
    plan.close()
    print(json.dumps({"tool": "gram_timing", "reps": a.reps, f"cholesky_{N}cubed": out}))


if __name__ == "__main__":
    main()
