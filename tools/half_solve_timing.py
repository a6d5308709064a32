"""GPU only: the half solves, the quadratic form and the sampler next to the plain solves on ONE plan, 128^3 Cholesky.  Prints one
JSON line: device ms (the plan's solve event pair, copies excluded) of `solve`, of `solve_half` L / Lt at nrhs = 1, of `solve_many`,
`solve_half` L / Lt, `quadform` and `sample` at 16 columns -- the minimum and the median over --reps calls after one warm-up call
each -- and k_sample_fill alone (HIP events around the launcher of the library) against the time to stream n x 16 x 8 bytes at HBM
speed."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sf = __import__("sparse-matrix-factorization-library_amd")
gen = sf.gen

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0       # MI355X HBM3E: specification; what a streaming copy reaches


def timed(call, stat, reps):
    call()
    ts = []
    for _ in range(reps):
        call()
        ts.append(stat())
    return {"min_ms": round(float(min(ts)), 3), "median_ms": round(float(np.median(ts)), 3)}


def fill_alone(n, W, reps):
    """k_sample_fill on a buffer of its own: sf::launch_sample_fill of the library, on the null stream between two events"""
    so = os.path.join(ROOT, "sparse-matrix-factorization-library_amd", "libsparseframe_hip.so")
    nm = subprocess.run(["nm", "-D", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    (name,) = [ln.split()[-1] for ln in nm.splitlines() if "launch_sample_fill" in ln and " T " in ln]
    launch = getattr(sf.lib, name)
    launch.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
    launch.restype = None
    hip = sf.lib            # (a symbol lookup on the library's handle reaches the one HIP runtime it is linked to)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    buf, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipSetDevice(0))
    ok(hip.hipMalloc(C.byref(buf), C.c_size_t(n * W * 8)))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    ts = []
    for r in range(reps + 1):
        ok(hip.hipEventRecord(e0, None))
        launch(buf, n, W, 2024, W * r, None)
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        ts.append(ms.value)
    ok(hip.hipEventDestroy(e0))
    ok(hip.hipEventDestroy(e1))
    ok(hip.hipFree(buf))
    ts = ts[1:]
    nbytes = n * W * 8
    return {"min_ms": round(float(min(ts)), 4), "median_ms": round(float(np.median(ts)), 4), "bytes": nbytes,
            "stream_ms_at_hbm_peak": round(nbytes / (HBM_PEAK_GBS * 1e6), 4),
            "stream_ms_at_hbm_achievable": round(nbytes / (HBM_ACHIEVABLE_GBS * 1e6), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if sf.device_count() < 1:
        raise SystemExit("half_solve_timing: no HIP device")
    N = a.N
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), sf.REFERENCE_SLOT_1GPU)
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx)
    plan.factorize()
    W = int(plan.stat("solve_many_width"))
    rng = np.random.default_rng(2024)
    b = rng.standard_normal(n)
    B = np.asfortranarray(rng.standard_normal((n, W)))
    half, many = (lambda: plan.stat("last_half_ms")), (lambda: plan.stat("last_solve_many_ms"))
    out = {"n": n, "width": W}
    out["solve"] = timed(lambda: plan.solve(b), lambda: plan.stat("last_solve_ms"), a.reps)
    out["solve_half_L_1"] = timed(lambda: plan.solve_half(b, "L"), half, a.reps)
    out["solve_half_Lt_1"] = timed(lambda: plan.solve_half(b, "Lt"), half, a.reps)
    out["quadform_1"] = timed(lambda: plan.quadform(b), lambda: plan.stat("last_quadform_ms"), a.reps)
    out["solve_many_16"] = timed(lambda: plan.solve_many(B), many, a.reps)
    out["solve_half_L_16"] = timed(lambda: plan.solve_half(B, "L"), half, a.reps)
    out["solve_half_Lt_16"] = timed(lambda: plan.solve_half(B, "Lt"), half, a.reps)
    out["quadform_16"] = timed(lambda: plan.quadform(B), lambda: plan.stat("last_quadform_ms"), a.reps)
    out["sample_16"] = timed(lambda: plan.sample(W, seed=2024), lambda: plan.stat("last_sample_ms"), a.reps)
    # what the numbers are numbers of: the halves compose to the solve, the quadratic form is b^T A^-1 b
    x = plan.solve(b)
    y = plan.solve_half(plan.solve_half(b, "L"), "Lt")
    out["halves_vs_solve_rel_diff"] = float(np.abs(y - x).max() / np.abs(x).max())
    q = plan.quadform(b)
    out["quadform_vs_dot_rel_diff"] = abs(q - float(b @ x)) / abs(q)
    plan.close()
    out["sample_fill_alone"] = fill_alone(n, W, a.reps)
    print(json.dumps({"tool": "half_solve_timing", "reps": a.reps, f"cholesky_{N}cubed": out}))


if __name__ == "__main__":
    main()
