"""GPU only: Sigma read on the pattern of A (`selinv_values_device`, `selinv_trace_device`, `selinv_entries`) on the
128^3 Cholesky plan and, with --lu, on the config 5 LU plan (unsymmetric stencil 79^3).  Prints one JSON line; per call:
  device_ms     "last_selinv_pattern_ms" (the kernels, copies excluded), minimum and median of --reps calls after one warm-up
  bytes         what the kernels must touch: the 8-byte map entry plus one 8-byte Sigma gather per entry, plus m * 8 bytes of V per
                entry for a trace (the off-diagonal marks of a Cholesky plan: one more byte), plus the output
  stream_ms     the time to stream those bytes at the HBM specification and at what a streaming copy reaches
  old_route     wall time of what a caller had to do before, once: get_selinv() -- the whole arena over PCIe -- and the host gather
                (--no-old skips it: it needs the arena's size in host memory)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sf = __import__("sparse-matrix-factorization-library_amd")
gen = sf.gen

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0       # MI355X HBM3E: specification; what a streaming copy reaches


def stats(ts):
    return {"min_ms": round(float(min(ts)), 4), "median_ms": round(float(np.median(ts)), 4)}


def timed(call, stat, reps):
    call()
    dev = []
    for _ in range(reps):
        call()
        dev.append(stat())
    return stats(dev)


def model(nbytes):
    return {"bytes": int(nbytes), "stream_ms_at_hbm_peak": round(nbytes / (HBM_PEAK_GBS * 1e6), 4),
            "stream_ms_at_hbm_achievable": round(nbytes / (HBM_ACHIEVABLE_GBS * 1e6), 4)}


def run(plan, sym, lu, reps, n_pairs, old):
    import torch
    import selinv_pattern_ref as spr
    own_u = lu and not sym.symmetric
    nnz, unz = len(sym.Li), (len(sym.Ui) if own_u else 0)
    live_entries = nnz + (unz if own_u else (nnz if lu else 0))     # what a trace walks: L and U (aliased: the L structure twice)
    out = {"n": int(sym.n), "nnz": nnz, "unz": unz, "arena_doubles": int(plan.stat("stored_doubles")) * (2 if lu else 1)}
    t0 = time.perf_counter()
    plan.selinv()
    out["selinv_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["selinv_device_ms"] = round(plan.stat("last_selinv_ms"), 1)
    ms = lambda: plan.stat("last_selinv_pattern_ms")
    dev = "cuda:0"
    dL = torch.empty(nnz, dtype=torch.float64, device=dev)
    dU = torch.empty(unz, dtype=torch.float64, device=dev) if own_u else None
    out["values_device"] = dict(timed(lambda: plan.selinv_values_device(dL, dU), ms, reps), **model((nnz + unz) * 24))
    for m in (1, 8, 64):
        VL = torch.rand((m, nnz), dtype=torch.float64, device=dev).t()             # column-major (nnz, m)
        VU = torch.rand((m, unz), dtype=torch.float64, device=dev).t() if own_u else None
        res = torch.empty(m, dtype=torch.float64, device=dev)
        r = timed(lambda: plan.selinv_trace_device(VL, VU, out=res), ms, reps)
        a, b = plan.selinv_trace_device(VL, VU).cpu().numpy(), plan.selinv_trace_device(VL, VU).cpu().numpy()
        r["repeatable_bitwise"] = bool(np.array_equal(a, b))
        out[f"trace_device_m{m}"] = dict(r, **model(live_entries * (16 + 8 * m) + (0 if lu else nnz)))
        del VL, VU
    rr, cc = spr.pattern_pairs(sym)
    k = np.random.default_rng(1).integers(0, len(rr), n_pairs)
    rows, cols = rr[k], cc[k]
    t0 = time.perf_counter()
    vals, outside = plan.selinv_entries(rows, cols)
    wall = (time.perf_counter() - t0) * 1e3
    out["entries"] = dict(timed(lambda: plan.selinv_entries(rows, cols), ms, reps), pairs=n_pairs, outside=outside, first_call_wall_ms=round(wall, 2))
    out["bytes_selinv_pattern"] = int(plan.stat("bytes_selinv_pattern"))
    if old:
        t0 = time.perf_counter()
        S = plan.get_selinv()
        t1 = time.perf_counter()
        ref = spr.lu_values(sym, S, bool(sym.symmetric))[0] if lu else spr.chol_values(sym, S)
        t2 = time.perf_counter()
        out["old_route_wall"] = {"get_selinv_ms": round((t1 - t0) * 1e3, 1), "host_gather_ms": round((t2 - t1) * 1e3, 1)}
        out["values_equal_old_route_bitwise"] = bool(np.array_equal(dL.cpu().numpy(), ref))
        t0 = time.perf_counter()
        plan.selinv_values()
        out["values_host_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--lu", action="store_true", help="the config 5 LU plan (unsymmetric stencil, default 79^3) instead")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--no-old", action="store_true")
    a = ap.parse_args()
    if sf.device_count() < 1:
        raise SystemExit("selinv_pattern_timing: no HIP device")
    if a.lu:
        N = 79 if a.N == 128 else a.N
        n, Cp, Ci, Cx = gen.unsymmetric_stencil(N, N, N, extra_per_row=0, seed=2024, drop=0.05)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), sf.REFERENCE_SLOT_1GPU, "lu", False)
        plan = sf.LUPlan(sym)
        plan.set_values(sym.Lx, sym.Ux)
    else:
        N = a.N
        n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), sf.REFERENCE_SLOT_1GPU)
        plan = sf.CholPlan(sym)
        plan.set_values(sym.Lx)
    plan.factorize()
    print("selinv_pattern_timing: factorized", file=sys.stderr, flush=True)
    out = run(plan, sym, a.lu, a.reps, a.pairs, not a.no_old)
    plan.close()
    print(json.dumps({"tool": "selinv_pattern_timing", "reps": a.reps, ("lu" if a.lu else "cholesky") + f"_{N}cubed": out}))


if __name__ == "__main__":
    main()
