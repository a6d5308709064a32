"""GPU only: `adjoint_values_device` on the 128^3 Cholesky plan for k in {1, 16} against the torch composition a caller
had to write before it.  Writes profiles/<round>_adjoint_timing.json (--out overrides) and prints the same JSON line.  Per k:
  kernel        "last_adjoint_ms" (the kernel, copies excluded): minimum and median of --reps calls after one warm-up, and the
                bandwidth the byte model implies at the median
  bytes_min     positions x (row index 4 + column 4 + mark 1 + output 8) plus every element of the two n x k blocks once
  bytes_gather  the same with the operand rows as the kernel asks for them: per position 2 (diagonal) or 4 (off the diagonal)
                rows of k doubles -- what reaches HBM lies between the two, depending on what the caches keep
  torch         the same gradient by index gathers, multiply, sum over the columns and the symmetric second term: device time
                (events) of --reps calls after a warm-up, the peak extra device memory of one call, and the largest difference
                from the kernel's result relative to the largest entry
The plan is never factorized: adjoint_values reads the structure alone."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sf = __import__("sparse-matrix-factorization-library_amd")
gen = sf.gen

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0       # MI355X HBM3E: specification; what a streaming copy reaches


def stats(ts):
    return {"min_ms": round(float(min(ts)), 4), "median_ms": round(float(np.median(ts)), 4)}


def torch_gradient(torch, Lam, X, rows, cols, off):
    """-(Lam X^T + X Lam^T) on the pattern, the diagonal once: what a caller writes with torch indexing"""
    g = (Lam[rows] * X[cols]).sum(1)
    g = g + torch.where(off, (Lam[cols] * X[rows]).sum(1), torch.zeros_like(g))
    return -g


def run(plan, sym, k, reps):
    import torch
    dev = "cuda:0"
    n, nnz = int(sym.n), len(sym.Li)
    gen_ = torch.Generator(device=dev).manual_seed(k)
    Lam = torch.rand((k, n), dtype=torch.float64, device=dev, generator=gen_).t()      # column-major (n, k)
    X = torch.rand((k, n), dtype=torch.float64, device=dev, generator=gen_).t()
    out = torch.empty(nnz, dtype=torch.float64, device=dev)
    call = lambda: plan.adjoint_values_device(Lam, X, out=out, alpha=-1.0)
    call()
    ts = []
    for _ in range(reps):
        call()
        ts.append(plan.stat("last_adjoint_ms"))
    res = {"kernel": stats(ts)}
    Li = np.asarray(sym.Li)
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(sym.Lp)))
    ndiag = int(np.count_nonzero(Li == col))
    bytes_min = nnz * 17 + 2 * n * k * 8
    bytes_gather = nnz * 17 + (2 * ndiag + 4 * (nnz - ndiag)) * k * 8
    med = res["kernel"]["median_ms"]
    for name, b in (("bytes_min", bytes_min), ("bytes_gather", bytes_gather)):
        res[name] = {"bytes": int(b), "gbs_at_median": round(b / (med * 1e6), 1) if med > 0 else None,
                     "stream_ms_at_hbm_achievable": round(b / (HBM_ACHIEVABLE_GBS * 1e6), 4)}
    # ---- the torch composition ----
    rows, cols = torch.from_numpy(Li.astype(np.int64)).to(dev), torch.from_numpy(col).to(dev)
    off = rows != cols
    Lr, Xr = Lam.contiguous(), X.contiguous()          # row-major: a gathered row is one run (the caller's best case)
    torch.cuda.synchronize()
    g = torch_gradient(torch, Lr, Xr, rows, cols, off)
    torch.cuda.synchronize()
    scale = float(out.abs().max())
    res["torch"] = {"max_abs_diff_over_max": float((g - out).abs().max()) / scale if scale else 0.0}
    del g
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    g = torch_gradient(torch, Lr, Xr, rows, cols, off)
    torch.cuda.synchronize()
    res["torch"]["peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    res["torch"]["nnz_x_k_temporary_bytes"] = int(nnz * k * 8)
    del g
    tt = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g = torch_gradient(torch, Lr, Xr, rows, cols, off)
        e1.record()
        torch.cuda.synchronize()
        tt.append(e0.elapsed_time(e1))
        del g
    res["torch"].update(stats(tt))
    res["kernel_over_torch_median"] = round(med / res["torch"]["median_ms"], 3) if res["torch"]["median_ms"] > 0 else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--round", default="r24_a")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if sf.device_count() < 1:
        raise SystemExit("adjoint_timing: no HIP device")
    N = a.N
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), sf.REFERENCE_SLOT_1GPU)
    plan = sf.CholPlan(sym)
    res = {"tool": "adjoint_timing", "reps": a.reps, "workload": f"cholesky_{N}cubed", "n": int(n), "nnz": len(sym.Li)}
    for k in (1, 16):
        res[f"k{k}"] = run(plan, sym, k, a.reps)
    res["bytes_adjoint"] = int(plan.stat("bytes_adjoint"))
    plan.close()
    path = a.out or os.path.join(ROOT, "profiles", f"{a.round}_adjoint_timing.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
