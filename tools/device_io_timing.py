"""GPU only: the device-pointer solves next to the host-array solves on ONE plan, 128^3 Cholesky.  Prints one JSON line: for 1 and
16 columns, `solve` / `solve_many` on host arrays and `solve_device` on torch tensors without and with both permutation flags --
device ms from the plan's stats ("last_solve_ms" / "last_solve_many_ms": first to last kernel of the call, so the device-pointer
numbers include their load / store kernels and the host-array numbers their pack / unpack but no copy) and, separately, the wall
time of the whole call (host clock; every call ends in a synchronise) -- the minimum and the median over --reps calls after one
warm-up call each.  Also `set_values` against `set_values_device` / `set_values_mapped_device` (wall time), and the bytes the
pack / unpack kernels stream, for the kernel times of a `rocprofv3 --kernel-trace --stats` run of this tool (--reps 2 is enough
there: k_dev_pack / k_dev_unpack with and without the ordering, and k_solve_many_pack / _unpack, the untiled form, next to them)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sf = __import__("sparse-matrix-factorization-library_amd")
gen = sf.gen

HBM_PEAK_GBS, HBM_ACHIEVABLE_GBS = 8000.0, 6300.0       # MI355X HBM3E: specification; what a streaming copy reaches


def timed(call, stat, reps):
    call()
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        if stat is not None:
            dev.append(stat())
    out = {"wall_min_ms": round(float(min(wall)), 3), "wall_median_ms": round(float(np.median(wall)), 3)}
    if stat is not None:
        out.update({"device_min_ms": round(float(min(dev)), 3), "device_median_ms": round(float(np.median(dev)), 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if sf.device_count() < 1:
        raise SystemExit("device_io_timing: no HIP device")
    import torch
    N = a.N
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    perm = sf.grid_nd_perm(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, perm, sf.REFERENCE_SLOT_1GPU)
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx)
    plan.factorize()
    plan.set_ordering(perm)
    W = int(plan.stat("solve_many_width"))
    rng = np.random.default_rng(2024)
    b = rng.standard_normal(n)
    B = np.asfortranarray(rng.standard_normal((n, W)))
    bd = torch.from_numpy(b).to("cuda:0")
    Bd = torch.from_numpy(np.ascontiguousarray(B.T)).to("cuda:0").t()       # column-major on the device
    xd, Xd = torch.empty_like(bd), torch.empty_strided((n, W), (1, n), dtype=torch.float64, device="cuda:0")
    one, many = (lambda: plan.stat("last_solve_ms")), (lambda: plan.stat("last_solve_many_ms"))
    out = {"n": n, "width": W}
    # alternating host-array and device-pointer calls: the same sweeps in the same session
    out["solve_host_1"] = timed(lambda: plan.solve(b), one, a.reps)
    out["solve_device_1"] = timed(lambda: plan.solve_device(bd, out=xd), one, a.reps)
    out["solve_device_1_perm"] = timed(lambda: plan.solve_device(bd, out=xd, perm_in=True, perm_out=True), one, a.reps)
    out["solve_host_1_again"] = timed(lambda: plan.solve(b), one, a.reps)
    out["solve_many_host_16"] = timed(lambda: plan.solve_many(B), many, a.reps)
    out["solve_device_16"] = timed(lambda: plan.solve_device(Bd, out=Xd), many, a.reps)
    out["solve_device_16_perm"] = timed(lambda: plan.solve_device(Bd, out=Xd, perm_in=True, perm_out=True), many, a.reps)
    out["solve_many_host_16_again"] = timed(lambda: plan.solve_many(B), many, a.reps)
    out["permute_device_16"] = timed(lambda: plan.permute_device(Bd, out=Xd), None, a.reps)
    out["permute_device_16_inverse"] = timed(lambda: plan.permute_device(Bd, out=Xd, inverse=True), None, a.reps)
    # what the numbers are numbers of
    X = plan.solve_many(B)
    plan.solve_device(Bd, out=Xd)
    out["device_vs_host_rel_diff"] = float(np.abs(Xd.cpu().numpy() - X).max() / np.abs(X).max())
    Bo = np.empty_like(B)
    Bo[perm] = B
    Bod = torch.from_numpy(np.ascontiguousarray(Bo.T)).to("cuda:0").t()
    plan.solve_device(Bod, out=Xd, perm_in=True, perm_out=True)
    out["device_perm_vs_host_rel_diff"] = float(np.abs(Xd.cpu().numpy()[perm] - X).max() / np.abs(X).max())
    # values
    Lxd = torch.from_numpy(sym.Lx).to("cuda:0")
    Axd = torch.from_numpy(np.asarray(Cx, dtype=np.float64)).to("cuda:0")
    nsrc, mapL, mapU = sym.value_map()
    plan.set_value_map(nsrc, mapL, mapU)
    out["nnz"] = int(sym.nnz)
    out["set_values_host"] = timed(lambda: plan.set_values(sym.Lx), None, a.reps)
    out["set_values_device"] = timed(lambda: plan.set_values_device(Lxd), None, a.reps)
    out["set_values_mapped_device"] = timed(lambda: plan.set_values_mapped_device(Axd), None, a.reps)
    out["bytes_ordering"] = plan.stat("bytes_ordering")
    plan.close()
    nbytes = n * W * 8
    out["block_bytes"] = nbytes
    # a pack or an unpack reads the block once and writes it once
    out["pack_stream_ms_at_hbm_peak"] = round(2 * nbytes / (HBM_PEAK_GBS * 1e6), 4)
    out["pack_stream_ms_at_hbm_achievable"] = round(2 * nbytes / (HBM_ACHIEVABLE_GBS * 1e6), 4)
    print(json.dumps({"tool": "device_io_timing", "reps": a.reps, f"cholesky_{N}cubed": out}))


if __name__ == "__main__":
    main()
