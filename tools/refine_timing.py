#!/usr/bin/env python3
"""What a refined solve costs: the device loop (plan.refine) against the hand-rolled one (host scipy residual + plan.solve, two
n-vectors over PCIe per step), at 128^3 Cholesky and at config 5 (79^3 unsymmetric stencil, LU with in-block pivoting).

    python tools/refine_timing.py --mode device --out profiles/r09_a_refine_timing.json
    python tools/refine_timing.py --mode host --root <checkout of the parent commit, built> --merge profiles/r09_a_refine_timing.json

--mode device needs this tree's library; --mode host only uses plan.solve, so it can run on
the parent commit's library: --root puts that checkout's package first on the path.  --merge adds the section to an existing file.
Expectation to compare with (not a pass/fail number): refine of k iterations = (k + 1) solves + (k + 1) residual passes, a pass
being small next to a solve."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["device", "host"], default="device")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--grid-chol", type=int, default=128)
ap.add_argument("--grid-lu", type=int, default=79)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--merge", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
sf = importlib.import_module("sparse-matrix-factorization-library_amd")


def cases():
    slot = int(sf.lib.sf_reference_slot_size(1, 288 << 30))
    M = args.grid_chol
    n, Cp, Ci, Cx = sf.gen.laplacian_lower(M, M, M)
    S = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(M, M, M, 3, 1), slot)
    plan = sf.CholPlan(S)
    plan.set_values(S.Lx)
    yield f"cholesky_lap3d_{M}", S, plan
    M = args.grid_lu
    n, Cp, Ci, Cx = sf.gen.unsymmetric_stencil(M, M, M, extra_per_row=0, seed=2024, drop=0.05)
    S = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(M, M, M, 3, 1), slot, "lu", False)
    plan = sf.LUPlan(S)
    plan.set_values(S.Lx, S.Ux)
    plan.set_pivoting(0.1)
    yield f"lu_config5_{M}_pivoting", S, plan


def host_matrix(S):
    """P A P^T as scipy CSR (one triangle mirrored, or L by column + U by row)"""
    import scipy.sparse as sp
    n = S.n
    lc = np.repeat(np.arange(n), np.diff(S.Lp))
    if S.method == "lu":
        ur = np.repeat(np.arange(n), np.diff(S.Up))
        off = S.Ui != ur
        return (sp.coo_matrix((S.Lx, (S.Li, lc)), shape=(n, n)) + sp.coo_matrix((S.Ux[off], (ur[off], S.Ui[off])), shape=(n, n))).tocsr()
    off = S.Li != lc
    return (sp.coo_matrix((S.Lx, (S.Li, lc)), shape=(n, n)) + sp.coo_matrix((S.Lx[off], (lc[off], S.Li[off])), shape=(n, n))).tocsr()


def best_of(fn, reps):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t) * 1e3)
    return min(out), r


result = {}
for name, S, plan in cases():
    n = S.n
    plan.factorize()
    b = 1.0 + np.arange(n) / n
    x = plan.solve(b)                      # warm-up
    solve_wall, x = best_of(lambda: plan.solve(b), args.reps)
    rec = {"n": int(n), "solve_wall_ms": solve_wall, "solve_device_ms": plan.stat("last_solve_ms")}
    if args.mode == "device":
        plan.refine(b, max_iter=2)         # builds the row form
        rec["bytes_refine"] = plan.stat("bytes_refine")
        wall, (xr, info) = best_of(lambda: plan.refine(b, max_iter=2, return_info=True), args.reps)
        rec.update(refine2_wall_ms=wall, refine2_device_ms=plan.stat("last_refine_ms"), refine2_iters=info["iters"],
                   refine2_berr0=info["berr0"], refine2_berr=info["berr"])
        res = []
        for _ in range(args.reps):
            plan.residual(b, x)
            res.append(plan.stat("last_residual_ms"))
        entries = plan.stat("refine_row_entries")
        # per entry: column index 4 B, position 8 B, value 8 B, x gather 8 B; per row: two pointers' worth 8 B, b 8 B, r and w 16 B
        bytes_pass = entries * 28.0 + n * 32.0
        rec.update(resid_kernel_ms=min(res), resid_row_entries=entries, resid_bytes_model=bytes_pass,
                   resid_bytes_per_s=bytes_pass / (min(res) * 1e-3) if min(res) > 0 else None)
    else:
        A = host_matrix(S)

        def two_steps():
            y = plan.solve(b)
            for _ in range(2):
                y = y + plan.solve(b - A @ y)
            return y

        wall, y = best_of(two_steps, args.reps)
        t_res, _ = best_of(lambda: b - A @ y, args.reps)
        r = A @ y - b
        rec.update(host_loop2_wall_ms=wall, host_residual_ms=t_res,
                   scaled_residual=float(np.abs(r).max() / (abs(A).sum(axis=0).max() * np.abs(y).max() + np.abs(b).max())))
    plan.close()
    result[name] = rec
    print(name, json.dumps(rec), flush=True)

doc = {}
if args.merge and os.path.exists(args.merge):
    with open(args.merge) as f:
        doc = json.load(f)
doc["device_loop" if args.mode == "device" else "host_loop_parent_library"] = result
dest = args.out or args.merge
if dest:
    with open(dest, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
