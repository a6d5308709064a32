"""GPU only: selected inversion (sf_chol_plan_selinv) of the resident 128^3 Cholesky factor.  Prints one JSON line: factorize
ms, last_selinv_ms, flops_selinv, the rate and its fraction of the 78.6 TFLOP/s fp64 MFMA peak, the wall time of logdet and
selinv_diag, and the bytes of the arena plus scratch."""
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

PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    if sf.device_count() < 1:
        raise SystemExit("selinv_timing: no HIP device")
    N = a.N
    n, Cp, Ci, Cx = gen.laplacian_lower(N, N, N)
    sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N, 3, 1), sf.REFERENCE_SLOT_1GPU)
    plan = sf.CholPlan(sym)
    plan.set_values(sym.Lx)
    plan.factorize()
    fact_ms = plan.stat("last_ms")
    ts = []
    for _ in range(a.reps):
        plan.selinv()
        ts.append(plan.stat("last_selinv_ms"))
    ms = float(min(ts))
    fl = plan.stat("flops_selinv")
    t0 = time.perf_counter()
    ld = plan.logdet()
    logdet_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    d = plan.selinv_diag()
    diag_ms = (time.perf_counter() - t0) * 1e3
    c = 2.0 * np.cos(np.arange(1, N + 1) * np.pi / (N + 1))
    lam = 6.0 - c[:, None, None] - c[None, :, None] - c[None, None, :]
    res = {"tool": "selinv_timing", "N": N, "n": n, "factorize_ms": round(fact_ms, 3), "selinv_ms": [round(t, 3) for t in ts],
           "last_selinv_ms": round(ms, 3), "flops_selinv": fl, "flops_exec_factorize": plan.stat("flops_exec"),
           "selinv_tflops": round(fl / ms * 1e-9, 2), "frac_of_78_6": round(fl / (ms * 1e-3) / PEAK, 4),
           "logdet_ms_wall": round(logdet_ms, 3), "selinv_diag_ms_wall": round(diag_ms, 3),
           "bytes_selinv": plan.stat("bytes_selinv"), "bytes_device": plan.stat("bytes_device"),
           "trace_rel_err": abs(float(d.sum()) - float(np.sum(1.0 / lam))) / float(np.sum(1.0 / lam)),
           "logdet_rel_err": abs(ld - float(np.sum(np.log(lam)))) / abs(float(np.sum(np.log(lam))))}
    plan.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
