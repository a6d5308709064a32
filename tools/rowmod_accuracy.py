"""What rowadd's one-term-at-a-time sweep costs in accuracy against a factorization:
    python tools/rowmod_accuracy.py [--case arrow_900_200] [--out profiles/r11_b_rowmod_sweep_accuracy.json]
The case is one of tests/util.py's (the helpers of tests/ are imported from there).  Rows: those the tests try (rowmod_ref.rows_to_try),
the first column of the last supernode and the last two rows.  Per row, with the measure of the tests -- the backward error
|L L^T - A|_F / |A|_F in longdouble:
    emulated   tests/rowmod_ref.py's rowadd of A's own column onto the fp64 numpy Cholesky factor of A' (row and column j the
               identity's), over the error of the fp64 numpy factor of A, and over that of the longdouble factor rounded to fp64 (the
               denominator of tests/test_rowmod_ref.py)
    device     CholPlan.rowadd onto the plan's factorization of A', over the error of the same plan's factorization of A; rowdel of
               the factor of A over the error of the plan's factorization of A'
Without a HIP device only the emulated figures are written."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sf = importlib.import_module("sparse-matrix-factorization-library_amd")
import rowmod_ref as rr         # noqa: E402
import updown_ref as ur         # noqa: E402
from util import small_cases, wide_cases        # noqa: E402


def panels_fp64(st, A):
    """the fp64 numpy Cholesky factor of A in the supernodal layout"""
    L = np.linalg.cholesky(A)
    out = np.zeros(st.xsize)
    for s in range(st.nsuper):
        P, c0 = st.panel(out, s), int(st.Super[s])
        for c in range(st.nscol(s)):
            P[c:, c] = L[st.rows(s)[c:], c0 + c]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="arrow_900_200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_b_rowmod_sweep_accuracy.json"))
    a = ap.parse_args()
    _, n, Cp, Ci, Cx, perm, slot = next(c for c in small_cases() + wide_cases() if c[0] == a.case)
    sym = sf.analyze(n, Cp, Ci, Cx, perm, slot)
    st, A = ur.Structure(sym), ur.dense_matrix(sym)
    e_ld = ur.backward_error(st, ur.chol_panels(sym, st, A), A)
    e_64 = ur.backward_error(st, panels_fp64(st, A), A)
    gpu = sf.device_count() >= 1
    res = {"case": a.case, "n": int(n), "nsuper": int(st.nsuper), "error_longdouble_factor": e_ld, "error_fp64_numpy_factor": e_64,
           "device": gpu, "rows": []}

    def plan_factor(M):
        plan = sf.CholPlan(sym, device=0)
        plan.set_values(ur.values_of(sym, M))
        plan.factorize()
        return plan

    if gpu:
        plan = plan_factor(A)
        res["error_plan_factor"] = e_plan = ur.backward_error(st, plan.get_factor(), A)
        plan.close()
    rows = rr.rows_to_try(st, 0) + [int(st.Super[st.nsuper - 1]), n - 2, n - 1]
    for j in sorted(set(r for r in rows if 0 <= r < n)):
        A1 = rr.deleted(A, j)
        idx, vals = rr.column_of(st, A, j)
        La, failed, what = rr.rowadd_emulate(st, panels_fp64(st, A1), j, idx, vals)
        e = ur.backward_error(st, La, A)
        s, c = rr.locate(st, j)
        row = {"row": j, "sweep_supernodes": len(what["sweep"]),
               "sweep_columns": int(sum(st.nscol(p) for p in what["sweep"]) + c), "update_path_supernodes": len(what["update"]),
               "emulated_rowadd_over_fp64_factor": e / e_64, "emulated_rowadd_over_longdouble_factor": e / e_ld}
        if gpu:
            plan = plan_factor(A1)
            e_del_ref = ur.backward_error(st, plan.get_factor(), A1)
            plan.rowadd(j, idx, vals)
            row["device_rowadd_over_plan_factor"] = ur.backward_error(st, plan.get_factor(), A) / e_plan
            plan.close()
            plan = plan_factor(A)
            plan.rowdel(j)
            row["device_rowdel_over_plan_factor"] = ur.backward_error(st, plan.get_factor(), A1) / e_del_ref
            plan.close()
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
