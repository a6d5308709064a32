"""Device time of sf_chol_plan_rowdel / _rowadd against a k = 1 update and a full factorization of the same plan, in one process
(DESIGN 8q):
    python tools/rowmod_timing.py [--size 128] [--repeats 5] [--out profiles/r11_a_rowmod_timing.json]
3-D 7-point Laplacian size^3 with the geometric nested dissection of bench.py.  Two rows -- the first column (the first leaf of the
ordering) and the first column of the last supernode (the root separator) -- and for each, after one warm-up pair, `repeats` pairs
of rowdel and rowadd of A's own column, so that the matrix returns to A every time; then `repeats` pairs of a k = 1 update and
downdate of a diagonal bump at the same row.  Recorded: "last_updown_ms" of every call (device events around the call's kernels;
rowadd's check launch and its read-back come before them and are not in it), the launches, the sweep's supernodes, the path.  The
baseline is "last_ms" of `repeats` factorizations of the same plan in the same run, after one warm-up.  Without a HIP device the
JSON says that nothing was measured."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sf = importlib.import_module("sparse-matrix-factorization-library_amd")


def own_column(sym, j):
    """(indices, values) of column j of the symmetric permuted matrix from its lower triangle (Lp, Li, Lx)"""
    Lp, Li, Lx = np.asarray(sym.Lp), np.asarray(sym.Li), np.asarray(sym.Lx)
    col = np.repeat(np.arange(sym.n), np.diff(Lp))
    left = np.flatnonzero((Li == j) & (col != j))
    idx = np.concatenate([col[left], Li[Lp[j]:Lp[j + 1]]])
    return idx.astype(np.int64), np.concatenate([Lx[left], Lx[Lp[j]:Lp[j + 1]]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_a_rowmod_timing.json"))
    a = ap.parse_args()
    N = a.size
    res = {"workload": f"3D 7-point Laplacian {N}^3 SPD Cholesky fp64, geometric ND", "repeats": a.repeats, "measured": False}
    if sf.device_count() < 1:
        res["note"] = "no HIP device: nothing was measured"
    else:
        n, Cp, Ci, Cx = sf.gen.laplacian_lower(N, N, N)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(N, N, N), sf.REFERENCE_SLOT_1GPU)
        Super = np.asarray(sym.Super)
        plan = sf.CholPlan(sym, device=0)
        plan.set_values(sym.Lx)
        fact = []
        for r in range(a.repeats + 1):
            plan.factorize()
            fact.append(plan.stat("last_ms"))
        fact = fact[1:]
        res.update(n=int(n), nsuper=int(sym.nsuper), factorize_ms=fact, factorize_ms_median=statistics.median(fact), cases=[])
        for kind, j in (("leaf", 0), ("root", int(Super[sym.nsuper - 1]))):
            idx, vals = own_column(sym, j)
            what = plan.rowmod_path(j, idx)
            dele, add, up, down, stats = [], [], [], [], {}
            for r in range(a.repeats + 1):
                plan.rowdel(j)
                dele.append(plan.stat("last_updown_ms"))
                stats["rowdel_launches"] = int(plan.stat("rowmod_launches"))
                plan.rowadd(j, idx, vals)
                add.append(plan.stat("last_updown_ms"))
                stats["rowadd_launches"] = int(plan.stat("rowmod_launches"))
            W = (np.array([0, 1]), np.array([j]), np.array([0.5 * np.sqrt(6.0)]))
            for r in range(a.repeats + 1):
                plan.update(W)
                up.append(plan.stat("last_updown_ms"))
                stats["update_launches"] = int(plan.stat("update_launches"))
                plan.update(W, downdate=True)
                down.append(plan.stat("last_updown_ms"))
            med = lambda v: statistics.median(v[1:])        # noqa: E731
            res["cases"].append({"kind": kind, "row": j, "rowdel_ms": dele[1:], "rowadd_ms": add[1:], "update_k1_ms": up[1:],
                                 "downdate_k1_ms": down[1:], "rowdel_ms_median": med(dele), "rowadd_ms_median": med(add),
                                 "update_k1_ms_median": med(up), "downdate_k1_ms_median": med(down),
                                 "row_panels": len(what["rows"]), "sweep_supernodes": len(what["sweep"]),
                                 "path_supernodes": len(what["update"]), **stats,
                                 "factorize_over_rowdel": statistics.median(fact) / med(dele),
                                 "factorize_over_rowadd": statistics.median(fact) / med(add)})
            print(json.dumps(res["cases"][-1]), flush=True)
        # the factor after all the pairs still is the factor of A, to rounding
        _, info = plan.refine(np.ones(n), max_iter=0, return_info=True)
        res["berr_after_all_pairs"] = info["berr0"]
        res["measured"] = True
        plan.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({key: res[key] for key in res if key != "cases"}))


if __name__ == "__main__":
    main()
