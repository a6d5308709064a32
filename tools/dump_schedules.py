#!/usr/bin/env python3
"""Dumps, as JSON lines, everything the inspection ABI tells about the schedules of a fixed list of schedule-only plans (no device
needed): launch, segment, owner and solve-reduce tables, segment regions, panel offsets and the schedule statistics (floating-point
ones with repr, i.e. all bits).  Two builds whose dumps are byte-identical build the same schedules:

    python tools/dump_schedules.py --tree . > new.jsonl
    python tools/dump_schedules.py --tree ../other-checkout > old.jsonl && cmp old.jsonl new.jsonl

--tree names the checkout whose (built) package is loaded; the script uses nothing but sf.Schedule and the inspection calls."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

PKG = "sparse-matrix-factorization-library_amd"
STATS = ("levels", "launches", "gemm_tasks", "update_pairs", "flops_exec", "flops_update", "flops_update_small", "flops_panel_gemm",
         "flops_outer_gemm", "flops_tiles", "flops_tiles_update", "scatter_elems", "bytes_device", "download_pieces", "top_doubles",
         "stored_doubles")
KNOBS = ({"SF_LOOKAHEAD": "0"}, {"SF_TOP_OWNER": "1"}, {"SF_FUSE_MAX": "0"}, {"SF_DL_SLOT_MB": "1"})


def dump(name, plan, nsuper, out, **extra):
    rec = {"case": name, **extra}
    rec["launch_table"] = plan.launch_table().tolist()
    rec["segment_table"] = plan.segment_table().tolist()
    rec["segment_owner_table"] = plan.segment_owner_table().tolist()
    rec["segment_regions"] = [plan.segment_regions(k) for k in range(plan.num_segments())]
    rec["solve_reduce_table"] = plan.solve_reduce_table().tolist()
    rec["panel_offsets"] = plan.panel_offsets(nsuper).tolist()
    rec["stats"] = {s: repr(plan.stat(s)) for s in STATS}
    plan.close()
    out.write(json.dumps(rec, sort_keys=True) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--quick", action="store_true", help="leave out the 64^3 cases")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sf = importlib.import_module(PKG)
    sharded = importlib.import_module(PKG + ".sharded")
    gen, lib = sf.gen, importlib.import_module(PKG + "._lib").lib
    out = sys.stdout

    def laplacian(g, slot=1 << 30, levels=None):
        n, Cp, Ci, Cx = gen.laplacian_lower(g, g, g)
        perm = sf.grid_nd_perm(g, g, g) if levels is None else sf.grid_nd_perm(g, g, g, *levels)
        return sf.analyze(n, Cp, Ci, Cx, perm, slot)

    def in_core(name, sym):
        dump(name, sf.Schedule(sym, None, 0, 1, ooc_group=np.zeros(sym.nsuper, dtype=np.int32), ooc_ngroups=1), sym.nsuper, out)

    def mapped(name, sym, W, owner=None, lu=False):
        if owner is None:
            owner, _, _ = sf.subtree_partition(sym, W, 1.0 / W + sharded.TOP_CHAIN_SHARE)
        for r in range(W):
            dump(name, sf.Schedule(sym, owner, r, W, lu=lu), sym.nsuper, out, rank=r, nranks=W)

    def mapped_laplacian(g, W):      # the grids of tests/test_config4_schedules.py: the reference's slot size for W devices
        slot = int(lib.sf_reference_slot_size(W, 288 << 30))
        return laplacian(g, slot, (3, 1))

    # in-core Cholesky
    for g in (12, 40) + (() if args.quick else (64,)):
        in_core("chol_incore_%d^3" % g, laplacian(g))
    n, Cp, Ci, Cx = gen.stencil_spd_lower(300, 300)
    in_core("chol_incore_stencil_300x300", sf.analyze(n, Cp, Ci, Cx, None, 1 << 30))

    # mapped Cholesky, every rank
    for g, W in ((24, 2), (40, 4)) + (() if args.quick else ((64, 8),)):
        mapped("chol_mapped_%d^3_%d" % (g, W), mapped_laplacian(g, W), W)
    mapped("chol_mapped_12^3_7_more_ranks_than_subtrees", mapped_laplacian(12, 7), 7)
    n1, Cp1, Ci1, Cx1 = gen.laplacian_lower(6, 6, 6)
    Cp = np.concatenate([Cp1, Cp1[1:] + Cp1[-1], Cp1[1:] + 2 * Cp1[-1]])
    Ci = np.concatenate([Ci1, Ci1 + n1, Ci1 + 2 * n1])
    forest = sf.analyze(3 * n1, Cp, Ci, np.concatenate([Cx1, Cx1, Cx1]), None, 1 << 30)
    mapped("chol_mapped_forest_3x6^3_3", forest, 3, owner=sf.subtree_partition(forest, 3, 0.5)[0])

    # mapped LU, every rank: symmetric pattern (U aliases L) and an unsymmetric one
    for g, W in ((24, 2), (32, 4)):
        n, Cp, Ci, Cx = gen.laplacian_lower(g, g, g)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(g, g, g), 8 << 30, method="lu", symmetric=True)
        mapped("lu_sym_mapped_%d^3_%d" % (g, W), sym, W, lu=True)
        n, Cp, Ci, Cx = gen.unsymmetric_stencil(g, g, g, seed=5)
        sym = sf.analyze(n, Cp, Ci, Cx, sf.grid_nd_perm(g, g, g), 8 << 30, method="lu", symmetric=False)
        mapped("lu_unsym_mapped_%d^3_%d" % (g, W), sym, W, lu=True)

    # out-of-core Cholesky: budgets of 1/2 and 1/3 of the factor (top modes 1 and 2 at this size: the top panels resident only while
    # active) and of 3/5 and 3/4 (top mode 0: the whole top resident)
    sym = laplacian(40)
    total = int(((sym.Super[1:] - sym.Super[:-1]) * (sym.Lsip[1:] - sym.Lsip[:-1])).sum())
    modes = set()
    for num, den in ((1, 2), (1, 3), (3, 5), (3, 4)):
        cut = sf.ooc_partition(sym, total * num // den)
        modes.add(int(cut.top_mode))
        dump("chol_ooc_40^3_budget_%d/%d" % (num, den), sf.Schedule(sym, None, 0, 1, ooc_group=cut[0], ooc_ngroups=cut[1], ooc_top_mode=cut.top_mode),
             sym.nsuper, out, ngroups=int(cut[1]), top_mode=int(cut.top_mode))
    assert 0 in modes and max(modes) >= 1, modes

    # creation-time knobs: 40^3 / 4 mapped and 40^3 in core again
    sym_m, sym_i = mapped_laplacian(40, 4), laplacian(40)
    for env in KNOBS:
        (k, v), = env.items()
        os.environ[k] = v
        try:
            mapped("chol_mapped_40^3_4_%s=%s" % (k, v), sym_m, 4)
            in_core("chol_incore_40^3_%s=%s" % (k, v), sym_i)
        finally:
            del os.environ[k]


if __name__ == "__main__":
    main()
