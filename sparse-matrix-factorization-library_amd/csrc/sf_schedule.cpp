// The schedule of the supernodal Cholesky / LU numeric factorization: everything that is decided once per pattern -- the panel
// layout, the launch list and its task tables, the solve and download schedules.  Host code only, no HIP (sf_schedule.h);
// sf_plan_build.hip creates the device resources that hold what is built here.
//
// Replaces the reference's task-queue scheduler and GPU branch (Cholesky/Source/SparseFrame.c:2150-3017).
// The reference is left-looking with descendant lists, one supernode at a time, every panel staged over
// PCIe (C:2345-2954).  Here the whole factor stays resident in HBM and the elimination tree is swept
// level by level (level = height above the leaves in the supernodal tree, parent as in C:2247):
//
//   memset(Lsx) ; k_load_panels                                          (loadA, C:1998-2028)
//   for level l = 0 .. L-1:
//       for every outer block column J (512 columns) of the panels of the level:
//           k_gemm<0>      left-looking update of the block column by all columns to its left (K = J)
//           for t = 0 .. 7:                            64-column steps inside the block, also left-looking
//               k_gemm<0>      update of block column t by block columns 0..t-1 of this outer block (K = 64 t)
//               k_potrf_block  64x64 diagonal block of every panel that still has one
//               k_trsm_block   rows below that block
//       k_gemm<1>          every (supernode of the level -> ancestor) Schur update, scatter fused
//
// A supernode's updates are pushed to all its ancestors as soon as it is factored (right-looking);
// the sums are the same as the reference's left-looking sums, applied in a different order, so the
// factor agrees to rounding (the reference itself is order-nondeterministic: qsort + atomicAdd).
// All task tables depend on the structure only and are built once at plan creation.
#include "sf_schedule.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <time.h>
#include <vector>

#include "sf_symbolic.h"

// ---------------- every environment knob of plan creation ----------------
static bool exp_on(const char* name) {          // experiment switch that is ON unless set to 0 (EXP builds only)
    const char* env = sf_exp_env(name);
    return !(env && atoi(env) == 0);
}

PlanKnobs read_knobs() {
    PlanKnobs k;
    k.trace = getenv("SF_TRACE") != nullptr;
    if (const char* env = sf_exp_env("SF_SU_MAXK")) k.su_maxk = atoi(env);
    if (const char* env = getenv("SF_FUSE_MAX")) k.fuse_max = strtoll(env, nullptr, 10);
    if (const char* env = getenv("SF_LOOKAHEAD")) k.lookahead = atoi(env) != 0;
    if (const char* env = getenv("SF_GRAPH")) k.use_graph = atoi(env) != 0;
    if (const char* env = getenv("SF_TOP_OWNER")) k.top_owner = atoi(env) != 0;
    k.solve_diagT = exp_on("SF_SOLVE_DIAGT");
    k.solve_bwd_ahead = exp_on("SF_SOLVE_BWD_AHEAD");
    k.solve_bwd_fused = exp_on("SF_SOLVE_BWD_FUSED");
    k.solve_fwd_ahead = exp_on("SF_SOLVE_FWD_AHEAD");
    k.solve_fwd_far_first = exp_on("SF_SOLVE_FWD_FAR_FIRST");
    if (const char* env = sf_exp_env("SF_SOLVE_FAR_WGS")) k.solve_far_wgs = std::max(1, atoi(env));
    if (const char* env = sf_exp_env("SF_SOLVE_FAR_GROUPS")) k.solve_far_groups = std::max(1, std::min(64, atoi(env)));
    if (const char* env = getenv("SF_DL_WORKERS")) k.dl_workers = k.dl_workers_fresh = std::max(1, std::min(DL_WORKERS_MAX, atoi(env)));
    k.dl_host_wait = exp_on("SF_DL_HOST_WAIT");
    if (const char* env = getenv("SF_DL_SLOT_MB")) k.dl_slot = (int64_t)std::max(1, atoi(env)) << 17;
    k.dl_2d = exp_on("SF_DL_2D");
    if (const char* env = sf_exp_env("SF_DL_LU_PACK")) k.dl_lu_pack = atoi(env) != 0;
    k.stream_priority = exp_on("SF_STREAM_PRIORITY");
    k.gemm_dynamic = exp_on("SF_GEMM_DYNAMIC");
    if (const char* env = getenv("SF_LU_PIVOT_TOL")) {
        k.piv_tol = std::min(1.0, std::max(0.0, atof(env)));
        if (k.piv_tol > 0.0) k.piv_perturb = 1.4901161193847656e-08;      // sqrt(eps): pivoting comes with its fallback
    }
    if (const char* env = getenv("SF_LU_PERTURB")) k.piv_perturb = std::max(0.0, atof(env));
    return k;
}

static double now_ms() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec / 1e6; }

// ---------------- argument checks (the device's are plan_create's own, right after these) ----------------
int sf_schedule_check_arguments(const PlanInput& in) {
    if (in.nranks < 1 || in.nranks > 32 || in.rank < 0 || in.rank >= in.nranks || (in.nranks > 1 && !in.phase_in)) return SF_ERR_ARG;
    if (in.ooc() && (in.nranks != 1 || in.phase_in || in.ooc_ngroups > 32767)) return SF_ERR_ARG;
    if (in.n < 0 || in.nsuper < 0 || !in.Super || !in.Lsip || !in.Lsxp || !in.Lp || (in.n > 0 && (!in.SuperMap || !in.Lsi || !in.Li))) return SF_ERR_ARG;
    if (in.n >= (sf_long)0x7fffffff) return SF_ERR_ARG;   // device row indices are 32-bit
    return SF_OK;
}

// ---------------- panel layout: phases, groups of ranks, device offsets ----------------
int sf_schedule_layout(const PlanInput& in, SfSchedule& p, Layout& lay) {
    p.dry = in.dry;
    p.lu = in.lu;
    p.rank = in.rank;
    p.nranks = in.nranks;
    p.n = in.n;
    p.nsuper = in.nsuper;
    p.nnz = in.Lp[in.n];
    p.isize = in.Lsip[in.nsuper];
    p.xsize = in.Lsxp[in.nsuper];
    p.u_alias = in.lu && (!in.Up || !in.Ui);
    p.unz = (in.lu && !p.u_alias) ? in.Up[in.n] : 0;
    // Device offsets of the nsrow x nscol panels: the owned (phase 0) panels in supernode order, then the top
    // (phase 1) panels, contiguous, so that the multi-GPU merge is ONE all-reduce over [top_off, top_off+top_size).
    // With no phase array every supernode is phase 0 and the layout is the reference's Lsxp (Cholesky).
    p.phase.assign(in.nsuper, 0);
    if (in.ooc()) {
        for (sf_long s = 0; s < in.nsuper; ++s) {
            if (in.ooc_group[s] < -1 || in.ooc_group[s] >= in.ooc_ngroups) return SF_ERR_ARG;
            p.phase[s] = in.ooc_group[s] < 0 ? 1 : 0;
        }
        p.ooc_groups = in.ooc_ngroups;
    }
    if (in.phase_in)
        for (sf_long s = 0; s < in.nsuper; ++s) {
            if (in.phase_in[s] < -1 || in.phase_in[s] > 1) return SF_ERR_ARG;
            p.phase[s] = (int8_t)in.phase_in[s];
        }
    // group of every top supernode stored here: mask, this rank's index in it and its size
    lay.all_ranks = in.nranks >= 32 ? 0xffffffffu : ((1u << in.nranks) - 1u);
    lay.gmask.assign(in.nsuper, 0);
    for (sf_long s = 0; s < in.nsuper; ++s) {
        if (p.phase[s] != 1) continue;
        const uint32_t m = (in.top_mask && in.nranks > 1) ? (in.top_mask[s] & lay.all_ranks) : lay.all_ranks;
        if (!((m >> in.rank) & 1u)) return SF_ERR_ARG;      // a stored top supernode must list this rank
        lay.gmask[s] = m;
    }
    if (in.top_mask && in.nranks > 1) {
        for (sf_long s = 0; s < in.nsuper; ++s)
            if (in.top_mask[s] & lay.all_ranks) p.all_masks.push_back(in.top_mask[s] & lay.all_ranks);
        std::sort(p.all_masks.begin(), p.all_masks.end());
        p.all_masks.erase(std::unique(p.all_masks.begin(), p.all_masks.end()), p.all_masks.end());
    } else if (in.nranks > 1) {
        p.all_masks.push_back(lay.all_ranks);
    }
    lay.rank = in.rank;
    lay.XP.assign(in.nsuper + 1, -1);
    if (in.ooc()) {
        // two buffers of the largest group's size, then the top; group g's panels from the start of buffer g & 1
        std::vector<int64_t> gsz((size_t)in.ooc_ngroups, 0);
        for (sf_long s = 0; s < in.nsuper; ++s)
            if (in.ooc_group[s] >= 0) gsz[(size_t)in.ooc_group[s]] += in.nscol(s) * in.nsrow(s);
        p.ooc_buf = *std::max_element(gsz.begin(), gsz.end());
        std::vector<int64_t> run((size_t)in.ooc_ngroups);
        for (int g = 0; g < in.ooc_ngroups; ++g) run[(size_t)g] = (g & 1) * p.ooc_buf;
        int64_t top = 2 * p.ooc_buf;
        p.top_off = top;
        if (in.ooc_top_mode >= 1) {
            p.ooc_first.assign((size_t)std::max<sf_long>(in.nsuper, 1), 0);
            p.ooc_last.assign((size_t)std::max<sf_long>(in.nsuper, 1), 0);
            std::vector<int64_t> toff((size_t)std::max<sf_long>(in.nsuper, 1), -1);
            std::vector<int32_t> twait((size_t)std::max<sf_long>(in.nsuper, 1), -1);
            int64_t arena = 0;
            if (in.ooc_top_mode > 2 || sf::ooc_top_layout(in.nsuper, in.Super, in.SuperMap, in.Lsip, in.Lsi, in.ooc_group, in.ooc_ngroups, in.ooc_top_mode, p.ooc_first.data(),
                                                       p.ooc_last.data(), toff.data(), twait.data(), &arena))
                return SF_ERR_ARG;
            // the group whose copies have to be over before group g's first launch may write: g - 2 for its buffer, later ones for the
            // places of the top panels that start with it (mode 2)
            p.ooc_wait.assign((size_t)in.ooc_ngroups, -1);
            for (int g = 0; g < in.ooc_ngroups; ++g) p.ooc_wait[(size_t)g] = g - 2;
            for (sf_long s = 0; s < in.nsuper; ++s)
                if (in.ooc_group[s] < 0) p.ooc_wait[(size_t)p.ooc_first[(size_t)s]] = std::max(p.ooc_wait[(size_t)p.ooc_first[(size_t)s]], twait[(size_t)s]);
            for (sf_long s = 0; s < in.nsuper; ++s) {
                if (in.ooc_group[s] >= 0) { int64_t& r = run[(size_t)in.ooc_group[s]]; lay.XP[s] = r; r += in.nscol(s) * in.nsrow(s); }
                else lay.XP[s] = top + toff[(size_t)s];
            }
            top += arena;
        } else {
            for (sf_long s = 0; s < in.nsuper; ++s) {
                int64_t& r = in.ooc_group[s] >= 0 ? run[(size_t)in.ooc_group[s]] : top;
                lay.XP[s] = r;
                r += in.nscol(s) * in.nsrow(s);
            }
        }
        p.ooc_top_mode = in.ooc_top_mode >= 1 ? in.ooc_top_mode : 0;
        p.top_size = top - p.top_off;
        p.xC = top;
        lay.XP[in.nsuper] = top;
    } else {
        int64_t run = 0;
        for (int ph = 0; ph < 2; ++ph) {
            if (ph == 1) p.top_off = run;
            for (sf_long s = 0; s < in.nsuper; ++s)
                if (p.phase[s] == ph) { lay.XP[s] = run; run += in.nscol(s) * in.nsrow(s); }
        }
        p.top_size = run - p.top_off;
        p.xC = run;
        lay.XP[in.nsuper] = run;
    }
    p.h_XP = lay.XP;
    for (sf_long s = 0; s < in.nsuper; ++s)
        if (p.phase[s] != 0) p.partial = true;
    if (in.load_top != 1) p.partial = true;
    if (in.ooc()) p.partial = true;         // (also without a top -- a forest: the panels sit at aliased offsets, and there is no resident factor)
    lay.ushift = p.xC;
    return SF_OK;
}

// ---------------- validate the structure the kernels index with ----------------
// SF_ERR_ARG, or the drop lists of the load maps (p.load_dropL / load_dropU)
static int validate_structure(const PlanInput& in, SfSchedule& p) {
    // (row indices and SuperMap: 10^8 entries at 128^3 -- a few threads over ranges of supernodes; the pointer arrays first, alone)
    std::atomic<bool> bad{false};
    for (sf_long s = 0; s < in.nsuper; ++s) {
        const sf_long nscol = in.nscol(s), nsrow = in.nsrow(s);
        const sf_long want = in.lu ? nscol * (2 * nsrow - nscol) : nscol * nsrow;
        if (nscol <= 0 || nsrow < nscol || in.Lsxp[s + 1] - in.Lsxp[s] != want || nsrow >= (sf_long)0x7fffffff || in.Lsip[s] < 0) bad = true;
    }
    if (bad || in.Super[0] != 0 || in.Super[in.nsuper] != in.n) return SF_ERR_ARG;
    for (sf_long j = 0; j < in.n; ++j)
        if (in.Lp[j] < 0 || in.Lp[j + 1] < in.Lp[j] || (in.lu && in.Up && in.Ui && (in.Up[j] < 0 || in.Up[j + 1] < in.Up[j]))) bad = true;
    if (bad) return SF_ERR_ARG;
    // Matrix entries: every (i, j) of column j of supernode s must have a place in its panel -- i >= Super[s], and i is a
    // column of s or one of its rows below (the assembly kernels search the row list and would store a foreign row somewhere
    // else).  An entry given twice resolves to the LAST one, as in the reference's sequential loadA (C:2009-2020): the earlier
    // ones are collected in drop[] and taken out of the load map, whose entries are stored in parallel.
    std::vector<std::vector<int64_t>> dropL_t, dropU_t;
    auto check_entries = [&](const sf_long* Cp, const sf_long* Ci, sf_long s, std::vector<int32_t>& seen_col, std::vector<int64_t>& seen_p,
                             std::vector<int64_t>& drop) {
        const sf_long c0 = in.Super[s], c1 = in.Super[s + 1], nscol = c1 - c0, nsrow = in.nsrow(s);
        const sf_long* below = in.Lsi + in.Lsip[s] + nscol;
        if ((sf_long)seen_col.size() < nsrow) { seen_col.assign((size_t)nsrow, -1); seen_p.resize((size_t)nsrow); }
        for (sf_long j = c0; j < c1; ++j) {
            for (sf_long q = Cp[j]; q < Cp[j + 1]; ++q) {
                const sf_long i = Ci[q];
                if (i < c0 || i >= in.n) return false;
                sf_long si = i - c0;
                if (i >= c1) {
                    const sf_long* it = std::lower_bound(below, below + (nsrow - nscol), i);
                    if (it == below + (nsrow - nscol) || *it != i) return false;
                    si = nscol + (it - below);
                }
                if (seen_col[(size_t)si] == (int32_t)j) drop.push_back(seen_p[(size_t)si]);
                seen_col[(size_t)si] = (int32_t)j;
                seen_p[(size_t)si] = q;
            }
        }
        return true;
    };
    auto check_range = [&](sf_long s0, sf_long s1, int t) {
        std::vector<int32_t> seen_col;
        std::vector<int64_t> seen_p;
        for (sf_long s = s0; s < s1 && !bad.load(std::memory_order_relaxed); ++s) {
            const sf_long nscol = in.nscol(s), nsrow = in.nsrow(s);
            for (sf_long k = 0; k < nsrow; ++k) {
                const sf_long g = in.Lsi[in.Lsip[s] + k];
                const bool ok = (k < nscol) ? (g == in.Super[s] + k) : (g > in.Lsi[in.Lsip[s] + k - 1] && g < in.n);
                if (!ok) { bad = true; return; }
            }
            // SuperMap indexes level[] / phase[] below: it must be the inverse of Super (foreign arrays: checked, not trusted)
            for (sf_long j = in.Super[s]; j < in.Super[s + 1]; ++j)
                if (in.SuperMap[j] != s) { bad = true; return; }
            if (!check_entries(in.Lp, in.Li, s, seen_col, seen_p, dropL_t[(size_t)t])) { bad = true; return; }
            if (in.lu && in.Up && in.Ui) {
                std::fill(seen_col.begin(), seen_col.end(), -1);
                if (!check_entries(in.Up, in.Ui, s, seen_col, seen_p, dropU_t[(size_t)t])) { bad = true; return; }
            }
        }
    };
    const int64_t work = (int64_t)in.Lsip[in.nsuper] + in.n + in.Lp[in.n] + ((in.lu && in.Up && in.Ui) ? in.Up[in.n] : 0);
    const int T = work < (1 << 22) ? 1 : (int)std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency()));
    dropL_t.resize((size_t)T);
    dropU_t.resize((size_t)T);
    if (T == 1) check_range(0, in.nsuper, 0);
    else {
        std::vector<std::thread> th;
        sf_long s0 = 0;
        for (int t = 0; t < T; ++t) {       // equal shares of the row-index array
            const int64_t upto = (int64_t)in.Lsip[in.nsuper] * (t + 1) / T;
            sf_long s1 = (t == T - 1) ? in.nsuper : (sf_long)(std::upper_bound(in.Lsip + s0, in.Lsip + in.nsuper, (sf_long)upto) - in.Lsip);
            s1 = std::min(std::max(s1, s0), in.nsuper);
            th.emplace_back(check_range, s0, s1, t);
            s0 = s1;
        }
        for (std::thread& t : th) t.join();
    }
    if (bad) return SF_ERR_ARG;
    for (auto& d : dropL_t) p.load_dropL.insert(p.load_dropL.end(), d.begin(), d.end());
    for (auto& d : dropU_t) p.load_dropU.insert(p.load_dropU.end(), d.begin(), d.end());
    return SF_OK;
}

// ---------------- levels of the supernodal tree; sharding and out-of-core consistency ----------------
static int tree_levels(const PlanInput& in, SfSchedule& p) {
    p.level_of.assign(in.nsuper, 0);
    p.nlevels = in.nsuper > 0 ? 1 : 0;
    for (sf_long s = 0; s < in.nsuper; ++s) {
        const sf_long nscol = in.nscol(s), nsrow = in.nsrow(s);
        if (nscol < nsrow) {
            const sf_long par = in.SuperMap[in.Lsi[in.Lsip[s] + nscol]];
            if (par <= s) return SF_ERR_ARG;   // must be postordered
            p.level_of[par] = std::max(p.level_of[par], p.level_of[s] + 1);
            p.nlevels = std::max(p.nlevels, p.level_of[par] + 1);
        }
    }
    // sharding consistency: every row of a stored supernode must belong to a stored supernode (its updates have
    // a local target), and a top supernode only has top ancestors
    for (sf_long s = 0; s < in.nsuper && (in.phase_in || in.ooc()); ++s) {         // (nothing to check when every supernode is simply stored: 10^8 row indices at 128^3)
        if (p.phase[s] < 0) continue;
        const sf_long nscol = in.nscol(s), nsrow = in.nsrow(s);
        for (sf_long k = nscol; k < nsrow; ++k) {
            // out of core: a streamed supernode only updates panels of its own group (alive in the same buffer) or of the resident top
            if (in.ooc() && in.ooc_group[s] >= 0) {
                const int32_t ga = in.ooc_group[in.SuperMap[in.Lsi[in.Lsip[s] + k]]];
                if (ga >= 0 && ga != in.ooc_group[s]) return SF_ERR_ARG;
            }
            const int8_t pa = p.phase[in.SuperMap[in.Lsi[in.Lsip[s] + k]]];
            if (pa < 0 || (p.phase[s] == 1 && pa != 1)) return SF_ERR_ARG;
        }
    }
    return SF_OK;
}

// ---------------- the level sets of the sweep, in the order they run ----------------
static std::vector<LevelSet> level_sets(const PlanInput& in, const Layout& lay, const SfSchedule& p) {
    std::vector<LevelSet> sets;
    if (in.ooc()) {      // out of core: the groups one after the other, each with its own level sets (then the top, below)
        std::vector<std::vector<std::vector<sf_long>>> by_gl((size_t)in.ooc_ngroups);
        for (sf_long s = 0; s < in.nsuper; ++s)
            if (in.ooc_group[s] >= 0) {
                auto& bl = by_gl[(size_t)in.ooc_group[s]];
                if ((int)bl.size() <= p.level_of[s]) bl.resize((size_t)p.level_of[s] + 1);
                bl[(size_t)p.level_of[s]].push_back(s);
            }
        std::vector<std::vector<std::vector<sf_long>>> top_gl((size_t)in.ooc_ngroups);      // mode 1: the top supernodes by (last group below, level)
        if (in.ooc_top_mode >= 1)
            for (sf_long s = 0; s < in.nsuper; ++s)
                if (in.ooc_group[s] < 0) {
                    auto& bl = top_gl[(size_t)p.ooc_last[(size_t)s]];
                    if ((int)bl.size() <= p.level_of[s]) bl.resize((size_t)p.level_of[s] + 1);
                    bl[(size_t)p.level_of[s]].push_back(s);
                }
        for (int g = 0; g < in.ooc_ngroups; ++g) {
            for (auto& v : by_gl[(size_t)g])
                if (!v.empty()) { sets.push_back(LevelSet{0, std::move(v), 0, 0, 1}); sets.back().group = g; }
            for (auto& v : top_gl[(size_t)g])
                if (!v.empty()) sets.push_back(LevelSet{1, std::move(v), lay.all_ranks, 0, 1});
        }
        // (Measured and not kept: every top supernode right after the last group below it -- the lower separators factorized and
        // on their way to the host while later groups still stream.  128^3 with 8 groups: 0.69 s against 0.60 s with the top at the end:
        // a top supernode then runs alone instead of with its level, and it delays the next group, whose download is what the
        // group phase is bound by.)
    }
    for (int ph = in.ooc() ? 1 : 0; ph < 2 && !(in.ooc() && in.ooc_top_mode >= 1); ++ph) {
        std::vector<std::vector<sf_long>> by_level(p.nlevels);
        for (sf_long s = 0; s < in.nsuper; ++s)
            if (p.phase[s] == ph) by_level[p.level_of[s]].push_back(s);
        for (int l = 0; l < p.nlevels; ++l) {
            if (by_level[l].empty()) continue;
            if (ph == 0) { sets.push_back(LevelSet{0, by_level[l], 0, 0, 1}); continue; }
            std::vector<uint32_t> ms;
            for (sf_long s : by_level[l]) ms.push_back(lay.gmask[s]);
            std::sort(ms.begin(), ms.end());
            ms.erase(std::unique(ms.begin(), ms.end()), ms.end());
            for (uint32_t m : ms) {
                LevelSet LS{1, {}, m, lay.group_idx(m), __builtin_popcount(m)};
                LS.lo = (double)LS.share_idx / LS.share_cnt;
                LS.hi = (double)(LS.share_idx + 1) / LS.share_cnt;
                if (in.root_cum && LS.share_cnt == in.nranks && in.nranks > 1) { LS.lo = in.root_cum[in.rank]; LS.hi = in.root_cum[in.rank + 1]; }
                for (sf_long s : by_level[l])
                    if (lay.gmask[s] == m) LS.sn.push_back(s);
                sets.push_back(std::move(LS));
            }
        }
    }
    return sets;
}

// ---------------- factorization schedule ----------------
// Tiles of one problem are emitted in "supertile" order: blocks of (up to) 8 tile columns x 8 tile rows.
// The kernel hands each XCD a contiguous run of tasks, so the ~64 workgroups resident on one XCD at a
// time work on one supertile and march through K together: per K step they touch 8 + 8 operand slices
// instead of 1 + 64, i.e. each slice is fetched into that XCD's L2 once and re-used 8 times.
// A task = one tile over one slice of its problem's K range, emitted slice by slice (the kernel deals consecutive tasks
// out in rounds, so a round would be 512 adjacent tiles over the SAME K range).  Measured at 128^3 on one box: no
// slicing 556 ms; slices of 512 / 256 / 128 steps 563 / 569 / 569 ms -- every extra slice is one more atomic pass over
// the target tile, which costs more than the extra rounds gain.  GEMM_SLICE is therefore "never" (one slice).
// kt_lo / kt_hi: the K steps [kt_lo, kt_hi) of the problem only (look-ahead: the far part and the last block's part of an outer
// GEMM are separate launches); default = all of K
static void add_tiles(PlanTables& T, SfSchedule& p, int32_t prob_id, int kt_lo = 0, int kt_hi = -1) {
    const int M = T.probs[prob_id].M, N = T.probs[prob_id].N, K = T.probs[prob_id].K;
    const int gemm_slice = sf::GEMM_SLICE;
    const int tmn = (M + sf::GEMM_BM - 1) / sf::GEMM_BM, tnn = (N + sf::GEMM_BN - 1) / sf::GEMM_BN;
    const int sw = std::min(tnn, 8), sh = std::max(1, 64 / sw);
    const int nkt_all = kt_hi >= 0 ? kt_hi : (K + sf::GEMM_BK - 1) / sf::GEMM_BK;
    for (int k0 = kt_lo; k0 < nkt_all; k0 += gemm_slice)
    for (int sj = 0; sj < tnn; sj += sw)
        for (int si = 0; si < tmn; si += sh)
            for (int tn = sj; tn < std::min(sj + sw, tnn); ++tn)
                for (int tm = si; tm < std::min(si + sh, tmn); ++tm) {
                    // keep tiles that contain at least one element with ci >= cj
                    if ((tm + 1) * sf::GEMM_BM - 1 < tn * sf::GEMM_BN) continue;
                    T.gtasks.push_back(GemmTask{prob_id, (uint16_t)tm, (uint16_t)tn, (uint32_t)k0, (uint32_t)std::min(gemm_slice, nkt_all - k0)});
                    p.flops_tiles += 2.0 * sf::GEMM_BM * sf::GEMM_BN * sf::GEMM_BK * (double)std::min(gemm_slice, nkt_all - k0);
                }
}

// The problem g once per side -- side 0: the (L) panel, side 1 (LU): the U^T panel, with the two operand roles taken from the
// other panel each -- reading at `src` and writing at `dst` of the panel set.  Returns the index of the first; the sides are consecutive.
static int32_t push_sides(const PlanInput& in, const Layout& lay, PlanTables& T, GemmProb g, int64_t src, int64_t dst) {
    const int32_t first = (int32_t)T.probs.size();
    for (int side = 0; side < in.sides(); ++side) {
        g.y_off = src + (side ? lay.ushift : 0);
        g.x_off = src + ((in.lu && !side) ? lay.ushift : 0);
        g.c_off = dst + (side ? lay.ushift : 0);
        g.strict = (in.lu && !side) ? 1 : 0;
        T.probs.push_back(g);
    }
    return first;
}

// a launch of a set whose work is dealt out over the set's group of ranks (when it has more than one)
static void stamp_share(Launch& L, const LevelSet& LS, bool split) {
    L.split = split && LS.share_cnt > 1;
    L.share_idx = LS.share_idx; L.share_cnt = LS.share_cnt;
    L.share_lo = LS.lo; L.share_hi = LS.hi;
}

// additive updates split over the group, block columns reduced
static bool set_is_shared(const PlanInput& in, const LevelSet& LS) { return LS.ph == 1 && in.nranks > 1; }

// The left-looking update of the outer block at column J2: K steps [kt_lo, kt_hi) of its K = J2 columns (all of them:
// kt_hi < 0), one launch for the panels of the set; `split`: shared among the ranks of the group (its result is part of a
// sum that is reduced later) or executed in full by every rank (its target has already been reduced)
static void outer_gemm(const PlanInput& in, const Layout& lay, const LevelSet& LS, PlanTables& T, SfSchedule& p,
                       int J2, int kt_lo, int kt_hi, bool split) {
    const int64_t g0 = (int64_t)T.gtasks.size();
    for (sf_long s : LS.sn) {
        const int nscol = (int)in.nscol(s), nsrow = (int)in.nsrow(s);
        if (J2 >= nscol) continue;
        GemmProb g{};
        g.lda = nsrow; g.ldc = nsrow;
        g.M = nsrow - J2; g.N = std::min(sf::OUTER_NB, nscol - J2); g.K = J2;
        const int64_t src = lay.XP[s] + J2;                    // rows J2.. , columns 0..J2-1
        const int64_t dst = lay.XP[s] + J2 + (int64_t)J2 * nsrow;
        const double kk = (kt_hi < 0 ? g.K : (kt_hi - kt_lo) * sf::GEMM_BK);
        const double fl = (double)g.N * (g.N + 1) * kk + 2.0 * (g.M - g.N) * (double)g.N * kk;
        const int32_t first = push_sides(in, lay, T, g, src, dst);
        for (int32_t id = first; id < (int32_t)T.probs.size(); ++id) {
            p.flops_outer_gemm += fl; p.flops_panel_gemm += fl;
            add_tiles(T, p, id, kt_lo, kt_hi);
        }
    }
    if ((int64_t)T.gtasks.size() > g0) {
        p.launches.push_back(Launch{LAUNCH_GEMM_OUTER, g0, (int)(T.gtasks.size() - g0)});
        stamp_share(p.launches.back(), LS, split);
        p.launches.back().whole_tiles = set_is_shared(in, LS) && !split && LS.share_cnt > 1;      // replicated inside a group: reproducible
    }
}

// reduce point: block column jo (at column J) of every panel of the set is complete up to the sum over the group's ranks
static void reduce_point(const PlanInput& in, const Layout& lay, const LevelSet& LS, SfSchedule& p, int jo, bool ahead) {
    const int J = jo * sf::OUTER_NB;
    if (!p.segments.empty()) p.segments.back().l1 = p.launches.size();
    Segment sg;
    sg.mask = LS.mask;
    sg.l0 = p.launches.size();
    for (sf_long s : LS.sn) {
        const int64_t nscol = in.nscol(s), nsrow = in.nsrow(s);
        if (J >= nscol) continue;
        const int64_t w = std::min<int64_t>(sf::OUTER_NB, nscol - J);
        for (int side = 0; side < in.sides(); ++side) {         // LU: the L panel and the U^T panel
            const int64_t base = lay.XP[s] + (side ? lay.ushift : 0);
            sg.off.push_back(base + (int64_t)J * nsrow);
            sg.cnt.push_back(w * nsrow);
            sg.src.push_back(base + (int64_t)J * nsrow + J);
            sg.rows.push_back(nsrow - J);
            sg.cols.push_back(w);
            sg.ld.push_back(nsrow);
            sg.packed += (nsrow - J) * w;
        }
    }
    sg.early = ahead && jo > 0;
    // owner-computes prototype: the sets EVERY rank takes part in (the root separator), look-ahead schedule only
    if (p.top_owner && ahead && LS.share_cnt == in.nranks) sg.owner_gi = jo % LS.share_cnt;
    p.segments.push_back(std::move(sg));
}

// what the sweep carries from one level set to the next
struct SweepState {
    bool split_set = false;
    int ooc_open = -1;                  // out of core: the group whose (zero + assemble) launch has been issued last
    // LU fused steps: the step for which panel s's diagonal block last received its pre-update (outer block * 16 + step)
    std::vector<int32_t> pre_updated;
};

// Latency-bound step at column `diag` (step ti of the outer block jo at column J): the (update, POTRF / GETRF, TRSM) triple is
// ONE launch of k_step.  Steps with more tiles are throughput-bound and keep the three launches (three_launch_step).
static int fused_step(const PlanInput& in, const Layout& lay, const LevelSet& LS, SweepState& sw, PlanTables& T, SfSchedule& p,
                      int jo, int ti, int diag) {
    const bool lu = in.lu;
    const int J = jo * sf::OUTER_NB, ninner = sf::OUTER_NB / sf::NB;
    const int64_t ushift = lay.ushift;
    const std::vector<int64_t>& XP = lay.XP;
    std::vector<StepTask>& steps = T.steps;
    const int64_t d0 = (int64_t)steps.size();
    std::vector<int32_t> flag_of, slot_of;
    for (sf_long s : LS.sn) {
        const int nscol = (int)in.nscol(s), nsrow = (int)in.nsrow(s);
        if (diag >= nscol) { flag_of.push_back(-1); slot_of.push_back(-1); continue; }
        const int b = std::min(sf::NB, nscol - diag);
        flag_of.push_back(T.n_flags);
        // (the two halves of an LU diagonal block's update are tied together here, not by convention: a diagonal task that
        // applies only the last 64 columns must find the pre-update task of the launch before it)
        if (lu && ti >= 2 && sw.pre_updated[(size_t)s] != jo * 16 + ti) {
            fprintf(stderr, "[sparseframe-hip] plan_create: LU step %d of outer block %d of supernode %lld has no pre-update task\n", ti, jo, (long long)s);
            return SF_ERR_ARG;
        }
        // Cholesky: J = diag (no left-looking update): the diagonal block arrives up to date, see k_step
        // LU: the diagonal block's own left-looking update is cut in two -- its far part (columns [J, diag - 64): final
        // before the PREVIOUS step starts) was applied by a pre-update task of that step's launch (below), the
        // diagonal workgroup only applies the last 64 columns before it factors
        steps.push_back(StepTask{XP[s], XP[s] + (lu ? ushift : 0), nsrow, lu ? (ti >= 2 ? diag - sf::NB : J) : diag, diag, b, diag, b, T.n_flags++, 0, (int32_t)(steps.size() - d0), 0, (int32_t)in.Super[s], 0});
        slot_of.push_back((int32_t)(steps.size() - 1 - d0));
        if (ti > 0) p.flops_panel_gemm += (lu ? 2.0 : 1.0) * ((double)b * (b + 1) * (diag - J) + 2.0 * (nsrow - diag - b) * (double)b * (diag - J));
    }
    if (lu && ti >= 1 && ti + 1 < ninner) {
        // pre-update tasks (mode bit 1): the far part of the NEXT step's diagonal-block update, K = [J, diag) -- the
        // columns of the steps before this one, final when this launch starts.  Right behind the diagonal tasks:
        // they never wait and are the longest tasks of the launch.
        const int dnext = diag + sf::NB;
        for (sf_long s : LS.sn) {
            const int nscol = (int)in.nscol(s), nsrow = (int)in.nsrow(s);
            if (dnext >= nscol) continue;
            const int bn = std::min(sf::NB, nscol - dnext);
            steps.push_back(StepTask{XP[s], XP[s] + ushift, nsrow, J, dnext, bn, dnext, bn, -1, 2, 0, 0, (int32_t)in.Super[s], 0});
            sw.pre_updated[(size_t)s] = jo * 16 + ti + 1;
        }
    }
    size_t si = 0;
    for (sf_long s : LS.sn) {
        const int nscol = (int)in.nscol(s), nsrow = (int)in.nsrow(s);
        const int32_t fl = flag_of[si], sl = slot_of[si];
        ++si;
        if (fl < 0) continue;
        const int b = std::min(sf::NB, nscol - diag);
        for (int r = diag + b; r < nsrow; r += sf::ST_ROWS) {
            const int nr = std::min(sf::ST_ROWS, nsrow - r);
            if (!lu) {
                // rows that are a later diagonal block of this outer block get this step's X X^T pushed into them
                const int nb = (r < std::min(nscol, J + sf::OUTER_NB)) ? std::min(sf::NB, nscol - r) : 0;
                steps.push_back(StepTask{XP[s], XP[s], nsrow, J, diag, b, r, nr, fl, 0, sl, nb, (int32_t)in.Super[s], 0});
            } else {
                steps.push_back(StepTask{XP[s], XP[s] + ushift, nsrow, J, diag, b, r, nr, fl, 0, sl, 0, (int32_t)in.Super[s], 0});     // L21 <- (L21 - ..) U11^{-1}
                steps.push_back(StepTask{XP[s] + ushift, XP[s], nsrow, J, diag, b, r, nr, fl, 1, sl, 0, (int32_t)in.Super[s], 0});     // U12^T <- (U12^T - ..) L11^{-T}
            }
        }
    }
    if ((int64_t)steps.size() > d0) {
        p.launches.push_back(Launch{LAUNCH_STEP, d0, (int)(steps.size() - d0)});
        p.launches.back().ticket = p.n_tickets++;
    }
    T.max_diag_tasks = std::max<int64_t>(T.max_diag_tasks, (int64_t)slot_of.size());
    return SF_OK;
}

// Throughput-bound step at column `diag` of the outer block at column J, as three launches: the stream-K GEMM that brings
// block column `diag` up to date (K = diag - J), one-wave POTRF / GETRF of the diagonal blocks, 256-row TRSM workgroups.
static void three_launch_step(const PlanInput& in, const Layout& lay, const LevelSet& LS, PlanTables& T, SfSchedule& p, int J, int diag) {
    const std::vector<int64_t>& XP = lay.XP;
    const int64_t ushift = lay.ushift;
    const int64_t p0 = (int64_t)T.potrf.size(), t0 = (int64_t)T.trsm.size(), g0 = (int64_t)T.gtasks.size();
    for (sf_long s : LS.sn) {
        const int nscol = (int)in.nscol(s), nsrow = (int)in.nsrow(s);
        if (diag >= nscol) continue;
        const int b = std::min(sf::NB, nscol - diag);
        if (diag > J) {
            GemmProb g{};
            g.lda = nsrow; g.ldc = nsrow;
            g.M = nsrow - diag; g.N = b; g.K = diag - J;
            const int64_t src = XP[s] + diag + (int64_t)J * nsrow;     // rows diag.., columns J..diag-1
            const int64_t dst = XP[s] + diag + (int64_t)diag * nsrow;
            const int32_t first = push_sides(in, lay, T, g, src, dst);
            for (int32_t id = first; id < (int32_t)T.probs.size(); ++id) {
                p.flops_panel_gemm += (double)g.N * (g.N + 1) * g.K + 2.0 * (g.M - g.N) * (double)g.N * g.K;
                add_tiles(T, p, id);
            }
        }
        T.potrf.push_back(PotrfTask{XP[s], nsrow, diag, b, (int32_t)in.Super[s]});
        const int below = diag + b;
        for (int r = below; r < nsrow; r += sf::TRSM_ROWS) {
            const int nr = std::min(sf::TRSM_ROWS, nsrow - r);
            if (!in.lu) {
                T.trsm.push_back(TrsmTask{XP[s], XP[s], nsrow, diag, b, r, nr, 0, (int32_t)in.Super[s], 0});
            } else {
                T.trsm.push_back(TrsmTask{XP[s], XP[s] + ushift, nsrow, diag, b, r, nr, 0, (int32_t)in.Super[s], 0});            // L21 <- L21 U11^{-1}
                T.trsm.push_back(TrsmTask{XP[s] + ushift, XP[s], nsrow, diag, b, r, nr, 1, (int32_t)in.Super[s], 0});            // U12^T <- U12^T L11^{-T}
            }
        }
    }
    if ((int64_t)T.gtasks.size() > g0) {
        p.launches.push_back(Launch{LAUNCH_GEMM_INNER, g0, (int)(T.gtasks.size() - g0)});
        // a chain step of a shared panel runs replicated on every rank of its group: no tile split by K, so that each target
        // element receives ONE addition and the replicas stay bit-identical (LU pivot decisions rest on that)
        p.launches.back().whole_tiles = set_is_shared(in, LS) && LS.share_cnt > 1;
    }
    if ((int64_t)T.potrf.size() > p0) p.launches.push_back(Launch{LAUNCH_POTRF, p0, (int)(T.potrf.size() - p0)});
    if ((int64_t)T.trsm.size() > t0) p.launches.push_back(Launch{LAUNCH_TRSM, t0, (int)(T.trsm.size() - t0)});
}

// Schur updates of every supernode of the set into its ancestors (LAUNCH_GEMM_SCATTER and LAUNCH_UPDATE_SMALL), and the pair table of the selected inversion
static void schur_updates(const PlanInput& in, const PlanKnobs& kn, const Layout& lay, const LevelSet& LS, PlanTables& T, SfSchedule& p) {
    const bool lu = in.lu;
    const int64_t g0 = (int64_t)T.gtasks.size(), s0 = (int64_t)T.stasks.size();
    double level_small_flops = 0;
    // longest K first: the tiles are claimed in list order (k_gemm's dynamic rounds), so the launch ends on its short tiles
    std::vector<sf_long> Su(LS.sn.begin(), LS.sn.end());
    std::stable_sort(Su.begin(), Su.end(), [&](sf_long a, sf_long b) { return in.nscol(a) > in.nscol(b); });
    for (sf_long s : Su) {
        const int nscol = (int)in.nscol(s), nsrow = (int)in.nsrow(s);
        const sf_long* rows = in.Lsi + in.Lsip[s];
        const double nk = nscol;
        p.flops_exec += lu ? ((double)nsrow * nk * nk - nk * nk * nk / 3.0 + (double)(nsrow - nscol) * nk * nk)
                           : (nk * nk * nk / 3.0 + (double)(nsrow - nscol) * nk * nk);
        int i = nscol;
        while (i < nsrow) {
            const sf_long a = in.SuperMap[rows[i]];
            int e = i;
            while (e < nsrow && in.SuperMap[rows[e]] == a) ++e;
            const int dn = e - i, dnm = nsrow - i;
            GemmProb g{};
            g.src_rows = in.Lsip[s] + i;
            const int a_nscol = (int)in.nscol(a), a_nsrow = (int)in.nsrow(a);
            g.tgt_rows = in.Lsip[a] + a_nscol;
            g.lda = nsrow; g.ldc = a_nsrow;
            g.M = dnm; g.N = dn; g.K = nscol;
            g.tgt_first_col = (int32_t)in.Super[a];
            g.tgt_nscol = a_nscol;
            g.tgt_nbelow = a_nsrow - a_nscol;
            g.map_off = T.relmap_size;            // one relative map per (s, a) pair, shared by the L and U^T sides
            p.sel_pair_J.push_back((int32_t)s);        // (the pair table of the selected inversion)
            p.sel_pair_i.push_back(i);
            p.sel_pair_off.push_back(T.relmap_size);
            T.relmap_size += dnm;
            T.scatter_probs.push_back((int64_t)T.probs.size());
            const int32_t first = push_sides(in, lay, T, g, lay.XP[s] + i, lay.XP[a]);
            for (int32_t id = first; id < (int32_t)T.probs.size(); ++id) {
                if (g.K <= kn.su_maxk) {
                    // short inner dimension: one wave per 64 x 32 tile (k_update_small); tiles entirely above the diagonal are skipped
                    const int tmn = (g.M + sf::SU_TM - 1) / sf::SU_TM, tnn = (g.N + sf::SU_TN - 1) / sf::SU_TN;
                    for (int tn = 0; tn < tnn; ++tn)
                        for (int tm = 0; tm < tmn; ++tm)
                            if ((tm + 1) * sf::SU_TM - 1 >= tn * sf::SU_TN)
                                T.stasks.push_back(GemmTask{id, (uint16_t)tm, (uint16_t)tn, 0u, 0u});
                } else {
                    const double t0f = p.flops_tiles;
                    add_tiles(T, p, id);
                    p.flops_tiles_update += p.flops_tiles - t0f;
                }
            }
            // executed flops of the tiles' useful part: Cholesky dn(dn+1)dk + 2 dm dn dk; LU twice minus the
            // diagonal the L side skips (the reference's two GEMMs do 2(dn+dm)dn dk + 2 dm dn dk, L:2570-2577)
            const double fl = lu ? (2.0 * (double)dnm * dn * nk + 2.0 * (double)(dnm - dn) * dn * nk)
                                 : ((double)dn * (dn + 1) * nk + 2.0 * (double)(dnm - dn) * dn * nk);
            p.flops_update += fl;
            if (g.K <= kn.su_maxk) { p.flops_update_small += fl; level_small_flops += fl; }
            p.flops_exec += fl;
            p.scatter_elems += lu ? ((double)dnm * dn + (double)(dnm - dn) * dn)
                                  : ((double)dn * (dn + 1) / 2.0 + (double)(dnm - dn) * dn);
            p.n_pairs++;
            i = e;
        }
    }
    const bool shared = set_is_shared(in, LS);
    if ((int64_t)T.gtasks.size() > g0) {
        p.launches.push_back(Launch{LAUNCH_GEMM_SCATTER, g0, (int)(T.gtasks.size() - g0)});
        stamp_share(p.launches.back(), LS, shared);
    }
    if ((int64_t)T.stasks.size() > s0) {
        p.launches.push_back(Launch{LAUNCH_UPDATE_SMALL, s0, (int)(T.stasks.size() - s0)});
        stamp_share(p.launches.back(), LS, shared);
        p.launches.back().flops = level_small_flops;
    }
}

// The launches of one level set: per outer block column its left-looking update, the reduce point (shared sets), the chain of
// 64-column steps; then the set's Schur updates.
static int schedule_set(const PlanInput& in, const PlanKnobs& kn, const Layout& lay, const LevelSet& LS, SweepState& sw, PlanTables& T,
                        SfSchedule& p) {
    if (LS.ph == 1 && !sw.split_set) { p.launch_split = p.launches.size(); sw.split_set = true; }
    // out of core: every group starts by zeroing and assembling its buffer (LAUNCH_OOC_GROUP, first = the group); groups without supernodes
    // still get theirs, so that the buffers' turn-taking is the same whatever the tree looks like
    while (in.ooc() && LS.group > sw.ooc_open) p.launches.push_back(Launch{LAUNCH_OOC_GROUP, (int64_t)++sw.ooc_open, 0});
    const bool shared = set_is_shared(in, LS);
    sf_long maxcol = 0;
    for (sf_long s : LS.sn) maxcol = std::max(maxcol, in.nscol(s));
    // Two-level blocking of the in-panel factorization.  Outer block columns of OUTER_NB columns are
    // brought up to date left-looking with ONE large-K GEMM (K = all columns to their left), then
    // factored right-looking in NB-column steps whose trailing update stays inside the outer block.
    // The K = NB updates are HBM-bound read-modify-writes; confining them to OUTER_NB columns cuts
    // their traffic by n / OUTER_NB, the rest of the flops run at large K out of LDS/registers.
    const int nouter = (int)((maxcol + sf::OUTER_NB - 1) / sf::OUTER_NB);
    // Look-ahead for shared panels (several ranks): the update of block jo is cut into the FAR part (columns of the blocks
    // 0 .. jo-2, issued right after the chain of block jo-2, shared among the ranks) and the part of block jo-1 (issued after
    // the reduce point of block jo, executed in full by every rank: 512 columns of K).  The far part is all a block's sum over
    // the ranks has to wait for, so that sum travels while the chain of block jo-1 runs (sf_chol_plan_factorize_distributed).
    // (The same cut on ONE GPU, the far part on a second stream, was measured and not adopted: DESIGN 5.2.)
    const bool ahead = shared && p.lookahead && LS.share_cnt > 1;
    constexpr int KT_BLOCK = sf::OUTER_NB / sf::GEMM_BK;
    for (int jo = 0; jo < nouter; ++jo) {
        const int J = jo * sf::OUTER_NB;
        if (jo > 0 && !ahead) outer_gemm(in, lay, LS, T, p, J, 0, -1, shared);
        if (shared) {
            reduce_point(in, lay, LS, p, jo, ahead);
            if (ahead && jo > 0) outer_gemm(in, lay, LS, T, p, J, (jo - 1) * KT_BLOCK, jo * KT_BLOCK, false);       // block jo-1 -> block jo, replicated
        }
        // Inside the outer block the 64-column steps are LEFT-looking as well: block column t is first
        // updated by the t block columns of this outer block already factored (K = 64 t, written once),
        // then its diagonal block is factored and the rows below are solved.  (A right-looking trailing
        // update would read-modify-write the rest of the outer block at every step with K = 64.)
        const int ninner = sf::OUTER_NB / sf::NB;
        bool block_fused = false;       // decided at the block's first step (the largest), kept for all its steps: the
                                        // fused Cholesky steps push updates into the block's FUTURE diagonal blocks
        for (int ti = 0; ti < ninner; ++ti) {
            const int diag = J + ti * sf::NB;
            if (diag >= maxcol) break;
            int64_t step_wgs = 0;
            for (sf_long s : LS.sn) {
                const int64_t nscol = in.nscol(s), nsrow = in.nsrow(s);
                if (diag < nscol) step_wgs += 1 + in.sides() * ((nsrow - std::min<int64_t>(nscol, diag + sf::NB) + sf::ST_ROWS - 1) / sf::ST_ROWS);
            }
            if (ti == 0) block_fused = step_wgs <= kn.fuse_max;
            if (!block_fused) three_launch_step(in, lay, LS, T, p, J, diag);
            else if (int rc = fused_step(in, lay, LS, sw, T, p, jo, ti, diag)) return rc;
        }
        const bool owner_block = shared && !p.segments.empty() && p.segments.back().owner_gi >= 0;
        if (owner_block) p.segments.back().lc = p.launches.size();       // near GEMM + chain = the owner's part; then the broadcast
        for (sf_long s : LS.sn)     // (owner-computes: final on every rank only after the broadcast, i.e. once the next launch is in)
            if (J < in.nscol(s)) T.blk_ready[T.blk_first[s] + jo] = p.launches.size() + (owner_block ? 1 : 0);
        if (ahead && jo + 2 < nouter) outer_gemm(in, lay, LS, T, p, J + 2 * sf::OUTER_NB, 0, (jo + 1) * KT_BLOCK, true);    // blocks 0 .. jo -> block jo+2
    }
    schur_updates(in, kn, lay, LS, T, p);
    return SF_OK;
}

static int schedule_factorization(const PlanInput& in, const PlanKnobs& kn, const Layout& lay, const std::vector<LevelSet>& sets,
                                  PlanTables& T, SfSchedule& p) {
    T.blk_first.assign(in.nsuper + 1, 0);
    for (sf_long s = 0; s < in.nsuper; ++s) T.blk_first[s + 1] = T.blk_first[s] + (in.nscol(s) + sf::OUTER_NB - 1) / sf::OUTER_NB;
    T.blk_ready.assign(T.blk_first[in.nsuper], 0);
    p.lookahead = kn.lookahead;
    p.use_graph = kn.use_graph;
    p.top_owner = kn.top_owner && !in.lu;
    SweepState sw;
    sw.pre_updated.assign(in.lu ? (size_t)std::max<sf_long>(in.nsuper, 1) : 0, -1);
    p.launch_split = 0;
    for (const LevelSet& LS : sets)
        if (int rc = schedule_set(in, kn, lay, LS, sw, T, p)) return rc;
    if (!sw.split_set) p.launch_split = p.launches.size();
    if (!p.segments.empty()) p.segments.back().l1 = p.launches.size();
    p.n_gemm_tasks = (int64_t)T.gtasks.size() + (int64_t)T.stasks.size();
    return SF_OK;
}

// ---------------- device solve schedule (unsharded plans) ----------------
// per (level, SV_B-column step): a forward launch [diagonal tasks, SV_ROWS-row tiles] and a backward launch [tiles, diagonal tasks]
static void schedule_solve(const PlanInput& in, const PlanKnobs& kn, const Layout& lay, PlanTables& T, SfSchedule& p) {
    int32_t n_solve_sync = 0;
    // A mapped plan (create_mapped: one rank's subtrees + the top supernodes above them) gets a schedule too, over the panels it
    // stores -- the distributed solve (sf_chol_plan_solve_distributed, sf_multi.hip):
    //   forward   x[columns of a shared supernode] is summed over its group before the supernode's first step (the right-hand side
    //             is loaded by the group's first rank only, every rank adds the updates of its own descendants); the diagonal
    //             solves and the tiles inside the supernode's own columns are replicated in the group, the tiles that update
    //             ANCESTORS' rows are dealt out over the group (their sums meet again at the ancestor's reduce point);
    //   backward  no communication: every rank of a group solves the group's supernodes in full (it holds the panels and, by
    //             then, the solution of all their ancestors).
    const bool solve_mapped = p.partial && in.top_mask != nullptr && in.load_top == 2;
    if (!p.partial || solve_mapped) {
        std::vector<std::vector<sf_long>> by_level(p.nlevels);
        for (sf_long s = 0; s < in.nsuper; ++s)
            if (lay.XP[s] >= 0) by_level[p.level_of[s]].push_back(s);
        auto shared_sn = [&](sf_long s) { return solve_mapped && p.phase[s] == 1 && __builtin_popcount(lay.gmask[s]) > 1; };
        if (solve_mapped) {
            for (sf_long s = 0; s < in.nsuper; ++s) {
                if (lay.XP[s] < 0) continue;
                const bool first = p.phase[s] == 0 || lay.group_idx(lay.gmask[s]) == 0;
                if (first) {
                    if (!p.solve_own.empty() && p.solve_own.back().second == in.Super[s]) p.solve_own.back().second = in.Super[s + 1];
                    else p.solve_own.push_back({in.Super[s], in.Super[s + 1]});
                }
            }
            p.solve_load = p.solve_own;
        }
        const int tile = sf::SV_ROWS;
        const bool solve_diagT = kn.solve_diagT, bwd_fused = kn.solve_bwd_fused, bwd_ahead = kn.solve_bwd_ahead && bwd_fused;
        const bool fwd_ahead = kn.solve_fwd_ahead, fwd_far_first = kn.solve_fwd_far_first;
        const int solve_far_wgs = kn.solve_far_wgs, solve_far_groups = kn.solve_far_groups;
        p.solve_bwd_fused = bwd_fused;
        for (int l = 0; l < p.nlevels; ++l) {
            sf_long maxcol = 0;
            for (sf_long s : by_level[l]) maxcol = std::max(maxcol, in.nscol(s));
            // the narrow panels of the level (nscol <= 64; the swarm levels consist of nothing else) go to the
            // one-wave-per-supernode kernels as a step of their own, the wide ones through the general 256-column steps
            std::vector<sf_long> narrow, wide;
            for (sf_long s : by_level[l]) ((in.nscol(s) <= sf::NB && !shared_sn(s)) ? narrow : wide).push_back(s);
            if (narrow.size() < 64) { wide = by_level[l]; narrow.clear(); }     // not worth a launch of their own
            // sums that precede this level's first step: the columns of its shared supernodes, each inside its group
            const int red_first = (int)p.solve_reduces.size();
            for (sf_long s : wide)
                if (shared_sn(s)) p.solve_reduces.push_back(SfSchedule::SolveReduce{in.Super[s], in.nscol(s), lay.gmask[s]});
            int red_count = (int)p.solve_reduces.size() - red_first;
            if (!narrow.empty()) {
                SfSchedule::SolveStep st{};
                st.small = 1;
                st.fwd_first = st.bwd_first = (int64_t)T.solve.size();
                for (sf_long s : narrow) {
                    const int nscol = (int)in.nscol(s), nsrow = (int)in.nsrow(s);
                    T.solve.push_back(sf::SolveTask{lay.XP[s], in.Lsip[s], nsrow, 0, nscol, 0, 0, (int32_t)in.Super[s], 0, 0});
                }
                st.count = st.ndiag = st.fwd_count = (int)narrow.size();
                st.red_first = red_first; st.red_count = 0;
                p.solve_steps.push_back(st);
            }
            maxcol = 0;
            for (sf_long s : wide) maxcol = std::max(maxcol, in.nscol(s));
            // Backward look-ahead: the sum a diagonal task waits for, S_J = sum over the row blocks I > J of L_IJ^T x_I, only
            // needs x_{J+1} -- solved one launch earlier -- for the tiles whose rows lie in block J + 1 ("near").  All other tiles of
            // step J ("far": rows two blocks further down, or below the panel) read values that were final a launch earlier, so
            // they ride in the launch of step J + 1, behind its diagonal task, and the diagonal task of step J waits for its few
            // near tiles only.  (Forward sweep: unchanged.  SF_SOLVE_BWD_AHEAD=0 or the two-launch form: every tile is near.)
            // The forward sweep looks ahead the same way: the tiles of step J whose rows lie two blocks further down (or below the
            // panel) are not needed by the next diagonal task, so they ride in the launch of step J + 1 -- there their flag (step J's,
            // set one launch earlier, never reset within a solve) is already up and they run at once, next to that launch's
            // diagonal task, instead of holding a CU slot while they spin on it.  (SF_SOLVE_FWD_AHEAD=0: off.)
            std::vector<sf::SolveTask> pending_far;        // far tiles of the step built in the previous iteration
            std::vector<sf::SolveTask> pending_far_fwd;
            // Far tiles are merged into tasks of up to 8 consecutive 64-row groups of one panel (k_solve_*: one workgroup streams
            // through them; backward: ONE butterfly and ONE set of atomics per task instead of one per 64 rows, on the 256 words
            // all tiles of a step add to), as long as that leaves ~512 workgroups to the launch.  SF_SOLVE_FAR_GROUPS=1: off.
            auto group_far = [&](std::vector<sf::SolveTask>& v) {
                const int G = std::max(1, std::min(solve_far_groups, (int)(v.size() / (size_t)solve_far_wgs)));
                if (G <= 1 || v.empty()) return false;
                std::vector<sf::SolveTask> out;
                for (const sf::SolveTask& t : v) {
                    if (!out.empty() && out.back().panel == t.panel && out.back().diag == t.diag && out.back().flag == t.flag &&
                        out.back().row0 + out.back().nrows == t.row0 && out.back().nrows % tile == 0 && out.back().nrows + t.nrows <= G * tile)
                        out.back().nrows += t.nrows;
                    else out.push_back(t);
                }
                v.swap(out);
                return true;
            };
            for (int diag = 0; diag < maxcol; diag += sf::SV_B) {
                SfSchedule::SolveStep st{};
                std::vector<sf::SolveTask> dg, rows, rows_fwd, far_next, far_next_fwd;
                for (sf_long s : wide) {
                    const int nscol = (int)in.nscol(s), nsrow = (int)in.nsrow(s);
                    if (diag >= nscol) continue;
                    const int b = std::min(sf::SV_B, nscol - diag);
                    const bool sh = shared_sn(s);
                    // a shared supernode's tiles are cut at the end of its own columns: the ones inside are replicated in the
                    // group, the ones below (ancestors' rows) are dealt out in the forward sweep
                    int ntiles = 0;
                    const int cut = sh ? std::max(nscol, diag + b) : nsrow;
                    const int g = sh ? __builtin_popcount(lay.gmask[s]) : 1, gi = sh ? lay.group_idx(lay.gmask[s]) : 0;
                    int below = 0;
                    // (a supernode with no later block in this level has nothing to look ahead to: all its tiles are near)
                    const int near_end = (bwd_ahead && nscol > diag + b) ? std::min(nscol, diag + b + sf::SV_B) : nsrow;
                    const int near_end_fwd = (fwd_ahead && nscol > diag + b) ? std::min(nscol, diag + b + sf::SV_B) : nsrow;
                    for (int r0 = diag + b, r1 = cut; r0 < nsrow; r0 = r1, r1 = nsrow) {
                        for (int r = r0; r < r1; r += tile) {
                            const sf::SolveTask t{lay.XP[s], in.Lsip[s], nsrow, diag, b, r, std::min(tile, r1 - r), (int32_t)in.Super[s], n_solve_sync, 0};
                            if (r < near_end) { rows.push_back(t); ++ntiles; }
                            else { far_next.push_back(t); far_next.back().flag = -1; }       // counts for nobody: a scratch word, set below
                            if (!sh || r < nscol || (below++ % g) == gi) ((fwd_ahead && r >= near_end_fwd) ? far_next_fwd : rows_fwd).push_back(t);
                        }
                        if (r1 >= nsrow) break;
                    }
                    // sync words: [flag] forward "solved" flag, [flag + 1] backward tile counter
                    dg.push_back(sf::SolveTask{lay.XP[s], in.Lsip[s], nsrow, diag, b, 0, 0, (int32_t)in.Super[s], n_solve_sync, ntiles});
                    n_solve_sync += 2;
                }
                st.fwd_first = (int64_t)T.solve.size();
                T.solve.insert(T.solve.end(), dg.begin(), dg.end());
                // order of the forward list = order in which workgroups take their tasks: diagonal tasks, then the far tiles of the
                // step before (nothing to wait for: they start at once), the near tiles last -- taken first they would sit in
                // the CU slots spinning on the diagonal tasks' flags and keep the far tiles out until those are up
                const bool grouped_fwd = group_far(pending_far_fwd);
                if (fwd_far_first) T.solve.insert(T.solve.end(), pending_far_fwd.begin(), pending_far_fwd.end());
                T.solve.insert(T.solve.end(), rows_fwd.begin(), rows_fwd.end());
                if (!fwd_far_first) T.solve.insert(T.solve.end(), pending_far_fwd.begin(), pending_far_fwd.end());
                st.fwd_count = (int)(dg.size() + rows_fwd.size() + pending_far_fwd.size());
                pending_far_fwd.swap(far_next_fwd);
                st.red_first = red_first; st.red_count = red_count;
                red_count = 0;                      // the sums belong to the level's first step
                st.bwd_first = (int64_t)T.solve.size();
                for (sf::SolveTask t : rows) { t.flag += 1; T.solve.push_back(t); }
                // backward: one launch, the diagonal task waits for a tile counter (SF_SOLVE_BWD_FUSED=0: the row tiles and
                // the diagonal tasks as TWO launches -- measured slower)
                for (sf::SolveTask t : dg) {
                    t.flag += 1;
                    if (!bwd_fused) t.expect = 0;
                    // the steps of the top levels (few supernodes per level: their chain of diagonal tasks IS the backward
                    // sweep's critical path) read their diagonal block from a row-major copy: coalesced instead of one cache line
                    // per lane (128^3: backward sweep 19.8 -> see DESIGN 8; SF_SOLVE_DIAGT=0: off)
                    if (solve_diagT && wide.size() <= 16 && t.b > sf::NB) {
                        t.tdiag = 1 + T.solveT_size;
                        T.solveT_size += (int64_t)t.b * t.b;
                        T.solveT_list.push_back((int64_t)T.solve.size());
                    }
                    T.solve.push_back(t);
                }
                // the far tiles of the step before this one (lower column block): their rows' x is final when this launch starts
                const bool grouped_bwd = group_far(pending_far);
                T.solve.insert(T.solve.end(), pending_far.begin(), pending_far.end());
                st.count = (int)(dg.size() + rows.size() + pending_far.size());
                pending_far.swap(far_next);
                st.nrows_tasks = (int)rows.size();
                st.big = 0;
                for (const sf::SolveTask& t : dg) st.big |= t.b > sf::NB;
                if (grouped_bwd || grouped_fwd) st.big = 1;     // only that instantiation of the kernels walks through row groups
                st.small = 0;
                st.ndiag = (int)dg.size();
                p.solve_steps.push_back(st);
            }
        }
    }
    for (sf::SolveTask& t : T.solve)
        if (t.flag < 0) t.flag = n_solve_sync;        // the scratch word the far tiles count on
    p.n_solve_sync = n_solve_sync + 1;
}

// ---------------- K-step prefix of every GEMM launch (stream-K work distribution, see k_gemm) ----------------
static int kstep_prefixes(PlanTables& T, SfSchedule& p) {
    for (Launch& L : p.launches) {
        if (!launch_is_gemm(L.kind)) continue;
        L.prefix_first = (int64_t)T.ktprefix.size();
        uint64_t run = 0;
        int32_t last_prob = -1;
        for (int k = 0; k < L.count; ++k) {
            T.ktprefix.push_back((uint32_t)run);
            const int32_t pi = T.gtasks[L.first + k].prob;
            const GemmProb& g = T.probs[pi];
            run += (uint64_t)T.gtasks[L.first + k].nkt;
            if (pi != last_prob) {      // tasks of one problem are contiguous
                L.flops += (double)g.N * (g.N + 1) * g.K + 2.0 * (double)(g.M - g.N) * g.N * g.K;
                last_prob = pi;
            }
        }
        if (run >= (uint64_t)0x7fffffff) return SF_ERR_ARG;   // one launch holds < 2^31 units
        T.ktprefix.push_back((uint32_t)run);
        L.units = (uint32_t)run;
    }
    return SF_OK;
}

// ---------------- download schedule (sf_chol_plan_factorize_to_host) and the U11 fill tiles ----------------
// Block columns in host order, merged while contiguous in the host layout (Cholesky: and in the device layout) up to
// one staging slot, larger runs cut into slot-sized pieces.  Top panels of a sharded plan are identical on every
// rank once factored: their pieces are dealt out over the ranks so that every PCIe link carries a share.
static void schedule_download(const PlanInput& in, const PlanKnobs& kn, const Layout& lay, PlanTables& T, const SfSchedule& p, sf::DlSchedule& dl) {
    dl.workers = kn.dl_workers; dl.workers_fresh = kn.dl_workers_fresh;
    dl.host_wait = kn.dl_host_wait;
    dl.slot = kn.dl_slot;
    const int64_t DL_SLOT = dl.slot;
    const bool dl_2d = kn.dl_2d;
    std::vector<DlPiece> runs;
    std::vector<uint32_t> run_mask;
    int last_phase = -2;
    uint32_t last_mask = 0;
    int32_t last_group = -2;        // out of core: a piece never spans two groups (each group's copy is counted on its own)
    auto grp = [&](sf_long s) { return in.ooc() ? in.ooc_group[s] : (int32_t)-1; };
    // LU: the reference keeps one packed panel per supernode, column j = [ L11 \ U11 (nscol) | L21 | U12^T ] (L:2514-2517), the
    // device an L panel and a U^T panel.  DIRECT form (default): the pieces are whole columns; the compute stream writes U11 into
    // the (unused) upper triangle of the L panel's diagonal block before a piece's event (k_lu_fill_u11), the L and U^T runs
    // travel as they are and the copy worker interleaves them column by column.  SF_DL_LU_PACK=1 (and any matrix with a
    // packed column longer than a staging slot): the older form, a gather kernel per piece on the worker's stream -- which has
    // to find free CUs next to the factorization's persistent kernels and made the LU struct call 2x its resident step.
    bool lu_direct = in.lu && !kn.dl_lu_pack;
    for (sf_long s = 0; s < in.nsuper && lu_direct; ++s)
        if (lay.XP[s] >= 0 && 2 * in.nsrow(s) - in.nscol(s) > DL_SLOT) lu_direct = false;
    dl.lu_direct = lu_direct;
    for (sf_long s = 0; s < in.nsuper; ++s) {
        if (lay.XP[s] < 0) continue;
        const int64_t nscol = in.nscol(s), nsrow = in.nsrow(s);
        const int64_t hld = in.lu ? 2 * nsrow - nscol : nsrow;
        if (lu_direct) {
            const int64_t cntL = nsrow * nscol;
            if (2 * cntL <= DL_SLOT) {                       // a whole supernode, merged with its neighbours while they fit a slot
                size_t ready = 0;
                for (int64_t jo = 0; jo * sf::OUTER_NB < nscol; ++jo) ready = std::max(ready, T.blk_ready[T.blk_first[s] + jo]);
                DlPiece pc{lay.XP[s], in.Lsxp[s], nscol * hld, ready, 0};
                pc.s0 = (int32_t)s; pc.s1 = (int32_t)s + 1; pc.dev_count = cntL;
                const bool can_merge = !runs.empty() && runs.back().s0 >= 0 && runs.back().ld == 0 && runs.back().s1 == (int32_t)s &&
                                       last_phase == p.phase[s] && last_mask == lay.gmask[s] && last_group == grp(s) &&
                                       runs.back().dev_off + runs.back().dev_count == pc.dev_off &&
                                       runs.back().host_off + runs.back().count == pc.host_off &&
                                       2 * (runs.back().dev_count + cntL) <= DL_SLOT;
                if (can_merge) {
                    runs.back().count += pc.count;
                    runs.back().dev_count += cntL;
                    runs.back().s1 = (int32_t)s + 1;
                    runs.back().ready = std::max(runs.back().ready, pc.ready);
                } else {
                    pc.ev = p.phase[s];
                    runs.push_back(pc);
                    run_mask.push_back(lay.gmask[s]);
                }
            } else {
                for (int64_t jo = 0; jo * sf::OUTER_NB < nscol; ++jo) {     // block columns, cut to slot size below
                    const int64_t J = jo * sf::OUTER_NB, w = std::min<int64_t>(sf::OUTER_NB, nscol - J);
                    DlPiece pc{lay.XP[s] + J * nsrow, in.Lsxp[s] + J * hld, w * hld, T.blk_ready[T.blk_first[s] + jo], 0};
                    pc.s0 = (int32_t)s; pc.s1 = (int32_t)s + 1; pc.j0 = J; pc.ncols = w; pc.ld = nsrow; pc.dev_count = w * nsrow;
                    pc.ev = p.phase[s];
                    runs.push_back(pc);
                    run_mask.push_back(lay.gmask[s]);
                }
            }
            last_phase = p.phase[s];
            last_mask = lay.gmask[s];
            last_group = grp(s);
            continue;
        }
        for (int64_t jo = 0; jo * sf::OUTER_NB < nscol; ++jo) {
            const int64_t J = jo * sf::OUTER_NB, w = std::min<int64_t>(sf::OUTER_NB, nscol - J);
            DlPiece pc{lay.XP[s] + J * nsrow, in.Lsxp[s] + J * hld, w * hld, T.blk_ready[T.blk_first[s] + jo], 0};
            // Cholesky, block columns right of the first: rows [0, J) of these columns are zeros on both sides -- 7 % of the
            // factor at 128^3 -- and stay off the link (SF_DL_2D=0: copy them like everything else)
            const bool two_d = !in.lu && J > 0 && dl_2d;
            if (two_d) { pc.skip = J; pc.ld = nsrow; pc.ncols = w; pc.count = w * (nsrow - J); }
            const bool can_merge = !two_d && !runs.empty() && runs.back().ld == 0 && last_phase == p.phase[s] && last_mask == lay.gmask[s] &&
                                   last_group == grp(s) &&
                                   runs.back().host_off + runs.back().count == pc.host_off &&
                                   (in.lu || runs.back().dev_off + runs.back().count == pc.dev_off) &&
                                   runs.back().count + pc.count <= DL_SLOT;
            if (can_merge) {
                runs.back().count += pc.count;
                runs.back().ready = std::max(runs.back().ready, pc.ready);
            } else {
                pc.ev = p.phase[s];        // phase kept here until the pieces are dealt out below
                runs.push_back(pc);
                run_mask.push_back(lay.gmask[s]);
            }
            last_phase = p.phase[s];
            last_mask = lay.gmask[s];
            last_group = grp(s);
        }
    }
    std::vector<std::pair<uint32_t, int64_t>> seen_by_mask;     // pieces of a group's panels are dealt out inside the group
    for (size_t ri = 0; ri < runs.size(); ++ri) {
        const DlPiece& r = runs[ri];
        if (r.ev == 1 && in.nranks > 1) {
            const uint32_t m = run_mask[ri];
            size_t k = 0;
            while (k < seen_by_mask.size() && seen_by_mask[k].first != m) ++k;
            if (k == seen_by_mask.size()) seen_by_mask.push_back({m, 0});
            const int64_t seq = seen_by_mask[k].second++;
            if ((int)(seq % __builtin_popcount(m)) != lay.group_idx(m)) continue;
        }
        if (r.s0 >= 0) {        // LU, direct form
            if (r.ld == 0) { dl.pieces.push_back(r); dl.pieces.back().ev = 0; continue; }
            const int64_t hld = 2 * r.ld - in.nscol(r.s0), cper = std::max<int64_t>(1, DL_SLOT / hld);
            for (int64_t c = 0; c < r.ncols; c += cper) {
                DlPiece q = r;
                q.ev = 0;
                q.j0 = r.j0 + c; q.ncols = std::min(cper, r.ncols - c);
                q.dev_off = r.dev_off + c * r.ld; q.host_off = r.host_off + c * hld; q.count = q.ncols * hld; q.dev_count = q.ncols * r.ld;
                dl.pieces.push_back(q);
            }
            continue;
        }
        if (r.ld > 0) {         // 2-D piece: cut by whole columns
            const int64_t rows = r.ld - r.skip, cper = std::max<int64_t>(1, DL_SLOT / std::max<int64_t>(rows, 1));
            if (rows > DL_SLOT) {       // one column longer than a slot (never with the default 32 MiB slot): plain pieces
                for (int64_t o = 0; o < r.ncols * r.ld; o += DL_SLOT)
                    dl.pieces.push_back(DlPiece{r.dev_off + o, r.host_off + o, std::min(DL_SLOT, r.ncols * r.ld - o), r.ready, 0});
                continue;
            }
            for (int64_t c = 0; c < r.ncols; c += cper) {
                DlPiece q{r.dev_off + c * r.ld, r.host_off + c * r.ld, std::min(cper, r.ncols - c) * rows, r.ready, 0};
                q.skip = r.skip; q.ld = r.ld; q.ncols = std::min(cper, r.ncols - c);
                dl.pieces.push_back(q);
            }
            continue;
        }
        for (int64_t o = 0; o < r.count; o += DL_SLOT)
            dl.pieces.push_back(DlPiece{r.dev_off + o, r.host_off + o, std::min(DL_SLOT, r.count - o), r.ready, 0});
    }
    std::stable_sort(dl.pieces.begin(), dl.pieces.end(), [](const DlPiece& a, const DlPiece& b) { return a.ready < b.ready; });
    if (in.ooc()) {
        // the group of every piece (from the supernode its first host entry belongs to) and the number of pieces per group: what
        // the launch that re-uses a buffer waits for
        dl.group_pieces.assign((size_t)in.ooc_ngroups, 0);
        for (DlPiece& pc : dl.pieces) {
            const sf_long s = (sf_long)(std::upper_bound(in.Lsxp, in.Lsxp + in.nsuper + 1, (sf_long)pc.host_off) - in.Lsxp) - 1;
            pc.group = (s >= 0 && s < in.nsuper) ? (in.ooc_group[s] >= 0 ? in.ooc_group[s] : (in.ooc_top_mode >= 1 ? p.ooc_last[(size_t)s] : -1)) : -1;
            if (pc.group >= 0) ++dl.group_pieces[(size_t)pc.group];
        }
    }
    for (DlPiece& pc : dl.pieces) {
        if (dl.ev_ready.empty() || dl.ev_ready.back() != pc.ready) dl.ev_ready.push_back(pc.ready);
        pc.ev = (int)dl.ev_ready.size() - 1;
    }
    if (lu_direct) {            // the U11 fill tiles of every piece, grouped by the piece's event
        std::vector<std::vector<sf::FillTile>> by_ev(dl.ev_ready.size());
        for (const DlPiece& pc : dl.pieces)
            for (int32_t s = pc.s0; s < pc.s1; ++s) {
                const int32_t nscol = (int32_t)in.nscol(s), nsrow = (int32_t)in.nsrow(s);
                const int32_t cb = pc.ld > 0 ? (int32_t)pc.j0 : 0, ce = pc.ld > 0 ? (int32_t)(pc.j0 + pc.ncols) : nscol;
                for (int32_t c0 = cb / 64 * 64; c0 < ce; c0 += 64)
                    for (int32_t r0 = 0; r0 <= c0; r0 += 64) by_ev[pc.ev].push_back(sf::FillTile{lay.XP[s], nsrow, r0, c0, cb, ce});
            }
        dl.fill_first.assign(1, 0);
        for (const auto& v : by_ev) {
            T.fill_tiles.insert(T.fill_tiles.end(), v.begin(), v.end());
            dl.fill_first.push_back((int64_t)T.fill_tiles.size());
        }
    }
}

// ---------------- a rank's input from an owner map ----------------
// Rank `rank`'s plan of an nranks-way factorization from the owner map of sf_subtree_partition* (owner[s] = rank of the
// subtree holding s, -1 = top): PROPORTIONAL MAPPING of the top -- a top supernode belongs to the ranks whose subtrees lie
// below it, only they store its panel, split its GEMMs and sum its block columns.
// Fills in.phase_in / top_mask / root_cum / load_top / rank / nranks; the arrays they point to live in `store`.
int sf_schedule_map_input(PlanInput& in, const int32_t* owner, int rank, int nranks, MappedInput& store) {
    const sf_long n = in.n, nsuper = in.nsuper;
    const sf_long *Super = in.Super, *SuperMap = in.SuperMap, *Lsip = in.Lsip, *Lsi = in.Lsi;
    const bool lu = in.lu;
    std::vector<uint32_t>& mask = store.mask;
    std::vector<int32_t>& phase = store.phase;
    std::vector<double>& cum = store.cum;
    if (!owner || nranks < 1 || nranks > 32 || rank < 0 || rank >= nranks) return SF_ERR_ARG;
    if (nsuper < 0 || !Super || !Lsip || (nsuper > 0 && (!SuperMap || !Lsi))) return SF_ERR_ARG;
    mask.assign((size_t)std::max<sf_long>(nsuper, 1), 0);
    phase.assign((size_t)std::max<sf_long>(nsuper, 1), 0);
    for (sf_long s = 0; s < nsuper; ++s) {
        if (owner[s] < -1 || owner[s] >= nranks) return SF_ERR_ARG;
        if (owner[s] >= 0) mask[s] |= 1u << owner[s];
        const sf_long nscol = Super[s + 1] - Super[s], nsrow = Lsip[s + 1] - Lsip[s];
        if (nscol < nsrow) {        // parents follow their children in the postorder
            const sf_long row = Lsi[Lsip[s] + nscol];
            if (row < 0 || row >= n) return SF_ERR_ARG;
            const sf_long par = SuperMap[row];
            if (par <= s || par >= nsuper) return SF_ERR_ARG;
            mask[par] |= mask[s];
        }
    }
    for (sf_long s = 0; s < nsuper; ++s) {
        if (owner[s] >= 0) { phase[s] = owner[s] == rank ? 0 : -1; mask[s] = 0; }
        else phase[s] = ((mask[s] >> rank) & 1u) ? 1 : -1;
    }
    // Weighted shares of the sets every rank takes part in (the root's GEMMs: the largest pool of divisible work).  The relaxed
    // amalgamation can make the tree lopsided -- at 161^3 over 4 ranks one pair of ranks shares a 14,641-column separator, the other
    // pair a 6,720-column one -- so the ranks arrive at the root with different loads.  Model (every rank evaluates the same
    // numbers): time of a rank before the root = its subtrees' flops at 42 TFLOP/s + for each smaller group it belongs to the
    // replicated part (chains: 45 us per 64 columns; in-block and near-part updates) + its equal share of that group's divisible
    // flops at 48 TFLOP/s (calibrated on tools/emulate_rank.py, 128^3 / 8 and 161^3 / 4); the root's divisible flops, at 58 TFLOP/s, are
    // then dealt out so that the ranks finish together (shares clamped to [0.2, 3] / nranks).  SF_WEIGHTED_SHARES=0: equal shares.
    const char* wenv = sf_exp_env("SF_WEIGHTED_SHARES");
    if (nranks > 1 && !(wenv && atoi(wenv) == 0)) {
        const uint32_t all = nranks >= 32 ? 0xffffffffu : ((1u << nranks) - 1u);
        std::vector<double> before(nranks, 0.0);
        double root_ms = 0.0;
        for (sf_long s = 0; s < nsuper; ++s) {
            const double k = (double)(Super[s + 1] - Super[s]), r = (double)(Lsip[s + 1] - Lsip[s]), m = r - k;
            double f = k * k * k / 3.0 + m * k * k;
            {
                const sf_long* rows = Lsi + Lsip[s];
                sf_long i = (sf_long)k;
                const sf_long nsrow = (sf_long)r;
                while (i < nsrow) {
                    const sf_long o = SuperMap[rows[i]];
                    sf_long e = i;
                    while (e < nsrow && SuperMap[rows[e]] == o) ++e;
                    const double dn = (double)(e - i), dm = (double)(nsrow - e);
                    f += dn * (dn + 1) * k + 2.0 * dm * dn * k;
                    i = e;
                }
            }
            if (lu) f *= 2.0;
            if (owner[s] >= 0) { before[owner[s]] += f / 42e9; continue; }
            const double rep = std::min(f, (lu ? 2.0 : 1.0) * 1472.0 * (r * k - 0.5 * k * k));
            const double chain_ms = std::ceil(k / 64.0) * 0.045;
            const int g = __builtin_popcount(mask[s]);
            if (mask[s] == all) { root_ms += (f - rep) / 58e9; continue; }
            for (int q = 0; q < nranks; ++q)
                if ((mask[s] >> q) & 1u) before[q] += chain_ms + (rep + (f - rep) / std::max(g, 1)) / 48e9;
        }
        if (root_ms > 0.0) {
            const double smin = 0.2 / nranks, smax = 3.0 / nranks;
            double lo = *std::min_element(before.begin(), before.end()), hi = *std::max_element(before.begin(), before.end()) + root_ms;
            std::vector<double> sh(nranks, 1.0 / nranks);
            for (int it = 0; it < 60; ++it) {            // bisection on the common finishing time
                const double t_end = 0.5 * (lo + hi);
                double sum = 0.0;
                for (int q = 0; q < nranks; ++q) sum += std::min(smax, std::max(smin, (t_end - before[q]) / root_ms));
                if (sum > 1.0) hi = t_end; else lo = t_end;
            }
            double sum = 0.0;
            for (int q = 0; q < nranks; ++q) { sh[q] = std::min(smax, std::max(smin, (0.5 * (lo + hi) - before[q]) / root_ms)); sum += sh[q]; }
            cum.assign(nranks + 1, 0.0);
            for (int q = 0; q < nranks; ++q) cum[q + 1] = cum[q] + sh[q] / sum;
            cum[nranks] = 1.0;
        }
    }
    in.phase_in = phase.data(); in.load_top = 2; in.rank = rank; in.nranks = nranks;
    in.top_mask = mask.data();
    in.root_cum = cum.empty() ? nullptr : cum.data();
    return SF_OK;
}

// ---------------- what is left: assembly masks, claim counters, host copies of the structure ----------------
static void finish_schedule(const PlanInput& in, const Layout& lay, PlanTables& T, SfSchedule& p) {
    if (in.ooc()) {
        // one assembly mask per group, then the top's: d_loadmask + g * nsuper (g = ooc_ngroups: the top)
        T.loadmask.assign((size_t)(in.ooc_ngroups + 1) * (size_t)std::max<sf_long>(in.nsuper, 1), 0);
        for (sf_long s = 0; s < in.nsuper; ++s) {
            const int unit = in.ooc_group[s] >= 0 ? in.ooc_group[s] : (in.ooc_top_mode >= 1 ? p.ooc_first[(size_t)s] : in.ooc_ngroups);
            T.loadmask[(size_t)unit * (size_t)in.nsuper + (size_t)s] = 1;
        }
        if (in.ooc_top_mode >= 1) {        // what a group's first launch zeroes besides its buffer: the places of the top panels that start with it
            p.ooc_zero.assign((size_t)in.ooc_ngroups, {});
            for (sf_long s = 0; s < in.nsuper; ++s)
                if (in.ooc_group[s] < 0) {
                    auto& z = p.ooc_zero[(size_t)p.ooc_first[(size_t)s]];
                    const int64_t o = lay.XP[s], len = in.nscol(s) * in.nsrow(s);
                    if (!z.empty() && z.back().first + z.back().second == o) z.back().second += len;
                    else z.push_back({o, len});
                }
        }
    } else if (p.partial) {
        T.loadmask.assign((size_t)std::max<sf_long>(in.nsuper, 1), 0);
        // the matrix entries of a shared top panel enter the sum once: on the first rank of its group (load_top == 2),
        // or on the rank the caller names (load_top 0 / 1: the older interface, one group of all ranks)
        for (sf_long s = 0; s < in.nsuper; ++s)
            T.loadmask[(size_t)s] = (p.phase[s] == 0 || (p.phase[s] == 1 && (in.load_top == 2 ? lay.group_idx(lay.gmask[s]) == 0 : in.load_top != 0))) ? 1 : 0;
    }
    // GEMM launches: 8 claim counters each (one per XCD) for the dynamic deal of their whole-tile rounds, behind the k_step launches' own
    for (Launch& L : p.launches)
        if (launch_is_gemm(L.kind)) { L.ticket = p.n_tickets; p.n_tickets += 8; }
    p.n_flags = std::max<int32_t>(T.n_flags, 1);
    p.h_Lsip.assign(in.Lsip, in.Lsip + in.nsuper + 1);
    p.h_Lsxp.assign(in.Lsxp, in.Lsxp + in.nsuper + 1);
    p.h_Super.resize((size_t)in.nsuper + 1);
    for (sf_long k = 0; k <= in.nsuper; ++k) p.h_Super[(size_t)k] = (int32_t)in.Super[k];
    if (!in.lu) {       // the row lists, for the update paths (sf_updown_path.cpp)
        const sf_long isize = in.nsuper > 0 ? in.Lsip[in.nsuper] : 0;
        p.h_Lsi.resize((size_t)isize);
        for (sf_long k = 0; k < isize; ++k) p.h_Lsi[(size_t)k] = (int32_t)in.Lsi[k];
    }
}

// ---------------- the whole of it ----------------
// plan_create (sf_plan_build.hip) calls the three entry points in this order, with its own steps in between.  Ways out, in the order
// the checks fire (every one leaves *out null; the plan, once it exists, goes through sf_chol_plan_destroy):
//   out == nullptr                                                                        SF_ERR_ARG
//   sf_schedule_check_arguments   rank / nranks out of range, several ranks without a phase array     SF_ERR_ARG
//                     out of core with several ranks, a phase array or > 32767 groups     SF_ERR_ARG
//                     negative sizes, a missing array, n >= 2^31 - 1                      SF_ERR_ARG
//   plan_create       no HIP device                                                       SF_ERR_NO_DEVICE
//                     device out of range / hipSetDevice fails                            SF_ERR_ARG / SF_ERR_HIP
//   the plan cannot be allocated                                                          SF_ERR_ALLOC
//   sf_schedule_layout   ooc_group[s] or phase_in[s] out of range                         SF_ERR_ARG
//                     a stored top supernode whose mask does not list this rank           SF_ERR_ARG
//                     top mode > 2, or no layout of the top arena                         SF_ERR_ARG
//   -- the factor-buffer offer is taken here (EarlyDevice::start); everything above leaves it standing --
//   sf_schedule_build:
//   validate_structure  supernode shapes, Super / Lsxp bounds; column pointers; row lists, SuperMap, entries without a place   SF_ERR_ARG
//   tree_levels       not postordered; a row of a stored supernode without a stored target, a streamed supernode that
//                     updates another group                                               SF_ERR_ARG
//   schedule_factorization   an LU fused step without its pre-update task                 SF_ERR_ARG
//   kstep_prefixes    a launch of 2^31 or more units                                      SF_ERR_ARG
//   create_device_resources  streams, events, copies, kernels of the maps                 SF_ERR_HIP
//                     the factor, a hipMalloc of a scratch or map buffer                  SF_ERR_ALLOC
//                     an upload (early ones included)                                     SF_ERR_HIP
int sf_schedule_build(const PlanInput& in, const PlanKnobs& kn, SfSchedule& p, sf::DlSchedule& dl, Layout& lay, PlanTables& T, double* stamps) {
    double none[4];
    double* t = stamps ? stamps : none;
    t[0] = now_ms();
    if (int rc = validate_structure(in, p)) return rc;
    if (int rc = tree_levels(in, p)) return rc;
    t[1] = now_ms();
    if (int rc = schedule_factorization(in, kn, lay, level_sets(in, lay, p), T, p)) return rc;
    t[2] = now_ms();
    schedule_solve(in, kn, lay, T, p);
    if (int rc = kstep_prefixes(T, p)) return rc;
    schedule_download(in, kn, lay, T, p, dl);
    finish_schedule(in, lay, T, p);
    t[3] = now_ms();
    return SF_OK;
}
