// Device plan of the supernodal Cholesky / LU numeric factorization: its release, the values and the stream it works on, execution
// (run_launches, the segments of a distributed top, the hipGraph form), validation, reading the factor
// back and importing one, the pivoting policy and the statistics of a plan.  The plan itself -- the level-by-level sweep, its
// launch list and task tables, the solve and download schedules, the device resources -- is built in sf_plan_build.hip; the
// overlapped download (sf_chol_plan_factorize_to_host) is sf_download.hip; the solves and everything else that takes columns
// through the resident factor live in files of their own (sf_solve.hip, sf_apply.hip and the entry points' files).
#include <sparseframe_hip.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sf_plan_internal.h"
#include "sf_symbolic.h"

extern "C" {

int sf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

size_t sf_device_memory(int device) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
    return (size_t)prop.totalGlobalMem;
}

size_t sf_reference_slot_size(int ndev, size_t min_mem) {
    if (ndev <= 0) return 0;
    // C:36-41 numSplit = max(GPU_SPLIT_LIMIT / numGPU_physical, 1), GPU_SPLIT_LIMIT = 4 (parameter.h:19);
    // C:82-87: (mem - 64 MiB) * 0.9 / numSplit / 8 slots, rounded down to 1 MiB; C:199 devSlotSize = that
    const int numSplit = std::max(4 / ndev, 1);
    size_t m = (size_t)(((double)min_mem - 64.0 * (0x400 * 0x400)) * 0.9);
    m /= numSplit;
    m /= 8;
    m -= m % (0x400 * 0x400);
    return m;
}

int sf_plan_factor_borrowed(const sf_chol_plan* p) { return p && p->factor_borrowed ? 1 : 0; }

int sf_chol_plan_destroy(sf_chol_plan* p) {
    delete p;
    return SF_OK;
}

// the group of ranks that sums segment k's block columns (bit r = rank r); 0 for a plan that is not distributed
uint32_t sf_chol_plan_segment_group(const sf_chol_plan* p, sf_long k) {
    return (p && k >= 0 && k < (sf_long)p->segments.size()) ? p->segments[k].mask : 0u;
}

int sf_chol_plan_set_values(sf_chol_plan* p, const sf_float* Lx) {
    if (!p || p->lu || (!Lx && p->nnz > 0)) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    if (p->nnz > 0) HIP_TRY(hipMemcpyAsync(p->d_Lx, Lx, p->nnz * sizeof(double), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->values_set = true;
    ++p->factor_gen;        // the resident factor (and a selected inverse from it) no longer belongs to the values
    return SF_OK;
}

int sf_lu_plan_set_values(sf_lu_plan* p, const sf_float* Lx, const sf_float* Ux) {
    if (!p || !p->lu || (!Lx && p->nnz > 0) || (!p->u_alias && !Ux && p->unz > 0)) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    if (p->nnz > 0) HIP_TRY(hipMemcpyAsync(p->d_Lx, Lx, p->nnz * sizeof(double), hipMemcpyHostToDevice, p->stream));
    if (!p->u_alias && p->unz > 0) HIP_TRY(hipMemcpyAsync(p->d_Ux, Ux, p->unz * sizeof(double), hipMemcpyHostToDevice, p->stream));
    {   // max |a_ij|: scale of the pivot perturbation
        double m = 0;
        for (int64_t k = 0; k < p->nnz; ++k) m = std::max(m, std::fabs(Lx[k]));
        if (!p->u_alias) for (int64_t k = 0; k < p->unz; ++k) m = std::max(m, std::fabs(Ux[k]));
        p->amax = m;
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->values_set = true;
    ++p->factor_gen;
    return SF_OK;
}

int sf_chol_plan_sync(sf_chol_plan* p) {
    if (!p) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    int info = 0;
    HIP_TRY(hipMemcpy(&info, p->d_info, sizeof(int), hipMemcpyDeviceToHost));
    float ms = 0;
    // (a run driven segment by segment never records ev1: the call then fails, and the error must not stay behind as the thread's
    // "last error" -- a caller that checks hipGetLastError after its own launches, as PyTorch does, would trip over it)
    if (elapsed_ms(&ms, p->ev0, p->ev1)) p->last_ms = ms;
    if (p->lu) HIP_TRY(hipMemcpy(&p->last_perturbed, p->d_piv + 2 * std::max<int64_t>(p->n, 1), sizeof(int), hipMemcpyDeviceToHost));
    // 1: non-positive / zero pivot; 2: a fused step's flag wait timed out (internal error, never seen)
    p->last_status = (info & 2) ? SF_ERR_HIP : (info ? SF_ERR_NOT_POSDEF : SF_OK);
    if (p->last_status == SF_OK && p->fact_done) p->ok_gen = p->fact_gen;
    return p->last_status;
}

// This rank's window [lo, hi) of a launch's `total` divisible items (GEMM launches: stream-K units; k_update_small: tiles); all of
// them unless the launch is split over a group.  The boundaries are the same doubles on the two ranks they separate, so the windows
// of a group's members tile [0, total) exactly (checked for every launch of 256^3 / 8 by tests/test_config4_schedules.py).
static inline void launch_window(const Launch& L, int64_t total, int64_t* lo, int64_t* hi) {
    *lo = 0; *hi = total;
    if (!L.split) return;
    *lo = (int64_t)((double)total * L.share_lo);
    *hi = L.share_hi >= 1.0 ? total : (int64_t)((double)total * L.share_hi);
}

// launches [l0, l1); first: start of a factorization (timer, memset, assembly); last: its end (timer, status)
static int run_launches(sf_chol_plan* p, size_t l0, size_t l1, bool first, bool last, int sync) {
    if (!p->values_set) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    if (p->ooc_groups > 1 && !p->dl.active) return SF_ERR_ARG;      // an out-of-core plan only exists together with its copy-back
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = p->stream;
    struct EventList {      // profiling events; destroyed on every exit path
        std::vector<hipEvent_t> v;
        ~EventList() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
    } evlist;
    std::vector<hipEvent_t>& evs = evlist.v;
    auto mark = [&]() {
        if (!p->profiling) return;
        hipEvent_t e;
        if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, st); evs.push_back(e); }
    };
    if (first) {
        if (!p->capturing) HIP_TRY(hipEventRecord(p->ev0, st));
        p->packed_pending = -1;
        p->epoch = (p->epoch == 0x7fffffff) ? 1 : p->epoch + 1;     // flag value of this factorization's fused steps (never 0)
        p->fact_gen = ++p->factor_gen;
        p->upd_failed = false;
        p->fact_done = false;
        if (p->capturing) {
            // a captured factorization is replayed with the SAME kernel arguments: its flag value is fixed (never seen in the array
            // again: epochs only grow) and the flags are cleared by a node of the graph itself
            p->graph_epoch = p->epoch;
            HIP_TRY(hipMemsetAsync(p->d_flags, 0, (size_t)p->n_flags * sizeof(int), st));
        }
    }
    sf::PivotCtl pc{0.0, 0.0, nullptr, nullptr, nullptr};
    if (p->lu) {
        const bool piv = p->piv_tol > 0.0;
        pc.tol = p->piv_tol;
        pc.eps = p->piv_perturb * p->amax;
        pc.pivpos = piv ? p->d_piv : nullptr;
        pc.pivinv = piv ? p->d_piv + std::max<int64_t>(p->n, 1) : nullptr;
        pc.nperturb = (int*)(p->d_piv + 2 * std::max<int64_t>(p->n, 1));
        if (first) HIP_TRY(hipMemsetAsync(pc.nperturb, 0, sizeof(int), st));
    }
    // the matrix entries of the panels `mask` selects (nullptr: all) into the zeroed panels
    auto assemble = [&](const int8_t* mask, hipStream_t s_) {
        if (!mask && p->d_loadmapL) {           // a whole plan: the entries' places are known (plan_create)
            sf::launch_load_mapped(p->d_Lx, p->d_loadmapL, p->nnz, p->d_Lsx, s_);
            if (p->lu) sf::launch_load_mapped(p->u_alias ? p->d_Lx : p->d_Ux, p->d_loadmapU, p->u_alias ? p->nnz : p->unz, p->d_Lsx, s_);
            return;
        }
        const int64_t* xp = (p->lu || p->partial) ? p->d_Xp : p->d_Lsxp;
        if (!p->lu) {
            sf::launch_load_panels(p->d_Lp, p->d_Li, p->d_Lx, (int32_t)p->n, p->d_Super, p->d_SuperMap, p->d_Lsip,
                                   p->d_Lsi, xp, p->d_Lsx, 0, mask, s_);
        } else {
            // L panel: strictly lower entries of the columns of L; U^T panel: row j of U (diagonal included) goes to
            // column j of PU at the positions of its column indices (reference loadA, L:2490-2533)
            sf::launch_load_panels(p->d_Lp, p->d_Li, p->d_Lx, (int32_t)p->n, p->d_Super, p->d_SuperMap, p->d_Lsip,
                                   p->d_Lsi, xp, p->d_Lsx, 1, mask, s_);
            if (p->u_alias)
                sf::launch_load_panels(p->d_Lp, p->d_Li, p->d_Lx, (int32_t)p->n, p->d_Super, p->d_SuperMap, p->d_Lsip,
                                       p->d_Lsi, xp, p->d_Lsx + p->xC, 0, mask, s_);
            else
                sf::launch_load_panels(p->d_Up, p->d_Ui, p->d_Ux, (int32_t)p->n, p->d_Super, p->d_SuperMap, p->d_Lsip,
                                       p->d_Lsi, xp, p->d_Lsx + p->xC, 0, mask, s_);
        }
    };
    if (first) {
        HIP_TRY(hipMemsetAsync(p->d_info, 0, (1 + p->n_tickets) * sizeof(int), st));
        if (p->xC > 0) HIP_TRY(hipMemsetAsync(p->d_Lsx, 0, (p->lu ? 2 : 1) * p->xC * sizeof(double), st));
        // (out of core: the top panels only; every group assembles its own buffer when its turn comes, LAUNCH_OOC_GROUP)
        assemble(p->ooc_groups > 1 ? p->d_loadmask + (size_t)p->ooc_groups * (size_t)p->nsuper : p->d_loadmask, st);
    }
    mark();
    std::vector<int> kinds;
    for (size_t li = l0; li < l1; ++li) {
        const Launch& L = p->launches[li];
        switch (L.kind) {
            case LAUNCH_POTRF:
                if (p->lu) sf::launch_getrf(p->d_potrf + L.first, L.count, p->d_Lsx, p->xC, p->d_info, pc, st);
                else sf::launch_potrf(p->d_potrf + L.first, L.count, p->d_Lsx, p->d_info, st);
                break;
            case LAUNCH_TRSM: sf::launch_trsm(p->d_trsm + L.first, L.count, p->d_Lsx, pc.pivinv, st); break;
            case LAUNCH_OOC_GROUP: {       // out of core: group L.first takes over buffer L.first & 1
                const int g = (int)L.first;
                if (int rc = sf_dl_wait_groups(p, g)) return rc;    // ... once the pieces that lie in it have left the device
                if (g >= 2 && p->ooc_buf > 0) {      // (the first factorization step zeroed everything: groups 0 and 1 find clean buffers)
                    const size_t off = (size_t)(g & 1) * (size_t)p->ooc_buf, nb = (size_t)p->ooc_buf * sizeof(double);
                    HIP_TRY(hipMemsetAsync(p->d_Lsx + off, 0, nb, st));
                    if (p->lu) HIP_TRY(hipMemsetAsync(p->d_Lsx + p->xC + off, 0, nb, st));
                }
                if (p->ooc_top_mode >= 1)       // the top panels that become active with this group (their places may have held others)
                    for (const auto& z : p->ooc_zero[(size_t)g]) {
                        HIP_TRY(hipMemsetAsync(p->d_Lsx + z.first, 0, (size_t)z.second * sizeof(double), st));
                        if (p->lu) HIP_TRY(hipMemsetAsync(p->d_Lsx + p->xC + z.first, 0, (size_t)z.second * sizeof(double), st));
                    }
                assemble(p->d_loadmask + (size_t)g * (size_t)p->nsuper, st);
                break;
            }
            case LAUNCH_UPDATE_SMALL: {       // k_update_small; a split launch (distributed top): this rank's share of the tiles (the update is a sum)
                int64_t lo, hi;
                launch_window(L, L.count, &lo, &hi);
                sf::launch_update_small(p->d_probs, p->d_stasks + L.first + lo, (int)(hi - lo), p->d_Lsx, p->d_relmap, st);
                break;
            }
            case LAUNCH_STEP:
                sf::launch_step(p->d_steps + L.first, L.count, p->lu ? 1 : 0, p->d_Lsx, p->d_flags, p->epoch, p->d_info, p->d_tinv,
                                p->d_info + 1 + L.ticket, pc, st);
                break;
            case LAUNCH_GEMM_INNER:
            case LAUNCH_GEMM_SCATTER:
            case LAUNCH_GEMM_OUTER: {
                int64_t w0, w1;
                launch_window(L, L.units, &w0, &w1);
                const uint32_t u0 = (uint32_t)w0, u1 = (uint32_t)w1;
                sf::launch_gemm(p->d_probs, p->d_gtasks + L.first, p->d_ktprefix + L.prefix_first, L.count, u0, u1,
                                L.kind == LAUNCH_GEMM_SCATTER ? 1 : 0, p->d_Lsx, p->d_relmap, p->gemm_dynamic ? p->d_info + 1 + L.ticket : nullptr, st,
                                (L.whole_tiles && !L.split) ? 1 : 0, 0);
                break;
            }
        }
        if (p->profiling) { kinds.push_back(L.kind); mark(); }
        if (p->dl.active) HIP_TRY(sf_dl_publish(p, li + 1));
    }
    if (last && !p->capturing) HIP_TRY(hipEventRecord(p->ev1, st));
    HIP_TRY(hipGetLastError());
    if (p->profiling) {
        HIP_TRY(hipStreamSynchronize(st));
        if (first) {
            p->last_load_ms = p->last_panel_ms = p->last_update_ms = 0;
            for (double& v : p->last_kind_ms) v = 0;
        }
        float ms = 0;
        if (first && !evs.empty() && elapsed_ms(&ms, p->ev0, evs[0])) p->last_load_ms = ms;
        FILE* dump = nullptr;
        if (const char* path = getenv("SF_PROFILE_DUMP")) dump = fopen(path, first ? "w" : "a");
        if (dump && first) fprintf(dump, "launch,kind,tasks,units,flops,ms\n");
        for (size_t k = 0; k + 1 < evs.size(); ++k) {
            if (!elapsed_ms(&ms, evs[k], evs[k + 1])) continue;
            if (kinds[k] == LAUNCH_GEMM_SCATTER) p->last_update_ms += ms; else if (kinds[k] != LAUNCH_UPDATE_SMALL) p->last_panel_ms += ms;
            p->last_kind_ms[kinds[k]] += ms;
            if (dump) {
                const Launch& L = p->launches[l0 + k];
                fprintf(dump, "%zu,%d,%d,%u,%.6e,%.4f\n", l0 + k, L.kind, L.count, L.units, L.flops, ms);
            }
        }
        if (dump) fclose(dump);
    }
    if (last) p->fact_done = true;
    if (sync) {
        if (!last) { HIP_TRY(hipStreamSynchronize(st)); return SF_OK; }
        return sf_chol_plan_sync(p);
    }
    return SF_OK;
}

// phase 0: assemble + owned subtrees; phase 1: top supernodes (replicated); -1: both (single-GPU path)
int sf_chol_plan_factorize_phase(sf_chol_plan* p, int which, int sync) {
    if (!p || which < -1 || which > 1) return SF_ERR_ARG;
    if (p->nranks > 1 && which != 0) return SF_ERR_ARG;      // distributed top: phase 1 runs segment by segment
    const size_t l0 = (which == 1) ? p->launch_split : 0;
    const size_t l1 = (which == 0) ? p->launch_split : p->launches.size();
    // a distributed plan without top supernodes (a forest of independent trees) is finished after phase 0
    const bool last = (which != 0) || (p->nranks > 1 && p->segments.empty());
    return run_launches(p, l0, l1, which != 1, last, sync);
}

sf_long sf_chol_plan_num_segments(const sf_chol_plan* p) { return p ? (sf_long)p->segments.size() : 0; }

// ---- schedule inspection (real and schedule-only plans; tests/test_config4_schedules.py, tools/) ----
sf_long sf_chol_plan_num_launches(const sf_chol_plan* p) { return p ? (sf_long)p->launches.size() : 0; }

int sf_chol_plan_launch_info(const sf_chol_plan* p, sf_long k, sf_long* out) {
    if (!p || !out || k < 0 || k >= (sf_long)p->launches.size()) return SF_ERR_ARG;
    const Launch& L = p->launches[(size_t)k];
    const bool gemm = launch_is_gemm(L.kind);
    const int64_t total = gemm ? (int64_t)L.units : (int64_t)L.count;
    int64_t lo, hi;
    launch_window(L, total, &lo, &hi);
    sf_long seg = -1;
    if ((size_t)k >= p->launch_split && !p->segments.empty()) {
        size_t a = 0, b = p->segments.size();       // last segment with l0 <= k
        while (b - a > 1) { const size_t m = (a + b) / 2; if (p->segments[m].l0 <= (size_t)k) a = m; else b = m; }
        if (p->segments[a].l0 <= (size_t)k && (size_t)k < p->segments[a].l1) seg = (sf_long)a;
    }
    out[0] = L.kind; out[1] = L.count; out[2] = total; out[3] = L.split ? 1 : 0; out[4] = lo; out[5] = hi;
    out[6] = (L.whole_tiles && !L.split) ? 1 : 0; out[7] = seg; out[8] = L.share_idx; out[9] = L.share_cnt;
    return SF_OK;
}

int sf_chol_plan_segment_info(const sf_chol_plan* p, sf_long k, sf_long* out) {
    if (!p || !out || k < 0 || k >= (sf_long)p->segments.size()) return SF_ERR_ARG;
    const Segment& sg = p->segments[(size_t)k];
    out[0] = (sf_long)sg.mask; out[1] = (sf_long)sg.l0; out[2] = (sf_long)sg.l1; out[3] = sg.packed; out[4] = sg.early ? 1 : 0;
    out[5] = (sf_long)sg.off.size();
    return SF_OK;
}

// owner-computes prototype (SF_TOP_OWNER=1): out[0] = group index of the rank that runs the block's near GEMM and chain (-1: everybody,
// the default), out[1] = number of launches of that part (the segment's first out[1] launches)
int sf_chol_plan_segment_owner(const sf_chol_plan* p, sf_long k, sf_long* out) {
    if (!p || !out || k < 0 || k >= (sf_long)p->segments.size()) return SF_ERR_ARG;
    const Segment& sg = p->segments[(size_t)k];
    out[0] = sg.owner_gi;
    out[1] = sg.owner_gi >= 0 ? (sf_long)(sg.lc - sg.l0) : 0;
    return SF_OK;
}

int sf_chol_plan_panel_offsets(const sf_chol_plan* p, sf_long* xp) {
    if (!p || (!xp && p->nsuper > 0)) return SF_ERR_ARG;
    for (int64_t s = 0; s < p->nsuper; ++s) xp[s] = p->h_XP[(size_t)s];
    return SF_OK;
}

sf_long sf_chol_plan_num_solve_reduces(const sf_chol_plan* p) { return p ? (sf_long)p->solve_reduces.size() : 0; }

int sf_chol_plan_solve_reduce_info(const sf_chol_plan* p, sf_long k, sf_long* out) {
    if (!p || !out || k < 0 || k >= (sf_long)p->solve_reduces.size()) return SF_ERR_ARG;
    out[0] = (sf_long)p->solve_reduces[(size_t)k].mask; out[1] = p->solve_reduces[(size_t)k].off; out[2] = p->solve_reduces[(size_t)k].cnt;
    return SF_OK;
}

int sf_chol_plan_segment_regions(const sf_chol_plan* p, sf_long k, sf_long capacity, sf_long* nregions, sf_long* offsets, sf_long* counts) {
    if (!p || k < 0 || k >= (sf_long)p->segments.size() || !nregions) return SF_ERR_ARG;
    const Segment& sg = p->segments[k];
    *nregions = (sf_long)sg.off.size();
    if (offsets && counts) {
        if (capacity < (sf_long)sg.off.size()) return SF_ERR_ARG;
        for (size_t i = 0; i < sg.off.size(); ++i) { offsets[i] = sg.off[i]; counts[i] = sg.cnt[i]; }
    }
    return SF_OK;
}

// gather the possibly non-zero part of segment k's regions into one contiguous buffer (strided device copies on
// the plan's stream): ONE all-reduce per segment, and the structurally zero rows above each block's diagonal
// (half of a square root panel) stay off the wire
static int seg_copy(sf_chol_plan* p, const Segment& sg, double* buf, bool pack, hipStream_t st) {
    int64_t pos = 0;
    for (size_t i = 0; i < sg.src.size(); ++i) {
        if (pack)
            HIP_TRY(hipMemcpy2DAsync(buf + pos, sg.rows[i] * sizeof(double), p->d_Lsx + sg.src[i], sg.ld[i] * sizeof(double),
                                     sg.rows[i] * sizeof(double), sg.cols[i], hipMemcpyDeviceToDevice, st));
        else
            HIP_TRY(hipMemcpy2DAsync(p->d_Lsx + sg.src[i], sg.ld[i] * sizeof(double), buf + pos, sg.rows[i] * sizeof(double),
                                     sg.rows[i] * sizeof(double), sg.cols[i], hipMemcpyDeviceToDevice, st));
        pos += sg.rows[i] * sg.cols[i];
    }
    return SF_OK;
}

int sf_chol_plan_segment_pack(sf_chol_plan* p, sf_long k, void** dptr, sf_long* count) {
    if (!p || k < 0 || k >= (sf_long)p->segments.size() || !dptr || !count) return SF_ERR_ARG;
    if (p->packed_pending >= 0) return SF_ERR_ARG;           // the previous packed segment has not been run
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    const Segment& sg = p->segments[k];
    double* buf = p->d_scratch + (k & 1) * p->scratch_elems;
    int rc = seg_copy(p, sg, buf, true, p->stream);
    if (rc) return rc;
    p->packed_pending = k;
    *dptr = (void*)buf;
    *count = sg.packed;
    return SF_OK;
}

int sf_chol_plan_factorize_segment(sf_chol_plan* p, sf_long k, int sync) {
    if (!p || k < 0 || k >= (sf_long)p->segments.size()) return SF_ERR_ARG;
    const Segment& sg = p->segments[k];
    if (p->packed_pending >= 0) {
        if (p->packed_pending != k) return SF_ERR_ARG;
        if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
        HIP_TRY(hipSetDevice(p->device));
        int rc = seg_copy(p, sg, p->d_scratch + (k & 1) * p->scratch_elems, false, p->stream);
        if (rc) return rc;
        p->packed_pending = -1;
    }
    const bool last = k + 1 == (sf_long)p->segments.size();
    if (sg.owner_gi >= 0) {
        // owner-computes prototype driven from outside (tools/emulate_rank.py: no collectives, timing only): the owner's part, then the rest
        const bool mine = sg.owner_gi == __builtin_popcount(sg.mask & ((1u << p->rank) - 1u));
        if (mine && sg.lc > sg.l0) { const int rc = run_launches(p, sg.l0, sg.lc, false, false, 0); if (rc) return rc; }
        return run_launches(p, sg.lc, sg.l1, false, last, sync);
    }
    return run_launches(p, sg.l0, sg.l1, false, last, sync);
}

}  // extern "C"

// Gathers a factor that is distributed over the plans of several ranks (sharded / mapped plans of ONE pattern, factorized and
// synchronised) into a whole plan of that pattern: every panel from the first part that stores it (a shared top panel is complete
// on every rank of its group once its chain has run), device to device over xGMI (hipMemcpyPeerAsync), LU: both panels and the
// pivot records.  After it `dst` solves as if it had factorized itself.  Used by the struct path's solve after a multi-handler
// factorization (sf_handlers.hip).
int sf_plan_import_from(sf_chol_plan* dst, sf_chol_plan* const* parts, int nparts) {
    if (!dst || dst->partial || !parts || nparts < 1) return SF_ERR_ARG;
    for (int r = 0; r < nparts; ++r) {
        const sf_chol_plan* P = parts[r];
        if (!P || P->n != dst->n || P->nsuper != dst->nsuper || P->lu != dst->lu || P->ooc_groups > 1) return SF_ERR_ARG;
        HIP_TRY(hipSetDevice(P->device));
        HIP_TRY(hipStreamSynchronize(P->stream));
    }
    HIP_TRY(hipSetDevice(dst->device));
    sf_long s = 0;
    while (s < dst->nsuper) {
        int src = -1;
        for (int r = 0; r < nparts && src < 0; ++r)
            if (parts[r]->h_XP[s] >= 0) src = r;
        if (src < 0) return SF_ERR_ARG;                 // a panel nobody stores
        const sf_chol_plan* P = parts[src];
        sf_long e = s;
        int64_t len = 0;
        while (e < dst->nsuper && P->h_XP[e] >= 0 && P->h_XP[e] == P->h_XP[s] + len && dst->h_XP[e] == dst->h_XP[s] + len) {
            bool earlier = false;                       // keep "the first part that stores it" for every panel of the run
            for (int r = 0; r < src; ++r) earlier = earlier || parts[r]->h_XP[e] >= 0;
            if (earlier) break;
            len += (dst->h_Super[e + 1] - dst->h_Super[e]) * (dst->h_Lsip[e + 1] - dst->h_Lsip[e]);
            ++e;
        }
        if (e == s) return SF_ERR_ARG;
        HIP_TRY(hipMemcpyPeerAsync(dst->d_Lsx + dst->h_XP[s], dst->device, P->d_Lsx + P->h_XP[s], P->device, len * sizeof(double), dst->stream));
        if (dst->lu) {
            HIP_TRY(hipMemcpyPeerAsync(dst->d_Lsx + dst->xC + dst->h_XP[s], dst->device, P->d_Lsx + P->xC + P->h_XP[s], P->device,
                                       len * sizeof(double), dst->stream));
            if (dst->d_piv && P->d_piv)
                HIP_TRY(hipMemcpyPeerAsync(dst->d_piv + dst->h_Super[s], dst->device, P->d_piv + dst->h_Super[s], P->device,
                                           (size_t)(dst->h_Super[e] - dst->h_Super[s]) * sizeof(int32_t), dst->stream));
        }
        s = e;
    }
    dst->piv_tol = parts[0]->piv_tol;
    dst->piv_perturb = parts[0]->piv_perturb;
    dst->hash_epoch = -1;           // the factor changed without a factorization of dst's own: cached fingerprints are stale
    dst->ok_gen = ++dst->factor_gen;        // ... and so is a selected inverse; the imported factor counts as factorized
    dst->upd_failed = false;
    HIP_TRY(hipStreamSynchronize(dst->stream));
    return SF_OK;
}

// The pieces of the pipelined driver (sf_multi.hip).  Segment k's sum uses half k & 1 of the scratch buffer and the plan's second
// stream:  begin (everything the sum needs has been enqueued on the main stream) -> pack on the second stream, returns the buffer for
// the collective, which the caller issues on sf_plan_stream2 -> reduced (marks the collective's end on the second stream) ->
// finish: the main stream waits for it, scatters the sums back and runs the segment's launches.
int sf_seg_begin(sf_chol_plan* p, sf_long k, void** dptr, sf_long* count) {
    if (!p || k < 0 || k >= (sf_long)p->segments.size() || !dptr || !count || !p->stream2) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    const int h = (int)(k & 1);
    HIP_TRY(hipEventRecord(p->ev_contrib[h], p->stream));
    HIP_TRY(hipStreamWaitEvent(p->stream2, p->ev_contrib[h], 0));
    // the half's previous user (segment k - 2) has been scattered back on the main stream
    if (p->unpacked_recorded[h]) HIP_TRY(hipStreamWaitEvent(p->stream2, p->ev_unpacked[h], 0));
    double* buf = p->d_scratch + h * p->scratch_elems;
    int rc = seg_copy(p, p->segments[k], buf, true, p->stream2);
    if (rc) return rc;
    *dptr = (void*)buf;
    *count = p->segments[k].packed;
    return SF_OK;
}
void* sf_plan_stream2(sf_chol_plan* p) { return p ? (void*)p->stream2 : nullptr; }
int sf_seg_reduced(sf_chol_plan* p, sf_long k) {
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipEventRecord(p->ev_reduced[k & 1], p->stream2));
    return SF_OK;
}
int sf_seg_finish(sf_chol_plan* p, sf_long k) {
    if (!p || k < 0 || k >= (sf_long)p->segments.size()) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    const int h = (int)(k & 1);
    const Segment& sg = p->segments[k];
    HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_reduced[h], 0));
    int rc = seg_copy(p, sg, p->d_scratch + h * p->scratch_elems, false, p->stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(p->ev_unpacked[h], p->stream));
    p->unpacked_recorded[h] = true;
    if (sg.owner_gi >= 0) {
        // the owner's part only (near GEMM + chain); sf_seg_bcast_begin / _finish follow
        const bool mine = sg.owner_gi == __builtin_popcount(sg.mask & ((1u << p->rank) - 1u));
        return (mine && sg.lc > sg.l0) ? run_launches(p, sg.l0, sg.lc, false, false, 0) : SF_OK;
    }
    return run_launches(p, sg.l0, sg.l1, false, k + 1 == (sf_long)p->segments.size(), 0);
}
int sf_seg_is_owner_segment(const sf_chol_plan* p, sf_long k) {
    return (p && k >= 0 && k < (sf_long)p->segments.size() && p->segments[(size_t)k].owner_gi >= 0) ? 1 : 0;
}
int sf_seg_bcast_begin(sf_chol_plan* p, sf_long k, void** dptr, sf_long* count) {
    if (!p || k < 0 || k >= (sf_long)p->segments.size() || !dptr || !count) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    const Segment& sg = p->segments[(size_t)k];
    if (sg.owner_gi < 0) return SF_ERR_ARG;
    double* buf = p->d_scratch + 2 * p->scratch_elems;
    const bool mine = sg.owner_gi == __builtin_popcount(sg.mask & ((1u << p->rank) - 1u));
    if (mine) { const int rc = seg_copy(p, sg, buf, true, p->stream); if (rc) return rc; }
    else if (sg.packed > 0) HIP_TRY(hipMemsetAsync(buf, 0, (size_t)sg.packed * sizeof(double), p->stream));
    *dptr = (void*)buf;
    *count = sg.packed;
    return SF_OK;
}
int sf_seg_bcast_finish(sf_chol_plan* p, sf_long k) {
    if (!p || k < 0 || k >= (sf_long)p->segments.size()) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    const Segment& sg = p->segments[(size_t)k];
    if (sg.owner_gi < 0) return SF_ERR_ARG;
    const int rc = seg_copy(p, sg, p->d_scratch + 2 * p->scratch_elems, false, p->stream);
    if (rc) return rc;
    // the block column is final on this rank NOW: its copy-back pieces carry "ready = lc + 1"; with launches behind the broadcast
    // run_launches publishes them after the first of those, without any it is done here
    if (p->dl.active && sg.lc == sg.l1) HIP_TRY(sf_dl_publish(p, sg.lc + 1));
    return run_launches(p, sg.lc, sg.l1, false, k + 1 == (sf_long)p->segments.size(), 0);
}
int sf_seg_early(const sf_chol_plan* p, sf_long k) { return (p && k >= 0 && k < (sf_long)p->segments.size() && p->segments[k].early) ? 1 : 0; }

extern "C" {

int sf_chol_plan_set_stream(sf_chol_plan* p, void* stream) {
    if (!p) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->stream.reset((hipStream_t)stream, false);
    p->own_stream = false;
    return SF_OK;
}


// SF_GRAPH=1: a whole resident factorization (memsets, assembly, every launch of the plan) is captured ONCE into a hipGraph and
// replayed -- one submission instead of ~1,500 at 128^3.  Only the plain resident form: no overlapped download (its events are
// recorded between the launches for host threads to wait on), no profiling, one rank, one lane.  The graph is rebuilt when a kernel
// argument it froze changes (the LU pivot threshold / perturbation scale, the plan's stream).
static int factorize_graph(sf_chol_plan* p, int sync) {
    HIP_TRY(hipSetDevice(p->device));
    const double eps = p->lu ? p->piv_perturb * p->amax : 0.0, tol = p->lu ? p->piv_tol : 0.0;
    if (p->graph_exec && (p->graph_tol != tol || p->graph_eps != eps || p->graph_stream != p->stream)) {
        p->graph_exec.reset();
    }
    bool fresh = false;
    if (!p->graph_exec) {
        fresh = true;
        hipGraph_t g = nullptr;
        HIP_TRY(hipStreamBeginCapture(p->stream, hipStreamCaptureModeThreadLocal));
        p->capturing = true;
        const int rc = run_launches(p, 0, p->launches.size(), true, true, 0);
        p->capturing = false;
        const hipError_t e = hipStreamEndCapture(p->stream, &g);
        if (rc || e != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); (void)hipGetLastError(); return rc ? rc : SF_ERR_HIP; }
        hipGraphExec_t ge = nullptr;
        const hipError_t ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ei != hipSuccess) { (void)hipGetLastError(); return SF_ERR_HIP; }
        p->graph_exec.reset(ge);
        p->graph_tol = tol; p->graph_eps = eps; p->graph_stream = p->stream;
    }
    // (the captured kernels compare the flags with graph_epoch and the graph clears the flags itself; p->epoch stays what it is for
    //  everybody else -- the generation of the factor on the device -- and moves on with every replay)
    if (!fresh) {
        p->epoch = (p->epoch == 0x7fffffff) ? 1 : p->epoch + 1;
        p->fact_gen = ++p->factor_gen;
        p->upd_failed = false;
        p->fact_done = true;
    }
    p->packed_pending = -1;
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    HIP_TRY(hipGraphLaunch(p->graph_exec, p->stream));
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    return sync ? sf_chol_plan_sync(p) : SF_OK;
}

int sf_chol_plan_factorize(sf_chol_plan* p, int sync) {
    if (p && !p->dry && p->values_set && p->use_graph && p->nranks == 1 && !p->partial && !p->dl.active && !p->profiling) {
        const int rc = factorize_graph(p, sync);
        if (rc != SF_ERR_HIP) return rc;
        p->use_graph = false;               // capture is not available here: the eager path from now on
        (void)hipGetLastError();
    }
    return sf_chol_plan_factorize_phase(p, -1, sync);
}

// The whole of SparseFrame_validate on the device (C:3141-3266, L:3702-3858): b_i = 1 + i/n, the supernodal solve with the
// resident factor, r = A x - b from the plan's copy of the matrix, residual = |r|_inf / (|A|_1 |x|_inf + |b|_inf).  Nothing
// but the scalar comes back (x_host may be NULL).
int sf_chol_plan_validate(sf_chol_plan* p, sf_float* residual, sf_float* x_host) {
    if (!p || !residual) return SF_ERR_ARG;
    if (p->partial || (p->nsuper > 0 && !p->d_solve) || !p->values_set) return SF_ERR_ARG;
    *residual = 0.0;
    if (p->n <= 0) return SF_OK;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    if (!p->d_resid) {
        if (p->d_resid.alloc(3 * (size_t)p->n + 4)) return SF_ERR_HIP;
        p->bytes_device += (3 * (size_t)p->n + 4) * sizeof(double);
    }
    std::vector<double> b(p->n), x(p->n);
    for (int64_t i = 0; i < p->n; ++i) b[i] = 1.0 + (double)i / (double)p->n;
    int rc = sf_chol_plan_solve(p, b.data(), x.data());          // leaves the solution in d_x
    if (rc) return rc;
    double* r = p->d_resid, *colsum = r + p->n, *bb = colsum + p->n, *norms = bb + p->n;
    HIP_TRY(hipMemsetAsync(norms, 0, 4 * sizeof(double), p->stream));
    const bool unsym = p->lu && !p->u_alias;
    sf::launch_residual(p->d_Lp, p->d_Li, p->d_Lx, unsym ? p->d_Up : nullptr, unsym ? p->d_Ui : nullptr, unsym ? p->d_Ux : nullptr,
                        (int32_t)p->n, p->d_x, r, colsum, bb, norms, p->stream);
    HIP_TRY(hipGetLastError());
    double h[4];
    HIP_TRY(hipMemcpyAsync(h, norms, sizeof(h), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    // k_resid_norms keeps a NaN (and an infinity) in its maxima: a non-finite r_i or x_i makes the residual NaN, which fails every
    // `residual <= tol`; the return code stays SF_OK
    *residual = (std::isfinite(h[0]) && std::isfinite(h[2])) ? h[0] / (h[1] * h[2] + h[3]) : std::numeric_limits<double>::quiet_NaN();
    if (x_host) memcpy(x_host, x.data(), p->n * sizeof(double));
    return SF_OK;
}

int sf_chol_plan_top_region(sf_chol_plan* p, void** dptr, sf_long* count) {
    if (!p || !dptr || !count) return SF_ERR_ARG;
    *dptr = (void*)(p->d_Lsx + p->top_off);
    *count = p->top_size;
    return SF_OK;
}

int sf_chol_plan_get_factor(sf_chol_plan* p, sf_float* Lsx) {
    if (!p || (!Lsx && p->xsize > 0)) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    if (p->ooc_groups > 1) return SF_ERR_ARG;       // an out-of-core plan's factor never exists on the device as a whole
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (p->xsize <= 0) return SF_OK;
    if (!p->lu && !p->partial) {
        HIP_TRY(hipMemcpy(Lsx, p->d_Lsx, p->xsize * sizeof(double), hipMemcpyDeviceToHost));
        return SF_OK;
    }
    if (!p->lu) {
        // sharded plan: copy the panels stored here to their reference positions, one copy per run of
        // supernodes that is contiguous in both layouts; panels of other ranks are left untouched
        sf_long s = 0;
        while (s < p->nsuper) {
            if (p->h_XP[s] < 0) { ++s; continue; }
            sf_long e = s;
            int64_t len = 0;
            while (e < p->nsuper && p->h_XP[e] == p->h_XP[s] + len) {
                len += p->h_Lsxp[e + 1] - p->h_Lsxp[e];
                ++e;
            }
            HIP_TRY(hipMemcpy(Lsx + p->h_Lsxp[s], p->d_Lsx + p->h_XP[s], len * sizeof(double), hipMemcpyDeviceToHost));
            s = e;
        }
        return SF_OK;
    }
    // (sharded LU: panels not stored on this rank come back as zeros, k_pack_lu skips them)
    if (!p->d_pack) {
        if (p->d_pack.alloc(p->xsize)) return SF_ERR_HIP;
        p->bytes_device += p->xsize * sizeof(double);
    }
    sf::launch_pack_lu(p->d_Super, p->d_Lsip, p->d_Xp, p->d_Lsxp, (int32_t)p->nsuper, p->d_Lsx, p->d_Lsx + p->xC,
                       p->d_pack, 0, p->xsize, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(Lsx, p->d_pack, p->xsize * sizeof(double), hipMemcpyDeviceToHost));
    return SF_OK;
}

// values [e_begin, e_end) of the factor in the reference layout (a whole plan only): what the struct path samples to make sure a
// host copy still is what the device holds before it solves with the resident factor
int sf_chol_plan_get_factor_range(sf_chol_plan* p, sf_long e_begin, sf_long e_end, sf_float* out) {
    if (!p || p->partial || e_begin < 0 || e_end > p->xsize || e_end < e_begin || (!out && e_end > e_begin)) return SF_ERR_ARG;
    if (e_end == e_begin) return SF_OK;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    if (!p->lu) {
        HIP_TRY(hipMemcpyAsync(out, p->d_Lsx + e_begin, (e_end - e_begin) * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return SF_OK;
    }
    sf::DevMem<double> tmp;
    if (tmp.alloc(e_end - e_begin)) return SF_ERR_HIP;
    sf::launch_pack_lu(p->d_Super, p->d_Lsip, p->d_Xp, p->d_Lsxp, (int32_t)p->nsuper, p->d_Lsx, p->d_Lsx + p->xC, tmp, e_begin, e_end, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, tmp, (e_end - e_begin) * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SF_OK;
}

int sf_plan_panel_hashes(sf_chol_plan* p, const uint64_t** out) {
    if (!p || !out || p->ooc_groups > 1) return SF_ERR_ARG;
    if (p->hash_epoch != p->epoch || p->h_hash.size() != (size_t)std::max<int64_t>(p->nsuper, 1)) {
        if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
        HIP_TRY(hipSetDevice(p->device));
        const size_t nh = (size_t)std::max<int64_t>(p->nsuper, 1), nb = nh * sizeof(unsigned long long);
        sf::DevMem<unsigned long long> d_h;
        if (d_h.alloc(nh)) return SF_ERR_HIP;
        const int64_t* xp = (p->lu || p->partial) ? p->d_Xp : p->d_Lsxp;
        p->hash_epoch = -1;     // (until the hashes have arrived)
        HIP_TRY(hipMemsetAsync(d_h, 0, nb, p->stream));
        sf::launch_factor_hash(p->d_Super, p->d_Lsip, xp, p->d_Lsxp, (int32_t)p->nsuper, p->d_Lsx, p->d_Lsx + p->xC, p->lu ? 1 : 0,
                               p->xsize, d_h, p->stream);
        HIP_TRY(hipGetLastError());
        p->h_hash.assign(nh, 0);
        HIP_TRY(hipMemcpyAsync(p->h_hash.data(), d_h, nb, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        p->hash_epoch = p->epoch;
    }
    *out = p->h_hash.data();
    return SF_OK;
}

int sf_lu_plan_set_pivoting(sf_lu_plan* p, double tol, double perturb) {
    if (!p || !p->lu || !(tol >= 0.0) || tol > 1.0 || !(perturb >= 0.0)) return SF_ERR_ARG;
    p->piv_tol = tol;
    p->piv_perturb = perturb;
    return SF_OK;
}

// pivpos[g] (global permuted index) = the row position original row g was given by the interchanges of its 64-column
// block; the identity where nothing moved, for panels not stored on this rank (left untouched) and when pivoting is off
int sf_lu_plan_get_pivots(sf_lu_plan* p, sf_long* pivpos) {
    if (!p || !p->lu || (!pivpos && p->n > 0)) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (!(p->piv_tol > 0.0)) {
        for (int64_t s = 0; s < p->nsuper; ++s)
            if (p->h_XP[s] >= 0)
                for (int64_t j = p->h_Super[s]; j < p->h_Super[s + 1]; ++j) pivpos[j] = j;
        return SF_OK;
    }
    std::vector<int32_t> h(std::max<int64_t>(p->n, 1));
    HIP_TRY(hipMemcpy(h.data(), p->d_piv, p->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < p->nsuper; ++s)
        if (p->h_XP[s] >= 0)
            for (int64_t j = p->h_Super[s]; j < p->h_Super[s + 1]; ++j) pivpos[j] = h[j];
    return SF_OK;
}

int sf_lu_plan_factorize(sf_lu_plan* p, int sync) { return (p && p->lu) ? sf_chol_plan_factorize(p, sync) : SF_ERR_ARG; }
int sf_lu_plan_sync(sf_lu_plan* p) { return sf_chol_plan_sync(p); }
int sf_lu_plan_get_factor(sf_lu_plan* p, sf_float* Lsx) { return (p && p->lu) ? sf_chol_plan_get_factor(p, Lsx) : SF_ERR_ARG; }
double sf_lu_plan_stat(const sf_lu_plan* p, const char* name) { return sf_chol_plan_stat(p, name); }
int sf_lu_plan_set_profiling(sf_lu_plan* p, int on) { return sf_chol_plan_set_profiling(p, on); }
int sf_lu_plan_destroy(sf_lu_plan* p) { return sf_chol_plan_destroy(p); }

void* sf_chol_plan_factor_device_ptr(sf_chol_plan* p) { return p ? (void*)p->d_Lsx : nullptr; }

int sf_chol_plan_set_profiling(sf_chol_plan* p, int on) {
    if (!p) return SF_ERR_ARG;
    p->profiling = on != 0;
    return SF_OK;
}

double sf_chol_plan_stat(const sf_chol_plan* p, const char* name) {
    if (!p || !name) return -1;
    const std::string k(name);
    if (k == "levels") return p->nlevels;
    if (k == "last_solve_ms") return p->last_solve_ms;
    if (k == "last_solve_many_ms") return p->last_solve_many_ms;
    if (k == "bytes_solve_many") return (double)p->bytes_solve_many;
    if (k == "solve_many_width") return (double)sf::SVM_W;
    if (k == "last_half_ms") return p->last_half_ms;
    if (k == "last_quadform_ms") return p->last_quadform_ms;
    if (k == "last_sample_ms") return p->last_sample_ms;
    if (k == "bytes_ordering") return (double)p->bytes_ordering;
    if (k == "ordering_set") return p->d_perm ? 1.0 : 0.0;
    if (k == "bytes_gram") return (double)p->bytes_gram;
    if (k == "last_gram_ms") return p->last_gram_ms;
    if (k == "last_gram_parts") return (double)p->last_gram_parts;
    if (k == "bytes_selinv") return (double)p->bytes_selinv;
    if (k == "last_selinv_ms") return p->last_selinv_ms;
    if (k == "flops_selinv") return p->flops_selinv;
    if (k == "selinv_valid") return (p->d_sel && p->sel_gen == p->factor_gen) ? 1.0 : 0.0;
    if (k == "bytes_selinv_pattern") return (double)p->bytes_selinv_pattern;
    if (k == "last_selinv_pattern_ms") return p->last_selinv_pattern_ms;
    if (k == "last_selinv_outside") return (double)p->last_selinv_outside;
    if (k == "selinv_pattern_chunk") return sf_selpat_constant(0);
    if (k == "selinv_pattern_tile") return sf_selpat_constant(1);
    if (k == "selinv_entries_chunk") return sf_selpat_constant(2);
    if (k == "selinv_pattern_max_m") return sf_selpat_constant(3);
    if (k == "factor_generation") return (double)p->factor_gen;
    if (k == "factor_usable") return (p->ok_gen >= 0 && p->ok_gen >= p->fact_gen && !p->upd_failed) ? 1.0 : 0.0;
    if (k == "bytes_adjoint") return (double)p->bytes_adjoint;
    if (k == "last_adjoint_ms") return p->last_adjoint_ms;
    if (k == "last_refine_iters") return (double)p->last_refine_iters;
    if (k == "last_refine_berr0") return p->last_refine_berr0;
    if (k == "last_refine_berr") return p->last_refine_berr;
    if (k == "last_refine_ms") return p->last_refine_ms;
    if (k == "last_residual_ms") return p->last_residual_ms;
    if (k == "bytes_refine") return (double)p->bytes_refine;
    if (k == "refine_row_entries") return (double)p->rf_entries;
    if (k == "last_condest_solves") return (double)p->last_condest_solves;
    if (k == "last_condest_ms") return p->last_condest_ms;
    if (k == "bytes_condest") return (double)p->bytes_condest;
    if (k == "last_updown_ms") return p->last_updown_ms;
    if (k == "update_path_supernodes") return (double)p->upd_path_supers;
    if (k == "update_path_columns") return (double)p->upd_path_cols;
    if (k == "update_launches") return (double)p->upd_launches;
    if (k == "update_bad_column") return (double)p->upd_bad_column;
    if (k == "rowmod_row_tasks") return (double)p->rowmod_row_tasks;
    if (k == "rowmod_sweep_supernodes") return (double)p->rowmod_sweep_supers;
    if (k == "rowmod_launches") return (double)p->rowmod_launches;
    if (k == "rowmod_bad_index") return (double)p->rowmod_bad_index;
    if (k == "rowmod_not_deleted") return (double)p->rowmod_not_deleted;
    if (k == "bytes_update") return (double)p->bytes_update;
    if (k == "perturbed_pivots") return (double)p->last_perturbed;
    if (k == "pivot_tol") return p->piv_tol;
    if (k == "last_to_host_ms") return p->last_to_host_ms;
    if (k == "download_pieces") return (double)p->dl.pieces.size();
    if (k == "top_doubles") return (double)p->top_size;
    if (k == "stored_doubles") return (double)p->xC;
    if (k == "launches") return (double)p->launches.size();
    if (k == "gemm_tasks") return (double)p->n_gemm_tasks;
    if (k == "update_pairs") return (double)p->n_pairs;
    if (k == "flops_exec") return p->flops_exec;
    if (k == "flops_update") return p->flops_update;
    if (k == "flops_panel_gemm") return p->flops_panel_gemm;
    if (k == "scatter_elems") return p->scatter_elems;
    if (k == "bytes_device") return (double)p->bytes_device;
    if (k == "last_ms") return p->last_ms;
    if (k == "last_load_ms") return p->last_load_ms;
    if (k == "last_panel_ms") return p->last_panel_ms;
    if (k == "last_update_ms") return p->last_update_ms;
    if (k == "last_potrf_ms") return p->last_kind_ms[LAUNCH_POTRF];
    if (k == "last_trsm_ms") return p->last_kind_ms[LAUNCH_TRSM];
    if (k == "last_inner_gemm_ms") return p->last_kind_ms[LAUNCH_GEMM_INNER];
    if (k == "last_outer_gemm_ms") return p->last_kind_ms[LAUNCH_GEMM_OUTER];
    if (k == "last_step_ms") return p->last_kind_ms[LAUNCH_STEP];
    if (k == "last_small_update_ms") return p->last_kind_ms[LAUNCH_UPDATE_SMALL];
    if (k == "flops_update_small") return p->flops_update_small;
    if (k == "flops_outer_gemm") return p->flops_outer_gemm;
    if (k == "flops_tiles") return p->flops_tiles;
    if (k == "flops_tiles_update") return p->flops_tiles_update;
    return -1;
}

}  // extern "C"
