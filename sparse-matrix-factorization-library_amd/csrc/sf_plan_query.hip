// Everything about a device plan that only reads: the devices, the schedule's inspection (real and schedule-only plans), where the
// factor lies on the device, and the statistics.
#include <sparseframe_hip.h>

#include <algorithm>
#include <string>

#include "sf_plan_internal.h"

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

int sf_chol_plan_top_region(sf_chol_plan* p, void** dptr, sf_long* count) {
    if (!p || !dptr || !count) return SF_ERR_ARG;
    *dptr = (void*)(p->d_Lsx + p->top_off);
    *count = p->top_size;
    return SF_OK;
}

void* sf_chol_plan_factor_device_ptr(sf_chol_plan* p) { return p ? (void*)p->d_Lsx : nullptr; }

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
    if (k == "selinv_valid") return (p->d_sel && p->fs.selinv_matches()) ? 1.0 : 0.0;
    if (k == "bytes_selinv_pattern") return (double)p->bytes_selinv_pattern;
    if (k == "last_selinv_pattern_ms") return p->last_selinv_pattern_ms;
    if (k == "last_selinv_outside") return (double)p->last_selinv_outside;
    if (k == "selinv_pattern_chunk") return sf_selpat_constant(0);
    if (k == "selinv_pattern_tile") return sf_selpat_constant(1);
    if (k == "selinv_entries_chunk") return sf_selpat_constant(2);
    if (k == "selinv_pattern_max_m") return sf_selpat_constant(3);
    if (k == "factor_generation") return (double)p->fs.factor_generation();
    if (k == "factor_usable") return (p->fs.usable() && !p->fs.broken()) ? 1.0 : 0.0;
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
double sf_lu_plan_stat(const sf_lu_plan* p, const char* name) { return sf_chol_plan_stat(p, name); }

}  // extern "C"
