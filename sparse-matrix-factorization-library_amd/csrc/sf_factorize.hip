// The factorization driver of a device plan: sf_run_launches enqueues a range of the plan's launch list on its stream (the start of
// a factorization, the launch switch, the out-of-core group step, the profiling report), the entry points that call it for a
// phase or a whole factorization, the hipGraph form, collecting the status (sf_chol_plan_sync) and the two questions about the
// factor's state that may have to collect first (sf_factor_state.h).  The launch list is built by sf_schedule.cpp /
// sf_plan_build.hip; the segments of a distributed top call sf_run_launches from sf_segments.hip, the overlapped download from
// sf_download.hip.
#include <sparseframe_hip.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sf_plan_internal.h"

namespace {

// the profiling events of one sf_run_launches call (none unless the plan is profiling); destroyed on every exit path
struct ProfileMarks {
    sf_chol_plan* p;
    std::vector<hipEvent_t> evs;
    std::vector<int> kinds;         // kinds[k]: the launch between evs[k] and evs[k + 1]
    ~ProfileMarks() { for (hipEvent_t e : evs) (void)hipEventDestroy(e); }
    void mark() {
        if (!p->profiling) return;
        hipEvent_t e;
        if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, p->stream); evs.push_back(e); }
    }
    // wait for the stream, add the launches' times to the plan's sums (first: from zero) and write the SF_PROFILE_DUMP rows
    int report(bool first, size_t l0) {
        HIP_TRY(hipStreamSynchronize(p->stream));
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
        return SF_OK;
    }
};

// LU: the pivoting policy as the kernels take it (Cholesky: nothing)
sf::PivotCtl pivot_ctl(const sf_chol_plan* p) {
    sf::PivotCtl pc{0.0, 0.0, nullptr, nullptr, nullptr};
    if (p->lu) {
        const bool piv = p->piv_tol > 0.0;
        pc.tol = p->piv_tol;
        pc.eps = p->piv_perturb * p->amax;
        pc.pivpos = piv ? p->d_piv : nullptr;
        pc.pivinv = piv ? p->d_piv + std::max<int64_t>(p->n, 1) : nullptr;
        pc.nperturb = (int*)(p->d_piv + 2 * std::max<int64_t>(p->n, 1));
    }
    return pc;
}

// the matrix entries of the panels `mask` selects (nullptr: all) into the zeroed panels
void assemble(sf_chol_plan* p, const int8_t* mask, hipStream_t s_) {
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
}

// the start of a factorization: the timer, the state, the words and panels the launches count on being zero, the first assembly
int start_factorization(sf_chol_plan* p, const sf::PivotCtl& pc, hipStream_t st) {
    if (!p->capturing) HIP_TRY(hipEventRecord(p->ev0, st));
    p->packed_pending = -1;
    p->fs.factorization_started();
    if (p->capturing) {
        // a captured factorization is replayed with the SAME kernel arguments: its flag value is fixed (never seen in the array
        // again: epochs only grow) and the flags are cleared by a node of the graph itself
        p->graph_epoch = p->fs.factor_epoch();
        HIP_TRY(hipMemsetAsync(p->d_flags, 0, (size_t)p->n_flags * sizeof(int), st));
    }
    if (p->lu) HIP_TRY(hipMemsetAsync(pc.nperturb, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(p->d_info, 0, (1 + p->n_tickets) * sizeof(int), st));
    if (p->xC > 0) HIP_TRY(hipMemsetAsync(p->d_Lsx, 0, (p->lu ? 2 : 1) * p->xC * sizeof(double), st));
    // (out of core: the top panels only; every group assembles its own buffer when its turn comes, LAUNCH_OOC_GROUP)
    assemble(p, p->ooc_groups > 1 ? p->d_loadmask + (size_t)p->ooc_groups * (size_t)p->nsuper : p->d_loadmask, st);
    return SF_OK;
}

// out of core: group g takes over buffer g & 1
int ooc_group_begin(sf_chol_plan* p, int g, hipStream_t st) {
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
    assemble(p, p->d_loadmask + (size_t)g * (size_t)p->nsuper, st);
    return SF_OK;
}

int enqueue_launch(sf_chol_plan* p, const Launch& L, const sf::PivotCtl& pc, hipStream_t st) {
    switch (L.kind) {
        case LAUNCH_POTRF:
            if (p->lu) sf::launch_getrf(p->d_potrf + L.first, L.count, p->d_Lsx, p->xC, p->d_info, pc, st);
            else sf::launch_potrf(p->d_potrf + L.first, L.count, p->d_Lsx, p->d_info, st);
            break;
        case LAUNCH_TRSM: sf::launch_trsm(p->d_trsm + L.first, L.count, p->d_Lsx, pc.pivinv, st); break;
        case LAUNCH_OOC_GROUP: return ooc_group_begin(p, (int)L.first, st);
        case LAUNCH_UPDATE_SMALL: {       // k_update_small; a split launch (distributed top): this rank's share of the tiles (the update is a sum)
            int64_t lo, hi;
            launch_window(L, L.count, &lo, &hi);
            sf::launch_update_small(p->d_probs, p->d_stasks + L.first + lo, (int)(hi - lo), p->d_Lsx, p->d_relmap, st);
            break;
        }
        case LAUNCH_STEP:
            sf::launch_step(p->d_steps + L.first, L.count, p->lu ? 1 : 0, p->d_Lsx, p->d_flags, p->fs.factor_epoch(), p->d_info, p->d_tinv,
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
    return SF_OK;
}

}  // namespace

int sf_run_launches(sf_chol_plan* p, size_t l0, size_t l1, bool first, bool last, int sync) {
    if (!p->fs.has_values()) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    if (p->ooc_groups > 1 && !p->dl.active) return SF_ERR_ARG;      // an out-of-core plan only exists together with its copy-back
    HIP_TRY(hipSetDevice(p->device));
    hipStream_t st = p->stream;
    ProfileMarks marks{p};
    const sf::PivotCtl pc = pivot_ctl(p);
    if (first)
        if (int rc = start_factorization(p, pc, st)) return rc;
    marks.mark();
    for (size_t li = l0; li < l1; ++li) {
        const Launch& L = p->launches[li];
        if (int rc = enqueue_launch(p, L, pc, st)) return rc;
        if (p->profiling) { marks.kinds.push_back(L.kind); marks.mark(); }
        if (p->dl.active) HIP_TRY(sf_dl_publish(p, li + 1));
    }
    if (last && !p->capturing) HIP_TRY(hipEventRecord(p->ev1, st));
    HIP_TRY(hipGetLastError());
    if (p->profiling)
        if (int rc = marks.report(first, l0)) return rc;
    if (last) p->fs.factorization_enqueued();
    if (sync) {
        if (!last) { HIP_TRY(hipStreamSynchronize(st)); return SF_OK; }
        return sf_chol_plan_sync(p);
    }
    return SF_OK;
}

bool sf_factor_usable(sf_chol_plan* p) {
    if (p->fs.needs_collect_for_usable()) (void)sf_chol_plan_sync(p);
    return p->fs.usable();
}

bool sf_factor_current(sf_chol_plan* p) {
    if (p->fs.needs_collect_for_current()) (void)sf_chol_plan_sync(p);
    return p->fs.current();
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
        const int rc = sf_run_launches(p, 0, p->launches.size(), true, true, 0);
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
    // (the captured kernels compare the flags with graph_epoch and the graph clears the flags itself; the state's epoch stays what it
    //  is for everybody else -- the generation of the factor on the device -- and moves on with every replay)
    if (!fresh) {
        p->fs.factorization_started();
        p->fs.factorization_enqueued();
    }
    p->packed_pending = -1;
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    HIP_TRY(hipGraphLaunch(p->graph_exec, p->stream));
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    return sync ? sf_chol_plan_sync(p) : SF_OK;
}

extern "C" {

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
    return p->fs.collected((info & 2) ? SF_ERR_HIP : (info ? SF_ERR_NOT_POSDEF : SF_OK));
}

// phase 0: assemble + owned subtrees; phase 1: top supernodes (replicated); -1: both (single-GPU path)
int sf_chol_plan_factorize_phase(sf_chol_plan* p, int which, int sync) {
    if (!p || which < -1 || which > 1) return SF_ERR_ARG;
    if (p->nranks > 1 && which != 0) return SF_ERR_ARG;      // distributed top: phase 1 runs segment by segment
    const size_t l0 = (which == 1) ? p->launch_split : 0;
    const size_t l1 = (which == 0) ? p->launch_split : p->launches.size();
    // a distributed plan without top supernodes (a forest of independent trees) is finished after phase 0
    const bool last = (which != 0) || (p->nranks > 1 && p->segments.empty());
    return sf_run_launches(p, l0, l1, which != 1, last, sync);
}

int sf_chol_plan_factorize(sf_chol_plan* p, int sync) {
    if (p && !p->dry && p->fs.has_values() && p->use_graph && p->nranks == 1 && !p->partial && !p->dl.active && !p->profiling) {
        const int rc = factorize_graph(p, sync);
        if (rc != SF_ERR_HIP) return rc;
        p->use_graph = false;               // capture is not available here: the eager path from now on
        (void)hipGetLastError();
    }
    return sf_chol_plan_factorize_phase(p, -1, sync);
}

int sf_chol_plan_set_stream(sf_chol_plan* p, void* stream) {
    if (!p) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->stream.reset((hipStream_t)stream, false);
    p->own_stream = false;
    return SF_OK;
}

int sf_chol_plan_set_profiling(sf_chol_plan* p, int on) {
    if (!p) return SF_ERR_ARG;
    p->profiling = on != 0;
    return SF_OK;
}

}  // extern "C"
