// The distributed top of a device plan: the segments of the launch list that follow a sum over a group of ranks -- packing a
// segment's regions for the collective and scattering the sums back (seg_copy), the one-call-per-segment form of the C ABI, the
// pieces of the pipelined driver (sf_multi.hip) with the owner-computes prototype -- and gathering a distributed factor into one
// whole plan (sf_plan_import_from).  The launches themselves are enqueued by sf_run_launches (sf_factorize.hip).
#include <sparseframe_hip.h>

#include "sf_plan_internal.h"

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

// the owner-computes prototype (Segment::owner_gi >= 0): this rank is the member of the segment's group that runs the owner's part
static bool segment_is_mine(const sf_chol_plan* p, const Segment& sg) {
    return sg.owner_gi == __builtin_popcount(sg.mask & ((1u << p->rank) - 1u));
}

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
    dst->fs.factor_replaced(true);          // the imported factor counts as factorized
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
        const bool mine = segment_is_mine(p, sg);
        return (mine && sg.lc > sg.l0) ? sf_run_launches(p, sg.l0, sg.lc, false, false, 0) : SF_OK;
    }
    return sf_run_launches(p, sg.l0, sg.l1, false, k + 1 == (sf_long)p->segments.size(), 0);
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
    const bool mine = segment_is_mine(p, sg);
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
    // sf_run_launches publishes them after the first of those, without any it is done here
    if (p->dl.active && sg.lc == sg.l1) HIP_TRY(sf_dl_publish(p, sg.lc + 1));
    return sf_run_launches(p, sg.lc, sg.l1, false, k + 1 == (sf_long)p->segments.size(), 0);
}
int sf_seg_early(const sf_chol_plan* p, sf_long k) { return (p && k >= 0 && k < (sf_long)p->segments.size() && p->segments[k].early) ? 1 : 0; }

extern "C" {

// the group of ranks that sums segment k's block columns (bit r = rank r); 0 for a plan that is not distributed
uint32_t sf_chol_plan_segment_group(const sf_chol_plan* p, sf_long k) {
    return (p && k >= 0 && k < (sf_long)p->segments.size()) ? p->segments[k].mask : 0u;
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
        const bool mine = segment_is_mine(p, sg);
        if (mine && sg.lc > sg.l0) { const int rc = sf_run_launches(p, sg.l0, sg.lc, false, false, 0); if (rc) return rc; }
        return sf_run_launches(p, sg.lc, sg.l1, false, last, sync);
    }
    return sf_run_launches(p, sg.l0, sg.l1, false, last, sync);
}

}  // extern "C"
