// Device plan of the supernodal Cholesky / LU numeric factorization, values in and factor out: its release, the values,
// validation, reading the factor back, its fingerprints and the pivoting policy.  The plan is built in sf_plan_build.hip, run
// by sf_factorize.hip (the segments of a distributed top: sf_segments.hip; the overlapped download: sf_download.hip) and
// inspected through sf_plan_query.hip; the solves and everything else that takes columns through the resident factor live in
// files of their own (sf_solve.hip, sf_apply.hip and the entry points' files).
#include <sparseframe_hip.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sf_plan_internal.h"

extern "C" {

int sf_chol_plan_destroy(sf_chol_plan* p) {
    delete p;
    return SF_OK;
}

int sf_chol_plan_set_values(sf_chol_plan* p, const sf_float* Lx) {
    if (!p || p->lu || (!Lx && p->nnz > 0)) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    if (p->nnz > 0) HIP_TRY(hipMemcpyAsync(p->d_Lx, Lx, p->nnz * sizeof(double), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    p->fs.values_changed();
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
    p->fs.values_changed();
    return SF_OK;
}

// The whole of SparseFrame_validate on the device (C:3141-3266, L:3702-3858): b_i = 1 + i/n, the supernodal solve with the
// resident factor, r = A x - b from the plan's copy of the matrix, residual = |r|_inf / (|A|_1 |x|_inf + |b|_inf).  Nothing
// but the scalar comes back (x_host may be NULL).
int sf_chol_plan_validate(sf_chol_plan* p, sf_float* residual, sf_float* x_host) {
    if (!p || !residual) return SF_ERR_ARG;
    if (p->partial || (p->nsuper > 0 && !p->d_solve) || !p->fs.has_values()) return SF_ERR_ARG;
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
    if (!p->fs.hashes_current() || p->h_hash.size() != (size_t)std::max<int64_t>(p->nsuper, 1)) {
        if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
        HIP_TRY(hipSetDevice(p->device));
        const size_t nh = (size_t)std::max<int64_t>(p->nsuper, 1), nb = nh * sizeof(unsigned long long);
        sf::DevMem<unsigned long long> d_h;
        if (d_h.alloc(nh)) return SF_ERR_HIP;
        const int64_t* xp = (p->lu || p->partial) ? p->d_Xp : p->d_Lsxp;
        p->fs.hashes_pending();
        HIP_TRY(hipMemsetAsync(d_h, 0, nb, p->stream));
        sf::launch_factor_hash(p->d_Super, p->d_Lsip, xp, p->d_Lsxp, (int32_t)p->nsuper, p->d_Lsx, p->d_Lsx + p->xC, p->lu ? 1 : 0,
                               p->xsize, d_h, p->stream);
        HIP_TRY(hipGetLastError());
        p->h_hash.assign(nh, 0);
        HIP_TRY(hipMemcpyAsync(p->h_hash.data(), d_h, nb, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        p->fs.hashes_arrived();
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
int sf_lu_plan_set_profiling(sf_lu_plan* p, int on) { return sf_chol_plan_set_profiling(p, on); }
int sf_lu_plan_destroy(sf_lu_plan* p) { return sf_chol_plan_destroy(p); }

}  // extern "C"
