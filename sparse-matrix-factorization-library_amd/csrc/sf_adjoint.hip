// Adjoints on the pattern of A: what a solve, a quadratic form or a log-determinant contributes to the gradient with
// respect to the matrix VALUES, as an array in set_values order (or, mapped, in the caller's own value layout).  Cholesky and LU plans.
//
// With M(V) the matrix sf_*_plan_set_values(V) assembles:
//   adjoint_values      sum_p out[p] dV[p] = alpha sum_c y_c^T M(dV) x_c     for every dV  (Y, X: n x k blocks)
//   logdet_grad_values  sum_p out[p] dV[p] = alpha tr(Sigma M(dV))           for every dV  (Sigma: the arena of sf_*_plan_selinv)
// A position p at (i, j) that the assembly puts at M(i, j) collects Y[i, .] . X[j, .]  (mark ADJ_A), one it puts at M(j, i) collects
// Y[j, .] . X[i, .] (ADJ_B); a Cholesky position off the diagonal and a position of an LU plan whose U aliases L do both.  A position
// the assembly does not read (-1 in the load maps: a superseded duplicate, the L diagonal of an LU plan) has no mark and gets +0.0.
//
//   k_adj_index   : once per plan: the column of every position (a search in the column pointers) and its marks from the load maps
//   k_adj_values  : thread = position.  The operands are read where the caller has them: column-major, row r(i) and r(j) of column c,
//                   r the stored ordering with SF_DEV_PERM_IN -- no staged copy of the blocks, see DESIGN 8r for the choice.  One
//                   accumulator, ascending c, fma, A before B: the bits of out[p] are a function of (p, k) and the operands alone.
//   k_adj_logdet  : thread = position: the arena through the load maps (they address Sigma as they address the factor)
//   k_adj_scatter : thread = source entry of the value map: the unmapped results of the positions that name it, summed in ascending
//                   position (L's before U's) from +0.0.  No floating-point atomic anywhere, no kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "sf_plan_internal.h"

namespace sf {

__global__ void __launch_bounds__(256)
k_adj_index(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, int32_t n, int64_t count, int side,
            const int64_t* __restrict__ mapA, const int64_t* __restrict__ mapB, int32_t* __restrict__ col, uint8_t* __restrict__ mark) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= count) return;
    // the last j in [0, n) with ptr[j] <= p (ptr[0] = 0 <= p < count = ptr[n]; empty columns are stepped over)
    int32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (ptr[mid] <= p) lo = mid; else hi = mid;
    }
    const int32_t j = lo, i = idx[p];
    const bool a = mapA[p] >= 0;
    uint8_t m = 0;
    switch (side) {
        case ADJ_SIDE_CHOL: m = a ? (i != j ? (ADJ_A | ADJ_B) : ADJ_A) : 0; break;
        case ADJ_SIDE_LU_L: m = a ? ADJ_A : 0; break;
        case ADJ_SIDE_LU_ALIAS: m = (a ? ADJ_A : 0) | (mapB[p] >= 0 ? (i != j ? ADJ_B : ADJ_A) : 0); break;
        default: m = a ? ADJ_B : 0; break;
    }
    col[p] = j;
    mark[p] = m;
}

template <bool PERM>
__global__ void __launch_bounds__(256)
k_adj_values(const int32_t* __restrict__ idx, const int32_t* __restrict__ col, const uint8_t* __restrict__ mark, int64_t count,
             const int32_t* __restrict__ perm, int k, const double* __restrict__ Y, int64_t ldy, const double* __restrict__ X, int64_t ldx,
             double alpha, double* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= count) return;
    const uint8_t m = mark[p];
    if (m == 0 || k <= 0) {
        out[p] = 0.0;
        return;
    }
    int64_t ri = idx[p], rj = col[p];
    if (PERM) {
        ri = perm[ri];
        rj = perm[rj];
    }
    const double* __restrict__ yi = Y + ri;
    const double* __restrict__ yj = Y + rj;
    const double* __restrict__ xi = X + ri;
    const double* __restrict__ xj = X + rj;
    double acc = 0.0;
    if (m == (ADJ_A | ADJ_B)) {
#pragma unroll 4
        for (int c = 0; c < k; ++c) {
            acc = __builtin_fma(yi[(int64_t)c * ldy], xj[(int64_t)c * ldx], acc);
            acc = __builtin_fma(yj[(int64_t)c * ldy], xi[(int64_t)c * ldx], acc);
        }
    } else if (m == ADJ_A) {
#pragma unroll 4
        for (int c = 0; c < k; ++c) acc = __builtin_fma(yi[(int64_t)c * ldy], xj[(int64_t)c * ldx], acc);
    } else {
#pragma unroll 4
        for (int c = 0; c < k; ++c) acc = __builtin_fma(yj[(int64_t)c * ldy], xi[(int64_t)c * ldx], acc);
    }
    out[p] = alpha * acc;
}

__global__ void __launch_bounds__(256)
k_adj_logdet(const int64_t* __restrict__ mapA, int64_t shiftA, const int64_t* __restrict__ mapB, int64_t shiftB,
             const uint8_t* __restrict__ mark, int twice, int64_t count, const double* __restrict__ S, double alpha, double* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= count) return;
    const int64_t qa = mapA[p], qb = mapB ? mapB[p] : -1;
    double v = 0.0;
    if (qa >= 0) {
        v = S[qa + shiftA];
        if (twice && mark[p] == (ADJ_A | ADJ_B)) v *= 2.0;
        if (qb >= 0) v += S[qb + shiftB];
    } else if (qb >= 0) {
        v = S[qb + shiftB];
    }
    out[p] = (qa >= 0 || qb >= 0) ? alpha * v : 0.0;
}

__global__ void __launch_bounds__(256)
k_adj_scatter(const int64_t* __restrict__ sptr, const int64_t* __restrict__ list, int64_t nsrc, const double* __restrict__ tmp,
              double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= nsrc) return;
    double acc = 0.0;
    for (int64_t q = sptr[s]; q < sptr[s + 1]; ++q) acc += tmp[list[q]];
    out[s] = acc;
}

static inline dim3 adj_grid(int64_t count) { return dim3((unsigned)((count + 255) / 256)); }

void launch_adj_index(const int64_t* ptr, const int32_t* idx, int32_t n, int64_t count, int side, const int64_t* mapA, const int64_t* mapB,
                      int32_t* col, uint8_t* mark, hipStream_t st) {
    if (count <= 0 || n <= 0) return;
    hipLaunchKernelGGL(k_adj_index, adj_grid(count), dim3(256), 0, st, ptr, idx, n, count, side, mapA, mapB, col, mark);
}

void launch_adj_values(const int32_t* idx, const int32_t* col, const uint8_t* mark, int64_t count, const int32_t* perm, int k, const double* Y,
                       int64_t ldy, const double* X, int64_t ldx, double alpha, double* out, hipStream_t st) {
    if (count <= 0) return;
    if (perm)
        hipLaunchKernelGGL(k_adj_values<true>, adj_grid(count), dim3(256), 0, st, idx, col, mark, count, perm, k, Y, ldy, X, ldx, alpha, out);
    else
        hipLaunchKernelGGL(k_adj_values<false>, adj_grid(count), dim3(256), 0, st, idx, col, mark, count, perm, k, Y, ldy, X, ldx, alpha, out);
}

void launch_adj_logdet(const int64_t* mapA, int64_t shiftA, const int64_t* mapB, int64_t shiftB, const uint8_t* mark, int twice, int64_t count,
                       const double* S, double alpha, double* out, hipStream_t st) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_adj_logdet, adj_grid(count), dim3(256), 0, st, mapA, shiftA, mapB, shiftB, mark, twice, count, S, alpha, out);
}

void launch_adj_scatter(const int64_t* sptr, const int64_t* list, int64_t nsrc, const double* tmp, double* out, hipStream_t st) {
    if (nsrc <= 0) return;
    hipLaunchKernelGGL(k_adj_scatter, adj_grid(nsrc), dim3(256), 0, st, sptr, list, nsrc, tmp, out);
}

}  // namespace sf

// ===========================================================================================================================
// host side
// ===========================================================================================================================
namespace {

// the plans the entry points accept: of the right kind, whole and resident (what sf_*_plan_solve_device accepts), with load maps
bool adj_accepts(const sf_chol_plan* p, bool lu) {
    if (!p || p->lu != lu || !sf_plan_whole_resident(p)) return false;
    return p->d_loadmapL && (!lu || p->d_loadmapU);
}

bool own_u(const sf_chol_plan* p) { return p->lu && !p->u_alias; }
size_t adj_nl(const sf_chol_plan* p) { return (size_t)std::max<int64_t>(p->nnz, 1); }
int64_t adj_nu(const sf_chol_plan* p) { return own_u(p) ? p->unz : 0; }

// the column and the marks of every position (first call)
int adj_index(sf_chol_plan* p) {
    if (p->d_adj_col) return SF_OK;
    const size_t nl = adj_nl(p), total = nl + (size_t)adj_nu(p);
    sf::DevMem<int32_t> col;
    sf::DevMem<uint8_t> mark;
    if (int rc = col.alloc(total)) return rc;
    if (int rc = mark.alloc(total)) return rc;
    const int side = !p->lu ? sf::ADJ_SIDE_CHOL : p->u_alias ? sf::ADJ_SIDE_LU_ALIAS : sf::ADJ_SIDE_LU_L;
    sf::launch_adj_index(p->d_Lp, p->d_Li, (int32_t)p->n, p->nnz, side, p->d_loadmapL, p->lu ? p->d_loadmapU.get() : nullptr, col, mark, p->stream);
    if (own_u(p))
        sf::launch_adj_index(p->d_Up, p->d_Ui, (int32_t)p->n, p->unz, sf::ADJ_SIDE_LU_U, p->d_loadmapU, nullptr, col + nl, mark + nl, p->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return SF_ERR_HIP;
    p->d_adj_col = std::move(col);
    p->d_adj_mark = std::move(mark);
    p->bytes_adjoint += total * (sizeof(int32_t) + sizeof(uint8_t));
    return SF_OK;
}

// room for the unmapped result of a mapped call
int adj_tmp(sf_chol_plan* p) {
    if (p->d_adj_tmp) return SF_OK;
    const size_t total = adj_nl(p) + (size_t)adj_nu(p);
    if (int rc = p->d_adj_tmp.alloc(total)) return rc;
    p->bytes_adjoint += total * sizeof(double);
    return SF_OK;
}

// The value map by source entry: for every s the positions q with map[q] == s, ascending (q = p for L's positions, nl + p for U's) --
// a counting sort of the stored map on the host, once per sf_*_plan_set_value_map.
int adj_sources(sf_chol_plan* p) {
    if (p->d_adj_src && p->adj_vmap_gen == p->vmap_gen) return SF_OK;
    const size_t nl = adj_nl(p);
    const int64_t nu = adj_nu(p), nsrc = p->vmap_nsrc;
    std::vector<int64_t> map(nl + (size_t)nu, -1);
    if (p->nnz > 0) HIP_TRY(hipMemcpy(map.data(), p->d_vmap, (size_t)p->nnz * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (nu > 0) HIP_TRY(hipMemcpy(map.data() + nl, p->d_vmap + nl, (size_t)nu * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> h((size_t)nsrc + 1, 0);
    int64_t named = 0;
    for (int64_t m : map)
        if (m >= 0) { ++h[(size_t)m + 1]; ++named; }
    for (int64_t s = 0; s < nsrc; ++s) h[(size_t)s + 1] += h[(size_t)s];
    std::vector<int64_t> next(h.begin(), h.end() - 1);
    h.resize((size_t)nsrc + 1 + (size_t)std::max<int64_t>(named, 1), 0);
    for (size_t q = 0; q < map.size(); ++q)
        if (map[q] >= 0) h[(size_t)nsrc + 1 + (size_t)next[(size_t)map[q]]++] = (int64_t)q;
    sf::DevMem<int64_t> src;
    if (int rc = src.alloc(h.size())) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));       // (nothing of an earlier call still reads the old lists)
    HIP_TRY(hipMemcpy(src, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (p->d_adj_src) p->bytes_adjoint -= ((size_t)p->adj_src_entries) * sizeof(int64_t);
    p->d_adj_src = std::move(src);
    p->adj_src_entries = (int64_t)h.size();
    p->bytes_adjoint += h.size() * sizeof(int64_t);
    p->adj_vmap_gen = p->vmap_gen;
    return SF_OK;
}

// what one call computes: adjoint_values of (Y, X) or (k < 0) logdet_grad_values
struct AdjJob {
    int k;
    const int32_t* perm;
    const double *Y, *X;
    int64_t ldy, ldx;
    double alpha;
};

// the kernels of one call, results in device memory: outL (nnz), outU (unz, plans with their own U) or, mapped, outL (nsrc)
int adj_run(sf_chol_plan* p, const AdjJob& j, bool mapped, double* outL, double* outU) {
    if (int rc = adj_index(p)) return rc;
    if (mapped) {
        if (int rc = adj_tmp(p)) return rc;
        if (int rc = adj_sources(p)) return rc;
    }
    const size_t nl = adj_nl(p);
    const int64_t nu = adj_nu(p);
    double* tL = mapped ? p->d_adj_tmp.get() : outL;
    double* tU = mapped ? p->d_adj_tmp + nl : outU;
    hipStream_t st = p->stream;
    SfStretch t{p};
    if (int rc = t.open()) return rc;
    if (j.k >= 0) {
        sf::launch_adj_values(p->d_Li, p->d_adj_col, p->d_adj_mark, p->nnz, j.perm, j.k, j.Y, j.ldy, j.X, j.ldx, j.alpha, tL, st);
        if (nu > 0) sf::launch_adj_values(p->d_Ui, p->d_adj_col + nl, p->d_adj_mark + nl, nu, j.perm, j.k, j.Y, j.ldy, j.X, j.ldx, j.alpha, tU, st);
    } else if (!p->lu) {
        sf::launch_adj_logdet(p->d_loadmapL, 0, nullptr, 0, p->d_adj_mark, 1, p->nnz, p->d_sel, j.alpha, tL, st);
    } else {
        // an entry of L meets Sigma(j, i) in SU at its own offset, an entry of U (its map carries the xC of the U^T panels) Sigma(c, j) in
        // SL: the pairing of sf_lu_plan_selinv_trace
        sf::launch_adj_logdet(p->d_loadmapL, p->xC, p->u_alias ? p->d_loadmapU.get() : nullptr, -p->xC, p->d_adj_mark, 0, p->nnz, p->d_sel, j.alpha,
                              tL, st);
        if (nu > 0) sf::launch_adj_logdet(p->d_loadmapU, -p->xC, nullptr, 0, p->d_adj_mark + nl, 0, nu, p->d_sel, j.alpha, tU, st);
    }
    if (mapped) sf::launch_adj_scatter(p->d_adj_src, p->d_adj_src + (p->vmap_nsrc + 1), p->vmap_nsrc, p->d_adj_tmp, outL, st);
    if (int rc = t.mark()) return rc;
    if (int rc = t.close(false)) return rc;
    p->last_adjoint_ms = t.total_ms;
    return SF_OK;
}

// a host block of k columns of n doubles, ld apart, into fresh device memory (leading dimension max(n, 1))
int adj_upload(const double* B, int64_t n, int64_t ld, int k, sf::DevMem<double>& d) {
    if (int rc = d.alloc((size_t)std::max<int64_t>(n * k, 1))) return rc;
    if (n <= 0 || k <= 0) return SF_OK;
    const size_t col = (size_t)n * sizeof(double);
    if (hipMemcpy2D(d, col, B, (size_t)ld * sizeof(double), col, (size_t)k, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        d.reset();
        return SF_ERR_HIP;
    }
    return SF_OK;
}

// k >= 0: adjoint_values; k == -1: logdet_grad_values (Y, X, ldy, ldx unused)
int adj_entry(sf_chol_plan* p, bool lu, bool dev, int flags, sf_long k, const double* Y, sf_long ldy, const double* X, sf_long ldx, double alpha,
              double* outL, double* outU) {
    const bool logdet = k == -1;
    if (!p || p->lu != lu || k < -1) return SF_ERR_ARG;
    if (flags & ~(SF_ADJ_MAPPED | ((dev && !logdet) ? SF_DEV_PERM_IN : 0))) return SF_ERR_ARG;
    const bool mapped = (flags & SF_ADJ_MAPPED) != 0, perm = (flags & SF_DEV_PERM_IN) != 0;
    const bool need_u = own_u(p) && !mapped;
    const int64_t n = p->n, count_l = mapped ? p->vmap_nsrc : p->nnz, count_u = need_u ? p->unz : 0;
    if (!logdet) {
        const sf_long ldmin = std::max<sf_long>(n, 1);
        if (ldy < ldmin || ldx < ldmin) return SF_ERR_ARG;
        if ((!Y || !X) && k > 0 && n > 0) return SF_ERR_ARG;
        if (k > (sf_long)INT32_MAX) return SF_ERR_ARG;
    }
    if ((!outL && count_l > 0) || (need_u && !outU && count_u > 0) || (!need_u && outU)) return SF_ERR_ARG;
    if (!adj_accepts(p, lu) || (mapped && !p->d_vmap) || (perm && !p->d_perm)) return SF_ERR_ARG;
    if (logdet && (!p->d_sel || !p->fs.selinv_matches())) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (count_l + count_u <= 0) return SF_OK;
    AdjJob j{logdet ? -1 : (int)k, perm ? p->d_perm.get() : nullptr, Y, X, ldy, ldx, alpha};
    if (dev) {
        const size_t sy = logdet ? 0 : sf_block_span(n, k, ldy), sx = logdet ? 0 : sf_block_span(n, k, ldx);
        if ((sy && !sf_device_ptr_ok(p, Y, sy)) || (sx && !sf_device_ptr_ok(p, X, sx))) return SF_ERR_ARG;
        double* outs[2] = {outL, need_u ? outU : nullptr};
        const int64_t counts[2] = {count_l, count_u};
        for (int s = 0; s < 2; ++s) {
            if (counts[s] <= 0) continue;
            if (!sf_device_ptr_ok(p, outs[s], (size_t)counts[s])) return SF_ERR_ARG;
            if ((sy && sf_blocks_overlap(outs[s], (size_t)counts[s], Y, sy)) || (sx && sf_blocks_overlap(outs[s], (size_t)counts[s], X, sx)))
                return SF_ERR_ARG;
        }
        if (count_l > 0 && count_u > 0 && sf_blocks_overlap(outL, (size_t)count_l, outU, (size_t)count_u)) return SF_ERR_ARG;
        return adj_run(p, j, mapped, outL, count_u > 0 ? outU : nullptr);
    }
    sf::DevMem<double> dY, dX, dO;
    if (!logdet) {
        if (int rc = adj_upload(Y, n, ldy, (int)k, dY)) return rc;
        if (int rc = adj_upload(X, n, ldx, (int)k, dX)) return rc;
        j.Y = dY;
        j.X = dX;
        j.ldy = j.ldx = std::max<int64_t>(n, 1);
    }
    const size_t nl = (size_t)std::max<int64_t>(count_l, 1);
    if (int rc = dO.alloc(nl + (size_t)count_u)) return rc;
    if (int rc = adj_run(p, j, mapped, dO, count_u > 0 ? dO + nl : nullptr)) return rc;
    if (count_l > 0) HIP_TRY(hipMemcpy(outL, dO, (size_t)count_l * sizeof(double), hipMemcpyDeviceToHost));
    if (count_u > 0) HIP_TRY(hipMemcpy(outU, dO + nl, (size_t)count_u * sizeof(double), hipMemcpyDeviceToHost));
    return SF_OK;
}

}  // namespace

extern "C" {

int sf_chol_plan_adjoint_values(sf_chol_plan* p, sf_long k, const sf_float* Y, sf_long ldy, const sf_float* X, sf_long ldx, double alpha, int flags,
                                sf_float* out) {
    return k < 0 ? SF_ERR_ARG : adj_entry(p, false, false, flags, k, Y, ldy, X, ldx, alpha, out, nullptr);
}
int sf_chol_plan_adjoint_values_device(sf_chol_plan* p, int flags, sf_long k, const sf_float* dY, sf_long ldy, const sf_float* dX, sf_long ldx,
                                       double alpha, sf_float* d_out) {
    return k < 0 ? SF_ERR_ARG : adj_entry(p, false, true, flags, k, dY, ldy, dX, ldx, alpha, d_out, nullptr);
}
int sf_lu_plan_adjoint_values(sf_lu_plan* p, sf_long k, const sf_float* Y, sf_long ldy, const sf_float* X, sf_long ldx, double alpha, int flags,
                              sf_float* outL, sf_float* outU) {
    return k < 0 ? SF_ERR_ARG : adj_entry(p, true, false, flags, k, Y, ldy, X, ldx, alpha, outL, outU);
}
int sf_lu_plan_adjoint_values_device(sf_lu_plan* p, int flags, sf_long k, const sf_float* dY, sf_long ldy, const sf_float* dX, sf_long ldx,
                                     double alpha, sf_float* d_outL, sf_float* d_outU) {
    return k < 0 ? SF_ERR_ARG : adj_entry(p, true, true, flags, k, dY, ldy, dX, ldx, alpha, d_outL, d_outU);
}

int sf_chol_plan_logdet_grad_values(sf_chol_plan* p, double alpha, int flags, sf_float* out) {
    return adj_entry(p, false, false, flags, -1, nullptr, 0, nullptr, 0, alpha, out, nullptr);
}
int sf_chol_plan_logdet_grad_values_device(sf_chol_plan* p, double alpha, int flags, sf_float* d_out) {
    return adj_entry(p, false, true, flags, -1, nullptr, 0, nullptr, 0, alpha, d_out, nullptr);
}
int sf_lu_plan_logdet_grad_values(sf_lu_plan* p, double alpha, int flags, sf_float* outL, sf_float* outU) {
    return adj_entry(p, true, false, flags, -1, nullptr, 0, nullptr, 0, alpha, outL, outU);
}
int sf_lu_plan_logdet_grad_values_device(sf_lu_plan* p, double alpha, int flags, sf_float* d_outL, sf_float* d_outU) {
    return adj_entry(p, true, true, flags, -1, nullptr, 0, nullptr, 0, alpha, d_outL, d_outU);
}

}  // extern "C"
