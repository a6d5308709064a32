// Rank-k update and downdate of the resident Cholesky factor: A' = A +- W W^T with the pattern of L unchanged.
//
// W lives on the device as a row-major n x UPD_W block.  For every supernode of the path (sf_updown_path.h), ascending, and every
// 64-column block of it, two launches on the plan's stream: k_updown_diag rotates the diagonal block against its rows of W and
// leaves the pairs (c, s); k_updown_rows applies them to every panel row below the block and to the rows of W those panel rows name.
// No kernel waits for another workgroup: the order of the launches is the stream's.
//
// One rotation, sigma = sign, d = L_jj, w = W_jt:  r = sqrt(d^2 + sigma w^2) (downdate: sqrt((d - w)(d + w))), c = r / d, s = w / d,
// L_jj <- r, and for the rows i below:  L_ij <- (L_ij + sigma s W_it) (1 / c),  W_it <- c W_it - s L_ij (the new L_ij).
// Square root and divisions are the IEEE ones (correctly rounded), not rsqrt_full / rcp_full: a column of W that is zero on a block
// must give c = 1 and s = 0 EXACTLY -- sqrt(fl(d d)) = d holds for the correctly rounded root only -- because the kernels do not
// branch around such columns, and a chunk narrower than its kernel's width rotates its zero columns too.
#include <sparseframe_hip.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sf_plan_internal.h"
#include "sf_updown_path.h"
#include "sf_panel.h"

namespace sf {

namespace {

constexpr int UPD_ROWS_WG = 256;

__global__ void k_updown_scatter(const int64_t* __restrict__ dest, const double* __restrict__ val, int64_t count, double* __restrict__ W) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < count) W[dest[q]] = val[q];
}

// lane = row of the block, its K values of W in registers.  The lower triangle of the block waits in LDS (column-major) and column j
// passes through one register per lane: column j is rotated at step j only, so nothing goes back to LDS.  (The block in 64
// registers per lane, as the factorization's one-wave kernels keep it, needs the 64 x K rotations unrolled in full; with the IEEE
// square root and divisions inlined in each, the compiler gives that up from K = 4 on and puts the block into scratch.)  The
// rotations' parameters are wave-uniform: every lane computes them from the same d and w.
template <int K, bool DOWN>
__global__ __launch_bounds__(64) void k_updown_diag(double* __restrict__ D, int64_t ld, int b, double* __restrict__ W, double* __restrict__ rot,
                                                     int* __restrict__ info) {
    __shared__ double blk[UPD_B * UPD_B];
    const int lane = threadIdx.x;
    const bool in = lane < b;
    for (int j = 0; j < b; ++j)
        if (in && j <= lane) blk[j * UPD_B + lane] = D[(int64_t)j * ld + lane];
    double w[K];
#pragma unroll
    for (int t = 0; t < K; ++t) w[t] = in ? W[(int64_t)lane * UPD_W + t] : 0.0;
    bool bad = *info != 0;
    __syncthreads();
    for (int j0 = 0; j0 < b; ++j0) {
        const int j = __builtin_amdgcn_readfirstlane(j0);
        double d = blk[j * UPD_B + j];
        double x = (in && lane > j) ? blk[j * UPD_B + lane] : 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const double wj = readlane_dyn_f64(w[t], j);
            const double r2 = DOWN ? (d - wj) * (d + wj) : d * d + wj * wj;
            bad = bad || !(r2 > 0.0);           // (NaN takes this branch too)
            const double r = bad ? d : sqrt(r2);
            const double c = bad ? 1.0 : r / d;
            const double s = bad ? 0.0 : wj / d;
            const double ci = 1.0 / c;
            if (lane > j) {
                x = (DOWN ? x - s * w[t] : x + s * w[t]) * ci;
                w[t] = c * w[t] - s * x;
            }
            d = r;
            if (lane == 0) {
                rot[2 * (j * UPD_W + t)] = c;
                rot[2 * (j * UPD_W + t) + 1] = s;
            }
        }
        if (in && lane >= j) D[(int64_t)j * ld + lane] = lane == j ? d : x;
    }
    if (in) {
#pragma unroll
        for (int t = 0; t < UPD_W; ++t) W[(int64_t)lane * UPD_W + t] = 0.0;
    }
    if (bad && lane == 0) *info = 1;
}


// lane = panel row.  The block's pairs (with 1 / c) sit in LDS, where every lane reads the same word; the row's K values of W stay in
// registers, column j of the panel passes through one.
template <int K, bool DOWN>
__global__ __launch_bounds__(UPD_ROWS_WG) void k_updown_rows(double* __restrict__ P, int64_t ld, int b, int64_t nrows,
                                                              const int32_t* __restrict__ rows, double* __restrict__ W,
                                                              const double* __restrict__ rot) {
    __shared__ double sh[UPD_B * K * 3];
    for (int q = threadIdx.x; q < b * K; q += UPD_ROWS_WG) {
        const int j = q / K, t = q % K;
        const double c = rot[2 * (j * UPD_W + t)];
        sh[3 * q] = c;
        sh[3 * q + 1] = rot[2 * (j * UPD_W + t) + 1];
        sh[3 * q + 2] = 1.0 / c;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * UPD_ROWS_WG + threadIdx.x;
    if (i >= nrows) return;
    double* wrow = W + (int64_t)rows[i] * UPD_W;
    double w[K];
#pragma unroll
    for (int t = 0; t < K; ++t) w[t] = wrow[t];
    double* p = P + i;
#pragma unroll 4
    for (int j = 0; j < b; ++j) {
        double x = p[(int64_t)j * ld];
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const double c = sh[3 * (j * K + t)], s = sh[3 * (j * K + t) + 1], ci = sh[3 * (j * K + t) + 2];
            x = (DOWN ? x - s * w[t] : x + s * w[t]) * ci;
            w[t] = c * w[t] - s * x;
        }
        p[(int64_t)j * ld] = x;
    }
#pragma unroll
    for (int t = 0; t < K; ++t) wrow[t] = w[t];
}

template <int K>
void diag_k(double* D, int64_t ld, int b, int sign, double* W, double* rot, int* info, hipStream_t st) {
    if (sign < 0) hipLaunchKernelGGL((k_updown_diag<K, true>), dim3(1), dim3(64), 0, st, D, ld, b, W, rot, info);
    else hipLaunchKernelGGL((k_updown_diag<K, false>), dim3(1), dim3(64), 0, st, D, ld, b, W, rot, info);
}
template <int K>
void rows_k(double* P, int64_t ld, int b, int64_t nrows, const int32_t* rows, int sign, double* W, const double* rot, hipStream_t st) {
    const dim3 g((unsigned)((nrows + UPD_ROWS_WG - 1) / UPD_ROWS_WG));
    if (sign < 0) hipLaunchKernelGGL((k_updown_rows<K, true>), g, dim3(UPD_ROWS_WG), 0, st, P, ld, b, nrows, rows, W, rot);
    else hipLaunchKernelGGL((k_updown_rows<K, false>), g, dim3(UPD_ROWS_WG), 0, st, P, ld, b, nrows, rows, W, rot);
}

}  // namespace

void launch_updown_scatter(const int64_t* dest, const double* val, int64_t count, double* W, hipStream_t st) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_updown_scatter, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, dest, val, count, W);
}

void launch_updown_diag(double* D, int64_t ld, int b, int kw, int sign, double* W, int64_t col0, double* rot, int* info, hipStream_t st) {
    if (b <= 0 || b > UPD_B) return;
    double* w = W + col0 * UPD_W;
    switch (kw) {
        case 1: diag_k<1>(D, ld, b, sign, w, rot, info, st); break;
        case 2: diag_k<2>(D, ld, b, sign, w, rot, info, st); break;
        case 4: diag_k<4>(D, ld, b, sign, w, rot, info, st); break;
        case 8: diag_k<8>(D, ld, b, sign, w, rot, info, st); break;
        default: diag_k<16>(D, ld, b, sign, w, rot, info, st); break;
    }
}

void launch_updown_rows(double* P, int64_t ld, int b, int64_t nrows, const int32_t* rows, int kw, int sign, double* W, const double* rot,
                        hipStream_t st) {
    if (b <= 0 || b > UPD_B || nrows <= 0) return;
    switch (kw) {
        case 1: rows_k<1>(P, ld, b, nrows, rows, sign, W, rot, st); break;
        case 2: rows_k<2>(P, ld, b, nrows, rows, sign, W, rot, st); break;
        case 4: rows_k<4>(P, ld, b, nrows, rows, sign, W, rot, st); break;
        case 8: rows_k<8>(P, ld, b, nrows, rows, sign, W, rot, st); break;
        default: rows_k<16>(P, ld, b, nrows, rows, sign, W, rot, st); break;
    }
}

}  // namespace sf

// ---------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------
sf::UpdownStruct sf_updown_struct(const sf_chol_plan* p) {
    sf::UpdownStruct S;
    S.n = p->n;
    S.nsuper = p->nsuper;
    S.Super = p->h_Super.data();
    S.Lsip = p->h_Lsip.data();
    S.Lsi = p->h_Lsi.data();
    return S;
}

// the inverse of the ordering of sf_chol_plan_set_ordering: iperm[old] = new
int sf_updown_inverse_ordering(const sf_chol_plan* p, std::vector<int32_t>& iperm) {
    std::vector<int32_t> perm((size_t)std::max<int64_t>(p->n, 1));
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpy(perm.data(), p->d_perm, (size_t)p->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    iperm.assign(perm.size(), 0);
    for (int64_t i = 0; i < p->n; ++i) iperm[(size_t)perm[(size_t)i]] = (int32_t)i;
    return SF_OK;
}

namespace {

int kernel_width(int cw) {
    int kw = 1;
    while (kw < cw) kw *= 2;
    return kw;
}

}  // namespace

// ---- what the row modifications share with the update (sf_plan_internal.h) ----
int sf_updown_accepts(sf_chol_plan* p, int flags) {
    if (!p || p->lu) return SF_ERR_ARG;
    if (flags & ~SF_DEV_PERM_IN) return SF_ERR_ARG;
    if (!sf_plan_whole_resident(p)) return SF_ERR_ARG;
    if ((flags & SF_DEV_PERM_IN) && !p->d_perm) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (p->fs.broken() || !sf_factor_usable(p)) return SF_ERR_ARG;
    return SF_OK;
}

// the block of W, the pairs of one diagonal block, the info word
constexpr size_t UPD_ROT = 2 * (size_t)sf::UPD_B * sf::UPD_W;
int sf_updown_block(sf_chol_plan* p) {
    if (p->d_upd) return SF_OK;
    const size_t count = (size_t)p->n * sf::UPD_W + UPD_ROT + 1;
    if (int rc = p->d_upd.alloc(count)) return rc;
    p->bytes_update = count * sizeof(double);
    return SF_OK;
}

SfUpdownBlock sf_updown_parts(sf_chol_plan* p) {
    SfUpdownBlock B;
    B.W = p->d_upd;
    B.rot = B.W + (size_t)p->n * sf::UPD_W;
    B.info = (int*)(B.rot + UPD_ROT);
    return B;
}

int sf_updown_clear_w(sf_chol_plan* p) {
    if (p->upd_w_dirty) HIP_TRY(hipMemsetAsync(p->d_upd, 0, (size_t)p->n * sf::UPD_W * sizeof(double), p->stream));
    p->upd_w_dirty = true;
    return SF_OK;
}

int64_t sf_updown_rotate(sf_chol_plan* p, const std::vector<int64_t>& supers, int sign, int kw) {
    hipStream_t st = p->stream;
    const SfUpdownBlock B = sf_updown_parts(p);
    int64_t launches = 0;
    for (int64_t s : supers) {
        const int64_t c0 = p->h_Super[s], nscol = p->h_Super[s + 1] - c0, nsrow = p->h_Lsip[s + 1] - p->h_Lsip[s];
        double* panel = p->d_Lsx + p->h_Lsxp[s];
        for (int64_t j0 = 0; j0 < nscol; j0 += sf::UPD_B) {
            const int b = (int)std::min<int64_t>(sf::UPD_B, nscol - j0);
            sf::launch_updown_diag(panel + j0 * nsrow + j0, nsrow, b, kw, sign, B.W, c0 + j0, B.rot, B.info, st);
            const int64_t below = nsrow - (j0 + b);
            sf::launch_updown_rows(panel + j0 * nsrow + j0 + b, nsrow, b, below, p->d_Lsi + p->h_Lsip[s] + j0 + b, kw, sign, B.W, B.rot, st);
            launches += below > 0 ? 2 : 1;
        }
    }
    return launches;
}

int sf_updown_collect(sf_chol_plan* p, int* h_info) {
    hipStream_t st = p->stream;
    HIP_TRY(hipEventRecord(p->ev_s1, st));
    HIP_TRY(hipMemcpyAsync(h_info, sf_updown_parts(p).info, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SF_OK;
}

int sf_updown_commit(sf_chol_plan* p, int rrc, int h_info, const std::vector<int64_t>& supers, int64_t launches) {
    int64_t path_cols = 0;
    for (int64_t s : supers) path_cols += p->h_Super[s + 1] - p->h_Super[s];
    float ms = 0;
    if (rrc == SF_OK && elapsed_ms(&ms, p->ev_s0, p->ev_s1)) p->last_updown_ms = ms;
    p->upd_path_supers = (int64_t)supers.size();
    p->upd_path_cols = path_cols;
    p->upd_launches = launches;
    const bool ok = rrc == SF_OK && !h_info;
    p->fs.factor_replaced(ok);      // as for an import: the updated factor counts as factorized; half rotated: no factor
    if (ok) return SF_OK;
    p->upd_w_dirty = true;
    return rrc != SF_OK ? rrc : SF_ERR_NOT_POSDEF;
}

namespace {

int update_run(sf_chol_plan* p, int sign, sf_long k, const sf_long* Wp, const sf_long* Wi, const sf_float* Wx, bool wx_dev, int flags) {
    if (!p || (sign != SF_UPDATE && sign != SF_DOWNDATE) || k < 0 || !Wp) return SF_ERR_ARG;
    if (int rc = sf_updown_accepts(p, flags)) return rc;
    std::vector<int32_t> iperm;
    if (flags & SF_DEV_PERM_IN)
        if (int rc = sf_updown_inverse_ordering(p, iperm)) return rc;
    std::vector<int64_t> supers;
    std::vector<int32_t> rows;
    int64_t bad = -1;
    const int prc = sf::updown_path(sf_updown_struct(p), k, Wp, Wi, iperm.empty() ? nullptr : iperm.data(), supers, &bad, &rows);
    if (prc == sf::UPDOWN_INADMISSIBLE) p->upd_bad_column = bad;      // (the stat that names it; nothing else of the plan changes)
    if (prc != sf::UPDOWN_OK) return SF_ERR_ARG;
    const int64_t nz = Wp[k] - Wp[0];
    if (nz > 0 && !Wx) return SF_ERR_ARG;
    if (wx_dev && nz > 0 && !sf_device_ptr_ok(p, Wx + Wp[0], (size_t)nz)) return SF_ERR_ARG;
    if (k == 0) return SF_OK;
    if (int rc = sf_updown_block(p)) return rc;

    hipStream_t st = p->stream;
    const SfUpdownBlock B = sf_updown_parts(p);
    // where every value goes in the block of its chunk, and the values themselves
    std::vector<int64_t> dest((size_t)std::max<int64_t>(nz, 1));
    for (sf_long t = 0; t < k; ++t)
        for (sf_long q = Wp[t]; q < Wp[t + 1]; ++q) dest[(size_t)(q - Wp[0])] = (int64_t)rows[(size_t)(q - Wp[0])] * sf::UPD_W + t % sf::UPD_W;
    sf::DevMem<int64_t> d_dest;
    sf::DevMem<double> d_val;
    if (int rc = d_dest.alloc(dest.size())) return rc;
    HIP_TRY(hipMemcpyAsync(d_dest, dest.data(), dest.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const double* val = Wx ? Wx + Wp[0] : nullptr;
    if (!wx_dev && nz > 0) {
        if (int rc = d_val.alloc((size_t)nz)) return rc;
        HIP_TRY(hipMemcpyAsync(d_val, val, (size_t)nz * sizeof(double), hipMemcpyHostToDevice, st));
        val = d_val;
    }
    HIP_TRY(hipMemsetAsync(B.info, 0, sizeof(double), st));

    int64_t launches = 0;
    int h_info = 0;
    // From the first launch on the factor may be partly rotated: whatever goes wrong in here, the plan no longer holds a factor.
    auto rotate = [&]() -> int {
        HIP_TRY(hipEventRecord(p->ev_s0, st));
        for (sf_long t0 = 0; t0 < k; t0 += sf::UPD_W) {
            const int cw = (int)std::min<sf_long>(sf::UPD_W, k - t0), kw = kernel_width(cw);
            // A finished chunk leaves the block zero again: the diagonal launches zero the rows of their columns, and every row a
            // row launch writes is a column of an ancestor on the path.  Only a fresh block, or one an error left behind, is cleared.
            if (int rc = sf_updown_clear_w(p)) return rc;
            sf::launch_updown_scatter(d_dest + (Wp[t0] - Wp[0]), val + (Wp[t0] - Wp[0]), Wp[t0 + cw] - Wp[t0], B.W, st);
            // (a chunk only touches the chains of its own columns, but a supernode off them sees zero rows of W: identities)
            launches += sf_updown_rotate(p, supers, sign, kw);
            HIP_TRY(hipGetLastError());
            p->upd_w_dirty = false;
        }
        return sf_updown_collect(p, &h_info);
    };
    const int rrc = rotate();
    return sf_updown_commit(p, rrc, h_info, supers, launches);
}

}  // namespace

extern "C" {

int sf_chol_plan_update(sf_chol_plan* p, int sign, sf_long k, const sf_long* Wp, const sf_long* Wi, const sf_float* Wx, int flags) {
    return update_run(p, sign, k, Wp, Wi, Wx, false, flags);
}

int sf_chol_plan_update_device(sf_chol_plan* p, int sign, sf_long k, const sf_long* Wp, const sf_long* Wi, const sf_float* dWx, int flags) {
    return update_run(p, sign, k, Wp, Wi, dWx, true, flags);
}

int sf_chol_plan_update_path(const sf_chol_plan* p, sf_long k, const sf_long* Wp, const sf_long* Wi, int flags, sf_long* count,
                             sf_long* supers, sf_long* bad_column) {
    if (count) *count = 0;
    if (bad_column) *bad_column = -1;
    if (!p || p->lu || k < 0 || !Wp || !count) return SF_ERR_ARG;
    if (flags & ~SF_DEV_PERM_IN) return SF_ERR_ARG;
    std::vector<int32_t> iperm;
    if (flags & SF_DEV_PERM_IN) {
        if (p->dry || !p->d_perm) return SF_ERR_ARG;
        if (int rc = sf_updown_inverse_ordering(p, iperm)) return rc;
    }
    std::vector<int64_t> path;
    int64_t bad = -1;
    const int prc = sf::updown_path(sf_updown_struct(p), k, Wp, Wi, iperm.empty() ? nullptr : iperm.data(), path, &bad);
    if (bad_column) *bad_column = bad;
    if (prc != sf::UPDOWN_OK) return SF_ERR_ARG;
    *count = (sf_long)path.size();
    if (supers) std::copy(path.begin(), path.end(), supers);
    return SF_OK;
}

}  // extern "C"
