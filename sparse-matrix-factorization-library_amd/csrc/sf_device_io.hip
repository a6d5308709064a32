// Device-pointer solves, orderings and value updates (sf_*_plan_set_ordering, _solve_device, _permute_device, _sample_device,
// _set_values_device, _set_value_map, _set_values_mapped_device).  DESIGN 8g.
//
// The sweeps, their task lists, sync words and tickets are sf_solve.hip's and sf_solve_t.hip's; the generator is sf_sample.hip's.
// What is new here is how a block gets to and from them: straight between the caller's DEVICE memory (column-major, leading
// dimension ld, optionally in the caller's own numbering) and the plan's d_x (one column) or row-major n x SVM_W block d_xm, with
// no staging half and no copy in between.  perm[new] = old, as sf_symbolic_create takes it:
//   load  with PERM:  x[i] = B[perm[i]]      the sweeps see P B
//   store with PERM:  X[perm[i]] = x[i]      the caller gets P^T x
// One array serves both directions (a gather on the way in, a scatter on the way out); no inverse is stored.
#include <sparseframe_hip.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sf_plan_internal.h"

namespace sf {

// ---- one column: n doubles between the caller's vector and d_x ----
template <bool PERM>
__global__ void __launch_bounds__(256)
k_dev_load1(const double* __restrict__ B, const int32_t* __restrict__ perm, int64_t n, double* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    x[i] = B[PERM ? (int64_t)perm[i] : i];
}

template <bool PERM>
__global__ void __launch_bounds__(256)
k_dev_store1(const double* __restrict__ x, const int32_t* __restrict__ perm, int64_t n, double* __restrict__ X) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    X[PERM ? (int64_t)perm[i] : i] = x[i];
}

// ---- a chunk of cw <= SVM_W columns: column-major caller block <-> the row-major n x SVM_W block ----
// A workgroup moves a tile of DIO_ROWS rows x SVM_W columns through LDS.  On the column-major side lane = row (wave w takes the
// columns w, w + 4, ...): 64 consecutive doubles of one column per instruction, or with PERM 64 gathered / scattered ones.  On the
// row-major side the tile is DIO_ROWS * SVM_W consecutive doubles, thread t takes the doubles t, t + 256, ...: 128-byte rows,
// fully coalesced.  LDS rows are DIO_LD = SVM_W + 1 doubles apart: lane = row then walks an odd stride (no bank conflict), and the
// row-major side's index e + e / SVM_W is nearly consecutive.
constexpr int DIO_ROWS = 64;
constexpr int DIO_LD = SVM_W + 1;

template <bool PERM>
__global__ void __launch_bounds__(256)
k_dev_pack(const double* __restrict__ B, int64_t ldb, const int32_t* __restrict__ perm, int64_t n, int cw, double* __restrict__ X) {
    __shared__ double tile[DIO_ROWS * DIO_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * DIO_ROWS;
    const int64_t i = i0 + lane;
    if (i < n) {
        const int64_t src = PERM ? (int64_t)perm[i] : i;
#pragma unroll
        for (int c = wave; c < SVM_W; c += 4) tile[lane * DIO_LD + c] = (c < cw) ? B[src + (int64_t)c * ldb] : 0.0;
    }
    __syncthreads();
    const int64_t left = (n - i0) * SVM_W;      // doubles of the tile that exist
#pragma unroll
    for (int e = tid; e < DIO_ROWS * SVM_W; e += 256)
        if (e < left) X[i0 * SVM_W + e] = tile[(e / SVM_W) * DIO_LD + (e % SVM_W)];
}

template <bool PERM>
__global__ void __launch_bounds__(256)
k_dev_unpack(const double* __restrict__ X, const int32_t* __restrict__ perm, int64_t n, int cw, double* __restrict__ D, int64_t ldx) {
    __shared__ double tile[DIO_ROWS * DIO_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * DIO_ROWS;
    const int64_t left = (n - i0) * SVM_W;
#pragma unroll
    for (int e = tid; e < DIO_ROWS * SVM_W; e += 256)
        if (e < left) tile[(e / SVM_W) * DIO_LD + (e % SVM_W)] = X[i0 * SVM_W + e];
    __syncthreads();
    const int64_t i = i0 + lane;
    if (i < n) {
        const int64_t dst = PERM ? (int64_t)perm[i] : i;
#pragma unroll
        for (int c = wave; c < SVM_W; c += 4)
            if (c < cw) D[dst + (int64_t)c * ldx] = tile[lane * DIO_LD + c];
    }
}

// ---- values: Lx[p] = map[p] >= 0 ? Ax[map[p]] : 0.0, thread = entry, the store coalesced ----
__global__ void __launch_bounds__(256)
k_dev_gather_values(const double* __restrict__ Ax, const int64_t* __restrict__ map, int64_t count, double* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= count) return;
    const int64_t m = map[p];
    out[p] = m >= 0 ? Ax[m] : 0.0;
}

// part[blk] = max |v[k]| over the entries this workgroup strides over (LU plans: the scale of the pivot perturbation, which
// sf_lu_plan_set_values takes from its host array).  fmax drops a NaN, as std::max does there.
// (DIO_MAXB, sf_kernels.h: workgroups at most, and so the size of the parts buffer)
__global__ void __launch_bounds__(256)
k_dev_absmax(const double* __restrict__ v, int64_t count, double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double m = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + tid; k < count; k += (int64_t)gridDim.x * 256) m = fmax(m, fabs(v[k]));
    red[tid] = m;
    for (int h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

void launch_dev_load1(const double* B, const int32_t* perm, int64_t n, double* x, hipStream_t st) {
    const dim3 g((unsigned)((n + 255) / 256));
    if (perm) hipLaunchKernelGGL(k_dev_load1<true>, g, dim3(256), 0, st, B, perm, n, x);
    else hipLaunchKernelGGL(k_dev_load1<false>, g, dim3(256), 0, st, B, perm, n, x);
}
void launch_dev_store1(const double* x, const int32_t* perm, int64_t n, double* X, hipStream_t st) {
    const dim3 g((unsigned)((n + 255) / 256));
    if (perm) hipLaunchKernelGGL(k_dev_store1<true>, g, dim3(256), 0, st, x, perm, n, X);
    else hipLaunchKernelGGL(k_dev_store1<false>, g, dim3(256), 0, st, x, perm, n, X);
}
void launch_dev_pack(const double* B, int64_t ldb, const int32_t* perm, int64_t n, int cw, double* X, hipStream_t st) {
    const dim3 g((unsigned)((n + DIO_ROWS - 1) / DIO_ROWS));
    if (perm) hipLaunchKernelGGL(k_dev_pack<true>, g, dim3(256), 0, st, B, ldb, perm, n, cw, X);
    else hipLaunchKernelGGL(k_dev_pack<false>, g, dim3(256), 0, st, B, ldb, perm, n, cw, X);
}
void launch_dev_unpack(const double* X, const int32_t* perm, int64_t n, int cw, double* D, int64_t ldx, hipStream_t st) {
    const dim3 g((unsigned)((n + DIO_ROWS - 1) / DIO_ROWS));
    if (perm) hipLaunchKernelGGL(k_dev_unpack<true>, g, dim3(256), 0, st, X, perm, n, cw, D, ldx);
    else hipLaunchKernelGGL(k_dev_unpack<false>, g, dim3(256), 0, st, X, perm, n, cw, D, ldx);
}

void launch_dev_gather_values(const double* Ax, const int64_t* map, int64_t count, double* out, hipStream_t st) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_dev_gather_values, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, Ax, map, count, out);
}
int launch_dev_absmax(const double* v, int64_t count, double* part, hipStream_t st) {
    if (count <= 0) return 0;
    const int nb = (int)std::min<int64_t>(DIO_MAXB, (count + 255) / 256);
    hipLaunchKernelGGL(k_dev_absmax, dim3(nb), dim3(256), 0, st, v, count, part);
    return nb;
}

}  // namespace sf

// ---------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------
namespace {

enum { DIO_PERMUTE = -1 };      // not an op of the ABI: load and store with nothing in between

// load -> sweeps -> store for nrhs columns; pin / pout: the ordering for the way in / out, or null.  *total_ms: device time from
// the first to the last kernel of every chunk.
int dio_run(sf_chol_plan* p, int op, const int32_t* pin, const int32_t* pout, sf_long nrhs, const double* dB, sf_long ldb, double* dX,
            sf_long ldx, double* total_ms) {
    const int W = nrhs == 1 ? 1 : sf::SVM_W;        // (a lone column is never padded to SVM_W: the one-column family on d_x)
    if (W > 1)
        if (int rc = sf_solve_many_block(p)) return rc;
    const SfCols src{const_cast<double*>(dB), ldb, true, pin}, dst{dX, ldx, true, pout};
    const SfApply a{&src, &dst, nrhs, W, W == 1 ? p->d_x : p->d_xm, 0, op != DIO_PERMUTE};
    SfStretch t{p};
    int rc;
    if (op == DIO_PERMUTE) {
        rc = sf_apply_chunks(p, a, t, [](double*, sf_long, int) { return SF_OK; });
    } else {
        const SfSweep sweep = op == SF_OP_SOLVE ? SF_SWEEP_SOLVE : op == SF_OP_TRANS ? SF_SWEEP_TRANS : op == SF_OP_HALF_L ? SF_SWEEP_FWD_L : SF_SWEEP_BWD;
        // (the diagonal blocks' row-major copies: once per call; SF_OP_HALF_LT: no forward half has made them)
        rc = sf_apply_chunks(p, a, t, [&](double* x, sf_long j0, int) { return sf_apply_sweep(p, sweep, x, W, j0 == 0); });
    }
    *total_ms = t.total_ms;
    return rc;
}

int solve_device(sf_chol_plan* p, bool lu, int op, int flags, sf_long nrhs, const sf_float* dB, sf_long ldb, sf_float* dX, sf_long ldx) {
    if (!p || !dB || !dX || nrhs < 0) return SF_ERR_ARG;
    if (flags & ~(SF_DEV_PERM_IN | SF_DEV_PERM_OUT)) return SF_ERR_ARG;
    if (lu ? (op != SF_OP_SOLVE && op != SF_OP_TRANS) : (op != SF_OP_SOLVE && op != SF_OP_HALF_L && op != SF_OP_HALF_LT)) return SF_ERR_ARG;
    if (p->lu != lu) return SF_ERR_ARG;
    const sf_long ldmin = std::max<sf_long>(p->n, 1);
    if (ldb < ldmin || ldx < ldmin) return SF_ERR_ARG;
    if ((const void*)dX == (const void*)dB && ldx != ldb) return SF_ERR_ARG;
    if (!sf_plan_whole_resident(p)) return SF_ERR_ARG;
    if (flags && !p->d_perm) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (nrhs == 0 || p->n <= 0) return SF_OK;
    if (!sf_device_ptr_ok(p, dB, sf_block_span(p->n, nrhs, ldb)) || !sf_device_ptr_ok(p, dX, sf_block_span(p->n, nrhs, ldx))) return SF_ERR_ARG;
    double ms = 0;
    if (int rc = dio_run(p, op, (flags & SF_DEV_PERM_IN) ? p->d_perm : nullptr, (flags & SF_DEV_PERM_OUT) ? p->d_perm : nullptr, nrhs, dB, ldb,
                         dX, ldx, &ms))
        return rc;
    if (op == SF_OP_HALF_L || op == SF_OP_HALF_LT) p->last_half_ms = ms;
    else if (nrhs == 1) p->last_solve_ms = ms;
    else p->last_solve_many_ms = ms;
    return SF_OK;
}

// the side effects of sf_*_plan_set_values once the values are in d_Lx / d_Ux on the stream
int dio_values_done(sf_chol_plan* p) {
    hipStream_t st = p->stream;
    if (p->lu) {
        // max |a_ij| from the device arrays: the scale of the pivot perturbation
        if (!p->d_dio_part)
            if (int rc = p->d_dio_part.alloc(2 * (size_t)sf::DIO_MAXB)) return rc;
        std::vector<double> h(2 * sf::DIO_MAXB, 0.0);
        int nb[2] = {0, 0};
        const double* src[2] = {p->d_Lx, p->u_alias ? nullptr : p->d_Ux};
        const int64_t cnt[2] = {p->nnz, p->u_alias ? 0 : p->unz};
        for (int k = 0; k < 2; ++k) {
            if (!src[k] || cnt[k] <= 0) continue;
            nb[k] = sf::launch_dev_absmax(src[k], cnt[k], p->d_dio_part + (size_t)k * sf::DIO_MAXB, st);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h.data() + (size_t)k * sf::DIO_MAXB, p->d_dio_part + (size_t)k * sf::DIO_MAXB, (size_t)nb[k] * sizeof(double),
                                   hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
        double m = 0;
        for (int k = 0; k < 2; ++k)
            for (int b = 0; b < nb[k]; ++b) m = std::max(m, h[(size_t)k * sf::DIO_MAXB + b]);
        p->amax = m;
    } else {
        HIP_TRY(hipStreamSynchronize(st));
    }
    p->fs.values_changed();
    return SF_OK;
}

int set_values_device(sf_chol_plan* p, bool lu, const sf_float* dLx, const sf_float* dUx) {
    if (!p || p->lu != lu || (!dLx && p->nnz > 0)) return SF_ERR_ARG;
    const bool need_u = lu && !p->u_alias && p->unz > 0;
    if (need_u && !dUx) return SF_ERR_ARG;
    if (!sf_plan_whole_resident(p)) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (p->nnz > 0 && !sf_device_ptr_ok(p, dLx, (size_t)p->nnz)) return SF_ERR_ARG;
    if (need_u && !sf_device_ptr_ok(p, dUx, (size_t)p->unz)) return SF_ERR_ARG;
    if (p->nnz > 0) HIP_TRY(hipMemcpyAsync(p->d_Lx, dLx, p->nnz * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
    if (need_u) HIP_TRY(hipMemcpyAsync(p->d_Ux, dUx, p->unz * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
    return dio_values_done(p);
}

// map[0 .. count) all in [-1, nsrc)
bool dio_map_ok(const sf_long* map, int64_t count, sf_long nsrc) {
    for (int64_t k = 0; k < count; ++k)
        if (map[k] < -1 || map[k] >= nsrc) return false;
    return true;
}

}  // namespace

extern "C" {

int sf_chol_plan_set_ordering(sf_chol_plan* p, const sf_long* perm) {
    if (!p) return SF_ERR_ARG;
    const int64_t n = p->n;
    if (n > (int64_t)INT32_MAX) return SF_ERR_ARG;      // (the plan's own row indices, Lsi, are 32-bit: so are these)
    std::vector<int32_t> h((size_t)std::max<int64_t>(n, 1), 0);
    if (perm) {
        std::vector<char> seen((size_t)std::max<int64_t>(n, 1), 0);
        for (int64_t i = 0; i < n; ++i) {
            const sf_long o = perm[i];
            if (o < 0 || o >= n || seen[o]) return SF_ERR_ARG;
            seen[o] = 1;
            h[i] = (int32_t)o;
        }
    } else {
        for (int64_t i = 0; i < n; ++i) h[i] = (int32_t)i;
    }
    if (!sf_plan_whole_resident(p)) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    const size_t bytes = h.size() * sizeof(int32_t);
    sf::DevMem<int32_t> fresh;      // the first call's; the plan takes it once it is filled
    if (!p->d_perm)
        if (int rc = fresh.alloc(h.size())) return rc;
    HIP_TRY(hipStreamSynchronize(p->stream));       // (nothing of an earlier call still reads the old ordering)
    HIP_TRY(hipMemcpy(fresh ? fresh.get() : p->d_perm.get(), h.data(), bytes, hipMemcpyHostToDevice));
    if (fresh) {
        p->d_perm = std::move(fresh);
        p->bytes_ordering += bytes;
    }
    return SF_OK;
}
int sf_lu_plan_set_ordering(sf_lu_plan* p, const sf_long* perm) { return (p && p->lu) ? sf_chol_plan_set_ordering(p, perm) : SF_ERR_ARG; }

int sf_chol_plan_solve_device(sf_chol_plan* p, int op, int flags, sf_long nrhs, const sf_float* dB, sf_long ldb, sf_float* dX, sf_long ldx) {
    return solve_device(p, false, op, flags, nrhs, dB, ldb, dX, ldx);
}
int sf_lu_plan_solve_device(sf_lu_plan* p, int op, int flags, sf_long nrhs, const sf_float* dB, sf_long ldb, sf_float* dX, sf_long ldx) {
    return solve_device(p, true, op, flags, nrhs, dB, ldb, dX, ldx);
}

int sf_chol_plan_permute_device(sf_chol_plan* p, int inverse, sf_long nrhs, const sf_float* dB, sf_long ldb, sf_float* dX, sf_long ldx) {
    if (!p || !dB || !dX || nrhs < 0) return SF_ERR_ARG;
    const sf_long ldmin = std::max<sf_long>(p->n, 1);
    if (ldb < ldmin || ldx < ldmin) return SF_ERR_ARG;
    if ((const void*)dX == (const void*)dB) return SF_ERR_ARG;      // not in place: a permutation has no chunk-local form
    if (!sf_plan_whole_resident(p) || !p->d_perm) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (nrhs == 0 || p->n <= 0) return SF_OK;
    if (!sf_device_ptr_ok(p, dB, sf_block_span(p->n, nrhs, ldb)) || !sf_device_ptr_ok(p, dX, sf_block_span(p->n, nrhs, ldx))) return SF_ERR_ARG;
    double ms = 0;
    return dio_run(p, DIO_PERMUTE, inverse ? nullptr : p->d_perm, inverse ? p->d_perm : nullptr, nrhs, dB, ldb, dX, ldx, &ms);
}
int sf_lu_plan_permute_device(sf_lu_plan* p, int inverse, sf_long nrhs, const sf_float* dB, sf_long ldb, sf_float* dX, sf_long ldx) {
    return (p && p->lu) ? sf_chol_plan_permute_device(p, inverse, nrhs, dB, ldb, dX, ldx) : SF_ERR_ARG;
}

int sf_chol_plan_sample_device(sf_chol_plan* p, sf_long nsamples, uint64_t seed, uint64_t first_sample, int flags, sf_float* dX, sf_long ldx) {
    if (!p || !dX || nsamples < 0) return SF_ERR_ARG;
    if (flags & ~SF_DEV_PERM_OUT) return SF_ERR_ARG;
    if (ldx < std::max<sf_long>(p->n, 1)) return SF_ERR_ARG;
    if (p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    if (flags && !p->d_perm) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (nsamples == 0 || p->n <= 0) return SF_OK;
    if (!sf_device_ptr_ok(p, dX, sf_block_span(p->n, nsamples, ldx))) return SF_ERR_ARG;
    if (int rc = sf_solve_many_block(p)) return rc;
    const int W = sf::SVM_W;
    const SfCols dst{dX, ldx, true, flags ? p->d_perm : nullptr};
    SfStretch t{p};
    if (int rc = sf_apply_chunks(p, SfApply{nullptr, &dst, nsamples, W, p->d_xm, 0, true}, t, [&](double* x, sf_long j0, int cw) {
            sf::launch_sample_fill(x, p->n, cw, seed, first_sample + (uint64_t)j0, p->stream);
            return sf_apply_sweep(p, SF_SWEEP_BWD, x, W, j0 == 0);
        }))
        return rc;
    p->last_sample_ms = t.total_ms;
    return SF_OK;
}

int sf_chol_plan_set_values_device(sf_chol_plan* p, const sf_float* dLx) { return set_values_device(p, false, dLx, nullptr); }
int sf_lu_plan_set_values_device(sf_lu_plan* p, const sf_float* dLx, const sf_float* dUx) { return set_values_device(p, true, dLx, dUx); }

int sf_chol_plan_set_value_map(sf_chol_plan* p, sf_long nsrc, const sf_long* mapL, const sf_long* mapU) {
    if (!p || nsrc < 0 || (!mapL && p->nnz > 0)) return SF_ERR_ARG;
    const bool need_u = p->lu && !p->u_alias && p->unz > 0;
    if (need_u && !mapU) return SF_ERR_ARG;
    if (!dio_map_ok(mapL, p->nnz, nsrc) || (need_u && !dio_map_ok(mapU, p->unz, nsrc))) return SF_ERR_ARG;
    if (!sf_plan_whole_resident(p)) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    const size_t nl = (size_t)std::max<int64_t>(p->nnz, 1), nu = need_u ? (size_t)p->unz : 0;
    sf::DevMem<int64_t> fresh;      // the first call's; the plan takes it once it is filled
    if (!p->d_vmap)
        if (int rc = fresh.alloc(nl + nu)) return rc;
    int64_t* vmap = fresh ? fresh.get() : p->d_vmap.get();
    if (p->nnz > 0) HIP_TRY(hipMemcpy(vmap, mapL, (size_t)p->nnz * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nu) HIP_TRY(hipMemcpy(vmap + nl, mapU, nu * sizeof(int64_t), hipMemcpyHostToDevice));
    if (fresh) {
        p->d_vmap = std::move(fresh);
        p->bytes_ordering += (nl + nu) * sizeof(int64_t);
    }
    p->vmap_nsrc = nsrc;
    ++p->vmap_gen;      // (what sf_adjoint.hip derived from the old map is stale)
    return SF_OK;
}
int sf_lu_plan_set_value_map(sf_lu_plan* p, sf_long nsrc, const sf_long* mapL, const sf_long* mapU) {
    return (p && p->lu) ? sf_chol_plan_set_value_map(p, nsrc, mapL, mapU) : SF_ERR_ARG;
}

int sf_chol_plan_set_values_mapped_device(sf_chol_plan* p, const sf_float* dAx) {
    if (!p || !dAx) return SF_ERR_ARG;
    if (!sf_plan_whole_resident(p) || !p->d_vmap) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (p->vmap_nsrc > 0 && !sf_device_ptr_ok(p, dAx, (size_t)p->vmap_nsrc)) return SF_ERR_ARG;
    hipStream_t st = p->stream;
    const bool need_u = p->lu && !p->u_alias && p->unz > 0;
    const size_t nl = (size_t)std::max<int64_t>(p->nnz, 1);
    sf::launch_dev_gather_values(dAx, (const int64_t*)p->d_vmap, p->nnz, p->d_Lx, st);
    if (need_u) sf::launch_dev_gather_values(dAx, (const int64_t*)(p->d_vmap + nl), p->unz, p->d_Ux, st);
    HIP_TRY(hipGetLastError());
    return dio_values_done(p);
}
int sf_lu_plan_set_values_mapped_device(sf_lu_plan* p, const sf_float* dAx) {
    return (p && p->lu) ? sf_chol_plan_set_values_mapped_device(p, dAx) : SF_ERR_ARG;
}

}  // extern "C"
