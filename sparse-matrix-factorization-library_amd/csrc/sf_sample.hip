// Half solves, quadratic forms and Gaussian sampling with a resident Cholesky factor (sf_chol_plan_solve_half, _quadform,
// _sample).  DESIGN 8f.
//
// Permuted space, A = L L^T.  The two sweeps of the plain solve run on their own:
//   X <- L^{-1} B      the forward steps (sf_solve_step_fwd), nothing else           -- whitening
//   X <- L^{-T} B      the backward sweep (sf_solve_sweep_bwd), nothing else
//   q_j = |L^{-1} b_j|^2 = b_j^T A^{-1} b_j     forward steps, then a per-column sum of squares (k_quadform_part / _final)
//   x = L^{-T} z, z ~ N(0, I)                    k_sample_fill writes z into the row-major block, then the backward sweep:
//                                                Cov(x) = L^{-T} L^{-1} = A^{-1}
// No new sweep kernel: the kernels, task lists, sync words and tickets are sf_solve.hip's.  One column runs the one-column family
// on d_x (a 16-wide chunk costs about 5 x a one-column solve), more than one the SVM_W family on d_xm with
// sf_chol_plan_solve_many's pack / unpack and staging; sample always the SVM_W family, its block is generated in that layout.
// The backward-only calls ask for the row-major copies of the top steps' diagonal blocks on their first chunk: no forward half
// of the same call has made them, and a refactorization since the last solve would have left them stale.
#include <sparseframe_hip.h>

#include <algorithm>
#include <cmath>

#include "sf_plan_internal.h"
#include "sf_solve_common.h"

namespace sf {

// ---------------------------------------------------------------------------------------------------
// The normal generator.  Element (i, s) of the infinite matrix -- i = permuted row, s = global sample index -- is a function of
// (seed, i, s) alone: Philox4x32-10 on the counter (i lo, i hi, p lo, p hi), p = s >> 1, with the key (seed lo, seed hi) gives
// four words -> two uniforms -> one Box-Muller pair; the even s of the pair takes the cosine, the odd one the sine.
// ---------------------------------------------------------------------------------------------------
struct NormalPair { double c, s; };

__device__ __forceinline__ double sample_uniform(uint32_t a, uint32_t b) {
    // 27 + 26 bits, then the half that keeps 0 out: (0, 1]
    const uint64_t k = ((uint64_t)(a >> 5) << 26) + (uint64_t)(b >> 6);
    return ((double)k + 0.5) * 0x1p-53;
}

__device__ __forceinline__ NormalPair sample_normal_pair(uint64_t seed, uint64_t i, uint64_t p) {
    uint32_t c0 = (uint32_t)i, c1 = (uint32_t)(i >> 32), c2 = (uint32_t)p, c3 = (uint32_t)(p >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const double u1 = sample_uniform(c0, c1), u2 = sample_uniform(c2, c3);
    const double rad = sqrt(-2.0 * log(u1));
    const double th = 6.283185307179586 * u2;
    return NormalPair{rad * cos(th), rad * sin(th)};
}

// X[i][c] = normal(i, s0 + c) for c < cw, 0 for cw <= c < SVM_W: the n x SVM_W row-major block.  Thread e = (row e / 8, column
// pair e % 8) stores two adjacent doubles, eight consecutive threads one 128-byte row.  s0 even: the two columns are one Box-Muller
// pair, one Philox evaluation; s0 odd: they are the sine of one pair and the cosine of the next (the branch is uniform).
__global__ void __launch_bounds__(256)
k_sample_fill(double* __restrict__ X, int64_t n, int cw, uint64_t seed, uint64_t s0) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * (SVM_W / 2)) return;
    const int64_t i = e / (SVM_W / 2);
    const int c = 2 * (int)(e % (SVM_W / 2));
    double2 v = {0.0, 0.0};
    if (c < cw) {
        const uint64_t s = s0 + (uint64_t)c;
        const NormalPair a = sample_normal_pair(seed, (uint64_t)i, s >> 1);
        if (!(s & 1)) {
            v.x = a.c;
            v.y = a.s;
        } else {
            v.x = a.s;
            if (c + 1 < cw) v.y = sample_normal_pair(seed, (uint64_t)i, (s >> 1) + 1).c;
        }
        if (c + 1 >= cw) v.y = 0.0;
    }
    *reinterpret_cast<double2*>(X + i * SVM_W + c) = v;
}

// ---------------------------------------------------------------------------------------------------
// q[c] = sum_i X[i][c]^2 of the row-major n x W block (W = 1: the vector), two passes in a fixed order, no floating-point atomics:
// the same block gives the same bits on every call, and a NaN or Inf stays in its column.
// Thread t = (row group t / W, column t % W); consecutive threads read consecutive doubles.
// ---------------------------------------------------------------------------------------------------
// (QF_MAXB, sf_kernels.h: workgroups of the first pass at most -- they stride over the rows -- and so the size of the parts buffer)
template <int W>
__device__ __forceinline__ double qf_tree(double* red, double v, int tid) {
    red[tid] = v;
    for (int h = 128; h >= W; h >>= 1) {
        __syncthreads();
        if (tid < h) red[tid] += red[tid + h];          // (h is a multiple of W: the partner holds the same column)
    }
    __syncthreads();
    return red[tid % W];
}

// part[blk][c] = the sum over the rows this workgroup visits: row group g takes the rows g, g + G, ... of every stretch (G = 256 / W)
template <int W>
__global__ void __launch_bounds__(256)
k_quadform_part(const double* __restrict__ X, int64_t n, double* __restrict__ part) {
    __shared__ double red[256];
    constexpr int G = 256 / W;
    const int tid = threadIdx.x, c = tid % W;
    double v = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * G + tid / W; i < n; i += (int64_t)gridDim.x * G) {
        const double x = X[i * W + c];
        v += x * x;
    }
    const double sum = qf_tree<W>(red, v, tid);
    if (tid < W) part[(int64_t)blockIdx.x * W + c] = sum;
}

// out[c] = sum over the np parts: row group g sums the parts g, g + G, ... in order, then the same tree
template <int W>
__global__ void __launch_bounds__(256)
k_quadform_final(const double* __restrict__ part, int np, double* __restrict__ out) {
    __shared__ double red[256];
    constexpr int G = 256 / W;
    const int tid = threadIdx.x, c = tid % W;
    double v = 0.0;
    for (int k = tid / W; k < np; k += G) v += part[(int64_t)k * W + c];
    const double sum = qf_tree<W>(red, v, tid);
    if (tid < W) out[c] = sum;
}

void launch_sample_fill(double* X, int64_t n, int cw, uint64_t seed, uint64_t s0, hipStream_t st) {
    const int64_t m = n * (SVM_W / 2);
    if (m > 0) hipLaunchKernelGGL(k_sample_fill, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, X, n, cw, seed, s0);
}

// scratch: QF_MAXB x width parts, then the width results
void launch_quadform(const double* X, int64_t n, int width, double* scratch, hipStream_t st) {
    const int G = 256 / width;
    const int nb = (int)std::min<int64_t>(QF_MAXB, (n + G - 1) / G);
    double* out = scratch + (size_t)QF_MAXB * width;
    if (width == 1) {
        hipLaunchKernelGGL(k_quadform_part<1>, dim3(nb), dim3(256), 0, st, X, n, scratch);
        hipLaunchKernelGGL(k_quadform_final<1>, dim3(1), dim3(256), 0, st, (const double*)scratch, nb, out);
    } else {
        hipLaunchKernelGGL(k_quadform_part<SVM_W>, dim3(nb), dim3(256), 0, st, X, n, scratch);
        hipLaunchKernelGGL(k_quadform_final<SVM_W>, dim3(1), dim3(256), 0, st, (const double*)scratch, nb, out);
    }
}

}  // namespace sf

// ---------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------
namespace {

// the checks every entry point makes once its own arguments are in order, on whole, resident Cholesky plans; *go = false: nothing
// to do (SF_OK)
int half_begin(sf_chol_plan* p, sf_long count, bool* go) {
    *go = false;
    if (p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    *go = count > 0 && p->n > 0;
    return SF_OK;
}

}  // namespace

extern "C" {

int sf_chol_plan_solve_half(sf_chol_plan* p, int which, sf_long nrhs, const sf_float* B, sf_long ldb, sf_float* X, sf_long ldx) {
    if (!p || !B || !X || nrhs < 0 || (which != SF_HALF_L && which != SF_HALF_LT)) return SF_ERR_ARG;
    const sf_long ldmin = std::max<sf_long>(p->n, 1);
    if (ldb < ldmin || ldx < ldmin) return SF_ERR_ARG;
    if ((const void*)X == (const void*)B && ldx != ldb) return SF_ERR_ARG;
    bool go = false;
    if (int rc = half_begin(p, nrhs, &go)) return rc;
    if (!go) return SF_OK;
    const int W = nrhs == 1 ? 1 : sf::SVM_W;        // (one column: the one-column family on d_x)
    if (W > 1)
        if (int rc = sf_solve_many_block(p)) return rc;
    const SfSweep op = which == SF_HALF_L ? SF_SWEEP_FWD_L : SF_SWEEP_BWD;
    const SfCols src{const_cast<double*>(B), ldb, false, nullptr}, dst{X, ldx, false, nullptr};
    SfStretch t{p};
    // (the diagonal blocks' row-major copies: once per call)
    if (int rc = sf_apply_chunks(p, SfApply{&src, &dst, nrhs, W, W == 1 ? p->d_x : p->d_xm, 0, true}, t,
                                 [&](double* x, sf_long j0, int) { return sf_apply_sweep(p, op, x, W, j0 == 0); }))
        return rc;
    p->last_half_ms = t.total_ms;
    return SF_OK;
}

int sf_chol_plan_quadform(sf_chol_plan* p, sf_long nrhs, const sf_float* B, sf_long ldb, sf_float* q) {
    if (!p || !B || !q || nrhs < 0) return SF_ERR_ARG;
    if (ldb < std::max<sf_long>(p->n, 1)) return SF_ERR_ARG;
    bool go = false;
    if (int rc = half_begin(p, nrhs, &go)) return rc;
    if (!go) {
        for (sf_long j = 0; j < nrhs; ++j) q[j] = 0.0;      // (n == 0: the empty sum)
        return SF_OK;
    }
    if (int rc = sf_quadform_scratch(p)) return rc;
    hipStream_t st = p->stream;
    const int W = nrhs == 1 ? 1 : sf::SVM_W;
    if (W > 1)
        if (int rc = sf_solve_many_block(p)) return rc;
    const double* d_q = p->d_qf + (size_t)sf::QF_MAXB * W;
    const SfCols src{const_cast<double*>(B), ldb, false, nullptr};
    SfStretch t{p};
    if (int rc = sf_apply_chunks(
            p, SfApply{&src, nullptr, nrhs, W, W == 1 ? p->d_x : p->d_xm, 0, true}, t,
            [&](double* x, sf_long, int) {
                if (int rc = sf_apply_sweep(p, SF_SWEEP_FWD_L, x, W, false)) return rc;
                sf::launch_quadform(x, p->n, W, p->d_qf, st);
                return SF_OK;
            },
            [&](double*, sf_long j0, int cw) {
                HIP_TRY(hipMemcpyAsync(q + j0, d_q, (size_t)cw * sizeof(double), hipMemcpyDeviceToHost, st));
                return SF_OK;
            }))
        return rc;
    p->last_quadform_ms = t.total_ms;
    return SF_OK;
}

int sf_chol_plan_sample(sf_chol_plan* p, sf_long nsamples, uint64_t seed, uint64_t first_sample, sf_float* X, sf_long ldx, sf_float* Z,
                        sf_long ldz) {
    if (!p || !X || nsamples < 0) return SF_ERR_ARG;
    const sf_long ldmin = std::max<sf_long>(p->n, 1);
    if (ldx < ldmin || (Z && ldz < ldmin) || (Z && (const void*)Z == (const void*)X)) return SF_ERR_ARG;
    bool go = false;
    if (int rc = half_begin(p, nsamples, &go)) return rc;
    if (!go) return SF_OK;
    if (int rc = sf_solve_many_block(p)) return rc;
    hipStream_t st = p->stream;
    const int W = sf::SVM_W;
    double* stage = p->d_xm + (size_t)p->n * W;
    const SfCols dst{X, ldx, false, nullptr}, zdst{Z, ldz, false, nullptr};
    SfStretch t{p};
    if (int rc = sf_apply_chunks(p, SfApply{nullptr, &dst, nsamples, W, p->d_xm, 0, true}, t, [&](double* x, sf_long j0, int cw) {
            sf::launch_sample_fill(x, p->n, cw, seed, first_sample + (uint64_t)j0, st);
            if (Z) {
                // the normals leave through the staging half before the sweep overwrites the block; their copy is not device time,
                // so the timed stretch ends here and a second one holds the sweep
                sf_cols_store(p, zdst, j0, cw, W, x, stage);
                if (int rc = t.mark()) return rc;
                if (int rc = sf_cols_stage_out(p, zdst, j0, cw, stage)) return rc;
                if (int rc = t.close(false)) return rc;
                if (int rc = t.open()) return rc;
            }
            return sf_apply_sweep(p, SF_SWEEP_BWD, x, W, j0 == 0);
        }))
        return rc;
    p->last_sample_ms = t.total_ms;
    return SF_OK;
}

}  // extern "C"
