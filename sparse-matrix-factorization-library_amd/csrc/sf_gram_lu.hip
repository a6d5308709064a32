// Half solves, G = C^T A^{-1} B and bordered systems with a resident LU factor (sf_lu_plan_solve_half, _gram, _gram_device).
// DESIGN 8i.
//
// Permuted space, A = L U in the plan's panels PL = d_Lsx and PU = d_Lsx + xC (U^T, lower, non-unit diagonal).  F is what the forward
// sweep of the solve applies (L^{-1}, or with pivoting on E_K^{-1} P_K ... E_1^{-1} P_1), so A^{-1} = U^{-1} F, A^{-T} = F^T U^{-T}:
//   half L   X <- F B        the forward steps over PL          (sf_solve_step_fwd)
//   half U   X <- U^{-1} B   the backward sweep over PU         (sf_solve_sweep_bwd)
//   half UT  X <- U^{-T} B   the forward steps over PU          (tsolve_sweep_fwd)
//   half LT  X <- F^T B      the backward twins over PL         (tsolve_sweep_bwd)
// and for an n x m block C and an n x k block B:  Z = U^{-T} C,  Y = F B,  G = Z^T Y -- two FORWARD sweeps, no backward one, the
// row-major diagonal copies (d_solveT) never touched.  Every sweep kernel, task list, sync word and ticket is sf_solve.hip's or
// sf_solve_t.hip's.  What is new here is the reduction over two stores:
//   k_gram2_part   the 16 x 16 tiles T(a, b) = Z_a^T Y_b, a = blockIdx.y, over one slab of rows each (k_gram_part's lane mapping,
//                  waves, accumulator chains and combine: gram_rows<false> of sf_gram_common.h)
//   k_gram2_final  the slabs' parts of a tile summed in slab order, the m x k result written -- no mirror, no triangle rule
// Chunk COLUMN b is reduced as soon as chunk b of B has been swept: one launch of each kernel, every a on a grid axis.
// One column (m == k == 1): the one-column sweeps on two n-vectors and k_dot_part / k_dot_final.  Nothing is padded to 16.
// No floating-point atomics and a fixed order in every reduction: for given Z and Y, G repeats bit for bit; entry (i, j) is a
// function of column i of C and column j of B alone.  G is not symmetric.
#include <sparseframe_hip.h>

#include <algorithm>

#include "sf_gram_common.h"
#include "sf_plan_internal.h"

namespace sf {

// part[(a * gridDim.x + slab) * 256 + 16 i + j] = sum over the slab's rows of Z_a[row][i] Yb[row][j], a = blockIdx.y.  slab_rows is
// a multiple of GRAM_STRETCH.  The four accumulators are added pairwise, the waves' sums then in wave order through LDS.
__global__ void __launch_bounds__(64 * GRAM_WAVES)
k_gram2_part(const double* __restrict__ Z, const double* __restrict__ Yb, int64_t n, int64_t slab_rows, double* __restrict__ part) {
    __shared__ double red[GRAM_WAVES][GRAM_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
    const int64_t r1 = min(n, r0 + slab_rows);
    const double* Za = Z + (int64_t)a * n * SVM_W;
    double4_t acc[GRAM_ACC];
#pragma unroll
    for (int u = 0; u < GRAM_ACC; ++u) acc[u] = double4_t{0.0, 0.0, 0.0, 0.0};
    gram_rows<false>(Za, Yb, r0, r1, wave, lane, acc);
    const double4_t s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) red[wave][((lane >> 4) + 4 * q) * SVM_W + (lane & 15)] = s[q];
    __syncthreads();
    double v = red[0][tid];
#pragma unroll
    for (int w = 1; w < GRAM_WAVES; ++w) v += red[w][tid];
    part[((int64_t)a * gridDim.x + blockIdx.x) * GRAM_TILE + tid] = v;
}

// tile (a = blockIdx.x, b) = its nparts parts in slab order; thread t = (i = t / 16 of chunk a of C, j = t % 16 of chunk b of B)
// writes G[16 a + i][16 b + j] (column-major, leading dimension ldg); an index >= m or >= k is padding and is never written
__global__ void __launch_bounds__(GRAM_TILE)
k_gram2_final(const double* __restrict__ part, int nparts, int b, int64_t m, int64_t k, double* __restrict__ G, int64_t ldg) {
    const int tid = threadIdx.x, a = blockIdx.x;
    const double* p = part + (int64_t)a * nparts * GRAM_TILE + tid;
    double v = 0.0;
    for (int s = 0; s < nparts; ++s) v += p[(int64_t)s * GRAM_TILE];
    const int64_t gi = (int64_t)a * SVM_W + tid / SVM_W, gj = (int64_t)b * SVM_W + tid % SVM_W;
    if (gi >= m || gj >= k) return;
    G[gi + gj * ldg] = v;
}

// part[blk] = the sum of x[i] y[i] over the entries this workgroup strides over, then a tree over its 256 threads: a fixed order
__global__ void __launch_bounds__(256)
k_dot_part(const double* __restrict__ x, const double* __restrict__ y, int64_t n, double* __restrict__ part) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) v += x[i] * y[i];
    red[tid] = v;
    for (int h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (tid < h) red[tid] += red[tid + h];
    }
    if (tid == 0) part[blockIdx.x] = red[0];
}

// *out = the np parts: thread t sums the parts t, t + 256, ... in order, then the same tree
__global__ void __launch_bounds__(256)
k_dot_final(const double* __restrict__ part, int np, double* __restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int q = tid; q < np; q += 256) v += part[q];
    red[tid] = v;
    for (int h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (tid < h) red[tid] += red[tid + h];
    }
    if (tid == 0) *out = red[0];
}

void launch_gram2_col(const double* Z, const double* Yb, int64_t n, int nza, int b, int64_t m, int64_t k, double* part, double* G,
                      int64_t ldg, hipStream_t st) {
    int64_t slab_rows = 0;
    const int ns = gram_slabs(n, &slab_rows);
    hipLaunchKernelGGL(k_gram2_part, dim3(ns, nza), dim3(64 * GRAM_WAVES), 0, st, Z, Yb, n, slab_rows, part);
    hipLaunchKernelGGL(k_gram2_final, dim3(nza), dim3(GRAM_TILE), 0, st, (const double*)part, ns, b, m, k, G, ldg);
}

void launch_dot(const double* x, const double* y, int64_t n, double* scratch, double* out, hipStream_t st) {
    const int nb = (int)std::min<int64_t>(QF_MAXB, (n + 255) / 256);
    hipLaunchKernelGGL(k_dot_part, dim3(nb), dim3(256), 0, st, x, y, n, scratch);
    hipLaunchKernelGGL(k_dot_final, dim3(1), dim3(256), 0, st, (const double*)scratch, nb, out);
}

}  // namespace sf

// ---------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------
namespace {

// doubles of the store for nz chunks of C and ny chunks of B: the Z blocks | the Y blocks | the parts of one chunk column | the
// padded (16 nz) x (16 ny) result of the host-array call
struct Gram2Layout { size_t z, y, part, g; };
Gram2Layout lug_layout(int64_t n, int64_t nz, int64_t ny) {
    int64_t slab_rows = 0;
    const int ns = sf::gram_slabs(n, &slab_rows);
    return Gram2Layout{(size_t)nz * n * sf::SVM_W, (size_t)ny * n * sf::SVM_W, (size_t)nz * ns * sf::GRAM_TILE,
                       (size_t)(nz * sf::SVM_W) * (ny * sf::SVM_W)};
}

// the store for nz and ny chunks: allocated or grown here (never shrunk on either side); a failure leaves the plan and a smaller
// store as they were
int lug_store(sf_chol_plan* p, int64_t nz, int64_t ny) {
    if (p->d_gram && p->gram_chunks >= nz && p->gram_chunks_y >= ny) return SF_OK;
    nz = std::max(nz, p->gram_chunks);
    ny = std::max(ny, p->gram_chunks_y);
    const Gram2Layout L = lug_layout(p->n, nz, ny);
    const size_t count = L.z + L.y + L.part + L.g;
    sf::DevMem<double> fresh;
    if (int rc = fresh.alloc(count)) return rc;
    p->d_gram = std::move(fresh);       // (frees the smaller store: every call returns with its work complete, nothing still reads it)
    p->gram_chunks = nz;
    p->gram_chunks_y = ny;
    p->bytes_gram = count * sizeof(double);
    return SF_OK;
}

// C, B (host, dev == false; device otherwise, pin = the ordering for the way in or null) -> G.  Host: G is the caller's array, filled
// from the store's result block; device: the final kernel writes the caller's dG itself.
int lug_run(sf_chol_plan* p, bool dev, const int32_t* pin, sf_long m, const double* C, sf_long ldc, sf_long k, const double* B, sf_long ldb,
            double* G, sf_long ldg) {
    hipStream_t st = p->stream;
    const int64_t n = p->n;
    const int W = sf::SVM_W;
    const SfCols srcC{const_cast<double*>(C), ldc, dev, pin}, srcB{const_cast<double*>(B), ldb, dev, pin};
    SfStretch t{p};
    if (!dev || (m == 1 && k == 1))
        if (int rc = sf_solve_many_block(p)) return rc;     // (its staging half takes the chunks of a host block; one column: z)
    if (m == 1 && k == 1) {
        // the one-column family: z = U^{-T} c in the first n doubles of d_xm, y = F b in d_x, then their dot product
        if (int rc = sf_quadform_scratch(p)) return rc;
        double* z = p->d_xm;
        double* d_out = p->d_qf + (size_t)sf::QF_MAXB;
        // spelled out with the driver's pieces: both columns are staged before the first of the two stretches
        if (int rc = sf_cols_stage_in(p, srcC, 0, 1, z)) return rc;
        if (int rc = sf_cols_stage_in(p, srcB, 0, 1, p->d_x)) return rc;
        if (int rc = t.open()) return rc;
        sf_cols_load(p, srcC, 0, 1, 1, z, z);
        if (int rc = sf_apply_sweep(p, SF_SWEEP_FWD_UT, z, 1, false)) return rc;
        if (int rc = t.mark()) return rc;
        if (int rc = t.close(true)) return rc;
        if (int rc = t.open()) return rc;
        sf_cols_load(p, srcB, 0, 1, 1, p->d_x, p->d_x);
        if (int rc = sf_apply_sweep(p, SF_SWEEP_FWD_L, p->d_x, 1, false)) return rc;
        sf::launch_dot(z, p->d_x, n, p->d_qf, d_out, st);
        if (int rc = t.mark()) return rc;
        HIP_TRY(hipMemcpyAsync(G, d_out, sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        if (int rc = t.close(true)) return rc;
        p->last_gram_ms = t.total_ms;
        p->last_gram_parts = 0;
        return SF_OK;
    }
    const int64_t nz = (m + W - 1) / W, ny = (k + W - 1) / W;
    if (int rc = lug_store(p, nz, ny)) return rc;
    const Gram2Layout L = lug_layout(n, p->gram_chunks, p->gram_chunks_y);
    double* Z = p->d_gram;
    double* Y = Z + L.z;
    double* part = Y + L.y;
    double* Gd = dev ? G : part + L.part;
    const int64_t ldgd = dev ? ldg : m;
    // every chunk into its own block of the store: Z = U^{-T} C first, then Y = F B, column b of G as soon as chunk b has been swept
    if (int rc = sf_apply_chunks(p, SfApply{&srcC, nullptr, m, W, Z, (size_t)n * W, true}, t,
                                 [&](double* Za, sf_long, int) { return sf_apply_sweep(p, SF_SWEEP_FWD_UT, Za, W, false); }))
        return rc;
    if (int rc = sf_apply_chunks(p, SfApply{&srcB, nullptr, k, W, Y, (size_t)n * W, true}, t, [&](double* Yb, sf_long j0, int) {
            if (int rc = sf_apply_sweep(p, SF_SWEEP_FWD_L, Yb, W, false)) return rc;
            sf::launch_gram2_col(Z, Yb, n, (int)nz, (int)(j0 / W), m, k, part, Gd, ldgd, st);
            return SF_OK;
        }))
        return rc;
    if (!dev) {
        HIP_TRY(hipMemcpy2DAsync(G, (size_t)ldg * sizeof(double), Gd, (size_t)m * sizeof(double), (size_t)m * sizeof(double), k,
                                 hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    int64_t slab_rows = 0;
    p->last_gram_parts = sf::gram_slabs(n, &slab_rows);
    p->last_gram_ms = t.total_ms;
    return SF_OK;
}

// the checks both gram entry points share once their pointers are known to be there: the arguments first, then the plan
int lug_args(sf_chol_plan* p, sf_long m, sf_long ldc, sf_long k, sf_long ldb, sf_long ldg) {
    if (m < 0 || m > SF_GRAM_MAX_K || k < 0 || k > SF_GRAM_MAX_K) return SF_ERR_ARG;
    const sf_long ldmin = std::max<sf_long>(p->n, 1);
    if (ldc < ldmin || ldb < ldmin || ldg < std::max<sf_long>(m, 1)) return SF_ERR_ARG;
    if (!p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    return SF_OK;
}

}  // namespace

extern "C" {

int sf_lu_plan_solve_half(sf_lu_plan* p, int which, sf_long nrhs, const sf_float* B, sf_long ldb, sf_float* X, sf_long ldx) {
    if (!p || !B || !X || nrhs < 0) return SF_ERR_ARG;
    if (which != SF_LU_HALF_L && which != SF_LU_HALF_U && which != SF_LU_HALF_UT && which != SF_LU_HALF_LT) return SF_ERR_ARG;
    const sf_long ldmin = std::max<sf_long>(p->n, 1);
    if (ldb < ldmin || ldx < ldmin) return SF_ERR_ARG;
    if ((const void*)X == (const void*)B && ldx != ldb) return SF_ERR_ARG;
    if (!p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (nrhs == 0 || p->n <= 0) return SF_OK;
    const int W = nrhs == 1 ? 1 : sf::SVM_W;        // (one column: the one-column family on d_x)
    if (W > 1)
        if (int rc = sf_solve_many_block(p)) return rc;
    const SfSweep op = which == SF_LU_HALF_L ? SF_SWEEP_FWD_L : which == SF_LU_HALF_U ? SF_SWEEP_BWD : which == SF_LU_HALF_UT ? SF_SWEEP_FWD_UT : SF_SWEEP_BWD_LT;
    const SfCols src{const_cast<double*>(B), ldb, false, nullptr}, dst{X, ldx, false, nullptr};
    SfStretch t{p};
    // (a backward half's diagonal copies: the first chunk of EVERY call)
    if (int rc = sf_apply_chunks(p, SfApply{&src, &dst, nrhs, W, W == 1 ? p->d_x : p->d_xm, 0, true}, t,
                                 [&](double* x, sf_long j0, int) { return sf_apply_sweep(p, op, x, W, j0 == 0); }))
        return rc;
    p->last_half_ms = t.total_ms;
    return SF_OK;
}

int sf_lu_plan_gram(sf_lu_plan* p, sf_long m, const sf_float* C, sf_long ldc, sf_long k, const sf_float* B, sf_long ldb, sf_float* G,
                    sf_long ldg) {
    if (!p || !C || !B || !G) return SF_ERR_ARG;
    if (int rc = lug_args(p, m, ldc, k, ldb, ldg)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (m == 0 || k == 0) return SF_OK;
    if (p->n <= 0) {
        for (sf_long j = 0; j < k; ++j)
            for (sf_long i = 0; i < m; ++i) G[i + j * ldg] = 0.0;       // (n == 0: the empty sums)
        return SF_OK;
    }
    return lug_run(p, false, nullptr, m, C, ldc, k, B, ldb, G, ldg);
}

int sf_lu_plan_gram_device(sf_lu_plan* p, int flags, sf_long m, const sf_float* dC, sf_long ldc, sf_long k, const sf_float* dB, sf_long ldb,
                           sf_float* dG, sf_long ldg) {
    if (!p || !dC || !dB || !dG) return SF_ERR_ARG;
    if (flags & ~SF_DEV_PERM_IN) return SF_ERR_ARG;
    if (int rc = lug_args(p, m, ldc, k, ldb, ldg)) return rc;
    if (flags && !p->d_perm) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (m == 0 || k == 0) return SF_OK;
    const size_t span_c = sf_block_span(p->n, m, ldc), span_b = sf_block_span(p->n, k, ldb), span_g = sf_block_span(m, k, ldg);
    if ((span_c && !sf_device_ptr_ok(p, dC, span_c)) || (span_b && !sf_device_ptr_ok(p, dB, span_b)) || !sf_device_ptr_ok(p, dG, span_g))
        return SF_ERR_ARG;
    // the result overlaps an input (n == 0: there are none)
    if (p->n > 0 && (sf_blocks_overlap(dG, span_g, dC, span_c) || sf_blocks_overlap(dG, span_g, dB, span_b))) return SF_ERR_ARG;
    if (p->n <= 0) {
        HIP_TRY(hipMemset2DAsync(dG, (size_t)ldg * sizeof(double), 0, (size_t)m * sizeof(double), k, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return SF_OK;
    }
    return lug_run(p, true, flags ? p->d_perm : nullptr, m, dC, ldc, k, dB, ldb, dG, ldg);
}

}  // extern "C"
