// The dense Schur complement of a border, G = B^T A^{-1} B, with a resident Cholesky factor (sf_chol_plan_gram, _gram_device).
// DESIGN 8h.
//
// Permuted space, A = L L^T:  Y = L^{-1} B,  G = Y^T Y.  One FORWARD sweep per chunk of SVM_W columns -- the kernels, task lists, sync
// words and tickets are sf_solve.hip's, as in sf_sample.hip -- into the plan's Y store (d_gram: chunk c is the row-major n x SVM_W
// block at c * n * SVM_W; Y never leaves the device), then the reduction, which is what is new here:
//   k_gram_part   the 16 x 16 tiles T(a, b) = Y_a^T Y_b, b <= a, over one slab of rows each: v_mfma_f64_16x16x4_f64 straight from
//                 the row-major blocks (64 consecutive doubles are one 4-row x 16-column operand slice: no transposition)
//   k_gram_final  the slabs' parts of a tile summed in order, the tile and its mirror written into the k x k result
// Chunk row a is reduced as soon as chunk a has been swept: one launch of each kernel per chunk row, the pair index b on a grid axis.
// No floating-point atomics and a fixed order everywhere: for a given Y, G repeats bit for bit; G is bit-for-bit symmetric (a tile
// below the diagonal is stored twice, a diagonal tile mirrors its lower triangle); entry (i, j) is a function of the columns i and j
// of Y alone, so a NaN or Inf in column j of B reaches row j and column j of G and nothing else.
// One column: the one-column sweep on d_x and launch_quadform, so G[0] is exactly what sf_chol_plan_quadform returns.
#include <sparseframe_hip.h>

#include <algorithm>

#include "sf_gram_common.h"
#include "sf_plan_internal.h"

namespace sf {

// (the stretches of a slab, GRAM_WAVES / GRAM_ACC / GRAM_STRETCH / GRAM_TILE and gram_rows: sf_gram_common.h, shared with sf_gram_lu.hip)

// part[(b * gridDim.x + slab) * 256 + 16 i + j] = sum over the slab's rows of Ya[row][i] Yb[row][j], a = the chunk row of the launch,
// b = blockIdx.y <= a.  slab_rows is a multiple of GRAM_STRETCH.  The four accumulators are added pairwise, the waves' sums then in
// wave order through LDS: a fixed order.
__global__ void __launch_bounds__(64 * GRAM_WAVES)
k_gram_part(const double* __restrict__ Y, int64_t n, int a, int64_t slab_rows, double* __restrict__ part) {
    __shared__ double red[GRAM_WAVES][GRAM_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
    const int64_t r1 = min(n, r0 + slab_rows);
    const double* Ya = Y + (int64_t)a * n * SVM_W;
    const double* Yb = Y + (int64_t)b * n * SVM_W;
    double4_t acc[GRAM_ACC];
#pragma unroll
    for (int u = 0; u < GRAM_ACC; ++u) acc[u] = double4_t{0.0, 0.0, 0.0, 0.0};
    if (a == b) gram_rows<true>(Ya, Ya, r0, r1, wave, lane, acc);
    else gram_rows<false>(Ya, Yb, r0, r1, wave, lane, acc);
    const double4_t s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) red[wave][((lane >> 4) + 4 * q) * SVM_W + (lane & 15)] = s[q];
    __syncthreads();
    double v = red[0][tid];
#pragma unroll
    for (int w = 1; w < GRAM_WAVES; ++w) v += red[w][tid];
    part[((int64_t)b * gridDim.x + blockIdx.x) * GRAM_TILE + tid] = v;
}

// tile (a, b = blockIdx.x) = its nparts parts in order; thread t = (i = t / 16 of chunk a, j = t % 16 of chunk b) writes
// G[16 a + i][16 b + j] and the mirror (column-major, leading dimension ldg; indices >= k are padding and are not written).
// a == b: the threads i >= j write both triangles from ONE value.
__global__ void __launch_bounds__(GRAM_TILE)
k_gram_final(const double* __restrict__ part, int nparts, int a, int64_t k, double* __restrict__ G, int64_t ldg) {
    const int tid = threadIdx.x, b = blockIdx.x;
    const double* p = part + (int64_t)b * nparts * GRAM_TILE + tid;
    double v = 0.0;
    for (int s = 0; s < nparts; ++s) v += p[(int64_t)s * GRAM_TILE];
    const int i = tid / SVM_W, j = tid % SVM_W;
    const int64_t gi = (int64_t)a * SVM_W + i, gj = (int64_t)b * SVM_W + j;
    if (gi >= k || gj >= k || (a == b && i < j)) return;
    G[gi + gj * ldg] = v;
    if (gi != gj) G[gj + gi * ldg] = v;
}

// The grid rule: slabs of about GRAM_SLAB_ROWS rows, a whole number of stretches each, GRAM_MAX_SLABS at most --
// two workgroups per tile from n = 2 * GRAM_SLAB_ROWS = 4096 upward, the device's 256 CUs covered by one tile from n = 2^19.
int gram_slabs(int64_t n, int64_t* slab_rows) {
    const int64_t want = std::min<int64_t>(GRAM_MAX_SLABS, std::max<int64_t>(1, (n + GRAM_SLAB_ROWS - 1) / GRAM_SLAB_ROWS));
    const int64_t rows = (((n + want - 1) / want + GRAM_STRETCH - 1) / GRAM_STRETCH) * GRAM_STRETCH;
    *slab_rows = rows;
    return (int)((n + rows - 1) / rows);
}

void launch_gram_row(const double* Y, int64_t n, int a, int64_t k, double* part, double* G, int64_t ldg, hipStream_t st) {
    int64_t slab_rows = 0;
    const int ns = gram_slabs(n, &slab_rows);
    hipLaunchKernelGGL(k_gram_part, dim3(ns, a + 1), dim3(64 * GRAM_WAVES), 0, st, Y, n, a, slab_rows, part);
    hipLaunchKernelGGL(k_gram_final, dim3(a + 1), dim3(GRAM_TILE), 0, st, (const double*)part, ns, a, k, G, ldg);
}

}  // namespace sf

// ---------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------
namespace {

// doubles of the store for nch chunks: the Y blocks | the parts of one chunk row | the (16 nch)^2 result of the host-array call
struct GramLayout { size_t y, part, g; };
GramLayout gram_layout(int64_t n, int64_t nch) {
    int64_t slab_rows = 0;
    const int ns = sf::gram_slabs(n, &slab_rows);
    return GramLayout{(size_t)nch * n * sf::SVM_W, (size_t)nch * ns * sf::GRAM_TILE, (size_t)(nch * sf::SVM_W) * (nch * sf::SVM_W)};
}

// the store for nch chunks: allocated or grown here; a failure leaves the plan (and a smaller store) as it was
int gram_store(sf_chol_plan* p, int64_t nch) {
    if (p->d_gram && p->gram_chunks >= nch) return SF_OK;
    const GramLayout L = gram_layout(p->n, nch);
    const size_t count = L.y + L.part + L.g;
    sf::DevMem<double> fresh;
    if (int rc = fresh.alloc(count)) return rc;
    p->d_gram = std::move(fresh);       // (frees the smaller store: every call returns with its work complete, nothing still reads it)
    p->gram_chunks = nch;
    p->bytes_gram = count * sizeof(double);
    return SF_OK;
}

// B (host, dev == false; device otherwise, pin = the ordering for the way in or null) -> G.  Host: G is the caller's array, filled
// from the store's result block; device: the final kernel writes the caller's dG itself.
int gram_run(sf_chol_plan* p, bool dev, const int32_t* pin, sf_long k, const double* B, sf_long ldb, double* G, sf_long ldg) {
    hipStream_t st = p->stream;
    const int64_t n = p->n;
    const SfCols src{const_cast<double*>(B), ldb, dev, pin};
    SfStretch t{p};
    if (k == 1) {
        // the one-column family on d_x and quadform's reduction
        if (int rc = sf_quadform_scratch(p)) return rc;
        const double* d_q = p->d_qf + (size_t)sf::QF_MAXB;
        if (int rc = sf_apply_chunks(
                p, SfApply{&src, nullptr, 1, 1, p->d_x, 0, true}, t,
                [&](double* x, sf_long, int) {
                    if (int rc = sf_apply_sweep(p, SF_SWEEP_FWD_L, x, 1, false)) return rc;
                    sf::launch_quadform(x, n, 1, p->d_qf, st);
                    return SF_OK;
                },
                [&](double*, sf_long, int) {
                    HIP_TRY(hipMemcpyAsync(G, d_q, sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
                    return SF_OK;
                }))
            return rc;
        p->last_gram_ms = t.total_ms;
        p->last_gram_parts = 0;
        return SF_OK;
    }
    const int W = sf::SVM_W;
    const int64_t nch = (k + W - 1) / W;
    if (!dev)
        if (int rc = sf_solve_many_block(p)) return rc;     // (its staging half takes the chunks of a host block)
    if (int rc = gram_store(p, nch)) return rc;
    const GramLayout L = gram_layout(n, p->gram_chunks);
    double* Y = p->d_gram;
    double* part = Y + L.y;
    double* Gd = dev ? G : part + L.part;
    const int64_t ldgd = dev ? ldg : k;
    // chunk c into its own block of the store, its row of G as soon as it has been swept
    if (int rc = sf_apply_chunks(p, SfApply{&src, nullptr, k, W, Y, (size_t)n * W, true}, t, [&](double* Yc, sf_long j0, int) {
            if (int rc = sf_apply_sweep(p, SF_SWEEP_FWD_L, Yc, W, false)) return rc;
            sf::launch_gram_row(Y, n, (int)(j0 / W), k, part, Gd, ldgd, st);
            return SF_OK;
        }))
        return rc;
    if (!dev) {
        HIP_TRY(hipMemcpy2DAsync(G, (size_t)ldg * sizeof(double), Gd, (size_t)k * sizeof(double), (size_t)k * sizeof(double), k,
                                 hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    int64_t slab_rows = 0;
    p->last_gram_parts = sf::gram_slabs(n, &slab_rows);
    p->last_gram_ms = t.total_ms;
    return SF_OK;
}

// the checks both entry points share once their pointers are known to be there: the arguments first, then the plan
int gram_args(sf_chol_plan* p, sf_long k, sf_long ldb, sf_long ldg) {
    if (k < 0 || k > SF_GRAM_MAX_K) return SF_ERR_ARG;
    if (ldb < std::max<sf_long>(p->n, 1) || ldg < std::max<sf_long>(k, 1)) return SF_ERR_ARG;
    if (p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    return SF_OK;
}

}  // namespace

extern "C" {

int sf_chol_plan_gram(sf_chol_plan* p, sf_long k, const sf_float* B, sf_long ldb, sf_float* G, sf_long ldg) {
    if (!p || !B || !G) return SF_ERR_ARG;
    if (int rc = gram_args(p, k, ldb, ldg)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (k == 0) return SF_OK;
    if (p->n <= 0) {
        for (sf_long j = 0; j < k; ++j)
            for (sf_long i = 0; i < k; ++i) G[i + j * ldg] = 0.0;       // (n == 0: the empty sums)
        return SF_OK;
    }
    return gram_run(p, false, nullptr, k, B, ldb, G, ldg);
}

int sf_chol_plan_gram_device(sf_chol_plan* p, int flags, sf_long k, const sf_float* dB, sf_long ldb, sf_float* dG, sf_long ldg) {
    if (!p || !dB || !dG) return SF_ERR_ARG;
    if (flags & ~SF_DEV_PERM_IN) return SF_ERR_ARG;
    if (int rc = gram_args(p, k, ldb, ldg)) return rc;
    if (flags && !p->d_perm) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (k == 0) return SF_OK;
    const size_t span_b = sf_block_span(p->n, k, ldb), span_g = sf_block_span(k, k, ldg);
    if ((span_b && !sf_device_ptr_ok(p, dB, span_b)) || !sf_device_ptr_ok(p, dG, span_g)) return SF_ERR_ARG;
    if (sf_blocks_overlap(dG, span_g, dB, span_b)) return SF_ERR_ARG;      // the result overlaps the block
    if (p->n <= 0) {
        HIP_TRY(hipMemset2DAsync(dG, (size_t)ldg * sizeof(double), 0, (size_t)k * sizeof(double), k, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return SF_OK;
    }
    return gram_run(p, true, flags ? p->d_perm : nullptr, k, dB, ldb, dG, ldg);
}

}  // extern "C"
