// What the selected inversions of a Cholesky factor (sf_selinv.hip) and of an LU factor (sf_selinv_lu.hip) share: the addressing of
// Sigma(R,R) through the scatter problems' relative maps, the fp64 MFMA GEMM with its gathered operand, and the host side's unit
// schedule.  Included by those two files only.
#pragma once
#include <hip/hip_runtime.h>

#include "sf_plan_internal.h"

namespace sf {

typedef double double4_v __attribute__((ext_vector_type(4)));

// panel position q of J (q >= the unit's first R position) as the column of a Sigma(hi, q) read: base offset of the column in the
// arena and the relative-map offset that turns the panel position hi of J into a row position of that column's panel (SEL_OWN: J's
// own column, the row position is hi itself; a real offset map_off - i can be negative).  Lsxp: the panels' offsets in the arena
// (the device layout of the factor: Lsxp for a Cholesky plan, Xp for an LU plan)
struct SelCol { int64_t base; int64_t moff; };
constexpr int64_t SEL_OWN = INT64_MIN;

__device__ __forceinline__ SelCol sel_col(const SelUnit& u, int q, const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap,
                                          const int64_t* __restrict__ Lsip, const int32_t* __restrict__ Lsi, const int64_t* __restrict__ Lsxp,
                                          const SelPair* __restrict__ pairs) {
    SelCol c;
    if (q < u.ncol) {
        c.base = u.lx + (int64_t)q * u.nsrow;
        c.moff = SEL_OWN;
        return c;
    }
    // the scatter problem (J, a) whose rows start at the last pair start <= q
    int lo = 0, hi = u.npair - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pairs[u.pair0 + mid].i <= q) lo = mid; else hi = mid - 1;
    }
    const SelPair pr = pairs[u.pair0 + lo];
    const int32_t g = Lsi[u.rows + q];
    const int32_t a = SuperMap[g];
    c.base = Lsxp[a] + (int64_t)(g - Super[a]) * (Lsip[a + 1] - Lsip[a]);
    c.moff = pr.map_off - pr.i;
    return c;
}

__device__ __forceinline__ double sel_at(const SelCol& c, int hi, const int32_t* __restrict__ relmap, const double* __restrict__ S) {
    return S[c.base + (c.moff == SEL_OWN ? (int64_t)hi : (int64_t)relmap[c.moff + hi])];
}

// ---------------------------------------------------------------------------------------------------------------------------
// C (M x N, leading dimension ldc) = op(A) B (+ C when acc), B column-major K x N (ldb).  AM = 0: A column-major M x K (lda);
// AM = 1: A = X^T with X column-major K x M (lda); AM = 2: A = Sigma(R,R) of unit u, gathered (M = K = |R|): entry (x, y) from S in
// column y's panel when x >= y, from S2 in column x's panel otherwise (Cholesky: S2 = S, the mirror; LU: (S, S2) = (SL, SU) gives
// Sigma(R,R) and (SU, SL) its transpose).  Workgroup (bx, by, z): the 64 x 64 tile (bx, by) over the K slab
// [z kslab, (z + 1) kslab), written to C + z cstride.  Four waves (2 x 2), each a 32 x 32 sub-tile = 2 x 2
// v_mfma_f64_16x16x4_f64 tiles; 16-deep K chunks staged in LDS.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SG_T = 64, SG_K = 16, SG_LD = SG_T + 4;

template <int AM>
__global__ void __launch_bounds__(256)
k_selinv_gemm(int M, int N, int K, const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
              double* __restrict__ C, int64_t ldc, int kslab, int64_t cstride, int acc_in, SelUnit u, const double* S, const double* S2,
              const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap, const int64_t* __restrict__ Lsip,
              const int32_t* __restrict__ Lsi, const int64_t* __restrict__ Lsxp, const SelPair* __restrict__ pairs,
              const int32_t* __restrict__ relmap) {
    __shared__ __attribute__((aligned(16))) double As[SG_K][SG_LD];
    __shared__ __attribute__((aligned(16))) double Bs[SG_K][SG_LD];
    __shared__ int64_t rbase[SG_T], rmoff[SG_T], kbase[SG_K], kmoff[SG_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, fr = lane & 15, fk = lane >> 4;
    const int m0 = blockIdx.x * SG_T, n0 = blockIdx.y * SG_T;
    const int k0 = blockIdx.z * kslab, k1 = min(K, k0 + kslab);
    C += (int64_t)blockIdx.z * cstride;
    const int ce = u.cb + u.w;
    if (AM == 2 && tid < SG_T && m0 + tid < M) {
        const SelCol c = sel_col(u, ce + m0 + tid, Super, SuperMap, Lsip, Lsi, Lsxp, pairs);
        rbase[tid] = c.base;
        rmoff[tid] = c.moff;
    }
    double4_v acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (double4_v){0.0, 0.0, 0.0, 0.0};
    for (int kc = k0; kc < k1; kc += SG_K) {
        __syncthreads();            // the previous chunk's reads are done (and, AM == 2, the row columns are in place)
        if (AM == 2 && tid < SG_K && kc + tid < k1) {
            const SelCol c = sel_col(u, ce + kc + tid, Super, SuperMap, Lsip, Lsi, Lsxp, pairs);
            kbase[tid] = c.base;
            kmoff[tid] = c.moff;
        }
        if (AM == 2) __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + 256 * r;
            int row, kk;
            if (AM == 1) { kk = e & 15; row = e >> 4; } else { row = e & 63; kk = e >> 6; }
            const int gi = m0 + row, gk = kc + kk;
            double v = 0.0;
            if (gi < M && gk < k1) {
                if (AM == 0) v = A[gi + (int64_t)gk * lda];
                else if (AM == 1) v = A[gk + (int64_t)gi * lda];
                else v = (gi >= gk) ? sel_at(SelCol{kbase[kk], kmoff[kk]}, ce + gi, relmap, S)
                                    : sel_at(SelCol{rbase[row], rmoff[row]}, ce + gk, relmap, S2);
            }
            As[kk][row] = v;
            const int bk = e & 15, bn = e >> 4;
            const int gn = n0 + bn, gbk = kc + bk;
            Bs[bk][bn] = (gn < N && gbk < k1) ? B[gbk + (int64_t)gn * ldb] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < SG_K / 4; ++s) {
            double a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = As[4 * s + fk][32 * wm + 16 * t + fr];
                b[t] = Bs[4 * s + fk][32 * wn + 16 * t + fr];
            }
#pragma unroll
            for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
        }
    }
    // D fragment: column lane & 15 (B side), rows (lane >> 4) + 4 r (A side)
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = m0 + 32 * wm + 16 * ta + fk + 4 * r, gn = n0 + 32 * wn + 16 * tb + fr;
                if (gi < M && gn < N) {
                    double* cp = C + gi + (int64_t)gn * ldc;
                    *cp = acc_in ? *cp + acc[ta][tb][r] : acc[ta][tb][r];
                }
            }
}

// the one place a product is launched from: launch_selinv_gemm (sf_selinv.hip) is a switch over these three, and the wide units of
// both plans call them directly (S, S2: the gathered operand's arenas, AM == 2 only)
template <int AM>
static inline void selinv_gemm(int M, int N, int K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                               int slabs, int64_t cstride, int acc_in, const SelUnit& u, const double* S, const double* S2, const SelStruct& t,
                               hipStream_t st) {
    if (M <= 0 || N <= 0) return;
    const int kslab = ((K + slabs - 1) / slabs + SG_K - 1) / SG_K * SG_K;
    const dim3 grid((M + 63) / 64, (N + 63) / 64, slabs);
    hipLaunchKernelGGL(k_selinv_gemm<AM>, grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C, ldc, kslab, cstride, acc_in, u, S, S2,
                       t.Super, t.SuperMap, t.Lsip, t.Lsi, t.Xp, t.pairs, t.relmap);
}

// the plan's structure arrays as the launchers take them
static inline SelStruct sel_struct(const sf_chol_plan* p) {
    return SelStruct{p->d_Super, p->d_SuperMap, p->d_Lsip, p->d_Lsi, p->lu ? p->d_Xp : p->d_Lsxp, p->d_sel_pairs, p->d_relmap};
}

}  // namespace sf

// ---- host side, defined in sf_selinv.hip ----
// a successful factorization of the plan's current values is on the device (a finished but unsynchronised one is collected here)
// the schedule (first call): units, pair table, scratch sizes, flops_selinv (an LU unit costs twice a Cholesky one)
int sf_selinv_schedule(sf_chol_plan* p);

// ---- the host driver both plans share ----
// The state of the first call: the arena (`arena` doubles), the diagonal, the narrow units, the pair table and the scratch of the
// wide units (`scratch` doubles).  A failure leaves the plan as it was.
static inline int sf_selinv_alloc(sf_chol_plan* p, size_t arena, size_t scratch) {
    if (p->d_sel) return SF_OK;
    const size_t ndiag = (size_t)std::max<int64_t>(p->n, 1), nunits = std::max<size_t>(p->sel_small.size(), 1), npairs = p->sel_pairs_h.size();
    sf::DevMem<double> sel, diag, scr;
    sf::DevMem<sf::SelUnit> units;
    sf::DevMem<sf::SelPair> pairs;
    if (sel.alloc(arena) || diag.alloc(ndiag) || units.alloc(nunits) || pairs.alloc(npairs) || scr.alloc(scratch)) return SF_ERR_ALLOC;
    if (!p->sel_small.empty()) HIP_TRY(hipMemcpy(units, p->sel_small.data(), nunits * sizeof(sf::SelUnit), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(pairs, p->sel_pairs_h.data(), npairs * sizeof(sf::SelPair), hipMemcpyHostToDevice));
    p->d_sel = std::move(sel);
    p->d_sel_diag = std::move(diag);
    p->d_sel_units = std::move(units);
    p->d_sel_pairs = std::move(pairs);
    p->d_sel_scratch = std::move(scr);
    p->bytes_selinv = (arena + ndiag + scratch) * sizeof(double) + nunits * sizeof(sf::SelUnit) + npairs * sizeof(sf::SelPair);
    return SF_OK;
}

// The selected inversion of a plan the entry point has accepted: the schedule and the allocations of a first call, then level by
// level the big units (big(unit, stream), in list order) and the level's narrow supernodes in one launch (small(units, count, stream)).
// scratch(): doubles of scratch, asked once the schedule is known.
template <class Scratch, class Big, class Small>
int sf_selinv_run(sf_chol_plan* p, size_t arena, Scratch&& scratch, Big&& big, Small&& small) {
    if (!sf_factor_current(p)) return SF_ERR_ARG;
    if (p->n <= 0) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    if (!p->sel_scheduled)
        if (int rc = sf_selinv_schedule(p)) return rc;
    if (int rc = sf_selinv_alloc(p, arena, scratch())) return rc;
    p->fs.selinv_started();
    hipStream_t st = p->stream;
    HIP_TRY(hipEventRecord(p->ev_s0, st));
    for (const auto& s : p->sel_steps) {
        for (int64_t k = s.big_first; k < s.big_first + s.big_count; ++k) big(p->sel_big[k], st);
        small(p->d_sel_units + s.small_first, (int)s.small_count, st);
    }
    HIP_TRY(hipEventRecord(p->ev_s1, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    if (elapsed_ms(&ms, p->ev_s0, p->ev_s1)) p->last_selinv_ms = ms;
    p->fs.selinv_finished();
    return SF_OK;
}

// diag(Sigma) of an accepted plan to the host, through `launch` (launch_selinv_diag or its LU twin)
static inline int sf_selinv_diag_run(sf_chol_plan* p, sf_float* d,
                                     void (*launch)(int64_t, const double*, const sf::SelStruct&, double*, hipStream_t)) {
    if (p->n <= 0) return SF_OK;
    if (!p->d_sel || !p->fs.selinv_matches()) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    launch((int64_t)p->n, p->d_sel, sf::sel_struct(p), p->d_sel_diag, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d, p->d_sel_diag, (size_t)p->n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SF_OK;
}
