// Hand-written gfx950 (CDNA4) kernels of the supernodal Cholesky / no-pivot LU numeric phase.
// Reference citations: C: = Cholesky/Source/SparseFrame.c, L: = LU/Source/SparseFrame.c, CK: = Cholesky/Source/cuda_kernel.cu.
//
//   k_load_panels   : SparseFrame_loadA (C:1998-2028, L:2478-2536) for ALL supernodes in one launch; the inverse row map
//                     (createMap, CK:22-30) is replaced by a binary search in the supernode's sorted row list.
//   k_potrf_block   : dpotrf_('L') on one <= 64x64 diagonal block, one wavefront, registers only   (C:2135, C:2766)
//   k_getrf_block   : no-pivot LU of the block (magma_dgetrf_nopiv L:2653, cusolverDnDgetrf/NULL L:3344), same scheme
//   k_trsm_block    : dtrsm_('R','L','C','N') of a row tile against that block (C:2142, C:2773); LU: D from the
//                     other panel, optional unit diagonal (L:2660)
//   k_gemm<mode>    : fp64 MFMA (v_mfma_f64_16x16x4_f64) C -= Y X^T on LDS-staged panels, persistent grid (tiles in rounds
//                     + stream-K remainder)
//       mode 0 : in-panel updates (the reference's blocked-potrf SYRK/GEMM, C:2854-2863)
//       mode 1 : Schur-complement update of an ancestor panel: dsyrk+dgemm (C:2061-2070; LU: L:2570-2577) with the
//                mapped scatter-subtract (mappedSubtract, CK:62-124; CPU loops C:2073-2086, L:2583-2604) fused into
//                the epilogue as native global_atomic_add_f64, lower trapezoid only
//   k_update_small  : the mode-1 update for K <= 64 (bottom-level supernodes): one wave per 64x32 tile, no LDS
//   k_build_relmaps : createRelativeMap (CK:42-60), once per plan for every (descendant, ancestor) pair
//   k_pack_lu       : gathers the device's (L, U^T) panel pairs into the reference's packed LU panels (L:2514-2517)
// (the fused 64-column step k_step<LU> -- update + POTRF / GETRF + TRSM in one launch -- lives in sf_step.hip, the device solve's
//  kernels, k_solve_*, in sf_solve.hip; the one-wave panel arithmetic k_potrf_block / k_getrf_block share with the step in sf_panel.h)
//
// Wavefronts are 64 wide; all tilings below are written for that.
#include "sf_kernels.h"
#include <cstdlib>
#include "sf_panel.h"
#include "sf_wave.h"

namespace sf {

// position of `key` in the ascending array a[0..n); key is known to be present
__device__ __forceinline__ int lower_bound_i32(const int32_t* __restrict__ a, int n, int32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------------
// assemble: one lane per matrix column; A[(j-Super[s])*nsrow + pos(i)] = Lx[p]
// The panels were zeroed by a memset on the same stream.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_load_panels(const int64_t* __restrict__ Lp, const int32_t* __restrict__ Li, const double* __restrict__ Lx, int32_t n,
              const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap,
              const int64_t* __restrict__ Lsip, const int32_t* __restrict__ Lsi,
              const int64_t* __restrict__ Lsxp, double* __restrict__ Lsx, int skip_diag,
              const int8_t* __restrict__ load_mask) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t s = SuperMap[j];
    if (load_mask && !load_mask[s]) return;     // multi-GPU: panel not stored here, or loaded by another rank
    const int32_t c0 = Super[s], c1 = Super[s + 1];
    const int64_t r0 = Lsip[s];
    const int32_t nsrow = (int32_t)(Lsip[s + 1] - r0);
    const int32_t nscol = c1 - c0;
    double* col = Lsx + Lsxp[s] + (int64_t)(j - c0) * nsrow;
    const int32_t* below = Lsi + r0 + nscol;
    for (int64_t p = Lp[j]; p < Lp[j + 1]; ++p) {
        const int32_t i = Li[p];
        if (skip_diag && i == j) continue;
        const int32_t si = (i < c1) ? (i - c0) : nscol + lower_bound_i32(below, nsrow - nscol, i);
        col[si] = Lx[p];
    }
}

// The same walk once per plan, keeping where every entry goes (offset into Lsx, -1: not loaded) -- so that the assembly of every
// later factorization is one coalesced pass over the values and the map (k_load_mapped) instead of a binary search per entry in
// dependent loads: config 3 (n = 10^6, 10^7 entries) 0.46 -> 0.07 ms per factorization.
__global__ void __launch_bounds__(256)
k_build_loadmap(const int64_t* __restrict__ Lp, const int32_t* __restrict__ Li, int32_t n,
                const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap,
                const int64_t* __restrict__ Lsip, const int32_t* __restrict__ Lsi,
                const int64_t* __restrict__ Lsxp, int64_t base, int skip_diag, int64_t* __restrict__ map) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t s = SuperMap[j];
    const int32_t c0 = Super[s], c1 = Super[s + 1];
    const int64_t r0 = Lsip[s];
    const int32_t nsrow = (int32_t)(Lsip[s + 1] - r0);
    const int32_t nscol = c1 - c0;
    const int64_t col = base + Lsxp[s] + (int64_t)(j - c0) * nsrow;
    const int32_t* below = Lsi + r0 + nscol;
    for (int64_t p = Lp[j]; p < Lp[j + 1]; ++p) {
        const int32_t i = Li[p];
        if (skip_diag && i == j) { map[p] = -1; continue; }
        const int32_t si = (i < c1) ? (i - c0) : nscol + lower_bound_i32(below, nsrow - nscol, i);
        map[p] = col + si;
    }
}

__global__ void __launch_bounds__(256)
k_load_mapped(const double* __restrict__ Lx, const int64_t* __restrict__ map, int64_t nnz, double* __restrict__ Lsx) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = map[p];
        if (m >= 0) Lsx[m] = Lx[p];
    }
}

__global__ void __launch_bounds__(256)
k_loadmap_drop(const int64_t* __restrict__ drop, int64_t count, int64_t* __restrict__ map) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (int64_t)gridDim.x * blockDim.x) map[drop[k]] = -1;
}

void launch_loadmap_drop(const int64_t* drop, int64_t count, int64_t* map, hipStream_t st) {
    if (count <= 0) return;
    const int64_t blocks = std::min<int64_t>((count + 255) / 256, 1024);
    hipLaunchKernelGGL(k_loadmap_drop, dim3((unsigned)blocks), dim3(256), 0, st, drop, count, map);
}

void launch_build_loadmap(const int64_t* Lp, const int32_t* Li, int32_t n, const int32_t* Super, const int32_t* SuperMap,
                          const int64_t* Lsip, const int32_t* Lsi, const int64_t* Lsxp, int64_t base, int skip_diag, int64_t* map, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_build_loadmap, dim3((n + 255) / 256), dim3(256), 0, st, Lp, Li, n, Super, SuperMap, Lsip, Lsi, Lsxp, base, skip_diag, map);
}

void launch_load_mapped(const double* Lx, const int64_t* map, int64_t nnz, double* Lsx, hipStream_t st) {
    if (nnz <= 0) return;
    const int64_t blocks = std::min<int64_t>((nnz + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_load_mapped, dim3((unsigned)blocks), dim3(256), 0, st, Lx, map, nnz, Lsx);
}

void launch_load_panels(const int64_t* Lp, const int32_t* Li, const double* Lx, int32_t n,
                        const int32_t* Super, const int32_t* SuperMap, const int64_t* Lsip, const int32_t* Lsi,
                        const int64_t* Lsxp, double* Lsx, int skip_diag, const int8_t* load_mask, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_load_panels, dim3((n + 255) / 256), dim3(256), 0, st,
                       Lp, Li, Lx, n, Super, SuperMap, Lsip, Lsi, Lsxp, Lsx, skip_diag, load_mask);
}

// ---------------------------------------------------------------------------------------------------
// Cholesky of a b x b (b <= 64) diagonal block, lower.  ONE wavefront per block, no LDS, no barrier:
// lane r keeps row r of the block in registers (a[c] = A(r,c)); at step j the pivot and the multipliers
// l(c,j) are broadcast out of lane j / lane c with v_readlane (the lane index is a compile-time
// constant after unrolling, so the broadcast lands in SGPRs and feeds v_fma_f64 directly).
// Rows/columns beyond b are padded with the identity.  (rsqrt_full and the other one-wave panel arithmetic: sf_panel.h)
// ---------------------------------------------------------------------------------------------------
// W = the smallest of 8 / 16 / 32 / 64 that holds the block: the elimination is fully unrolled over W columns (registers), and
// at the bottom levels of a 2-D problem most blocks have a handful of columns -- with W = 64 for all, a 3-column block cost the
// 2,016 FMAs + 4,032 v_readlane of a 64-column one (config 3: 21,000 such blocks = 0.30 ms, compute-bound on padding)
template <int W>
__device__ __forceinline__ void potrf_block_w(const PotrfTask& t, double* __restrict__ Lsx, int* __restrict__ info) {
    double* A = Lsx + t.panel + t.diag + (int64_t)t.diag * t.ld;
    const int b = t.b;
    const int lane = threadIdx.x;
    const int64_t ld = t.ld;

    double a[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = (c == lane) ? 1.0 : 0.0;
        if (lane < b && c <= lane) v = A[lane + c * ld];
        a[c] = v;
    }
    bool bad = false;
    double dnext = a[0];        // the next column's diagonal entry, formed in its own lane (see step_diag_chol's panel, sf_step.hip)
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const double djj = readlane_f64(dnext, j);
        bad = bad || !(djj > 0.0);          // also catches NaN; padded rows have djj = 1
        // 1/sqrt(djj) from v_rsq_f64 + one third-order step (rsqrt_full), the column scaled by it: the IEEE sqrt and divide sequences
        // are ~10x longer and sit on the sequential critical path.  Every lane multiplies: lane j's own entry IS djj, so it gets
        // djj / sqrt(djj) = the diagonal without a select; lanes above the diagonal carry values nobody reads (they only ever feed
        // other entries above the diagonal, and the store below keeps to the lower triangle)
        const double rinv = rsqrt_full(djj);
        const double lj = a[j] * rinv;
        a[j] = lj;
        if (j + 1 < W) dnext = __builtin_fma(-lj, lj, a[j + 1]);
#pragma unroll
        for (int c = j + 1; c < W; ++c) a[c] = __builtin_fma(-lj, readlane_f64(lj, c), a[c]);
    }
    if (bad && lane == 0) atomicOr(info, 1);
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (lane < b && c <= lane) A[lane + c * ld] = a[c];
}

__global__ void __launch_bounds__(64)
k_potrf_block(const PotrfTask* __restrict__ tasks, double* __restrict__ Lsx, int* __restrict__ info) {
    const PotrfTask t = tasks[blockIdx.x];
    if (t.b <= 8) potrf_block_w<8>(t, Lsx, info);
    else if (t.b <= 16) potrf_block_w<16>(t, Lsx, info);
    else if (t.b <= 32) potrf_block_w<32>(t, Lsx, info);
    else potrf_block_w<NB>(t, Lsx, info);
}

void launch_potrf(const PotrfTask* tasks, int ntasks, double* Lsx, int* info, hipStream_t st) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_potrf_block, dim3(ntasks), dim3(64), 0, st, tasks, Lsx, info);
}

// ---------------------------------------------------------------------------------------------------
// LU of a b x b (b <= 64) diagonal block in ONE wavefront: getrf_panel_wave (sf_panel.h, see there for the scheme and the implicit
// interchanges) on the whole block, W = the block's width class.
// ---------------------------------------------------------------------------------------------------
// The block lives in two panels: D(r,c), c < r (L, unit diagonal implied) in the L panel at (diag+r, diag+c); D(r,c), c >= r
// (U) in the U^T panel at (diag+c, diag+r).
template <int W>
__device__ __forceinline__ void getrf_block_w(const PotrfTask& t, double* __restrict__ Lsx, int64_t u_shift, int* __restrict__ info, const PivotCtl& pc) {
    double* PLd = Lsx + t.panel + t.diag + (int64_t)t.diag * t.ld;
    double* PUd = PLd + u_shift;
    const int b = t.b;
    const int lane = threadIdx.x;
    const int64_t ld = t.ld;

    double a[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double v = (c == lane) ? 1.0 : 0.0;
        if (lane < b && c < b) v = (c < lane) ? PLd[lane + c * ld] : PUd[c + lane * ld];
        a[c] = v;
    }
    bool bad = false, active = lane < b;
    int np = 0, pos = lane;
    getrf_panel_wave<false, W>(a, lane, 0, b, pc.tol, pc.eps, bad, np, pos, active, nullptr);
    if (bad && lane == 0) atomicOr(info, 1);
    if (np > 0 && lane == 0) atomicAdd(pc.nperturb, np);
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (lane < b && c < b) {
            if (c < pos) PLd[pos + c * ld] = a[c]; else PUd[c + pos * ld] = a[c];
        }
    }
    if (pc.pivpos && lane < b) {
        const int g0 = t.first_col + t.diag;
        pc.pivpos[g0 + lane] = g0 + pos;
        pc.pivinv[g0 + pos] = g0 + lane;
    }
}

// width-specialised like k_potrf_block
__global__ void __launch_bounds__(64)
k_getrf_block(const PotrfTask* __restrict__ tasks, double* __restrict__ Lsx, int64_t u_shift, int* __restrict__ info, PivotCtl pc) {
    const PotrfTask t = tasks[blockIdx.x];
    if (t.b <= 8) getrf_block_w<8>(t, Lsx, u_shift, info, pc);
    else if (t.b <= 16) getrf_block_w<16>(t, Lsx, u_shift, info, pc);
    else if (t.b <= 32) getrf_block_w<32>(t, Lsx, u_shift, info, pc);
    else getrf_block_w<NB>(t, Lsx, u_shift, info, pc);
}

void launch_getrf(const PotrfTask* tasks, int ntasks, double* Lsx, int64_t u_shift, int* info, PivotCtl pc, hipStream_t st) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_getrf_block, dim3(ntasks), dim3(64), 0, st, tasks, Lsx, u_shift, info, pc);
}

// ---------------------------------------------------------------------------------------------------
// LU download: thread per value of the reference layout; supernode found by binary search in RefXp.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pack_lu(const int32_t* __restrict__ Super, const int64_t* __restrict__ Lsip, const int64_t* __restrict__ Xp,
          const int64_t* __restrict__ RefXp, int32_t nsuper, const double* __restrict__ PL, const double* __restrict__ PU,
          double* __restrict__ out, int64_t e_begin, int64_t e_end) {
    // values [e_begin, e_end) of the reference layout -> out[0 .. e_end - e_begin)
    for (int64_t e = e_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < e_end; e += (int64_t)gridDim.x * blockDim.x) {
        double* __restrict__ dst = out + (e - e_begin);
        int lo = 0, hi = nsuper;            // largest s with RefXp[s] <= e
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (RefXp[mid] <= e) lo = mid; else hi = mid;
        }
        const int s = lo;
        if (Xp[s] < 0) { *dst = 0.0; continue; }      // sharded plan: the panel lives on another rank
        const int64_t nscol = Super[s + 1] - Super[s], nsrow = Lsip[s + 1] - Lsip[s];
        const int64_t lda = 2 * nsrow - nscol;
        const int64_t off = e - RefXp[s];
        const int64_t j = off / lda, R = off % lda;
        const double* pl = PL + Xp[s] + j * nsrow;       // column j of the L panel
        double v;
        if (R < nscol) v = (R > j) ? pl[R] : PU[Xp[s] + j + R * nsrow];          // packed L11 \ U11: U(R,j) = PU(j,R)
        else if (R < nsrow) v = pl[R];                                             // L21
        else v = PU[Xp[s] + (R - nsrow + nscol) + j * nsrow];                      // U12^T
        *dst = v;
    }
}

void launch_pack_lu(const int32_t* Super, const int64_t* Lsip, const int64_t* Xp, const int64_t* RefXp, int32_t nsuper,
                    const double* PL, const double* PU, double* out, int64_t e_begin, int64_t e_end, hipStream_t st) {
    if (e_end <= e_begin) return;
    const int64_t blocks = (e_end - e_begin + 255) / 256;
    hipLaunchKernelGGL(k_pack_lu, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st,
                       Super, Lsip, Xp, RefXp, nsuper, PL, PU, out, e_begin, e_end);
}

// ---------------------------------------------------------------------------------------------------
// Fingerprint of the factor as the HOST sees it (reference layout), one 64-bit word per supernode:
//   H[s] = sum over the values e of panel s of  bits(v_e) * (2 e + 1) * K   (mod 2^64),  e = index in the reference layout.
// Order-independent (a sum), position-dependent (odd multiplier per index), a changed value always changes it, zeros add nothing.
// The struct path's solve compares it with the same sum over the caller's host array before it trusts the resident factor
// (sf_handlers.hip).  A workgroup walks a contiguous range of `chunk` values; a thread keeps the supernode of its current value
// (monotone walk) and flushes its partial sum when the supernode changes.  LU: the value is gathered from the (L, U^T) panel pair
// exactly as k_pack_lu does, so the result does not depend on which block columns k_lu_fill_u11 has touched.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_factor_hash(const int32_t* __restrict__ Super, const int64_t* __restrict__ Lsip, const int64_t* __restrict__ Xp,
              const int64_t* __restrict__ RefXp, int32_t nsuper, const double* __restrict__ PL, const double* __restrict__ PU, int lu,
              int64_t total, int64_t chunk, unsigned long long* __restrict__ H) {
    const int64_t begin = (int64_t)blockIdx.x * chunk, end = min(begin + chunk, total);
    if (begin >= end) return;               // (whole workgroup)
    const bool idle = begin + threadIdx.x >= end;           // last chunk: these threads add nothing but join the barriers below
    int64_t e = idle ? end - 1 : begin + threadIdx.x;
    int lo = 0, hi = nsuper;                // largest s with RefXp[s] <= e
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (RefXp[mid] <= e) lo = mid; else hi = mid;
    }
    int s = lo;
    unsigned long long acc = 0;
    int64_t s_end = RefXp[s + 1], s_beg = RefXp[s], xp = Xp[s];
    int64_t nscol = Super[s + 1] - Super[s], nsrow = Lsip[s + 1] - Lsip[s];
    if (idle) e = end;                      // nothing to add; stays for the barriers below
    for (; e < end; e += 256) {
        if (e >= s_end) {
            if (acc) atomicAdd(&H[s], acc);
            acc = 0;
            while (e >= RefXp[s + 1]) ++s;
            s_end = RefXp[s + 1]; s_beg = RefXp[s]; xp = Xp[s];
            nscol = Super[s + 1] - Super[s]; nsrow = Lsip[s + 1] - Lsip[s];
        }
        if (xp < 0) {                       // not stored on this rank: on to this thread's first value behind the panel
            e += ((s_end - e + 255) / 256 - 1) * 256;
            continue;
        }
        const int64_t off = e - s_beg;
        double v;
        if (!lu) {
            v = PL[xp + off];
        } else {
            const int64_t lda = 2 * nsrow - nscol;
            const int64_t j = off / lda, R = off % lda;
            if (R < nscol) v = (R > j) ? PL[xp + j * nsrow + R] : PU[xp + j + R * nsrow];
            else if (R < nsrow) v = PL[xp + j * nsrow + R];
            else v = PU[xp + (R - nsrow + nscol) + j * nsrow];
        }
        acc += (unsigned long long)__double_as_longlong(v) * ((2ull * (unsigned long long)e + 1ull) * 0x9E3779B97F4A7C15ull);
    }
    // end of the chunk: inside a big panel all 256 threads hold partial sums of ONE supernode -- one atomic per workgroup instead of
    // 256 on the same word (the root panel alone would otherwise take 59 M serialised atomics); mixed workgroups add per thread
    __shared__ int s_first;
    __shared__ unsigned long long s_part[4];
    if (threadIdx.x == 0) s_first = s;
    __syncthreads();
    const bool uniform = __syncthreads_and(s == s_first) != 0;
    if (!uniform) { if (acc) atomicAdd(&H[s], acc); return; }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        if (tot) atomicAdd(&H[s], tot);
    }
}

void launch_factor_hash(const int32_t* Super, const int64_t* Lsip, const int64_t* Xp, const int64_t* RefXp, int32_t nsuper,
                        const double* PL, const double* PU, int lu, int64_t total, unsigned long long* H, hipStream_t st) {
    if (total <= 0 || nsuper <= 0) return;
    const int64_t chunk = 256 * 64;
    const int64_t blocks = (total + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_factor_hash, dim3((unsigned)blocks), dim3(256), 0, st, Super, Lsip, Xp, RefXp, nsuper, PL, PU, lu, total, chunk, H);
}

__global__ void __launch_bounds__(256)
k_lu_fill_u11(const FillTile* __restrict__ tiles, double* __restrict__ PL, const double* __restrict__ PU) {
    __shared__ double tile[64][65];
    const FillTile t = tiles[blockIdx.x];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int jlo = max(t.c0, t.cb), jhi = min(t.c0 + 64, t.ce);
    {
        const int j = t.c0 + tx;                    // consecutive lanes: consecutive rows of the U^T panel
        for (int rr = ty; rr < 64; rr += 4) {
            const int R = t.r0 + rr;
            if (j >= jlo && j < jhi && R <= j) tile[rr][tx] = PU[t.xp + j + (int64_t)R * t.nsrow];
        }
    }
    __syncthreads();
    {
        const int R = t.r0 + tx;                    // consecutive lanes: consecutive rows of the L panel
        for (int jj = ty; jj < 64; jj += 4) {
            const int j = t.c0 + jj;
            if (j >= jlo && j < jhi && R <= j) PL[t.xp + R + (int64_t)j * t.nsrow] = tile[tx][jj];
        }
    }
}

void launch_lu_fill_u11(const FillTile* tiles, int64_t ntiles, double* PL, const double* PU, hipStream_t st) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(k_lu_fill_u11, dim3((unsigned)ntiles), dim3(256), 0, st, tiles, PL, PU);
}

// ---------------------------------------------------------------------------------------------------
// X <- X * D^{-T} for a tile of rows, D = lower-triangular b x b block already factored.
// One row per lane (rows are contiguous in memory: coalesced 8-byte accesses per column).
// The row is solved 8 columns at a time: the 8 running sums live in registers, the contributions of
// the columns already solved are re-read from the panel (the lane's own earlier stores, L2-resident)
// and D is broadcast from LDS, transposed so that the 8 multipliers of one k are 64 contiguous bytes.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TRSM_ROWS)
k_trsm_block(const TrsmTask* __restrict__ tasks, double* __restrict__ Lsx, const int32_t* __restrict__ pivinv) {
    __shared__ __attribute__((aligned(16))) double Dt[NB][NB];   // Dt[k][j] = L(j,k) for k < j, else 0
    __shared__ double Dinv[NB];
    const TrsmTask t = tasks[blockIdx.x];
    const double* Dg = Lsx + t.dpanel + t.diag + (int64_t)t.diag * t.ld;
    const int b = t.b;
    const int tid = threadIdx.x;

    // (columns k >= b are never multiplied with: a 3-column panel of the bottom levels fills 3 x 64 entries, not 64 x 64 -- config 3 has
    //  26,000 such panels; the entries Dt[k][j >= b] only reach sums that are not stored)
    for (int e = tid; e < b * NB; e += (int)blockDim.x) {
        const int k = e / NB, j = e % NB;   // column k, row j of the block: coalesced along j
        Dt[k][j] = (j < b && k < j) ? Dg[j + (int64_t)k * t.ld] : 0.0;
    }
    if (tid < NB) Dinv[tid] = (tid < b && !t.unit) ? 1.0 / Dg[tid + (int64_t)tid * t.ld] : 1.0;
    __syncthreads();

    if (tid >= t.nrows) return;
    double* X = Lsx + t.panel + t.row0 + tid + (int64_t)t.diag * t.ld;
    const int64_t ld = t.ld;
    if (pivinv && t.unit) {
        // LU with pivoting: these are rows of U^T, i.e. the tile's columns are the block's rows of U -- bring them into
        // pivot order first (column at position p <- original column pivinv[p]); all loads precede the stores
        const int g0 = t.first_col + t.diag;
        const int32_t* pv = pivinv + g0;
        double tmp[NB];
#pragma unroll
        for (int c = 0; c < NB; ++c) tmp[c] = X[(int64_t)(pv[min(c, b - 1)] - g0) * ld];
#pragma unroll
        for (int c = 0; c < NB; ++c)
            if (c < b) X[(int64_t)c * ld] = tmp[c];
    }

    for (int jb = 0; jb < b; jb += 8) {
        double acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = X[min(jb + u, b - 1) * ld];      // unconditional, clamped: 8 loads in flight
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = (jb + u < b) ? acc[u] : 0.0;
        for (int k0 = 0; k0 < jb; k0 += 8) {       // jb is a multiple of 8: 8 independent re-reads in flight per round trip
            double xk[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) xk[v] = X[(k0 + v) * ld];
#pragma unroll
            for (int v = 0; v < 8; ++v)
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] -= xk[v] * Dt[k0 + v][jb + u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int v = 0; v < u; ++v) acc[u] -= acc[v] * Dt[jb + v][jb + u];
            acc[u] *= Dinv[jb + u];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (jb + u < b) X[(jb + u) * ld] = acc[u];
    }
}

// (64-thread workgroups for launches whose tiles have at most 64 rows -- the bottom levels -- were measured: SLOWER, 0.47 against
// 0.395 ms on config 3: the block's fill is what the other three waves are for)
void launch_trsm(const TrsmTask* tasks, int ntasks, double* Lsx, const int32_t* pivinv, hipStream_t st) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_trsm_block, dim3(ntasks), dim3(TRSM_ROWS), 0, st, tasks, Lsx, pivinv);
}

// ---------------------------------------------------------------------------------------------------
// fp64 MFMA GEMM  C[ci][cj] -= sum_k Y[ci][k] X[cj][k]   (lower trapezoid ci >= cj)
//
// Workgroup = 8 waves (2 x 4), tile 128 (ci) x 128 (cj), K step 16 in two LDS buffers, which the LDS-DMA loop uses as a ring
// of four 8-deep stages.  Each wave owns a 64 x 32 sub-tile = 4 x 2 MFMA tiles of v_mfma_f64_16x16x4_f64:
//     A operand (row index of D)  <- X rows (cj)      lane l: X[cj = l&15][k = l>>4]
//     B operand (col index of D)  <- Y rows (ci)      lane l: Y[ci = l&15][k = l>>4]
//     D[row = (l>>4) + 4*reg][col = l&15]             (f64 layout: NOT the f32 one)
// so that the 16 consecutive lanes of a quarter-wave hold 16 consecutive TARGET ROWS (ci), which are
// contiguous in the column-major target panel: the epilogue's atomics / stores hit 128-byte runs.
// LDS image of an operand tile: [k][row] with the row stride padded to 144 doubles, which makes the
// ds_read_b64 fragment reads (16 rows x 2 k per half-wave) hit all 64 banks exactly once.
// ---------------------------------------------------------------------------------------------------
constexpr int LDS_LD = GEMM_BM + 16;
constexpr int GEMM_SK = GEMM_BK / 2;    // depth of one stage of k_gemm's LDS-DMA ring (private to the kernel; a K step is two stages)
#ifndef SF_GEMM_MIN_UNITS_DEFAULT
#define SF_GEMM_MIN_UNITS_DEFAULT 16     // 16-deep K steps; swept in round 4: config 3 11.20 -> 10.99 ms, config 5 and 128^3 unchanged (tools/experiments/gemm_min_units.sh)
#endif

// largest i in [0, n) with a[i] <= key   (a ascending, a[0] = 0 <= key)
__device__ __forceinline__ int last_le_u32(const uint32_t* __restrict__ a, int n, uint32_t key) {
    int lo = 0, hi = n;     // invariant: a[lo] <= key, (hi == n or a[hi] > key)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

// Persistent launch: the work of one launch is the list of (tile, 16-deep K step) units of all its tiles, in
// task order; kt_prefix[i] = number of units before tile i.  The grid is a fixed number of workgroups (2 per CU).
// Whole tiles are dealt out in rounds (workgroup `share` takes tile r G + share in round r -- see the kernel body for
// why that matters for the L2); what does not fill a round is split "stream-K" style: each workgroup takes one
// contiguous, equal share of the remaining units, so the chip stays full whatever the mix of tile counts and K
// lengths (no tail of half-empty rounds).  Every tile is combined into its target with fp64 atomics (a K range
// split between workgroups needs them anyway).
// DMA: the operand tiles go global -> LDS directly (global_load_lds_dwordx4, "LDS-DMA"): the [k][row] LDS image of one k is
// 128 doubles = 1 KiB = exactly what one wave instruction writes (lane l: rows 2l, 2l+1), and it is 1 KiB of one panel column in
// memory too.  No staging registers, no ds_write, no select instructions; a k beyond K reads the X operand from a page of
// zeros (a DMA cannot mask), rows beyond M / N read valid memory whose products only reach entries that are never stored.
__device__ double g_zero_page[GEMM_BM + 16];

// One LDS-DMA of 16 bytes per lane (1 KiB per wave) as inline asm: the builtin form makes hipcc wait vmcnt(0) before the NEXT
// ds_read (it cannot tell the DMA's LDS destination from the buffer being read), which exposes the whole memory latency once per
// K step; an asm statement is outside its s_waitcnt bookkeeping, so the DMA stays in flight until the explicit
// `s_waitcnt vmcnt(n)` in front of a barrier of the K loop.  (Untracked operations can only make hipcc's own counted waits
// stricter: vmcnt retires in order.)  M0 = the wave-uniform LDS byte address, saved and restored around the instruction.
// The source is a wave-uniform base (scalar registers) plus a 32-bit byte offset per lane: no 64-bit vector address arithmetic
// and no address registers per staged row.
__device__ __forceinline__ void glds16(const void* sbase, uint32_t voff, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(sbase), "v"(voff), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p);
}

#ifdef SF_EXP_TIMING            // tools/experiments/gemm_overhead.sh: per-tile time stamps of every workgroup (s_memtime)
__device__ unsigned long long* g_exp_stamps = nullptr;      // [workgroup][64 tiles][4]
void exp_set_stamps(unsigned long long* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_exp_stamps), &p, sizeof(p)); }
#define SF_STAMP(slot) do { if (tid == 0 && g_exp_stamps && exp_tile < 64) \
        g_exp_stamps[((size_t)blockIdx.x * 64 + exp_tile) * 4 + (slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SF_STAMP(slot) do { } while (0)
#endif

template <int MODE, bool DMA>
__global__ void __launch_bounds__(GEMM_THREADS, GEMM_WAVES / 2)
k_gemm(const GemmProb* __restrict__ probs, const GemmTask* __restrict__ tasks,
       const uint32_t* __restrict__ kt_prefix, int ntasks, uint32_t u_lo, uint32_t u_hi,
       double* __restrict__ Lsx, const int32_t* __restrict__ RelMap, int* __restrict__ ticket, int whole_tiles, uint32_t min_units) {
    __shared__ int s_claim;
    __shared__ __attribute__((aligned(16))) double Ys[2][GEMM_BK][LDS_LD];
    __shared__ __attribute__((aligned(16))) double Xs[2][GEMM_BK][LDS_LD];
    __shared__ int32_t rowmap[GEMM_BM];
    __shared__ int32_t colmap[GEMM_BN];

    constexpr int WCJ = GEMM_BN / (GEMM_WAVES / 2);     // columns (cj) per wave: 64 with 4 waves, 32 with 8
    constexpr int TMN = WCJ / 16;                         // MFMA tiles per wave along cj
    constexpr int SQ = GEMM_BK / GEMM_WAVES;              // staging passes per K step
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;            // wave (wm, wn) owns rows [64 wm, +64) x columns [WCJ wn, +WCJ)
    const int fr = lane & 15, fk = lane >> 4;
    const int swave = __builtin_amdgcn_readfirstlane(wave);                 // the wave's number in scalar registers (DMA addressing)
    const uint32_t lds_ys = lds_addr(&Ys[0][0][0]), lds_xs = lds_addr(&Xs[0][0][0]);

    // XCD-aware share: workgroups b, b+8, b+16 ... run on one XCD (one L2); give each XCD a contiguous
    // run of shares so that the tiles it works on at any time are neighbours (supertile order).
    // [u_lo, u_hi): the units of this launch that this device executes (the whole launch on one GPU; one rank's
    // share when the launch is split over the ranks of a sharded factorization -- the update is a sum, any split is valid)
    const uint32_t T = u_hi - u_lo;
    const uint32_t G = gridDim.x;
    const uint32_t xcd = blockIdx.x & 7;
    const uint32_t xcd_n = (G >> 3) + (xcd < (G & 7) ? 1u : 0u);                              // workgroups of this XCD
    const uint32_t xcd_base = xcd < (G & 7) ? xcd * ((G >> 3) + 1) : (G & 7) * ((G >> 3) + 1) + (xcd - (G & 7)) * (G >> 3);
    const uint32_t share = xcd_base + (blockIdx.x >> 3);
    // Whole tiles are dealt out in ROUNDS: in round r workgroup `share` takes tile t0 + r G + share, so the 64 workgroups
    // of an XCD (consecutive shares) work on 64 CONSECUTIVE tiles -- one supertile -- at the same time and march through K
    // together: each operand slice is fetched into that XCD's L2 once per round and re-used by the 8 tiles of its
    // row / column.  (Contiguous shares of ~16 tiles each, the plain stream-K split, put concurrently running
    // workgroups 16 tiles apart: no operand was ever shared, PMC FETCH_SIZE = the no-reuse byte count.)
    // What does not fill a round -- the partial tiles at the ends of a rank's unit window and the last < G tiles -- is
    // split by (tile, K step) units as before, so the tail is still balanced.
    (void)T;
    int t0 = last_le_u32(kt_prefix, ntasks + 1, u_lo);
    if (kt_prefix[t0] < u_lo) ++t0;
    const int t1 = last_le_u32(kt_prefix, ntasks + 1, u_hi);          // tiles [t0, t1) lie inside [u_lo, u_hi)
    // whole_tiles: every tile is multiplied over its full K range by ONE workgroup (the last round is partial, nothing is split by
    // units), so each target element receives exactly one addition from this launch and the result does not depend on the order
    // workgroups run in -- what a launch that several ranks execute redundantly needs (the ranks' copies must stay bit-identical)
    const int R = (t1 > t0) ? (int)(((uint32_t)(t1 - t0) + (whole_tiles ? G - 1 : 0)) / G) : 0;
    const uint32_t head_end = (R > 0) ? kt_prefix[t0] : u_hi;
    const uint32_t tail_beg = (R > 0 && !whole_tiles) ? kt_prefix[t0 + R * (int)G] : u_hi;

    // ticket != nullptr: the rounds are DYNAMIC -- the workgroups of an XCD claim the tiles of that XCD's slots (the same
    // tiles as in the static deal, so a supertile still shares one L2) from the XCD's counter in the order they get free; tiles of
    // different K (different source supernodes in one launch) no longer leave a workgroup idle while its neighbour works off a
    // round of long ones.  Head and tail are split statically as before.
    int ph = 0, rr = 0;
#ifdef SF_EXP_DEPHASE
    bool exp_dephased = false;
#endif
#ifdef SF_EXP_TIMING
    int exp_tile = 0;
    // per workgroup, behind the tile stamps: shader-clock and constant 100 MHz stamps at its first and last instruction
    if (tid == 0 && g_exp_stamps) {
        g_exp_stamps[(size_t)gridDim.x * 256 + blockIdx.x * 4 + 0] = __builtin_amdgcn_s_memtime();
        g_exp_stamps[(size_t)gridDim.x * 256 + blockIdx.x * 4 + 1] = wall_clock64();
    }
#endif
    for (;;) {
    uint32_t u, u_end;
    int ti;
    SF_STAMP(0);
    if (ph == 1) {
        uint32_t slot = share;
        if (ticket != nullptr && R > 0) {
            if (tid == 0) s_claim = __hip_atomic_fetch_add(ticket + xcd, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();                     // the barrier that ends a tile separates this read from the next claim
            const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane(s_claim);
            rr = (int)(c / xcd_n);
            slot = xcd_base + c % xcd_n;
        }
        if (rr >= R) { ph = 2; continue; }
        ti = t0 + rr * (int)G + (int)slot;
        ++rr;
        if (ti >= t1) continue;                 // (whole_tiles: the last round is partial)
        u = kt_prefix[ti];
        u_end = kt_prefix[ti + 1];
#ifdef SF_EXP_DEPHASE           // experiment (round 4): the second workgroup of every CU (blockIdx >= grid / 2: the dispatcher fills the CUs
        // round-robin) starts its first whole tile half a K loop late, so that the two co-resident workgroups do not sit in their
        // prologues and atomic epilogues -- no MFMA work -- at the same time for the rest of the launch
        if (!exp_dephased && blockIdx.x >= gridDim.x / 2) {
            const int naps = (int)(u_end - u) * SF_EXP_DEPHASE / 16;       // one s_sleep 127 = 8128 cycles; a 16-deep K step of two workgroups ~ 8.5k
            for (int i = 0; i < naps; ++i) __builtin_amdgcn_s_sleep(127);
        }
        exp_dephased = true;
#endif
    } else {
        const uint32_t ra = (ph == 0) ? u_lo : tail_beg, rb = (ph == 0) ? head_end : u_hi;
        // (a share of fewer than min_units K steps costs more in its epilogue -- a whole 128 x 128 tile of atomics, on elements that up
        //  to G / tiles other workgroups add to at the same time -- than it saves: small launches run on fewer workgroups instead)
        const uint32_t Ueq = (rb > ra) ? (rb - ra + G - 1) / G : 0, U = max(Ueq, min_units);
        // (when the floor applies only some workgroups get a share: take them round-robin over the XCDs -- blockIdx -- instead of
        //  XCD by XCD, or the first XCDs would do all the work)
        const uint32_t sh = (U > Ueq) ? blockIdx.x : share;
        if (rb <= ra || sh * U >= rb - ra) {
            if (ph == 0) { ph = 1; continue; }
            break;
        }
        u = ra + sh * U;
        u_end = min(rb, u + U);
        ti = last_le_u32(kt_prefix, ntasks + 1, u);
    }

    while (u < u_end) {
        const GemmTask tk = tasks[ti];
        const GemmProb pb = probs[tk.prob];
        const uint32_t tbase = kt_prefix[ti];
        const int nkt = (int)(kt_prefix[ti + 1] - tbase);
        const int kt0 = (int)(u - tbase);
        const int kt1 = min(nkt, kt0 + (int)(u_end - u));
        u += (uint32_t)(kt1 - kt0);
        ++ti;

        const int ci0 = tk.tm * GEMM_BM, cj0 = tk.tn * GEMM_BN;
        // the task covers the K steps [tk.kt0, tk.kt0 + nkt) of its tile: operand pointers and K are those of the slice
        const int M = pb.M, N = pb.N;
        const int lda = pb.lda;
        const int kfirst = (int)tk.kt0 * GEMM_BK;
        const int K = min(pb.K - kfirst, nkt * GEMM_BK);
        const double* __restrict__ Yg = Lsx + pb.y_off + ci0 + (int64_t)kfirst * lda;
        const double* __restrict__ Xg = Lsx + pb.x_off + cj0 + (int64_t)kfirst * lda;

        if (MODE == 1) {
            // relative map of this tile's rows/columns inside the target panel (precomputed once per plan)
            if (tid < GEMM_BM) {
                const int ci = ci0 + tid;
                rowmap[tid] = (ci < M) ? RelMap[pb.map_off + ci] : 0;
            } else if (tid < GEMM_BM + GEMM_BN) {
                const int cj = cj0 + (tid - GEMM_BM);
                colmap[tid - GEMM_BM] = (cj < N) ? RelMap[pb.map_off + cj] : 0;
            }
        }

        // global -> register staging: lane handles the ROW PAIR (2*(tid & 63), +1) for k = (tid >> 6) + GEMM_WAVES*q:
        // one 16-byte load and one ds_write_b128 per pair (a wave reads 128 consecutive rows = 1 KiB of one panel
        // column).  gfx950 services 16-byte global loads from 8-byte-aligned addresses (tools/unaligned_load_test.hip),
        // so no alignment of the panel offsets is required.  Loads are unconditional: rows are clamped to a valid
        // pair and k to K-1; the values of invalid rows / k are zeroed when they are staged into LDS.
        const int prow = 2 * (tid & 63), pk0 = tid >> 6;
        const bool y0_ok = (ci0 + prow) < M, y1_ok = (ci0 + prow + 1) < M;
        const bool x0_ok = (cj0 + prow) < N, x1_ok = (cj0 + prow + 1) < N;
        const double* __restrict__ yp = Yg + (y0_ok ? prow : 0);
        const double* __restrict__ xp = Xg + (x0_ok ? prow : 0);
        const uint32_t yoff = (y0_ok ? prow : 0) * (uint32_t)sizeof(double), xoff = (x0_ok ? prow : 0) * (uint32_t)sizeof(double);
        double2_t ry[DMA ? 1 : SQ], rx[DMA ? 1 : SQ];

        auto load_tile = [&](int k0) {
#pragma unroll
            for (int q = 0; q < SQ; ++q) {
                const int64_t off = (int64_t)min(k0 + pk0 + GEMM_WAVES * q, K - 1) * lda;
                ry[q] = *reinterpret_cast<const double2_t*>(yp + off);
                rx[q] = *reinterpret_cast<const double2_t*>(xp + off);
            }
        };
        auto store_tile = [&](int buf, int k0) {
#pragma unroll
            for (int q = 0; q < SQ; ++q) {
                const bool kin = (k0 + pk0 + GEMM_WAVES * q) < K;
                double2_t vy = ry[q], vx = rx[q];
                vy.x = (kin && y0_ok) ? vy.x : 0.0; vy.y = (kin && y1_ok) ? vy.y : 0.0;
                vx.x = (kin && x0_ok) ? vx.x : 0.0; vx.y = (kin && x1_ok) ? vx.y : 0.0;
                *reinterpret_cast<double2_t*>(&Ys[buf][pk0 + GEMM_WAVES * q][prow]) = vy;
                *reinterpret_cast<double2_t*>(&Xs[buf][pk0 + GEMM_WAVES * q][prow]) = vx;
            }
        };
        // DMA: one ring stage = GEMM_SK k rows = half a K step; wave `pk0` fills row pk0 of both operands (two 1 KiB DMAs per
        // stage and wave).  Stage (K step kt, half h) lives in rows [GEMM_SK h, +GEMM_SK) of buffer (kt - kt0) & 1.
        auto dma_stage = [&](int buf, int half, int kt) {
            const int kl = half * GEMM_SK + swave, k = kt * GEMM_BK + kl;
            const uint32_t slot = (uint32_t)((buf * GEMM_BK + kl) * LDS_LD) * (uint32_t)sizeof(double);
            const bool kin = k < K;                                     // wave-uniform, as are both source rows
            const double* ysrc = Yg + (int64_t)min(k, K - 1) * lda;
            const double* xsrc = kin ? Xg + (int64_t)k * lda : g_zero_page;
            glds16(ysrc, yoff, lds_ys + slot);
            glds16(xsrc, xoff, lds_xs + slot);
        };
        // the MFMA fragments of the 4-deep k group that starts at row `krow` of buffer `buf`
        auto read_frag = [&](double (&a)[TMN], double (&b)[4], int buf, int krow) {
#pragma unroll
            for (int t = 0; t < TMN; ++t) a[t] = Xs[buf][krow + fk][wn * WCJ + t * 16 + fr];
#pragma unroll
            for (int t = 0; t < 4; ++t) b[t] = Ys[buf][krow + fk][wm * 64 + t * 16 + fr];
        };

        // a wave whose 64x64 quadrant lies entirely outside the lower trapezoid does no MFMA work
        // (wave-uniform by construction; readfirstlane lets the compiler branch on it with the scalar unit)
        const int qci0 = ci0 + wm * 64, qcj0 = cj0 + wn * WCJ;
        const bool quad_active = __builtin_amdgcn_readfirstlane((int)((qci0 < M) && (qcj0 < N) && (qci0 + 63 >= qcj0))) != 0;

        double4_t acc[TMN][4];
#pragma unroll
        for (int a = 0; a < TMN; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};

        auto mma = [&](const double (&a)[TMN], const double (&b)[4]) {
#pragma unroll
            for (int tm = 0; tm < TMN; ++tm)
#pragma unroll
                for (int tn = 0; tn < 4; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
        };

        if constexpr (DMA) {
        // Software pipeline over a RING OF FOUR 8-deep stages (the two 16-deep buffers, each cut in halves), one barrier per
        // stage.  While stage s is multiplied, stage s+1 is complete in LDS, stage s+2 is landing and the DMAs of stage s+3 are
        // issued into the slot stage s-1 was read from.  The wait in front of the barrier that ends stage s is for this wave's
        // DMAs of stage s+2 only (vmcnt retires in order: the two DMAs of stage s+3 may stay in flight), so a DMA has two stage
        // times to land.  Because stage s+1 is visible to every wave before that barrier, the fragments of its first k group are
        // read during the last k group of stage s into a second set of fragment registers: the first MFMAs behind a barrier
        // issue without an LDS round trip.  The one barrier covers both hazards: every wave is done reading the slot that is
        // overwritten next, and every wave's DMAs into the stage after the next have landed.  k is accumulated in the same
        // order as by a 16-deep loop.  Nothing is staged beyond K step kt1 - 1: the wait is vmcnt(0) where nothing was issued.
        dma_stage(0, 0, kt0);
        dma_stage(0, 1, kt0);
        if (kt0 + 1 < kt1) {
            dma_stage(1, 0, kt0 + 1);
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();                    // stages 0 and 1 are complete
        SF_STAMP(1);
        // (the K steps are taken in pairs so that the buffer of every LDS access is a compile-time constant: all fragment reads
        //  are one base register per operand plus an immediate offset)
        if (quad_active) {
            double a0[TMN], b0[4], a1[TMN], b1[4];
            read_frag(a0, b0, 0, 0);
            auto k_step = [&](const int buf, int kt) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bool more = kt + 1 + h < kt1;
                    read_frag(a1, b1, buf, h * GEMM_SK + 4);
                    if (more) dma_stage(h ? buf : buf ^ 1, h ^ 1, kt + 1 + h);      // stage s+3
                    mma(a0, b0);
                    read_frag(a0, b0, h ? buf ^ 1 : buf, h ? 0 : GEMM_SK);         // first k group of stage s+1
                    mma(a1, b1);
                    if (more) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");     // stage s+2 has landed
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                }
            };
            int kt = kt0;
            for (; kt + 1 < kt1; kt += 2) {
                k_step(0, kt);
                k_step(1, kt + 1);
            }
            if (kt < kt1) k_step(0, kt);
        } else {
            for (int kt = kt0; kt < kt1; ++kt) {     // staging only, same barriers
                const int buf = (kt - kt0) & 1;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (kt + 1 + h < kt1) {
                        dma_stage(h ? buf : buf ^ 1, h ^ 1, kt + 1 + h);
                        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                    } else {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    __syncthreads();
                }
            }
        }
        } else {
        // Register staging, software pipeline with one barrier per K step: while step kt is multiplied out of LDS buffer `buf`,
        // the registers holding step kt+1 are written to the other buffer and re-filled with step kt+2 -- both in
        // the shadow of this wave's own MFMAs (an MFMA occupies the matrix pipe for 64 cycles after it issues).
        load_tile(kt0 * GEMM_BK);
        store_tile(0, kt0 * GEMM_BK);
        __syncthreads();
        SF_STAMP(1);
        load_tile((kt0 + 1) * GEMM_BK);
        int buf = 0;
        if (quad_active) {
            for (int kt = kt0; kt < kt1; ++kt) {
#pragma unroll
                for (int kk = 0; kk < GEMM_BK / 4; ++kk) {
                    double a[TMN], b[4];
                    read_frag(a, b, buf, kk * 4);
                    if (kk == 0) store_tile(buf ^ 1, (kt + 1) * GEMM_BK);
                    if (kk == 1) load_tile((kt + 2) * GEMM_BK);
                    mma(a, b);
                }
                __syncthreads();
                buf ^= 1;
            }
        } else {
            for (int kt = kt0; kt < kt1; ++kt) {     // staging only, same barriers
                store_tile(buf ^ 1, (kt + 1) * GEMM_BK);
                load_tile((kt + 2) * GEMM_BK);
                __syncthreads();
                buf ^= 1;
            }
        }
        }

        SF_STAMP(2);
#ifdef SF_EXP_SKIP_EPILOGUE      // ablation for tools/experiments/gemm_overhead.sh: one store per lane keeps the accumulators live
        if (quad_active) {
            double v = 0.0;
            for (int tm = 0; tm < TMN; ++tm) for (int tn = 0; tn < 4; ++tn) for (int r = 0; r < 4; ++r) v += acc[tm][tn][r];
            if (v == 12345.678) Lsx[pb.c_off] = v;
        }
#else
        if (quad_active) {
            double* __restrict__ Cg = Lsx + pb.c_off;
            const int64_t ldc = pb.ldc;
#pragma unroll
            for (int tm = 0; tm < TMN; ++tm) {
#pragma unroll
                for (int tn = 0; tn < 4; ++tn) {
                    const int lci = wm * 64 + tn * 16 + fr;
                    const int ci = ci0 + lci;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int lcj = wn * WCJ + tm * 16 + fk + 4 * r;
                        const int cj = cj0 + lcj;
                        if (ci < M && cj < N && ci >= cj + (pb.strict & 1)) {
                            const double v = acc[tm][tn][r];
                            if (MODE == 1) {
                                unsafeAtomicAdd(Cg + rowmap[lci] + (int64_t)colmap[lcj] * ldc, -v);
                            } else {
                                double* dst = Cg + ci + (int64_t)cj * ldc;
                                // always the atomic form: a plain read-modify-write makes every one of the lane's 32 loads a
                                // dependent round trip (wait, subtract, store); the atomic needs no return value (measured:
                                // 49.6 vs 46.3 TFLOP/s at K = 256, profiles/r01_g_gemm_microbench_8wave.txt)
                                unsafeAtomicAdd(dst, -v);
                            }
                        }
                    }
                }
            }
        }
#endif
        // the next tile re-uses the LDS buffers and the relative maps.  (A barrier that orders LDS only -- s_waitcnt lgkmcnt(0) +
        // s_barrier, letting the tile's atomics drain under the next claim -- measured neutral: 544.2 vs 543.1 ms at 128^3.)
        __syncthreads();
        SF_STAMP(3);
#ifdef SF_EXP_TIMING
        ++exp_tile;
        SF_STAMP(0);
#endif
    }
    if (ph == 2) break;
    if (ph == 0) ph = 1;
    }   // phases
#ifdef SF_EXP_TIMING
    if (tid == 0 && g_exp_stamps) {
        g_exp_stamps[(size_t)gridDim.x * 256 + blockIdx.x * 4 + 2] = __builtin_amdgcn_s_memtime();
        g_exp_stamps[(size_t)gridDim.x * 256 + blockIdx.x * 4 + 3] = wall_clock64();
    }
#endif
}

// ---------------------------------------------------------------------------------------------------
// Schur updates with a short inner dimension (K <= 64: the small supernodes of the bottom levels, tens of thousands
// of (descendant, ancestor) pairs of a few dozen rows each).  k_gemm's 128 x 128 tile per 8-wave workgroup spends
// ~8 us per such pair with 7 of its 8 waves idle; here ONE WAVE owns a 64 x 32 tile (4 x 2 MFMA tiles), loads its
// fragments straight from the source panel (no LDS, no barrier, up to 48 loads in flight) and scatters with the same
// relative maps and fp64 atomics.  4 independent tiles per 256-thread workgroup.
// (Measured variants: forcing 3 waves per SIMD / hoisting the relative-map loads made the compiler spill: 9.9 vs 7.7 ms.
// Round 4: PERSISTENT waves walking through chunks of 4 consecutive tiles with the next tile's descriptors prefetched, the map
// entries requested before the K loop and 4-step fragment batches (100 VGPRs + 64 AGPRs, 3 waves per SIMD) -- 7.94 vs 7.68 ms at
// 128^3, 1.65 vs 1.59 ms on config 3, 3.27 vs 3.06 ms on config 5 (gpurun_out r04_h / r04_i): the kernel is not bound by the
// per-tile latency chain but by its load and atomic instructions through the texture path -- 24 eight-byte loads per k-group and
// up to 32 atomics per lane and tile, nothing shared between waves.)
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_update_small(const GemmProb* __restrict__ probs, const GemmTask* __restrict__ tasks, int ntasks,
               double* __restrict__ Lsx, const int32_t* __restrict__ RelMap) {
    const int lane = threadIdx.x & 63;
    // uniform over the wave: say so, or the task, the problem and all address arithmetic live in VGPRs
    const int ti = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (ti >= ntasks) return;
    const GemmTask tk = tasks[ti];
    const GemmProb pb = probs[tk.prob];
    const int fr = lane & 15, fk = lane >> 4;
    const int ci0 = tk.tm * SU_TM, cj0 = tk.tn * SU_TN;
    const int M = pb.M, N = pb.N, K = pb.K;
    const int64_t lda = pb.lda;
    // fragment rows, clamped into the problem: values of rows beyond M / N only reach outputs that are not stored
    const double* __restrict__ yq[4];
    const double* __restrict__ xq[2];
#pragma unroll
    for (int q = 0; q < 4; ++q) yq[q] = Lsx + pb.y_off + min(ci0 + 16 * q + fr, M - 1);
#pragma unroll
    for (int q = 0; q < 2; ++q) xq[q] = Lsx + pb.x_off + min(cj0 + 16 * q + fr, N - 1);

    double4_t acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = (double4_t){0.0, 0.0, 0.0, 0.0};

    const int nkk = (K + 3) >> 2;
    for (int kk0 = 0; kk0 < nkk; kk0 += 8) {
        double fa[8][2], fb[8][4];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = 4 * (kk0 + kk) + fk;
            const int64_t off = (int64_t)min(k, K - 1) * lda;       // unconditional loads; k beyond K is zeroed in the A operand
#pragma unroll
            for (int q = 0; q < 2; ++q) fa[kk][q] = xq[q][off];
#pragma unroll
            for (int q = 0; q < 4; ++q) fb[kk][q] = yq[q][off];
#pragma unroll
            for (int q = 0; q < 2; ++q) fa[kk][q] = (k < K) ? fa[kk][q] : 0.0;
        }
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            if (kk0 + kk < nkk) {
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 4; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[kk][tm], fb[kk][tn], acc[tm][tn], 0, 0, 0);
            }
        }
    }

    double* __restrict__ Cg = Lsx + pb.c_off;
    const int64_t ldc = pb.ldc;
    const int32_t* __restrict__ rm = RelMap + pb.map_off;
    int32_t colm[2][4];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int r = 0; r < 4; ++r) colm[tm][r] = rm[min(cj0 + 16 * tm + fk + 4 * r, N - 1)];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
        const int ci = ci0 + 16 * tn + fr;
        const int32_t rowm = rm[min(ci, M - 1)];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cj = cj0 + 16 * tm + fk + 4 * r;
                if (ci < M && cj < N && ci >= cj + (pb.strict & 1))
                    unsafeAtomicAdd(Cg + rowm + (int64_t)colm[tm][r] * ldc, -acc[tm][tn][r]);
            }
    }
}

void launch_update_small(const GemmProb* probs, const GemmTask* tasks, int ntasks, double* Lsx, const int32_t* RelMap, hipStream_t st) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_update_small, dim3((ntasks + 3) / 4), dim3(256), 0, st, probs, tasks, ntasks, Lsx, RelMap);
}

// ---------------------------------------------------------------------------------------------------
// On-device validation (the device twin of SparseFrame_validate, C:3141-3266 / L:3702-3858): r = A x - b with the stored
// triangle(s) of P A P^T, then |r|_inf / (|A|_1 |x|_inf + |b|_inf).  One lane per column (row for U); the four maxima are
// taken with integer atomicMax on the bit patterns (non-negative doubles order like unsigned integers).
//   norms[0] = |r|_inf, [1] = |A|_1 (max column sum), [2] = |x|_inf, [3] = |b|_inf
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_resid_init(int32_t n, double* __restrict__ r, double* __restrict__ colsum, double* __restrict__ b_out) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double b = 1.0 + (double)i / (double)n;
    b_out[i] = b;
    r[i] = -b;
    colsum[i] = 0.0;
}

// sym != 0: (Lp, Li, Lx) is one triangle of a symmetric matrix, used for both (Cholesky; LU of a symmetric input);
// sym == 0: only its own entries (the L part by column of an unsymmetric matrix)
__global__ void __launch_bounds__(256)
k_resid_cols(const int64_t* __restrict__ Lp, const int32_t* __restrict__ Li, const double* __restrict__ Lx, int32_t n, int sym,
             const double* __restrict__ x, double* __restrict__ r, double* __restrict__ colsum) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double xj = x[j];
    double rj = 0.0, cj = 0.0;
    for (int64_t p = Lp[j]; p < Lp[j + 1]; ++p) {
        const int32_t i = Li[p];
        const double a = Lx[p];
        unsafeAtomicAdd(r + i, a * xj);
        cj += fabs(a);
        if (sym && i != j) {
            rj += a * x[i];
            unsafeAtomicAdd(colsum + i, fabs(a));
        }
    }
    if (rj != 0.0) unsafeAtomicAdd(r + j, rj);
    unsafeAtomicAdd(colsum + j, cj);
}

// U by ROW (unsymmetric LU): row i lists columns j >= i; the diagonal is already in the L part
__global__ void __launch_bounds__(256)
k_resid_urows(const int64_t* __restrict__ Up, const int32_t* __restrict__ Ui, const double* __restrict__ Ux, int32_t n,
              const double* __restrict__ x, double* __restrict__ r, double* __restrict__ colsum) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double ri = 0.0;
    for (int64_t p = Up[i]; p < Up[i + 1]; ++p) {
        const int32_t j = Ui[p];
        if (j == i) continue;
        ri += Ux[p] * x[j];
        unsafeAtomicAdd(colsum + j, fabs(Ux[p]));
    }
    if (ri != 0.0) unsafeAtomicAdd(r + i, ri);
}

// The maximum that KEEPS a NaN (fmax returns the other operand): a non-finite r_i or x_i -- a NaN that a factorization or solve
// kernel let through -- must not be reported as a perfect solve.  The bit pattern of fabs(NaN) orders above +Inf, so the integer
// atomicMax carries it into norms[] and the residual formed from them is NaN (Inf / Inf for an infinite x).  For non-negative
// finite operands the result is fmax's, bit for bit.
__device__ __forceinline__ double resid_max(double m, double v) { return (v > m || v != v) ? v : m; }

__global__ void __launch_bounds__(256)
k_resid_norms(int32_t n, const double* __restrict__ r, const double* __restrict__ colsum, const double* __restrict__ x,
              const double* __restrict__ b, unsigned long long* __restrict__ norms) {
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        m[0] = resid_max(m[0], fabs(r[i])); m[1] = resid_max(m[1], colsum[i]); m[2] = resid_max(m[2], fabs(x[i]));
        m[3] = resid_max(m[3], fabs(b[i]));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = m[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = resid_max(v, __shfl_down(v, off, 64));
        if ((threadIdx.x & 63) == 0) atomicMax(norms + k, (unsigned long long)__double_as_longlong(v));
    }
}

__global__ void k_noop() {}
// one empty launch: loads this library's code object onto the current device (the first launch of a process pays for that)
void launch_noop(hipStream_t st) { hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, st); }

void launch_residual(const int64_t* Lp, const int32_t* Li, const double* Lx, const int64_t* Up, const int32_t* Ui, const double* Ux,
                     int32_t n, const double* x, double* r, double* colsum, double* b, double* norms, hipStream_t st) {
    if (n <= 0) return;
    const int g = (n + 255) / 256;
    hipLaunchKernelGGL(k_resid_init, dim3(g), dim3(256), 0, st, n, r, colsum, b);
    hipLaunchKernelGGL(k_resid_cols, dim3(g), dim3(256), 0, st, Lp, Li, Lx, n, Up ? 0 : 1, x, r, colsum);
    if (Up) hipLaunchKernelGGL(k_resid_urows, dim3(g), dim3(256), 0, st, Up, Ui, Ux, n, x, r, colsum);
    hipLaunchKernelGGL(k_resid_norms, dim3(g < 1024 ? g : 1024), dim3(256), 0, st, n, r, colsum, x, b, (unsigned long long*)norms);
}

// relative map of every scatter problem: one workgroup per problem, lanes stride over its M source rows
__global__ void __launch_bounds__(256)
k_build_relmaps(const GemmProb* __restrict__ probs, const int32_t* __restrict__ Lsi, int32_t* __restrict__ RelMap) {
    const GemmProb pb = probs[blockIdx.x];
    for (int ci = threadIdx.x; ci < pb.M; ci += blockDim.x) {
        const int32_t g = Lsi[pb.src_rows + ci];
        RelMap[pb.map_off + ci] = (ci < pb.N) ? (g - pb.tgt_first_col)
                                              : pb.tgt_nscol + lower_bound_i32(Lsi + pb.tgt_rows, pb.tgt_nbelow, g);
    }
}

void launch_build_relmaps(const GemmProb* probs, int nprobs, const int32_t* Lsi, int32_t* RelMap, hipStream_t st) {
    if (nprobs > 0) hipLaunchKernelGGL(k_build_relmaps, dim3(nprobs), dim3(256), 0, st, probs, Lsi, RelMap);
}

void launch_gemm(const GemmProb* probs, const GemmTask* tasks, const uint32_t* kt_prefix, int ntasks, uint32_t u_lo, uint32_t u_hi,
                 int mode, double* Lsx, const int32_t* RelMap, int* ticket, hipStream_t st, int whole_tiles, int grid_cap) {
    if (ntasks <= 0 || u_hi <= u_lo) return;
    const uint32_t units = u_hi - u_lo;
    const uint32_t cap = (grid_cap > 0 && grid_cap < GEMM_GRID) ? (uint32_t)grid_cap : (uint32_t)GEMM_GRID;
    const uint32_t grid = units < cap ? units : cap;
    // LDS-DMA staging is the default (68.9 vs 67.4 TFLOP/s at 16k x 16k x 4k, 552 vs 554 ms at 128^3); SF_GEMM_DMA=0 selects the
    // register-staged form (read per launch: the tests flip it)
    static const uint32_t min_units = [] { const char* m = getenv("SF_GEMM_MIN_UNITS"); return (uint32_t)(m ? std::max(1, atoi(m)) : SF_GEMM_MIN_UNITS_DEFAULT); }();
    const char* e = sf_exp_env("SF_GEMM_DMA");
    const bool dma = e ? atoi(e) != 0 : true;
    if (dma) {
        if (mode == 1)
            hipLaunchKernelGGL((k_gemm<1, true>), dim3(grid), dim3(GEMM_THREADS), 0, st, probs, tasks, kt_prefix, ntasks, u_lo, u_hi, Lsx, RelMap, ticket, whole_tiles, min_units);
        else
            hipLaunchKernelGGL((k_gemm<0, true>), dim3(grid), dim3(GEMM_THREADS), 0, st, probs, tasks, kt_prefix, ntasks, u_lo, u_hi, Lsx, RelMap, ticket, whole_tiles, min_units);
        return;
    }
    if (mode == 1)
        hipLaunchKernelGGL((k_gemm<1, false>), dim3(grid), dim3(GEMM_THREADS), 0, st, probs, tasks, kt_prefix, ntasks, u_lo, u_hi, Lsx, RelMap, ticket, whole_tiles, min_units);
    else
        hipLaunchKernelGGL((k_gemm<0, false>), dim3(grid), dim3(GEMM_THREADS), 0, st, probs, tasks, kt_prefix, ntasks, u_lo, u_hi, Lsx, RelMap, ticket, whole_tiles, min_units);
}

}  // namespace sf
