// The transposed solve with a resident LU factor, x <- A^{-T} b (sf_lu_plan_solve_transposed, _solve_many_transposed), and the
// 1-norm condition estimate that alternates it with the plain solve (sf_lu_plan_condest, sf_chol_plan_condest).  DESIGN 8e.
//
// Permuted space, as the plain solve.  A = L U with L unit lower in the L panels (PL) and U^T -- lower, non-unit diagonal -- in
// the U^T panels (PU), both sets with the same offsets, task lists and row indices.  So A^{-T} b = L^{-T} (U^T)^{-1} b:
//   forward sweep over PU : exactly what k_solve_fwd / k_solve_many_fwd do with base = PU, unit = 0, pivpos = nullptr -- the
//                           existing kernels, no new one (U's rows moved with the pivots, so PU is a true triangle)
//   backward sweep over PL: the kernels below, twins of the four backward kernels of sf_solve.hip with the SAME row tiles, tasks,
//                           tickets, sync words, `expect` counts and near / far order.  Only the diagonal task differs: the
//                           triangle is loaded with the diagonal implied (the stored diagonal and upper part of a PL diagonal
//                           block are not L), dinv = 1, and with pivoting on the block's interchanges are undone after its chain.
// Pivoting: the forward sweep of the plain solve computes E_K^{-1} P_K ... E_1^{-1} P_1 b (P_k: x_new[pivpos[g]] = x_old[g] on
// 64-column block k; E_k: elimination with the block's stored L columns, the entries left of a block keep their old rows), hence
// A^{-T} = P_1^T E_1^{-T} ... P_K^T E_K^{-T} U^{-T}: blocks from the last to the first, x_blk -= L(below, blk)^T x_below, the unit
// chain, then x_new[g] = x_old[pivpos[g]] BEFORE any earlier sub-block or step reads x_blk.  A step's 64-column sub-blocks are the
// pivot blocks (k_solve_fwd relies on that too).
#include <sparseframe_hip.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <limits>

#include "sf_plan_internal.h"
#include "sf_solve_common.h"

namespace sf {

// k_solve_bwd with the unit-diagonal triangle and the inverse interchanges (pivpos may be null)
template <bool BIG>
__global__ void __launch_bounds__(256, BIG ? 1 : 2)
k_tsolve_bwd(const SolveTask* __restrict__ tasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
             double* __restrict__ x, const int32_t* __restrict__ pivpos, int* __restrict__ sync, int* __restrict__ ticket,
             int* __restrict__ info, const double* __restrict__ Tbase) {
    __shared__ int s_ticket;
    __shared__ double xs[SV_B];
    __shared__ double pv[NB];           // the wave whose turn it is: its 64 values on their way back to their rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolveTask t = sv_claim(tasks, ticket, s_ticket, tid);
    const int b = t.b;
    const int64_t ld = t.ld;
    const int o = NB * wave;
    const int bw = min(NB, max(0, b - o));
    if (t.nrows > 0) {
        // ---- row tile: k_solve_bwd's (lane = row, wave = 64-column chunk, the transposing butterfly) ----
        double p[NB];
        if (bw > 0) {
            int nr = min(t.nrows, SV_ROWS);
            int rr = t.row0 + min(lane, nr - 1);
            {
                SV_LOAD_TILE_ROW(p, Lsx + t.panel + rr + (int64_t)(t.diag + o) * ld, ld, bw)
                const double xr = (lane < nr) ? x[Lsi[t.rows + rr]] : 0.0;
#pragma unroll
                for (int k = 0; k < NB; ++k) p[k] *= xr;
            }
            if (BIG) {
#pragma unroll 1
                for (int g0 = SV_ROWS; g0 < t.nrows; g0 += SV_ROWS) {
                    nr = min(t.nrows - g0, SV_ROWS);
                    rr = t.row0 + g0 + min(lane, nr - 1);
                    double q[NB];
                    SV_LOAD_TILE_ROW(q, Lsx + t.panel + rr + (int64_t)(t.diag + o) * ld, ld, bw)
                    const double xr = (lane < nr) ? x[Lsi[t.rows + rr]] : 0.0;
#pragma unroll
                    for (int k = 0; k < NB; ++k) p[k] += q[k] * xr;
                }
            }
            SV_BUTTERFLY64(p, lane)
            if (lane < bw) unsafeAtomicAdd(x + t.first_col + t.diag + o + lane, -p[0]);
        }
        sv_tile_done(sync + t.flag, tid);
        return;
    }
    // ---- diagonal task: x_blk <- P^T L^{-T} x_blk, sub-blocks from the last to the first; lane = column ----
    const double* P = Lsx + t.panel;
    const double* __restrict__ Td = (Tbase && t.tdiag) ? Tbase + (t.tdiag - 1) : nullptr;
    double bcol[NB];
    if (bw > 0) {
        SV_LOAD_UPPER_COL_UNIT(bcol, P, Td, ld, b, t.diag, o, bw, lane)
    } else {
        SV_LOAD_IDENTITY(bcol, lane)
    }
    const double dinv = 1.0;
    const int g0 = t.first_col + t.diag + o;
    // (the block's own interchanges; the clamp keeps a lane without a column on a valid address)
    const int q = (pivpos && bw > 0) ? (pivpos[g0 + min(lane, bw - 1)] - g0) & (NB - 1) : lane;
    if (t.expect > 0) {
        if (tid == 0) sv_wait<4>(sync + t.flag, t.expect, info);
        __syncthreads();
    }
    double* xq = x + g0;
    double v = (lane < bw) ? __builtin_nontemporal_load(xq + min(lane, max(bw, 1) - 1)) : 0.0;
    const int nsub = (b + NB - 1) / NB;
    for (int tt = nsub - 1; tt >= 0; --tt) {
        const bool above = BIG && wave < tt && bw > 0;
        double blk[NB];                                 // L(rows of sub-block tt, this lane's column); read only when BIG
        if (BIG && above) {
            const int bt = min(NB, b - NB * tt);            // rows of sub-block tt
#pragma unroll
            for (int k = 0; k < NB; ++k) blk[k] = SV_COL_RUN(k, P, Td, ld, b, t.diag, NB * tt, bt, o, bw, lane);
        }
        if (wave == tt) {
            SV_CHAIN(false, bcol, dinv, v, lane)
            if (pivpos) {
                // the rows go back where they were before this block's interchanges: x_new[g] = x_old[pivpos[g]] -- before the
                // waves above and every earlier step read them (one wave: LDS operations complete in order)
                pv[lane] = v;
                v = (lane < bw) ? pv[q] : 0.0;
            }
            xs[o + lane] = (lane < bw) ? v : 0.0;
        }
        if (BIG) {
            __syncthreads();
            if (above) {
#pragma unroll
                for (int k = 0; k < NB; ++k) v -= blk[k] * xs[NB * tt + k];       // rows beyond the sub-block's meet xs = 0
            }
        }
    }
    if (lane < bw) xq[lane] = v;
}

// k_solve_small_bwd's twin: one wave per narrow supernode (one pivot block)
__global__ void __launch_bounds__(256, 2)
k_tsolve_small_bwd(const SolveTask* __restrict__ tasks, int ntasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                   double* __restrict__ x, const int32_t* __restrict__ pivpos) {
    __shared__ double ptmp[4][NB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ti = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (ti >= ntasks) return;
    const SolveTask t = tasks[ti];
    const int b = t.b;
    const int64_t ld = t.ld;
    const double* P = Lsx + t.panel;
    // s_c = sum over the rows below of L(row, c) x[row]: lane = row (coalesced), then the transposing butterfly
    double s = 0.0;
    double p[NB];
    for (int r0 = b; r0 < (int)ld; r0 += NB) {
        const int row = min(r0 + lane, (int)ld - 1);
        SV_LOAD_TILE_ROW(p, P + row, ld, b)
        const double xr = (r0 + lane < (int)ld) ? x[Lsi[t.rows + row]] : 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) p[k] *= xr;
        SV_BUTTERFLY64(p, lane)
        s += p[0];
    }
    // L^T x_blk = x_blk - s with the diagonal implied, lane = column; then the interchanges undone
    SV_LOAD_UPPER_COL_UNIT(p, P, (const double*)nullptr, ld, b, 0, 0, b, lane)
    const double dinv = 1.0;
    double* xq = x + t.first_col;
    double v = (lane < b) ? xq[lane] - s : 0.0;
    SV_CHAIN(false, p, dinv, v, lane)
    if (pivpos) {
        const int q = (pivpos[t.first_col + min(lane, b - 1)] - t.first_col) & (NB - 1);
        ptmp[wave][lane] = v;
        v = ptmp[wave][q];              // (one wave: LDS operations complete in order)
    }
    if (lane < b) xq[lane] = v;
}

// k_solve_many_bwd's twin (one workgroup per CU as the register bound, as there)
template <bool BIG>
__global__ void __launch_bounds__(256, 1)
k_tsolve_many_bwd(const SolveTask* __restrict__ tasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                  double* __restrict__ x, const int32_t* __restrict__ pivpos, int* __restrict__ sync, int* __restrict__ ticket,
                  int* __restrict__ info, const double* __restrict__ Tbase) {
    __shared__ int s_ticket;
    __shared__ double xs[SV_B * SVM_LD];      // diagonal task: x_blk; row tile: the tile's x rows (SV_ROWS x SVM_W)
    __shared__ double acc_s[4 * NB * SVM_LD];  // row tile: the products, lane = column; diagonal task: the rows being interchanged
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolveTask t = sv_claim(tasks, ticket, s_ticket, tid);
    const int b = t.b;
    const int64_t ld = t.ld;
    const int o = NB * wave;
    const int bw = min(NB, max(0, b - o));
    if (t.nrows > 0) {
        // ---- row tile: k_solve_many_bwd's (lane = column, wave = 64-column chunk, the tile's x rows staged in LDS) ----
        double* arow = acc_s + (wave * NB + lane) * SVM_LD;        // -(the sum so far)
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) arow[c] = 0.0;
        for (int g0 = 0;;) {
            const int nr = min(t.nrows - g0, SV_ROWS);
            double lc[NB];
            if (bw > 0) {
                const double* Lc = Lsx + t.panel + (t.row0 + g0) + (int64_t)(t.diag + o + min(lane, bw - 1)) * ld;
#pragma unroll
                for (int k = 0; k < NB; ++k) lc[k] = Lc[min(k, nr - 1)];
            }
            if (g0 > 0) __syncthreads();        // xs of the previous group has been read
            for (int e = tid; e < SV_ROWS * SVM_W; e += 256) {
                const int rr = e / SVM_W, c = e % SVM_W;
                xs[rr * SVM_LD + c] = (rr < nr) ? x[(int64_t)Lsi[t.rows + t.row0 + g0 + min(rr, nr - 1)] * SVM_W + c] : 0.0;
            }
            __syncthreads();
            if (bw > 0) svm_product<true>(lc, xs, arow);          // rows beyond nr meet xs = 0
            g0 += SV_ROWS;
            if (!BIG || g0 >= t.nrows) break;
        }
        if (lane < bw) {
            double* xc = x + (int64_t)(t.first_col + t.diag + o + lane) * SVM_W;
#pragma unroll
            for (int c = 0; c < SVM_W; ++c) unsafeAtomicAdd(xc + c, arow[c]);
        }
        sv_tile_done(sync + t.flag, tid);
        return;
    }
    // ---- diagonal task (k_tsolve_bwd's; x_blk in LDS, row o + lane = this lane's; lane = column of the block) ----
    const double* P = Lsx + t.panel;
    const double* __restrict__ Td = (Tbase && t.tdiag) ? Tbase + (t.tdiag - 1) : nullptr;
    double bcol[NB];
    if (bw > 0) {
        SV_LOAD_UPPER_COL_UNIT(bcol, P, Td, ld, b, t.diag, o, bw, lane)
    } else {
        SV_LOAD_IDENTITY(bcol, lane)
    }
    const double dinv = 1.0;
    const int g0 = t.first_col + t.diag + o;
    const int q = (pivpos && bw > 0) ? (pivpos[g0 + min(lane, bw - 1)] - g0) & (NB - 1) : lane;
    if (t.expect > 0) {
        if (tid == 0) sv_wait<4>(sync + t.flag, t.expect, info);
        __syncthreads();
    }
    double* xq = x + (int64_t)g0 * SVM_W;
    double* xrow = xs + (o + lane) * SVM_LD;
    if (bw > 0) {
        const double* src = xq + (int64_t)min(lane, bw - 1) * SVM_W;
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xrow[c] = (lane < bw) ? __builtin_nontemporal_load(src + c) : 0.0;
    } else {
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xrow[c] = 0.0;
    }
    const int nsub = (b + NB - 1) / NB;
    for (int tt = nsub - 1; tt >= 0; --tt) {
        const bool above = BIG && wave < tt && bw > 0;
        double blk[NB];            // (read only when BIG)
        if (BIG && above) {
            const int bt = min(NB, b - NB * tt);            // rows of sub-block tt
#pragma unroll
            for (int k = 0; k < NB; ++k) blk[k] = SV_COL_RUN(k, P, Td, ld, b, t.diag, NB * tt, bt, o, bw, lane);
        }
        if (wave == tt) {
            svm_chain<false>(bcol, dinv, xrow, lane);
            if (pivpos) {
                // the block's interchanges undone, every column alike (through this wave's own part of acc_s; one wave: LDS in order)
                double* pw = acc_s + wave * NB * SVM_LD;
#pragma unroll
                for (int c = 0; c < SVM_W; ++c) pw[lane * SVM_LD + c] = xrow[c];
#pragma unroll
                for (int c = 0; c < SVM_W; ++c) xrow[c] = pw[q * SVM_LD + c];
            }
            if (lane >= bw) {
#pragma unroll
                for (int c = 0; c < SVM_W; ++c) xrow[c] = 0.0;
            }
        }
        if (BIG) {
            __syncthreads();
            if (above) svm_product<true>(blk, xs + NB * tt * SVM_LD, xrow);     // rows beyond the sub-block's hold 0
        }
    }
    if (lane < bw) {
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xq[(int64_t)lane * SVM_W + c] = xrow[c];
    }
}

// k_solve_many_small_bwd's twin
__global__ void __launch_bounds__(256, 2)
k_tsolve_many_small_bwd(const SolveTask* __restrict__ tasks, int ntasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                        double* __restrict__ x, const int32_t* __restrict__ pivpos) {
    __shared__ double xs[4 * NB * SVM_LD];     // the 64 rows' x being summed; afterwards the rows being interchanged
    __shared__ double vs[4 * NB * SVM_LD];     // x_blk, row lane = this lane's
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ti = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (ti >= ntasks) return;
    const SolveTask t = tasks[ti];
    const int b = t.b;
    const int64_t ld = t.ld;
    const double* P = Lsx + t.panel;
    double* xw = xs + wave * NB * SVM_LD;
    double* xrow = vs + (wave * NB + lane) * SVM_LD;
    double* xq = x + (int64_t)t.first_col * SVM_W;
    {
        const double* src = xq + (int64_t)min(lane, b - 1) * SVM_W;
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xrow[c] = (lane < b) ? src[c] : 0.0;
    }
    // x_blk[lane, :] -= sum over the rows below of L(row, lane) x[row, :]: lane = column, the 64 rows' x in LDS
    double p[NB];
    for (int r0 = b; r0 < (int)ld; r0 += NB) {
#pragma unroll
        for (int k = 0; k < NB; ++k) p[k] = P[min(r0 + k, (int)ld - 1) + (int64_t)min(lane, b - 1) * ld];
        const int row = min(r0 + lane, (int)ld - 1);
        const double* xr = x + (int64_t)Lsi[t.rows + row] * SVM_W;
        const bool live = r0 + lane < (int)ld;
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xw[lane * SVM_LD + c] = live ? xr[c] : 0.0;
        svm_product<true>(p, xw, xrow);            // rows beyond ld meet xw = 0
    }
    // L^T x_blk = x_blk - s with the diagonal implied, lane = column; then the interchanges undone
    SV_LOAD_UPPER_COL_UNIT(p, P, (const double*)nullptr, ld, b, 0, 0, b, lane)
    const double dinv = 1.0;
    svm_chain<false>(p, dinv, xrow, lane);
    if (pivpos) {
        const int q = (pivpos[t.first_col + min(lane, b - 1)] - t.first_col) & (NB - 1);
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xw[lane * SVM_LD + c] = xrow[c];
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xrow[c] = xw[q * SVM_LD + c];
    }
    if (lane < b) {
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xq[(int64_t)lane * SVM_W + c] = xrow[c];
    }
}

static bool tsv_single(int width) {
    assert(width == 1 || width == SVM_W);       // x has one of two layouts: any other width would run a kernel on the wrong one
    return width == 1;
}
void launch_tsolve_small_bwd(const SolveTask* t, int nt, int width, const double* Lsx, const int32_t* Lsi, double* x, const int32_t* pivpos,
                             hipStream_t st) {
    if (nt <= 0) return;
    hipLaunchKernelGGL(tsv_single(width) ? k_tsolve_small_bwd : k_tsolve_many_small_bwd, dim3((nt + 3) / 4), dim3(256), 0, st, t, nt, Lsx, Lsi, x,
                       pivpos);
}
void launch_tsolve_bwd(const SolveTask* t, int nt, int width, int big, const double* Lsx, const int32_t* Lsi, double* x,
                       const int32_t* pivpos, int* sync, int* ticket, int* info, hipStream_t st, const double* Tbase) {
    if (nt <= 0) return;
    const auto k = tsv_single(width) ? (big ? k_tsolve_bwd<true> : k_tsolve_bwd<false>) : (big ? k_tsolve_many_bwd<true> : k_tsolve_many_bwd<false>);
    hipLaunchKernelGGL(k, dim3(nt), dim3(256), 0, st, t, Lsx, Lsi, x, pivpos, sync, ticket, info, Tbase);
}

// ---------------------------------------------------------------------------------------------------
// The condition estimate's per-iteration work on the device (Hager / Higham, LAPACK xLACON; the driver is below).  n doubles are
// read once between two sweeps that read the whole factor, so each is ONE workgroup that strides over the vector and reduces in a
// fixed order (no floating-point atomics: the same factor gives the same estimate on every call).
// ---------------------------------------------------------------------------------------------------
constexpr int CE_T = 1024;
static_assert(sizeof(CondScalars) == 16, "the one small copy of an iteration");

// the safeguard vector x_i = (-1)^i (1 + i / (n - 1)), n > 1
__device__ __forceinline__ double ce_altsgn(int64_t i, int64_t n) {
    const double v = 1.0 + (double)i / (double)(n - 1);
    return (i & 1) ? -v : v;
}

// mode 0: x = 1 / n;  mode 2: the safeguard vector
__global__ void __launch_bounds__(256)
k_condest_fill(double* __restrict__ x, int64_t n, int mode) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = mode == 0 ? 1.0 / (double)n : ce_altsgn(i, n);
}

// s->nrm = |y|_1; bit 0 of s->flags = (sign(y) == xi everywhere); then xi = y = sign(y) (sign(0) = 1), the next A^{-T} sweep's input
__global__ void __launch_bounds__(CE_T)
k_condest_sign_norm(double* __restrict__ y, double* __restrict__ xi, int64_t n, const int* __restrict__ solve_info,
                    CondScalars* __restrict__ s) {
    __shared__ double sum[CE_T];
    __shared__ int diff[CE_T];
    const int tid = threadIdx.x;
    double acc = 0.0;
    int d = 0;
    for (int64_t i = tid; i < n; i += CE_T) {
        const double v = y[i];
        const double sg = v >= 0.0 ? 1.0 : -1.0;
        acc += fabs(v);
        d |= (sg != xi[i]) ? 1 : 0;
        xi[i] = sg;
        y[i] = sg;
    }
    sum[tid] = acc;
    diff[tid] = d;
    __syncthreads();
    for (int m = CE_T / 2; m >= 1; m >>= 1) {
        if (tid < m) { sum[tid] += sum[tid + m]; diff[tid] |= diff[tid + m]; }
        __syncthreads();
    }
    if (tid == 0) {
        s->nrm = sum[0];
        s->flags = (s->flags & 2) | (diff[0] ? 0 : 1) | (*solve_info ? 4 : 0);
    }
}

// j = the first index of the largest |x_i|.  Unless `first`: the iteration stops if x[previous j] is that maximum, or if this was
// the `last` allowed one.  Stopping: x = the safeguard vector (flag bit 1); otherwise x = e_j.  Either way the next sweep is A^{-1} x.
__global__ void __launch_bounds__(CE_T)
k_condest_argmax_next(double* __restrict__ x, int64_t n, CondScalars* __restrict__ s, int first, int last) {
    __shared__ double best[CE_T];
    __shared__ int64_t where[CE_T];
    __shared__ int s_stop;
    const int tid = threadIdx.x;
    double bv = -1.0;
    int64_t bi = n;
    for (int64_t i = tid; i < n; i += CE_T) {
        const double a = fabs(x[i]);
        if (a > bv) { bv = a; bi = i; }         // (ascending i: the first of equals stays)
    }
    best[tid] = bv;
    where[tid] = bi;
    __syncthreads();
    for (int m = CE_T / 2; m >= 1; m >>= 1) {
        if (tid < m) {
            const double ov = best[tid + m];
            const int64_t oi = where[tid + m];
            if (ov > best[tid] || (ov == best[tid] && oi < where[tid])) { best[tid] = ov; where[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t j = where[0] < n ? where[0] : 0;       // (every entry NaN: any column will do, the norm comes out NaN)
        const int64_t jlast = s->j;
        const int stop = !first && (last || (jlast >= 0 && jlast < n && x[jlast] == best[0]));
        s->j = (int32_t)j;
        s->flags = stop ? 2 : 0;
        s_stop = stop;
    }
    __syncthreads();
    const int stop = s_stop;
    const int64_t j = s->j;
    for (int64_t i = tid; i < n; i += CE_T) x[i] = stop ? ce_altsgn(i, n) : (i == j ? 1.0 : 0.0);
}

void launch_condest_fill(double* x, int64_t n, int mode, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_condest_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, mode);
}
void launch_condest_sign_norm(double* y, double* xi, int64_t n, const int* solve_info, CondScalars* s, hipStream_t st) {
    hipLaunchKernelGGL(k_condest_sign_norm, dim3(1), dim3(CE_T), 0, st, y, xi, n, solve_info, s);
}
void launch_condest_argmax_next(double* x, int64_t n, CondScalars* s, int first, int last, hipStream_t st) {
    hipLaunchKernelGGL(k_condest_argmax_next, dim3(1), dim3(CE_T), 0, st, x, n, s, first, last);
}

}  // namespace sf

// ---------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------
// x <- A^{-T} x for an LU plan (the caller has zeroed the sync block on the stream), in its two halves.  The row-major copies of the
// top steps' diagonal blocks (d_solveT) are made from the PL base by the second half, on every call that asks for them; their
// diagonal entries are copied too and simply not read.  sf_solve_sweep_bwd remakes them from PU at the start of every solve /
// solve_many / refine call, so neither sweep ever sees the other's copies (sf_apply_sweep states the rule for its callers).
// (U^T)^{-1}: the plain forward kernels on the other panel set -- non-unit diagonal, no interchanges
void tsolve_sweep_fwd(sf_chol_plan* p, double* x, int width, const SolveSync& y, hipStream_t st) {
    const double* PU = p->d_Lsx + p->xC;
    const size_t nsteps = p->solve_steps.size();
    for (size_t k = 0; k < nsteps; ++k) {
        const auto& s = p->solve_steps[k];
        int* tk = y.tickets + sf_chol_plan::SOLVE_TICKETS * k;
        if (s.small) sf::launch_solve_small_fwd(p->d_solve + s.fwd_first, s.ndiag, width, PU, p->d_Lsi, x, 0, nullptr, st);
        else sf::launch_solve_fwd(p->d_solve + s.fwd_first, s.fwd_count, width, s.big, PU, p->d_Lsi, x, 0, nullptr, y.sync, tk, y.info, st);
    }
}

// L^{-T} with the interchanges undone block by block: sf_solve_step_bwd's launches, the twin kernels
void tsolve_sweep_bwd(sf_chol_plan* p, double* x, int width, bool transpose_diag, const SolveSync& y, hipStream_t st) {
    const double* PL = p->d_Lsx;
    const int32_t* piv = p->piv_tol > 0.0 ? p->d_piv : nullptr;
    if (transpose_diag) sf::launch_solve_transpose_diag(p->d_solve, p->d_solveT_list, p->n_solveT, PL, p->d_solveT, st);
    for (size_t k = p->solve_steps.size(); k-- > 0;) {
        const auto& s = p->solve_steps[k];
        int* tk = y.tickets + sf_chol_plan::SOLVE_TICKETS * k;
        if (s.small) {
            sf::launch_tsolve_small_bwd(p->d_solve + s.bwd_first, s.ndiag, width, PL, p->d_Lsi, x, piv, st);
        } else if (p->solve_bwd_fused) {
            sf::launch_tsolve_bwd(p->d_solve + s.bwd_first, s.count, width, s.big, PL, p->d_Lsi, x, piv, y.sync, tk + 1, y.info, st, p->d_solveT);
        } else {
            sf::launch_tsolve_bwd(p->d_solve + s.bwd_first, s.nrows_tasks, width, 0, PL, p->d_Lsi, x, piv, y.sync, tk + 1, y.info, st, nullptr);
            sf::launch_tsolve_bwd(p->d_solve + s.bwd_first + s.nrows_tasks, s.count - s.nrows_tasks, width, s.big, PL, p->d_Lsi, x, piv, y.sync,
                                  tk + 2, y.info, st, p->d_solveT);
        }
    }
}

void tsolve_sweeps(sf_chol_plan* p, double* x, int width, bool transpose_diag, hipStream_t st) {
    const SolveSync y = sf_solve_sync(p);
    tsolve_sweep_fwd(p, x, width, y, st);
    tsolve_sweep_bwd(p, x, width, transpose_diag, y, st);
}

namespace {

int condest(sf_chol_plan* p, sf_float* anorm, sf_float* ainv_norm_est) {
    if (!sf_plan_whole_resident(p) || !p->fs.has_values()) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    *anorm = 0.0;
    *ainv_norm_est = 0.0;
    p->last_condest_solves = 0;
    p->last_condest_ms = 0.0;
    const int64_t n = p->n;
    if (n <= 0) return SF_OK;
    hipStream_t st = p->stream;
    const double* d_anorm = nullptr;
    if (int rc = sf_refine_anorm(p, &d_anorm, st)) return rc;      // |A|_1 of the current values (sf_refine.hip)
    if (!p->d_cond) {
        if (p->d_cond.alloc(2 * (size_t)n + 2)) return SF_ERR_HIP;
        p->bytes_condest = (2 * (size_t)n + 2) * sizeof(double);
    }
    double* x = p->d_cond;
    double* xi = x + n;
    sf::CondScalars* ds = (sf::CondScalars*)(xi + n);
    int solves = 0;
    bool solve_failed = false;
    // A^{-1} x and A^{-T} x in place.  LU: each sweep pair makes its own row-major diagonal copies (see tsolve_sweeps); Cholesky: the
    // plain sweeps serve for both (A = A^T) and the first one's copies stay good.
    auto sweep = [&](bool transposed) -> int {
        const bool trans = transposed && p->lu;
        ++solves;
        return sf_apply_sweep(p, trans ? SF_SWEEP_TRANS : SF_SWEEP_SOLVE, x, 1, p->lu || solves == 1);
    };
    // the one 16-byte copy and the one synchronisation of an iteration
    sf::CondScalars h;
    auto read = [&]() -> int {
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&h, ds, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h.flags & 4) solve_failed = true;
        return SF_OK;
    };
    hipEvent_t e0 = p->ev_s0, e1 = p->ev_s1;
    HIP_TRY(hipEventRecord(e0, st));
    HIP_TRY(hipMemsetAsync(xi, 0, ((size_t)n + 2) * sizeof(double), st));
    sf::launch_condest_fill(x, n, 0, st);
    if (int rc = sweep(false)) return rc;
    sf::launch_condest_sign_norm(x, xi, n, (const int*)p->d_solve_sync, ds, st);
    double h_anorm = 0.0;
    HIP_TRY(hipMemcpyAsync(&h_anorm, d_anorm, sizeof(double), hipMemcpyDeviceToHost, st));
    if (int rc = read()) return rc;
    double est = h.nrm;
    constexpr int ITMAX = 5;
    // xLACON's loop with its two host decisions moved so that a pass needs one read: whether pass k goes on after its A^{-T} sweep
    // (x[previous j] is the maximum, or k == ITMAX) only chooses the NEXT A^{-1} sweep's input, e_j or the safeguard vector, so
    // k_condest_argmax_next decides it on the device and says which it was.  At most 1 + 5 + 4 + 1 = 11 sweeps.
    for (int iter = 1; n > 1 && std::isfinite(est) && !solve_failed; ++iter) {
        if (int rc = sweep(true)) return rc;                                            // x = A^{-T} xi
        sf::launch_condest_argmax_next(x, n, ds, iter == 1 ? 1 : 0, iter >= ITMAX ? 1 : 0, st);
        if (int rc = sweep(false)) return rc;                                           // x = A^{-1} (e_j or the safeguard vector)
        sf::launch_condest_sign_norm(x, xi, n, (const int*)p->d_solve_sync, ds, st);
        if (int rc = read()) return rc;
        const bool safeguard = (h.flags & 2) != 0;
        if (!safeguard) {
            // |A^{-1} e_j|_1 is a lower bound whatever j: the larger of the old and the new one is kept (xLACON keeps the new one)
            const bool go_on = !(h.flags & 1) && h.nrm > est;
            est = std::isfinite(h.nrm) ? std::max(est, h.nrm) : h.nrm;
            if (go_on) continue;
            if (!std::isfinite(est) || solve_failed) break;
            sf::launch_condest_fill(x, n, 2, st);
            if (int rc = sweep(false)) return rc;
            sf::launch_condest_sign_norm(x, xi, n, (const int*)p->d_solve_sync, ds, st);
            if (int rc = read()) return rc;
        }
        const double alt = 2.0 * h.nrm / (3.0 * (double)n);
        est = std::isfinite(alt) ? std::max(est, alt) : alt;
        break;
    }
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    if (elapsed_ms(&ms, e0, e1)) p->last_condest_ms = ms;
    p->last_condest_solves = solves;
    if (solve_failed) return SF_ERR_HIP;        // a bounded in-launch wait ran out (never seen)
    *anorm = h_anorm;
    *ainv_norm_est = est;
    return SF_OK;
}

}  // namespace

extern "C" {

int sf_lu_plan_solve_transposed(sf_lu_plan* p, const sf_float* b_host, sf_float* x_host) {
    if (!p || !b_host || !x_host) return SF_ERR_ARG;
    if (!p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (p->n <= 0) return SF_OK;
    const SfCols src{const_cast<double*>(b_host), p->n, false, nullptr}, dst{x_host, p->n, false, nullptr};
    SfStretch t{p};
    if (int rc = sf_apply_chunks(p, SfApply{&src, &dst, 1, 1, p->d_x, 0, true}, t,
                                 [&](double* x, sf_long, int) { return sf_apply_sweep(p, SF_SWEEP_TRANS, x, 1, true); }))
        return rc;
    if (t.timed) p->last_solve_ms = t.total_ms;
    return SF_OK;
}

// sf_chol_plan_solve_many's chunking, staging and layouts (see there), the transposed sweeps in the middle
int sf_lu_plan_solve_many_transposed(sf_lu_plan* p, sf_long nrhs, const sf_float* B, sf_long ldb, sf_float* X, sf_long ldx) {
    if (!p || !B || !X || nrhs < 0) return SF_ERR_ARG;
    if (!p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    const sf_long ldmin = std::max<sf_long>(p->n, 1);
    if (ldb < ldmin || ldx < ldmin) return SF_ERR_ARG;
    if ((const void*)X == (const void*)B && ldx != ldb) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (nrhs == 0 || p->n <= 0) return SF_OK;
    if (int rc = sf_solve_many_block(p)) return rc;
    const SfCols src{const_cast<double*>(B), ldb, false, nullptr}, dst{X, ldx, false, nullptr};
    SfStretch t{p};
    // (the row-major copies of the diagonal blocks: once per call)
    if (int rc = sf_apply_chunks(p, SfApply{&src, &dst, nrhs, sf::SVM_W, p->d_xm, 0, true}, t,
                                 [&](double* x, sf_long j0, int) { return sf_apply_sweep(p, SF_SWEEP_TRANS, x, sf::SVM_W, j0 == 0); }))
        return rc;
    p->last_solve_many_ms = t.total_ms;
    return SF_OK;
}

int sf_chol_plan_condest(sf_chol_plan* p, sf_float* anorm, sf_float* ainv_norm_est) {
    return (p && !p->lu && anorm && ainv_norm_est) ? condest(p, anorm, ainv_norm_est) : SF_ERR_ARG;
}
int sf_lu_plan_condest(sf_lu_plan* p, sf_float* anorm, sf_float* ainv_norm_est) {
    return (p && p->lu && anorm && ainv_norm_est) ? condest(p, anorm, ainv_norm_est) : SF_ERR_ARG;
}

}  // extern "C"
