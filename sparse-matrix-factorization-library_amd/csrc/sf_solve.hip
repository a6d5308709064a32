// The device solve with the resident factor: the gfx950 kernels of the two triangular sweeps, their launchers, and the host
// drivers (sf_chol_plan_solve, sf_chol_plan_solve_many, the LU entry points; the distributed driver in sf_multi.hip shares the
// step functions and the backward half).  Reference: scalar host loops, C:3074-3134, L:3592-3700 (citations as in sf_kernels.hip).
//
// Two kernel families run the same tasks, schedule and sync words: the single-vector kernels (k_solve_*) and the SVM_W-column
// kernels (k_solve_many_*).  Everything the two share is written ONCE, in sf_solve_common.h (the transposed backward sweep of
// sf_solve_t.hip shares it too): the ticket claim and the hand-off protocol as
// functions (sv_*), the fragments on a lane's register array -- clamped triangle, column and row loads, the dinv select, the
// butterfly, the substitution chain -- as macros expanded in place (SV_*, see there for why).  Only the tile bodies differ on
// purpose (a butterfly in registers against a product out of LDS).
#include <sparseframe_hip.h>

#include <algorithm>
#include <cassert>

#include "sf_plan_internal.h"
#include "sf_solve_common.h"

namespace sf {

// ---------------------------------------------------------------------------------------------------
// Triangular solves with the resident factor (L L^T x = b or L U x = b, permuted space).
// The sweep is a chain of dependent steps, so the step is made BIG and its inside cheap:
// one launch per (level, 256-column step) and direction (SV_B = 256),
//   forward : x_blk <- D^{-1} x_blk  (256 x 256 lower-triangular block)  ;  x[rows below] -= L[rows, blk] x_blk
//   backward: x_blk -= L[rows below, blk]^T x[rows below]               ;  x_blk <- D^{-T} x_blk
// and both halves hand over INSIDE the launch (tasks claimed by ticket in execution order, producers first in the list).
// Diagonal task = one workgroup, wave w owns the 64-column sub-block w: its 64 x 64 triangle sits in the lane's registers
// from the start (all four waves load at once), the off-diagonal 64 x 64 blocks are prefetched one sub-step ahead, the
// solved sub-vector goes round through LDS: 4 substitution chains of 64 and 3 barriers instead of 4 launches with 4
// device-scope hand-offs.  No division on the chains (lane j forms 1 / D(j,j) up front).
// Row tiles = 64 rows x the step's columns: thread (lane, wave) = (row, 64-column chunk) forward, (column, chunk)
// backward, ALL its 64 matrix entries are in flight before the hand-off, after it 64 FMAs and one atomic.
// ---------------------------------------------------------------------------------------------------
template <bool BIG>
__global__ void __launch_bounds__(256, BIG ? 1 : 2)
k_solve_fwd(const SolveTask* __restrict__ tasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
            double* __restrict__ x, int unit, const int32_t* __restrict__ pivpos, int* __restrict__ sync, int* __restrict__ ticket,
            int* __restrict__ info) {
    __shared__ int s_ticket;
    __shared__ double xs[SV_B];
    __shared__ double part[4][NB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolveTask t = sv_claim(tasks, ticket, s_ticket, tid);
    const int b = t.b;                  // <= SV_B columns in this step
    const int64_t ld = t.ld;
    const int o = NB * wave;
    const int bw = min(NB, max(0, b - o));      // this wave's part of the step's columns
    if (t.nrows == 0) {                 // ---- diagonal task ----
        const double* P = Lsx + t.panel;
        double a[NB];
        if (bw > 0) {
            SV_LOAD_LOWER_ROW(a, P, ld, t.diag + o, bw, unit, lane)
        } else {
            SV_LOAD_IDENTITY(a, lane)
        }
        double* xq = x + t.first_col + t.diag + o;
        double v = (lane < bw) ? xq[lane] : 0.0;
        double dinv = 1.0;
        SV_DINV(dinv, a, lane)
        const int nsub = (b + NB - 1) / NB;
        for (int tt = 0; tt < nsub; ++tt) {
            const bool below = BIG && wave > tt && bw > 0;
            double blk[BIG ? NB : 1];       // L(this wave's row, columns of sub-block tt): in flight while wave tt solves
            if (BIG && below) {
#pragma unroll
                for (int k = 0; k < NB; ++k) blk[k] = P[(t.diag + o + min(lane, bw - 1)) + (int64_t)(t.diag + NB * tt + k) * ld];
            }
            if (wave == tt) {
                if (pivpos) {
                    // LU with pivoting: the row interchanges of this 64-column block, applied as the sweep reaches it
                    // (LINPACK-style: the L entries to the left of a block were stored at their rows' original places)
                    const int g0 = t.first_col + t.diag + o;
                    if (lane < bw) part[0][pivpos[g0 + lane] - g0] = v;
                    v = (lane < bw) ? part[0][lane] : 0.0;       // one wave: LDS operations complete in order
                }
                SV_CHAIN(true, a, dinv, v, lane)
                xs[o + lane] = (lane < bw) ? v : 0.0;
            }
            if (BIG) {
                __syncthreads();
                if (below) {
#pragma unroll
                    for (int k = 0; k < NB; ++k) v -= blk[k] * xs[NB * tt + k];
                }
            }
        }
        if (lane < bw) xq[lane] = v;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) sv_publish(sync + t.flag, 1);
        return;
    }
    // ---- row tile: lane = row, wave = 64-column chunk; the 64 entries are in flight while the diagonal block is solved ----
    // (a "far" tile of a look-ahead step may hold several 64-row groups, t.nrows > 64: one workgroup streams through them -- one
    // ticket, one task, one flag poll, one load of x_blk for all of them)
    int nr = min(t.nrows, SV_ROWS);
    int r = t.row0 + min(lane, nr - 1);
    double lr[NB];
    if (bw > 0) SV_LOAD_TILE_ROW(lr, Lsx + t.panel + r + (int64_t)(t.diag + o) * ld, ld, bw)
    int32_t gi = Lsi[t.rows + r];
    if (tid == 0) sv_wait<16>(sync + t.flag, 1, info);
    __syncthreads();
    xs[tid] = (tid < b) ? __builtin_nontemporal_load(x + t.first_col + t.diag + tid) : 0.0;
    __syncthreads();
    {
        double acc = 0.0;
        if (bw > 0) {
#pragma unroll
            for (int k = 0; k < NB; ++k) acc += lr[k] * xs[o + k];       // columns beyond b meet xs = 0
        }
        part[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && lane < nr) unsafeAtomicAdd(x + gi, -(part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane]));
    }
    if (BIG) {          // (only this instantiation walks through further row groups; the plan makes sure of it)
#pragma unroll 1
        for (int g0 = SV_ROWS; g0 < t.nrows; g0 += SV_ROWS) {
            nr = min(t.nrows - g0, SV_ROWS);
            r = t.row0 + g0 + min(lane, nr - 1);
            if (bw > 0) SV_LOAD_TILE_ROW(lr, Lsx + t.panel + r + (int64_t)(t.diag + o) * ld, ld, bw)
            gi = Lsi[t.rows + r];
            double acc = 0.0;
            if (bw > 0) {
#pragma unroll
                for (int k = 0; k < NB; ++k) acc += lr[k] * xs[o + k];
            }
            __syncthreads();            // part[] of the previous group has been read
            part[wave][lane] = acc;
            __syncthreads();
            if (wave == 0 && lane < nr) unsafeAtomicAdd(x + gi, -(part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane]));
        }
    }
}

template <bool BIG>
__global__ void __launch_bounds__(256, BIG ? 1 : 2)
k_solve_bwd(const SolveTask* __restrict__ tasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
            double* __restrict__ x, int* __restrict__ sync, int* __restrict__ ticket, int* __restrict__ info,
            const double* __restrict__ Tbase) {
    __shared__ int s_ticket;
    __shared__ double xs[SV_B];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolveTask t = sv_claim(tasks, ticket, s_ticket, tid);
    const int b = t.b;
    const int64_t ld = t.ld;
    const int o = NB * wave;
    const int bw = min(NB, max(0, b - o));
    if (t.nrows > 0) {
        // ---- row tile: lane = row (coalesced loads), wave = 64-column chunk.  p[k] = L(row, column k) x_row has to be summed
        // over the 64 lanes for every k: SV_BUTTERFLY64.
        // (a "far" tile of a look-ahead step may hold several 64-row groups, t.nrows > 64: their products are summed in
        // registers first -- the butterfly is linear -- so the group of tiles costs ONE butterfly and ONE set of atomics on the
        // 256 words every tile of the step adds to)
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
    // ---- diagonal task: x_blk <- D^{-T} x_blk, sub-blocks from the last to the first; lane = column ----
    const double* P = Lsx + t.panel;
    const double* __restrict__ Td = (Tbase && t.tdiag) ? Tbase + (t.tdiag - 1) : nullptr;
    double bcol[NB];
    if (bw > 0) {
        SV_LOAD_UPPER_COL(bcol, P, Td, ld, b, t.diag, o, bw, lane)
    } else {
        SV_LOAD_IDENTITY(bcol, lane)
    }
    double dinv = 1.0;
    SV_DINV(dinv, bcol, lane)
    if (t.expect > 0) {
        if (tid == 0) sv_wait<4>(sync + t.flag, t.expect, info);
        __syncthreads();
    }
    double* xq = x + t.first_col + t.diag + o;
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

// ---------------------------------------------------------------------------------------------------
// Steps in which every panel is narrow (nscol <= 64: the swarm levels, tens of thousands of supernodes of a few dozen
// columns): ONE WAVE per supernode does its whole part of the sweep -- diagonal solve and all its rows -- with no hand-off,
// four supernodes per workgroup.  (Through the general kernels such a supernode costs a diagonal workgroup plus one workgroup
// per 64 rows, three of four waves idle in each, and a device-scope hand-off.)  task.ld = nsrow, task.b = nscol.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 2)
k_solve_small_fwd(const SolveTask* __restrict__ tasks, int ntasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                  double* __restrict__ x, int unit, const int32_t* __restrict__ pivpos) {
    __shared__ double ptmp[4][NB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the task index is uniform over the wave: say so, or every field of the task (and all address arithmetic) lives in VGPRs
    const int ti = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (ti >= ntasks) return;
    const SolveTask t = tasks[ti];
    const int b = t.b;
    const int64_t ld = t.ld;
    const double* P = Lsx + t.panel;
    double a[NB];
    SV_LOAD_LOWER_ROW(a, P, ld, 0, b, unit, lane)
    double* xq = x + t.first_col;
    double v = (lane < b) ? xq[lane] : 0.0;
    if (pivpos) {
        if (lane < b) ptmp[wave][pivpos[t.first_col + lane] - t.first_col] = v;
        v = (lane < b) ? ptmp[wave][lane] : 0.0;
    }
    double dinv = 1.0;
    SV_DINV(dinv, a, lane)
    SV_CHAIN(true, a, dinv, v, lane)
    if (lane < b) xq[lane] = v;
    // the rows below: 64 at a time, lane = row; x_blk[k] is broadcast out of lane k's register
    for (int r0 = b; r0 < (int)ld; r0 += NB) {
        const int row = min(r0 + lane, (int)ld - 1);
        SV_LOAD_TILE_ROW(a, P + row, ld, b)
        const int32_t gi = Lsi[t.rows + row];
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k) acc += a[k] * readlane_f64(v, k);       // lanes >= b hold v = 0
        if (r0 + lane < (int)ld) unsafeAtomicAdd(x + gi, -acc);
    }
}

__global__ void __launch_bounds__(256, 2)
k_solve_small_bwd(const SolveTask* __restrict__ tasks, int ntasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                  double* __restrict__ x) {
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
    // D^T x_blk = x_blk - s, lane = column
    SV_LOAD_UPPER_COL(p, P, (const double*)nullptr, ld, b, 0, 0, b, lane)
    double dinv = 1.0;
    SV_DINV(dinv, p, lane)
    double* xq = x + t.first_col;
    double v = (lane < b) ? xq[lane] - s : 0.0;
    SV_CHAIN(false, p, dinv, v, lane)
    if (lane < b) xq[lane] = v;
}

// T(r, c) = D(r, c), row-major b x b, for the lower triangle's 64 x 64 tiles of a step's diagonal block (one workgroup per tile,
// transposed through LDS: reads run down the panel's columns, writes along the copy's rows)
__global__ void __launch_bounds__(256)
k_solve_transpose_diag(const SolveTask* __restrict__ tasks, const int64_t* __restrict__ list, const double* __restrict__ Lsx,
                       double* __restrict__ T) {
    __shared__ double tile[64][65];
    const SolveTask t = tasks[list[blockIdx.x >> 4]];
    const int ti = (blockIdx.x & 15) >> 2, tj = blockIdx.x & 3, b = t.b;
    if (tj > ti || 64 * ti >= b || 64 * tj >= b || !t.tdiag) return;
    const double* __restrict__ P = Lsx + t.panel;
    double* __restrict__ Td = T + (t.tdiag - 1);
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int cc = ty; cc < 64; cc += 4) {
        const int r = 64 * ti + tx, c = 64 * tj + cc;
        if (r < b && c < b) tile[cc][tx] = P[(t.diag + r) + (int64_t)(t.diag + c) * t.ld];
    }
    __syncthreads();
    for (int rr = ty; rr < 64; rr += 4) {
        const int r = 64 * ti + rr, c = 64 * tj + tx;
        if (r < b && c < b) Td[(int64_t)r * b + c] = tile[tx][rr];
    }
}

void launch_solve_transpose_diag(const SolveTask* tasks, const int64_t* list, int64_t ntasks, const double* Lsx, double* T, hipStream_t st) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_solve_transpose_diag, dim3((unsigned)(ntasks * 16)), dim3(256), 0, st, tasks, list, Lsx, T);
}

// ---------------------------------------------------------------------------------------------------
// The SVM_W-column family (sf_chol_plan_solve_many): the same tasks, schedule, sync words, tickets and look-ahead order,
// SVM_W right-hand sides carried through one sweep, so the factor is read once for all of them.
// x is an n x SVM_W block stored ROW-major, x[i * SVM_W + c]: the row a tile gathers or scatters through Lsi is one contiguous
// run of SVM_W doubles (128 bytes), and x_blk of a step is one contiguous run of b rows.  Every operation acts on each column
// on its own (no value of one right-hand side ever meets another's), so a NaN / Inf stays in its column.
//   diagonal tasks: the same substitution chains; the SVM_W values of a lane's row live in LDS and go through the chain
//                   SVM_CW columns per pass (a runtime loop: the registers stay statically indexed, nothing spills)
//   forward tile  : lane = row, wave = 64-column chunk, x_blk (b x SVM_W) staged in LDS and read by broadcast; the 4 waves'
//                   partial products meet in LDS and go out as SVM_W atomics per row, consecutive threads on consecutive words
//   backward tile : lane = COLUMN (its 64 entries one contiguous run down the panel column), the tile's x rows staged in LDS:
//                   a (b x 64) x (64 x SVM_W) product -- the single-vector transposing butterfly would need 64 * SVM_W registers
// LDS rows are padded to SVM_LD doubles (144 bytes: 16-byte aligned, staggered across the banks).
// ---------------------------------------------------------------------------------------------------

template <bool BIG>
__global__ void __launch_bounds__(256, BIG ? 1 : 2)
k_solve_many_fwd(const SolveTask* __restrict__ tasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                 double* __restrict__ x, int unit, const int32_t* __restrict__ pivpos, int* __restrict__ sync, int* __restrict__ ticket,
                 int* __restrict__ info) {
    __shared__ int s_ticket;
    __shared__ int32_t s_gi[SV_ROWS];
    __shared__ double xs[SV_B * SVM_LD];
    __shared__ double part[4 * NB * SVM_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolveTask t = sv_claim(tasks, ticket, s_ticket, tid);
    const int b = t.b;
    const int64_t ld = t.ld;
    const int o = NB * wave;
    const int bw = min(NB, max(0, b - o));
    if (t.nrows == 0) {                 // ---- diagonal task (k_solve_fwd's; x_blk in LDS, row o + lane = this lane's) ----
        const double* P = Lsx + t.panel;
        double a[NB];
        if (bw > 0) {
            SV_LOAD_LOWER_ROW(a, P, ld, t.diag + o, bw, unit, lane)
        } else {
            SV_LOAD_IDENTITY(a, lane)
        }
        double* xq = x + (int64_t)(t.first_col + t.diag + o) * SVM_W;
        double* xrow = xs + (o + lane) * SVM_LD;
        if (bw > 0) {
            const double* src = xq + (int64_t)min(lane, bw - 1) * SVM_W;
#pragma unroll
            for (int c = 0; c < SVM_W; ++c) xrow[c] = (lane < bw) ? src[c] : 0.0;
        } else {
#pragma unroll
            for (int c = 0; c < SVM_W; ++c) xrow[c] = 0.0;
        }
        double dinv = 1.0;
        SV_DINV(dinv, a, lane)
        const int nsub = (b + NB - 1) / NB;
        for (int tt = 0; tt < nsub; ++tt) {
            const bool below = BIG && wave > tt && bw > 0;
            double blk[NB];            // (read only when BIG)
            if (BIG && below) {
#pragma unroll
                for (int k = 0; k < NB; ++k) blk[k] = P[(t.diag + o + min(lane, bw - 1)) + (int64_t)(t.diag + NB * tt + k) * ld];
            }
            if (wave == tt) {
                if (pivpos) {
                    // the block's row interchanges, every column alike (through this wave's own part of `part`; one wave: LDS in order)
                    double* pw = part + wave * NB * SVM_LD;
                    const int g0 = t.first_col + t.diag + o;
                    if (lane < bw) {
                        const int q = pivpos[g0 + lane] - g0;
#pragma unroll
                        for (int c = 0; c < SVM_W; ++c) pw[q * SVM_LD + c] = xrow[c];
                    }
#pragma unroll
                    for (int c = 0; c < SVM_W; ++c) xrow[c] = (lane < bw) ? pw[lane * SVM_LD + c] : 0.0;
                }
                svm_chain<true>(a, dinv, xrow, lane);
                if (lane >= bw) {
#pragma unroll
                    for (int c = 0; c < SVM_W; ++c) xrow[c] = 0.0;
                }
            }
            if (BIG) {
                __syncthreads();
                if (below) svm_product<true>(blk, xs + NB * tt * SVM_LD, xrow);       // rows beyond b of sub-block tt hold 0
            }
        }
        if (lane < bw) {
#pragma unroll
            for (int c = 0; c < SVM_W; ++c) xq[(int64_t)lane * SVM_W + c] = xrow[c];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) sv_publish(sync + t.flag, 1);
        return;
    }
    // ---- row tile: lane = row, wave = 64-column chunk ----
    int nr = min(t.nrows, SV_ROWS);
    int r = t.row0 + min(lane, nr - 1);
    double lr[NB];
    if (bw > 0) SV_LOAD_TILE_ROW(lr, Lsx + t.panel + r + (int64_t)(t.diag + o) * ld, ld, bw)
    if (wave == 0) s_gi[lane] = Lsi[t.rows + r];
    if (tid == 0) sv_wait<16>(sync + t.flag, 1, info);
    __syncthreads();
    {
        const double* xb = x + (int64_t)(t.first_col + t.diag) * SVM_W;
        for (int e = tid; e < SV_B * SVM_W; e += 256) {
            const int rr = e / SVM_W, c = e % SVM_W;
            xs[rr * SVM_LD + c] = (rr < b) ? __builtin_nontemporal_load(xb + e) : 0.0;
        }
    }
    __syncthreads();
    double* prow = part + (wave * NB + lane) * SVM_LD;
    for (int g0 = 0;;) {
        if (bw > 0) svm_product<false>(lr, xs + o * SVM_LD, prow);      // columns beyond b meet xs = 0
        else {
#pragma unroll
            for (int c = 0; c < SVM_W; ++c) prow[c] = 0.0;
        }
        __syncthreads();
        for (int e = tid; e < SV_ROWS * SVM_W; e += 256) {
            const int rr = e / SVM_W, c = e % SVM_W;
            if (rr < nr)
                unsafeAtomicAdd(x + (int64_t)s_gi[rr] * SVM_W + c,
                                -(part[rr * SVM_LD + c] + part[(NB + rr) * SVM_LD + c] + part[(2 * NB + rr) * SVM_LD + c] +
                                  part[(3 * NB + rr) * SVM_LD + c]));
        }
        g0 += SV_ROWS;
        if (!BIG || g0 >= t.nrows) break;
        // (a far tile of several 64-row groups: the next group; x_blk stays in LDS)
        nr = min(t.nrows - g0, SV_ROWS);
        r = t.row0 + g0 + min(lane, nr - 1);
        if (bw > 0) SV_LOAD_TILE_ROW(lr, Lsx + t.panel + r + (int64_t)(t.diag + o) * ld, ld, bw)
        const int32_t gi = Lsi[t.rows + r];
        __syncthreads();                // part[] and s_gi[] of the previous group have been read
        if (wave == 0) s_gi[lane] = gi;
    }
}

// (one workgroup per CU as the register bound: at two, the BIG = false instantiation spills)
template <bool BIG>
__global__ void __launch_bounds__(256, 1)
k_solve_many_bwd(const SolveTask* __restrict__ tasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                 double* __restrict__ x, int* __restrict__ sync, int* __restrict__ ticket, int* __restrict__ info,
                 const double* __restrict__ Tbase) {
    __shared__ int s_ticket;
    __shared__ double xs[SV_B * SVM_LD];      // diagonal task: x_blk; row tile: the tile's x rows (SV_ROWS x SVM_W)
    __shared__ double acc_s[4 * NB * SVM_LD];  // row tile: the products, lane = column
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SolveTask t = sv_claim(tasks, ticket, s_ticket, tid);
    const int b = t.b;
    const int64_t ld = t.ld;
    const int o = NB * wave;
    const int bw = min(NB, max(0, b - o));
    if (t.nrows > 0) {
        // ---- row tile: x_blk[column, :] -= sum over the rows of L(row, column) x[row, :]; lane = column, wave = 64-column chunk
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
    // ---- diagonal task (k_solve_bwd's; x_blk in LDS, row o + lane = this lane's; lane = column of the block) ----
    const double* P = Lsx + t.panel;
    const double* __restrict__ Td = (Tbase && t.tdiag) ? Tbase + (t.tdiag - 1) : nullptr;
    double bcol[NB];
    if (bw > 0) {
        SV_LOAD_UPPER_COL(bcol, P, Td, ld, b, t.diag, o, bw, lane)
    } else {
        SV_LOAD_IDENTITY(bcol, lane)
    }
    double dinv = 1.0;
    SV_DINV(dinv, bcol, lane)
    if (t.expect > 0) {
        if (tid == 0) sv_wait<4>(sync + t.flag, t.expect, info);
        __syncthreads();
    }
    double* xq = x + (int64_t)(t.first_col + t.diag + o) * SVM_W;
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

// one wave per narrow supernode (k_solve_small_*), x_blk in this wave's part of LDS
__global__ void __launch_bounds__(256, 2)
k_solve_many_small_fwd(const SolveTask* __restrict__ tasks, int ntasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                       double* __restrict__ x, int unit, const int32_t* __restrict__ pivpos) {
    __shared__ double xs[4 * NB * SVM_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ti = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    if (ti >= ntasks) return;
    const SolveTask t = tasks[ti];
    const int b = t.b;
    const int64_t ld = t.ld;
    const double* P = Lsx + t.panel;
    double* xw = xs + wave * NB * SVM_LD;
    double* xrow = xw + lane * SVM_LD;
    double a[NB];
    SV_LOAD_LOWER_ROW(a, P, ld, 0, b, unit, lane)
    double* xq = x + (int64_t)t.first_col * SVM_W;
    {
        const double* src = xq + (int64_t)min(lane, b - 1) * SVM_W;
        // pivoting: row lane of x_blk goes to the row its interchanges gave it (rows >= b: zero, nothing moves there)
        const int q = (pivpos && lane < b) ? pivpos[t.first_col + lane] - t.first_col : lane;
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xw[q * SVM_LD + c] = (lane < b) ? src[c] : 0.0;
    }
    double dinv = 1.0;
    SV_DINV(dinv, a, lane)
    svm_chain<true>(a, dinv, xrow, lane);
    if (lane < b) {
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xq[(int64_t)lane * SVM_W + c] = xrow[c];
    } else {
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xrow[c] = 0.0;
    }
    // the rows below: 64 at a time, lane = row; x_blk read by broadcast out of LDS
    double acc[SVM_W];
    for (int r0 = b; r0 < (int)ld; r0 += NB) {
        const int row = min(r0 + lane, (int)ld - 1);
        SV_LOAD_TILE_ROW(a, P + row, ld, b)
        const int32_t gi = Lsi[t.rows + row];
        svm_product<false>(a, xw, acc);                   // rows >= b of xw hold 0
        if (r0 + lane < (int)ld) {
            double* xg = x + (int64_t)gi * SVM_W;
#pragma unroll
            for (int c = 0; c < SVM_W; ++c) unsafeAtomicAdd(xg + c, -acc[c]);
        }
    }
}

__global__ void __launch_bounds__(256, 2)
k_solve_many_small_bwd(const SolveTask* __restrict__ tasks, int ntasks, const double* __restrict__ Lsx, const int32_t* __restrict__ Lsi,
                       double* __restrict__ x) {
    __shared__ double xs[4 * NB * SVM_LD];     // the 64 rows' x being summed
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
    // D^T x_blk = x_blk - s, lane = column
    SV_LOAD_UPPER_COL(p, P, (const double*)nullptr, ld, b, 0, 0, b, lane)
    double dinv = 1.0;
    SV_DINV(dinv, p, lane)
    svm_chain<false>(p, dinv, xrow, lane);
    if (lane < b) {
#pragma unroll
        for (int c = 0; c < SVM_W; ++c) xq[(int64_t)lane * SVM_W + c] = xrow[c];
    }
}

// column-major n x cw (leading dimension n) <-> the row-major n x SVM_W block; pack zero-fills the columns [cw, SVM_W).
// Thread e = (column e / n, row e % n): the column-major side is read / written in coalesced runs.
__global__ void __launch_bounds__(256)
k_solve_many_pack(const double* __restrict__ Bc, int64_t n, int cw, double* __restrict__ X) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * SVM_W) return;
    const int64_t i = e % n;
    const int c = (int)(e / n);
    X[i * SVM_W + c] = (c < cw) ? Bc[i + (int64_t)c * n] : 0.0;
}

__global__ void __launch_bounds__(256)
k_solve_many_unpack(const double* __restrict__ X, int64_t n, int cw, double* __restrict__ Bc) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * cw) return;
    const int64_t i = e % n;
    const int c = (int)(e / n);
    Bc[i + (int64_t)c * n] = X[i * SVM_W + c];
}

void launch_solve_many_pack(const double* Bc, int64_t n, int cw, double* X, hipStream_t st) {
    const int64_t m = n * SVM_W;
    if (m > 0) hipLaunchKernelGGL(k_solve_many_pack, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, Bc, n, cw, X);
}
void launch_solve_many_unpack(const double* X, int64_t n, int cw, double* Bc, hipStream_t st) {
    const int64_t m = n * cw;
    if (m > 0) hipLaunchKernelGGL(k_solve_many_unpack, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, X, n, cw, Bc);
}

// ---- the step launchers: width 1 = the single-vector family on x[n], SVM_W = the block family on x[n][SVM_W] ----
static bool sv_single(int width) {
    assert(width == 1 || width == SVM_W);       // x has one of two layouts: any other width would run a kernel on the wrong one
    return width == 1;
}
void launch_solve_small_fwd(const SolveTask* t, int nt, int width, const double* Lsx, const int32_t* Lsi, double* x, int unit,
                            const int32_t* pivpos, hipStream_t st) {
    if (nt <= 0) return;
    hipLaunchKernelGGL(sv_single(width) ? k_solve_small_fwd : k_solve_many_small_fwd, dim3((nt + 3) / 4), dim3(256), 0, st, t, nt, Lsx, Lsi, x, unit,
                       pivpos);
}
void launch_solve_small_bwd(const SolveTask* t, int nt, int width, const double* Lsx, const int32_t* Lsi, double* x, hipStream_t st) {
    if (nt <= 0) return;
    hipLaunchKernelGGL(sv_single(width) ? k_solve_small_bwd : k_solve_many_small_bwd, dim3((nt + 3) / 4), dim3(256), 0, st, t, nt, Lsx, Lsi, x);
}
void launch_solve_fwd(const SolveTask* t, int nt, int width, int big, const double* Lsx, const int32_t* Lsi, double* x, int unit,
                      const int32_t* pivpos, int* sync, int* ticket, int* info, hipStream_t st) {
    if (nt <= 0) return;
    const auto k = sv_single(width) ? (big ? k_solve_fwd<true> : k_solve_fwd<false>) : (big ? k_solve_many_fwd<true> : k_solve_many_fwd<false>);
    hipLaunchKernelGGL(k, dim3(nt), dim3(256), 0, st, t, Lsx, Lsi, x, unit, pivpos, sync, ticket, info);
}
void launch_solve_bwd(const SolveTask* t, int nt, int width, int big, const double* Lsx, const int32_t* Lsi, double* x, int* sync, int* ticket,
                      int* info, hipStream_t st, const double* Tbase) {
    if (nt <= 0) return;
    const auto k = sv_single(width) ? (big ? k_solve_bwd<true> : k_solve_bwd<false>) : (big ? k_solve_many_bwd<true> : k_solve_many_bwd<false>);
    hipLaunchKernelGGL(k, dim3(nt), dim3(256), 0, st, t, Lsx, Lsi, x, sync, ticket, info, Tbase);
}

}  // namespace sf

// ---------------------------------------------------------------------------------------------------
// Host side: x <- (L L^T)^{-1} b (Cholesky, C:3036-3139) or (L U)^{-1} b (LU, L:3592-3700) with the resident factor, permuted
// space.  LU: unit-lower forward sweep over the L panels, backward sweep over the U^T panels (U x = y <=> (U^T)^T x = y).
// ---------------------------------------------------------------------------------------------------
SolveSync sf_solve_sync(const sf_chol_plan* p) {
    int* w = p->d_solve_sync;       // [info | n_solve_sync sync words | SOLVE_TICKETS tickets per step]
    return SolveSync{w, w ? w + 1 : nullptr, w ? w + 1 + p->n_solve_sync : nullptr, p->solve_sync_words() * sizeof(int)};
}

void sf_solve_step_fwd(sf_chol_plan* p, size_t k, const double* base, double* x, int width, const SolveSync& y, hipStream_t st) {
    const auto& s = p->solve_steps[k];
    const int32_t* piv = (p->lu && p->piv_tol > 0.0) ? p->d_piv : nullptr;
    const int unit = p->lu ? 1 : 0;
    int* tk = y.tickets + sf_chol_plan::SOLVE_TICKETS * k;
    if (s.small) {
        sf::launch_solve_small_fwd(p->d_solve + s.fwd_first, s.ndiag, width, base, p->d_Lsi, x, unit, piv, st);
    } else {
        sf::launch_solve_fwd(p->d_solve + s.fwd_first, s.fwd_count, width, s.big, base, p->d_Lsi, x, unit, piv, y.sync, tk, y.info, st);
    }
}

void sf_solve_step_bwd(sf_chol_plan* p, size_t k, const double* base, double* x, int width, const SolveSync& y, hipStream_t st) {
    const auto& s = p->solve_steps[k];
    int* tk = y.tickets + sf_chol_plan::SOLVE_TICKETS * k;
    if (s.small) {
        sf::launch_solve_small_bwd(p->d_solve + s.bwd_first, s.ndiag, width, base, p->d_Lsi, x, st);
    } else if (p->solve_bwd_fused) {
        sf::launch_solve_bwd(p->d_solve + s.bwd_first, s.count, width, s.big, base, p->d_Lsi, x, y.sync, tk + 1, y.info, st, p->d_solveT);
    } else {
        sf::launch_solve_bwd(p->d_solve + s.bwd_first, s.nrows_tasks, width, 0, base, p->d_Lsi, x, y.sync, tk + 1, y.info, st);
        sf::launch_solve_bwd(p->d_solve + s.bwd_first + s.nrows_tasks, s.count - s.nrows_tasks, width, s.big, base, p->d_Lsi, x, y.sync, tk + 2,
                             y.info, st, p->d_solveT);
    }
}

// transpose_diag: the row-major copies of the top steps' diagonal blocks, from the factor as it is now (117 MB at 128^3, ~0.1 ms)
void sf_solve_sweep_bwd(sf_chol_plan* p, double* x, int width, bool transpose_diag, const SolveSync& y, hipStream_t st) {
    const double* base = p->lu ? p->d_Lsx + p->xC : p->d_Lsx;
    if (transpose_diag) sf::launch_solve_transpose_diag(p->d_solve, p->d_solveT_list, p->n_solveT, base, p->d_solveT, st);
    for (size_t k = p->solve_steps.size(); k-- > 0;) sf_solve_step_bwd(p, k, base, x, width, y, st);
}

void sf_solve_sweeps(sf_chol_plan* p, double* x, int width, bool transpose_diag, hipStream_t st) {
    const SolveSync y = sf_solve_sync(p);
    for (size_t k = 0; k < p->solve_steps.size(); ++k) sf_solve_step_fwd(p, k, p->d_Lsx, x, width, y, st);
    sf_solve_sweep_bwd(p, x, width, transpose_diag, y, st);
}

int sf_solve_finish(sf_chol_plan* p, hipStream_t st) {
    int sinfo = 0;
    if (p->d_solve_sync) HIP_TRY(hipMemcpyAsync(&sinfo, p->d_solve_sync, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return sinfo ? SF_ERR_HIP : SF_OK;      // set: a bounded in-launch wait ran out (never seen)
}

extern "C" {

int sf_chol_plan_solve(sf_chol_plan* p, const sf_float* b_host, sf_float* x_host) {
    if (!p || !b_host || !x_host) return SF_ERR_ARG;
    if (p->partial || (p->nsuper > 0 && !p->d_solve)) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    if (p->fs.broken()) return SF_ERR_ARG;       // a failed downdate: no factor until the next factorization
    HIP_TRY(hipSetDevice(p->device));
    if (p->n <= 0) return SF_OK;
    const SfCols src{const_cast<double*>(b_host), p->n, false, nullptr}, dst{x_host, p->n, false, nullptr};
    SfStretch t{p};
    if (int rc = sf_apply_chunks(p, SfApply{&src, &dst, 1, 1, p->d_x, 0, true}, t,
                                 [&](double* x, sf_long, int) { return sf_apply_sweep(p, SF_SWEEP_SOLVE, x, 1, true); }))
        return rc;
    if (t.timed) p->last_solve_ms = t.total_ms;
    return SF_OK;
}

// X <- (L L^T)^{-1} B (LU: (L U)^{-1} B) for nrhs columns, SVM_W of them per forward + backward sweep.  A chunk goes H2D
// column-major into the staging half of d_xm (one copy when ldb == n, one 2-D copy otherwise), a small kernel transposes it
// into the row-major block the sweep kernels work on (zero columns pad a partial chunk), and the way back is the same in
// reverse (sf_apply_chunks).  Row-major on the device because every row a tile gathers or scatters through Lsi is then one
// 128-byte run; the transposes run on the device, where they cost two streaming passes over n x SVM_W doubles, instead of as
// strided host loops or 2-D copies with 8-byte pieces.
int sf_chol_plan_solve_many(sf_chol_plan* p, sf_long nrhs, const sf_float* B, sf_long ldb, sf_float* X, sf_long ldx) {
    if (!p || !B || !X || nrhs < 0) return SF_ERR_ARG;
    // (not sf_plan_whole_resident: this entry point has never looked at nranks)
    if (p->dry || p->partial || p->ooc_groups > 1 || (p->nsuper > 0 && !p->d_solve)) return SF_ERR_ARG;
    if (p->fs.broken()) return SF_ERR_ARG;
    const sf_long ldmin = std::max<sf_long>(p->n, 1);
    if (ldb < ldmin || ldx < ldmin) return SF_ERR_ARG;
    if ((const void*)X == (const void*)B && ldx != ldb) return SF_ERR_ARG;
    if (nrhs == 0 || p->n <= 0) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    if (int rc = sf_solve_many_block(p)) return rc;
    const SfCols src{const_cast<double*>(B), ldb, false, nullptr}, dst{X, ldx, false, nullptr};
    SfStretch t{p};
    // (the row-major copies of the diagonal blocks: once per call)
    if (int rc = sf_apply_chunks(p, SfApply{&src, &dst, nrhs, sf::SVM_W, p->d_xm, 0, true}, t,
                                 [&](double* x, sf_long j0, int) { return sf_apply_sweep(p, SF_SWEEP_SOLVE, x, sf::SVM_W, j0 == 0); }))
        return rc;
    p->last_solve_many_ms = t.total_ms;
    return SF_OK;
}

int sf_lu_plan_solve(sf_lu_plan* p, const sf_float* b_host, sf_float* x_host) { return (p && p->lu) ? sf_chol_plan_solve(p, b_host, x_host) : SF_ERR_ARG; }
int sf_lu_plan_solve_many(sf_lu_plan* p, sf_long nrhs, const sf_float* B, sf_long ldb, sf_float* X, sf_long ldx) {
    return (p && p->lu) ? sf_chol_plan_solve_many(p, nrhs, B, ldb, X, ldx) : SF_ERR_ARG;
}

}  // extern "C"
