// What the device solve's kernel files share (sf_solve.hip: x <- A^{-1} b; sf_solve_t.hip: the transposed backward sweep of
// x <- A^{-T} b): the ticket claim and the hand-off protocol as functions (sv_*), the fragments on a lane's register array as
// macros expanded in place (SV_*, see there for why), and the chain / product of the SVM_W-column family (svm_*).
#pragma once
#include "sf_kernels.h"
#include "sf_wave.h"

namespace sf {

constexpr int SV_SPIN_LIMIT = 1 << 22;

// the launch's next task in execution order (s_ticket: the kernel's LDS word)
__device__ __forceinline__ SolveTask sv_claim(const SolveTask* tasks, int* ticket, int& s_ticket, int tid) {
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return tasks[__builtin_amdgcn_readfirstlane(s_ticket)];
}

__device__ __forceinline__ void sv_publish(int* flag, int value) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread waits for *flag == value.  SLEEP = 16 for the forward tiles (hundreds of waiting workgroups poll ONE address: keep the
// L2 channel usable for its writer), 4 for the backward diagonal task (the one reader of its counter, on the critical path)
template <int SLEEP>
__device__ __forceinline__ void sv_wait(const int* flag, int value, int* info) {
    int spins = 0;
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != value) {
        __builtin_amdgcn_s_sleep(SLEEP);
        if (++spins > SV_SPIN_LIMIT) { atomicOr(info, 2); break; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// a backward tile has added its sums to x_blk: count it for the diagonal task
__device__ __forceinline__ void sv_tile_done(int* counter, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- the fragments that work on a lane's 64-entry register array are MACROS, not functions: a function that takes the array by
// reference is optimised on its own before it is inlined, and the kernels then come out with other schedules and register counts
// (one of them, the butterfly, with the array in scratch).  Expanded in place, the compiler sees the kernel as it was written out.
// Arguments are plain names or side-effect-free expressions; the loop variables end in an underscore.

// a[c] = D(lane, c): row `lane` of the bw x bw lower triangle (bw >= 1) at (d0, d0) of the panel P, padded to the 64 x 64 identity;
// unit: the diagonal is implied (LU: the L panel).  Unconditional loads from clamped addresses, then select (a load under a
// per-element condition becomes a branch plus its own s_waitcnt: 64 dependent round trips).
#define SV_LOAD_LOWER_ROW(a, P, ld, d0, bw, unit, lane)                                                               \
    _Pragma("unroll") for (int c_ = 0; c_ < NB; ++c_) {                                                              \
        const double v_ = (P)[((d0) + min(lane, (bw) - 1)) + (int64_t)((d0) + min(c_, (bw) - 1)) * (ld)];            \
        (a)[c_] = ((lane) < (bw) && c_ + (unit) <= (lane)) ? v_ : ((c_ == (lane)) ? 1.0 : 0.0);                      \
    }

// row / column `lane` of the 64 x 64 identity (a wave with no columns of the step)
#define SV_LOAD_IDENTITY(a, lane) \
    _Pragma("unroll") for (int c_ = 0; c_ < NB; ++c_) (a)[c_] = (c_ == (lane)) ? 1.0 : 0.0;

// D(r0 + min(k, br - 1), o + min(lane, bw - 1)) of the step's b x b diagonal block at (diag, diag) of P: entry k of a run down column
// `lane` of the sub-block at o (one contiguous run per lane: 64 cache lines per load instruction, ~7 us per block -- measured
// cheaper than coalesced row loads plus an in-wave transpose through LDS, which made the backward sweep 23 -> 36 ms).  Td != null:
// the block's ROW-major copy (steps of the top levels, t.tdiag, made at the start of the solve) -- then the run lies across the
// lanes, i.e. coalesced.
#define SV_COL_RUN(k, P, Td, ld, b, diag, r0, br, o, bw, lane)                                   \
    ((Td) ? (Td)[(int64_t)((r0) + min(k, (br) - 1)) * (b) + ((o) + min(lane, (bw) - 1))]         \
          : (P)[((diag) + (r0) + min(k, (br) - 1)) + (int64_t)((diag) + (o) + min(lane, (bw) - 1)) * (ld)])

// bcol[c] = D(o + c, o + lane), c >= lane: column `lane` of the sub-block's triangle (bw >= 1), padded to the identity
#define SV_LOAD_UPPER_COL(bcol, P, Td, ld, b, diag, o, bw, lane)                                                      \
    _Pragma("unroll") for (int c_ = 0; c_ < NB; ++c_) {                                                              \
        const double v_ = SV_COL_RUN(c_, P, Td, ld, b, diag, o, bw, o, bw, lane);                                     \
        (bcol)[c_] = ((lane) < (bw) && c_ < (bw) && c_ >= (lane)) ? v_ : ((c_ == (lane)) ? 1.0 : 0.0);               \
    }

// dinv = 1 / (the lane's own diagonal entry)
#define SV_DINV(dinv, a, lane) \
    _Pragma("unroll") for (int c_ = 0; c_ < NB; ++c_) dinv = (c_ == (lane)) ? 1.0 / (a)[c_] : dinv;

// lr[k] = Lr[min(k, bw - 1) * ld]: 64 entries of one panel row, the columns clamped to the bw the step has
#define SV_LOAD_TILE_ROW(lr, Lr, ld, bw) \
    _Pragma("unroll") for (int k_ = 0; k_ < NB; ++k_) (lr)[k_] = (Lr)[(int64_t)min(k_, (bw) - 1) * (ld)];

// p[0] <- sum over the 64 lanes of p[lane]: a transposing butterfly -- in the step with mask m a lane keeps the half of its
// array that matches its bit m and adds the partner's other half -- leaves lane l with the sum of ONE column after 63 exchanges
// instead of 64 full reductions (lane l ends with the column whose index has bit m set exactly where l has it: column l)
#define SV_BUTTERFLY64(p, lane)                                          \
    _Pragma("unroll") for (int m_ = 32; m_ >= 1; m_ >>= 1) {            \
        const bool up_ = ((lane) & m_) != 0;                             \
        _Pragma("unroll") for (int i_ = 0; i_ < m_; ++i_) {             \
            const double keep_ = up_ ? (p)[i_ + m_] : (p)[i_];           \
            const double give_ = up_ ? (p)[i_] : (p)[i_ + m_];           \
            (p)[i_] = keep_ + __shfl_xor(give_, m_, 64);                 \
        }                                                                \
    }

// substitution with a 64 x 64 triangle on the lane's entry v of ONE right-hand side.  FWD: a[j] = D(lane, j), from the first row
// down; else a[j] = D(j, lane) (the transpose), from the last row up.  (The 16-column family: svm_chain.)
#define SV_CHAIN(FWD, a, dinv, v, lane)                                                                          \
    _Pragma("unroll") for (int j_ = (FWD) ? 0 : NB - 1; (FWD) ? j_ < NB : j_ >= 0; j_ += (FWD) ? 1 : -1) {     \
        const double xj_ = readlane_f64(v, j_) * readlane_f64(dinv, j_);                                         \
        if ((lane) == j_) v = xj_;                                                                               \
        if ((FWD) ? (lane) > j_ : (lane) < j_) v -= (a)[j_] * xj_;                                               \
    }

// SV_LOAD_UPPER_COL with the diagonal implied (the L panel of an LU plan, whose stored diagonal and upper part are not L):
// bcol[c] = D(o + c, o + lane) for c > lane only, bcol[lane] = 1
#define SV_LOAD_UPPER_COL_UNIT(bcol, P, Td, ld, b, diag, o, bw, lane)                                                 \
    _Pragma("unroll") for (int c_ = 0; c_ < NB; ++c_) {                                                              \
        const double v_ = SV_COL_RUN(c_, P, Td, ld, b, diag, o, bw, o, bw, lane);                                     \
        (bcol)[c_] = ((lane) < (bw) && c_ < (bw) && c_ > (lane)) ? v_ : ((c_ == (lane)) ? 1.0 : 0.0);                \
    }

// ---- the SVM_W-column family: LDS rows are padded to SVM_LD doubles (sf_solve.hip, "The SVM_W-column family") ----
constexpr int SVM_LD = SVM_W + 2;
constexpr int SVM_CW = 4;

// SV_CHAIN on the SVM_W columns of the wave's rows (xrow = this lane's row in LDS), SVM_CW of them per pass
template <bool FWD>
__device__ __forceinline__ void svm_chain(const double (&a)[NB], double dinv, double* xrow, int lane) {
#pragma unroll 1
    for (int cg = 0; cg < SVM_W; cg += SVM_CW) {
        double v[SVM_CW];
#pragma unroll
        for (int c = 0; c < SVM_CW; ++c) v[c] = xrow[cg + c];
#pragma unroll
        for (int j = FWD ? 0 : NB - 1; FWD ? j < NB : j >= 0; j += FWD ? 1 : -1) {
            const double dj = readlane_f64(dinv, j);
#pragma unroll
            for (int c = 0; c < SVM_CW; ++c) {
                const double xj = readlane_f64(v[c], j) * dj;
                if (lane == j) v[c] = xj;
                if (FWD ? lane > j : lane < j) v[c] -= a[j] * xj;
            }
        }
#pragma unroll
        for (int c = 0; c < SVM_CW; ++c) xrow[cg + c] = v[c];
    }
}

// out[c] = sum_k w[k] S[k][c] (S in LDS, rows SVM_LD apart, read by broadcast); SUB: out[c] -= the sum
template <bool SUB>
__device__ __forceinline__ void svm_product(const double (&w)[NB], const double* S, double* out) {
#pragma unroll 1
    for (int cg = 0; cg < SVM_W; cg += SVM_CW) {
        double acc[SVM_CW];
#pragma unroll
        for (int c = 0; c < SVM_CW; ++c) acc[c] = 0.0;
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int c = 0; c < SVM_CW; ++c) acc[c] += w[k] * S[k * SVM_LD + cg + c];
#pragma unroll
        for (int c = 0; c < SVM_CW; ++c) {
            if (SUB) out[cg + c] -= acc[c];
            else out[cg + c] = acc[c];
        }
    }
}

}  // namespace sf
