// What the schedule of a plan is made of: the task descriptors that the host fills and the kernels read, and the tile and block
// constants both sides agree on.  No HIP here -- nothing but the host compiler's own headers -- so that the schedule builder
// (sf_schedule.cpp) and tools/schedule_sanitize.cpp compile without ROCm.  sf_kernels.h includes this file and adds everything
// that needs the runtime: PivotCtl and the launchers.
#pragma once
#include <cstdint>
#include <cstdlib>

// A/B switches of finished experiments (the alternative each one selects lost its measurement: DESIGN "Environment variables") are
// compiled OUT of release builds -- `make EXP=1` (-DSF_EXPERIMENTS) brings them back for re-measuring; sf_build_experiments() tells.
static inline const char* sf_exp_env(const char* name) {
#ifdef SF_EXPERIMENTS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

namespace sf {

constexpr int NB = 64;          // diagonal block size of the in-panel right-looking factorization
constexpr int OUTER_NB = 512;      // outer (left-looking) block-column width of the two-level panel factorization
constexpr int TRSM_ROWS = 256;  // rows per TRSM workgroup (one row per lane)
constexpr int ST_ROWS = 64;     // rows per workgroup of the fused 64-column step (k_step)
constexpr int GEMM_BM = 128;    // tile extent along ci (target rows; contiguous in memory)
constexpr int GEMM_BN = 128;    // tile extent along cj (target columns)
constexpr int GEMM_BK = 16;
constexpr int GEMM_WAVES = 8;     // waves per GEMM workgroup (2 along ci x GEMM_WAVES/2 along cj)
constexpr int GEMM_THREADS = 64 * GEMM_WAVES;
#ifndef SF_GEMM_GRID
#define SF_GEMM_GRID 512
#endif
constexpr int GEMM_GRID = SF_GEMM_GRID;   // persistent GEMM grid: 2 workgroups per CU x 256 CUs (the macro: experiment builds)
constexpr int GEMM_SLICE = 1 << 30;  // K steps per task (a tile's K range could be cut into slices; measured: it does not pay)
constexpr int SU_TM = 64, SU_TN = 32;   // tile of k_update_small (one wave): rows x columns
constexpr int SV_B = 256;         // columns per step of the device solve (4 sub-blocks of NB, one per wave)
constexpr int SV_ROWS = 64;       // rows per row tile of the device solve
constexpr int SU_MAXK = 64;      // Schur updates with K <= SU_MAXK go to k_update_small

// One C -= Y * X^T problem on rows of ONE source panel (column-major, leading dimension lda):
//   C[ci][cj] = sum_k src[y_off + ci + k*lda] * src[x_off + cj + k*lda],   0<=ci<M, 0<=cj<N, 0<=k<K
// only elements with ci >= cj are produced (lower trapezoid).
// mode 0 (panel):   target = Lsx[c_off + ci + cj*ldc], plain read-modify-write (tile owned by one workgroup)
// mode 1 (scatter): target = Lsx[c_off + rowmap(ci) + colmap(cj)*ldc] with the relative map of the
//                   source rows Lsi[src_rows + .] inside the target supernode's row list, fp64 atomic add.
struct GemmProb {
    int64_t y_off;      // doubles, into Lsx
    int64_t x_off;
    int64_t c_off;
    int64_t src_rows;   // index into Lsi of the source row id of ci = 0 (scatter mode)
    int64_t tgt_rows;   // index into Lsi of the target supernode's first below-diagonal row
    int32_t lda, ldc;
    int32_t M, N, K;
    int32_t tgt_first_col;  // Super[a]
    int32_t tgt_nscol;
    int32_t tgt_nbelow;     // nsrow_a - nscol_a
    int32_t strict;         // 1: only ci > cj is produced (LU: the L panel does not own the diagonal)
    int32_t pad_;
    int64_t map_off;        // scatter mode: offset of this (source, ancestor) pair's relative map (M entries) in RelMap
};

struct GemmTask {   // one 128x128 tile of a problem over ONE slice of its K range (k_update_small: a 64x32 tile, whole K)
    int32_t prob;
    uint16_t tm, tn;    // tile coordinates along ci / cj
    uint32_t kt0;       // first 16-deep K step of the slice
    uint32_t nkt;       // K steps in the slice
};

struct PotrfTask {  // factor the b x b diagonal block at (diag, diag) of a panel
    int64_t panel;      // doubles, into Lsx
    int32_t ld, diag, b;
    int32_t first_col;  // Super[s]: the block's rows are the global (permuted) indices first_col + diag + [0, b)  (LU pivot records)
};

struct TrsmTask {   // rows [row0, row0+nrows) of panel columns [diag, diag+b) <- X * D^{-T}
    int64_t panel;      // panel holding X
    int64_t dpanel;     // panel holding the triangular block D at (diag, diag) (same ld); Cholesky: == panel
    int32_t ld, diag, b;
    int32_t row0, nrows;
    int32_t unit;       // 1: D has an implicit unit diagonal (LU: U12^T <- U12^T * L11^{-T}); with pivoting the tile's columns are
                        // first brought into pivot order (they are rows of U)
    int32_t first_col;  // Super[s]
    int32_t pad;
};

struct StepTask {   // fused 64-column step on rows [row0, row0+nrows) of panel columns [diag, diag+b), updated by columns [J, diag)
    int64_t panel;          // panel of the tile (and of its own rows' operand)
    int64_t xpanel;         // panel of the other operand = the diagonal block's rows, and of the triangular block the rows are
                            // solved against (Cholesky: == panel; LU: the U^T panel for L rows and vice versa)
    int32_t ld, J, diag, b; // J: first column of the left-looking update (Cholesky diagonal tasks: J == diag, their block is kept
                            // up to date right-looking by the row tasks' pushes, see next_b)
    int32_t row0, nrows;    // row0 == diag: the diagonal block (POTRF / GETRF, publishes `flag`); else rows below it (wait for `flag`)
    int32_t flag;           // index of this (panel, step)'s flag
    int32_t mode;           // bit 0: the triangular block has an implicit unit diagonal (LU: U12^T <- U12^T L11^{-T})
    int32_t slot;           // index (within the launch) of the diagonal task whose 16 x 16 inverses the rows use
    int32_t next_b;         // row task, Cholesky: > 0 = these rows are a future diagonal block of the outer block, next_b wide:
                            // push X X^T into it
    int32_t first_col;      // Super[s] (LU pivot records)
    int32_t pad;
};

// LU download without a gather kernel: PL(R, j) <- PU(j, R) for R <= j inside a supernode's diagonal block, i.e. the L panel
// receives the reference's packed L11 \ U11 (L:2514-2517).  One workgroup per 64 x 64 tile: rows [r0, r0 + 64), columns
// [max(c0, cb), min(c0 + 64, ce)), transposed through LDS.  Nothing reads that part of an L panel (the solves mask it by index).
struct FillTile { int64_t xp; int32_t nsrow, r0, c0, cb, ce; };

// ---- device-side supernodal triangular solves with the resident factor (sf_solve.hip; reference: scalar host loops,
// Cholesky/Source/SparseFrame.c:3074-3134).  SV_B-column steps level by level; one launch per step and direction, the
// diagonal solve (one workgroup, wave w = 64-column sub-block w) and the SV_ROWS-row tiles hand over inside the launch.
struct SolveTask {
    int64_t panel;      // doubles, into Lsx
    int64_t rows;       // index into Lsi of the supernode's row list
    int32_t ld, diag, b;    // the step's columns [diag, diag + b), b <= SV_B
    int32_t row0, nrows;    // row tile: rows [row0, row0 + nrows) of the panel (below the block), nrows <= SV_ROWS; nrows == 0: the diagonal task
    int32_t first_col;      // Super[s]
    int32_t flag;           // index into the solve's sync words: forward = "x_blk is solved" flag, backward = tile counter
    int32_t expect;         // backward diagonal task: number of row tiles to wait for
    int64_t tdiag;          // backward diagonal task: 1 + offset (doubles) of the step's diagonal block stored ROW by row (b x b) in the
                            // solve's scratch, 0: none -- the task then reads the block's columns out of the panel
};
// width of the multi-right-hand-side family of the solve kernels (sf_chol_plan_solve_many): SVM_W right-hand sides per sweep, x an
// n x SVM_W block stored ROW-major (x[i * SVM_W + c]).  16 = the N of v_mfma_f64_16x16x4f64.
constexpr int SVM_W = 16;

}  // namespace sf
