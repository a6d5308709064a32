// Kernel launchers for the supernodal Cholesky / LU numeric phase (gfx950).  The task descriptors the launchers take and the tile
// constants are in sf_tasks.h, which needs no HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "sf_tasks.h"

namespace sf {

// LU pivoting (the reference never pivots, L:2653 / L:3344, and keeps a disabled static pre-pivot,
// L:589-673): threshold partial pivoting RESTRICTED to the 64 x 64 diagonal block of a step -- the symbolic structure is
// static, rows outside the block cannot be exchanged -- with a perturbation fallback.
//   tol  > 0 : at column j the natural row keeps the pivot while |a_jj| >= tol * max_i |a_ij| (i over the block's rows not
//              yet used); otherwise the row of the largest entry takes it.  tol = 0: no pivoting (the reference's behaviour).
//   eps  > 0 : a pivot smaller than eps in magnitude is replaced by +-eps (counted in *nperturb); eps = 0: a zero pivot is an
//              error (info bit 0) as before.
//   pivpos[g] = position (global index, inside the same block) that original row g of the block ends up in; pivinv = inverse.
// Only the block's rows of the block's own columns and of the columns to its RIGHT move (the U rows); the L entries to the
// left of the block stay where they are, so the interchanges are applied LINPACK-style, block by block, in the forward solve.
struct PivotCtl {
    double tol, eps;
    int32_t* pivpos;    // n entries each, or nullptr when tol == 0 (then no record is written: positions are the identity)
    int32_t* pivinv;
    int* nperturb;
};

// skip_diag != 0: entries with row == column are not stored (LU: the L panel)
void launch_build_loadmap(const int64_t* Lp, const int32_t* Li, int32_t n, const int32_t* Super, const int32_t* SuperMap,
                          const int64_t* Lsip, const int32_t* Lsi, const int64_t* Lsxp, int64_t base, int skip_diag, int64_t* map, hipStream_t st);
// map[drop[k]] = -1 for k < count: entries that a later duplicate in their column supersedes (last one wins, as in the sequential walk)
void launch_loadmap_drop(const int64_t* drop, int64_t count, int64_t* map, hipStream_t st);
void launch_load_mapped(const double* Lx, const int64_t* map, int64_t nnz, double* Lsx, hipStream_t st);
void launch_load_panels(const int64_t* Lp, const int32_t* Li, const double* Lx, int32_t n,
                        const int32_t* Super, const int32_t* SuperMap, const int64_t* Lsip, const int32_t* Lsi,
                        const int64_t* Lsxp, double* Lsx, int skip_diag, const int8_t* load_mask, hipStream_t st);
void launch_potrf(const PotrfTask* tasks, int ntasks, double* Lsx, int* info, hipStream_t st);
// LU: the diagonal block is split over two panels, L (strictly lower, at Lsx + task.panel) and U^T (lower
// including the diagonal, at Lsx + task.panel + u_shift)
void launch_getrf(const PotrfTask* tasks, int ntasks, double* Lsx, int64_t u_shift, int* info, PivotCtl pc, hipStream_t st);
// LU: gather the (L, U^T) panel pairs into the reference's (2*nsrow - nscol) x nscol panels (LU/Source/SparseFrame.c:2514-2517):
// values [e_begin, e_end) of that layout -> out[0 .. e_end - e_begin)
void launch_factor_hash(const int32_t* Super, const int64_t* Lsip, const int64_t* Xp, const int64_t* RefXp, int32_t nsuper,
                        const double* PL, const double* PU, int lu, int64_t total, unsigned long long* H, hipStream_t st);
void launch_lu_fill_u11(const FillTile* tiles, int64_t ntiles, double* PL, const double* PU, hipStream_t st);
void launch_pack_lu(const int32_t* Super, const int64_t* Lsip, const int64_t* Xp, const int64_t* RefXp, int32_t nsuper,
                    const double* PL, const double* PU, double* out, int64_t e_begin, int64_t e_end, hipStream_t st);
// pivinv != nullptr (LU with pivoting): the unit tasks (U^T rows) permute their columns by the block's interchanges first
void launch_trsm(const TrsmTask* tasks, int ntasks, double* Lsx, const int32_t* pivinv, hipStream_t st);
// tasks: the diagonal blocks first, then the 64-row tiles below them, any number (the grid need not be co-resident:
// workgroups claim tasks in execution order through *ticket, which must be 0 at launch and is private to the launch);
// flags[task.flag] == epoch once that diagonal block is factored
// lu != 0: the diagonal tasks hold (L panel, U^T panel) and are factored without pivoting
// tinv: scratch for the 16 x 16 inverses, 1024 (Cholesky) / 2048 (LU: of U11^T, then of L11) doubles per diagonal task of the launch
void launch_step(const StepTask* tasks, int ntasks, int lu, double* Lsx, int* flags, int epoch, int* info, double* tinv, int* ticket,
                 PivotCtl pc, hipStream_t st);
// One-time (plan creation): relative maps of all scatter problems [first, first+count) -- the device form of the
// reference's createRelativeMap (cuda_kernel.cu:42-60): RelMap[map_off + ci] = position of source row ci in the
// target supernode's row list.
void launch_build_relmaps(const GemmProb* probs, int nprobs, const int32_t* Lsi, int32_t* RelMap, hipStream_t st);

// kt_prefix[0..ntasks]: running count of 16-deep K steps of the launch's tiles (kt_prefix[ntasks] = total units);
// this call executes the units [u_lo, u_hi) of the launch.  ticket: 8 zeroed counters (one per XCD) for the dynamic deal of
// the whole-tile rounds, or nullptr for the static deal; whole_tiles != 0 (only with u_lo = 0, u_hi = all units): no tile is split by
// units -- an order-independent (bit-reproducible) result, for launches that several ranks execute redundantly
void launch_gemm(const GemmProb* probs, const GemmTask* tasks, const uint32_t* kt_prefix, int ntasks, uint32_t u_lo, uint32_t u_hi,
                 int mode, double* Lsx, const int32_t* RelMap, int* ticket, hipStream_t st, int whole_tiles = 0, int grid_cap = 0);

// Schur updates with K <= SU_MAXK: tasks are SU_TM x SU_TN tiles (GemmTask.tm / .tn in those units), one wave each
void launch_update_small(const GemmProb* probs, const GemmTask* tasks, int ntasks, double* Lsx, const int32_t* RelMap, hipStream_t st);

// ---- device-side supernodal triangular solves with the resident factor (sf_solve.hip; SolveTask: sf_tasks.h) ----
// forward launch: tasks = the step's diagonal tasks, then its row tiles; backward launch: the row tiles, then the diagonal
// tasks.  sync: one word per (panel, step) and direction, zero at the start of the solve; ticket: zero, private to the launch
// pivpos != nullptr (LU with pivoting): x_blk is brought into the block's pivot order before the unit-lower solve
// steps whose panels are all narrow (nscol <= 64): one wave per supernode does its diagonal solve and all its rows, no
// hand-off; tasks = the step's diagonal tasks only (task.ld = nsrow, task.b = nscol)
// width: 1 = the single-vector kernels on x[n]; SVM_W = the multi-right-hand-side family (sf_chol_plan_solve_many): the same
// tasks, schedule and sync words, SVM_W right-hand sides per sweep, x an n x SVM_W block stored ROW-major (x[i * SVM_W + c]).
// 16 = the N of v_mfma_f64_16x16x4f64.
void launch_solve_small_fwd(const SolveTask* t, int nt, int width, const double* Lsx, const int32_t* Lsi, double* x, int unit,
                            const int32_t* pivpos, hipStream_t st);
void launch_solve_small_bwd(const SolveTask* t, int nt, int width, const double* Lsx, const int32_t* Lsi, double* x, hipStream_t st);
// big != 0: some panel of the step has more than one 64-column sub-block (the variant with the prefetch registers)
void launch_solve_fwd(const SolveTask* t, int nt, int width, int big, const double* Lsx, const int32_t* Lsi, double* x, int unit,
                      const int32_t* pivpos, int* sync, int* ticket, int* info, hipStream_t st);
void launch_solve_bwd(const SolveTask* t, int nt, int width, int big, const double* Lsx, const int32_t* Lsi, double* x, int* sync, int* ticket,
                      int* info, hipStream_t st, const double* Tbase = nullptr);
// row-major copies of the diagonal blocks of the backward diagonal tasks list[0 .. ntasks) (indices into `tasks`) into T
void launch_solve_transpose_diag(const SolveTask* tasks, const int64_t* list, int64_t ntasks, const double* Lsx, double* T, hipStream_t st);

// the transposed backward sweep over the L panels of an LU plan (sf_solve_t.hip): launch_solve_small_bwd's / launch_solve_bwd's task
// lists, sync words and tickets; the diagonal is implied, and with pivpos != nullptr a block's interchanges are undone after its chain
void launch_tsolve_small_bwd(const SolveTask* t, int nt, int width, const double* Lsx, const int32_t* Lsi, double* x, const int32_t* pivpos,
                             hipStream_t st);
void launch_tsolve_bwd(const SolveTask* t, int nt, int width, int big, const double* Lsx, const int32_t* Lsi, double* x,
                       const int32_t* pivpos, int* sync, int* ticket, int* info, hipStream_t st, const double* Tbase);

// ---- the 1-norm condition estimate's device steps (sf_solve_t.hip, sf_*_plan_condest) ----
struct CondScalars { double nrm; int32_t flags, j; };      // flags: bit 0 = sign vector unchanged, bit 1 = x was the safeguard vector,
                                                            // bit 2 = the info word of the sweeps before (a bounded wait ran out)
// mode 0: x = 1 / n;  mode 2: the safeguard vector x_i = (-1)^i (1 + i / (n - 1)), n > 1
void launch_condest_fill(double* x, int64_t n, int mode, hipStream_t st);
// s->nrm = |y|_1, bit 0 of s->flags = (sign(y) == xi everywhere), bit 2 = (*solve_info != 0), bit 1 kept; then xi = y = sign(y)
void launch_condest_sign_norm(double* y, double* xi, int64_t n, const int* solve_info, CondScalars* s, hipStream_t st);
// s->j = the first index of the largest |x_i|; x = e_j, or (stopping: s->flags = 2) the safeguard vector; n > 1
void launch_condest_argmax_next(double* x, int64_t n, CondScalars* s, int first, int last, hipStream_t st);

// column-major n x cw (leading dimension n) -> row-major n x SVM_W, columns [cw, SVM_W) zero; and back (columns [0, cw) only)
void launch_solve_many_pack(const double* Bc, int64_t n, int cw, double* X, hipStream_t st);
void launch_solve_many_unpack(const double* X, int64_t n, int cw, double* Bc, hipStream_t st);

// ---- half solves, quadratic forms, sampling (sf_sample.hip; the sweeps are the launchers above) ----
// X[i][c] = the standard normal (i, s0 + c) of the stream `seed` for c < cw, 0 for cw <= c < SVM_W: the row-major n x SVM_W block
void launch_sample_fill(double* X, int64_t n, int cw, uint64_t seed, uint64_t s0, hipStream_t st);
// per-column sums of squares of the row-major n x width block X (width 1 or SVM_W), two passes in a fixed order; scratch:
// QF_MAXB x width parts, then the `width` results
constexpr int QF_MAXB = 1024;
void launch_quadform(const double* X, int64_t n, int width, double* scratch, hipStream_t st);

// ---- device-pointer loads and stores (sf_device_io.hip; called by sf_apply.hip): perm != nullptr gathers / scatters row perm[i] of
// the caller's block ----
// x[i] = B[perm ? perm[i] : i], and X[perm ? perm[i] : i] = x[i]
void launch_dev_load1(const double* B, const int32_t* perm, int64_t n, double* x, hipStream_t st);
void launch_dev_store1(const double* x, const int32_t* perm, int64_t n, double* X, hipStream_t st);
// the caller's column-major chunk of cw <= SVM_W columns -> the row-major n x SVM_W block X, columns [cw, SVM_W) zero
void launch_dev_pack(const double* B, int64_t ldb, const int32_t* perm, int64_t n, int cw, double* X, hipStream_t st);
// and back: the columns [0, cw) of the block into the caller's chunk D
void launch_dev_unpack(const double* X, const int32_t* perm, int64_t n, int cw, double* D, int64_t ldx, hipStream_t st);
// values in the plan's order: out[p] = map[p] >= 0 ? Ax[map[p]] : 0.0 for p < count
void launch_dev_gather_values(const double* Ax, const int64_t* map, int64_t count, double* out, hipStream_t st);
// part[blk] = max |v[k]| over the entries workgroup blk strides over (a NaN is dropped); returns the number of parts written,
// DIO_MAXB at most (0: count <= 0, nothing launched)
constexpr int DIO_MAXB = 1024;
int launch_dev_absmax(const double* v, int64_t count, double* part, hipStream_t st);

// ---- the Gram matrix Y^T Y of the chunks of a half-solved border (sf_gram.hip, sf_chol_plan_gram) ----
constexpr int GRAM_SLAB_ROWS = 2048;    // rows of a slab, about
constexpr int GRAM_MAX_SLABS = 256;     // slabs (workgroups per tile, parts per tile) at most
// slabs the rows [0, n) are cut into, *slab_rows = rows of each (a multiple of 64); n >= 1
int gram_slabs(int64_t n, int64_t* slab_rows);
// chunk row a of G = Y^T Y: the tiles (a, 0 .. a) and their mirrors into the column-major k x k result G (leading dimension ldg).
// Y: the chunks 0 .. a, chunk c the row-major n x SVM_W block at c * n * SVM_W; part: (a + 1) x gram_slabs x 256 doubles
void launch_gram_row(const double* Y, int64_t n, int a, int64_t k, double* part, double* G, int64_t ldg, hipStream_t st);

// ---- C^T A^{-1} B = Z^T Y with an LU plan (sf_gram_lu.hip, sf_lu_plan_gram) ----
// chunk column b of G = Z^T Y: the tiles (0 .. nza - 1, b) into the column-major m x k result G (leading dimension ldg).  Z: nza
// row-major n x SVM_W blocks, block a at a * n * SVM_W; Yb: the one block of chunk b; part: nza x gram_slabs x 256 doubles
void launch_gram2_col(const double* Z, const double* Yb, int64_t n, int nza, int b, int64_t m, int64_t k, double* part, double* G,
                      int64_t ldg, hipStream_t st);
// *out = sum_i x[i] y[i], two passes in a fixed order; scratch: QF_MAXB parts, out may follow them
void launch_dot(const double* x, const double* y, int64_t n, double* scratch, double* out, hipStream_t st);

// ---- selected inversion (sf_selinv.hip, sf_chol_plan_selinv) ----
// one unit: columns [cb, cb + w) of the supernode whose panel starts at lx (factor and arena share the layout), rows at Lsi[rows ..]
struct SelUnit {
    int64_t lx, rows;
    int32_t nsrow, ncol, cb, w;
    int32_t pair0, npair;       // the supernode's scatter problems (J, a) in the pair table, by first row
};
struct SelPair { int64_t map_off; int32_t i; int32_t pad_; };     // problem (J, a): relative map at map_off, J's rows from panel row i
constexpr int SEL_UW = OUTER_NB;      // unit width of the wide supernodes
constexpr int SEL_SMALL_W = 64;       // narrow supernodes (one workgroup each): nscol <= SEL_SMALL_W,
constexpr int SEL_SMALL_M = 512;      // rows below <= SEL_SMALL_M,
constexpr int SEL_SMALL_Y = 4096;     // (rows below) x nscol <= SEL_SMALL_Y
constexpr int SEL_MAX_SLABS = 16;     // K slabs of the split products

// the structure arrays Sigma(R,R) is addressed through (device pointers).  Xp: the panels' offsets in the arena and in the factor
// (Lsxp of a Cholesky plan, Xp of an LU plan); pairs / relmap: the scatter problems' table and relative maps
struct SelStruct {
    const int32_t *Super, *SuperMap;
    const int64_t* Lsip;
    const int32_t* Lsi;
    const int64_t* Xp;
    const SelPair* pairs;
    const int32_t* relmap;
};
// one launch each, on the kernels of sf_selinv.hip / sf_selinv_lu.hip; the plans' entry points run these and nothing else
void launch_selinv_small(const SelUnit* units, int nunits, const double* Lsx, double* S, const SelStruct& t, hipStream_t st);
void launch_selinv_trinv(const SelUnit& u, const double* Lsx, double* Linv, hipStream_t st);
// C (M x N, ldc) = op(A) B (+ C when acc_in), am = 0: A plain, 1: A = X^T, 2: A = Sigma(R,R) of unit u gathered from (S, S2); K cut
// into `slabs` slabs of kslab = the share of a slab rounded up to 16, slab z written to C + z cstride (a slab past K: zeros)
void launch_selinv_gemm(int am, int M, int N, int K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                        int slabs, int64_t cstride, int acc_in, const SelUnit& u, const double* S, const double* S2, const SelStruct& t,
                        hipStream_t st);
// dst[e] (+)= sum_{z < nslab} src[z * stride + e], e < count, z in increasing order
void launch_selinv_sum(const double* src, int nslab, int64_t stride, int64_t count, double* dst, int acc_in, hipStream_t st);
void launch_selinv_finish(const SelUnit& u, const double* Z, const double* Sc, double* S, hipStream_t st);
void launch_selinv_diag(int64_t n, const double* S, const SelStruct& t, double* d, hipStream_t st);
// buf: ceil(n / 256) partial sums, then the result 2 sum log L_jj
void launch_logdet(int64_t n, const double* Lsx, const SelStruct& t, double* buf, hipStream_t st);
void launch_lu_selinv_small(const SelUnit* units, int nunits, const double* PL, const double* PU, double* SL, double* SU, const SelStruct& t,
                            hipStream_t st);
void launch_lu_selinv_trinv(const SelUnit& u, const double* P, int unit, double* Tinv, hipStream_t st);
void launch_lu_selinv_finish(const SelUnit& u, const double* Zl, const double* Zu, const double* Sc, double* SL, double* SU, hipStream_t st);
// RefXp: the packed panels' offsets (nsuper + 1)
void launch_lu_selinv_pack(const SelStruct& t, const int64_t* RefXp, int32_t nsuper, const double* SL, const double* SU, double* out,
                           int64_t e_begin, int64_t e_end, hipStream_t st);
void launch_lu_selinv_diag(int64_t n, const double* SL, const SelStruct& t, double* d, hipStream_t st);
// buf: ceil(n / 256) partial sums, then sum log|U_jj| and the parity of the negative U_jj (as a double); neg: ceil(n / 256) counts
void launch_lu_logdet(int64_t n, const double* PU, const SelStruct& t, double* buf, int32_t* neg, hipStream_t st);

// ---- adjoints on the pattern of A (sf_adjoint.hip, sf_*_plan_adjoint_values / _logdet_grad_values) ----
// The marks of a position p at (row i, column j) of a structure: which of the two products its output collects.
constexpr uint8_t ADJ_A = 1;                            // Y[i, c] X[j, c]: the assembly puts V[p] at M(i, j)
constexpr uint8_t ADJ_B = 2;                            // Y[j, c] X[i, c]: ... at M(j, i)
// how launch_adj_index marks a position from the load maps (map < 0: the assembly does not read the position)
enum AdjSide {
    ADJ_SIDE_CHOL = 0,      // live: A, and B too off the diagonal
    ADJ_SIDE_LU_L = 1,      // live in mapA: A
    ADJ_SIDE_LU_ALIAS = 2,  // live in mapA (L's map): A; live in mapB (U's map over the same structure): B, on the diagonal A
    ADJ_SIDE_LU_U = 3,      // (ptr, idx) = U by rows; live in mapA: B
};
// one launch each, thread = position, 256 threads per workgroup; count <= 0: nothing launched
// col[p] = the column (U: row) j with ptr[j] <= p < ptr[j + 1], mark[p] as AdjSide says; p < count = ptr[n]
void launch_adj_index(const int64_t* ptr, const int32_t* idx, int32_t n, int64_t count, int side, const int64_t* mapA, const int64_t* mapB,
                      int32_t* col, uint8_t* mark, hipStream_t st);
// out[p] = alpha * sum_{c < k} ([A] Y[r(i), c] X[r(j), c] + [B] Y[r(j), c] X[r(i), c]), i = idx[p], j = col[p], r = perm or the identity
// (perm null); ascending c, one fma per product, A before B; mark[p] == 0 or k == 0: +0.0.  Y, X column-major.
void launch_adj_values(const int32_t* idx, const int32_t* col, const uint8_t* mark, int64_t count, const int32_t* perm, int k, const double* Y,
                       int64_t ldy, const double* X, int64_t ldx, double alpha, double* out, hipStream_t st);
// out[p] = alpha * ((mapA[p] >= 0 ? w S[mapA[p] + shiftA] : nothing) + (mapB && mapB[p] >= 0 ? S[mapB[p] + shiftB] : nothing)), w = 2
// where mark[p] has both ADJ_A and ADJ_B and twice is set, else 1; neither live: +0.0
void launch_adj_logdet(const int64_t* mapA, int64_t shiftA, const int64_t* mapB, int64_t shiftB, const uint8_t* mark, int twice, int64_t count,
                       const double* S, double alpha, double* out, hipStream_t st);
// out[s] = 0.0 + tmp[list[sptr[s]]] + ... + tmp[list[sptr[s + 1] - 1]] in that order, s < nsrc
void launch_adj_scatter(const int64_t* sptr, const int64_t* list, int64_t nsrc, const double* tmp, double* out, hipStream_t st);

// ---- Sigma on the pattern of A (sf_selinv_pattern.hip, sf_*_plan_selinv_values / _trace / _entries) ----
constexpr int SELPAT_CHUNK = 8;                         // columns of V a lane keeps partial sums for at a time (registers, no scratch)
constexpr int SELPAT_EPT = 8;                           // entries per lane: that many independent map -> Sigma gathers in flight
constexpr int SELPAT_TILE = 256 * SELPAT_EPT;           // entries per workgroup = per part
constexpr int SELPAT_MAX_M = 64;                        // value arrays per call
constexpr int64_t SELPAT_ENT_CHUNK = (int64_t)1 << 16;  // (row, column) pairs per trip through the staging buffer
constexpr int SELPAT_GATHER_GRID = 256 * 16;            // workgroups of the gather at most: it strides above 256 times that many entries
// one launch each, on the kernels of sf_selinv_pattern.hip; the plans' entry points run these and nothing else
// pos[p] = the offset of entry p of the structure (Lp, Li) in one panel set (Xp: the panels' offsets), offd[p] = (row != column)
// when offd is not null; n <= 0: nothing launched
void launch_selpat_build(const int64_t* Lp, const int32_t* Li, int32_t n, const int32_t* Super, const int32_t* SuperMap, const int64_t* Lsip,
                         const int32_t* Lsi, const int64_t* Xp, int64_t* pos, uint8_t* offd, hipStream_t st);
// out[p] = S[pos[p]], p < count
void launch_selpat_gather(const int64_t* pos, int64_t count, const double* S, double* out, hipStream_t st);
// part[t * nparts + part0 + b] = sum over the entries p of tile b of w_p S[map[p] + shift] V_t[p], t < m, b < ceil(count / SELPAT_TILE);
// map[p] < 0: the entry is skipped; offd: null or the marks of w_p = 2; mapped: V_t[p] = V[vmap[p] + t ldv] (vmap[p] < 0: 0), otherwise
// V[p + t ldv].  Returns the number of workgroups (= parts per column) launched; count <= 0: 0, nothing launched
int64_t launch_selpat_part(bool mapped, const int64_t* map, const uint8_t* offd, int64_t count, const double* S, int64_t shift, const double* V,
                           int64_t ldv, const int64_t* vmap, int m, double* part, int64_t part0, int64_t nparts, hipStream_t st);
// out[t] = the sum of part[t * nparts .. + nparts) in the fixed order of k_selpat_final, t < m
void launch_selpat_final(const double* part, int64_t nparts, int m, double* out, hipStream_t st);
// out[k] = Sigma(rows[k], cols[k]), k < count, a quiet NaN outside the pattern, counted in *outside (added to what it holds);
// lu != 0: i >= j from S, i < j from S + xC
void launch_selpat_entries(const int64_t* rows, const int64_t* cols, int64_t count, int lu, int64_t xC, const double* S, const SelStruct& t,
                           double* out, unsigned long long* outside, hipStream_t st);

void launch_noop(hipStream_t st);

// ---- residual and iterative refinement (sf_refine.hip, sf_chol_plan_residual / sf_chol_plan_refine) ----
// A by rows (or by columns): run i = entries [ptr[i], ptr[i + 1]), entry e = (index col[e], value Vd[pos[e]] when pos[e] >= 0,
// Vt[~pos[e]] otherwise) -- positions into the plan's value arrays, never copies of the values
struct RefineForm {
    const int64_t* ptr;
    const int32_t* col;
    const int64_t* pos;
    const double *Vd, *Vt;
};
// r = b - A x and w = |A| |x| + |b|, one pass over the rows, a fixed summation order (no floating-point atomics)
void launch_refine_resid(const RefineForm& rows, int64_t n, const double* x, const double* b, double* r, double* w, hipStream_t st);
// *amax = max over the runs of the form of sum |value| (zero it first): |A|_1 from the column form
void launch_refine_abs_sums(const RefineForm& f, int64_t n, double* amax, hipStream_t st);
// s[0] = max_i |r_i| / w_i over w_i > 0, s[1] = |r|_inf, s[2] = |x|_inf, s[3] = |b|_inf, s[4] = flag word (bit 0: a non-finite r_i,
// x_i or b_i; bit 1: *solve_info != 0); zero the five words first
void launch_refine_norms(int64_t n, const double* r, const double* w, const double* x, const double* b, const int* solve_info, double* s,
                         hipStream_t st);
// save != 0: best <- x first; then x += d
void launch_refine_update(int64_t n, double* x, const double* d, double* best, int save, hipStream_t st);

// device twin of SparseFrame_validate's residual (C:3182-3263): b_i = 1 + i/n is written to b, r = A x - b, the four maxima
// |r|_inf, |A|_1, |x|_inf, |b|_inf to norms[0..3] (zero them first).  Up == nullptr: (Lp, Li, Lx) is one triangle used symmetrically.
void launch_residual(const int64_t* Lp, const int32_t* Li, const double* Lx, const int64_t* Up, const int32_t* Ui, const double* Ux,
                     int32_t n, const double* x, double* r, double* colsum, double* b, double* norms, hipStream_t st);

// ---- rank-k update / downdate of the resident Cholesky factor (sf_updown.hip) ----
// W: the row-major n x UPD_W block of the update's columns (zero outside their pattern); rot: UPD_B x UPD_W pairs (c, s), pair
// (j, t) at rot[2 (j UPD_W + t)]; kw: the columns in use rounded up to a power of two (1, 2, 4, 8 or 16 -- the columns behind the
// chunk are zero and rotate nothing); sign: +1 update, -1 downdate.
constexpr int UPD_W = 16, UPD_B = 64;
// W[dest[q]] = val[q], q < count
void launch_updown_scatter(const int64_t* dest, const double* val, int64_t count, double* W, hipStream_t st);
// One launch of one wave on the b x b (b <= UPD_B) diagonal block D (column-major, leading dimension ld; only its lower triangle is
// read and written) whose first column is col0: the b kw rotations in (j, t) order, the pairs to rot, zeros to the rows
// [col0, col0 + b) of W.  A rotation whose radicand is not positive sets *info to 1 and it and every later one -- of this launch and,
// *info being read first, of every later launch -- is the identity.
void launch_updown_diag(double* D, int64_t ld, int b, int kw, int sign, double* W, int64_t col0, double* rot, int* info, hipStream_t st);
// The same rotations, read from rot, on the nrows panel rows below the block: row i of P (column-major, leading dimension ld, b
// columns) with row rows[i] of W.  rows[] are distinct.
void launch_updown_rows(double* P, int64_t ld, int b, int64_t nrows, const int32_t* rows, int kw, int sign, double* W, const double* rot,
                        hipStream_t st);

// ---- row deletion / addition on the resident Cholesky factor (sf_rowmod.hip); W, UPD_W, UPD_B as above, column 0 ----
// One launch over ntasks tasks (tasks[3 q ..]: offset of the first entry from L, stride, length), one workgroup each.  check == 0:
// the entries <- 0, nothing else is written.  check != 0: nothing of L is written; *flag <- 1 when an entry is not zero or, with
// one_off >= 0, L[one_off] is not 1 (*flag is never cleared).  ntasks <= 0: no launch.
void launch_rowmod_zero_rows(double* L, const int64_t* tasks, int64_t ntasks, int64_t one_off, int check, int* flag, hipStream_t st);
// col = the address of L_jj in its panel, the nbelow entries behind it the column below the diagonal, rows[i] the row of entry
// 1 + i:  W[rows[i]] <- col[1 + i], col[1 + i] <- 0, col[0] <- 1
void launch_rowdel_column(double* col, int64_t nbelow, const int32_t* rows, double* W, hipStream_t st);
// One launch of one wave: D y = W[col0 .. col0 + b) on the b x b block D (lower triangle read only), y to y[0 .. b), zeros to
// column 0 of those rows of W
void launch_rowadd_sweep_diag(const double* D, int64_t ld, int b, double* W, int64_t col0, double* y, hipStream_t st);
// The nrows panel rows below the block: W[rows[i]] -= sum_col P(i, col) y[col], column after column.  The row with rows[i] ==
// target (-1: none) is first overwritten with y.  rows[] are distinct.
void launch_rowadd_sweep_rows(double* P, int64_t ld, int b, int64_t nrows, const int32_t* rows, int32_t target, double* W, const double* y,
                              hipStream_t st);
// One workgroup.  d = W[jrow]: not positive, NaN, or *info set on entry: *info <- 1 and nothing else is written.  Otherwise
// col[0] <- sqrt(d), col[1 + i] <- W[rows[i]] / sqrt(d), which also stays in W[rows[i]], and W[jrow] <- 0.
void launch_rowadd_column(double* col, int64_t nbelow, const int32_t* rows, double* W, int64_t jrow, int* info, hipStream_t st);

}  // namespace sf
