/*
 * sparseframe_flat.h -- the flat ("plan") C ABI of the MI355X-native numeric-factorization core, shared by the
 * Cholesky and the LU struct headers.  extern "C", plain pointers and sizes only; everything here is exported by
 * libsparseframe_hip.so.  Citations: C: = Cholesky/Source/SparseFrame.c, L: = LU/Source/SparseFrame.c of the reference.
 */
#ifndef SPARSEFRAME_FLAT_H
#define SPARSEFRAME_FLAT_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scalar types: reference arch.h:6-16 (Int=int, Long=long, Float=double) ---- */
typedef int64_t sf_long;   /* reference `Long`  (LP64 long)  */
typedef double  sf_float;  /* reference `Float`               */

/* reference type.h:4-5 */
enum FactorizeType { TYPE_CHOLESKY, TYPE_QR, TYPE_LU };
enum PermMethod { PERM_IDENTITY, PERM_AMD, PERM_METIS };

/* ---- reference I:12-29.  Field order and types are the ABI. ---- */
struct common_info_struct
{
    int numCPU;
    int numGPU;
    int numGPU_physical;
    size_t minDevMemSize;
    size_t minHostMemSize;
    int matrixThreadNum;
    int numSparseMatrix;
    size_t devSlotSize;      /* INPUT of symbolic analysis (C:1402): caps supernode/stage size */
    double allocateTime;
    double computeTime;
    double freeTime;
};

/* ---- reference I:31-68 embeds CUDA/cuBLAS/cuSOLVER handles and is only touched by
 * allocate_gpu / free_gpu / factorize.  Here it is opaque HIP state: one element per
 * device handler, allocated and freed by this library only. ---- */
struct gpu_info_struct;

/* =====================================================================================
 * Layer 2: flat ABI.
 * ===================================================================================== */

#define SF_OK                0
#define SF_ERR_ARG           1
#define SF_ERR_NO_DEVICE     2   /* no HIP device / HIP runtime error */
#define SF_ERR_ALLOC         3
#define SF_ERR_NOT_POSDEF    4   /* non-positive pivot met in a diagonal block */
#define SF_ERR_HIP           5
#define SF_ERR_PEER          6   /* multi-GPU: another rank of the group reported a failure; this rank stopped with it */

/* ---- host-side symbolic analysis on plain arrays (what SparseFrame_analyze forwards to).
 * The result object owns its arrays; read them through sf_symbolic_get. ---- */
typedef struct sf_symbolic sf_symbolic;

int sf_symbolic_create(sf_symbolic **out, sf_long n, const sf_long *Cp, const sf_long *Ci, const sf_float *Cx,
                       const sf_long *perm /* NULL = identity */, size_t devSlotSize);
/* LU variant (reference LU/Source/SparseFrame.c:1068-2231): elimination tree / counts / row structures of the
 * pattern of L + U^T, panels of (2*nsrow - nscol) x nscol values (L:1946).  is_symmetric != 0: Cp/Ci/Cx hold one
 * triangle of a symmetric matrix (then U aliases L, L:2718-2729); otherwise the whole matrix in CSC.
 * Extra arrays: Long "Up","Ui","UTp","UTi" (U by ROW and its transpose, L:1179-1282), double "Ux","UTx". */
int sf_symbolic_create_lu(sf_symbolic **out, sf_long n, const sf_long *Cp, const sf_long *Ci, const sf_float *Cx,
                          const sf_long *perm /* NULL = identity */, size_t devSlotSize, int is_symmetric);
void sf_symbolic_destroy(sf_symbolic *sym);
/* scalar outputs: "n","nnz","nfsuper","nsuper","nstage","isize","xsize","csize","nsleaf","lu","symmetric","unz" */
sf_long sf_symbolic_scalar(const sf_symbolic *sym, const char *name);
/* array outputs (borrowed pointers, valid until destroy):
 * Long arrays: "Perm","Parent","Post","ColCount","ColCount0","Lp","Li","LTp","LTi","Super","SuperMap","Sparent",
 *              "Lsip","Lsxp","Lsi","LeafQueue","ST_Map","ST_Pointer","ST_Index","Aoffset","Moffset"
 * "Post" and "ColCount0"/"Parent0" are the PRE-supernodal values (before C:1429-1445 renumbers them).
 * double arrays: "Lx","LTx" */
const sf_long *sf_symbolic_long_array(const sf_symbolic *sym, const char *name, sf_long *len);
const sf_float *sf_symbolic_float_array(const sf_symbolic *sym, const char *name, sf_long *len);
/* algorithmic flop counts: which = 0 -> F_struct = sum_j ColCount_j^2 (unrelaxed),
 * 1 -> F_exec (executed, relaxed supernodes), 2 -> executed SYRK/GEMM update flops only */
double sf_symbolic_flops(const sf_symbolic *sym, int which);

/* deterministic geometric nested dissection of an nx*ny*nz grid (node id = x + nx*(y + ny*z)):
 * recursive longest-axis bisection with sep_width-plane separators, leaf boxes of at most
 * leaf^3 nodes in natural order.  perm[new] = old.  Stands in for METIS (unpinned third party). */
int sf_grid_nd_perm(sf_long nx, sf_long ny, sf_long nz, sf_long leaf, sf_long sep_width, sf_long *perm);

/* Built-in fill-reducing ordering for a general symmetric pattern (any triangle or both in Cp/Ci): nested dissection
 * by BFS level-structure separators, pieces of at most `leaf` vertices in reverse BFS order.  perm[new] = old.
 * A self-contained stand-in for the reference's METIS_NodeND call (C:942); orderings are outside the parity contract. */
int sf_graph_nd_perm(sf_long n, const sf_long *Cp, const sf_long *Ci, sf_long leaf, sf_long *perm);

/* ---- device plan for supernodal Cholesky (replaces C:2150-3017 + CK:22-158) ---- */
typedef struct sf_chol_plan sf_chol_plan;

/* Uploads the symbolic structure to `device`, builds the level schedule and the grouped
 * task tables, allocates the device-resident factor (xsize doubles).  Depends on the
 * structure only: reusable for any number of numeric factorizations of the same pattern.
 * Every entry (Li[p], j) of a column j of supernode s must have a place in its panel: Super[s] <= Li[p] < n, and Li[p] is
 * a column of s or one of the rows Lsi lists for s -- otherwise SF_ERR_ARG (for every plan constructor, LU's Ui likewise).
 * An entry given more than once in its column is loaded from its LAST occurrence, as the reference's sequential loadA does. */
int sf_chol_plan_create(sf_chol_plan **plan, int device,
                        sf_long n, sf_long nsuper,
                        const sf_long *Super, const sf_long *SuperMap,
                        const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                        const sf_long *Lp, const sf_long *Li);
/* H2D copy of the CSC values of lower(P A P^T) (nnz = Lp[n] doubles). */
int sf_chol_plan_set_values(sf_chol_plan *plan, const sf_float *Lx);
/* The timed hot path: assemble (loadA) + factor every supernode + Schur updates with the
 * mapped scatter, entirely on the device.  Asynchronous on the plan's stream unless
 * `sync` != 0.  Returns SF_ERR_NOT_POSDEF (after sync) when a pivot <= 0 was met. */
int sf_chol_plan_factorize(sf_chol_plan *plan, int sync);
/* waits for the plan's stream and returns the factorization status */
int sf_chol_plan_sync(sf_chol_plan *plan);
/* D2H copy of the factor into the reference layout (xsize doubles). */
int sf_chol_plan_get_factor(sf_chol_plan *plan, sf_float *Lsx);
/* values H2D + numeric factorization + factor D2H into host_out (reference layout, xsize doubles), the download of
 * finished blocks overlapped with the computation of the levels above them (the reference's copy-back stream,
 * C:2888-2895).  host_out may be ordinary pageable memory (it is never pinned or registered).  Ux: LU plans only (NULL
 * when U aliases L).  "last_to_host_ms" reports the wall time of the call. */
int sf_chol_plan_factorize_to_host(sf_chol_plan *plan, const sf_float *Lx, const sf_float *Ux, sf_float *host_out);
/* device pointer of the resident factor (for device-side consumers) */
void *sf_chol_plan_factor_device_ptr(sf_chol_plan *plan);
/* device-side supernodal solve with the resident factor: x <- (L L^T)^{-1} b, permuted space */
int sf_chol_plan_solve(sf_chol_plan *plan, const sf_float *b_host, sf_float *x_host);
/* device-side supernodal solve of nrhs right-hand sides with the resident factor, permuted space: X <- (L L^T)^{-1} B
 * (LU plans: (L U)^{-1} B, with the plan's pivots when pivoting is on).  B, X: column-major host arrays, leading dimensions
 * ldb, ldx >= n; X may be B (ldx == ldb).  nrhs == 0: no-op.  Whole, resident plans only (partial, sharded, mapped,
 * out-of-core and schedule-only plans: SF_ERR_ARG).  16 right-hand sides per sweep (stat "solve_many_width"); the device
 * block is allocated by the first call and kept (stat "bytes_solve_many", not in "bytes_device"; SF_ERR_ALLOC leaves the
 * plan usable); "last_solve_many_ms": device time of the sweeps of the last call, copies excluded. */
int sf_chol_plan_solve_many(sf_chol_plan *plan, sf_long nrhs, const sf_float *B, sf_long ldb, sf_float *X, sf_long ldx);
/* values [e_begin, e_end) of the factor in the reference layout (whole plans only) */
int sf_chol_plan_get_factor_range(sf_chol_plan *plan, sf_long e_begin, sf_long e_end, sf_float *out);
/* selected inversion: Sigma = A^{-1} = (L L^T)^{-1} on the pattern of L, permuted space, into a plan-owned device arena with the
 * factor's reference layout (xsize doubles, panel s at Lsxp[s], nsrow x nscol column-major; the strict upper part of each
 * diagonal block holds the mirror of its lower part).  Synchronous.  The arena and its scratch are allocated by the first call and
 * kept until destroy (stat "bytes_selinv", not in "bytes_device"); SF_ERR_ALLOC leaves the plan usable.  Needs a successful
 * factorization of the current values; whole, resident Cholesky plans only (schedule-only, partial, sharded, mapped, out-of-core
 * and LU plans: SF_ERR_ARG).  Stats: "last_selinv_ms" (device time), "flops_selinv" (operation count of the unit decomposition),
 * "selinv_valid" (1 while the arena belongs to the resident factor: set_values, a factorization or an import clear it). */
int sf_chol_plan_selinv(sf_chol_plan *plan);
/* arena values [e_begin, e_end) (SF_ERR_ARG when the arena is not valid) */
int sf_chol_plan_get_selinv_range(sf_chol_plan *plan, sf_long e_begin, sf_long e_end, sf_float *out);
/* diag(Sigma), n doubles, gathered on the device (SF_ERR_ARG when the arena is not valid) */
int sf_chol_plan_selinv_diag(sf_chol_plan *plan, sf_float *d);
/* log det A = 2 sum_j log L_jj of the resident factor, reduced on the device in a fixed order (independent of selinv) */
int sf_chol_plan_logdet(sf_chol_plan *plan, sf_float *out);
/* ---- Sigma read where the caller wants it: on the pattern the plan was created with, as tr(Sigma M(V)), and at
 * (row, column) pairs.  Gathers and fixed-order reductions over the arena of sf_chol_plan_selinv; everything in permuted space, as
 * sf_chol_plan_get_selinv_range.  All of them need what sf_chol_plan_selinv needs AND a valid arena (stat "selinv_valid" == 1):
 * otherwise -- schedule-only, partial, sharded, mapped, out-of-core and LU plans, no or a stale arena -- SF_ERR_ARG with every output
 * untouched; so are NULL pointers, negative counts and a short leading dimension.  Device state (the position of every entry, the
 * parts of a trace, the staging buffer of the pairs) is allocated by the first call that needs it and kept until destroy: stat
 * "bytes_selinv_pattern", not in "bytes_device"; SF_ERR_ALLOC leaves the plan usable.  "last_selinv_pattern_ms": device time of the
 * last call's kernels, copies excluded. ---- */
/* out[p] = Sigma(Li[p], j) for EVERY position p of column j of the structure the plan was created with (Lp / Li), nnz doubles --
 * also where the assembly ignores the position: an entry given again later in its column gets the Sigma of its (i, j) all the same */
int sf_chol_plan_selinv_values(sf_chol_plan *plan, sf_float *out /* nnz */);
/* the same into device memory of the plan's device (checked as sf_chol_plan_solve_device checks its blocks) */
int sf_chol_plan_selinv_values_device(sf_chol_plan *plan, sf_float *d_out /* nnz */);
#define SF_SEL_MAPPED 1      /* V is in the caller's own layout and read through the map of sf_chol_plan_set_value_map */
#define SF_SEL_MAX_M 64
/* out[t] = tr(Sigma M(V_t)), t < m, where M(V_t) is the matrix sf_chol_plan_set_values(V_t) would assemble (positions the assembly
 * ignores do not count, their V is never read): sum over the diagonal entries of Sigma_jj V_jj plus twice the sum over the others
 * of Sigma_ij V_ij -- for V = dA/dtheta the derivative of log det A.  V: column-major, column t = V + t ldv, nnz doubles each, ldv >=
 * max(nnz, 1); with SF_SEL_MAPPED column t has nsrc doubles in the caller's layout (a -1 map entry counts as 0), ldv >= max(nsrc, 1),
 * and a plan without a stored map is refused.  0 <= m <= SF_SEL_MAX_M; m == 0: SF_OK, nothing written.  One pass over the load map
 * and the arena whatever m is, no floating-point atomics; the order of every sum is a function of nnz alone, so the same arena and
 * V give the same bits every time, and out[t] depends on column t of V only (a NaN there reaches out[t] and nothing else). */
int sf_chol_plan_selinv_trace(sf_chol_plan *plan, sf_long m, const sf_float *V, sf_long ldv, int flags /* 0 | SF_SEL_MAPPED */,
                              sf_float *out /* m */);
int sf_chol_plan_selinv_trace_device(sf_chol_plan *plan, sf_long m, const sf_float *dV, sf_long ldv, int flags, sf_float *d_out /* m */);
/* out[k] = Sigma(rows[k], cols[k]), permuted indices, either triangle; found on the device by the search of the assembly (the
 * column's supernode, then its row list).  A pair outside the pattern of L gets a quiet NaN and is counted in *outside (may be
 * NULL; also stat "last_selinv_outside") -- the call still returns SF_OK.  An index outside [0, n): SF_ERR_ARG before anything is
 * written.  The pairs go up in chunks of 65536 (stat "selinv_entries_chunk"). */
int sf_chol_plan_selinv_entries(sf_chol_plan *plan, sf_long count, const sf_long *rows, const sf_long *cols, sf_float *out,
                                sf_long *outside /* or NULL */);
/* ---- adjoints on the pattern: what a solve, a quadratic form or a log-determinant contributes to the gradient with
 * respect to the matrix values, as an array in set_values order.  M(V) is the matrix sf_chol_plan_set_values(V) assembles, as for
 * sf_chol_plan_selinv_trace.  Plans: those sf_chol_plan_solve_device accepts (schedule-only, partial, sharded, mapped and out-of-core
 * plans: SF_ERR_ARG).  SF_ERR_ARG -- a NULL pointer, k < 0, a short leading dimension, an unknown flag bit, a flag whose stored
 * ordering or map is missing, a device pointer that sf_chol_plan_solve_device would refuse, an output that overlaps an input --
 * leaves every output untouched.  Device state (the column and the kind of every position, 5 bytes each; for SF_ADJ_MAPPED the
 * unmapped result and the map by source entry) is allocated by the first call that needs it and kept until destroy: stat
 * "bytes_adjoint", not in "bytes_device".  "last_adjoint_ms": device time of the last call's kernels, copies excluded. ---- */
#define SF_ADJ_MAPPED 4      /* out has nsrc doubles in the caller's own value layout, written through the map of sf_chol_plan_set_value_map */
/* out such that  sum_p out[p] dV[p] = alpha sum_{c<k} y_c^T M(dV) x_c  for every dV: for position p of column j with row i = Li[p]
 *     i != j:  out[p] = alpha sum_c (Y[i,c] X[j,c] + Y[j,c] X[i,c])          i == j:  out[p] = alpha sum_c Y[i,c] X[i,c]
 * and exactly 0 where the assembly does not read the position (an entry given again later in its column).  With X = A^{-1} B,
 * Y = A^{-1} G and alpha = -1 this is the gradient of a loss with respect to the values when G is its gradient with respect to X.
 * Y, X: column-major n x k, ldy, ldx >= max(n, 1), permuted space; NULL only with k == 0.  k is limited by memory alone; k == 0
 * writes zeros.  Needs the plan's structure only: no values, no factor -- it works before the first factorization and after a failed
 * one.  Every out[p] is one accumulator over ascending c, one fma per product, (i, j) before (j, i), then one multiplication by alpha;
 * no floating-point atomics: the same inputs give the same bits on every call, and a NaN in row r of Y or X reaches only the
 * positions whose row or column is r.
 * SF_ADJ_MAPPED: out has nsrc doubles, out[s] = the sum of the unmapped results of the positions p with map[p] == s, added to +0.0
 * in ascending p (a map may name one source entry at several positions -- a symmetric source feeding both triangles of an LU plan,
 * for one: they are summed, in this fixed order); a source entry no position names gets 0.  A plan without a stored map is refused.
 * _device: Y, X, out in device memory of the plan's device; flags may add SF_DEV_PERM_IN: Y and X are in the caller's numbering and
 * row perm[i] is read where row i is due (needs sf_chol_plan_set_ordering) -- bit for bit the result of the call on the permuted blocks. */
int sf_chol_plan_adjoint_values(sf_chol_plan *plan, sf_long k, const sf_float *Y, sf_long ldy, const sf_float *X, sf_long ldx, double alpha,
                                int flags /* 0 | SF_ADJ_MAPPED */, sf_float *out /* nnz; mapped: nsrc */);
int sf_chol_plan_adjoint_values_device(sf_chol_plan *plan, int flags /* 0 | SF_DEV_PERM_IN | SF_ADJ_MAPPED */, sf_long k, const sf_float *dY,
                                       sf_long ldy, const sf_float *dX, sf_long ldx, double alpha, sf_float *d_out);
/* out such that  sum_p out[p] dV[p] = alpha sf_chol_plan_selinv_trace(dV)  for every dV -- alpha times the gradient of log det A with
 * respect to the values: (i != j ? 2 : 1) alpha Sigma(i, j) where the assembly reads the position, exactly 0 where it does not
 * (sf_chol_plan_selinv_values has neither the factor 2 nor the zeros).  Needs a valid arena exactly as sf_chol_plan_selinv_values
 * does and is refused the same way.  flags: 0 or SF_ADJ_MAPPED (as above). */
int sf_chol_plan_logdet_grad_values(sf_chol_plan *plan, double alpha, int flags, sf_float *out /* nnz; mapped: nsrc */);
int sf_chol_plan_logdet_grad_values_device(sf_chol_plan *plan, double alpha, int flags, sf_float *d_out);
/* SparseFrame_validate on the device (C:3141-3266; LU plans: L:3702-3858): b_i = 1 + i/n, solve with the resident factor,
 * r = A x - b from the plan's copy of the matrix values, *residual = |r|_inf / (|A|_1 |x|_inf + |b|_inf).  x_host may be NULL.
 * *residual is NaN when any r_i or x_i is not finite (NaN fails every `<=`); the return code is SF_OK all the same.  The struct
 * path's SparseFrame_validate (both libraries) sets matrix_info->residual by the same rule. */
int sf_chol_plan_validate(sf_chol_plan *plan, sf_float *residual, sf_float *x_host);
/* r = b - A x on the device with the plan's CURRENT matrix values (the last set_values; permuted space), for the caller's own b
 * and x.  With w = |A| |x| + |b|:
 *     *berr = max_i |r_i| / w_i over the rows with w_i > 0     (componentwise backward error, as LAPACK xPORFS / xGERFS report it)
 *     *nerr = |r|_inf / (|A|_1 |x|_inf + |b|_inf)              (the number sf_chol_plan_validate reports)
 * If any r_i, x_i or b_i is not finite, both come back not finite (NaN), never a finite value that hides it.  r_host, berr, nerr
 * may each be NULL.  Plain fp64 with FMA, one pass over the rows of A in a fixed summation order: the same b and x give the same
 * bits on every call.  An entry given more than once in its column counts as the factorization counts it (the last one); an
 * unsymmetric LU plan takes the diagonal from U, as its factorization does.  Needs set_values only, no factorization.
 * Whole, resident plans (schedule-only, partial, sharded, mapped and out-of-core plans: SF_ERR_ARG).  The row form of A --
 * positions into the plan's value arrays, so a later set_values needs no rebuild -- and the work vectors are allocated by the
 * first residual / refine call and kept (stat "bytes_refine", not in "bytes_device"; SF_ERR_ALLOC leaves the plan usable). */
int sf_chol_plan_residual(sf_chol_plan *plan, const sf_float *b_host, const sf_float *x_host,
                          sf_float *r_host /* or NULL */, sf_float *berr /* or NULL */, sf_float *nerr /* or NULL */);
/* Iterative refinement on the device: x0 = solve(b), then at most max_iter steps  r = b - A x;  d = solve(r);  x += d.
 * Before step k (k = 0, 1, ...) the loop stops if berr_k <= tol (tol <= 0: 2^-52), if k == max_iter, if berr_k is not finite, or if
 * k >= 1 and berr_k > berr_{k-1} / 2 (stagnation).  x_host receives the iterate with the SMALLEST finite berr seen (kept in a
 * second device vector) and *berr that value; if berr_0 is not finite, x0 and that berr -- the return code stays SF_OK.
 * max_iter == 0: the plain solve plus its berr.  max_iter < 0, NULL b or x: SF_ERR_ARG.  x_host may be b_host.
 * The solves use the RESIDENT factor, the residual the CURRENT values: the last factorization that was started must have
 * succeeded, but it need NOT be a factorization of the current values -- set_values after factorize is allowed and refines
 * towards the new matrix with the old factor as preconditioner (values that drift over time steps, one factorization kept).
 * Per step one 48-byte copy and one synchronisation; b, x, r, w and the best x stay on the device.  Same plans as residual.
 * Stats: "last_refine_iters" (solves after the first), "last_refine_berr0", "last_refine_berr", "last_refine_ms" (device
 * time from events, the copies of b and x excluded), "bytes_refine". */
int sf_chol_plan_refine(sf_chol_plan *plan, const sf_float *b_host, sf_float *x_host,
                        int max_iter, double tol, sf_float *berr /* or NULL */);
/* w = |A| |x| + |b| (n doubles) of the last residual evaluation of this plan (a residual call, or the last step of a refine
 * call); Cholesky and LU plans; SF_ERR_ARG before the first one */
int sf_chol_plan_residual_weights(sf_chol_plan *plan, sf_float *w_host);
/* 1-norm condition estimate with the resident factor: *anorm = |A|_1 of the plan's CURRENT values (the residual's device code),
 * *ainv_norm_est = a lower bound of |A^{-1}|_1 of the RESIDENT factor that is almost always within a factor 3 of it, so
 * kappa_1(A) ~ *anorm * *ainv_norm_est when the factor is one of the current values.  The ordering leaves both norms unchanged:
 * they are the caller's matrix's.  Hager's algorithm as in Higham / LAPACK xLACON: at most 5 passes of one A^{-1} and one A^{-T}
 * sweep of width 1 (Cholesky: the same sweeps twice), then the alternating-sign safeguard vector -- at most 11 sweeps.  Where
 * xLACON replaces its estimate by a smaller later column norm, the larger one is kept (both are lower bounds).  The vectors stay
 * on the device; per pass one 16-byte copy and one synchronisation.  Same plans as sf_chol_plan_refine, and like it refused
 * (SF_ERR_ARG) when the last factorization that was started has not succeeded; an LU plan is refused here (sf_lu_plan_condest).
 * Stats: "last_condest_solves" (sweep pairs run), "last_condest_ms" (device time from the first to the last kernel, the waits for
 * the host's decisions included), "bytes_condest" (2 n + 2 doubles kept after the first call, not in "bytes_device"). */
int sf_chol_plan_condest(sf_chol_plan *plan, sf_float *anorm, sf_float *ainv_norm_est);
/* The two halves of the solve on their own, with the resident factor L (A = L L^T of the permuted matrix), permuted space:
 * X <- L^{-1} B (SF_HALF_L, the forward sweep: whitening) or X <- L^{-T} B (SF_HALF_LT, the backward sweep); SF_HALF_L and then
 * SF_HALF_LT is sf_chol_plan_solve_many.  B, X: column-major host arrays, leading dimensions ldb, ldx >= max(n, 1); X may be B
 * (ldx == ldb).  nrhs == 0: no-op.  nrhs == 1 runs the one-column kernels of sf_chol_plan_solve, nrhs > 1 the 16-wide ones of
 * sf_chol_plan_solve_many in chunks of 16 (its device block, allocated by whichever call comes first: "bytes_solve_many"; SF_ERR_ALLOC
 * leaves the plan usable).  Whole, resident Cholesky plans only (schedule-only, partial, sharded, mapped, out-of-core and LU plans:
 * SF_ERR_ARG), and like sf_chol_plan_refine refused (SF_ERR_ARG) when the last factorization that was started has not succeeded.
 * "last_half_ms": device time of the sweeps of the last call, copies excluded. */
#define SF_HALF_L  0   /* X <- L^{-1} B   (forward sweep only)  */
#define SF_HALF_LT 1   /* X <- L^{-T} B   (backward sweep only) */
int sf_chol_plan_solve_half(sf_chol_plan *plan, int which, sf_long nrhs,
                            const sf_float *B, sf_long ldb, sf_float *X, sf_long ldx);
/* q[j] = b_j^T A^{-1} b_j = |L^{-1} b_j|_2^2 for j < nrhs (the Mahalanobis term of a Gaussian log-density; with sf_chol_plan_logdet
 * the log-likelihood): the forward sweep and a per-column sum of squares on the device, two passes in a fixed order without
 * floating-point atomics -- a NaN or Inf stays in its column, a zero column gives exactly 0.  Only q (nrhs doubles) comes back.
 * B, plans, kernels and chunking as sf_chol_plan_solve_half.  "last_quadform_ms": device time of the last call, copies excluded. */
int sf_chol_plan_quadform(sf_chol_plan *plan, sf_long nrhs, const sf_float *B, sf_long ldb, sf_float *q);
/* Gaussian sampling with precision matrix A: X[:, j] = L^{-T} z_j with z_j ~ N(0, I) generated on the device, so Cov(x) = A^{-1}
 * (permuted space); Z != NULL also returns the normals used (X, Z: column-major host arrays, ldx, ldz >= max(n, 1); Z != X).
 * Column j is sample number s = first_sample + j of the stream `seed`: element (i, s) depends on (seed, i, s) alone, never on
 * nsamples or on how a run is cut into calls.  Philox4x32-10 with the counter (i lo, i hi, p lo, p hi), p = s >> 1, and the key
 * (seed lo, seed hi) gives r0..r3; u1 = ((r0 >> 5) * 2^26 + (r1 >> 6) + 0.5) * 2^-53, u2 likewise from r2, r3; Box-Muller:
 * rad = sqrt(-2 log u1), th = 2 pi u2, the normal is rad cos(th) for even s and rad sin(th) for odd s.  nsamples == 0: no-op.
 * Always the 16-wide kernels (the block is generated in their layout).  Plans as sf_chol_plan_solve_half.  "last_sample_ms":
 * device time of the last call (generator and sweeps), copies excluded. */
int sf_chol_plan_sample(sf_chol_plan *plan, sf_long nsamples, uint64_t seed, uint64_t first_sample,
                        sf_float *X, sf_long ldx, sf_float *Z /* or NULL */, sf_long ldz);
/* ---- device-pointer entry points: right-hand sides, solutions, samples and matrix values that stay on the device,
 * optionally in the caller's own numbering.  Whole, resident plans only (schedule-only, partial, sharded, mapped and out-of-core
 * plans: SF_ERR_ARG, as sf_chol_plan_solve_many).
 * Synchronisation: the work runs on the plan's stream and every call returns after its result is complete.  The caller must have
 * completed whatever produces the device arrays it passes, or run the plan on the producers' stream (sf_chol_plan_set_stream).
 * There is no asynchronous variant.
 * Pointers: every device pointer is checked with hipPointerGetAttributes before anything is enqueued -- one that is not device
 * (or managed) memory of the plan's device, or whose allocation ends before the block does, is SF_ERR_ARG. ---- */
/* the ordering for SF_DEV_PERM_IN / SF_DEV_PERM_OUT and sf_chol_plan_permute_device: perm[new] = old, n entries, as
 * sf_symbolic_create takes it (NULL: the identity).  Not a permutation of 0..n-1: SF_ERR_ARG, the plan keeps what it had.  Uploaded
 * as 32-bit indices, like the plan's own row lists; stat "bytes_ordering" (with the value map's bytes, not in "bytes_device"),
 * stat "ordering_set" (1 once a call has succeeded).
 * Cholesky and LU plans. */
int sf_chol_plan_set_ordering(sf_chol_plan *plan, const sf_long *perm);
#define SF_OP_SOLVE   0   /* X <- A^{-1} B                                   (Cholesky and LU plans) */
#define SF_OP_HALF_L  1   /* X <- L^{-1} B, as SF_HALF_L                     (Cholesky plans)        */
#define SF_OP_HALF_LT 2   /* X <- L^{-T} B, as SF_HALF_LT                    (Cholesky plans)        */
#define SF_OP_TRANS   3   /* X <- A^{-T} B, as sf_lu_plan_solve_transposed   (LU plans)              */
#define SF_DEV_PERM_IN  1 /* row i of the block the sweeps see is row perm[i] of dB: dB is in the caller's numbering */
#define SF_DEV_PERM_OUT 2 /* row i of the result goes to row perm[i] of dX: dX is in the caller's numbering          */
/* sf_chol_plan_solve / _solve_many / _solve_half on device memory.  dB, dX: column-major device arrays, ldb, ldx >= max(n, 1);
 * dX == dB with ldx == ldb is allowed, the flags included (a chunk is loaded whole before any of it is stored).  With P the
 * ordering, the sweeps run on (PERM_IN ? P dB : dB) and dX receives (PERM_OUT ? P^T : I) times their result: both flags on
 * SF_OP_SOLVE solve the caller's own system.  A flag without sf_chol_plan_set_ordering, an op the plan kind does not have, a
 * plan whose last started factorization has not succeeded: SF_ERR_ARG.  nrhs == 1 runs the one-column kernels on the plan's
 * vector, nrhs > 1 the 16-wide ones in chunks ("bytes_solve_many", allocated by whichever call comes first).  A block moves
 * straight between the caller's memory and the plan's: no staging copy.  Stats: "last_solve_ms" (nrhs == 1), "last_solve_many_ms"
 * (SF_OP_SOLVE, SF_OP_TRANS with nrhs > 1), "last_half_ms" (the halves): device time from the first to the last kernel of the
 * call, the load and store kernels included. */
int sf_chol_plan_solve_device(sf_chol_plan *plan, int op, int flags, sf_long nrhs,
                              const sf_float *dB, sf_long ldb, sf_float *dX, sf_long ldx);
/* the ordering alone: dX = P dB (row i = row perm[i] of dB), or with inverse != 0 dX = P^T dB (row perm[i] = row i of dB).  Not in
 * place (dX == dB: SF_ERR_ARG).  Needs sf_chol_plan_set_ordering, no factorization.  Cholesky and LU plans. */
int sf_chol_plan_permute_device(sf_chol_plan *plan, int inverse, sf_long nrhs,
                                const sf_float *dB, sf_long ldb, sf_float *dX, sf_long ldx);
/* sf_chol_plan_sample with the samples stored into device memory (flags: 0 or SF_DEV_PERM_OUT); the same generator and stream
 * definition, so column j holds what sf_chol_plan_sample gives for the same (seed, first_sample + j).  No Z output. */
int sf_chol_plan_sample_device(sf_chol_plan *plan, sf_long nsamples, uint64_t seed, uint64_t first_sample, int flags,
                               sf_float *dX, sf_long ldx);
/* sf_chol_plan_set_values from device memory (nnz doubles): a device-to-device copy with the same effects on the plan */
int sf_chol_plan_set_values_device(sf_chol_plan *plan, const sf_float *dLx);
/* values straight from the caller's own value array: map[p] in [-1, nsrc) for every entry p of Lx (mapU: of Ux, LU plans with an
 * unsymmetric input, else NULL) is the position of that entry in an array of nsrc doubles, -1 an entry the caller does not supply
 * (value 0).  Validated (SF_ERR_ARG, the plan keeps what it had) and uploaded once ("bytes_ordering");
 * sf_chol_plan_set_values_mapped_device(dAx) is then one gather kernel per time step with every effect of set_values.  Cholesky
 * and LU plans. */
int sf_chol_plan_set_value_map(sf_chol_plan *plan, sf_long nsrc, const sf_long *mapL, const sf_long *mapU /* or NULL */);
int sf_chol_plan_set_values_mapped_device(sf_chol_plan *plan, const sf_float *dAx);
/* ---- the dense Schur complement of a border: G = B^T A^{-1} B for an n x k block B, permuted space.  With A = L L^T
 * and Y = L^{-1} B, G = Y^T Y: one FORWARD sweep per chunk of 16 columns (the kernels of sf_chol_plan_solve_half), Y kept on the
 * device, a v_mfma_f64_16x16x4_f64 reduction over the rows, and only k x k doubles come back.  The diagonal of G is what
 * sf_chol_plan_quadform returns; k == 1 runs quadform's own one-column path, so G[0] is exactly its value.
 * B: column-major, ldb >= max(n, 1); G: column-major k x k, ldg >= max(k, 1), written in full (both triangles).  k == 0: SF_OK,
 * nothing written.  NULL pointers, k < 0, k > SF_GRAM_MAX_K, a short leading dimension: SF_ERR_ARG, nothing written; plans as
 * sf_chol_plan_quadform (LU, schedule-only, partial, sharded, mapped and out-of-core plans and a plan whose last started
 * factorization has not succeeded: SF_ERR_ARG).
 * Determinism: no floating-point atomics and a fixed summation order in the reduction, so for a given Y the result repeats bit
 * for bit (Y itself repeats to rounding only where the sweep scatters with atomics); G is bit-for-bit symmetric; entry (i, j) is a
 * function of the columns i and j of B alone, so a NaN or Inf in column j reaches row j and column j of G and nothing else.
 * The Y store (ceil(k / 16) blocks of n x 16 doubles, the parts of the reduction and the host call's k x k result block) is
 * allocated or grown by the first call that needs it and kept: stat "bytes_gram", not in "bytes_device"; SF_ERR_ALLOC leaves the
 * plan as it was.  Stats: "last_gram_ms" (device time of the sweeps and reductions of the last call, copies excluded),
 * "last_gram_parts" (row slabs, i.e. workgroups per 16 x 16 tile, of the last call; 0 for k == 1). ---- */
#define SF_GRAM_MAX_K 1024
int sf_chol_plan_gram(sf_chol_plan *plan, sf_long k, const sf_float *B, sf_long ldb,
                      sf_float *G, sf_long ldg);            /* host, column-major */
/* the same on device memory (pointer checks and synchronisation as sf_chol_plan_solve_device; the result is complete on return).
 * flags: 0 or SF_DEV_PERM_IN (dB is in the caller's numbering; needs sf_chol_plan_set_ordering), any other bit: SF_ERR_ARG.  dG
 * must not overlap dB (SF_ERR_ARG).  The block goes straight from dB into the Y store: no staging copy. */
int sf_chol_plan_gram_device(sf_chol_plan *plan, int flags /* 0 | SF_DEV_PERM_IN */, sf_long k,
                             const sf_float *dB, sf_long ldb, sf_float *dG, sf_long ldg);
/* ---- rank-k update and downdate of the resident factor: A' = A + sign W W^T without a factorization, for a W that
 * leaves the pattern of L as it is.  W = k sparse columns (Wp[k + 1], Wi, Wx) in the plan's numbering -- with SF_DEV_PERM_IN in the
 * caller's, mapped through the ordering of sf_chol_plan_set_ordering --, the rows of a column in any order.  A column is ADMISSIBLE
 * when, with j0 its smallest row and s0 the supernode of j0, every other row is a column of s0 or one of the rows Lsi lists below
 * s0: a change of a diagonal entry or of the weight of an existing edge, w = alpha (e_i - e_j), always is.  Only the supernodes on
 * the paths from the s0 to their roots are rewritten, 64 columns per pair of launches; more than 16 columns run as chunks of 16.
 * Refused with SF_ERR_ARG and nothing changed: sign not SF_UPDATE / SF_DOWNDATE, k < 0, a row outside [0, n), a row twice in a
 * column, an unknown flag, SF_DEV_PERM_IN without an ordering, an inadmissible column in any chunk (every column is checked before
 * the first launch; stat "update_bad_column" names the first), LU, schedule-only, partial, sharded, mapped and out-of-core plans,
 * a plan whose last started factorization has not succeeded.  k == 0: SF_OK, nothing changed.
 * On success the updated factor counts as factorized, as an imported one does: solves, logdet, selinv (the arena is invalidated:
 * "selinv_valid" 0), sample, gram and condest see A'.  The plan's stored VALUES are not touched: residual, refine and validate keep
 * using what set_values last put there -- for a consistent plan call set_values(A') first, then the update.
 * A downdate that meets d^2 - w^2 <= 0 (A' is not positive definite, or too close) returns SF_ERR_NOT_POSDEF; the factor is then
 * half rotated and counts as NOT factorized until the next sf_chol_plan_factorize: everything that needs it refuses (SF_ERR_ARG).
 * The block of W (n x 16 doubles) is allocated by the first call and kept: stat "bytes_update", not in "bytes_device".  Stats:
 * "last_updown_ms" (device time of the last call's kernels; "last_update_ms" is the factorization's Schur-update phase),
 * "update_path_supernodes", "update_path_columns", "update_launches". ---- */
#define SF_UPDATE    1
#define SF_DOWNDATE -1
int sf_chol_plan_update(sf_chol_plan *plan, int sign, sf_long k, const sf_long *Wp, const sf_long *Wi, const sf_float *Wx,
                        int flags /* 0 | SF_DEV_PERM_IN */);
/* the same with the values in device memory, aligned with Wi (Wp and Wi stay host arrays); the same kernels, the same bits */
int sf_chol_plan_update_device(sf_chol_plan *plan, int sign, sf_long k, const sf_long *Wp, const sf_long *Wi /* host */,
                               const sf_float *dWx /* device */, int flags);
/* the supernodes an update with this pattern would rewrite, ascending (a topological order); needs no device: schedule-only plans
 * answer too.  *count = their number, supers (NULL or nsuper entries) receives them; *bad_column (may be NULL) = -1, or the first
 * inadmissible column, in which case the call returns SF_ERR_ARG as for any other bad argument. */
int sf_chol_plan_update_path(const sf_chol_plan *plan, sf_long k, const sf_long *Wp, const sf_long *Wi, int flags,
                             sf_long *count, sf_long *supers /* NULL or nsuper entries */, sf_long *bad_column /* or NULL */);
/* ---- row deletion and row addition on the resident factor: the companions of the update for taking a variable out
 * of the system and putting one back, the pattern of L unchanged.  `row` (and Ai) are in the plan's numbering, with SF_DEV_PERM_IN
 * in the caller's.  With j the row, s its supernode:
 * rowdel: the factor of A becomes that of A', A with row and column j replaced by the identity's.  Row j of L left of the diagonal
 * and column j below it become 0, L_jj 1, and the trailing factor takes a rank-1 UPDATE with the old column -- only the supernodes
 * from s (or its parent, for the last column of s) to the root are rotated.
 * rowadd: the inverse.  Row and column j of the factor must be the identity's -- after rowdel, or because A was factorized that
 * way --: this is checked on the device before anything is written (stat "rowmod_not_deleted" 1 when not).  (Ai, Ax)[nz] is the new
 * column of A, the diagonal among its entries, each index once.  An index i < j is ADMISSIBLE when j is in the row list of the
 * supernode of i or that supernode is s, an index i > j when it is a column of s or a row below s: the pattern of A's own column
 * and row j always is.  Row j of L comes from a forward solve along the chains of the indices i < j, L_jj and column j from what it
 * leaves, and the trailing factor takes a rank-1 DOWNDATE with the new column.
 * Refused with SF_ERR_ARG and nothing changed: what sf_chol_plan_update refuses; rowadd also a row outside [0, n), an index twice,
 * a missing diagonal, an inadmissible index (stat "rowmod_bad_index" = its position in Ai), a row that is not the identity's.
 * rowadd whose a_jj - l12^T l12 is not positive returns SF_ERR_NOT_POSDEF and leaves the plan as a failed downdate does.  On
 * success the state changes as after an update: the factor counts as factorized, the selected inverse is invalid, the stored
 * VALUES are untouched -- call set_values(A') first.  Stats: "rowmod_row_tasks" (stretches of row j zeroed or checked),
 * "rowmod_sweep_supernodes", "rowmod_launches" (every launch of the call, the check included); the device time goes to
 * "last_updown_ms", the rotated path to the update's stats, "update_launches" counting the rotations' launches only.
 * "rowmod_bad_index" and "rowmod_not_deleted" describe the last call that passed the update's refusals: each such call starts
 * them at -1 and 0.  The identity check works in the update's block of W, so a rowadd refused for a row that is not the
 * identity's has allocated that block ("bytes_update") where no earlier call had; every other refusal allocates nothing.
 * Accuracy: rowadd forms row j one term per sweep column, in the order of the sweep, so its rounding error grows with the number
 * of columns the sweep crosses where a factorization sums the same terms in blocks (DESIGN 8q has the measured loss).
 * Out of scope as for the update: LU, schedule-only (except rowmod_path), partial, sharded, mapped and out-of-core plans. ---- */
int sf_chol_plan_rowdel(sf_chol_plan *plan, sf_long row, int flags /* 0 | SF_DEV_PERM_IN */);
int sf_chol_plan_rowadd(sf_chol_plan *plan, sf_long row, sf_long nz, const sf_long *Ai, const sf_float *Ax, int flags);
/* no device needed: what the two calls would touch.  rows_supers / rows_pos: the supernodes p (ascending) that hold row `row`
 * below their own columns and its position in their row list; sweep: the supernodes of rowadd's forward sweep (nz = 0, Ai = NULL
 * for rowdel: empty); update: the path of the rank-1 update that follows.  Every list has room for nsuper entries or is NULL, any
 * count may be NULL; *bad (may be NULL) = -1 or the first index of Ai that is not admissible (SF_ERR_ARG then) */
int sf_chol_plan_rowmod_path(const sf_chol_plan *plan, sf_long row, sf_long nz, const sf_long *Ai, int flags,
                             sf_long *nrows, sf_long *rows_supers, sf_long *rows_pos,
                             sf_long *nsweep, sf_long *sweep, sf_long *nupdate, sf_long *update, sf_long *bad);
/* statistics: "levels","launches","gemm_tasks","update_pairs","flops_exec","flops_update",
 * "scatter_elems","bytes_device","last_ms" (device time of the last factorize, HIP events),
 * "last_update_ms","last_panel_ms","last_load_ms" (only when profiling is on) */
double sf_chol_plan_stat(const sf_chol_plan *plan, const char *name);
/* 1 -> record HIP events around each phase of the next factorize calls */
int sf_chol_plan_set_profiling(sf_chol_plan *plan, int on);
int sf_chol_plan_destroy(sf_chol_plan *plan);

/* ---- multi-GPU sharding of ONE factorization by elimination-tree subtrees (the reference has no
 * inter-GPU path: its handlers exchange panels through host memory, C:2267, C:2421-2467).
 * sf_subtree_partition: owner[s] = rank whose subtree holds supernode s, or -1 for the replicated top supernodes.
 * Rank r then builds a plan with phase[s] = 0 (owner[s] == r), 1 (owner[s] == -1), -1 (otherwise) and runs
 *     sf_chol_plan_factorize_phase(plan, 0)   assemble + own subtrees; their updates of top panels accumulate locally
 *     all-reduce(sum) of sf_chol_plan_top_region over the ranks (RCCL)   -- the one exchange step
 *     sf_chol_plan_factorize_phase(plan, 1)   top supernodes, replicated on every rank
 * load_top != 0 on exactly ONE rank (it contributes the matrix entries of the top panels to the sum). ---- */
int sf_subtree_partition(sf_long nsuper, const sf_long *Super, const sf_long *SuperMap, const sf_long *Lsip,
                         const sf_long *Lsi, int nranks, int32_t *owner, double *top_fraction, double *max_load_fraction);
int sf_chol_plan_create_sharded(sf_chol_plan **plan, int device, sf_long n, sf_long nsuper,
                                const sf_long *Super, const sf_long *SuperMap,
                                const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                                const sf_long *Lp, const sf_long *Li, const int32_t *phase, int load_top);
int sf_chol_plan_factorize_phase(sf_chol_plan *plan, int phase /* 0, 1, or -1 = both */, int sync);
/* device pointer and length (doubles) of the contiguous region holding every top panel */
int sf_chol_plan_top_region(sf_chol_plan *plan, void **device_ptr, sf_long *count);

/* ---- a factor LARGER than the device's memory (the reference streams slot-sized "stages" through the device and keeps the factor
 * on the host, C:1721-1846, C:2421-2467; here: whole subtrees).  sf_ooc_partition cuts the supernodal tree for a budget of
 * `budget_entries` resident panel entries (doubles; LU stores two per entry): group[s] = streamed group of supernode s (whole
 * subtrees, consecutive in the postorder) or -1 = top.  The plan keeps the top panels resident and streams the groups through two
 * alternating buffers: group g is factorized while group g - 1 is copied to the host (device need = top + 2 x largest group;
 * *need_entries).  *top_mode (pass it on to the plan): 0 = all top panels resident, factorized after the last group; 1 = when
 * that does not fit: a top panel only while it is ACTIVE (from the first group below it until its own factorization, right after
 * the last one) -- *top_entries is then the arena the active panels share; slower, reaches factors of about three times the budget.  SF_OK: fits (ngroups == 1: in core); SF_ERR_ALLOC: no cut fits, group[] holds the cheapest one.
 * An out-of-core plan runs through sf_chol_plan_factorize_to_host only (the factor exists on the host, never as a whole on the
 * device): it refuses solve / validate / get_factor (SF_ERR_ARG).  SparseFrame_factorize picks this path by itself when the
 * in-core plan does not fit (SF_DEVICE_BUDGET_MB lowers the budget for tests). ---- */
int sf_ooc_partition(sf_long nsuper, const sf_long *Super, const sf_long *SuperMap, const sf_long *Lsip, const sf_long *Lsi,
                     sf_long budget_entries, int32_t *group, int *ngroups, sf_long *group_entries, sf_long *top_entries,
                     sf_long *need_entries, int *top_mode);
int sf_chol_plan_create_ooc(sf_chol_plan **plan, int device, sf_long n, sf_long nsuper,
                            const sf_long *Super, const sf_long *SuperMap,
                            const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                            const sf_long *Lp, const sf_long *Li, const int32_t *group, int ngroups, int top_mode);
/* the same plan without a device (launch list, storage map, byte counts only; see sf_chol_plan_schedule_mapped) */
int sf_chol_plan_schedule_ooc(sf_chol_plan **plan, sf_long n, sf_long nsuper,
                              const sf_long *Super, const sf_long *SuperMap,
                              const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                              const sf_long *Lp, const sf_long *Li, const int32_t *group, int ngroups, int top_mode);

/* ---- distributed top: the top supernodes' large GEMMs are SPLIT over the ranks instead of
 * replicated.  Every top panel is summed over the ranks exactly once, one 512-column block at a time, right before
 * the block's sequential 64-column POTRF/TRSM chain (the only replicated work); everything that updates a block
 * before that -- subtree Schur updates, top-level Schur updates, the block's large-K left-looking GEMM -- is additive,
 * so each rank applies only ITS share (units [rank, rank+1) * units / nranks of the stream-K launch) to its own copy.
 *     sf_chol_plan_factorize_phase(plan, 0)                    own subtrees (as above)
 *     for k in 0 .. sf_chol_plan_num_segments(plan) - 1:
 *         all-reduce(sum) of every region of segment k         (RCCL over xGMI; regions are offsets into
 *         sf_chol_plan_factorize_segment(plan, k)               sf_chol_plan_factor_device_ptr, in doubles)
 * sf_subtree_partition_weighted: partition cost = top_weight * top flops + heaviest rank's subtree flops
 * (top_weight 1 = replicated top; about 1/nranks + the chain's share for the distributed top).
 * sf_chol_plan_set_stream: run the plan on a caller-owned HIP stream (e.g. the stream the collectives are ordered
 * with), so that segments and all-reduces need no host synchronisation between them. ---- */
int sf_subtree_partition_weighted(sf_long nsuper, const sf_long *Super, const sf_long *SuperMap, const sf_long *Lsip,
                                  const sf_long *Lsi, int nranks, double top_weight, int32_t *owner,
                                  double *top_fraction, double *max_load_fraction);
int sf_chol_plan_create_distributed(sf_chol_plan **plan, int device, sf_long n, sf_long nsuper,
                                    const sf_long *Super, const sf_long *SuperMap,
                                    const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                                    const sf_long *Lp, const sf_long *Li, const int32_t *phase, int load_top,
                                    int rank, int nranks);
/* PROPORTIONAL MAPPING of the top: rank `rank`'s plan straight from the owner map of
 * sf_subtree_partition[_weighted].  A top supernode belongs to the GROUP of ranks whose subtrees lie below it: only they
 * store its panel, split its GEMMs and sum its block columns (a sub-communicator per group), and the groups of one level
 * work concurrently.  A rank stores its own subtrees plus the top supernodes on its path to the root instead of the
 * whole top.  Run with sf_chol_plan_factorize_distributed (it creates the sub-communicators on first use). */
int sf_chol_plan_create_mapped(sf_chol_plan **plan, int device, sf_long n, sf_long nsuper,
                               const sf_long *Super, const sf_long *SuperMap,
                               const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                               const sf_long *Lp, const sf_long *Li, const int32_t *owner, int rank, int nranks);
/* ---- schedule inspection: what a rank WILL do, readable without running it.  sf_chol_plan_schedule_mapped /
 * sf_lu_plan_schedule_mapped build rank `rank`'s plan exactly as sf_*_plan_create_mapped does but touch no device and allocate
 * nothing (no GPU needed; the handle only serves the inspection calls below, "bytes_device" of sf_chol_plan_stat -- the bytes the
 * real plan would allocate -- and sf_chol_plan_destroy; everything else returns SF_ERR_ARG).  With them all N plans of a
 * factorization that needs N GPUs (BASELINE config 4: 256^3 over 8) can be checked against each other on a box with one GPU or
 * none: same collective sequence inside every group, split launches partitioned exactly once, every top panel stored by exactly
 * its group (tests/test_config4_schedules.py).  The reference has no counterpart (one host task queue, C:2267).
 *   launch_info   out[10] = kind (0 potrf/getrf, 1 trsm, 2 in-block GEMM, 3 Schur GEMM, 4 outer GEMM, 5 fused step, 6 small Schur),
 *                 tasks, divisible items (GEMM: stream-K units, kind 6: tiles), split (0/1), this rank's window [lo, hi) of the
 *                 items, replicated-bit-identical (0/1), segment index (-1: the rank's own subtrees), index in group, group size
 *   segment_info  out[6] = group mask, first launch, end launch, packed doubles of its all-reduce, early (issued one segment ahead
 *                 on the second stream: 0/1), regions
 *   panel_offsets xp[nsuper] = offset (doubles) of supernode s's panel on this rank, -1 = not stored here
 *   solve_reduce_info  out[3] = group mask, first column, columns: the sums of the distributed forward sweep, in issue order */
int sf_chol_plan_schedule_mapped(sf_chol_plan **plan, sf_long n, sf_long nsuper,
                                 const sf_long *Super, const sf_long *SuperMap,
                                 const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                                 const sf_long *Lp, const sf_long *Li, const int32_t *owner, int rank, int nranks);
sf_long sf_chol_plan_num_launches(const sf_chol_plan *plan);
int sf_chol_plan_launch_info(const sf_chol_plan *plan, sf_long k, sf_long *out10);
int sf_chol_plan_segment_info(const sf_chol_plan *plan, sf_long k, sf_long *out6);
int sf_chol_plan_panel_offsets(const sf_chol_plan *plan, sf_long *xp);
/* OWNER-COMPUTES PROTOTYPE (environment SF_TOP_OWNER=1 at plan creation, Cholesky): in the sets every rank takes
 * part in (the root separator) the near GEMM and the 64-column chain of a 512-column block run on ONE rank (block number mod group
 * size) and the finished block column is broadcast before the split far GEMMs that read it -- instead of running replicated on
 * every rank.  out2[0] = owner's index in the group (-1: replicated, the default), out2[1] = launches of the owner's part.
 * Measured and NOT the default: DESIGN.md section 7. */
int sf_chol_plan_segment_owner(const sf_chol_plan *plan, sf_long k, sf_long *out2);
sf_long sf_chol_plan_num_solve_reduces(const sf_chol_plan *plan);
int sf_chol_plan_solve_reduce_info(const sf_chol_plan *plan, sf_long k, sf_long *out3);
/* bit r set = rank r takes part in the all-reduce of segment k */
uint32_t sf_chol_plan_segment_group(const sf_chol_plan *plan, sf_long k);
sf_long sf_chol_plan_num_segments(const sf_chol_plan *plan);
/* offsets/counts may be NULL to query *nregions only */
int sf_chol_plan_segment_regions(const sf_chol_plan *plan, sf_long k, sf_long capacity, sf_long *nregions,
                                 sf_long *offsets, sf_long *counts);
/* alternative to reducing the regions in place: gather the part of segment k's regions that can be non-zero (rows from
 * each block's first column down) into ONE contiguous device buffer; all-reduce(sum) *device_ptr[0 .. *count) and call
 * sf_chol_plan_factorize_segment(plan, k), which scatters it back first.  One collective per segment and the
 * structurally zero rows above the blocks' diagonals (half of a square root panel) stay off the wire. */
int sf_chol_plan_segment_pack(sf_chol_plan *plan, sf_long k, void **device_ptr, sf_long *count);
int sf_chol_plan_factorize_segment(sf_chol_plan *plan, sf_long k, int sync);
int sf_chol_plan_set_stream(sf_chol_plan *plan, void *hip_stream);

/* ---- the parent-front merge in C: a communicator per rank, RCCL (= NCCL on ROCm, over xGMI) underneath,
 * loaded at run time (librccl.so.1) so that single-GPU users do not need it.
 *   one process per GPU:   rank 0 calls sf_comm_unique_id, hands the 128 bytes to the other ranks by any means (MPI,
 *                          torch.distributed, a file), every rank calls sf_comm_create_rccl(&comm, device, rank, nranks, id)
 *   one process, N GPUs:   SparseFrame_allocate_gpu / sf_handlers_allocate create the communicators themselves
 * sf_chol_plan_factorize_distributed (Cholesky and LU plans): own subtrees, then per segment pack -> all-reduce(sum) ->
 * chain + this rank's share of the split GEMMs, all on the plan's stream; host_out != NULL also copies this rank's pieces
 * of the factor (own panels + its share of the top panels) into host_out while it computes. ---- */
typedef struct sf_comm sf_comm;
int sf_comm_unique_id(char *id128);
int sf_comm_create_rccl(sf_comm **comm, int device, int rank, int nranks, const char *id128);
int sf_comm_rank(const sf_comm *comm);
int sf_comm_size(const sf_comm *comm);
int sf_comm_allreduce_sum(sf_comm *comm, void *device_buf, sf_long count, void *hip_stream);
int sf_comm_destroy(sf_comm *comm);
/* test hook: split the communicator (all ranks, one colour), all-reduce on the child, destroy it */
int sf_comm_selftest_split(sf_comm *comm, void *device_buf, sf_long count, void *hip_stream);
/* Optional, collective: create the sub-communicators of the plan's groups now and check the world and every group of this rank
 * with one 8-byte sum (SF_ERR_HIP when a result is wrong) -- so that a launcher can still fall back when RCCL is not usable. */
int sf_chol_plan_prepare_comm(sf_chol_plan *plan, sf_comm *comm);
int sf_chol_plan_factorize_distributed(sf_chol_plan *plan, sf_comm *comm, sf_float *host_out /* or NULL */, int sync);
/* The solve with a factor that stays distributed (mapped plans after sf_chol_plan_factorize_distributed; Cholesky and LU): b_host =
 * the whole right-hand side in the permuted numbering on every rank; every rank writes into x_host the entries it is responsible
 * for (its subtrees' columns + the columns of the shared supernodes whose group it leads), the others are left alone.  One small
 * sum per shared supernode in the forward sweep is all that travels. */
int sf_chol_plan_solve_distributed(sf_chol_plan *plan, sf_comm *comm, const sf_float *b_host, sf_float *x_host);
/* Failure behaviour of the two distributed drivers: everything that can fail on one rank alone is done first and the ranks agree on
 * the outcome with one 8-byte sum BEFORE the first data collective (a failed rank always joins that sum; its word is allocated with
 * the plan); if any rank failed, every rank returns (its own code, or SF_ERR_PEER) with nothing enqueued on the communicator.  A
 * failure in the MIDDLE of a run (a device or link failure by then) aborts THIS rank's communicator (ncclCommAbort, a local
 * operation): this rank returns its error and later calls on the communicator return SF_ERR_PEER; RCCL peers already inside a
 * collective are NOT released by that -- they rely on their own timeout / the job's supervisor.  Emulated ranks keep their host-side
 * hand-shakes going, so all of them return.  The RCCL paths have been exercised with one rank only (no multi-GPU box so far).
 * sf_test_inject_failure (test hook): rank `rank` fails once at `where` = 1 before the first collective of a factorization, 2 in the
 * middle of its segments, 3 before the first collective of a solve, 4 in the middle of its forward sweep. */
void sf_test_inject_failure(int rank, int where);

/* ---- device plan for supernodal no-pivot LU (replaces L:2668-3573 + LU/Source/cuda_kernel.cu:22-176).
 * Symbolic arrays from sf_symbolic_create_lu; Lsxp is the reference's (packed (2*nsrow-nscol) x nscol) offsets.
 * Up/Ui = U by row; pass NULL for both when the input is symmetric (U aliases L, L:2718-2729).
 * The reference never pivots (magma_dgetrf_nopiv L:2653, cusolverDnDgetrf with devIpiv = NULL L:3344): inputs must
 * be factorizable without pivoting (e.g. diagonally dominant); a zero pivot returns SF_ERR_NOT_POSDEF. ---- */
typedef struct sf_chol_plan sf_lu_plan;
int sf_lu_plan_create(sf_lu_plan **plan, int device, sf_long n, sf_long nsuper,
                      const sf_long *Super, const sf_long *SuperMap,
                      const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                      const sf_long *Lp, const sf_long *Li, const sf_long *Up, const sf_long *Ui);
/* multi-GPU: as sf_chol_plan_create_distributed; the phase / segment / pack / stream entry points of sf_chol_plan_*
 * take an LU plan as they are (same handle type); each segment carries the L and the U^T blocks */
int sf_lu_plan_create_distributed(sf_lu_plan **plan, int device, sf_long n, sf_long nsuper,
                                  const sf_long *Super, const sf_long *SuperMap,
                                  const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                                  const sf_long *Lp, const sf_long *Li, const sf_long *Up, const sf_long *Ui,
                                  const int32_t *phase, int load_top, int rank, int nranks);
int sf_lu_plan_create_mapped(sf_lu_plan **plan, int device, sf_long n, sf_long nsuper,
                             const sf_long *Super, const sf_long *SuperMap,
                             const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                             const sf_long *Lp, const sf_long *Li, const sf_long *Up, const sf_long *Ui,
                             const int32_t *owner, int rank, int nranks);
int sf_lu_plan_schedule_mapped(sf_lu_plan **plan, sf_long n, sf_long nsuper,
                               const sf_long *Super, const sf_long *SuperMap,
                               const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                               const sf_long *Lp, const sf_long *Li, const sf_long *Up, const sf_long *Ui,
                               const int32_t *owner, int rank, int nranks);   /* schedule-only, see sf_chol_plan_schedule_mapped */
/* out of core: as sf_chol_plan_create_ooc (budget: two device doubles per panel entry) */
int sf_lu_plan_create_ooc(sf_lu_plan **plan, int device, sf_long n, sf_long nsuper,
                          const sf_long *Super, const sf_long *SuperMap,
                          const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                          const sf_long *Lp, const sf_long *Li, const sf_long *Up, const sf_long *Ui,
                          const int32_t *group, int ngroups, int top_mode);
int sf_lu_plan_set_values(sf_lu_plan *plan, const sf_float *Lx, const sf_float *Ux /* NULL if U aliases L */);
/* Pivoting (BASELINE config 5 asks for it, the reference has none: magma_dgetrf_nopiv L:2653, devIpiv = NULL
 * L:3344, static pre-pivot L:589-673 disabled).  The symbolic structure is static, so rows can only be exchanged where that
 * keeps the structure: INSIDE the 64 x 64 diagonal block of a 64-column step.  Threshold partial pivoting there -- the natural
 * row keeps the pivot while |a_jj| >= tol * max over the block's unused rows of |a_ij| -- and a pivot smaller than
 * perturb * max|a_ij| is replaced by +- that value ("perturbed_pivots" stat; refine the solution then: sf_lu_plan_refine).
 * tol in [0, 1]: 0 = no pivoting (exactly the reference's behaviour; a zero pivot is SF_ERR_NOT_POSDEF when perturb is 0 too),
 * 1 = partial pivoting.  Defaults: tol 0, perturb 0 = the reference (env SF_LU_PIVOT_TOL at plan creation: that tol and perturb sqrt(eps); SF_LU_PERTURB).  On a
 * matrix whose natural pivots pass the threshold (e.g. diagonally dominant) the factor is bit-identical to the no-pivot one.
 * The interchanges are recorded per block and applied block by block in the forward solve (LINPACK-style: the L entries to
 * the left of a block keep their rows). */
int sf_lu_plan_set_pivoting(sf_lu_plan *plan, double tol, double perturb);
/* pivpos[g] = row position (global permuted index, inside the same 64-column block) of original row g; n entries */
int sf_lu_plan_get_pivots(sf_lu_plan *plan, sf_long *pivpos);
int sf_lu_plan_factorize(sf_lu_plan *plan, int sync);
int sf_lu_plan_sync(sf_lu_plan *plan);
/* D2H copy of the factor gathered into the reference layout: panel s = (2*nsrow-nscol) x nscol column-major,
 * rows [0,nscol) packed L11\U11, [nscol,nsrow) L21, [nsrow,2*nsrow-nscol) U12^T (L:2514-2517) */
int sf_lu_plan_get_factor(sf_lu_plan *plan, sf_float *Lsx);
/* device-side solve with the resident factors: x <- (L U)^{-1} b, permuted space (device twin of L:3592-3700) */
int sf_lu_plan_solve(sf_lu_plan *plan, const sf_float *b_host, sf_float *x_host);
/* sf_chol_plan_solve_many for an LU plan: X <- (L U)^{-1} B, the plan's pivots applied when pivoting is on */
int sf_lu_plan_solve_many(sf_lu_plan *plan, sf_long nrhs, const sf_float *B, sf_long ldb, sf_float *X, sf_long ldx);
/* the transposed solves with the SAME resident factor: x <- A^{-T} b = L^{-T} U^{-T} b, permuted space, the plan's interchanges undone
 * block by block when pivoting is on (no second analysis or factorization of A^T).  Arguments, chunking, layouts, the in-place
 * rule and the stats ("last_solve_ms", "last_solve_many_ms") as sf_lu_plan_solve / sf_lu_plan_solve_many (the device
 * block of the _many form too: allocated by whichever call comes first, SF_ERR_ALLOC leaves the plan usable).  NULL arguments,
 * Cholesky plans (A = A^T: use the plain solve), schedule-only, partial, sharded, mapped and out-of-core plans: SF_ERR_ARG; so is a
 * plan whose last started factorization has not succeeded (as sf_lu_plan_refine). */
int sf_lu_plan_solve_transposed(sf_lu_plan *plan, const sf_float *b_host, sf_float *x_host);
int sf_lu_plan_solve_many_transposed(sf_lu_plan *plan, sf_long nrhs, const sf_float *B, sf_long ldb, sf_float *X, sf_long ldx);
/* ---- half solves and C^T A^{-1} B for LU plans.  Permuted space.  A = L U in the plan's panels; F is what the forward
 * sweep of sf_lu_plan_solve applies: F = L^{-1} without pivoting, F = E_K^{-1} P_K ... E_1^{-1} P_1 with it (the interchanges block
 * by block, see sf_lu_plan_set_pivoting).  So A^{-1} = U^{-1} F and A^{-T} = F^T U^{-T}. ---- */
/* One half of a solve on its own: SF_LU_HALF_L then SF_LU_HALF_U is sf_lu_plan_solve_many, SF_LU_HALF_UT then SF_LU_HALF_LT is
 * sf_lu_plan_solve_many_transposed (e.g. the two sides of a split preconditioner).  Arguments, the chunks of 16, the in-place rule
 * (X == B needs ldx == ldb), the one-column kernels for nrhs == 1 and the stat "last_half_ms" as sf_chol_plan_solve_half; the
 * kernels are those of sf_lu_plan_solve[_many][_transposed].  The two backward halves (U, LT) make their row-major copies of the
 * wide diagonal blocks on the first chunk of every call, from the U^T panels and from the L panels respectively.  nrhs == 0: no-op.
 * NULL pointers, any other `which`, nrhs < 0, a short leading dimension, Cholesky plans, schedule-only, partial, sharded, mapped
 * and out-of-core plans and a plan whose last started factorization has not succeeded: SF_ERR_ARG, nothing written. */
#define SF_LU_HALF_L  0   /* X <- F B       forward sweep over the L panels, unit diagonal, the interchanges applied   */
#define SF_LU_HALF_U  1   /* X <- U^{-1} B  backward sweep over the U^T panels                                         */
#define SF_LU_HALF_UT 2   /* X <- U^{-T} B  forward sweep over the U^T panels, no interchanges                         */
#define SF_LU_HALF_LT 3   /* X <- F^T B     backward sweep over the L panels, the interchanges undone                  */
int sf_lu_plan_solve_half(sf_lu_plan *plan, int which, sf_long nrhs,
                          const sf_float *B, sf_long ldb, sf_float *X, sf_long ldx);
/* G = C^T A^{-1} B for an n x m block C and an n x k block B (m, k <= SF_GRAM_MAX_K): with Z = U^{-T} C and Y = F B, G = Z^T Y --
 * two FORWARD sweeps per pair of chunks and no backward one.  Every chunk of 16 columns of C is swept into its Z block first; then
 * each chunk of B is swept into its Y block and its chunk column of G, the tiles Z_a^T Y_b for every a, is reduced at once with
 * v_mfma_f64_16x16x4_f64.  Z and Y never leave the device; m x k doubles come back.  m == k == 1 runs the one-column sweeps on two
 * n-vectors and a dot product.  C, B: column-major, ldc, ldb >= max(n, 1), both read only (C == B is allowed: B^T A^{-1} B, which
 * is NOT symmetric for an unsymmetric A).  G: column-major m x k, ldg >= max(m, 1), nothing outside the m x k entries is written.
 * m == 0 or k == 0: SF_OK, nothing written; n == 0: zeros.  Refusals as sf_lu_plan_solve_half, and m or k negative or above
 * SF_GRAM_MAX_K.
 * Determinism: the reductions use no floating-point atomics and a fixed order, so for given Z and Y the result repeats bit for
 * bit; entry (i, j) is a function of column i of C and column j of B alone, so a NaN or Inf in column j of B reaches column j
 * of G only and one in column i of C row i of G only.  G is not symmetric, and two calls agree to rounding only where the sweeps
 * scatter with atomics (bit for bit where a sweep has nothing to reorder).
 * The store -- ceil(m / 16) Z blocks and ceil(k / 16) Y blocks of n x 16 doubles, the parts of one chunk column, the padded result
 * block of the host call -- is allocated or grown by the first call that needs it and kept: "bytes_gram" (not in "bytes_device");
 * SF_ERR_ALLOC leaves the plan and a smaller store as they were.  "last_gram_ms", "last_gram_parts" as sf_chol_plan_gram (parts: 0
 * on the one-column path). */
int sf_lu_plan_gram(sf_lu_plan *plan, sf_long m, const sf_float *C, sf_long ldc,
                    sf_long k, const sf_float *B, sf_long ldb, sf_float *G, sf_long ldg);   /* host, column-major */
/* the same on device memory: pointer checks (over the spans of all three blocks) and synchronisation as sf_chol_plan_gram_device;
 * dG must overlap neither input (SF_ERR_ARG).  flags: 0 or SF_DEV_PERM_IN -- BOTH inputs are then in the caller's numbering, the one
 * ordering of sf_lu_plan_set_ordering. */
int sf_lu_plan_gram_device(sf_lu_plan *plan, int flags /* 0 | SF_DEV_PERM_IN */,
                           sf_long m, const sf_float *dC, sf_long ldc,
                           sf_long k, const sf_float *dB, sf_long ldb, sf_float *dG, sf_long ldg);
/* the device-pointer entry points for an LU plan (see sf_chol_plan_set_ordering and below): op is SF_OP_SOLVE or SF_OP_TRANS, both with
 * the plan's interchanges when pivoting is on; set_values_device takes dUx as sf_lu_plan_set_values takes Ux (NULL when U aliases
 * L) and finds max |a_ij|, the scale of the pivot perturbation, on the device.  A Cholesky plan is refused (SF_ERR_ARG). */
int sf_lu_plan_set_ordering(sf_lu_plan *plan, const sf_long *perm);
int sf_lu_plan_solve_device(sf_lu_plan *plan, int op, int flags, sf_long nrhs,
                            const sf_float *dB, sf_long ldb, sf_float *dX, sf_long ldx);
int sf_lu_plan_permute_device(sf_lu_plan *plan, int inverse, sf_long nrhs,
                              const sf_float *dB, sf_long ldb, sf_float *dX, sf_long ldx);
int sf_lu_plan_set_values_device(sf_lu_plan *plan, const sf_float *dLx, const sf_float *dUx /* or NULL */);
int sf_lu_plan_set_value_map(sf_lu_plan *plan, sf_long nsrc, const sf_long *mapL, const sf_long *mapU /* or NULL */);
int sf_lu_plan_set_values_mapped_device(sf_lu_plan *plan, const sf_float *dAx);
/* sf_chol_plan_condest for an LU plan (pivoting on or off); a Cholesky plan is refused (SF_ERR_ARG) */
int sf_lu_plan_condest(sf_lu_plan *plan, sf_float *anorm, sf_float *ainv_norm_est);
/* sf_chol_plan_residual / sf_chol_plan_refine for an LU plan (the solves apply the plan's pivots when pivoting is on); a Cholesky
 * plan is refused (SF_ERR_ARG) */
int sf_lu_plan_residual(sf_lu_plan *plan, const sf_float *b_host, const sf_float *x_host,
                        sf_float *r_host /* or NULL */, sf_float *berr /* or NULL */, sf_float *nerr /* or NULL */);
int sf_lu_plan_refine(sf_lu_plan *plan, const sf_float *b_host, sf_float *x_host,
                      int max_iter, double tol, sf_float *berr /* or NULL */);
/* selected inversion of an LU plan: Sigma = A^{-1} = (L U)^{-1} on the pattern of L + U, permuted space, into a plan-owned pair of
 * device arenas with the device factor's layout.  Synchronous.  Arenas and scratch are allocated by the first call
 * and kept until destroy (stat "bytes_selinv", not in "bytes_device"); SF_ERR_ALLOC leaves the plan usable.  Needs a successful
 * factorization of the current values; whole, resident LU plans only, U aliasing L included (schedule-only, partial, sharded,
 * mapped, out-of-core and Cholesky plans: SF_ERR_ARG).  A plan whose pivot threshold tol is > 0 is refused too (SF_ERR_ARG): the
 * in-block interchanges leave the L entries left of a block in their old rows, so the stored panels are not factors of one
 * row-permuted A.  perturb > 0 with tol == 0 is accepted: Sigma is then the inverse of the perturbed factorization L U, not of A
 * ("perturbed_pivots" tells).  Stats as for sf_chol_plan_selinv: "last_selinv_ms", "flops_selinv", "selinv_valid". */
int sf_lu_plan_selinv(sf_lu_plan *plan);
/* values [e_begin, e_end) of Sigma in the layout of sf_lu_plan_get_factor (xsize doubles, panel s at Lsxp[s],
 * (2*nsrow-nscol) x nscol column-major): rows [0,nscol) the full block Sigma(C_s,C_s), [nscol,nsrow) Sigma(R,C_s),
 * [nsrow,2*nsrow-nscol) Sigma(C_s,R)^T.  SF_ERR_ARG when the arena is not valid. */
int sf_lu_plan_get_selinv_range(sf_lu_plan *plan, sf_long e_begin, sf_long e_end, sf_float *out);
/* diag(Sigma), n doubles, gathered on the device (SF_ERR_ARG when the arena is not valid) */
int sf_lu_plan_selinv_diag(sf_lu_plan *plan, sf_float *d);
/* log|det A| = sum_j log|U_jj| of the resident factor, reduced on the device in a fixed order, and (sign may be NULL) the sign of
 * det A = (-1)^(number of negative U_jj) x the parity of the plan's row interchanges.  Independent of selinv and allowed with
 * pivoting on (the pivot policy must be the one the resident factor was computed with, as for the solves); otherwise refused for the
 * same plan kinds.  Needs a successful factorization of the current values.  In permuted space, which has the determinant of the
 * caller's matrix: the ordering is applied to rows and columns alike. */
int sf_lu_plan_logdet(sf_lu_plan *plan, sf_float *logabs, int *sign);
/* Sigma of an LU plan where the caller wants it (see sf_chol_plan_selinv_values and DESIGN 8k; refusals as there, a Cholesky plan
 * included).  outL[p] = Sigma(Li[p], j) for every position p of column j of L -- the diagonal positions, which the assembly skips,
 * get Sigma_jj; outU[p] = Sigma(j, Ui[p]) for every position p of row j of U.  A plan whose U aliases L has one structure for both
 * triangles: outU must be NULL (otherwise SF_ERR_ARG), and the upper triangle is what the _t form returns. */
int sf_lu_plan_selinv_values(sf_lu_plan *plan, sf_float *outL /* nnz */, sf_float *outU /* unz; NULL when U aliases L */);
int sf_lu_plan_selinv_values_device(sf_lu_plan *plan, sf_float *d_outL, sf_float *d_outU);
/* the transposed entries at the same positions: outL[p] = Sigma(j, Li[p]), outU[p] = Sigma(Ui[p], j) */
int sf_lu_plan_selinv_values_t(sf_lu_plan *plan, sf_float *outL, sf_float *outU);
int sf_lu_plan_selinv_values_t_device(sf_lu_plan *plan, sf_float *d_outL, sf_float *d_outU);
/* out[t] = tr(Sigma M(VL_t, VU_t)) = sum_ij Sigma(j, i) M_ij for the matrix sf_lu_plan_set_values(VL_t, VU_t) would assemble: an
 * entry of L meets the U-side Sigma, an entry of U the L-side one, the diagonal counts once (from U, which stores it) -- for
 * dA/dtheta the derivative of log|det A|.  VU / ldvu as VL / ldvl with unz; U aliasing L: VU must be NULL, VL feeds both
 * triangles.  SF_SEL_MAPPED: VL is the caller's one array (nsrc doubles per column, both parts of the stored map read from it) and
 * VU must be NULL.  Otherwise as sf_chol_plan_selinv_trace. */
int sf_lu_plan_selinv_trace(sf_lu_plan *plan, sf_long m, const sf_float *VL, sf_long ldvl, const sf_float *VU /* or NULL */, sf_long ldvu,
                            int flags /* 0 | SF_SEL_MAPPED */, sf_float *out /* m */);
int sf_lu_plan_selinv_trace_device(sf_lu_plan *plan, sf_long m, const sf_float *dVL, sf_long ldvl, const sf_float *dVU, sf_long ldvu,
                                   int flags, sf_float *d_out /* m */);
/* out[k] = Sigma(rows[k], cols[k]) with (i, j) taken literally; outside the pattern of L + U: a quiet NaN, counted */
int sf_lu_plan_selinv_entries(sf_lu_plan *plan, sf_long count, const sf_long *rows, const sf_long *cols, sf_float *out,
                              sf_long *outside /* or NULL */);
/* sf_chol_plan_adjoint_values for an LU plan: sum_p outL[p] dVL[p] + sum_p outU[p] dVU[p] = alpha sum_c y_c^T M(dVL, dVU) x_c.
 *     outL[p] = alpha sum_c Y[i,c] X[j,c]       for position p at (i, j) of the L structure (column j, i = Li[p])
 *     outU[p] = alpha sum_c Y[j,c] X[Ui[p],c]   for position p of row j of U
 * and exactly 0 where the assembly does not read the position: a superseded duplicate, and the diagonal positions of L (the diagonal
 * is U's).  U aliasing L: outL carries both sums, the diagonal once, and outU must be NULL.  SF_ADJ_MAPPED: outL has nsrc doubles
 * for both parts of the stored map (L's positions are added before U's), outU must be NULL.  For X = A^{-1} B the matching Y is
 * A^{-T} G (SF_OP_TRANS); for X = A^{-T} B the gradient is the call with the two blocks exchanged. */
int sf_lu_plan_adjoint_values(sf_lu_plan *plan, sf_long k, const sf_float *Y, sf_long ldy, const sf_float *X, sf_long ldx, double alpha,
                              int flags /* 0 | SF_ADJ_MAPPED */, sf_float *outL, sf_float *outU /* or NULL */);
int sf_lu_plan_adjoint_values_device(sf_lu_plan *plan, int flags /* 0 | SF_DEV_PERM_IN | SF_ADJ_MAPPED */, sf_long k, const sf_float *dY,
                                     sf_long ldy, const sf_float *dX, sf_long ldx, double alpha, sf_float *d_outL, sf_float *d_outU);
/* sum_p outL[p] dVL[p] + sum_p outU[p] dVU[p] = alpha sf_lu_plan_selinv_trace(dVL, dVU): alpha times the gradient of log|det A|.
 * outL[p] = alpha Sigma(j, i), outU[p] = alpha Sigma(Ui[p], j) where the assembly reads the position, 0 elsewhere -- the diagonal
 * once, from U; U aliasing L: outL[p] = alpha (Sigma(j, i) + Sigma(i, j)) off the diagonal.  Arena and refusals as
 * sf_lu_plan_selinv_values; outU, SF_ADJ_MAPPED as above. */
int sf_lu_plan_logdet_grad_values(sf_lu_plan *plan, double alpha, int flags, sf_float *outL, sf_float *outU /* or NULL */);
int sf_lu_plan_logdet_grad_values_device(sf_lu_plan *plan, double alpha, int flags, sf_float *d_outL, sf_float *d_outU);
double sf_lu_plan_stat(const sf_lu_plan *plan, const char *name);
int sf_lu_plan_set_profiling(sf_lu_plan *plan, int on);
int sf_lu_plan_destroy(sf_lu_plan *plan);

/* ---- device handlers: what SparseFrame_allocate_gpu / _free_gpu / _factorize_supernodal of BOTH struct libraries
 * forward to (reference C:16-366, C:2150-3017).  A handler keeps a lock and a cache of device plans keyed by the
 * symbolic pattern, so repeated factorizations of one pattern pay for the plan once.  lu != 0: LU arrays (Up/Ui/Ux
 * NULL when U aliases L).  serial selects the handler (matrix threads spread over the devices). ---- */
int sf_handlers_allocate(struct common_info_struct *common_info, struct gpu_info_struct **gpu_info_list_ptr);
int sf_handlers_free(struct common_info_struct *common_info, struct gpu_info_struct **gpu_info_list_ptr);
/* device plans built so far by the handlers of a list (a repeated sparsity pattern must not add to it) */
int64_t sf_handlers_plan_builds(struct gpu_info_struct *gpu_info_list, int n_handlers);
/* The device pool of handler d (allocated once in SparseFrame_allocate_gpu, where the reference allocates its eight device slots,
 * C:92-283: min(8 x devSlotSize, a quarter of the device); SF_DEVICE_POOL_MB overrides, 0 = none; one-matrix-per-handler lists only).
 * The handler lends it to the plan of ONE cached pattern at a time for its factor, so that the first SparseFrame_factorize of a
 * pattern does not start with a hipMalloc of tens of GB.  out[0] = bytes, out[1] = 1 while lent, out[2] = n of the borrowing plan. */
int sf_handlers_pool_info(struct gpu_info_struct *list, int d, sf_long *out);
int sf_handlers_factorize(struct common_info_struct *common_info, struct gpu_info_struct *gpu_info_list, int lu, int serial,
                          sf_long n, sf_long nsuper, const sf_long *Super, const sf_long *SuperMap,
                          const sf_long *Lsip, const sf_long *Lsi, const sf_long *Lsxp,
                          const sf_long *Lp, const sf_long *Li, const sf_long *Up, const sf_long *Ui,
                          const sf_float *Lx, const sf_float *Ux, sf_float *Lsx_out,
                          sf_long *PivOut /* LU: row positions after the in-block interchanges (n entries), or NULL */);

/* LU pivoting policy of the struct entry points (process-wide, takes effect at the next SparseFrame_factorize of the LU library).
 * Default: none set = the reference's behaviour, no pivoting and no perturbation (L:2653); tol in (0, 1] switches on threshold partial
 * pivoting inside the 64 x 64 diagonal blocks, perturb > 0 the replacement of pivots below perturb * max|a_ij| (see
 * sf_lu_plan_set_pivoting).  sf_handlers_perturbed_pivots: perturbed pivots of the factorization that filled this host array
 * (-1: unknown array; with several handlers a shared panel's perturbations are counted once per rank that stores it). */
int sf_handlers_set_lu_pivoting(double tol, double perturb);
/* the policy of the NEXT sf_handlers_factorize call made by the calling thread only (how the LU struct library passes a
 * matrix_info's own setting, SparseFrame_set_matrix_pivoting); precedence: this, the process-wide one, the plan's creation default */
int sf_handlers_set_lu_pivoting_next_call(double tol, double perturb);
int64_t sf_handlers_perturbed_pivots(const sf_float *Lsx_host);

/* The struct path's solve with the RESIDENT factor: after SparseFrame_factorize the factor is still in the handler's cached plan (or
 * spread over the handlers' plans); SparseFrame_solve_supernodal (which only receives matrix_info) asks here, by the address of the
 * host copy.  Solves on the device(s) (b, x in the permuted numbering, n doubles each way) when the plan still holds THAT factorization
 * (generation counter) AND the caller's array still is what the device holds: a 64-bit fingerprint of every panel -- sum over its
 * values of bits(v) * (2 index + 1) * K mod 2^64, any single changed value changes it -- is computed over the WHOLE host array (one
 * threaded pass, ~0.1 s for 30 GB) and compared with the device's (computed once per factorization, about one read of the factor).
 * Otherwise returns SF_ERR_ARG and the caller solves on the host as the reference does (C:3036-3139).
 * sf_handlers_set_resident_solve(mode): 0 = never (always the host sweep), 1 = verified as above (default), 2 = trusted: the caller
 * guarantees it does not modify Lsx between factorize and solve; the comparison is skipped (0.02 s instead of 0.13 s at 128^3).
 * SF_SOLVE=host in the environment forces the host solve.  forget: the host copy is being freed. */
int sf_handlers_set_resident_solve(int mode);
/* 1 if this build keeps the A/B environment switches of finished experiments (make EXP=1), 0 for a release build */
int sf_build_experiments(void);
int sf_handlers_solve_resident(const sf_float *Lsx_host, const sf_float *b, sf_float *x);
/* the same with the symbolic arrays of the matrix at hand: after a factorization by SEVERAL handlers the factor is spread over
 * their plans; with these arrays the library can build a whole plan on the first handler's device, gather the panels into it
 * (device to device) and solve there -- when one device has room for the whole factor; otherwise SF_ERR_ARG (host solve) */
int sf_handlers_solve_resident_sym(const sf_float *Lsx_host, const sf_float *b, sf_float *x, int lu, sf_long n, sf_long nsuper,
                                   const sf_long *Super, const sf_long *SuperMap, const sf_long *Lsip, const sf_long *Lsi,
                                   const sf_long *Lsxp, const sf_long *Lp, const sf_long *Li, const sf_long *Up, const sf_long *Ui);
void sf_handlers_forget(const sf_float *Lsx_host);
int64_t sf_handlers_replica_mismatches(const sf_float* Lsx_host); /* values of shared panels that differ bitwise between ranks (tests; -1: not a multi-handler factor) */
int64_t sf_handlers_resident_solves(void);     /* how many solves were served from a resident factor so far (tests) */
int64_t sf_handlers_fingerprint_fallbacks(void); /* verified solves that found Lsx changed (fingerprint mismatch) and left the solve to the host sweep */

/* number of HIP devices visible (0 on a CPU-only box; never fails) */
int sf_device_count(void);
/* version string */
const char *sf_version(void);
/* layout probe for FFI authors: "sizeof_common", "sizeof_matrix", "offsetof_Lsx", "offsetof_workspace",
 * "offsetof_residual", "offsetof_devSlotSize" as this library was compiled; -1 for an unknown name */
long sf_abi_layout(const char *name);

/* total memory of HIP device `device` in bytes (0 if it does not exist) */
size_t sf_device_memory(int device);
/* the reference's slot size for `ndev` devices whose smallest memory is min_mem (C:36-41, C:82-87, C:199) */
size_t sf_reference_slot_size(int ndev, size_t min_mem);

#ifdef __cplusplus
}
#endif
#endif /* SPARSEFRAME_FLAT_H */
