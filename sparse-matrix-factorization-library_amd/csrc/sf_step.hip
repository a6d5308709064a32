// k_step<LU>: one 64-column step of the in-panel factorization in ONE launch (gfx950) -- left-looking update (MFMA) + POTRF / GETRF
// of the diagonal block + TRSM of the rows below (MFMA, from 16 x 16 inverses), with a flag hand-off from the diagonal workgroup to
// the row workgroups inside the launch.  The kernel body claims a task, runs the update and dispatches by ROLE; every role is one
// function below (step_*), inlined into the kernel.  The one-wave panel arithmetic is shared with k_potrf_block / k_getrf_block
// (sf_kernels.hip) through sf_panel.h.  Reference citations as in sf_kernels.hip.
#include "sf_kernels.h"
#include "sf_panel.h"
#include "sf_wave.h"

namespace sf {

// ---------------------------------------------------------------------------------------------------
// Fused 64-column step of the in-panel factorization (latency-bound steps: up to a few rounds of workgroups).
// ONE launch does what used to be three (left-looking update K = 64 t, POTRF / GETRF of the diagonal block, TRSM of
// the rows below):
//   diagonal workgroup (one per panel):   D <- D - Y_D Y_D^T (MFMA) ; D <- chol(D)  (blocked, wave 0 + MFMA) ; publish
//   row workgroups (one per 64 rows):     R <- R - Y_R Y_D^T (MFMA) ; wait for D ; R <- R D^{-T} (blocked, MFMA)
// The row workgroups' update -- most of the step's work -- runs WHILE the diagonal block is being factored; they
// pick the factored block up through a per-(panel, step) flag (release fence + relaxed store by the diagonal
// workgroup, relaxed polls + one acquire fence by the waiting one, device scope; the flag value is the
// factorization's epoch, so flags are never reset).  Liveness: tasks are handed out by an atomic ticket in the order
// the workgroups actually start, and the diagonal tasks (which never wait) come first in the list -- see the top of
// the kernel.  No assumption about the dispatch order or about co-residency of the grid is made.  The wait is
// bounded all the same (info |= 2 -> SF_ERR_HIP instead of a hang).
// Every element of the block column is read and written once.  4 waves (2 x 2), each a 32 x 32 sub-tile = 2 x 2
// v_mfma_f64_16x16x4_f64 tiles; K is short (<= 448), so the MFMA fragments are loaded straight from the panel
// (16 consecutive rows x 4 k per load), 32 k ahead in registers, no LDS staging and no barriers in the K loop.
// The updated 64 x 64 tile then goes to LDS (U[column][row]) where the POTRF wave / the blocked solve picks it up.
// ---------------------------------------------------------------------------------------------------
#ifndef SF_LU_STEP_WGS
#define SF_LU_STEP_WGS 3      // workgroups per CU the LU variant of k_step is compiled for (168 VGPRs; the throughput-bound launches of the lower levels want the third)
#endif
#ifndef SF_POTRF_PW
#define SF_POTRF_PW 16        // columns per panel of the fused step's 64 x 64 POTRF (16 or 32; 32 measured slower, see step_diag_chol)
#endif
constexpr int ST_ULD = ST_ROWS + 1;      // LDS column stride of the updated tile U[c][r]
constexpr int ST_KC = 32;                // K chunk of the update's LDS-staged operand
constexpr int ST_XLD = ST_ROWS + 16;     // its LDS row stride
constexpr int ST_SPIN_LIMIT = 1 << 22;   // ~ seconds

// ONE LDS array, re-used by the phases of a task; the kernel declares the views once and hands each role the ones it uses:
//   Xs[2][32][80]      update:         X staging buffers
//   U[c][r]            diagonal task:  the updated block (POTRF / GETRF works on it);  LU U^T row task: the column permutation
//   Dt[k][j] = D(j,k)  row task:       the factored block;  Cholesky push: X_q parked over the rows 16 q .. of Dt already used
//   Tl[4][16][16]      row task:       the inverses of the four 16 x 16 diagonal sub-blocks of D, behind Dt
// Which view is live between which barriers (every role is entered behind a barrier and leaves the image dead or says otherwise):
//   role                 view     live from                                   until
//   step_update          Xs       the kernel's claim barrier                  the barrier that ends its last chunk
//   step_diag_lu         U        its gather (behind step_update)             its last read, before step_publish's barrier
//   step_diag_chol       U        its gather (behind step_update)             its last read, before step_publish's barrier
//   step_permute_cols    U        step_wait's barrier                         its own closing barrier (Dt / Tl overwrite the image)
//   step_row_solve       Dt, Tl   step_wait's / step_permute_cols' barrier    the end of the solve (push: the barrier of its block q)
//   step_push_next       Dt       the barrier at its top (X parked by solve)  the end of the task
// step_pre_store and the row task's tile load work on registers and global memory only.
constexpr int ST_SMEM = 2 * ST_KC * ST_XLD;
static_assert(NB == ST_ROWS && NB == 64, "one wavefront per 64 x 64 tile");
static_assert(NB * ST_ULD <= ST_SMEM && NB * NB + 4 * 256 <= ST_SMEM, "phases must fit the LDS array");

// What every role needs of its task: set once by the kernel.  (The roles' pointer parameters carry no __restrict__: they are inlined
// into the kernel, whose own parameters do.)
struct StepCtx {
    StepTask t;
    int tid, lane, wave;        // wave w owns rows 16 w .. 16 w + 15 of the tile
    int fr, fk;                 // MFMA fragment coordinates of the lane: lane & 15, lane >> 4
    int64_t ld;
    int b, nrows;
    double* Ag;                 // this tile: rows row0.., columns diag..
    // the diagonal block in the panel the OTHER operand comes from (Cholesky: the same panel; LU: L rows are updated with
    // and solved against the U^T panel's block and vice versa)
    const double* Dg;
    bool is_diag;
};

#ifdef SF_EXP_STEP_STAMPS       // tools/experiments/step_stamps.sh: where the diagonal workgroup of a step spends its time (100 MHz stamps)
__device__ unsigned long long* g_step_stamps = nullptr;
void exp_set_step_stamps(unsigned long long* p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_step_stamps), &p, sizeof(p)); }
#define ST_STAMP(slot) do { if (c.is_diag && c.tid == 0 && g_step_stamps) g_step_stamps[slot] = wall_clock64(); } while (0)
#else
#define ST_STAMP(slot) do { } while (0)
#endif

// Agent-scope coherent load (global_load ... sc1): sees what another workgroup of the RUNNING launch -- possibly on another XCD, whose
// L2 is not coherent with this one's -- stored and released before it raised a flag this workgroup has observed.  The row tasks
// read the few values they take from their diagonal task this way (the factored 64 x 64 block, the 16 x 16 inverses, LU: the pivot
// list) INSTEAD of an agent-scope acquire fence, which invalidates the whole XCD's L2 (buffer_inv sc1): 1.7 us per waiting
// workgroup, 4 us with 500 of them polling (tools/experiments/README.md, step_fence.sh), and every co-resident task's cached
// operands with it.
__device__ __forceinline__ double ld_agent(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_agent(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The MFMA accumulator layout of a task's 64 x 64 tile: wave w holds rows ci = 16 w + fr; entry [q][r] of its four double4
// accumulators is column cj = 16 q + fk + 4 r.  ST_FOR_EACH_ACC(q, r) { ... } runs its body for the lane's 16 entries, fully
// unrolled.  (A macro, like the SV_* fragments of sf_solve.hip: the same loop as a function taking a lambda cost k_step<true> 25
// more spilled SGPRs and 270 v_readlane to reload them, k_step<false> 12.)
#define ST_FOR_EACH_ACC(q, r) _Pragma("unroll") for (int q = 0; q < 4; ++q) _Pragma("unroll") for (int r = 0; r < 4; ++r)
#define ST_ACC_ROW (16 * c.wave + c.fr)
#define ST_ACC_COL(q, r) (16 * (q) + c.fk + 4 * (r))

// Update: wave w owns rows 16 w .. 16 w + 15 of the tile x all 64 columns (4 MFMA tiles).  Its own rows' fragments
// (B operand) come straight from the panel, one chunk ahead in registers -- each element is loaded once; the
// diagonal block's rows (A operand, shared by the 4 waves) go through LDS in 32-deep chunks, staged like k_gemm
// (16-byte row-pair loads, [k][row] image, double-buffered, one barrier per chunk).
// acc += Y X^T over the columns [t.J, t.J + 64 nhp), nhp > 0: K = 64 nhp = 2 nhp chunks of ST_KC = 32
__device__ __forceinline__ void step_update(const StepCtx& c, const double* Lsx, double (*Xs)[ST_KC][ST_XLD], int nhp, double4_t (&acc)[4]) {
    const StepTask& t = c.t;
    const int tid = c.tid, wave = c.wave, fr = c.fr, fk = c.fk, b = c.b, nrows = c.nrows;
    const int64_t ld = c.ld;
    const int nch = 2 * nhp;
    const int prow = 2 * (tid & 31), pk0 = tid >> 5;       // row pair, k = pk0 + 8 q
    // rows beyond b / nrows are clamped: their values only reach accumulator entries replaced by the padding below
    const double* __restrict__ xp = Lsx + t.xpanel + t.diag + (int64_t)t.J * ld + ((prow < b) ? prow : 0);
    const double* __restrict__ yp = Lsx + t.panel + t.row0 + (int64_t)(t.J + fk) * ld + min(16 * wave + fr, nrows - 1);
    // K is short and most launches are a few hundred workgroups (one wave per SIMD): the loop lives on the distance of its
    // prefetches, not on occupancy.  Y fragments: a ring of 4 HALF chunks (16 k each) in registers, every half chunk loaded
    // 1.5 chunks before its use; X: two register sets, loaded 3 chunks ahead of their use and stored to the other LDS buffer
    // one chunk ahead.
    const int nhalf = 2 * nch;
    double2_t rx[2][4];
    double fy[4][4];
    auto load_x = [&](int sel, int h) __attribute__((always_inline)) {
        const int hc = min(h, nch - 1);
#pragma unroll
        for (int q = 0; q < 4; ++q) rx[sel][q] = *reinterpret_cast<const double2_t*>(xp + (int64_t)(hc * ST_KC + pk0 + 8 * q) * ld);
    };
    auto store_x = [&](int buf, int sel) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<double2_t*>(&Xs[buf][pk0 + 8 * q][prow]) = rx[sel][q];
    };
    auto load_y = [&](int slot, int hh) __attribute__((always_inline)) {          // half chunk hh -> ring slot
        const int hc = min(hh, nhalf - 1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) fy[slot][kk] = yp[(int64_t)(hc * (ST_KC / 2) + 4 * kk) * ld];
    };
    // chunk h (h & 1 == par): X from Xs[par], Y from the ring slots 2 par, 2 par + 1; stores chunk h + 1 (register set
    // par ^ 1) and reloads that set with chunk h + 3; half chunks 2 h + 3 and 2 h + 4 are requested on the way
    auto compute = [&](int par, int h) __attribute__((always_inline)) {
        load_y((2 * par + 3) & 3, 2 * h + 3);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            double a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = Xs[par][4 * kk + fk][16 * q + fr];
            if (kk == 0) store_x(par ^ 1, par ^ 1);
            if (kk == 1) load_x(par ^ 1, h + 3);
            if (kk == 4) load_y(2 * par, 2 * h + 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], fy[2 * par + (kk >> 2)][kk & 3], acc[q], 0, 0, 0);
        }
    };
    load_x(0, 0);
    load_x(1, 1);
    load_y(0, 0);
    load_y(1, 1);
    load_y(2, 2);
    store_x(0, 0);
    load_x(0, 2);
    __syncthreads();
    for (int hp = 0; hp < nhp; ++hp) {
        compute(0, 2 * hp);
        __syncthreads();
        compute(1, 2 * hp + 1);
        __syncthreads();
    }
}

// LU pre-update task (mode bit 1): store and done.
// D <- D - (far part of the update), in place: D(ci,cj) lives in the L panel for cj < ci, in the U^T panel (transposed)
// otherwise.  One writer: this launch's row tasks write other columns of these rows, the block's own step comes later.
__device__ __forceinline__ void step_pre_store(const StepCtx& c, double* Lsx, const double4_t (&acc)[4]) {
    const StepTask& t = c.t;
    const int b = c.b;
    const int64_t ld = c.ld;
    double* Ag = c.Ag;
    double* __restrict__ Dw = Lsx + t.xpanel + t.diag + (int64_t)t.diag * ld;
    const int ci = ST_ACC_ROW;
    ST_FOR_EACH_ACC(q, r) {
        const int cj = ST_ACC_COL(q, r);
        const int cic = min(ci, b - 1), cjc = min(cj, b - 1);
        const double dl = Ag[cic + (int64_t)cjc * ld], du = Dw[cjc + (int64_t)cic * ld];       // unconditional, clamped
        if (ci < b && cj < b) {
            if (cj < ci) Ag[ci + (int64_t)cj * ld] = dl - acc[q][r];
            else Dw[cj + (int64_t)ci * ld] = du - acc[q][r];
        }
    }
}

// Row task: the updated tile stays in the MFMA accumulator layout (wave w: rows 16 w + fr, column tile q:
// columns 16 q + fk + 4 r), which is also the B-operand layout of the next MFMA -- the solve below runs on registers
__device__ __forceinline__ void step_row_tile(const StepCtx& c, const double4_t (&acc)[4], double4_t (&rt)[4]) {
    const int b = c.b, nrows = c.nrows;
    const int64_t ld = c.ld;
    const double* Ag = c.Ag;
    const int ci = ST_ACC_ROW;
    ST_FOR_EACH_ACC(q, r) {
        const int cj = ST_ACC_COL(q, r);
        const int cic = min(ci, nrows - 1);
        const double av = Ag[cic + (int64_t)min(cj, b - 1) * ld];          // unconditional, clamped (see step_diag_chol)
        rt[q][r] = (ci < nrows && cj < b) ? av - acc[q][r] : 0.0;
    }
}

// publish: EVERY storing wave drains, the barrier collects them, then ONE device-scope release by lane 0 and
// the flag (the explicit waits keep the order whatever the compiler does with the fence's own wait)
__device__ __forceinline__ void step_publish(const StepCtx& c, int* flags, int flag, int epoch) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (c.tid == 0) {
#ifndef SF_EXP_NO_RELEASE_FENCE     // timing ablation only (tools/experiments/step_fence.sh): what the device-scope release costs
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(flags + flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// LU diagonal task: gather of the block from its two panels, blocked GETRF with threshold pivoting, store in pivot order, the two
// sets of 16 x 16 inverses.  s_piv / s_pos: the kernel's LDS words for the pivot list and the rows' positions.
__device__ __forceinline__ void step_diag_lu(const StepCtx& c, double* Lsx, double* U, int* s_piv, int* s_pos, bool updated,
                                             const double4_t (&acc)[4], int* info, double* tinv, const PivotCtl& pc) {
    const StepTask& t = c.t;
    const int tid = c.tid, lane = c.lane, wave = c.wave, fr = c.fr, fk = c.fk, b = c.b;
    const int64_t ld = c.ld;
    double* Ag = c.Ag;
    const double* Dg = c.Dg;
    // accumulators -> U[cj][ci] = A(ci, cj) - update (padded with the identity / zeros); the staging buffers are dead
    // (the chunk loop ends with a barrier)
    // LU diagonal task: the 64 x 64 block lives in two panels -- D(ci,cj), cj < ci in the L panel, the rest transposed in the U^T
    // panel.  Both halves are read column by column (L) and row by row (U^T) with the lane along the panels' contiguous
    // direction: 32 fully coalesced loads per thread in flight, then the image U[cj][ci] = D(ci, cj) (identity padding beyond
    // b), then the update (the last 64 columns' contribution, in the accumulator layout) subtracted in LDS.  (The first form
    // read the U half in the accumulator layout -- 64 cache lines per load instruction: 3.4 us from entry to the first panel
    // against 2.6 now, profiles/r04_*_step_stamps.txt.  Requested BEFORE the update's K loop the loads overlap it, but their 64
    // registers stay live through the loop for every task of the launch: 247 VGPRs, 2 workgroups per CU instead of 3, and the
    // throughput-bound launches of the lower levels lose more than the diagonal workgroup gains.)
    {
        // (one half at a time: 32 VGPRs each; both in flight at once pushed the kernel past 168 VGPRs = 3 workgroups per CU)
        const int lc = min(lane, b - 1);
        double blk[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) blk[i] = Ag[lc + (int64_t)min(16 * wave + i, b - 1) * ld];     // D(lane, k): column k below its diagonal
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = 16 * wave + i;
            if (lane > k) U[k * ST_ULD + lane] = (lane < b && k < b) ? blk[i] : 0.0;                // (ci = lane, cj = k)
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) blk[i] = Dg[lc + (int64_t)min(16 * wave + i, b - 1) * ld];     // D(k, lane) = PU(lane, k): row k from its diagonal on
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int k = 16 * wave + i;
            if (lane >= k) U[lane * ST_ULD + k] = (lane < b && k < b) ? blk[i] : ((lane == k) ? 1.0 : 0.0);    // (ci = k, cj = lane)
        }
    }
    if (updated) {
        __syncthreads();
        const int ci = ST_ACC_ROW;
        ST_FOR_EACH_ACC(q, r) {
            const int cj = ST_ACC_COL(q, r);
            if (ci < b && cj < b) U[cj * ST_ULD + ci] -= acc[q][r];
        }
    }

    // LU of the updated block with threshold pivoting inside it (pc.tol > 0; implicit interchanges: rows stay where they are
    // until the final store), BLOCKED by 16 columns like the Cholesky path below:
    //   panel    wave 0, lane r holds the 16 panel entries of row r: getrf_panel_wave (pivot search over the rows not used yet,
    //            v_readlane broadcasts of the pivot row, multipliers by v_rcp_f64 + two Newton steps);
    //   U12      the 16 pivot rows of the panel in the columns to its right: one thread per column, forward substitution
    //            with the panel's multipliers (LDS broadcasts);
    //   trailing every wave its 16 rows x the columns to the right with MFMA out of LDS, the multipliers of rows that are
    //            already used (in this or an earlier panel) masked to zero, the U12 rows gathered through the pivot list.
    // The unblocked form (a 64-value row per lane in getrf_panel_wave<true, 64>, 4,000 v_readlane pairs on the critical path) cost 68 us per
    // step and 256 VGPRs; see DESIGN 6b for the figures of this one.
    if (tid < NB) { s_pos[tid] = -1; s_piv[tid] = tid; }
    __syncthreads();
    ST_STAMP(2);
    bool bad = false, active = lane < b;
    int np = 0, pos = lane;
    bool nat_all = true;        // wave 0: every pivot so far was the natural row (wave-uniform)
#pragma unroll 1
    for (int q = 0; q < NB / 16; ++q) {
        const int c0 = 16 * q;
        if (wave == 0) {
            double a[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) a[u] = U[(c0 + u) * ST_ULD + lane];
            // natural pivots first (straight-line code, see getrf_panel_natural); the general search only when one of them fails
            bool done = false;
            if (nat_all) {
                done = getrf_panel_natural<16>(a, lane, c0, b, pc.tol, pc.eps);
                if (done) {
                    if (lane >= c0 && lane < c0 + 16) { active = false; s_piv[lane] = lane; }       // pos stays = lane
                } else {
#pragma unroll
                    for (int u = 0; u < 16; ++u) a[u] = U[(c0 + u) * ST_ULD + lane];
                }
            }
            if (!done) {
                nat_all = false;
                getrf_panel_wave<true, 16>(a, lane, c0, b, pc.tol, pc.eps, bad, np, pos, active, s_piv);
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) U[(c0 + u) * ST_ULD + lane] = a[u];
            s_pos[lane] = active ? -1 : pos;
        }
        if (q == NB / 16 - 1 || c0 + 16 >= b) break;      // nothing but identity padding to the right (narrow panel)
        __syncthreads();
        const int ntr = NB - c0 - 16;               // columns to the right of the panel
        if (tid < ntr) {
            const int cc = c0 + 16 + tid;
            double x[16];
            int pr[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) { pr[k] = s_piv[c0 + k]; x[k] = U[cc * ST_ULD + pr[k]]; }
#pragma unroll
            for (int k = 1; k < 16; ++k)
#pragma unroll
                for (int jj = 0; jj < k; ++jj) x[k] -= U[(c0 + jj) * ST_ULD + pr[k]] * x[jj];
#pragma unroll
            for (int k = 1; k < 16; ++k) U[cc * ST_ULD + pr[k]] = x[k];
        }
        __syncthreads();
        {
            const int ci = 16 * wave + fr;          // this wave's 16 rows
            const bool free_row = s_pos[ci] < 0;
            double lf[4];
            int pk[4];
#pragma unroll
            for (int sgm = 0; sgm < 4; ++sgm) {
                const double v = U[(c0 + 4 * sgm + fk) * ST_ULD + ci];
                lf[sgm] = free_row ? v : 0.0;                                                   // B[k][j = ci]
                pk[sgm] = s_piv[c0 + 4 * sgm + fk];
            }
            // (this loop and its twin in step_diag_chol stay two: one function for both, the A operand passed as a lambda, added
            //  3 / 2 ds_read instructions to k_step<true> / k_step<false>)
            for (int ct = q + 1; ct < NB / 16; ++ct) {
                const int cb = 16 * ct;
                double4_t d;
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r] = U[(cb + fk + 4 * r) * ST_ULD + ci];          // D[i = column][j = row ci]
#pragma unroll
                for (int sgm = 0; sgm < 4; ++sgm)
                    d = __builtin_amdgcn_mfma_f64_16x16x4f64(-U[(cb + fr) * ST_ULD + pk[sgm]], lf[sgm], d, 0, 0, 0);   // A[i][k] = U12(k, cb + i)
#pragma unroll
                for (int r = 0; r < 4; ++r) U[(cb + fk + 4 * r) * ST_ULD + ci] = d[r];
            }
        }
        __syncthreads();
        ST_STAMP(3 + q);
    }
    ST_STAMP(6);
    if (wave == 0) {
        if (bad && lane == 0) atomicOr(info, 1);
        if (np > 0 && lane == 0) atomicAdd(pc.nperturb, np);
        if (pc.pivpos && lane < b) {
            const int g0 = t.first_col + t.diag;
            pc.pivpos[g0 + lane] = g0 + pos;
            pc.pivinv[g0 + pos] = g0 + lane;
        }
    }
    __syncthreads();
    {
        // The factored block goes to the two panels, rows at their pivot positions, every store instruction along a panel's
        // contiguous direction.  L part: wave w takes the columns 16 w .. 16 w + 15, lane = row POSITION (its values come from
        // the row s_piv[position] of the LDS image); with interchanges the image itself is brought into pivot order on the way
        // (a wave's reads of a column precede its writes, no other wave touches these columns).  U part: from the ordered image,
        // wave w takes the rows 16 w .. 16 w + 15, lane = column.  (Stored in the accumulator-like layout, the first form issued
        // 64 cache lines per store instruction for the U half: 2.0 us + a longer drain before the flag.)
        const int src = s_piv[lane];                     // the row that ended at position `lane`
        const bool moved = !__all(src == lane);         // same answer in every wave (one pivot list)
        double* __restrict__ PUd = Lsx + t.xpanel + t.diag + (int64_t)t.diag * ld;
        double a[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) a[u] = U[(16 * wave + u) * ST_ULD + src];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int cc = 16 * wave + u;
            if (lane < b && cc < lane) Ag[lane + (int64_t)cc * ld] = a[u];
            if (moved) U[cc * ST_ULD + lane] = a[u];
        }
        if (moved) __syncthreads();
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = 16 * wave + u;
            const double v = U[lane * ST_ULD + r];
            if (lane < b && r <= lane) PUd[lane + (int64_t)r * ld] = v;
        }
    }
    ST_STAMP(7);
    {
        // inverses of the 16 x 16 diagonal sub-blocks the row tasks solve against: of U11^T (lower, for the L rows) at
        // tinv[slot][0][w], of the unit-lower L11 (for the U^T rows) at tinv[slot][1][w]; wave w does block w of both -- the two
        // sets side by side in ONE substitution: lanes 0..15 hold the columns of the first, lanes 16..31 of the second (the
        // matrix entry a step multiplies by is an LDS broadcast per set: two addresses per read), lanes 32..63 repeat them.
        // (One set after the other in every lane, the first form, was 3.3 us of the diagonal workgroup's 40; Cholesky's one set 2.0.)
        // (The substitution is written out here and in step_diag_chol: one function for both -- strides, unit flag and column as
        //  arguments, constants in Cholesky's call -- cost k_step<true> a sixth spilled VGPR, 28 instead of 24 bytes of scratch.)
        const int o = 16 * wave, j = lane & 15;
        const bool lset = (lane & 16) != 0;
        // entry (r, c) of the set's matrix: U11^T(r,c) = U11(c,r) = row o+c, column o+r of the block (U[column][row] image:
        // offset r * ULD + c); L11(r,c) = row o+r, column o+c (offset c * ULD + r) -- per-lane strides, ONE read per step
        const int sr = lset ? 1 : ST_ULD, sc = lset ? ST_ULD : 1;
        const double* __restrict__ Ub = U + o * ST_ULD + o;
        double w[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            double sacc = (r == j) ? 1.0 : 0.0;
#pragma unroll
            for (int cc = 0; cc < r; ++cc) sacc -= Ub[r * sr + cc * sc] * w[cc];
            const double trr = Ub[r * (ST_ULD + 1)];
            const double rp = rcp_full(trr);
            w[r] = lset ? sacc : sacc * rp;
        }
        double* __restrict__ out = tinv + (int64_t)t.slot * 2048 + (lset ? 1024 : 0) + wave * 256 + j * 16;
        if (lane < 32) {
#pragma unroll
            for (int r = 0; r < 16; ++r) out[r] = w[r];
        }
    }
    ST_STAMP(8);
}

// Cholesky diagonal task: gather of the block, blocked POTRF, the 16 x 16 inverses.
__device__ __forceinline__ void step_diag_chol(const StepCtx& c, double* U, const double4_t (&acc)[4], int* info, double* tinv) {
    const StepTask& t = c.t;
    const int lane = c.lane, wave = c.wave, fr = c.fr, fk = c.fk, b = c.b, nrows = c.nrows;
    const int64_t ld = c.ld;
    double* Ag = c.Ag;
    // accumulators -> U[cj][ci] = A(ci, cj) - update (padded with the identity / zeros); the staging buffers are dead
    // (the chunk loop ends with a barrier)
    const int ci = ST_ACC_ROW;
    ST_FOR_EACH_ACC(q, r) {
        const int cj = ST_ACC_COL(q, r);
        // loads are unconditional (clamped addresses) and selected afterwards: a load under a per-element
        // condition costs a branch and its own wait, i.e. 16 dependent round trips per lane
        const int cic = min(ci, nrows - 1), cjc = min(cj, b - 1);
        double v = (ci == cj) ? 1.0 : 0.0;
        const double av = Ag[cic + (int64_t)cjc * ld];
        if (ci < nrows && cj < b && cj <= ci) v = av - acc[q][r];
        U[cj * ST_ULD + ci] = v;
    }

    __syncthreads();
    ST_STAMP(2);
    // POTRF of the updated block, blocked by 16 columns.  Panel part: wave 0, lane r holds row r of the 16 columns
    // (k_potrf_block's scheme; the column scaling of all 64 rows comes with it, so there is no separate TRSM).
    // Trailing part: every wave updates its 16 rows of the columns to the right with MFMA out of LDS,
    //   U[cj][ci] -= sum_k L(cj,k) L(ci,k),  k in the panel  (A operand = -L rows cj, B operand = L rows ci)
    bool bad = false;
    // PW columns per panel.  32 = two panels per block instead of four -- half the barriers and trailing passes on the step's
    // critical path, at the price of more of the elimination in the broadcast form (496 instead of 120 (column, column) pairs per
    // panel) -- was measured (round 4) and is SLOWER: the panel becomes issue-bound on its v_readlane / v_fma pairs; config 3
    // 11.6 ms against 11.2 (fused steps 5.4 against 5.0), 128^3 fused steps 58.0 against 55.7 ms.
    constexpr int PW = SF_POTRF_PW;
#pragma unroll
    for (int q = 0; q < NB / PW; ++q) {
        const int c0 = q * PW;
        if (wave == 0) {
            double a[PW];
#pragma unroll
            for (int u = 0; u < PW; ++u) a[u] = U[(c0 + u) * ST_ULD + lane];
            // dnext: what the NEXT column's diagonal entry will be, formed in its own lane (a[j+1] - lj^2 there: the same fused
            // multiply-add as the general update below, whose multiplier for that lane is the lane's own lj) -- so the chain from one
            // pivot to the next has ONE lane broadcast in it instead of two
            double dnext = a[0];
#pragma unroll
            for (int j = 0; j < PW; ++j) {
                if (PW > 16 && j == 16 && c0 + 16 >= b) break;          // narrow block: the rest of the panel is identity padding
                const double djj = readlane_f64(dnext, c0 + j);
                bad = bad || !(djj > 0.0);
                // (rsqrt_full; no select: the diagonal lane's own entry is djj, lanes above the diagonal carry values nobody reads --
                //  see potrf_block_w)
                const double rinv = rsqrt_full(djj);
                const double lj = a[j] * rinv;
                a[j] = lj;
                if (j + 1 < PW) dnext = __builtin_fma(-lj, lj, a[j + 1]);
#pragma unroll
                for (int cc = j + 1; cc < PW; ++cc) a[cc] = __builtin_fma(-lj, readlane_f64(lj, c0 + cc), a[cc]);
            }
#pragma unroll
            for (int u = 0; u < PW; ++u) {
                U[(c0 + u) * ST_ULD + lane] = a[u];
                if (lane < b && c0 + u <= lane) Ag[lane + (int64_t)(c0 + u) * ld] = a[u];
            }
        }
        if (q == NB / PW - 1 || c0 + PW >= b) break;      // nothing but identity padding to the right (narrow panel)
        __syncthreads();
        if (16 * wave >= c0 + PW) {
            const int ci = wave * 16 + fr;                  // this wave's 16 rows
            double lf[PW / 4];
#pragma unroll
            for (int sgm = 0; sgm < PW / 4; ++sgm) lf[sgm] = U[(c0 + 4 * sgm + fk) * ST_ULD + ci];            // B[k][j = ci]
            for (int ct = (c0 + PW) / 16; ct <= wave; ++ct) {
                const int cb = ct * 16;
                double4_t d;
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r] = U[(cb + fk + 4 * r) * ST_ULD + ci];                    // D[i = cj][j = ci]
#pragma unroll
                for (int sgm = 0; sgm < PW / 4; ++sgm)
                    d = __builtin_amdgcn_mfma_f64_16x16x4f64(-U[(c0 + 4 * sgm + fk) * ST_ULD + cb + fr], lf[sgm], d, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) U[(cb + fk + 4 * r) * ST_ULD + ci] = d[r];
            }
        }
        __syncthreads();
        ST_STAMP(3 + q);
    }
    ST_STAMP(6);
    if (bad && wave == 0 && lane == 0) atomicOr(info, 1);
    // Inverses of the four 16 x 16 diagonal sub-blocks of L (what MAGMA-style TRSMs use): wave w inverts block w by
    // forward substitution, lane j (< 16) holds column j of the inverse, the entries of T are LDS broadcasts.  The
    // row tasks then solve with MFMA only -- X_q = R_q T_q^{-T} -- instead of a one-wave substitution.
    __syncthreads();
    {
        const int o = 16 * wave;
        double wv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            double sacc = (r == (lane & 15)) ? 1.0 : 0.0;
#pragma unroll
            for (int cc = 0; cc < r; ++cc) sacc -= U[(o + cc) * ST_ULD + o + r] * wv[cc];
            const double trr = U[(o + r) * ST_ULD + o + r];
            const double rp = rcp_full(trr);
            wv[r] = sacc * rp;          // rows above the diagonal come out as exact zeros (zero right-hand side so far)
        }
        // Tinv_w(r, j) at tinv[slot][w][j][r]: the [k][i] image the consumers' MFMA A operand reads
        double* __restrict__ out = tinv + (int64_t)t.slot * 1024 + wave * 256 + (lane & 15) * 16;
        if (lane < 16) {
#pragma unroll
            for (int r = 0; r < 16; ++r) out[r] = wv[r];
        }
    }
    ST_STAMP(8);
}

// Row task: wait for this panel's diagonal block of this step
__device__ __forceinline__ void step_wait(const StepCtx& c, int* flags, int flag, int epoch, int* info) {
    if (c.tid == 0) {
        int spins = 0;
        // relaxed polls (an acquire load would invalidate this CU's caches at every iteration, and with hundreds of
        // waiting workgroups that slows the whole chip down).  No acquire fence follows: everything this task reads of the
        // diagonal task's output is read with agent-scope loads (ld_agent), issued after the barrier below, i.e. after the flag
        // has been SEEN; the diagonal task released its stores (L2 write-back) before it raised the flag.
        while (__hip_atomic_load(flags + flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
            __builtin_amdgcn_s_sleep(16);
            if (++spins > ST_SPIN_LIMIT) { atomicOr(info, 2); break; }
        }
#ifdef SF_EXP_ACQUIRE_FENCE         // the former protocol (timing comparison only)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}

// LU row task with mode bit 0, pivoting on:
// U^T rows: the tile's 64 columns are the block's rows of U; the diagonal workgroup interchanged rows, so the columns
// are brought into pivot order (position p <- original column pivinv[p]).  Through LDS ([column][row] image), the
// accumulator layout is per-lane fixed.  Skipped (wave-uniform test) when the block kept its natural order.
__device__ __forceinline__ void step_permute_cols(const StepCtx& c, const int32_t* pivinv, double* U, double4_t (&rt)[4]) {
    const int b = c.b;
    const int g0 = c.t.first_col + c.t.diag;
    int src[16];
    bool ident = true;
    ST_FOR_EACH_ACC(q, r) {
        const int cj = ST_ACC_COL(q, r);
        src[4 * q + r] = (cj < b) ? ld_agent(pivinv + g0 + cj) - g0 : cj;
        ident = ident && src[4 * q + r] == cj;
    }
    if (!__all(ident)) {            // per wave; the waves' rows are disjoint, so is their part of the LDS image
        const int ci = ST_ACC_ROW;
        ST_FOR_EACH_ACC(q, r) U[ST_ACC_COL(q, r) * ST_ULD + ci] = rt[q][r];
        ST_FOR_EACH_ACC(q, r) rt[q][r] = U[src[4 * q + r] * ST_ULD + ci];
    }
    __syncthreads();                // the image is overwritten by Dt / Tl below
}

// X <- R D^{-T} with MFMA only, per wave (its 16 rows are independent of the other waves'): for every 16-column
// block q   X_q = R_q T_q^{-T}   (A operand = the block's inverse, B operand = R_q as it sits in the registers),
// then   R_q' -= X_q D(q', q)^T  for the blocks q' to the right (A operand = -D from Dt, B operand = X_q).
// D = L11 (Cholesky), U11^T (LU, L rows) or the unit-lower L11 (LU, U^T rows: mode bit 0)
// park (Cholesky, t.next_b > 0): X_q is left in LDS for step_push_next
template <bool LU>
__device__ __forceinline__ void step_row_solve(const StepCtx& c, const double* tinv, double (*Dt)[NB], double* Tl, bool park, double4_t (&rt)[4]) {
    const StepTask& t = c.t;
    const int tid = c.tid, wave = c.wave, fr = c.fr, fk = c.fk, b = c.b, nrows = c.nrows;
    const int64_t ld = c.ld;
    double* Ag = c.Ag;
    const double* Dg = c.Dg;
    const double* __restrict__ tsrc = tinv + (int64_t)t.slot * (LU ? 2048 : 1024) + ((LU && (t.mode & 1)) ? 1024 : 0);
    {
        double dv[NB * NB / 256], tv[4];
#pragma unroll
        for (int i = 0; i < NB * NB / 256; ++i) {       // all loads in flight (clamped addresses), then select + store
            const int e = tid + 256 * i, k = e / NB, j = e % NB;
            dv[i] = ld_agent(Dg + min(j, b - 1) + (int64_t)min(k, b - 1) * ld);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) tv[i] = ld_agent(tsrc + tid + 256 * i);
#pragma unroll
        for (int i = 0; i < NB * NB / 256; ++i) {
            const int e = tid + 256 * i, k = e / NB, j = e % NB;
            Dt[k][j] = (j < b && k < j) ? dv[i] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) Tl[tid + 256 * i] = tv[i];
    }
    __syncthreads();
    const int ci = 16 * wave + fr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (16 * q >= b) break;                              // narrow panel: the remaining blocks are padding
        double4_t x = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int sg = 0; sg < 4; ++sg)
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(Tl[q * 256 + (4 * sg + fk) * 16 + fr], rt[q][sg], x, 0, 0, 0);
#pragma unroll
        for (int qq = q + 1; qq < 4; ++qq)
#pragma unroll
            for (int sg = 0; sg < 4; ++sg)
                rt[qq] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Dt[16 * q + 4 * sg + fk][16 * qq + fr], x[sg], rt[qq], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cj = 16 * q + fk + 4 * r;
            if (ci < nrows && cj < b) Ag[ci + (int64_t)cj * ld] = x[r];
        }
        if (park) {
            // (push, see step_push_next) park X_q in LDS where Dt rows 16 q .. 16 q + 15 were: [k][row] image, dead once every
            // wave has passed this iteration.  next_b > 0 implies b == 64: all waves run all four iterations.
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 4; ++r) Dt[16 * q + fk + 4 * r][ci] = x[r];
        }
    }
}

// Cholesky row task with t.next_b > 0, behind step_row_solve (which parked X in Dt):
// These 64 rows are a FUTURE diagonal block of this outer block (rows = columns [row0, row0 + next_b) of the
// panel): subtract this step's contribution X X^T from it now (right-looking, lower triangle), so that its own
// step finds it up to date and its diagonal workgroup -- the step's critical path -- starts the POTRF at once.
// One workgroup per (step, future block), steps are separate launches: plain read-modify-write.
__device__ __forceinline__ void step_push_next(const StepCtx& c, double* Lsx, double (*Dt)[NB]) {
    const StepTask& t = c.t;
    const int wave = c.wave, fr = c.fr, fk = c.fk;
    const int64_t ld = c.ld;
    const int ci = 16 * wave + fr;
    __syncthreads();
    double* __restrict__ Dn = Lsx + t.panel + t.row0 + (int64_t)t.row0 * ld;
    const int nb = t.next_b;
    for (int ct = 0; ct <= wave; ++ct) {
        double4_t d = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int sg = 0; sg < 16; ++sg)         // A[i = cj][k], B[k][j = ci]
            d = __builtin_amdgcn_mfma_f64_16x16x4f64(Dt[4 * sg + fk][16 * ct + fr], Dt[4 * sg + fk][ci], d, 0, 0, 0);
        double old[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cj = 16 * ct + fk + 4 * r;
            old[r] = Dn[min(ci, nb - 1) + (int64_t)min(cj, nb - 1) * ld];               // unconditional, clamped
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int cj = 16 * ct + fk + 4 * r;
            if (ci < nb && cj <= ci) Dn[ci + (int64_t)cj * ld] = old[r] - d[r];
        }
    }
}

template <bool LU>
__global__ void __launch_bounds__(256, LU ? SF_LU_STEP_WGS : 3)   // LU: the unblocked GETRF keeps a 64-value row per lane
k_step(const StepTask* __restrict__ tasks, double* __restrict__ Lsx, int* __restrict__ flags, int epoch, int* __restrict__ info,
       double* __restrict__ tinv, int* __restrict__ ticket, PivotCtl pc) {
    // the LDS array and its views (see the table at ST_SMEM)
    __shared__ __attribute__((aligned(16))) double smem[ST_SMEM];
    double (*Xs)[ST_KC][ST_XLD] = reinterpret_cast<double (*)[ST_KC][ST_XLD]>(smem);
    double* U = smem;
    double (*Dt)[NB] = reinterpret_cast<double (*)[NB]>(smem);
    double* Tl = smem + NB * NB;

    // Tasks are claimed in EXECUTION order (one atomic ticket per workgroup), not by blockIdx: the diagonal tasks come
    // first in the list, so every one of them is held by a workgroup that is already running -- and never waits -- by
    // the time any row task is claimed.  A waiting workgroup can therefore never keep the one it waits for off the
    // chip, whatever order the hardware dispatches the grid in and whatever else shares the GPU.
    __shared__ int s_ticket;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef SF_EXP_STEP_STAMPS
    const unsigned long long st_entry = wall_clock64();
#endif
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const StepTask t = tasks[__builtin_amdgcn_readfirstlane(s_ticket)];
    // LU, mode bit 1: a PRE-UPDATE task -- the far part (columns [J, diag - 64)) of the left-looking update of the diagonal block of
    // the NEXT step, done one launch early and off the critical path (everything it reads is final when this launch starts); that
    // step's diagonal workgroup then only applies the last 64 columns before it factors (see the task list in sf_chol_plan.hip)
    const bool is_pre = LU && (t.mode & 2);
    const bool is_diag = t.row0 == t.diag && !is_pre;
    const StepCtx c = {t, tid, lane, wave, lane & 15, lane >> 4, t.ld, t.b, t.nrows,
                       Lsx + t.panel + t.row0 + (int64_t)t.diag * t.ld, Lsx + t.xpanel + t.diag + (int64_t)t.diag * t.ld, is_diag};
#ifdef SF_EXP_STEP_STAMPS
    if (is_diag && tid == 0 && g_step_stamps) g_step_stamps[0] = st_entry;
#endif
    ST_STAMP(1);

    double4_t acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = (double4_t){0.0, 0.0, 0.0, 0.0};
    // (Cholesky diagonal tasks come with J == diag, i.e. no update: the block was brought up to date right-looking by the
    // earlier steps of this outer block -- each step's row tile that holds a future diagonal block pushes its own X X^T
    // into it, see step_push_next -- so the diagonal workgroup, the step's critical path, starts its POTRF at once)
    const int nhp = ((is_pre ? t.diag - NB : t.diag) - t.J) / NB;
    if (nhp > 0) step_update(c, Lsx, Xs, nhp, acc);

    if (is_pre) {
        step_pre_store(c, Lsx, acc);
        return;
    }
    double4_t rt[4];
    if (!is_diag) step_row_tile(c, acc, rt);
    if (is_diag) {
        if constexpr (LU) {
            __shared__ int s_piv[NB], s_pos[NB];
            step_diag_lu(c, Lsx, U, s_piv, s_pos, nhp > 0, acc, info, tinv, pc);
        } else {
            step_diag_chol(c, U, acc, info, tinv);
        }
        step_publish(c, flags, t.flag, epoch);
        ST_STAMP(9);
        return;
    }

    step_wait(c, flags, t.flag, epoch, info);
    if (LU && (t.mode & 1) && pc.pivinv) step_permute_cols(c, pc.pivinv, U, rt);
    const bool push = !LU && t.next_b > 0;
    step_row_solve<LU>(c, tinv, Dt, Tl, push, rt);
    if (push) step_push_next(c, Lsx, Dt);
}

void launch_step(const StepTask* tasks, int ntasks, int lu, double* Lsx, int* flags, int epoch, int* info, double* tinv, int* ticket,
                 PivotCtl pc, hipStream_t st) {
    if (ntasks <= 0) return;
    if (lu) hipLaunchKernelGGL(k_step<true>, dim3(ntasks), dim3(256), 0, st, tasks, Lsx, flags, epoch, info, tinv, ticket, pc);
    else hipLaunchKernelGGL(k_step<false>, dim3(ntasks), dim3(256), 0, st, tasks, Lsx, flags, epoch, info, tinv, ticket, pc);
}

}  // namespace sf
