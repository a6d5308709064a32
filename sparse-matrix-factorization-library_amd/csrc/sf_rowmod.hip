// Row deletion and row addition on the resident Cholesky factor: row and column j of A become the identity's
// (rowdel) or get new values (rowadd) with the pattern of L unchanged, on top of the rank-1 rotations of sf_updown.hip.
//
// rowdel(j), j = column c of supernode s:  row j of L left of the diagonal <- 0 (k_rowmod_zero_rows over the panels that hold it),
// w <- L(j + 1:, j) into column 0 of the block of W, that column <- 0, L_jj <- 1 (k_rowdel_column), then the rank-1 UPDATE of
// the trailing factor with w.
// rowadd(j, a): a into column 0 of W; the forward sweep L11 l12 = a12 along the chains of a12's indices, 64 columns per pair of
// launches: k_rowadd_sweep_diag solves one diagonal block against its rows of W and leaves y, k_rowadd_sweep_rows does
// W[row] -= sum L(row, col) y_col for the panel rows below -- the lane whose row is j stores y into L(j, cols) first, so that W[j]
// collects a22 - l12^T l12 by itself --; k_rowadd_column writes L_jj = sqrt(W[j]) and L(j + 1:, j) = W / L_jj, which stays in W as
// the vector of the rank-1 DOWNDATE that follows.
// No kernel waits for another workgroup: the order of the launches is the stream's.  Square root and divisions are the IEEE ones,
// as in sf_updown.hip.
#include <sparseframe_hip.h>

#include <algorithm>
#include <vector>

#include "sf_plan_internal.h"
#include "sf_rowmod_path.h"
#include "sf_panel.h"

namespace sf {

namespace {

constexpr int RM_WG = 256;

// one workgroup per task (offset of the row's first entry from L, its stride, its length).  check == 0: the entries <- 0.
// check != 0: nothing is written but *flag <- 1 when an entry is not zero, or L[one_off] (one_off >= 0) is not 1.
__global__ __launch_bounds__(RM_WG) void k_rowmod_zero_rows(double* __restrict__ L, const int64_t* __restrict__ tasks, int64_t one_off, int check,
                                                            int* __restrict__ flag) {
    const int64_t off = tasks[3 * (int64_t)blockIdx.x], ld = tasks[3 * (int64_t)blockIdx.x + 1], count = tasks[3 * (int64_t)blockIdx.x + 2];
    bool bad = false;
    for (int64_t q = threadIdx.x; q < count; q += RM_WG) {
        if (check) bad = bad || !(L[off + q * ld] == 0.0);
        else L[off + q * ld] = 0.0;
    }
    if (check && blockIdx.x == 0 && threadIdx.x == 0 && one_off >= 0) bad = bad || !(L[one_off] == 1.0);
    if (bad) *flag = 1;
}

// col = &L_jj in its panel, the nbelow entries behind it are the column below the diagonal; rows[i] = the row of entry 1 + i
__global__ __launch_bounds__(RM_WG) void k_rowdel_column(double* __restrict__ col, int64_t nbelow, const int32_t* __restrict__ rows,
                                                         double* __restrict__ W) {
    const int64_t i = (int64_t)blockIdx.x * RM_WG + threadIdx.x;
    if (i == 0) col[0] = 1.0;
    if (i >= nbelow) return;
    W[(int64_t)rows[i] * UPD_W] = col[1 + i];
    col[1 + i] = 0.0;
}

// One wave, lane = row of the b x b block D (lower triangle, column-major): forward substitution D y = w on column 0 of the
// block's rows of W.  The triangle waits in LDS as in k_updown_diag (32 KB); y_j is wave-uniform: every lane divides the same w_j
// by the same d.  y goes to y[0 .. b), zeros to column 0 of the block's rows of W.
__global__ __launch_bounds__(64) void k_rowadd_sweep_diag(const double* __restrict__ D, int64_t ld, int b, double* __restrict__ W,
                                                          double* __restrict__ y) {
    __shared__ double blk[UPD_B * UPD_B];
    const int lane = threadIdx.x;
    const bool in = lane < b;
    for (int j = 0; j < b; ++j)
        if (in && j <= lane) blk[j * UPD_B + lane] = D[(int64_t)j * ld + lane];
    double w = in ? W[(int64_t)lane * UPD_W] : 0.0;
    double mine = 0.0;
    __syncthreads();
    for (int j0 = 0; j0 < b; ++j0) {
        const int j = __builtin_amdgcn_readfirstlane(j0);
        const double yj = readlane_dyn_f64(w, j) / blk[j * UPD_B + j];
        if (lane == j) mine = yj;
        if (in && lane > j) w -= blk[j * UPD_B + lane] * yj;
    }
    if (in) {
        y[lane] = mine;
        W[(int64_t)lane * UPD_W] = 0.0;
    }
}

// lane = panel row i below the block (b columns, leading dimension ld), rows[i] its row of W:  W[rows[i]] -= sum_col P(i, col)
// y_col, column after column.  The lane whose row is `target` (-1: none) stores y into its panel row first.
__global__ __launch_bounds__(RM_WG) void k_rowadd_sweep_rows(double* __restrict__ P, int64_t ld, int b, int64_t nrows,
                                                             const int32_t* __restrict__ rows, int32_t target, double* __restrict__ W,
                                                             const double* __restrict__ y) {
    __shared__ double sh[UPD_B];
    if (threadIdx.x < b) sh[threadIdx.x] = y[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * RM_WG + threadIdx.x;
    if (i >= nrows) return;
    const int32_t r = rows[i];
    double* p = P + i;
    double w = W[(int64_t)r * UPD_W];
    if (r == target) {
        for (int j = 0; j < b; ++j) {
            const double v = sh[j];
            p[(int64_t)j * ld] = v;
            w -= v * v;
        }
    } else {
#pragma unroll 4
        for (int j = 0; j < b; ++j) w -= p[(int64_t)j * ld] * sh[j];
    }
    W[(int64_t)r * UPD_W] = w;
}

// ONE workgroup.  d = W[jrow]: not positive (or NaN, or *info set on entry) sets *info and writes nothing.  Otherwise L_jj <-
// sqrt(d), every entry 1 + i behind it <- W[rows[i]] / sqrt(d), the same value stays in W, and W[jrow] <- 0 (every lane has read d
// before the barrier that precedes that store).
__global__ __launch_bounds__(RM_WG) void k_rowadd_column(double* __restrict__ col, int64_t nbelow, const int32_t* __restrict__ rows,
                                                         double* __restrict__ W, int64_t jrow, int* __restrict__ info) {
    const double d = W[jrow * UPD_W];
    const bool bad = *info != 0 || !(d > 0.0);
    __syncthreads();
    if (bad) {
        if (threadIdx.x == 0) *info = 1;
        return;
    }
    const double r = sqrt(d);
    if (threadIdx.x == 0) {
        col[0] = r;
        W[jrow * UPD_W] = 0.0;
    }
    for (int64_t i = threadIdx.x; i < nbelow; i += RM_WG) {
        const double v = W[(int64_t)rows[i] * UPD_W] / r;
        col[1 + i] = v;
        W[(int64_t)rows[i] * UPD_W] = v;
    }
}

}  // namespace

void launch_rowmod_zero_rows(double* L, const int64_t* tasks, int64_t ntasks, int64_t one_off, int check, int* flag, hipStream_t st) {
    if (ntasks <= 0) return;
    hipLaunchKernelGGL(k_rowmod_zero_rows, dim3((unsigned)ntasks), dim3(RM_WG), 0, st, L, tasks, one_off, check, flag);
}

void launch_rowdel_column(double* col, int64_t nbelow, const int32_t* rows, double* W, hipStream_t st) {
    const int64_t count = std::max<int64_t>(nbelow, 1);
    hipLaunchKernelGGL(k_rowdel_column, dim3((unsigned)((count + RM_WG - 1) / RM_WG)), dim3(RM_WG), 0, st, col, nbelow, rows, W);
}

void launch_rowadd_sweep_diag(const double* D, int64_t ld, int b, double* W, int64_t col0, double* y, hipStream_t st) {
    if (b <= 0 || b > UPD_B) return;
    hipLaunchKernelGGL(k_rowadd_sweep_diag, dim3(1), dim3(64), 0, st, D, ld, b, W + col0 * UPD_W, y);
}

void launch_rowadd_sweep_rows(double* P, int64_t ld, int b, int64_t nrows, const int32_t* rows, int32_t target, double* W, const double* y,
                              hipStream_t st) {
    if (b <= 0 || b > UPD_B || nrows <= 0) return;
    hipLaunchKernelGGL(k_rowadd_sweep_rows, dim3((unsigned)((nrows + RM_WG - 1) / RM_WG)), dim3(RM_WG), 0, st, P, ld, b, nrows, rows, target, W, y);
}

void launch_rowadd_column(double* col, int64_t nbelow, const int32_t* rows, double* W, int64_t jrow, int* info, hipStream_t st) {
    hipLaunchKernelGGL(k_rowadd_column, dim3(1), dim3(RM_WG), 0, st, col, nbelow, rows, W, jrow, info);
}

}  // namespace sf

// ---------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------
namespace {

// the path of one call (row, Ai in the caller's numbering with SF_DEV_PERM_IN); *bad as sf::rowmod_path leaves it
int path_of(const sf_chol_plan* p, sf_long row, sf_long nz, const sf_long* Ai, int flags, sf::RowmodPath& path, int64_t* bad) {
    std::vector<int32_t> iperm;
    if (flags & SF_DEV_PERM_IN) {
        if (p->dry || !p->d_perm) return SF_ERR_ARG;
        if (int rc = sf_updown_inverse_ordering(p, iperm)) return rc;
    }
    const int prc = sf::rowmod_path(sf_updown_struct(p), row, nz, Ai, iperm.empty() ? nullptr : iperm.data(), path, bad);
    return prc == sf::UPDOWN_OK ? SF_OK : SF_ERR_ARG;
}

// (offset from d_Lsx, stride, length) of every stretch of row j left of the diagonal; with_column: and of the column below it
std::vector<int64_t> row_tasks(const sf_chol_plan* p, const sf::RowmodPath& path, bool with_column) {
    std::vector<int64_t> t;
    for (size_t q = 0; q < path.rows_supers.size(); ++q) {
        const int64_t s = path.rows_supers[q];
        t.insert(t.end(), {p->h_Lsxp[s] + path.rows_pos[q], p->h_Lsip[s + 1] - p->h_Lsip[s], (int64_t)p->h_Super[s + 1] - p->h_Super[s]});
    }
    const int64_t nsrow = p->h_Lsip[path.s + 1] - p->h_Lsip[path.s];
    if (path.c > 0) t.insert(t.end(), {p->h_Lsxp[path.s] + path.c, nsrow, path.c});
    if (with_column && nsrow > path.c + 1) t.insert(t.end(), {p->h_Lsxp[path.s] + path.c * nsrow + path.c + 1, 1, nsrow - path.c - 1});
    return t;
}

struct Column {             // column j below the diagonal in the panel of s
    double* diag;
    int64_t nbelow;
    const int32_t* rows;
};
Column column_of(sf_chol_plan* p, const sf::RowmodPath& path) {
    const int64_t nsrow = p->h_Lsip[path.s + 1] - p->h_Lsip[path.s];
    return {p->d_Lsx + p->h_Lsxp[path.s] + path.c * nsrow + path.c, nsrow - path.c - 1, p->d_Lsi + p->h_Lsip[path.s] + path.c + 1};
}

void note(sf_chol_plan* p, const sf::RowmodPath& path, size_t ntasks, int64_t launches) {
    p->rowmod_row_tasks = (int64_t)ntasks;
    p->rowmod_sweep_supers = (int64_t)path.sweep.size();
    p->rowmod_launches = launches;
}

}  // namespace

extern "C" {

int sf_chol_plan_rowdel(sf_chol_plan* p, sf_long row, int flags) {
    if (int rc = sf_updown_accepts(p, flags)) return rc;
    p->rowmod_bad_index = -1;           // (of the last call that came this far: every such call starts them afresh)
    p->rowmod_not_deleted = 0;
    sf::RowmodPath path;
    if (int rc = path_of(p, row, 0, nullptr, flags, path, nullptr)) return rc;
    if (int rc = sf_updown_block(p)) return rc;
    hipStream_t st = p->stream;
    const SfUpdownBlock B = sf_updown_parts(p);
    const std::vector<int64_t> tasks = row_tasks(p, path, false);
    const size_t ntasks = tasks.size() / 3;
    sf::DevMem<int64_t> d_tasks;
    if (int rc = d_tasks.alloc(std::max<size_t>(tasks.size(), 1))) return rc;
    if (ntasks) HIP_TRY(hipMemcpyAsync(d_tasks, tasks.data(), tasks.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(B.info, 0, sizeof(double), st));

    int64_t launches = 0, rotations = 0;
    int h_info = 0;
    auto run = [&]() -> int {
        HIP_TRY(hipEventRecord(p->ev_s0, st));
        if (int rc = sf_updown_clear_w(p)) return rc;
        const Column col = column_of(p, path);
        sf::launch_rowmod_zero_rows(p->d_Lsx, d_tasks, (int64_t)ntasks, -1, 0, B.info, st);
        sf::launch_rowdel_column(col.diag, col.nbelow, col.rows, B.W, st);
        launches += ntasks ? 2 : 1;
        rotations = sf_updown_rotate(p, path.update, SF_UPDATE, 1);
        HIP_TRY(hipGetLastError());
        p->upd_w_dirty = false;
        return sf_updown_collect(p, &h_info);
    };
    const int rrc = run();
    note(p, path, ntasks, launches + rotations);
    return sf_updown_commit(p, rrc, h_info, path.update, rotations);        // ("update_launches": the rotations only)
}

int sf_chol_plan_rowadd(sf_chol_plan* p, sf_long row, sf_long nz, const sf_long* Ai, const sf_float* Ax, int flags) {
    if (int rc = sf_updown_accepts(p, flags)) return rc;
    p->rowmod_bad_index = -1;
    p->rowmod_not_deleted = 0;
    if (nz <= 0 || !Ai || !Ax) return SF_ERR_ARG;                   // (the diagonal at least)
    sf::RowmodPath path;
    int64_t bad = -1;
    const int prc = path_of(p, row, nz, Ai, flags, path, &bad);
    p->rowmod_bad_index = bad;                                      // (the stat that names it; nothing else of the plan changes)
    if (prc) return prc;
    if (std::find(path.mapped.begin(), path.mapped.end(), (int32_t)path.j) == path.mapped.end()) return SF_ERR_ARG;
    if (int rc = sf_updown_block(p)) return rc;
    hipStream_t st = p->stream;
    const SfUpdownBlock B = sf_updown_parts(p);
    const std::vector<int64_t> tasks = row_tasks(p, path, true);
    const size_t ntasks = tasks.size() / 3;
    const Column col = column_of(p, path);
    sf::DevMem<int64_t> d_tasks, d_dest;
    sf::DevMem<double> d_val;
    // one task at least in check mode: an empty one carries the test of L_jj
    std::vector<int64_t> up(tasks);
    if (up.empty()) up = {0, 1, 0};
    if (int rc = d_tasks.alloc(up.size())) return rc;
    if (int rc = d_dest.alloc((size_t)nz)) return rc;
    if (int rc = d_val.alloc((size_t)nz)) return rc;
    std::vector<int64_t> dest((size_t)nz);
    for (sf_long q = 0; q < nz; ++q) dest[(size_t)q] = (int64_t)path.mapped[(size_t)q] * sf::UPD_W;
    HIP_TRY(hipMemcpyAsync(d_tasks, up.data(), up.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_dest, dest.data(), dest.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_val, Ax, (size_t)nz * sizeof(double), hipMemcpyHostToDevice, st));
    // row and column j are the identity's: checked before anything is written
    HIP_TRY(hipMemsetAsync(B.info, 0, sizeof(double), st));
    sf::launch_rowmod_zero_rows(p->d_Lsx, d_tasks, (int64_t)(up.size() / 3), col.diag - (double*)p->d_Lsx, 1, B.info, st);
    int h_info = 0;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h_info, B.info, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    p->rowmod_not_deleted = h_info ? 1 : 0;
    if (h_info) return SF_ERR_ARG;

    int64_t launches = 1, rotations = 0;
    auto run = [&]() -> int {
        HIP_TRY(hipEventRecord(p->ev_s0, st));
        if (int rc = sf_updown_clear_w(p)) return rc;
        sf::launch_updown_scatter(d_dest, d_val, nz, B.W, st);
        ++launches;
        // the sweep: every supernode of the chains in full, then the columns of s before c
        auto sweep = [&](int64_t s, int64_t ncols) {
            const int64_t c0 = p->h_Super[s], nsrow = p->h_Lsip[s + 1] - p->h_Lsip[s];
            double* panel = p->d_Lsx + p->h_Lsxp[s];
            for (int64_t j0 = 0; j0 < ncols; j0 += sf::UPD_B) {
                const int b = (int)std::min<int64_t>(sf::UPD_B, ncols - j0);
                sf::launch_rowadd_sweep_diag(panel + j0 * nsrow + j0, nsrow, b, B.W, c0 + j0, B.rot, st);
                sf::launch_rowadd_sweep_rows(panel + j0 * nsrow + j0 + b, nsrow, b, nsrow - (j0 + b), p->d_Lsi + p->h_Lsip[s] + j0 + b,
                                             (int32_t)path.j, B.W, B.rot, st);
                launches += 2;              // (the row of j is below every block of the sweep)
            }
        };
        for (int64_t s : path.sweep) sweep(s, (int64_t)p->h_Super[s + 1] - p->h_Super[s]);
        sweep(path.s, path.c);
        sf::launch_rowadd_column(col.diag, col.nbelow, col.rows, B.W, path.j, B.info, st);
        ++launches;
        rotations = sf_updown_rotate(p, path.update, SF_DOWNDATE, 1);
        HIP_TRY(hipGetLastError());
        p->upd_w_dirty = false;
        return sf_updown_collect(p, &h_info);
    };
    const int rrc = run();
    note(p, path, ntasks, launches + rotations);
    return sf_updown_commit(p, rrc, h_info, path.update, rotations);        // ("update_launches": the rotations only)
}

int sf_chol_plan_rowmod_path(const sf_chol_plan* p, sf_long row, sf_long nz, const sf_long* Ai, int flags, sf_long* nrows,
                             sf_long* rows_supers, sf_long* rows_pos, sf_long* nsweep, sf_long* sweep, sf_long* nupdate, sf_long* update,
                             sf_long* bad) {
    if (nrows) *nrows = 0;
    if (nsweep) *nsweep = 0;
    if (nupdate) *nupdate = 0;
    if (bad) *bad = -1;
    if (!p || p->lu || nz < 0) return SF_ERR_ARG;
    if (flags & ~SF_DEV_PERM_IN) return SF_ERR_ARG;
    sf::RowmodPath path;
    int64_t b = -1;
    const int rc = path_of(p, row, nz, Ai, flags, path, &b);
    if (bad) *bad = b;
    if (rc) return rc;
    if (nrows) *nrows = (sf_long)path.rows_supers.size();
    if (nsweep) *nsweep = (sf_long)path.sweep.size();
    if (nupdate) *nupdate = (sf_long)path.update.size();
    if (rows_supers) std::copy(path.rows_supers.begin(), path.rows_supers.end(), rows_supers);
    if (rows_pos) std::copy(path.rows_pos.begin(), path.rows_pos.end(), rows_pos);
    if (sweep) std::copy(path.sweep.begin(), path.sweep.end(), sweep);
    if (update) std::copy(path.update.begin(), path.update.end(), update);
    return SF_OK;
}

}  // extern "C"
