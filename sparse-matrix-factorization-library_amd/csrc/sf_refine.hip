// Residual and iterative refinement with the resident factor (sf_chol_plan_residual, sf_chol_plan_refine and the LU entry
// points): r = b - A x from the plan's CURRENT matrix values, the componentwise backward error
//     berr = max_i |r_i| / (|A| |x| + |b|)_i          (Oettli-Prager; LAPACK xPORFS / xGERFS, SuperLU dgsrfs)
// next to the normwise number sf_chol_plan_validate reports, and the loop  x <- solve(b);  r = b - A x;  x += solve(r).
// Plain fp64 with FMA: by Skeel's result that is what componentwise backward stability needs.
//
//   row form        : the plan stores one triangle by column (and, unsymmetric LU, U by row).  Row i of A is a DIRECT run
//                     (symmetric: column i of the triangle; unsymmetric: row i of U) plus a TRANSPOSED run (the entries
//                     (i, j), j < i, of the columns j of the triangle / of L).  Built by the first call: row pointers, column
//                     indices and a POSITION into the plan's value arrays per entry -- values are always read from
//                     d_Lx / d_Ux as they are now, so a later set_values is honoured without rebuilding.  pos >= 0 indexes
//                     the direct array, ~pos the transposed one (symmetric: both are d_Lx and every pos is >= 0).  An entry
//                     that a later duplicate in its column supersedes is left out (the load maps say which: -1).
//   k_refine_resid  : RF_G lanes per row, striding over longer rows; r_i and w_i = (|A| |x| + |b|)_i in one pass, summed in a
//                     fixed order (lane-serial, then xor 4, 2, 1 inside the group): no floating-point atomics, the same x
//                     and b give the same bits on every call.  SUMS: only sum |a| per row of the form (the column sums of
//                     |A|_1 from the column form; symmetric: the row form serves).
//   k_refine_norms  : the maxima (integer atomicMax on the bit patterns of non-negative doubles) and a separate flag word
//                     for a non-finite r_i, x_i or b_i, which fmax would swallow.
//   k_refine_update : x += d; the iterate is first saved when it is the best seen so far.
#include <sparseframe_hip.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "sf_plan_internal.h"

namespace sf {

// RF_G = 8 lanes per row: the rows of the target matrices have 7 (7-point stencil) to 27 entries, so one or a few passes of 8
// keep 7/8 of the lanes busy, and the 8 rows of a wave are neighbours in the entry arrays -- a wave's loads of col / pos are one
// contiguous run.  A wave per row would idle 57 lanes of 64 on a 7-entry row, a lane per row would stride the entry arrays.
constexpr int RF_G = 8;
constexpr int RF_ROWS = 256 / RF_G;     // rows per workgroup

template <bool SUMS>
__global__ void __launch_bounds__(256)
k_refine_resid(int64_t n, const int64_t* __restrict__ ptr, const int32_t* __restrict__ col, const int64_t* __restrict__ pos,
               const double* __restrict__ Vd, const double* __restrict__ Vt, const double* __restrict__ x,
               const double* __restrict__ b, double* __restrict__ r, double* __restrict__ w, unsigned long long* __restrict__ amax) {
    const int g = threadIdx.x & (RF_G - 1);
    const int64_t row = (int64_t)blockIdx.x * RF_ROWS + (threadIdx.x / RF_G);
    const bool live = row < n;
    const int64_t e0 = live ? ptr[row] : 0, e1 = live ? ptr[row + 1] : 0;
    double acc = 0.0, mag = 0.0;
    for (int64_t e = e0 + g; e < e1; e += RF_G) {
        const int64_t ps = pos[e];
        const double a = ps >= 0 ? Vd[ps] : Vt[~ps];
        if (SUMS) {
            mag += fabs(a);
        } else {
            const double xv = x[col[e]];
            acc = fma(a, xv, acc);
            mag = fma(fabs(a), fabs(xv), mag);
        }
    }
#pragma unroll
    for (int m = RF_G / 2; m >= 1; m >>= 1) {
        if (!SUMS) acc += __shfl_xor(acc, m, RF_G);
        mag += __shfl_xor(mag, m, RF_G);
    }
    if (SUMS) {
        // max over the wave's rows (every lane of a group holds its row's sum; rows beyond n hold 0), one atomic per wave.
        // A NaN among the values fails every comparison of fmax's: it is caught by the flag of k_refine_norms through r.
        double v = mag;
#pragma unroll
        for (int off = 32; off >= RF_G; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
        if ((threadIdx.x & 63) == 0) atomicMax(amax, (unsigned long long)__double_as_longlong(v));
    } else if (live && g == 0) {
        const double bi = b[row];
        r[row] = bi - acc;
        w[row] = mag + fabs(bi);
    }
}

// s[0] = berr = max |r_i| / w_i over w_i > 0, s[1] = |r|_inf, s[2] = |x|_inf, s[3] = |b|_inf (bit patterns),
// s[4] = flags: bit 0 = some r_i, x_i or b_i is not finite, bit 1 = the info word of the solve before (a bounded wait ran out)
__global__ void __launch_bounds__(256)
k_refine_norms(int64_t n, const double* __restrict__ r, const double* __restrict__ w, const double* __restrict__ x,
               const double* __restrict__ b, const int* __restrict__ solve_info, unsigned long long* __restrict__ s) {
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double ri = fabs(r[i]), wi = w[i], xi = fabs(x[i]), bi = fabs(b[i]);
        // (x - x is 0 for a finite x and NaN for an infinity or a NaN)
        if ((ri - ri) != 0.0 || (xi - xi) != 0.0 || (bi - bi) != 0.0) bad = 1;
        if (wi > 0.0) m[0] = fmax(m[0], ri / wi);
        m[1] = fmax(m[1], ri); m[2] = fmax(m[2], xi); m[3] = fmax(m[3], bi);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = m[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
        if ((threadIdx.x & 63) == 0 && v > 0.0) atomicMax(s + k, (unsigned long long)__double_as_longlong(v));
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(s + 4, 1ull);
    if (blockIdx.x == 0 && threadIdx.x == 0 && solve_info && *solve_info) atomicOr(s + 4, 2ull);
}

__global__ void __launch_bounds__(256)
k_refine_update(int64_t n, double* __restrict__ x, const double* __restrict__ d, double* __restrict__ best, int save) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double xi = x[i];
    if (save) best[i] = xi;
    x[i] = xi + d[i];
}

void launch_refine_resid(const RefineForm& f, int64_t n, const double* x, const double* b, double* r, double* w, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_refine_resid<false>, dim3((unsigned)((n + RF_ROWS - 1) / RF_ROWS)), dim3(256), 0, st, n, f.ptr, f.col, f.pos, f.Vd, f.Vt,
                       x, b, r, w, (unsigned long long*)nullptr);
}

void launch_refine_abs_sums(const RefineForm& f, int64_t n, double* amax, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_refine_resid<true>, dim3((unsigned)((n + RF_ROWS - 1) / RF_ROWS)), dim3(256), 0, st, n, f.ptr, f.col, f.pos, f.Vd, f.Vt,
                       (const double*)nullptr, (const double*)nullptr, (double*)nullptr, (double*)nullptr, (unsigned long long*)amax);
}

void launch_refine_norms(int64_t n, const double* r, const double* w, const double* x, const double* b, const int* solve_info, double* s,
                         hipStream_t st) {
    if (n <= 0) return;
    const int64_t g = (n + 255) / 256;
    hipLaunchKernelGGL(k_refine_norms, dim3((unsigned)std::min<int64_t>(g, 1024)), dim3(256), 0, st, n, r, w, x, b, solve_info,
                       (unsigned long long*)s);
}

void launch_refine_update(int64_t n, double* x, const double* d, double* best, int save, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_refine_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, x, d, best, save);
}

}  // namespace sf

// ===========================================================================================================================
// host side
// ===========================================================================================================================
namespace {

constexpr int RF_SCALARS = 6;       // the five words of k_refine_norms + |A|_1 (kept while the values stay)

bool refine_refused(const sf_chol_plan* p) {
    return p->dry || p->partial || p->nranks > 1 || p->ooc_groups > 1 || !p->d_loadmapL || (p->lu && !p->d_loadmapU);
}

template <class T>
int fetch(std::vector<T>& h, const typename std::vector<T>::value_type* d, int64_t count) {
    h.resize((size_t)std::max<int64_t>(count, 0));
    if (count > 0) HIP_TRY(hipMemcpy(h.data(), d, (size_t)count * sizeof(T), hipMemcpyDeviceToHost));
    return SF_OK;
}

struct HostForm { std::vector<int64_t> ptr, pos; std::vector<int32_t> col; };

// Run i = the live entries of the direct structure's run i (index = Di[p], pos = p), then the live entries (i, j) of the
// transposed structure's runs j in ascending j and p (index = j, pos = ~p, or p when both runs read one array); i == j only
// with keep_diag (otherwise the direct run holds the diagonal).
// A counting sort: the order inside a run is fixed by the structure alone.
void build_form(int64_t n, const std::vector<int64_t>& Dp, const std::vector<int32_t>& Di, const std::vector<int64_t>& Dlive,
                const std::vector<int64_t>& Tp, const std::vector<int32_t>& Ti, const std::vector<int64_t>& Tlive, bool one_array,
                bool keep_diag, HostForm& f) {
    f.ptr.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = Dp[i]; p < Dp[i + 1]; ++p)
            if (Dlive[p] >= 0) ++f.ptr[i + 1];
    for (int64_t j = 0; j < n; ++j)
        for (int64_t p = Tp[j]; p < Tp[j + 1]; ++p)
            if (Tlive[p] >= 0 && (keep_diag || Ti[p] != j)) ++f.ptr[Ti[p] + 1];
    for (int64_t i = 0; i < n; ++i) f.ptr[i + 1] += f.ptr[i];
    const size_t total = (size_t)f.ptr[n];
    f.col.resize(std::max<size_t>(total, 1));
    f.pos.resize(std::max<size_t>(total, 1));
    std::vector<int64_t> cur(f.ptr.begin(), f.ptr.end() - 1);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = Dp[i]; p < Dp[i + 1]; ++p)
            if (Dlive[p] >= 0) { f.col[cur[i]] = Di[p]; f.pos[cur[i]++] = p; }
    for (int64_t j = 0; j < n; ++j)
        for (int64_t p = Tp[j]; p < Tp[j + 1]; ++p)
            if (Tlive[p] >= 0 && (keep_diag || Ti[p] != j)) { const int64_t i = Ti[p]; f.col[cur[i]] = (int32_t)j; f.pos[cur[i]++] = one_array ? p : ~p; }
}

template <class T>
bool put(T* d, const std::vector<T>& h, size_t count) {
    return count == 0 || hipMemcpy(d, h.data(), count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
}

// first call: the row form (unsymmetric LU: and the column form for |A|_1), the five vectors b | x | best x | r | w, the scalars
int refine_setup(sf_chol_plan* p) {
    if (p->d_rf_vec) return SF_OK;
    const int64_t n = p->n;
    const bool unsym = p->lu && !p->u_alias;
    std::vector<int64_t> Lp, Up, liveL, liveU;
    std::vector<int32_t> Li, Ui;
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (int rc = fetch(Lp, p->d_Lp, n + 1)) return rc;
    if (int rc = fetch(Li, p->d_Li, p->nnz)) return rc;
    // which entries count: the load map of the side that stores the diagonal (LU keeps it out of the L panel), -1 = superseded
    if (int rc = fetch(liveL, (p->lu && !unsym) ? p->d_loadmapU : p->d_loadmapL, p->nnz)) return rc;
    HostForm rows, cols;
    if (unsym) {
        if (int rc = fetch(Up, p->d_Up, n + 1)) return rc;
        if (int rc = fetch(Ui, p->d_Ui, p->unz)) return rc;
        if (int rc = fetch(liveU, p->d_loadmapU, p->unz)) return rc;
        // row i: U's row (with the diagonal), then L's entries of row i (its load map leaves the diagonal out: LU assembles U's);
        // column j, for |A|_1: L's column, then U's entries of column j with the diagonal
        build_form(n, Up, Ui, liveU, Lp, Li, liveL, false, false, rows);
        build_form(n, Lp, Li, liveL, Up, Ui, liveU, false, true, cols);
    } else {
        build_form(n, Lp, Li, liveL, Lp, Li, liveL, true, false, rows);
    }
    const size_t nr = (size_t)rows.ptr[n], nc = unsym ? (size_t)cols.ptr[n] : 0, nv = 5 * (size_t)std::max<int64_t>(n, 1) + RF_SCALARS;
    const size_t nr1 = std::max<size_t>(nr, 1), nc1 = std::max<size_t>(nc, 1);
    sf::DevMem<int64_t> rptr, rpos, cptr, cpos;
    sf::DevMem<int32_t> rcol, ccol;
    sf::DevMem<double> vec;
    size_t bytes = ((size_t)n + 1 + nr1) * sizeof(int64_t) + nr1 * sizeof(int32_t) + nv * sizeof(double);
    if (rptr.alloc((size_t)n + 1) || rcol.alloc(nr1) || rpos.alloc(nr1)) return SF_ERR_ALLOC;
    if (unsym) {
        if (cptr.alloc((size_t)n + 1) || ccol.alloc(nc1) || cpos.alloc(nc1)) return SF_ERR_ALLOC;
        bytes += ((size_t)n + 1 + nc1) * sizeof(int64_t) + nc1 * sizeof(int32_t);
    }
    if (vec.alloc(nv)) return SF_ERR_ALLOC;
    bool ok = put(rptr.get(), rows.ptr, (size_t)n + 1) && put(rcol.get(), rows.col, nr) && put(rpos.get(), rows.pos, nr);
    if (unsym) ok = ok && put(cptr.get(), cols.ptr, (size_t)n + 1) && put(ccol.get(), cols.col, nc) && put(cpos.get(), cols.pos, nc);
    if (!ok) { (void)hipGetLastError(); return SF_ERR_HIP; }
    p->d_rf_ptr = std::move(rptr); p->d_rf_col = std::move(rcol); p->d_rf_pos = std::move(rpos);
    p->d_rf_cptr = std::move(cptr); p->d_rf_ccol = std::move(ccol); p->d_rf_cpos = std::move(cpos);
    p->d_rf_vec = std::move(vec);
    p->rf_entries = (int64_t)nr;
    p->bytes_refine = bytes;
    p->fs.anorm_forgotten();
    return SF_OK;
}

struct RefineVecs { double *b, *x, *best, *r, *w, *s; };
RefineVecs refine_vecs(const sf_chol_plan* p) {
    const size_t n = (size_t)std::max<int64_t>(p->n, 1);
    double* v = p->d_rf_vec;
    return RefineVecs{v, v + n, v + 2 * n, v + 3 * n, v + 4 * n, v + 5 * n};
}

sf::RefineForm row_form(const sf_chol_plan* p) {
    const bool unsym = p->lu && !p->u_alias;
    return sf::RefineForm{p->d_rf_ptr, p->d_rf_col, p->d_rf_pos, unsym ? p->d_Ux : p->d_Lx, p->d_Lx};
}

// v.s[5] = |A|_1 of the current values: the column sums of |A| (unsymmetric LU: the column form; symmetric: the row form serves),
// recomputed when the values have changed
int refine_anorm(sf_chol_plan* p, const RefineVecs& v, hipStream_t st) {
    if (p->fs.anorm_current()) return SF_OK;
    const bool unsym = p->lu && !p->u_alias;
    HIP_TRY(hipMemsetAsync(v.s + 5, 0, sizeof(double), st));
    sf::launch_refine_abs_sums(unsym ? sf::RefineForm{p->d_rf_cptr, p->d_rf_ccol, p->d_rf_cpos, p->d_Lx, p->d_Ux} : row_form(p), p->n,
                               v.s + 5, st);
    p->fs.anorm_computed();
    return SF_OK;
}

// r = b - A x, w, and the scalars on the device (nothing waits here).  |A|_1 is recomputed when the values have changed.
int refine_eval(sf_chol_plan* p, const RefineVecs& v, const double* x, bool after_solve, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(v.s, 0, 5 * sizeof(double), st));
    if (int rc = refine_anorm(p, v, st)) return rc;
    sf::launch_refine_resid(row_form(p), p->n, x, v.b, v.r, v.w, st);
    sf::launch_refine_norms(p->n, v.r, v.w, x, v.b, after_solve ? p->d_solve_sync : nullptr, v.s, st);
    HIP_TRY(hipGetLastError());
    return SF_OK;
}

struct RefineScalars { double berr, nerr; bool solve_failed; };

// the one small copy and the one synchronisation of a step
int refine_read(sf_chol_plan* p, const RefineVecs& v, RefineScalars* out, hipStream_t st) {
    double h[RF_SCALARS];
    HIP_TRY(hipMemcpyAsync(h, v.s, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long flags;
    memcpy(&flags, &h[4], sizeof(flags));
    out->solve_failed = (flags & 2ull) != 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if ((flags & 1ull) || !std::isfinite(h[0]) || !std::isfinite(h[5])) {
        out->berr = out->nerr = nan;
    } else {
        out->berr = h[0];
        const double den = h[5] * h[2] + h[3];
        out->nerr = h[1] == 0.0 ? 0.0 : h[1] / den;
    }
    return SF_OK;
}

}  // namespace

int sf_refine_anorm(sf_chol_plan* p, const double** d_anorm, hipStream_t st) {
    if (refine_refused(p) || !p->fs.has_values()) return SF_ERR_ARG;
    if (int rc = refine_setup(p)) return rc;
    const RefineVecs v = refine_vecs(p);
    if (int rc = refine_anorm(p, v, st)) return rc;
    HIP_TRY(hipGetLastError());
    *d_anorm = v.s + 5;
    return SF_OK;
}

extern "C" {

int sf_chol_plan_residual(sf_chol_plan* p, const sf_float* b_host, const sf_float* x_host, sf_float* r_host, sf_float* berr, sf_float* nerr) {
    if (!p || !b_host || !x_host) return SF_ERR_ARG;
    if (refine_refused(p) || !p->fs.has_values()) return SF_ERR_ARG;
    if (berr) *berr = 0.0;
    if (nerr) *nerr = 0.0;
    if (p->n <= 0) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    if (int rc = refine_setup(p)) return rc;
    hipStream_t st = p->stream;
    const RefineVecs v = refine_vecs(p);
    const size_t nb = (size_t)p->n * sizeof(double);
    HIP_TRY(hipMemcpyAsync(v.b, b_host, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(v.x, x_host, nb, hipMemcpyHostToDevice, st));
    if (int rc = refine_anorm(p, v, st)) return rc;     // (here, so that the timed stretch below holds the residual pass alone)
    HIP_TRY(hipMemsetAsync(v.s, 0, 5 * sizeof(double), st));
    HIP_TRY(hipEventRecord(p->ev_s0, st));
    sf::launch_refine_resid(row_form(p), p->n, v.x, v.b, v.r, v.w, st);
    HIP_TRY(hipEventRecord(p->ev_s1, st));
    sf::launch_refine_norms(p->n, v.r, v.w, v.x, v.b, nullptr, v.s, st);
    HIP_TRY(hipGetLastError());
    if (r_host) HIP_TRY(hipMemcpyAsync(r_host, v.r, nb, hipMemcpyDeviceToHost, st));
    RefineScalars s;
    if (int rc = refine_read(p, v, &s, st)) return rc;
    float ms = 0;
    if (elapsed_ms(&ms, p->ev_s0, p->ev_s1)) p->last_residual_ms = ms;
    if (berr) *berr = s.berr;
    if (nerr) *nerr = s.nerr;
    return SF_OK;
}

int sf_chol_plan_residual_weights(sf_chol_plan* p, sf_float* w_host) {
    if (!p || !w_host || p->dry || !p->d_rf_vec) return SF_ERR_ARG;
    if (p->n <= 0) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(w_host, refine_vecs(p).w, (size_t)p->n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SF_OK;
}

int sf_chol_plan_refine(sf_chol_plan* p, const sf_float* b_host, sf_float* x_host, int max_iter, double tol, sf_float* berr_out) {
    if (!p || !b_host || !x_host || max_iter < 0) return SF_ERR_ARG;
    if (refine_refused(p) || !p->fs.has_values() || (p->nsuper > 0 && !p->d_solve)) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!sf_factor_usable(p)) return SF_ERR_ARG;
    if (berr_out) *berr_out = 0.0;
    p->last_refine_iters = 0;
    p->last_refine_berr0 = p->last_refine_berr = 0.0;
    p->last_refine_ms = 0.0;
    if (p->n <= 0) return SF_OK;
    if (int rc = refine_setup(p)) return rc;
    if (!(tol > 0.0)) tol = 0x1p-52;
    hipStream_t st = p->stream;
    const RefineVecs v = refine_vecs(p);
    const size_t nb = (size_t)p->n * sizeof(double);
    hipEvent_t e0 = p->ev_s0, e1 = p->ev_s1;
    double total_ms = 0.0;
    RefineScalars s;
    // one stretch of device work, then the scalars: the one copy and the one synchronisation of the step
    auto finish_step = [&]() -> int {
        HIP_TRY(hipEventRecord(e1, st));
        if (int rc = refine_read(p, v, &s, st)) return rc;
        float ms = 0;
        if (elapsed_ms(&ms, e0, e1)) total_ms += ms;
        return s.solve_failed ? SF_ERR_HIP : SF_OK;
    };

    HIP_TRY(hipMemcpyAsync(v.b, b_host, nb, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(e0, st));
    HIP_TRY(hipMemcpyAsync(v.x, v.b, nb, hipMemcpyDeviceToDevice, st));
    if (int rc = sf_apply_sweep(p, SF_SWEEP_SOLVE, v.x, 1, true)) return rc;
    if (int rc = refine_eval(p, v, v.x, true, st)) return rc;
    if (int rc = finish_step()) return rc;

    const double berr0 = s.berr;
    double cur = berr0, prev = berr0, best = berr0;
    bool best_in_x = true;      // the best iterate so far is the current one; otherwise v.best holds it
    int k = 0;
    while (std::isfinite(cur) && cur > tol && k < max_iter && !(k >= 1 && cur > 0.5 * prev)) {
        HIP_TRY(hipEventRecord(e0, st));
        if (int rc = sf_apply_sweep(p, SF_SWEEP_SOLVE, v.r, 1, false)) return rc;      // d = solve(r), in place (the factor has not changed: no new transposes)
        sf::launch_refine_update(p->n, v.x, v.r, v.best, best_in_x ? 1 : 0, st);
        if (int rc = refine_eval(p, v, v.x, true, st)) return rc;
        if (int rc = finish_step()) return rc;
        ++k;
        prev = cur;
        cur = s.berr;
        best_in_x = std::isfinite(cur) && cur < best;
        if (best_in_x) best = cur;
    }
    HIP_TRY(hipMemcpyAsync(x_host, best_in_x ? v.x : v.best, nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    p->last_refine_iters = k;
    p->last_refine_berr0 = berr0;
    p->last_refine_berr = best;
    p->last_refine_ms = total_ms;
    if (berr_out) *berr_out = best;
    return SF_OK;
}

int sf_lu_plan_residual(sf_lu_plan* p, const sf_float* b_host, const sf_float* x_host, sf_float* r_host, sf_float* berr, sf_float* nerr) {
    return (p && p->lu) ? sf_chol_plan_residual(p, b_host, x_host, r_host, berr, nerr) : SF_ERR_ARG;
}
int sf_lu_plan_refine(sf_lu_plan* p, const sf_float* b_host, sf_float* x_host, int max_iter, double tol, sf_float* berr) {
    return (p && p->lu) ? sf_chol_plan_refine(p, b_host, x_host, max_iter, tol, berr) : SF_ERR_ARG;
}

}  // extern "C"
