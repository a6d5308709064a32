// Sigma = A^-1 read where the caller wants it: on the pattern the plan was created with, as tr(Sigma M(V)) for value
// arrays V in set_values order, and at arbitrary (row, column) pairs inside the factor's pattern.  Cholesky and LU plans.
//
// Nothing here computes Sigma: sf_*_plan_selinv has filled the arena(s), which have the device factor's layout -- so the load maps
// of plan creation (d_loadmapL / d_loadmapU: for every entry of the plan's structure its offset in the factor) address Sigma too.
// The kernels are gathers and fixed-order reductions; no sweep, schedule, sync word or floating-point atomic.
//
//   k_selpat_build  : the walk of k_build_loadmap (sf_kernels.hip) with no entry left out: the position of EVERY entry of the
//                     structure -- superseded duplicates and the L diagonal of an LU plan included -- and, for Cholesky plans, which
//                     entries are off the diagonal (they count twice in the trace)
//   k_selpat_gather : out[p] = S[pos[p]], grid-stride, coalesced on the map and the output (as k_load_mapped)
//   k_selpat_part   : one workgroup per SELPAT_TILE consecutive entries: every map entry and every Sigma value read once, multiplied
//                     against SELPAT_CHUNK columns of V at a time in registers, reduced in a fixed tree, one part per column
//   k_selpat_final  : one workgroup per column sums its parts in index order
//   k_selpat_entries: Sigma(i, j) by the binary search of the walk (the column's supernode, then its row list); a quiet NaN outside
//
// The orientation of an LU plan's pair of arenas (sf_selinv_lu.hip): SL(r, c) = Sigma(row of r, c), SU(r, c) = Sigma(c, row of r),
// SU xC doubles after SL.  An entry (i, j) of L (by column, i >= j) sits at the same panel position in both, so
//   Sigma(i, j) = SL[pos],  Sigma(j, i) = SU[pos];
// an entry (j, c) of U (by row, c >= j) sits at position pos' of column j of the U^T panels, so
//   Sigma(j, c) = SU[pos'],  Sigma(c, j) = SL[pos'].
// tr(Sigma M) = sum_ij Sigma(j, i) M_ij therefore pairs the L entries with SU and the U entries with SL.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "sf_plan_internal.h"

namespace sf {

// (the SELPAT_* constants: sf_kernels.h)

// position of the first element >= key in the ascending array a[0..n)
__device__ __forceinline__ int selpat_lower_bound(const int32_t* __restrict__ a, int n, int32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one lane per column j of the structure (Lp, Li) (LU: also per row j of U through (Up, Ui)): pos[p] = the offset of entry p in
// one panel set, offd[p] = 1 when its row differs from j (offd may be null).  plan_create has checked every index against the row
// lists, so the search finds its key.
__global__ void __launch_bounds__(256)
k_selpat_build(const int64_t* __restrict__ Lp, const int32_t* __restrict__ Li, int32_t n, const int32_t* __restrict__ Super,
               const int32_t* __restrict__ SuperMap, const int64_t* __restrict__ Lsip, const int32_t* __restrict__ Lsi,
               const int64_t* __restrict__ Xp, int64_t* __restrict__ pos, uint8_t* __restrict__ offd) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int32_t s = SuperMap[j];
    const int32_t c0 = Super[s], c1 = Super[s + 1];
    const int64_t r0 = Lsip[s];
    const int32_t nsrow = (int32_t)(Lsip[s + 1] - r0);
    const int32_t nscol = c1 - c0;
    const int64_t col = Xp[s] + (int64_t)(j - c0) * nsrow;
    const int32_t* below = Lsi + r0 + nscol;
    for (int64_t p = Lp[j]; p < Lp[j + 1]; ++p) {
        const int32_t i = Li[p];
        const int32_t si = (i < c1) ? (i - c0) : nscol + selpat_lower_bound(below, nsrow - nscol, i);
        pos[p] = col + si;
        if (offd) offd[p] = i != j;
    }
}

__global__ void __launch_bounds__(256)
k_selpat_gather(const int64_t* __restrict__ pos, int64_t count, const double* __restrict__ S, double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
#pragma unroll 4
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < count; p += stride) out[p] = S[pos[p]];
}

// part[t * nparts + part0 + blockIdx.x] = sum over the workgroup's entries p of w_p S[map[p] + shift] V_t[p], t < m.
// map: a live load map (-1: the entry is not part of the assembled matrix and is skipped, its V never read); offd: null or the
// off-diagonal marks (w_p = 2 there, 1 otherwise); MAPPED: V_t[p] = vmap[p] >= 0 ? V[vmap[p] + t ldv] : 0, otherwise V[p + t ldv].
// A lane takes the entries tile + tid + 256 e: all its map entries are loaded first, then all its Sigma values (SELPAT_EPT
// independent gathers), then per chunk of columns the V values.  Sum order of one column: the lane's entries by e, the wave's
// lanes by a shuffle tree, the four waves in order -- the same whatever m is, so a column's bits depend on that column alone.
template <bool MAPPED>
__global__ void __launch_bounds__(256)
k_selpat_part(const int64_t* __restrict__ map, const uint8_t* __restrict__ offd, int64_t count, const double* __restrict__ S,
              int64_t shift, const double* __restrict__ V, int64_t ldv, const int64_t* __restrict__ vmap, int m,
              double* __restrict__ part, int64_t part0, int64_t nparts) {
    __shared__ double red[4][SELPAT_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * SELPAT_TILE + tid;
    int64_t q[SELPAT_EPT];
    double s[SELPAT_EPT];
#pragma unroll
    for (int e = 0; e < SELPAT_EPT; ++e) {
        const int64_t p = p0 + 256 * e;
        q[e] = p < count ? map[p] : -1;
    }
#pragma unroll
    for (int e = 0; e < SELPAT_EPT; ++e) {
        const int64_t p = p0 + 256 * e;
        const bool live = q[e] >= 0;
        double v = live ? S[q[e] + shift] : 0.0;
        if (live && offd && offd[p]) v *= 2.0;
        s[e] = v;
        q[e] = live ? (MAPPED ? vmap[p] : p) : -1;      // from here on: where the entry's V values start, -1: they count as 0
    }
    for (int c0 = 0; c0 < m; c0 += SELPAT_CHUNK) {
        double acc[SELPAT_CHUNK];
#pragma unroll
        for (int c = 0; c < SELPAT_CHUNK; ++c) acc[c] = 0.0;
#pragma unroll
        for (int e = 0; e < SELPAT_EPT; ++e) {
            if (q[e] < 0) continue;
            const double* __restrict__ v = V + q[e] + (int64_t)c0 * ldv;
#pragma unroll
            for (int c = 0; c < SELPAT_CHUNK; ++c)
                if (c0 + c < m) acc[c] = __builtin_fma(s[e], v[(int64_t)c * ldv], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < SELPAT_CHUNK; ++c) {
            double v = acc[c];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) red[wave][c] = v;
        }
        __syncthreads();
        if (tid < SELPAT_CHUNK && c0 + tid < m)
            part[(int64_t)(c0 + tid) * nparts + part0 + blockIdx.x] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        __syncthreads();
    }
}

// out[t] = sum part[t * nparts .. + nparts): lane k sums the parts k, k + 256, ... in order, then a tree in LDS
__global__ void __launch_bounds__(256)
k_selpat_final(const double* __restrict__ part, int64_t nparts, double* __restrict__ out) {
    __shared__ double red[256];
    const double* __restrict__ col = part + (int64_t)blockIdx.x * nparts;
    double v = 0.0;
    for (int64_t k = threadIdx.x; k < nparts; k += 256) v += col[k];
    red[threadIdx.x] = v;
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// out[k] = Sigma(rows[k], cols[k]).  lu == 0: either triangle (the arena holds the lower one and the mirror inside the diagonal
// blocks); lu != 0: (i, j) literally, i >= j from SL, i < j from SU = S + xC.  Outside the pattern: a quiet NaN, counted.
__global__ void __launch_bounds__(256)
k_selpat_entries(const int64_t* __restrict__ rows, const int64_t* __restrict__ cols, int64_t count, int lu, int64_t xC,
                 const double* __restrict__ S, const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap,
                 const int64_t* __restrict__ Lsip, const int32_t* __restrict__ Lsi, const int64_t* __restrict__ Xp,
                 double* __restrict__ out, unsigned long long* __restrict__ outside) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const int32_t i = (int32_t)rows[k], j = (int32_t)cols[k];
    const int32_t col = min(i, j), row = max(i, j);
    const int32_t s = SuperMap[col];
    const int32_t c0 = Super[s], c1 = Super[s + 1];
    const int64_t r0 = Lsip[s];
    const int32_t nsrow = (int32_t)(Lsip[s + 1] - r0);
    const int32_t nscol = c1 - c0, nb = nsrow - nscol;
    int32_t si = row - c0;
    bool found = true;
    if (row >= c1) {
        const int32_t* below = Lsi + r0 + nscol;
        const int b = selpat_lower_bound(below, nb, row);
        found = b < nb && below[b] == row;
        si = nscol + b;
    }
    if (!found) {
        out[k] = __builtin_nan("");
        atomicAdd(outside, 1ull);
        return;
    }
    const int64_t off = Xp[s] + (int64_t)(col - c0) * nsrow + si;
    out[k] = S[off + ((lu && i < j) ? xC : 0)];
}

// ---- the launchers (sf_kernels.h): one launch each; the host side below and the per-launch tests run these and nothing else ----
void launch_selpat_build(const int64_t* Lp, const int32_t* Li, int32_t n, const int32_t* Super, const int32_t* SuperMap, const int64_t* Lsip,
                         const int32_t* Lsi, const int64_t* Xp, int64_t* pos, uint8_t* offd, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_selpat_build, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, st, Lp, Li, n, Super, SuperMap, Lsip, Lsi, Xp,
                       pos, offd);
}

void launch_selpat_gather(const int64_t* pos, int64_t count, const double* S, double* out, hipStream_t st) {
    if (count <= 0) return;
    const int64_t blocks = std::min<int64_t>((count + 255) / 256, SELPAT_GATHER_GRID);
    hipLaunchKernelGGL(k_selpat_gather, dim3((unsigned)blocks), dim3(256), 0, st, pos, count, S, out);
}

int64_t launch_selpat_part(bool mapped, const int64_t* map, const uint8_t* offd, int64_t count, const double* S, int64_t shift, const double* V,
                           int64_t ldv, const int64_t* vmap, int m, double* part, int64_t part0, int64_t nparts, hipStream_t st) {
    if (count <= 0) return 0;
    const int64_t nt = (count + SELPAT_TILE - 1) / SELPAT_TILE;
    if (mapped)
        hipLaunchKernelGGL(k_selpat_part<true>, dim3((unsigned)nt), dim3(256), 0, st, map, offd, count, S, shift, V, ldv, vmap, m, part, part0,
                           nparts);
    else
        hipLaunchKernelGGL(k_selpat_part<false>, dim3((unsigned)nt), dim3(256), 0, st, map, offd, count, S, shift, V, ldv, vmap, m, part, part0,
                           nparts);
    return nt;
}

void launch_selpat_final(const double* part, int64_t nparts, int m, double* out, hipStream_t st) {
    if (m <= 0) return;
    hipLaunchKernelGGL(k_selpat_final, dim3((unsigned)m), dim3(256), 0, st, part, nparts, out);
}

void launch_selpat_entries(const int64_t* rows, const int64_t* cols, int64_t count, int lu, int64_t xC, const double* S, const SelStruct& t,
                           double* out, unsigned long long* outside, hipStream_t st) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_selpat_entries, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, rows, cols, count, lu, xC, S, t.Super, t.SuperMap,
                       t.Lsip, t.Lsi, t.Xp, out, outside);
}

}  // namespace sf

// ===========================================================================================================================
// host side
// ===========================================================================================================================
namespace {

// the plans every entry point here accepts: of the right kind, whole and resident, with an arena that belongs to the resident factor
bool selpat_ready(const sf_chol_plan* p, bool lu) {
    if (!p || p->lu != lu || !sf_plan_whole_resident(p)) return false;
    if (!p->d_sel || !p->fs.selinv_matches()) return false;
    return p->d_loadmapL && (!lu || p->d_loadmapU);
}

int64_t u_count(const sf_chol_plan* p) { return !p->lu ? 0 : p->u_alias ? p->nnz : p->unz; }
int64_t tiles(int64_t count) { return (count + sf::SELPAT_TILE - 1) / sf::SELPAT_TILE; }

// the positions of every entry (first call that needs them): posL, then for an LU plan with its own U structure posU
int selpat_positions(sf_chol_plan* p) {
    if (p->d_sp_pos) return SF_OK;
    const bool own_u = p->lu && !p->u_alias;
    const size_t nl = (size_t)std::max<int64_t>(p->nnz, 1), nu = own_u ? (size_t)std::max<int64_t>(p->unz, 1) : 0;
    const size_t b_pos = (nl + nu) * sizeof(int64_t), b_off = p->lu ? 0 : nl;
    sf::DevMem<int64_t> pos;
    sf::DevMem<uint8_t> offd;
    if (int rc = pos.alloc(nl + nu)) return rc;
    if (b_off)
        if (int rc = offd.alloc(b_off)) return rc;
    const int64_t* xp = p->lu ? p->d_Xp : p->d_Lsxp;
    sf::launch_selpat_build(p->d_Lp, p->d_Li, (int32_t)p->n, p->d_Super, p->d_SuperMap, p->d_Lsip, p->d_Lsi, xp, pos, offd, p->stream);
    if (own_u)
        sf::launch_selpat_build(p->d_Up, p->d_Ui, (int32_t)p->n, p->d_Super, p->d_SuperMap, p->d_Lsip, p->d_Lsi, xp, pos + nl, nullptr, p->stream);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess) return SF_ERR_HIP;
    p->d_sp_pos = std::move(pos);
    p->d_sp_offd = std::move(offd);
    p->bytes_selinv_pattern += b_pos + b_off;
    return SF_OK;
}

// the parts of one trace call and its SELPAT_MAX_M results
int selpat_parts(sf_chol_plan* p) {
    if (p->d_sp_part) return SF_OK;
    const size_t np = (size_t)std::max<int64_t>(tiles(p->nnz) + tiles(u_count(p)), 1);
    if (int rc = p->d_sp_part.alloc((np + 1) * sf::SELPAT_MAX_M)) return rc;
    p->bytes_selinv_pattern += (np + 1) * sf::SELPAT_MAX_M * sizeof(double);
    return SF_OK;
}

// rows | cols | values of one chunk of pairs, then the count of pairs outside the pattern
int selpat_stage(sf_chol_plan* p) {
    if (p->d_sp_stage) return SF_OK;
    const size_t bytes = (size_t)sf::SELPAT_ENT_CHUNK * 3 * 8 + 8;
    if (int rc = p->d_sp_stage.alloc(bytes)) return rc;
    p->bytes_selinv_pattern += bytes;
    return SF_OK;
}

void gather(sf_chol_plan* p, const int64_t* pos, int64_t count, const double* S, double* out) {
    sf::launch_selpat_gather(pos, count, S, out, p->stream);
}

// Sigma on the structure into device memory: dL (nnz), dU (unz; LU plans with their own U structure).  transposed: Sigma(j, i) where
// the plain call gives Sigma(i, j) -- the other arena at the same position.
int values_run(sf_chol_plan* p, bool transposed, double* dL, double* dU) {
    if (int rc = selpat_positions(p)) return rc;
    const size_t nl = (size_t)std::max<int64_t>(p->nnz, 1);
    const double* SL = p->d_sel;
    const double* SU = p->lu ? p->d_sel + p->xC : p->d_sel;
    SfStretch t{p};
    if (int rc = t.open()) return rc;
    gather(p, p->d_sp_pos, p->nnz, transposed ? SU : SL, dL);
    if (dU) gather(p, p->d_sp_pos + nl, p->unz, transposed ? SL : SU, dU);
    if (int rc = t.mark()) return rc;
    if (int rc = t.close(false)) return rc;
    p->last_selinv_pattern_ms = t.total_ms;
    return SF_OK;
}

// host arrays: through temporary device buffers
int values_host(sf_chol_plan* p, bool transposed, double* outL, double* outU) {
    const int64_t nl = p->nnz, nu = outU ? p->unz : 0;
    if (nl + nu <= 0) return SF_OK;
    sf::DevMem<double> tmp;
    if (int rc = tmp.alloc((size_t)(nl + nu))) return rc;
    if (int rc = values_run(p, transposed, tmp, nu > 0 ? tmp + nl : nullptr)) return rc;
    if (nl > 0 && hipMemcpy(outL, tmp, (size_t)nl * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return SF_ERR_HIP;
    if (nu > 0 && hipMemcpy(outU, tmp + nl, (size_t)nu * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return SF_ERR_HIP;
    return SF_OK;
}

int values_entry(sf_chol_plan* p, bool lu, bool dev, bool transposed, double* outL, double* outU) {
    if (!p || p->lu != lu) return SF_ERR_ARG;
    const bool own_u = lu && !p->u_alias;
    if ((!outL && p->nnz > 0) || (own_u && !outU && p->unz > 0) || (!own_u && outU)) return SF_ERR_ARG;
    if (!selpat_ready(p, lu)) return SF_ERR_ARG;
    HIP_TRY(hipSetDevice(p->device));
    if (!dev) return values_host(p, transposed, outL, own_u ? outU : nullptr);
    if (p->nnz > 0 && !sf_device_ptr_ok(p, outL, (size_t)p->nnz)) return SF_ERR_ARG;
    if (own_u && p->unz > 0 && !sf_device_ptr_ok(p, outU, (size_t)p->unz)) return SF_ERR_ARG;
    return values_run(p, transposed, outL, (own_u && p->unz > 0) ? outU : nullptr);
}

struct TraceSide { const int64_t* map; const uint8_t* offd; int64_t count, shift; const double* V; int64_t ldv; const int64_t* vmap; };

// the kernels of one trace call: parts of every side, then the sums into d_res (device)
void trace_launch(sf_chol_plan* p, const TraceSide* side, int nside, bool mapped, int m, double* d_res) {
    int64_t nparts = 0;
    for (int k = 0; k < nside; ++k) nparts += tiles(side[k].count);
    int64_t part0 = 0;
    for (int k = 0; k < nside; ++k) {
        const TraceSide& s = side[k];
        part0 += sf::launch_selpat_part(mapped, s.map, s.offd, s.count, p->d_sel, s.shift, s.V, s.ldv, s.vmap, m, p->d_sp_part, part0, nparts,
                                        p->stream);
    }
    sf::launch_selpat_final(p->d_sp_part, nparts, m, d_res, p->stream);
}

// VL / VU: device memory.  d_out: device memory of the caller's, or null -- the results then go to `out` on the host.
int trace_run(sf_chol_plan* p, bool mapped, int m, const double* VL, int64_t ldvl, const double* VU, int64_t ldvu, double* d_out, double* out) {
    if (!p->lu)
        if (int rc = selpat_positions(p)) return rc;        // (the off-diagonal marks)
    if (int rc = selpat_parts(p)) return rc;
    const size_t nl = (size_t)std::max<int64_t>(p->nnz, 1);
    const size_t np = (size_t)std::max<int64_t>(tiles(p->nnz) + tiles(u_count(p)), 1);
    double* d_res = d_out ? d_out : p->d_sp_part + np * sf::SELPAT_MAX_M;
    TraceSide side[2];
    int nside = 1;
    if (!p->lu) {
        side[0] = TraceSide{p->d_loadmapL, p->d_sp_offd, p->nnz, 0, VL, ldvl, p->d_vmap};
    } else {
        // an entry of L meets Sigma(j, i) in SU at its own offset; an entry of U (its load map carries the xC of the U^T panels)
        // meets Sigma(c, j) in SL.  U aliasing L: the U side walks the L structure again, the values are VL's.
        const bool own_u = !p->u_alias;
        side[0] = TraceSide{p->d_loadmapL, nullptr, p->nnz, p->xC, VL, ldvl, p->d_vmap};
        side[1] = TraceSide{p->d_loadmapU, nullptr, u_count(p), -p->xC, (own_u && !mapped) ? VU : VL, (own_u && !mapped) ? ldvu : ldvl,
                            (own_u && p->d_vmap) ? p->d_vmap + nl : p->d_vmap};
        nside = 2;
    }
    SfStretch t{p};
    if (int rc = t.open()) return rc;
    trace_launch(p, side, nside, mapped, m, d_res);
    if (int rc = t.mark()) return rc;
    if (!d_out) HIP_TRY(hipMemcpyAsync(out, d_res, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (int rc = t.close(false)) return rc;
    p->last_selinv_pattern_ms = t.total_ms;
    return SF_OK;
}

// a host block of m columns of `rows` doubles, ld apart, into fresh device memory (leading dimension rows)
int upload_block(const double* V, int64_t rows, int64_t ld, int m, sf::DevMem<double>& d) {
    if (int rc = d.alloc((size_t)std::max<int64_t>(rows * m, 1))) return rc;
    if (rows <= 0) return SF_OK;
    const size_t col = (size_t)rows * sizeof(double);
    if (hipMemcpy2D(d, col, V, (size_t)ld * sizeof(double), col, m, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        d.reset();
        return SF_ERR_HIP;
    }
    return SF_OK;
}

int trace_entry(sf_chol_plan* p, bool lu, bool dev, sf_long m, const double* VL, sf_long ldvl, const double* VU, sf_long ldvu, int flags,
                double* out) {
    if (!p || p->lu != lu || !out || m < 0 || m > sf::SELPAT_MAX_M) return SF_ERR_ARG;
    if (flags & ~SF_SEL_MAPPED) return SF_ERR_ARG;
    const bool mapped = (flags & SF_SEL_MAPPED) != 0;
    const bool own_u = lu && !p->u_alias;
    const bool need_u = own_u && !mapped;           // (a mapped call reads both triangles from the one array)
    const int64_t rows_l = mapped ? p->vmap_nsrc : p->nnz, rows_u = need_u ? p->unz : 0;
    if ((!VL && rows_l > 0) || (need_u && !VU && rows_u > 0) || (!need_u && VU)) return SF_ERR_ARG;
    if (ldvl < std::max<int64_t>(rows_l, 1) || (need_u && ldvu < std::max<int64_t>(rows_u, 1))) return SF_ERR_ARG;
    if (!selpat_ready(p, lu) || (mapped && !p->d_vmap)) return SF_ERR_ARG;
    if (m == 0) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    const int mi = (int)m;
    if (dev) {
        const size_t sl = sf_block_span(rows_l, m, ldvl), su = sf_block_span(rows_u, m, ldvu);
        if ((sl && !sf_device_ptr_ok(p, VL, sl)) || (su && !sf_device_ptr_ok(p, VU, su)) || !sf_device_ptr_ok(p, out, (size_t)m)) return SF_ERR_ARG;
        return trace_run(p, mapped, mi, VL, ldvl, need_u ? VU : nullptr, ldvu, out, nullptr);
    }
    sf::DevMem<double> dL, dU;
    if (int rc = upload_block(VL, rows_l, ldvl, mi, dL)) return rc;
    if (need_u)
        if (int rc = upload_block(VU, rows_u, ldvu, mi, dU)) return rc;
    double res[sf::SELPAT_MAX_M];
    if (int rc = trace_run(p, mapped, mi, dL, std::max<int64_t>(rows_l, 1), dU, std::max<int64_t>(rows_u, 1), nullptr, res)) return rc;
    std::copy(res, res + mi, out);
    return SF_OK;
}

int entries_entry(sf_chol_plan* p, bool lu, sf_long count, const sf_long* rows, const sf_long* cols, double* out, sf_long* outside) {
    if (!p || p->lu != lu || count < 0 || (count > 0 && (!rows || !cols || !out))) return SF_ERR_ARG;
    if (!selpat_ready(p, lu)) return SF_ERR_ARG;
    for (sf_long k = 0; k < count; ++k)
        if (rows[k] < 0 || rows[k] >= p->n || cols[k] < 0 || cols[k] >= p->n) return SF_ERR_ARG;
    p->last_selinv_outside = 0;
    if (outside) *outside = 0;
    if (count == 0) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    if (int rc = selpat_stage(p)) return rc;
    const int64_t CH = sf::SELPAT_ENT_CHUNK;
    int64_t* d_rows = (int64_t*)p->d_sp_stage.get();
    int64_t* d_cols = d_rows + CH;
    double* d_val = (double*)(d_cols + CH);
    unsigned long long* d_cnt = (unsigned long long*)(d_val + CH);
    hipStream_t st = p->stream;
    const sf::SelStruct tab{p->d_Super, p->d_SuperMap, p->d_Lsip, p->d_Lsi, lu ? p->d_Xp : p->d_Lsxp, nullptr, nullptr};
    HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), st));
    SfStretch t{p};
    for (int64_t k0 = 0; k0 < count; k0 += CH) {
        const int64_t c = std::min<int64_t>(CH, count - k0);
        HIP_TRY(hipMemcpyAsync(d_rows, rows + k0, (size_t)c * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_cols, cols + k0, (size_t)c * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (int rc = t.open()) return rc;
        sf::launch_selpat_entries(d_rows, d_cols, c, lu ? 1 : 0, p->xC, p->d_sel, tab, d_val, d_cnt, st);
        if (int rc = t.mark()) return rc;
        HIP_TRY(hipMemcpyAsync(out + k0, d_val, (size_t)c * sizeof(double), hipMemcpyDeviceToHost, st));
        if (int rc = t.close(false)) return rc;     // (the pageable copies above are done before the next chunk overwrites the stage)
    }
    unsigned long long cnt = 0;
    HIP_TRY(hipMemcpy(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
    p->last_selinv_outside = (int64_t)cnt;
    p->last_selinv_pattern_ms = t.total_ms;
    if (outside) *outside = (sf_long)cnt;
    return SF_OK;
}

}  // namespace

extern "C" {

int sf_chol_plan_selinv_values(sf_chol_plan* p, sf_float* out) { return values_entry(p, false, false, false, out, nullptr); }
int sf_chol_plan_selinv_values_device(sf_chol_plan* p, sf_float* d_out) { return values_entry(p, false, true, false, d_out, nullptr); }
int sf_lu_plan_selinv_values(sf_lu_plan* p, sf_float* outL, sf_float* outU) { return values_entry(p, true, false, false, outL, outU); }
int sf_lu_plan_selinv_values_device(sf_lu_plan* p, sf_float* d_outL, sf_float* d_outU) { return values_entry(p, true, true, false, d_outL, d_outU); }
int sf_lu_plan_selinv_values_t(sf_lu_plan* p, sf_float* outL, sf_float* outU) { return values_entry(p, true, false, true, outL, outU); }
int sf_lu_plan_selinv_values_t_device(sf_lu_plan* p, sf_float* d_outL, sf_float* d_outU) { return values_entry(p, true, true, true, d_outL, d_outU); }

int sf_chol_plan_selinv_trace(sf_chol_plan* p, sf_long m, const sf_float* V, sf_long ldv, int flags, sf_float* out) {
    return trace_entry(p, false, false, m, V, ldv, nullptr, 0, flags, out);
}
int sf_chol_plan_selinv_trace_device(sf_chol_plan* p, sf_long m, const sf_float* dV, sf_long ldv, int flags, sf_float* d_out) {
    return trace_entry(p, false, true, m, dV, ldv, nullptr, 0, flags, d_out);
}
int sf_lu_plan_selinv_trace(sf_lu_plan* p, sf_long m, const sf_float* VL, sf_long ldvl, const sf_float* VU, sf_long ldvu, int flags, sf_float* out) {
    return trace_entry(p, true, false, m, VL, ldvl, VU, ldvu, flags, out);
}
int sf_lu_plan_selinv_trace_device(sf_lu_plan* p, sf_long m, const sf_float* dVL, sf_long ldvl, const sf_float* dVU, sf_long ldvu, int flags,
                                   sf_float* d_out) {
    return trace_entry(p, true, true, m, dVL, ldvl, dVU, ldvu, flags, d_out);
}

int sf_chol_plan_selinv_entries(sf_chol_plan* p, sf_long count, const sf_long* rows, const sf_long* cols, sf_float* out, sf_long* outside) {
    return entries_entry(p, false, count, rows, cols, out, outside);
}
int sf_lu_plan_selinv_entries(sf_lu_plan* p, sf_long count, const sf_long* rows, const sf_long* cols, sf_float* out, sf_long* outside) {
    return entries_entry(p, true, count, rows, cols, out, outside);
}

}  // extern "C"

// what sf_chol_plan_stat reports as "selinv_pattern_chunk" / "_tile" / "_entries_chunk" / "_max_m"
double sf_selpat_constant(int which) {
    switch (which) {
        case 0: return sf::SELPAT_CHUNK;
        case 1: return sf::SELPAT_TILE;
        case 2: return (double)sf::SELPAT_ENT_CHUNK;
        case 3: return sf::SELPAT_MAX_M;
    }
    return -1;
}
