// Selected inversion (Takahashi equations, supernodal SelInv) and the log-determinant of a resident Cholesky factor.
//
// Sigma = A^-1 = (L L^T)^-1 on the pattern of L, in a plan-owned arena with the factor's layout (panel s at Lsxp[s],
// nsrow x nscol column-major).  The factor is processed in column UNITS, from the last unit of the root down to the leaves
// (reverse level order; inside a supernode from its last unit to its first).  A unit is w consecutive columns C of one
// supernode J; R = the panel rows below the unit's diagonal block (J's later columns, then J's below-diagonal rows):
//
//   Linv = L(C,C)^-1,  Y = L(R,C) Linv,  Z = Sigma(R,R) Y,  Sigma(R,C) = -Z,  Sigma(C,C) = Linv^T Linv + Y^T Z
//
// Sigma(R,R) is read where the Schur-update scatter of the factorization writes: entry (hi, lo) of two panel positions
// lo <= hi of J lies in column lo's own panel -- J's (direct addressing) when lo < nscol, otherwise ancestor a =
// SuperMap[row lo], at the position the relative map of the scatter problem (J, a) gives for row hi (k_build_relmaps).
// Only the lower triangle is ever read; the strict upper part of each diagonal block gets the mirror for the caller.
//
//   k_selinv_small  : one workgroup per narrow supernode (nscol <= SEL_SMALL_W, short R), the whole supernode as one unit
//   k_selinv_trinv  : Linv of one unit, one workgroup per column
//   k_selinv_gemm   : (sf_selinv_common.h, shared with the LU selected inversion) fp64 MFMA (v_mfma_f64_16x16x4_f64) C = op(A) B, 64 x 64 tiles; A plain, transposed or the gathered
//                     Sigma(R,R); optional split of K into slabs (no atomics: the slabs are summed in a fixed order)
//   k_selinv_sum    : the fixed-order slab sum
//   k_selinv_finish : Sigma(R,C) = -Z (with the mirror for R rows inside J) and Sigma(C,C) with its mirror
//   k_selinv_diag   : diag(Sigma) gathered into n doubles
//   k_logdet_part / k_logdet_final : 2 sum log L_jj, fixed-order two-pass reduction
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "sf_selinv_common.h"

namespace sf {

// ---------------------------------------------------------------------------------------------------------------------------
// narrow supernodes: one workgroup does the whole supernode (cb = 0, w = nscol <= SEL_SMALL_W, R = its below rows) in LDS
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_selinv_small(const SelUnit* __restrict__ units, const double* __restrict__ Lsx, double* __restrict__ S,
               const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap, const int64_t* __restrict__ Lsip,
               const int32_t* __restrict__ Lsi, const int64_t* __restrict__ Lsxp, const SelPair* __restrict__ pairs,
               const int32_t* __restrict__ relmap) {
    __shared__ double Li[SEL_SMALL_W * SEL_SMALL_W];        // Linv, column-major, leading dimension w
    __shared__ double Ys[SEL_SMALL_Y];                      // Y, column-major, leading dimension m
    __shared__ int64_t cbase[SEL_SMALL_M], cmoff[SEL_SMALL_M];
    const SelUnit u = units[blockIdx.x];
    const int tid = threadIdx.x, w = u.w, ns = u.nsrow, ce = u.cb + w, m = ns - ce;
    const double* __restrict__ L = Lsx + u.lx;
    double* __restrict__ Sg = S + u.lx;
    // Linv, one column per lane: forward substitution L x = e_j
    if (tid < w) {
        const int j = tid;
        for (int i = 0; i < w; ++i) Li[i + j * w] = 0.0;
        for (int i = j; i < w; ++i) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s -= L[(int64_t)(u.cb + k) * ns + u.cb + i] * Li[k + j * w];
            Li[i + j * w] = s / L[(int64_t)(u.cb + i) * ns + u.cb + i];
        }
    }
    for (int x = tid; x < m; x += 256) {
        const SelCol c = sel_col(u, ce + x, Super, SuperMap, Lsip, Lsi, Lsxp, pairs);
        cbase[x] = c.base;
        cmoff[x] = c.moff;
    }
    __syncthreads();
    // Y(x, c) = sum_{k >= c} L(R_x, C_k) Linv(k, c)
    for (int e = tid; e < m * w; e += 256) {
        const int x = e % m, c = e / m;
        double s = 0.0;
        for (int k = c; k < w; ++k) s += L[(int64_t)(u.cb + k) * ns + ce + x] * Li[k + c * w];
        Ys[x + c * m] = s;
    }
    __syncthreads();
    // Z(x, c0 .. c0+15) = sum_y Sigma(R_x, R_y) Y(y, c), Sigma(R,C) = -Z straight into the arena
    const int ng = (w + 15) / 16;
    for (int e = tid; e < m * ng; e += 256) {
        const int x = e % m, c0 = 16 * (e / m);
        double acc[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = 0.0;
        const SelCol cx{cbase[x], cmoff[x]};
        for (int y = 0; y < m; ++y) {
            const double sv = (x >= y) ? sel_at(SelCol{cbase[y], cmoff[y]}, ce + x, relmap, S) : sel_at(cx, ce + y, relmap, S);
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (c0 + t < w) acc[t] += sv * Ys[y + (c0 + t) * m];
        }
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (c0 + t < w) Sg[(int64_t)(u.cb + c0 + t) * ns + ce + x] = -acc[t];
    }
    __syncthreads();
    // Sigma(C,C)(i, j), i >= j: Linv^T Linv + Y^T Z, with Z = -Sigma(R,C) as just written; lower part and mirror
    for (int e = tid; e < w * w; e += 256) {
        const int i = e % w, j = e / w;
        if (i < j) continue;
        double s = 0.0;
        for (int k = i; k < w; ++k) s += Li[k + i * w] * Li[k + j * w];
        for (int x = 0; x < m; ++x) s -= Ys[x + i * m] * Sg[(int64_t)(u.cb + j) * ns + ce + x];
        Sg[(int64_t)(u.cb + j) * ns + u.cb + i] = s;
        Sg[(int64_t)(u.cb + i) * ns + u.cb + j] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Linv = L(C,C)^-1 of one unit (w <= SEL_UW): workgroup j solves L x = e_j column-oriented, one lane per row
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SEL_UW)
k_selinv_trinv(SelUnit u, const double* __restrict__ Lsx, double* __restrict__ Linv) {
    __shared__ double b[SEL_UW];
    const int j = blockIdx.x, k = threadIdx.x, w = u.w, ns = u.nsrow;
    const double* __restrict__ L = Lsx + u.lx + (int64_t)u.cb * ns + u.cb;       // L(C,C), leading dimension ns
    if (k < w) {
        b[k] = (k == j) ? 1.0 : 0.0;
        if (k < j) Linv[k + (int64_t)j * w] = 0.0;
    }
    for (int i = j; i < w; ++i) {
        __syncthreads();
        const double xi = b[i] / L[(int64_t)i * ns + i];
        if (k > i && k < w) b[k] -= L[(int64_t)i * ns + k] * xi;
        if (k == i) Linv[i + (int64_t)j * w] = xi;
    }
}

// dst[e] (+)= sum_{z < nslab} src[z * stride + e], z in increasing order
__global__ void __launch_bounds__(256)
k_selinv_sum(const double* __restrict__ src, int nslab, int64_t stride, int64_t count, double* __restrict__ dst, int acc_in) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double s = acc_in ? dst[e] : 0.0;
    for (int z = 0; z < nslab; ++z) s += src[(int64_t)z * stride + e];
    dst[e] = s;
}

// Sigma(R,C) = -Z (m x w, leading dimension m), mirrored above the diagonal block for the R rows that are J's own columns;
// Sigma(C,C) from the lower triangle of Sc (w x w) into both triangles of the unit's diagonal block
__global__ void __launch_bounds__(256)
k_selinv_finish(SelUnit u, const double* __restrict__ Z, const double* __restrict__ Sc, double* __restrict__ S) {
    const int w = u.w, ns = u.nsrow, ce = u.cb + w, m = ns - ce;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double* __restrict__ Sg = S + u.lx;
    if (e < (int64_t)m * w) {
        const int x = (int)(e % m), c = (int)(e / m);
        const double v = -Z[e];
        Sg[(int64_t)(u.cb + c) * ns + ce + x] = v;
        if (ce + x < u.ncol) Sg[(int64_t)(ce + x) * ns + u.cb + c] = v;
        return;
    }
    const int64_t d = e - (int64_t)m * w;
    if (d >= (int64_t)w * w) return;
    const int i = (int)(d % w), j = (int)(d / w);
    Sg[(int64_t)(u.cb + j) * ns + u.cb + i] = (i >= j) ? Sc[i + (int64_t)j * w] : Sc[j + (int64_t)i * w];
}

// d[j] = Sigma(j, j)
__global__ void __launch_bounds__(256)
k_selinv_diag(int64_t n, const double* __restrict__ S, const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap,
              const int64_t* __restrict__ Lsip, const int64_t* __restrict__ Lsxp, double* __restrict__ d) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int32_t s = SuperMap[j];
    const int64_t c = j - Super[s];
    d[j] = S[Lsxp[s] + c * (Lsip[s + 1] - Lsip[s]) + c];
}

// per block of 256 columns: sum of log L_jj, tree in LDS (fixed order)
__global__ void __launch_bounds__(256)
k_logdet_part(int64_t n, const double* __restrict__ Lsx, const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap,
              const int64_t* __restrict__ Lsip, const int64_t* __restrict__ Lsxp, double* __restrict__ part) {
    __shared__ double red[256];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (j < n) {
        const int32_t s = SuperMap[j];
        const int64_t c = j - Super[s];
        v = log(Lsx[Lsxp[s] + c * (Lsip[s + 1] - Lsip[s]) + c]);
    }
    red[threadIdx.x] = v;
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// out = 2 sum part[0 .. np): lane t sums parts t, t + 256, ... in order, then the same tree
__global__ void __launch_bounds__(256)
k_logdet_final(const double* __restrict__ part, int64_t np, double* __restrict__ out) {
    __shared__ double red[256];
    double v = 0.0;
    for (int64_t k = threadIdx.x; k < np; k += 256) v += part[k];
    red[threadIdx.x] = v;
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    }
    if (threadIdx.x == 0) out[0] = 2.0 * red[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// the launchers (sf_kernels.h): one launch each
// ---------------------------------------------------------------------------------------------------------------------------
void launch_selinv_small(const SelUnit* units, int nunits, const double* Lsx, double* S, const SelStruct& t, hipStream_t st) {
    if (nunits <= 0) return;
    hipLaunchKernelGGL(k_selinv_small, dim3((unsigned)nunits), dim3(256), 0, st, units, Lsx, S, t.Super, t.SuperMap, t.Lsip, t.Lsi, t.Xp,
                       t.pairs, t.relmap);
}

void launch_selinv_trinv(const SelUnit& u, const double* Lsx, double* Linv, hipStream_t st) {
    hipLaunchKernelGGL(k_selinv_trinv, dim3(u.w), dim3(SEL_UW), 0, st, u, Lsx, Linv);
}

void launch_selinv_gemm(int am, int M, int N, int K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
                        int slabs, int64_t cstride, int acc_in, const SelUnit& u, const double* S, const double* S2, const SelStruct& t,
                        hipStream_t st) {
    if (am == 0) selinv_gemm<0>(M, N, K, A, lda, B, ldb, C, ldc, slabs, cstride, acc_in, u, S, S2, t, st);
    else if (am == 1) selinv_gemm<1>(M, N, K, A, lda, B, ldb, C, ldc, slabs, cstride, acc_in, u, S, S2, t, st);
    else selinv_gemm<2>(M, N, K, A, lda, B, ldb, C, ldc, slabs, cstride, acc_in, u, S, S2, t, st);
}

void launch_selinv_sum(const double* src, int nslab, int64_t stride, int64_t count, double* dst, int acc_in, hipStream_t st) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_selinv_sum, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, src, nslab, stride, count, dst, acc_in);
}

void launch_selinv_finish(const SelUnit& u, const double* Z, const double* Sc, double* S, hipStream_t st) {
    const int64_t w = u.w, m = u.nsrow - u.cb - u.w;
    const int64_t tot = m * w + w * w;
    hipLaunchKernelGGL(k_selinv_finish, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, u, Z, Sc, S);
}

void launch_selinv_diag(int64_t n, const double* S, const SelStruct& t, double* d, hipStream_t st) {
    hipLaunchKernelGGL(k_selinv_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, S, t.Super, t.SuperMap, t.Lsip, t.Xp, d);
}

void launch_logdet(int64_t n, const double* Lsx, const SelStruct& t, double* buf, hipStream_t st) {
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(k_logdet_part, dim3((unsigned)nb), dim3(256), 0, st, n, Lsx, t.Super, t.SuperMap, t.Lsip, t.Xp, buf);
    hipLaunchKernelGGL(k_logdet_final, dim3(1), dim3(256), 0, st, (const double*)buf, nb, buf + nb);
}

}  // namespace sf

// ===========================================================================================================================
// host side
// ===========================================================================================================================
namespace {

using sf::SelUnit;

int64_t slabs_for(int64_t tiles, int64_t K) {
    if (tiles <= 0 || tiles >= 256 || K < 512) return 1;         // (a unit with no rows below: no product at all)
    return std::max<int64_t>(1, std::min<int64_t>({sf::SEL_MAX_SLABS, (256 + tiles - 1) / tiles, K / 256}));
}

double unit_flops(double m, double w) { return 2.0 * m * m * w + 2.0 * m * w * w + 2.0 / 3.0 * w * w * w; }

}  // namespace

int sf_selinv_schedule(sf_chol_plan* p) {
    const int64_t ns = p->nsuper;
    const std::vector<int64_t>& Lsip = p->h_Lsip;
    const std::vector<int64_t>& Lsxp = p->lu ? p->h_XP : p->h_Lsxp;      // the panels' offsets on the device
    const double sides = p->lu ? 2.0 : 1.0;                              // LU: every product of a unit once per panel set
    const std::vector<int32_t>& Super = p->h_Super;
    // (J, a) -> map_off, bucketed by J (recorded in enumeration order while plan_create built the scatter problems)
    std::vector<int32_t> pf(ns + 1, 0);
    const size_t np = p->sel_pair_J.size();
    for (size_t k = 0; k < np; ++k) pf[p->sel_pair_J[k] + 1]++;
    for (int64_t s = 0; s < ns; ++s) pf[s + 1] += pf[s];
    std::vector<sf::SelPair> pairs(std::max<size_t>(np, 1));
    {
        std::vector<int32_t> fill(pf.begin(), pf.end() - 1);
        for (size_t k = 0; k < np; ++k) pairs[fill[p->sel_pair_J[k]]++] = sf::SelPair{p->sel_pair_off[k], p->sel_pair_i[k], 0};
        for (int64_t s = 0; s < ns; ++s)
            std::sort(pairs.begin() + pf[s], pairs.begin() + pf[s + 1], [](const sf::SelPair& a, const sf::SelPair& b) { return a.i < b.i; });
    }
    int maxlev = 0;
    for (int64_t s = 0; s < ns; ++s) maxlev = std::max(maxlev, p->level_of[s]);
    std::vector<std::vector<int64_t>> bylev(maxlev + 1);
    for (int64_t s = 0; s < ns; ++s) bylev[p->level_of[s]].push_back(s);
    p->sel_small.clear();
    p->sel_steps.clear();
    p->sel_big.clear();
    p->flops_selinv = 0;
    int64_t linv = 1, ysz = 1, zsl = 1, ssl = 1;
    for (int lev = maxlev; lev >= 0; --lev) {
        const size_t small0 = p->sel_small.size(), big0 = p->sel_big.size();
        for (int64_t s : bylev[lev]) {
            SelUnit u{};
            u.lx = Lsxp[s];
            u.rows = Lsip[s];
            u.nsrow = (int32_t)(Lsip[s + 1] - Lsip[s]);
            u.ncol = Super[s + 1] - Super[s];
            u.pair0 = pf[s];
            u.npair = pf[s + 1] - pf[s];
            const int64_t mb = u.nsrow - u.ncol;
            if (u.ncol <= sf::SEL_SMALL_W && mb <= sf::SEL_SMALL_M && mb * u.ncol <= sf::SEL_SMALL_Y) {
                u.cb = 0; u.w = u.ncol;
                p->sel_small.push_back(u);
                p->flops_selinv += sides * unit_flops((double)mb, (double)u.w);
                continue;
            }
            for (int cb = ((u.ncol - 1) / sf::SEL_UW) * sf::SEL_UW; cb >= 0; cb -= sf::SEL_UW) {
                u.cb = cb;
                u.w = std::min(sf::SEL_UW, u.ncol - cb);
                const int64_t m = u.nsrow - cb - u.w, w = u.w;
                const int64_t tw = (w + 63) / 64;
                const sf_chol_plan::SelBig b{u, (int)slabs_for(((m + 63) / 64) * tw, m), (int)slabs_for(tw * tw, m)};
                p->sel_big.push_back(b);
                linv = std::max(linv, w * w);
                ysz = std::max(ysz, m * w);
                zsl = std::max(zsl, (int64_t)b.zslabs * m * w);
                ssl = std::max(ssl, (int64_t)b.sslabs * w * w);
                p->flops_selinv += sides * unit_flops((double)m, (double)w);
            }
        }
        // one step per level: the level's big units (in list order), then its narrow supernodes in one launch
        p->sel_steps.push_back(sf_chol_plan::SelStep{(int64_t)small0, (int64_t)(p->sel_small.size() - small0), (int64_t)big0,
                                                     (int64_t)(p->sel_big.size() - big0)});
    }
    p->sel_linv_elems = linv;
    p->sel_y_elems = ysz;
    p->sel_z_elems = zsl;       // Z slabs (the summed Z goes to the Y-sized buffer Zs)
    p->sel_s_elems = ssl;
    p->sel_pairs_h = std::move(pairs);
    p->sel_scheduled = true;
    return SF_OK;
}

namespace {

template <int AM>
void gemm(sf_chol_plan* p, int M, int N, int K, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc,
          int slabs, int64_t cstride, int acc_in, const SelUnit& u, hipStream_t st) {
    sf::selinv_gemm<AM>(M, N, K, A, lda, B, ldb, C, ldc, slabs, cstride, acc_in, u, p->d_sel, p->d_sel, sf::sel_struct(p), st);
}

// one unit of a wide or long supernode
void run_big(sf_chol_plan* p, const sf_chol_plan::SelBig& b, hipStream_t st) {
    const SelUnit& u = b.u;
    const int w = u.w, m = u.nsrow - u.cb - u.w;
    double* Linv = p->d_sel_scratch;
    double* Y = Linv + p->sel_linv_elems;
    double* Zs = Y + p->sel_y_elems;
    double* Zsl = Zs + p->sel_y_elems;
    double* Ssl = Zsl + p->sel_z_elems;
    double* Sc = Ssl + p->sel_s_elems;
    const double* L = p->d_Lsx;
    sf::launch_selinv_trinv(u, L, Linv, st);
    // Sc = Linv^T Linv
    gemm<1>(p, w, w, w, Linv, w, Linv, w, Sc, w, 1, 0, 0, u, st);
    if (m > 0) {
        gemm<0>(p, m, w, w, L + u.lx + (int64_t)u.cb * u.nsrow + u.cb + w, u.nsrow, Linv, w, Y, m, 1, 0, 0, u, st);   // Y = L(R,C) Linv
        if (b.zslabs == 1) {
            gemm<2>(p, m, w, m, nullptr, 0, Y, m, Zs, m, 1, 0, 0, u, st);                                               // Z = Sigma(R,R) Y
        } else {
            gemm<2>(p, m, w, m, nullptr, 0, Y, m, Zsl, m, b.zslabs, (int64_t)m * w, 0, u, st);
            sf::launch_selinv_sum(Zsl, b.zslabs, (int64_t)m * w, (int64_t)m * w, Zs, 0, st);
        }
        if (b.sslabs == 1) {
            gemm<1>(p, w, w, m, Y, m, Zs, m, Sc, w, 1, 0, 1, u, st);                                                      // Sc += Y^T Z
        } else {
            gemm<1>(p, w, w, m, Y, m, Zs, m, Ssl, w, b.sslabs, (int64_t)w * w, 0, u, st);
            sf::launch_selinv_sum(Ssl, b.sslabs, (int64_t)w * w, (int64_t)w * w, Sc, 1, st);
        }
    }
    sf::launch_selinv_finish(u, Zs, Sc, p->d_sel, st);
}

}  // namespace

extern "C" {

int sf_chol_plan_selinv(sf_chol_plan* p) {
    if (!p || p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    return sf_selinv_run(
        p, (size_t)std::max<int64_t>(p->xsize, 1),
        [p] { return (size_t)(2 * p->sel_linv_elems + 2 * p->sel_y_elems + p->sel_z_elems + p->sel_s_elems); },
        [p](const sf_chol_plan::SelBig& b, hipStream_t st) { run_big(p, b, st); },
        [p](const SelUnit* units, int count, hipStream_t st) { sf::launch_selinv_small(units, count, p->d_Lsx, p->d_sel, sf::sel_struct(p), st); });
}

int sf_chol_plan_get_selinv_range(sf_chol_plan* p, sf_long e_begin, sf_long e_end, sf_float* out) {
    if (!p || p->lu || !sf_plan_whole_resident(p) || e_begin < 0 || e_end > p->xsize || e_end < e_begin || (!out && e_end > e_begin)) return SF_ERR_ARG;
    if (!p->d_sel || !p->fs.selinv_matches()) return SF_ERR_ARG;
    if (e_end == e_begin) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipMemcpyAsync(out, p->d_sel + e_begin, (e_end - e_begin) * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SF_OK;
}

int sf_chol_plan_selinv_diag(sf_chol_plan* p, sf_float* d) {
    if (!p || p->lu || !sf_plan_whole_resident(p) || (!d && p->n > 0)) return SF_ERR_ARG;
    return sf_selinv_diag_run(p, d, sf::launch_selinv_diag);
}

int sf_chol_plan_logdet(sf_chol_plan* p, sf_float* out) {
    if (!p || !out || p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    if (!sf_factor_current(p)) return SF_ERR_ARG;
    *out = 0.0;
    if (p->n <= 0) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    const int64_t nb = (p->n + 255) / 256;
    sf::DevMem<double> buf;
    if (buf.alloc((size_t)nb + 1)) return SF_ERR_HIP;
    sf::launch_logdet((int64_t)p->n, p->d_Lsx, sf::sel_struct(p), buf, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, buf + nb, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SF_OK;
}

}  // extern "C"
