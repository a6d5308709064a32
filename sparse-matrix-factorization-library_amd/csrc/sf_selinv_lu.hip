// Selected inversion and the log-determinant of a resident no-pivot LU factor.
//
// Sigma = A^-1 = (L U)^-1 on the pattern of L + U, in a plan-owned PAIR of arenas with the device factor's own layout (panel s at
// Xp[s], nsrow x nscol column-major; the second set xC doubles after the first):
//   SL(r, c) = Sigma(row of panel position r, column c),      SU(r, c) = Sigma(column c, row of panel position r)
// (diagonal blocks full in both: SL holds Sigma(C_J, C_J), SU its transpose).  Units, order and addressing are those of the
// Cholesky selected inversion (sf_selinv.hip); every operation is that one with its two operand roles taken from different panels.
// For a unit C of supernode J, R = the panel rows below the unit's diagonal block, PL(i,j) = L(i,j), PU(i,j) = U(j,i):
//
//   Tl = PL(C,C) (unit lower; only its strict lower part is read),  Tu = PU(C,C) = U(C,C)^T (lower),  G = Sigma(R,R)
//   Yl = PL(R,C) Tl^-1,  Yu = PU(R,C) Tu^-1,  Zl = G Yl,  Zu = G^T Yu
//   Sigma(R,C) = -Zl,  Sigma(C,R)^T = -Zu,  Sigma(C,C) = Tu^-T Tl^-1 + Yu^T Zl
//
// Entry (x, y) of G: panel position of x >= that of y -- from SL, in column y's own panel at the row position of x; otherwise from
// SU, in column x's own panel at the row position of y.  G^T: the two sets swapped.
//
//   k_lu_selinv_small  : one workgroup per narrow supernode, the whole supernode as one unit, Tl^-1, Tu^-1, Yl, Yu in LDS
//   k_lu_selinv_trinv  : the inverse of one unit's lower triangle (unit or stored diagonal), one workgroup per column
//   k_selinv_gemm      : (sf_selinv_common.h) plain, transposed, and gathered with the arenas (SL, SU) for G, (SU, SL) for G^T
//   k_lu_selinv_finish : -Zl and -Zu into SL(R,C) and SU(R,C), their mirrors for the R rows inside J, Sigma(C,C) into both sets
//   k_lu_selinv_pack   : the pair of arenas gathered into the reference's packed panels for the download
//   k_lu_selinv_diag   : diag(Sigma) gathered into n doubles
//   k_lu_logdet_part / k_lu_logdet_final : sum log|U_jj| and the number of negative U_jj, fixed-order two-pass reduction
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "sf_selinv_common.h"

namespace sf {

// ---------------------------------------------------------------------------------------------------------------------------
// narrow supernodes: one workgroup does the whole supernode (cb = 0, w = nscol <= SEL_SMALL_W, R = its below rows) in LDS
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_lu_selinv_small(const SelUnit* __restrict__ units, const double* __restrict__ PL, const double* __restrict__ PU, double* SL, double* SU,
                  const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap, const int64_t* __restrict__ Lsip,
                  const int32_t* __restrict__ Lsi, const int64_t* __restrict__ Xp, const SelPair* __restrict__ pairs,
                  const int32_t* __restrict__ relmap) {
    __shared__ double Tl[SEL_SMALL_W * SEL_SMALL_W], Tu[SEL_SMALL_W * SEL_SMALL_W];     // Tl^-1, Tu^-1, column-major, leading dimension w
    __shared__ double Yl[SEL_SMALL_Y], Yu[SEL_SMALL_Y];                                 // column-major, leading dimension m
    __shared__ int64_t cbase[SEL_SMALL_M], cmoff[SEL_SMALL_M];
    const SelUnit u = units[blockIdx.x];
    const int tid = threadIdx.x, w = u.w, ns = u.nsrow, ce = u.cb + w, m = ns - ce;
    // wave 0: Tl^-1 (unit diagonal, the stored one is not read), wave 1: Tu^-1; one column per lane, forward substitution T x = e_j
    if (tid < 128 && (tid & 63) < w) {
        const int j = tid & 63;
        const bool up = tid >= 64;
        const double* __restrict__ T = (up ? PU : PL) + u.lx;
        double* Ti = up ? Tu : Tl;
        for (int i = 0; i < j; ++i) Ti[i + j * w] = 0.0;
        for (int i = j; i < w; ++i) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s -= T[(int64_t)(u.cb + k) * ns + u.cb + i] * Ti[k + j * w];
            Ti[i + j * w] = up ? s / T[(int64_t)(u.cb + i) * ns + u.cb + i] : s;
        }
    }
    for (int x = tid; x < m; x += 256) {
        const SelCol c = sel_col(u, ce + x, Super, SuperMap, Lsip, Lsi, Xp, pairs);
        cbase[x] = c.base;
        cmoff[x] = c.moff;
    }
    __syncthreads();
    // Y(x, c) = sum_{k >= c} P(R_x, C_k) T^-1(k, c), for both panels
    for (int e = tid; e < 2 * m * w; e += 256) {
        const bool up = e >= m * w;
        const int f = up ? e - m * w : e, x = f % m, c = f / m;
        const double* __restrict__ P = (up ? PU : PL) + u.lx;
        const double* Ti = up ? Tu : Tl;
        double s = 0.0;
        for (int k = c; k < w; ++k) s += P[(int64_t)(u.cb + k) * ns + ce + x] * Ti[k + c * w];
        (up ? Yu : Yl)[x + c * m] = s;
    }
    __syncthreads();
    // Zl(x, c0 .. c0+15) = sum_y G(x, y) Yl(y, c) and Zu = sum_y G(y, x) Yu(y, c); -Zl, -Zu straight into the two arenas
    const int ng = (w + 15) / 16;
    for (int e = tid; e < 2 * m * ng; e += 256) {
        const bool up = e >= m * ng;
        const int f = up ? e - m * ng : e, x = f % m, c0 = 16 * (f / m);
        const double* Sa = up ? SU : SL;        // x >= y: column y's panel
        const double* Sb = up ? SL : SU;        // x <  y: column x's panel
        const double* Y = up ? Yu : Yl;
        double acc[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[t] = 0.0;
        const SelCol cx{cbase[x], cmoff[x]};
        for (int y = 0; y < m; ++y) {
            const double sv = (x >= y) ? sel_at(SelCol{cbase[y], cmoff[y]}, ce + x, relmap, Sa) : sel_at(cx, ce + y, relmap, Sb);
#pragma unroll
            for (int t = 0; t < 16; ++t)
                if (c0 + t < w) acc[t] += sv * Y[y + (c0 + t) * m];
        }
        double* D = (up ? SU : SL) + u.lx;
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (c0 + t < w) D[(int64_t)(u.cb + c0 + t) * ns + ce + x] = -acc[t];
    }
    __syncthreads();
    // Sigma(C,C)(i, j) = sum_k Tu^-1(k, i) Tl^-1(k, j) + sum_x Yu(x, i) Zl(x, j), with Zl = -SL(R,C) as just written
    double* SLg = SL + u.lx;
    double* SUg = SU + u.lx;
    for (int e = tid; e < w * w; e += 256) {
        const int i = e % w, j = e / w;
        double s = 0.0;
        for (int k = max(i, j); k < w; ++k) s += Tu[k + i * w] * Tl[k + j * w];
        for (int x = 0; x < m; ++x) s -= Yu[x + i * m] * SLg[(int64_t)(u.cb + j) * ns + ce + x];
        SLg[(int64_t)(u.cb + j) * ns + u.cb + i] = s;
        SUg[(int64_t)(u.cb + i) * ns + u.cb + j] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Tinv = T^-1 for the lower triangle T of one unit's diagonal block in the panel set P (w <= SEL_UW): workgroup j solves T x = e_j
// column-oriented, one lane per row.  unit != 0: the diagonal is 1 and the stored one is not read (PL); otherwise it is read (PU)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SEL_UW)
k_lu_selinv_trinv(SelUnit u, const double* __restrict__ P, int unit, double* __restrict__ Tinv) {
    __shared__ double b[SEL_UW];
    const int j = blockIdx.x, k = threadIdx.x, w = u.w, ns = u.nsrow;
    const double* __restrict__ T = P + u.lx + (int64_t)u.cb * ns + u.cb;       // leading dimension ns
    if (k < w) {
        b[k] = (k == j) ? 1.0 : 0.0;
        if (k < j) Tinv[k + (int64_t)j * w] = 0.0;
    }
    for (int i = j; i < w; ++i) {
        __syncthreads();
        const double xi = unit ? b[i] : b[i] / T[(int64_t)i * ns + i];
        if (k > i && k < w) b[k] -= T[(int64_t)i * ns + k] * xi;
        if (k == i) Tinv[i + (int64_t)j * w] = xi;
    }
}

// SL(R,C) = -Zl and SU(R,C) = -Zu (m x w, leading dimension m); for the R rows that are J's own later columns the same values
// belong to the other set's diagonal block (Sigma(R,C) to SU of those columns, Sigma(C,R) to SL); Sigma(C,C) = Sc (w x w) into SL
// and transposed into SU
__global__ void __launch_bounds__(256)
k_lu_selinv_finish(SelUnit u, const double* __restrict__ Zl, const double* __restrict__ Zu, const double* __restrict__ Sc, double* SL,
                   double* SU) {
    const int w = u.w, ns = u.nsrow, ce = u.cb + w, m = ns - ce;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double* SLg = SL + u.lx;
    double* SUg = SU + u.lx;
    if (e < (int64_t)m * w) {
        const int x = (int)(e % m), c = (int)(e / m);
        const double vl = -Zl[e], vu = -Zu[e];
        SLg[(int64_t)(u.cb + c) * ns + ce + x] = vl;
        SUg[(int64_t)(u.cb + c) * ns + ce + x] = vu;
        if (ce + x < u.ncol) {
            SUg[(int64_t)(ce + x) * ns + u.cb + c] = vl;
            SLg[(int64_t)(ce + x) * ns + u.cb + c] = vu;
        }
        return;
    }
    const int64_t d = e - (int64_t)m * w;
    if (d >= (int64_t)w * w) return;
    const int i = (int)(d % w), j = (int)(d / w);
    const double s = Sc[i + (int64_t)j * w];
    SLg[(int64_t)(u.cb + j) * ns + u.cb + i] = s;
    SUg[(int64_t)(u.cb + i) * ns + u.cb + j] = s;
}

// values [e_begin, e_end) of the reference's packed layout (panel s at RefXp[s], (2 nsrow - nscol) x nscol column-major): rows
// [0, nsrow) of a column from SL, rows [nsrow, 2 nsrow - nscol) = rows [nscol, nsrow) of SU
__global__ void __launch_bounds__(256)
k_lu_selinv_pack(const int32_t* __restrict__ Super, const int64_t* __restrict__ Lsip, const int64_t* __restrict__ Xp,
                 const int64_t* __restrict__ RefXp, int32_t nsuper, const double* __restrict__ SL, const double* __restrict__ SU,
                 double* __restrict__ out, int64_t e_begin, int64_t e_end) {
    for (int64_t e = e_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < e_end; e += (int64_t)gridDim.x * blockDim.x) {
        int lo = 0, hi = nsuper;            // largest s with RefXp[s] <= e
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (RefXp[mid] <= e) lo = mid; else hi = mid;
        }
        const int s = lo;
        const int64_t nscol = Super[s + 1] - Super[s], nsrow = Lsip[s + 1] - Lsip[s];
        const int64_t lda = 2 * nsrow - nscol;
        const int64_t off = e - RefXp[s];
        const int64_t j = off / lda, R = off % lda;
        out[e - e_begin] = (R < nsrow) ? SL[Xp[s] + j * nsrow + R] : SU[Xp[s] + j * nsrow + (R - nsrow + nscol)];
    }
}

// d[j] = Sigma(j, j)
__global__ void __launch_bounds__(256)
k_lu_selinv_diag(int64_t n, const double* __restrict__ SL, const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap,
                 const int64_t* __restrict__ Lsip, const int64_t* __restrict__ Xp, double* __restrict__ d) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int32_t s = SuperMap[j];
    const int64_t c = j - Super[s];
    d[j] = SL[Xp[s] + c * (Lsip[s + 1] - Lsip[s]) + c];
}

// per block of 256 columns: sum of log|U_jj| and the number of negative U_jj, trees in LDS (fixed order)
__global__ void __launch_bounds__(256)
k_lu_logdet_part(int64_t n, const double* __restrict__ PU, const int32_t* __restrict__ Super, const int32_t* __restrict__ SuperMap,
                 const int64_t* __restrict__ Lsip, const int64_t* __restrict__ Xp, double* __restrict__ part, int32_t* __restrict__ neg) {
    __shared__ double red[256];
    __shared__ int32_t cnt[256];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    int32_t c = 0;
    if (j < n) {
        const int32_t s = SuperMap[j];
        const int64_t k = j - Super[s];
        const double ujj = PU[Xp[s] + k * (Lsip[s + 1] - Lsip[s]) + k];
        v = log(fabs(ujj));
        c = ujj < 0.0 ? 1 : 0;
    }
    red[threadIdx.x] = v;
    cnt[threadIdx.x] = c;
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) {
            red[threadIdx.x] += red[threadIdx.x + h];
            cnt[threadIdx.x] += cnt[threadIdx.x + h];
        }
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = red[0];
        neg[blockIdx.x] = cnt[0];
    }
}

// out[0] = sum part[0 .. np), out[1] = (sum neg[0 .. np)) mod 2: lane t sums parts t, t + 256, ... in order, then the same tree
__global__ void __launch_bounds__(256)
k_lu_logdet_final(const double* __restrict__ part, const int32_t* __restrict__ neg, int64_t np, double* __restrict__ out) {
    __shared__ double red[256];
    __shared__ int32_t cnt[256];
    double v = 0.0;
    int32_t c = 0;
    for (int64_t k = threadIdx.x; k < np; k += 256) {
        v += part[k];
        c ^= neg[k] & 1;
    }
    red[threadIdx.x] = v;
    cnt[threadIdx.x] = c;
    for (int h = 128; h > 0; h >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < h) {
            red[threadIdx.x] += red[threadIdx.x + h];
            cnt[threadIdx.x] ^= cnt[threadIdx.x + h];
        }
    }
    if (threadIdx.x == 0) {
        out[0] = red[0];
        out[1] = (double)cnt[0];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the launchers (sf_kernels.h): one launch each
// ---------------------------------------------------------------------------------------------------------------------------
void launch_lu_selinv_small(const SelUnit* units, int nunits, const double* PL, const double* PU, double* SL, double* SU, const SelStruct& t,
                            hipStream_t st) {
    if (nunits <= 0) return;
    hipLaunchKernelGGL(k_lu_selinv_small, dim3((unsigned)nunits), dim3(256), 0, st, units, PL, PU, SL, SU, t.Super, t.SuperMap, t.Lsip, t.Lsi,
                       t.Xp, t.pairs, t.relmap);
}

void launch_lu_selinv_trinv(const SelUnit& u, const double* P, int unit, double* Tinv, hipStream_t st) {
    hipLaunchKernelGGL(k_lu_selinv_trinv, dim3(u.w), dim3(SEL_UW), 0, st, u, P, unit, Tinv);
}

void launch_lu_selinv_finish(const SelUnit& u, const double* Zl, const double* Zu, const double* Sc, double* SL, double* SU, hipStream_t st) {
    const int64_t w = u.w, m = u.nsrow - u.cb - u.w;
    const int64_t tot = m * w + w * w;
    hipLaunchKernelGGL(k_lu_selinv_finish, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, u, Zl, Zu, Sc, SL, SU);
}

void launch_lu_selinv_pack(const SelStruct& t, const int64_t* RefXp, int32_t nsuper, const double* SL, const double* SU, double* out,
                           int64_t e_begin, int64_t e_end, hipStream_t st) {
    const int64_t blocks = (e_end - e_begin + 255) / 256;
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_lu_selinv_pack, dim3((unsigned)std::min<int64_t>(blocks, 65536)), dim3(256), 0, st, t.Super, t.Lsip, t.Xp, RefXp, nsuper,
                       SL, SU, out, e_begin, e_end);
}

void launch_lu_selinv_diag(int64_t n, const double* SL, const SelStruct& t, double* d, hipStream_t st) {
    hipLaunchKernelGGL(k_lu_selinv_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, SL, t.Super, t.SuperMap, t.Lsip, t.Xp, d);
}

void launch_lu_logdet(int64_t n, const double* PU, const SelStruct& t, double* buf, int32_t* neg, hipStream_t st) {
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(k_lu_logdet_part, dim3((unsigned)nb), dim3(256), 0, st, n, PU, t.Super, t.SuperMap, t.Lsip, t.Xp, buf, neg);
    hipLaunchKernelGGL(k_lu_logdet_final, dim3(1), dim3(256), 0, st, (const double*)buf, (const int32_t*)neg, nb, buf + nb);
}

}  // namespace sf

// ===========================================================================================================================
// host side
// ===========================================================================================================================
namespace {

using sf::SelUnit;

// the scratch of the wide units, in d_sel_scratch
struct LuScratch { double *Tl, *Tu, *Yl, *Yu, *Zl, *Zu, *Zsl, *Ssl, *Sc; };

LuScratch lu_scratch(const sf_chol_plan* p) {
    LuScratch s;
    s.Tl = p->d_sel_scratch;
    s.Tu = s.Tl + p->sel_linv_elems;
    s.Yl = s.Tu + p->sel_linv_elems;
    s.Yu = s.Yl + p->sel_y_elems;
    s.Zl = s.Yu + p->sel_y_elems;
    s.Zu = s.Zl + p->sel_y_elems;
    s.Zsl = s.Zu + p->sel_y_elems;
    s.Ssl = s.Zsl + p->sel_z_elems;
    s.Sc = s.Ssl + p->sel_s_elems;
    return s;
}

// Z = op(G) Y over the unit's R rows: (S, S2) = (SL, SU) for G, (SU, SL) for G^T; K slabs summed in a fixed order
void gathered_product(sf_chol_plan* p, const sf_chol_plan::SelBig& b, const double* S, const double* S2, const double* Y, double* Z,
                      double* Zsl, hipStream_t st) {
    const SelUnit& u = b.u;
    const int w = u.w, m = u.nsrow - u.cb - u.w;
    const sf::SelStruct t = sf::sel_struct(p);
    if (b.zslabs == 1) {
        sf::selinv_gemm<2>(m, w, m, nullptr, 0, Y, m, Z, m, 1, 0, 0, u, S, S2, t, st);
    } else {
        sf::selinv_gemm<2>(m, w, m, nullptr, 0, Y, m, Zsl, m, b.zslabs, (int64_t)m * w, 0, u, S, S2, t, st);
        sf::launch_selinv_sum(Zsl, b.zslabs, (int64_t)m * w, (int64_t)m * w, Z, 0, st);
    }
}

// one unit of a wide or long supernode
void run_big(sf_chol_plan* p, const sf_chol_plan::SelBig& b, hipStream_t st) {
    const SelUnit& u = b.u;
    const int w = u.w, m = u.nsrow - u.cb - u.w;
    const LuScratch s = lu_scratch(p);
    const double* PL = p->d_Lsx;
    const double* PU = p->d_Lsx + p->xC;
    double* SL = p->d_sel;
    double* SU = p->d_sel + p->xC;
    const sf::SelStruct t = sf::sel_struct(p);
    const double* none = nullptr;       // the plain and transposed products gather nothing
    sf::launch_lu_selinv_trinv(u, PL, 1, s.Tl, st);
    sf::launch_lu_selinv_trinv(u, PU, 0, s.Tu, st);
    // Sc = Tu^-T Tl^-1
    sf::selinv_gemm<1>(w, w, w, s.Tu, w, s.Tl, w, s.Sc, w, 1, 0, 0, u, none, none, t, st);
    if (m > 0) {
        const int64_t below = u.lx + (int64_t)u.cb * u.nsrow + u.cb + w;        // P(R,C) in its panel set
        sf::selinv_gemm<0>(m, w, w, PL + below, u.nsrow, s.Tl, w, s.Yl, m, 1, 0, 0, u, none, none, t, st);      // Yl = PL(R,C) Tl^-1
        sf::selinv_gemm<0>(m, w, w, PU + below, u.nsrow, s.Tu, w, s.Yu, m, 1, 0, 0, u, none, none, t, st);      // Yu = PU(R,C) Tu^-1
        gathered_product(p, b, SL, SU, s.Yl, s.Zl, s.Zsl, st);                                            // Zl = G Yl
        gathered_product(p, b, SU, SL, s.Yu, s.Zu, s.Zsl, st);                                            // Zu = G^T Yu
        if (b.sslabs == 1) {
            sf::selinv_gemm<1>(w, w, m, s.Yu, m, s.Zl, m, s.Sc, w, 1, 0, 1, u, none, none, t, st);              // Sc += Yu^T Zl
        } else {
            sf::selinv_gemm<1>(w, w, m, s.Yu, m, s.Zl, m, s.Ssl, w, b.sslabs, (int64_t)w * w, 0, u, none, none, t, st);
            sf::launch_selinv_sum(s.Ssl, b.sslabs, (int64_t)w * w, (int64_t)w * w, s.Sc, 1, st);
        }
    }
    sf::launch_lu_selinv_finish(u, s.Zl, s.Zu, s.Sc, SL, SU, st);
}

// +1 / -1: the parity of the permutation pivpos (n - number of cycles)
int permutation_sign(const std::vector<sf_long>& pivpos) {
    const size_t n = pivpos.size();
    std::vector<char> seen(n, 0);
    size_t cycles = 0;
    for (size_t j = 0; j < n; ++j) {
        if (seen[j]) continue;
        ++cycles;
        for (size_t k = j; k < n && !seen[k]; k = (size_t)pivpos[k]) seen[k] = 1;
    }
    return ((n - cycles) & 1) ? -1 : 1;
}

}  // namespace

extern "C" {

int sf_lu_plan_selinv(sf_lu_plan* p) {
    if (!p || !p->lu || !sf_plan_whole_resident(p) || p->piv_tol > 0.0) return SF_ERR_ARG;
    // both arenas in one allocation: SL, then SU xC doubles later
    return sf_selinv_run(
        p, (size_t)std::max<int64_t>(2 * p->xC, 1),
        [p] { return (size_t)(3 * p->sel_linv_elems + 4 * p->sel_y_elems + p->sel_z_elems + p->sel_s_elems); },
        [p](const sf_chol_plan::SelBig& b, hipStream_t st) { run_big(p, b, st); },
        [p](const SelUnit* units, int count, hipStream_t st) {
            sf::launch_lu_selinv_small(units, count, p->d_Lsx, p->d_Lsx + p->xC, p->d_sel, p->d_sel + p->xC, sf::sel_struct(p), st);
        });
}

int sf_lu_plan_get_selinv_range(sf_lu_plan* p, sf_long e_begin, sf_long e_end, sf_float* out) {
    if (!p || !p->lu || !sf_plan_whole_resident(p) || e_begin < 0 || e_end > p->xsize || e_end < e_begin || (!out && e_end > e_begin)) return SF_ERR_ARG;
    if (!p->d_sel || !p->fs.selinv_matches()) return SF_ERR_ARG;
    if (e_end == e_begin) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    const int64_t count = e_end - e_begin;
    sf::DevMem<double> tmp;
    if (int rc = tmp.alloc((size_t)count)) return rc;
    sf::launch_lu_selinv_pack(sf::sel_struct(p), p->d_Lsxp, (int32_t)p->nsuper, p->d_sel, p->d_sel + p->xC, tmp, (int64_t)e_begin,
                              (int64_t)e_end, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, tmp, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return SF_OK;
}

int sf_lu_plan_selinv_diag(sf_lu_plan* p, sf_float* d) {
    if (!p || !p->lu || !sf_plan_whole_resident(p) || (!d && p->n > 0)) return SF_ERR_ARG;
    return sf_selinv_diag_run(p, d, sf::launch_lu_selinv_diag);
}

int sf_lu_plan_logdet(sf_lu_plan* p, sf_float* logabs, int* sign) {
    if (!p || !logabs || !p->lu || !sf_plan_whole_resident(p)) return SF_ERR_ARG;
    if (!sf_factor_current(p)) return SF_ERR_ARG;
    *logabs = 0.0;
    if (sign) *sign = 1;
    if (p->n <= 0) return SF_OK;
    HIP_TRY(hipSetDevice(p->device));
    const int64_t nb = (p->n + 255) / 256;
    // partial sums | result (2 doubles) | partial counts
    sf::DevMem<double> buf;
    if (buf.alloc((size_t)(nb + 2) + (size_t)(nb + 1) / 2)) return SF_ERR_HIP;
    int32_t* neg = (int32_t*)(buf + nb + 2);
    double res[2] = {0.0, 0.0};
    sf::launch_lu_logdet((int64_t)p->n, p->d_Lsx + p->xC, sf::sel_struct(p), buf, neg, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(res, buf + nb, 2 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    *logabs = res[0];
    if (sign) {
        int sg = res[1] != 0.0 ? -1 : 1;
        if (p->piv_tol > 0.0) {         // the row interchanges of the factorization: P A = L U
            std::vector<sf_long> pivpos((size_t)p->n);
            const int rc = sf_lu_plan_get_pivots(p, pivpos.data());
            if (rc) return rc;
            sg *= permutation_sign(pivpos);
        }
        *sign = sg;
    }
    return SF_OK;
}

}  // extern "C"
