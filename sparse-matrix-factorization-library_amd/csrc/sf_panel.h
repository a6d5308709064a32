// One-wave panel arithmetic of the 64 x 64 block factorizations (gfx950), shared by the stand-alone block kernels k_potrf_block /
// k_getrf_block (sf_kernels.hip) and by the fused step k_step (sf_step.hip): lane r keeps row r of the panel in registers.
#pragma once
#include "sf_wave.h"

namespace sf {

// 1 / sqrt(v) and 1 / v to full fp64 accuracy from the hardware's 24-bit approximations (v_rsq_f64, v_rcp_f64: 5e-8 relative) and ONE
// third-order step --  r (1 + e/2 + 3 e^2 / 8), e = 1 - v r^2;  c (1 + e + e^2), e = 1 - v c  -- instead of two Newton steps: one
// dependent operation less on the sequential chains of the panel factorizations (5 instead of 6, 3 instead of 4) AND closer to the
// correctly rounded value: 1.24 / 1.00 ulp worst case over 4 M arguments against 2.18 / 1.69 (tools/experiments/rsq_accuracy.hip).
__device__ __forceinline__ double rsqrt_full(double v) {
    const double r = __builtin_amdgcn_rsq(v);
    const double e = __builtin_fma(-(v * r), r, 1.0);
    return __builtin_fma(r, e * __builtin_fma(e, 0.375, 0.5), r);
}
__device__ __forceinline__ double rcp_full(double v) {
    const double c = __builtin_amdgcn_rcp(v);
    const double e = __builtin_fma(-v, c, 1.0);
    return __builtin_fma(c, __builtin_fma(e, e, e), c);
}

// ---------------------------------------------------------------------------------------------------
// LU of a b x b (b <= 64) diagonal block in ONE wavefront, lane r holds row r (a[c] = D(r,c), identity padding), the same
// register scheme as k_potrf_block.  Without pivoting this is the reference's magma_dgetrf_nopiv (LU/Source/SparseFrame.c:2653)
// / cusolverDnDgetrf with devIpiv = NULL (:3344).  With pivoting (PivotCtl, sf_kernels.h) the interchanges are IMPLICIT: rows
// never move between lanes; at column j a pivot lane p is chosen among the lanes not used yet, its row is broadcast with
// v_readlane (p is wave-uniform), and the lane remembers the position it was given.  The permutation is applied when the
// rows are stored.  RCP: multipliers by v_rcp_f64 + two Newton steps (k_step's variant) instead of the IEEE division.
// Returns this lane's final position; bad: a zero / NaN pivot was met and not perturbed.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double readlane_dyn_f64(double v, int l) {      // l wave-uniform, not a compile-time constant
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// W columns J0 .. J0 + W - 1 of the block (a[u] = D(lane, J0 + u)); `active` / `pos` carry the state of the lanes across the panels
// of a blocked factorization (k_step<true>), piv_rows[J] receives the row chosen at column J.  W = NB, J0 = 0 is the whole block.
template <bool RCP, int W>
__device__ __forceinline__ void getrf_panel_wave(double (&a)[W], int lane, int J0, int b, double tol, double eps, bool& bad, int& nperturbed,
                                                 int& pos, bool& active, int* piv_rows) {
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int J = J0 + j;
        int p = J;
        if (tol > 0.0 && J < b) {               // wave-uniform: no pivot search when pivoting is off or in the padding
            // The natural row keeps the pivot iff it is still free, non-zero, and NO free row has tol * |a_ij| > |a_jj| -- one
            // multiply, one compare and a ballot; no reduction.  (fl(tol * x) is monotonic in x, so this IS |a_jj| >= tol * max:
            // the decision of the reduction it replaces, which cost 2 us per 16-column panel.)  A NaN counts as larger.  Only when
            // the natural row fails is the arg-max looked for (two 32-bit DPP reductions and a ballot).
            const double nat = readlane_dyn_f64(a[j], J);
            const unsigned long long act = __ballot(active);
            const bool nat_free = ((act >> J) & 1ull) != 0;
            const double anat = fabs(nat);
            const unsigned long long larger = __ballot(active && !(tol * fabs(a[j]) <= anat));
            if (!(nat_free && larger == 0ull && nat != 0.0)) {
                double m;
                const int pm = wave_argmax_abs(a[j], active, &m);
                if (!(nat_free && fabs(nat) >= tol * m && nat != 0.0) && pm >= 0) p = pm;
            }
            p = __builtin_amdgcn_readfirstlane(p);
        }
        double piv = readlane_dyn_f64(a[j], p);
        if (J < b && eps > 0.0 && !(fabs(piv) >= eps) && piv == piv) {      // tiny (or zero) pivot: perturb
            piv = (piv < 0.0) ? -eps : eps;
            ++nperturbed;
            if (lane == p) a[j] = piv;
        }
        bad = bad || !(fabs(piv) > 0.0);        // zero or NaN pivot (NaN != 0.0 is true); padded rows have piv = 1
        const bool elim = active && lane != p;
        double l;
        if (RCP) {
            const double rp = rcp_full(piv);
            l = elim ? a[j] * rp : 0.0;
        } else {
            l = elim ? a[j] / piv : 0.0;
        }
        if (elim) a[j] = l;
        if (lane == p) { pos = J; active = false; }
        if (piv_rows != nullptr && lane == 0) piv_rows[J] = p;
#pragma unroll
        for (int c = j + 1; c < W; ++c) a[c] -= l * readlane_dyn_f64(a[c], p);
    }
}

// NATURAL-PIVOT FAST PATH of getrf_panel_wave (k_step<true>): the same W columns eliminated with the natural rows as pivots -- the
// arithmetic of the general path when every natural pivot passes, instruction for instruction (same reciprocal, same fused
// multiply-adds: bit-identical results) -- as STRAIGHT-LINE code: the threshold test of column j (does a free row have
// tol * |a_ij| > |a_jj|?  is the pivot zero, NaN, or below the perturbation threshold?) only accumulates into a wave-uniform mask
// instead of steering a branch, so nothing on the column's critical path waits for a vector compare to reach the scalar unit and
// the compiler schedules the 16 columns as one block (the general form's per-column branches cost it a copy of all 16 registers per
// column and 48 spilled SGPRs; profiles/r03_k_step_stamps.txt: 5.9 us per 16-column panel against 2.4 us for Cholesky's).
// Valid while every earlier pivot of the block was natural too (lanes < J0 used, lanes >= J0 free).  Returns false when some
// natural pivot does NOT pass: the caller then reloads the panel and runs getrf_panel_wave on it (a[] is garbage in that case).
template <int W>
__device__ __forceinline__ bool getrf_panel_natural(double (&a)[W], int lane, int J0, int b, double tol, double eps) {
    unsigned long long viol = 0ull;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        const int J = J0 + j;
        const double piv = readlane_dyn_f64(a[j], J);
        const bool below = lane > J;
        viol |= __ballot(below && !(tol * fabs(a[j]) <= fabs(piv)));            // a NaN entry counts as larger
        if (J < b && (!(fabs(piv) >= eps) || piv == 0.0)) viol |= 1ull;           // zero, NaN or tiny pivot (wave-uniform test)
        const double rp = rcp_full(piv);
        const double l = below ? a[j] * rp : 0.0;
        if (below) a[j] = l;
#pragma unroll
        for (int c = j + 1; c < W; ++c) a[c] -= l * readlane_dyn_f64(a[c], J);
    }
    return viol == 0ull;
}
}  // namespace sf
