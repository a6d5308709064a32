// The row walk of the Gram reductions, shared by sf_gram.hip (Y^T Y) and sf_gram_lu.hip (Z^T Y).
#pragma once
#include "sf_kernels.h"
#include "sf_wave.h"

namespace sf {

// A workgroup of GRAM_WAVES waves walks its slab in stretches of GRAM_STRETCH rows: in a stretch, wave w takes the four-row groups
// w, w + GRAM_WAVES, ..., one per accumulator -- GRAM_ACC independent MFMA chains per wave cover the instruction's latency.
constexpr int GRAM_WAVES = 4;
constexpr int GRAM_ACC = 4;
constexpr int GRAM_STRETCH = 4 * GRAM_WAVES * GRAM_ACC;     // 64 rows
constexpr int GRAM_TILE = SVM_W * SVM_W;                    // doubles of a part

// acc[u] += (rows r + 16 u + [0, 4) of Ya)^T (the same rows of Yb) for the stretches of [r0, r1) (r1 <= n), this wave's groups.
// Lane l holds element (row l >> 4, column l & 15) of a group: the doubles [16 r, 16 r + 64) of a block, one coalesced 512-byte
// run per operand (SAME: one run, both operands).  Rows >= r1 supply 0; their (clamped) address is the block's first double.
//   A operand (row index of D) <- Ya,  B operand (column index of D) <- Yb,  D[i = (l >> 4) + 4 reg][j = l & 15]   (as k_gemm)
template <bool SAME>
__device__ __forceinline__ void gram_rows(const double* __restrict__ Ya, const double* __restrict__ Yb, int64_t r0, int64_t r1, int wave,
                                          int lane, double4_t (&acc)[GRAM_ACC]) {
    const int fk = lane >> 4;
    for (int64_t r = r0 + 4 * wave; r < r1; r += GRAM_STRETCH) {
        double va[GRAM_ACC], vb[GRAM_ACC];
#pragma unroll
        for (int u = 0; u < GRAM_ACC; ++u) {
            const int64_t g = r + 4 * GRAM_WAVES * u;
            const bool ok = g + fk < r1;
            const int64_t idx = ok ? g * SVM_W + lane : 0;
            const double a = Ya[idx];
            va[u] = ok ? a : 0.0;
            if (!SAME) {
                const double b = Yb[idx];
                vb[u] = ok ? b : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < GRAM_ACC; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[u], SAME ? va[u] : vb[u], acc[u], 0, 0, 0);
    }
}

}  // namespace sf
