// The matrix-core Gram block of the two vertex fits (vertex_fit.hip; arm_vertex_fit.hip, §28; §31): J^T W J of a tile of
// 192 rows x 64 columns in LDS by v_mfma_f32_32x32x2_f32 (exact float32).  A workgroup of four waves; every wave takes 48 rows of the
// tile (its K slice) into three 32 x 32 accumulators — blocks (0,0), (1,0), (1,1) of the 64 x 64 product: the lower triangle is all the
// Cholesky reads — that live in registers across the tiles and meet in LDS at the end, wave after wave (fixed order).  The accumulation
// is here; the write-out of the blocks stays in the two files (shared, it costs arm_vertex_fit.hip three registers: DESIGN.md §31).
// Plain `inline`: the optimiser inlines it in its own pass, and no call remains in either code object.
#pragma once
#include "harp_common.h"

namespace lm {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// this wave's 48 rows of the tile J (row k weighted by wt[k / 3]) into the three accumulators
template <int LD>
__device__ inline void gram_accumulate(const float (*J)[LD], const float* wt, int wave, int lane, f32x16& acc00, f32x16& acc10,
                                       f32x16& acc11) {
  const int col = lane & 31, kh = lane >> 5;
#pragma unroll 4
  for (int kk = 0; kk < 24; ++kk) {
    const int k = 48 * wave + 2 * kk + kh;
    const float wk = wt[k / 3], j0 = J[k][col], j1 = J[k][32 + col];
    const float a0 = j0 * wk, a1 = j1 * wk;
    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, j0, acc00, 0, 0, 0);
    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, j0, acc10, 0, 0, 0);
    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, j1, acc11, 0, 0, 0);
  }
}

}  // namespace lm
