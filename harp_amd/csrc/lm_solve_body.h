// The solve of one Levenberg-Marquardt step of the five batched pose solvers (ik.hip, reproj_ik.hip, arm_ik.hip, vertex_fit.hip,
// arm_vertex_fit.hip): Jacobi scaling, the Cholesky factor of the scaled and damped normal matrix in place in LDS, both
// triangular solves and the damping update.  One wave solves, lane i = row i = unknown i; NX <= 64 unknowns, LD the (odd) row stride.
// All five take jacobi_scale and damped from here; the two vertex fits also solve(), while the three one-wave kernels carry solve()'s
// loops written out, because each measured slower through the call (§31): a change to solve() is repeated in those three.
//
//   scaling    s_i = 1 / sqrt(A_ii (1 + lambda)): S = s (A + lambda diag A) s has a unit diagonal
//   Cholesky   left-looking, in place over A's lower triangle, column by column (a dot of length j per lane, the pivot by a lane
//              broadcast); a non-positive or non-finite pivot marks the step rejected.  ONE workgroup barrier per column, which every
//              thread of the workgroup meets whether its wave works or not.
//   solves     L y = b and L^T z = y in registers with lane broadcasts, L read from LDS; the step is x' = x + s z.
// Every sum runs in a fixed order: a repeated call gives the same bits.
#pragma once
#include "harp_common.h"

#include <math.h>

namespace lm {

// for (i = 0; i < n; ++i) f(i) under `#pragma unroll U` (the loop shapes of the five kernels differ, each as measured).  U = 0: no hint,
// the compiler decides; U = 1: `#pragma unroll 1`, which FORBIDS unrolling and so is not the same as 0; U > 1: unroll by U.
template <int U, class F>
__device__ __forceinline__ void hinted_for(int n, F f) {
  if constexpr (U == 0) {
    for (int i = 0; i < n; ++i) f(i);
  } else {
#pragma unroll U
    for (int i = 0; i < n; ++i) f(i);
  }
}

// This lane's Jacobi scale; ok: every row's diagonal is positive and its scale finite (the verdict of the calling wave).
template <int NX>
__device__ __forceinline__ float jacobi_scale(int l, float diag, float lambda, bool& ok) {
  const float s = 1.0f / sqrtf(diag * (1.0f + lambda));
  ok = __all(l >= NX || (diag > 0.f && isfinite(s)));
  return s;
}

// z of (L L^T) z = b with L L^T = s (A + lambda diag A) s: A's lower triangle (diagonal as given: only its scale s enters) becomes L.
// l: this lane's row, s: its scale, b: its -g s; works: this wave is the one that solves (uniform over the wave; the others only meet the
// barriers); ok: cleared when a pivot is not positive and finite.  OUTER / INNER: the unroll hints of the loops over the columns / of the
// dot inside a column (0: none).  A must be visible to the wave on entry; a barrier follows the last column.
template <int NX, int LD, int OUTER, int INNER>
__device__ __forceinline__ float solve(float (*A)[LD], int l, float s, float b, bool works, bool& ok) {
  const bool row = (NX >= 64) || l < NX;                               // (this lane has a row)
  hinted_for<OUTER>(NX, [&](int j) __attribute__((always_inline)) {    // left-looking Cholesky, column j
    if (works) {
      const float sj = __shfl(s, j, 64);
      float v = 0.f;
      if (l >= j && row) {
        v = (l == j) ? 1.0f : A[l][j] * s * sj;
        hinted_for<INNER>(j, [&](int c) __attribute__((always_inline)) { v -= A[l][c] * A[j][c]; });
      }
      const float piv = __shfl(v, j, 64);
      ok = ok && (piv > 0.f) && isfinite(piv);
      const float ljj = sqrtf(piv);
      if (l >= j && row) A[l][j] = (l == j) ? ljj : v / ljj;
    }
    __syncthreads();
  });
  float z = 0.f;
  if (works) {
    float y = 0.f;
    b = row ? b : 0.f;
    hinted_for<OUTER>(NX, [&](int j) __attribute__((always_inline)) {  // L y = b
      const float yj = __shfl(b, j, 64) / A[j][j];
      if (l == j) y = yj;
      if (l > j && row) b -= A[l][j] * yj;
    });
    hinted_for<OUTER>(NX, [&](int i) __attribute__((always_inline)) {  // L^T z = y, last row first
      const int j = NX - 1 - i;
      const float zj = __shfl(y, j, 64) / A[j][j];
      if (l == j) z = zj;
      if (l < j) y -= A[j][l] * zj;
    });
  }
  return z;
}

// the damping after a step's verdict
__device__ __forceinline__ float damped(float lambda, bool accept) {
  return accept ? fmaxf(0.1f * lambda, 1e-9f) : fminf(10.0f * lambda, 1e6f);
}

}  // namespace lm
