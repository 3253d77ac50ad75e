// What a fit is WATCHED with while it runs (optimize_sequence.py:37-64 show_img_pair, :97-171 visualize_val, :490-501): one launch writes
// one finished uint8 contact sheet of up to rows x cols frames, so only the sheet crosses to the host.
//
// harp_sheet_u8: frames (N,H,W[,C]) float32, read in place through their strides -> out (rows * ch, cols * cw, 3) uint8 with
//   ch = ceil(H / d), cw = ceil(W / d); cell k = r * cols + c shows frame k, cells k >= N are white (an empty axis of the reference's
//   white figure).  Per source pixel a colour p in float32 (the four modes below), per output pixel the box average of p over its
//   d x d source box (clipped at the image's edge): summed by ONE lane in row-major order from 0.0f, divided by the number of pixels
//   summed (IEEE float32 division), then uint8(trunc(v * 255.0f)) — with d = 1 exactly harp_panels_u8's colour convention.
// Design: one lane = 4 neighbouring pixels of one SHEET row = 12 output bytes, as in panels_u8_kernel; the four pixels
//   may straddle two cells (cw need not be a multiple of 4), so the cell is looked up per pixel.  When the sheet's width is a multiple
//   of 4 every lane's 12 bytes are 4-byte aligned and leave as three 32-bit stores, otherwise as byte stores.  No LDS, no atomics.
#include "harp_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct SheetArgs {
  const float* a; const float* b; const float* m;
  long long an, ay, ax, ac, bn, by, bx, bc, mn, my, mx;
  int mode, N, H, W, rows, cols, d, ch, cw;
  unsigned char* out;
};

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }      // NaN -> 0

// the colour of source pixel (y, x) of frame n, each operation rounded on its own (no fma contraction)
template <int MODE>
__device__ __forceinline__ void source_colour(const SheetArgs& A, int n, int y, int x, float& p0, float& p1, float& p2) {
  const float* s = A.a + n * A.an + y * A.ay + x * A.ax;
  if (MODE == 0) {                                   // imshow of a float image clips to [0, 1] (:54, :156)
    p0 = clip01(s[0]); p1 = clip01(s[A.ac]); p2 = clip01(s[2 * A.ac]);
  } else if (MODE == 1) {                            // overlay[..., 0] = true mask, overlay[..., 2] = predicted mask (:48-52)
    p0 = clip01(s[0]); p1 = 0.f; p2 = clip01(A.b[n * A.bn + y * A.by + x * A.bx]);
  } else if (MODE == 2) {                            // |y_true * m - y_pred * m| (:499)
    const float* t = A.b + n * A.bn + y * A.by + x * A.bx;
    const float m = A.m[n * A.mn + y * A.my + x * A.mx];
    p0 = clip01(fabsf(__fsub_rn(__fmul_rn(s[0], m), __fmul_rn(t[0], m))));
    p1 = clip01(fabsf(__fsub_rn(__fmul_rn(s[A.ac], m), __fmul_rn(t[A.bc], m))));
    p2 = clip01(fabsf(__fsub_rn(__fmul_rn(s[2 * A.ac], m), __fmul_rn(t[2 * A.bc], m))));
  } else {                                           // F.normalize(dim=-1) * 0.5 + 0.5 (:166-167)
    const float v0 = s[0], v1 = s[A.ac], v2 = s[2 * A.ac];
    const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(v0, v0), __fmul_rn(v1, v1)), __fmul_rn(v2, v2)));
    const float den = fmaxf(nrm, 1e-12f);
    p0 = clip01(__fadd_rn(__fmul_rn(__fdiv_rn(v0, den), 0.5f), 0.5f));
    p1 = clip01(__fadd_rn(__fmul_rn(__fdiv_rn(v1, den), 0.5f), 0.5f));
    p2 = clip01(__fadd_rn(__fmul_rn(__fdiv_rn(v2, den), 0.5f), 0.5f));
  }
}

__device__ __forceinline__ unsigned level_u8(float v) { return (unsigned)(int)__fmul_rn(v, 255.f); }

// one lane = 4 neighbouring pixels of one sheet row
template <int MODE>
__global__ void __launch_bounds__(256) sheet_u8_kernel(SheetArgs A) {
  const int SW = A.cols * A.cw, SH = A.rows * A.ch;                 // the sheet's width and height in pixels
  const int gpr = (SW + 3) / 4;                                     // groups per sheet row
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)SH * gpr) return;
  const int Y = (int)(i / gpr), X0 = 4 * (int)(i % gpr);
  const int r = Y / A.ch, ci = Y - r * A.ch;                        // cell row, output row inside the cell
  const int y0 = ci * A.d, y1 = min(A.H, y0 + A.d);
  unsigned v[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned c0 = 255u, c1 = 255u, c2 = 255u;                       // an empty cell: white
    const int X = X0 + k;
    if (X < SW) {
      const int c = X / A.cw, cj = X - c * A.cw;
      const int n = r * A.cols + c;
      if (n < A.N) {
        const int x0 = cj * A.d, x1 = min(A.W, x0 + A.d);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int y = y0; y < y1; ++y)
          for (int x = x0; x < x1; ++x) {
            float p0, p1, p2;
            source_colour<MODE>(A, n, y, x, p0, p1, p2);
            s0 = __fadd_rn(s0, p0); s1 = __fadd_rn(s1, p1); s2 = __fadd_rn(s2, p2);
          }
        const float cnt = (float)((y1 - y0) * (x1 - x0));
        c0 = level_u8(__fdiv_rn(s0, cnt)); c1 = level_u8(__fdiv_rn(s1, cnt)); c2 = level_u8(__fdiv_rn(s2, cnt));
      }
    }
    v[3 * k] = c0; v[3 * k + 1] = c1; v[3 * k + 2] = c2;
  }
  unsigned char* o = A.out + ((size_t)Y * SW + X0) * 3;
  if ((SW & 3) == 0) {
    unsigned* o4 = (unsigned*)o;
#pragma unroll
    for (int k = 0; k < 3; ++k) o4[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
  } else {
    const int nb = 3 * min(4, SW - X0);
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < nb) o[k] = (unsigned char)v[k];
  }
}

}  // namespace

extern "C" int harp_sheet_u8(int mode, const float* a, const long long* a_strides, const float* b, const long long* b_strides, const float* mask,
                             const long long* mask_strides, int N, int H, int W, int rows, int cols, int d, unsigned char* out,
                             hipStream_t stream) {
  if (mode < 0 || mode > 3 || !a || !a_strides || !out || N <= 0 || H <= 0 || W <= 0 || rows <= 0 || cols <= 0 || d < 1 || d > 8) return HARP_ERR_ARG;
  if ((long long)rows * cols > 64 || N > rows * cols) return HARP_ERR_ARG;
  const bool two = mode == 1 || mode == 2;
  if (two != (b != nullptr) || (b && !b_strides) || (mode == 2) != (mask != nullptr) || (mask && !mask_strides)) return HARP_ERR_ARG;
  SheetArgs A;
  A.a = a; A.b = b; A.m = mask;
  A.an = a_strides[0]; A.ay = a_strides[1]; A.ax = a_strides[2]; A.ac = a_strides[3];
  A.bn = A.by = A.bx = A.bc = A.mn = A.my = A.mx = 0;
  if (b) { A.bn = b_strides[0]; A.by = b_strides[1]; A.bx = b_strides[2]; A.bc = b_strides[3]; }
  if (mask) { A.mn = mask_strides[0]; A.my = mask_strides[1]; A.mx = mask_strides[2]; }
  if (A.an < 0 || A.ay < 0 || A.ax < 0 || A.ac < 0 || A.bn < 0 || A.by < 0 || A.bx < 0 || A.bc < 0 || A.mn < 0 || A.my < 0 || A.mx < 0)
    return HARP_ERR_ARG;
  A.mode = mode; A.N = N; A.H = H; A.W = W; A.rows = rows; A.cols = cols; A.d = d;
  A.ch = (H + d - 1) / d; A.cw = (W + d - 1) / d;
  A.out = out;
  const long long SW = (long long)cols * A.cw, SH = (long long)rows * A.ch;
  if (SW > 0x7fffffffLL || SH > 0x7fffffffLL) return HARP_ERR_ARG;
  const long long blocks = (SH * ((SW + 3) / 4) + 255) / 256;
  if (blocks > 0x7fffffffLL) return HARP_ERR_ARG;
  const dim3 grid((unsigned)blocks), block(256);
  switch (mode) {
    case 0: hipLaunchKernelGGL(sheet_u8_kernel<0>, grid, block, 0, stream, A); break;
    case 1: hipLaunchKernelGGL(sheet_u8_kernel<1>, grid, block, 0, stream, A); break;
    case 2: hipLaunchKernelGGL(sheet_u8_kernel<2>, grid, block, 0, stream, A); break;
    default: hipLaunchKernelGGL(sheet_u8_kernel<3>, grid, block, 0, stream, A); break;
  }
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
