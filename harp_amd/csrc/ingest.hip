// What a fitting job is FED with (utils/data_util.py:11-51 load_img / ImagesDataset.__getitem__): the decoded uint8 frames and masks become
// the three float32 targets FitEngine.set_targets keeps resident, on the device, bit for bit what the host path computes.
//
// harp_targets_from_u8: rgb (N,H0,W0,3), mask (N,H0,W0) uint8 -> y_true (N,H,W,3), y_sil (N,H,W), y_sil_col (N,H,W) float32 with
//   H = ceil(H0 / d), W = ceil(W0 / d); output pixel (y, x) reads source pixel (y d, x d) (`img[::d, ::d]`, taken BEFORE the erosion).
//   y_true, y_sil = float(u) / 255.0f with the correctly rounded float32 division: equal to float32(float64(u) / 255.0) for all 256 codes
//   (a multiply by float32(1 / 255) is not).  y_sil_col = the same conversion of the minimum of the SUBSAMPLED mask over the 5 x 5 window
//   clipped to the H x W image: two passes of the 3 x 3 erosion with out-of-image neighbours ignored (cv2.erode's default border), taken
//   on the codes since the minimum commutes with the monotone conversion.
// Design: one workgroup of 256 threads = a tile of 16 rows x 64 columns of one frame; one lane = 4 neighbouring pixels of
//   one row.  The subsampled mask tile with a halo of 2 is staged as bytes in LDS (20 x 68; positions outside the image hold 255, the
//   identity of the minimum), a horizontal 5-minimum goes into a second LDS array (20 x 64), a barrier, then the vertical 5-minimum.
//   A lane's 12 source bytes come as three 32-bit loads and its 48 + 16 + 16 output bytes leave as 128-bit stores where the addresses
//   allow, as bytes / dwords otherwise (decided per lane from the address: the alignment of a row depends on W0, d and the frame).
//   No atomics, no scratch, no allocation: enqueue-only on the caller's stream.
#include "harp_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kTH = 16, kTW = 64, kHalo = 2;
constexpr int kSW = (kTW + 2 * kHalo) / 4;      // 17 words = 68 bytes per staged row
constexpr int kSH = kTH + 2 * kHalo;            // 20 staged rows
constexpr int kGW = kTW / 4;                    // 16 groups of 4 pixels per tile row

struct IngestArgs {
  const unsigned char* rgb; const unsigned char* mask;
  float* y_true; float* y_sil; float* y_col;
  int H0, W0, d, H, W, tiles_x, tiles_y;
};

__device__ __forceinline__ float unit(unsigned u) { return __fdiv_rn((float)u, 255.0f); }
__device__ __forceinline__ unsigned byte_of(unsigned w, int k) { return (w >> (8 * k)) & 255u; }
__device__ __forceinline__ unsigned min_u8x4(unsigned a, unsigned b) {                      // per-byte minimum of two packed words
  unsigned o = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) o |= min(byte_of(a, k), byte_of(b, k)) << (8 * k);
  return o;
}

// `cnt` (1..4) bytes at p, p + step, ... packed into one word (the others 0)
__device__ __forceinline__ unsigned load_u8x4(const unsigned char* p, int step, int cnt) {
  if (step == 1 && cnt == 4 && ((uintptr_t)p & 3) == 0) return *(const unsigned*)p;
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < cnt) v |= (unsigned)p[(size_t)k * step] << (8 * k);
  return v;
}

// the `cnt` (1..4) leading bytes of `w`, converted, to o[0..cnt)
__device__ __forceinline__ void store_unit4(float* o, unsigned w, int cnt) {
  if (cnt == 4 && ((uintptr_t)o & 15) == 0) {
    *(float4*)o = make_float4(unit(byte_of(w, 0)), unit(byte_of(w, 1)), unit(byte_of(w, 2)), unit(byte_of(w, 3)));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) o[k] = unit(byte_of(w, k));
  }
}

template <bool ERODE>
__global__ void __launch_bounds__(256) targets_from_u8_kernel(IngestArgs A) {
  __shared__ unsigned s0[ERODE ? kSH * kSW : 1];      // the mask tile and its halo, 4 codes per word
  __shared__ unsigned s1[ERODE ? kSH * kGW : 1];      // its horizontal 5-minimum
  const int t = threadIdx.x;
  const int tpf = A.tiles_x * A.tiles_y;              // tiles per frame
  const int n = (int)(blockIdx.x / (unsigned)tpf), rem = (int)blockIdx.x - n * tpf;
  const int tyi = rem / A.tiles_x, txi = rem - tyi * A.tiles_x;
  const int x0t = txi * kTW, y0t = tyi * kTH;
  const size_t frame0 = (size_t)n * A.H0 * A.W0;      // the frame's first source pixel
  const unsigned char* mk = A.mask + frame0;
  if (ERODE) {
    unsigned char* sb = (unsigned char*)s0;
    for (int i = t; i < kSH * kSW * 4; i += 256) {
      const int row = i / (kSW * 4), col = i - row * (kSW * 4);
      const int gy = y0t + row - kHalo, gx = x0t + col - kHalo;
      unsigned char v = 255;
      if (gy >= 0 && gy < A.H && gx >= 0 && gx < A.W) v = mk[(size_t)gy * A.d * A.W0 + (size_t)gx * A.d];
      sb[i] = v;
    }
    __syncthreads();
    for (int i = t; i < kSH * kGW; i += 256) {        // word g of a staged row holds the columns 4 g - 2 .. 4 g + 1 of the tile
      const int row = i / kGW, g = i - row * kGW;
      const unsigned w0 = s0[row * kSW + g], w1 = s0[row * kSW + g + 1];
      unsigned b[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) { b[k] = byte_of(w0, k); b[4 + k] = byte_of(w1, k); }
      unsigned o = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) o |= min(min(min(b[j], b[j + 1]), min(b[j + 2], b[j + 3])), b[j + 4]) << (8 * j);
      s1[i] = o;
    }
    __syncthreads();
  }
  const int r = t / kGW, g = t - r * kGW;
  const int y = y0t + r, x = x0t + 4 * g;
  if (y >= A.H || x >= A.W) return;                   // (behind the last barrier)
  const int cnt = min(4, A.W - x);
  const size_t src = frame0 + (size_t)y * A.d * A.W0 + (size_t)x * A.d, dst = ((size_t)n * A.H + y) * A.W + x;

  unsigned m4;
  if (ERODE) {
    const unsigned w0 = s0[(r + kHalo) * kSW + g], w1 = s0[(r + kHalo) * kSW + g + 1];
    m4 = (w0 >> 16) | (w1 << 16);
    unsigned e4 = s1[r * kGW + g];
#pragma unroll
    for (int k = 1; k < 5; ++k) e4 = min_u8x4(e4, s1[(r + k) * kGW + g]);
    store_unit4(A.y_col + dst, e4, cnt);
  } else {
    m4 = load_u8x4(mk + (src - frame0), A.d, cnt);
  }
  store_unit4(A.y_sil + dst, m4, cnt);

  const unsigned char* ps = A.rgb + src * 3;
  unsigned c[3] = {0u, 0u, 0u};                       // the lane's 12 colour bytes
  if (A.d == 1 && cnt == 4 && ((uintptr_t)ps & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ((const unsigned*)ps)[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) {
        const unsigned char* p = ps + (size_t)k * A.d * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) c[(3 * k + j) >> 2] |= (unsigned)p[j] << (8 * ((3 * k + j) & 3));
      }
  }
  float* po = A.y_true + dst * 3;
  if (cnt == 4 && ((uintptr_t)po & 15) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      ((float4*)po)[k] = make_float4(unit(byte_of(c[k], 0)), unit(byte_of(c[k], 1)), unit(byte_of(c[k], 2)), unit(byte_of(c[k], 3)));
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < 3 * cnt) po[k] = unit(byte_of(c[k >> 2], k & 3));
  }
}

}  // namespace

extern "C" int harp_targets_from_u8(const unsigned char* rgb, const unsigned char* mask, int N, int H0, int W0, int d, float* y_true, float* y_sil,
                                    float* y_sil_col, hipStream_t stream) {
  if (!rgb || !mask || !y_true || !y_sil || N <= 0 || H0 <= 0 || W0 <= 0 || d < 1 || d > 8) return HARP_ERR_ARG;
  IngestArgs A;
  A.rgb = rgb; A.mask = mask; A.y_true = y_true; A.y_sil = y_sil; A.y_col = y_sil_col;
  A.H0 = H0; A.W0 = W0; A.d = d;
  A.H = (H0 - 1) / d + 1; A.W = (W0 - 1) / d + 1;
  A.tiles_x = (A.W - 1) / kTW + 1; A.tiles_y = (A.H - 1) / kTH + 1;
  const long long tiles = (long long)A.tiles_x * A.tiles_y;
  // the 1-D grid and the kernel's int tile arithmetic; a tile reads at most 64 * 1024 source pixels (d = 8), so with this bound the
  // largest tensor holds fewer than 3 * 2^47 elements and every size_t offset in the kernel is far from wrapping
  if (tiles > 0x7fffffffLL / N) return HARP_ERR_ARG;
  const dim3 grid((unsigned)(tiles * N)), block(256);
  if (y_sil_col) hipLaunchKernelGGL(targets_from_u8_kernel<true>, grid, block, 0, stream, A);
  else hipLaunchKernelGGL(targets_from_u8_kernel<false>, grid, block, 0, stream, A);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
