// LPIPS v0.1, net='alex' (lpips.LPIPS(net='alex'), called at utils/eval_util.py:51-53 on every 64-frame chunk of the post-fit evaluation,
// optimize_sequence.py:737 / :795), forward only, float32.  lpips=True, spatial=False, eval mode (dropout off).
//
//   x' = (x - shift_c) / scale_c   (normalize != 0: x -> 2x - 1 first)            the scaling layer, folded into conv1's staging
//   relu1 = relu(conv1 11x11/s4/p2 (3 -> 64))                                       kernel conv_kxk_kernel<11, 4, 1, true>
//   relu2 = relu(conv2 5x5/p2 (64 -> 192)) of maxpool 3x3/s2 (floor) of relu1        maxpool3s2_kernel, conv_kxk_kernel<5, 1, 4, false>
//   relu3..5 = relu(conv 3x3/p1) 192 -> 384 -> 256 -> 256 of maxpool of relu2        maxpool3s2_kernel, harp_conv3x3 (HARP_CONV_F32) x 3
//   per tap k: f^ = f / (||f||_2 over channels + 1e-10); d = sum_c lin_k[c] (f^_ref - f^_pred)^2; mean over H_k x W_k;  LPIPS = sum of taps
//                                                                                    lpips_head_kernel (per tap), lpips_finish_kernel
// ref and pred go through the stack together as a batch of 2N images (ref first).  Activations are NHWC float32.
//
// conv_kxk_kernel: implicit GEMM on v_mfma_f32_32x32x2_f32 (M = output pixels, N = output channels, K = taps x input channels), so each
// output is a float32 fma chain.  A workgroup (4 waves) owns a 16x16-pixel x 64-channel output tile; a wave holds rows 4 wv .. 4 wv + 3 as
// two 32-pixel row blocks (columns 0-7 and 8-15) x two 32-channel column blocks.  The K loop runs over (channel chunk, filter row ky): a step
// stages the 16 input rows that filter row ky reads for the tile's 16 output rows (16 x PC columns x 4 Q channels) and the filter row's
// slab (KSP taps x 4 Q channels x 64 output channels) in LDS; the next step's global loads are in flight under the current step's MFMAs.
//   conv1: 3 channels staged as (r, g, b, 0) quads; the two k halves of the MFMA take two neighbouring taps kx = 2s, 2s + 1 (12 tap slots,
//     slot 11 is zero), three MFMAs per pair (the fourth channel is never multiplied): K = 363 padded to 366.  LDS: the input rows are
//     stored phase-split (column c at (c % 4) * 18 + c / 4) so that the 8 lanes of an A-fragment row, 4 columns apart in the image, read
//     8 consecutive 16-B slots.  16 rows x 72 columns x 16 B + 12 x 64 x 16 B = 30 KiB.
//   conv2: 16 channels per chunk as four quads, the k halves take quads 2g, 2g + 1 (as harp_conv3x3).  16 x 24 x 4 x 16 B + 5 x 4 x 64 x 16 B
//     = 45 KiB.
//   Row pitches are 8 mod 16 slots: the two image rows a 16-lane group of ds_read_b128 touches fall on disjoint banks.
// lpips_head_kernel: one wave per pixel (lanes over channels, up to 6 per lane), 16 pixels per wave, 64 per workgroup; the workgroup writes
// its own partial sum (no atomics), the finish kernel adds the partials in a fixed order in float64.  Two calls are bit-identical;
// identical ref and pred give exactly 0.
#include <math.h>
#include "harp_common.h"
#include "harp_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kT = 16;                       // output tile side
constexpr int kCN = 64;                      // output channels per workgroup
constexpr int kMinSide = 31;                 // the second pool needs a 3-pixel input
constexpr int kTaps = 5;
constexpr int kTapC[kTaps] = {64, 192, 384, 256, 256};
constexpr int kHeadPix = 16;                 // pixels per wave in the head
constexpr int kHeadTile = 4 * kHeadPix;      // pixels per head workgroup

template <int KS, int S, int Q, bool FIRST>
struct Cfg {
  static constexpr int kKSP = FIRST ? KS + 1 : KS;                 // tap slots per filter row (conv1: an even count, pairs over the k halves)
  static constexpr int kPC = (kT - 1) * S + kKSP;                  // staged input columns
  static constexpr int kPhase = kPC / S;                           // columns per phase (column c at (c % S) * kPhase + c / S)
  static constexpr int kRP = kPC + (8 - kPC % 16 + 16) % 16;       // row pitch in 16-B slots, 8 mod 16
  static constexpr int kIn4 = Q * kT * kRP;                        // float4 of the staged input
  static constexpr int kW4 = kKSP * Q * kCN;                       // float4 of a filter-row slab
  static constexpr int kInUnits = (kT * kPC * Q + 255) / 256;      // staging units per thread
  static constexpr int kWUnits = (kW4 + 255) / 256;
  static_assert(kPC % S == 0, "phase split");
  static_assert(kRP % 16 == 8, "row pitch");
};

struct ConvArgs {
  const float* in;                           // FIRST: ref (images 0..N-1) / pred (N..2N-1) through strides; else (B,H,W,Cin) NHWC
  const float* in2;
  long long sn, sc, sy, sx;
  int N;                                     // FIRST: images per input
  int B, H, W, Cin, Ho, Wo, Cout, pad;
  const float4* filters;                     // pack_kxk_kernel layout
  const float* bias;
  float* out;                                // (B,Ho,Wo,Cout)
  int tiles_x, tiles_y;
  int normalize;
};

__constant__ float kShift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float kScale[3] = {0.458f, 0.448f, 0.450f};

template <int KS, int S, int Q, bool FIRST>
__global__ __launch_bounds__(256, 2) void conv_kxk_kernel(const ConvArgs a) {
  using C = Cfg<KS, S, Q, FIRST>;
  __shared__ float4 smem[C::kIn4 + C::kW4];                      // one LDS object: input rows, then the filter slab
  float4* s_in = smem;
  float4* s_w = smem + C::kIn4;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, half = lane >> 5, m = lane & 31;
  const int ncb = a.Cout / kCN;
  int id = blockIdx.x;
  const int cb = id % ncb; id /= ncb;
  const int tx = id % a.tiles_x; id /= a.tiles_x;
  const int ty = id % a.tiles_y;
  const int b = id / a.tiles_y;
  const int y0 = ty * kT, x0 = tx * kT;
  const int H = a.H, W = a.W;
  const int nchunk = FIRST ? 1 : a.Cin / (4 * Q);
  const int nsteps = nchunk * KS;

  const float* __restrict__ src = nullptr;
  if (FIRST) src = (b < a.N ? a.in : a.in2) + (long long)(b < a.N ? b : b - a.N) * a.sn;
  else src = a.in + (size_t)b * H * W * a.Cin;
  const float4* __restrict__ wsl = a.filters + (size_t)cb * nsteps * C::kW4;

  // staging unit u: FIRST: (row u / PC, column u % PC), one pixel; else four consecutive units are one pixel's four channel quads
  int lidx[C::kInUnits], urow[C::kInUnits], ucol[C::kInUnits];
#pragma unroll
  for (int j = 0; j < C::kInUnits; ++j) {
    const int u = j * 256 + t;
    lidx[j] = -1;
    urow[j] = 0;
    ucol[j] = 0;
    if (u < kT * C::kPC * Q) {
      const int q = u % Q, pix = u / Q, r = pix / C::kPC, c = pix - r * C::kPC;
      urow[j] = r;
      ucol[j] = c;
      lidx[j] = q * kT * C::kRP + r * C::kRP + (c % S) * C::kPhase + c / S;
    }
  }
  // (named registers, not arrays: float4 arrays indexed by unrolled constants were still left in scratch, cf. DESIGN.md "A local array is
  //  not a register file")
  static_assert(C::kInUnits <= 5 && C::kWUnits <= 5, "five named staging registers");
  float4 ri0, ri1, ri2, ri3, ri4, rw0, rw1, rw2, rw3, rw4;
  unsigned rok = 0;                          // bit j: unit j lies inside the image
#define LPIPS_EACH(X) X(0, ri0, rw0) X(1, ri1, rw1) X(2, ri2, rw2) X(3, ri3, rw3) X(4, ri4, rw4)
  auto fetch = [&](int step) {
    const int cc = step / KS, ky = step - cc * KS;
    const float4* __restrict__ ws = wsl + (size_t)step * C::kW4;
    rok = 0;
#define LPIPS_FETCH(j, ri, rw)                                                                          \
    if (j < C::kInUnits) {                                                                              \
      const int iy = (y0 + urow[j]) * S + ky - a.pad, ix = x0 * S - a.pad + ucol[j];                    \
      const bool ok = lidx[j] >= 0 && iy >= 0 && iy < H && ix >= 0 && ix < W;                           \
      rok |= (unsigned)ok << j;                                                                         \
      if (FIRST) {                                                                                      \
        const long long off = ok ? (long long)iy * a.sy + (long long)ix * a.sx : 0;                     \
        ri = make_float4(src[off], src[off + a.sc], src[off + 2 * a.sc], 0.f);                          \
      } else {                                                                                          \
        const int q = (j * 256 + t) % Q;                                                                \
        ri = *(const float4*)(src + (ok ? (iy * W + ix) * a.Cin + cc * 4 * Q + 4 * q : 0));            \
      }                                                                                                 \
    }                                                                                                   \
    if (j < C::kWUnits && j * 256 + t < C::kW4) rw = ws[j * 256 + t];
    LPIPS_EACH(LPIPS_FETCH)
#undef LPIPS_FETCH
  };
  auto stage = [&]() {
#define LPIPS_STAGE(j, ri, rw)                                                                          \
    if (j < C::kInUnits && lidx[j] >= 0) {                                                              \
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                                                       \
      if ((rok >> j) & 1u) {                                                                            \
        v = ri;                                                                                         \
        if (FIRST) {   /* the scaling layer (and normalize's 2x - 1); padding stays zero in the scaled domain */ \
          if (a.normalize) v = make_float4(2.f * v.x - 1.f, 2.f * v.y - 1.f, 2.f * v.z - 1.f, 0.f);     \
          v = make_float4((v.x - kShift[0]) / kScale[0], (v.y - kShift[1]) / kScale[1], (v.z - kShift[2]) / kScale[2], 0.f); \
        }                                                                                               \
      }                                                                                                 \
      s_in[lidx[j]] = v;                                                                                \
    }                                                                                                   \
    if (j < C::kWUnits && j * 256 + t < C::kW4) s_w[j * 256 + t] = rw;
    LPIPS_EACH(LPIPS_STAGE)
#undef LPIPS_STAGE
  };
#undef LPIPS_EACH

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // this lane's A-fragment pixel in row block i: row 4 wv + dy, column 8 i + dx
  const int dy = m >> 3, dx = m & 7;
  const int rowoff = (4 * wv + dy) * C::kRP;
  fetch(0);
  for (int step = 0; step < nsteps; ++step) {
    __syncthreads();                         // every wave is done with the previous step's rows and slab
    stage();
    __syncthreads();
    if (step + 1 < nsteps) fetch(step + 1);  // in flight under this step's MFMAs
    if (FIRST) {
#pragma unroll
      for (int s = 0; s < C::kKSP / 2; ++s) {
        const int kx = 2 * s + half;
        const int ia = rowoff + (kx % S) * C::kPhase + dx + kx / S;
        const float4 a0 = s_in[ia], a1 = s_in[ia + 8];                   // (row block 1: 8 output columns = 8 S input columns, same phase)
        const float4 b0 = s_w[kx * kCN + m], b1 = s_w[kx * kCN + 32 + m];
        const float A0[3] = {a0.x, a0.y, a0.z}, A1[3] = {a1.x, a1.y, a1.z}, B0[3] = {b0.x, b0.y, b0.z}, B1[3] = {b1.x, b1.y, b1.z};
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[e], B0[e], acc[0][0], 0, 0, 0);
          acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[e], B1[e], acc[0][1], 0, 0, 0);
          acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[e], B0[e], acc[1][0], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[e], B1[e], acc[1][1], 0, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
#pragma unroll
        for (int g = 0; g < Q / 2; ++g) {
          const int quad = 2 * g + half;
          const int ia = quad * kT * C::kRP + rowoff + dx + kx;
          const float4 a0 = s_in[ia], a1 = s_in[ia + 8];
          const float4 b0 = s_w[(kx * Q + quad) * kCN + m], b1 = s_w[(kx * Q + quad) * kCN + 32 + m];
          const float A0[4] = {a0.x, a0.y, a0.z, a0.w}, A1[4] = {a1.x, a1.y, a1.z, a1.w};
          const float B0[4] = {b0.x, b0.y, b0.z, b0.w}, B1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[e], B0[e], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0[e], B1[e], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[e], B0[e], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1[e], B1[e], acc[1][1], 0, 0, 0);
          }
        }
      }
    }
  }

  // epilogue: register r of lane (half, m) in row block i / column block j is output channel 64 cb + 32 j + m of the block's pixel
  // p = 8 (r >> 2) + 4 half + (r & 3): row 4 wv + (p >> 3), column 8 i + (p & 7)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int co = cb * kCN + 32 * j + m;
    const float bias = a.bias[co];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = 8 * (r >> 2) + 4 * half + (r & 3);
        const int oy = y0 + 4 * wv + (p >> 3), ox = x0 + 8 * i + (p & 7);
        if (oy < a.Ho && ox < a.Wo) a.out[(((size_t)b * a.Ho + oy) * a.Wo + ox) * a.Cout + co] = fmaxf(acc[i][j][r] + bias, 0.f);
      }
    }
  }
}

// torch layout (Cout, Cin, KS, KS) -> slabs [Cout/64][chunk][ky][tap slot][quad][64][4]; channels and tap slots past the filter are zero
__global__ void pack_kxk_kernel(const float* __restrict__ w, int Cout, int Cin, int KS, int KSP, int Q, float* __restrict__ packed) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int nchunk = (Cin + 4 * Q - 1) / (4 * Q);
  const size_t total = (size_t)Cout * nchunk * KS * KSP * Q * 4;
  if (i >= total) return;
  size_t r = i;
  const int e = r % 4; r /= 4;
  const int col = r % kCN; r /= kCN;
  const int q = r % Q; r /= Q;
  const int kx = r % KSP; r /= KSP;
  const int ky = r % KS; r /= KS;
  const int cc = r % nchunk; r /= nchunk;
  const int cb = (int)r;
  const int co = cb * kCN + col, ci = cc * 4 * Q + 4 * q + e;
  float v = 0.f;
  if (co < Cout && ci < Cin && kx < KS) v = w[(((size_t)co * Cin + ci) * KS + ky) * KS + kx];
  packed[i] = v;
}

// max_pool2d(3, stride 2), floor mode, NHWC; one thread per output pixel and channel quad
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float4* __restrict__ in, float4* __restrict__ out, int B, int H, int W, int C4, int Ho,
                                                         int Wo) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)B * Ho * Wo * C4;
  if (i >= total) return;
  const int c = i % C4;
  size_t r = i / C4;
  const int ox = r % Wo; r /= Wo;
  const int oy = r % Ho;
  const size_t b = r / Ho;
  const float4* p = in + ((b * H + 2 * oy) * W + 2 * ox) * C4 + c;
  float4 v = p[0];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const float4 u = p[((size_t)ky * W + kx) * C4];
      v = make_float4(fmaxf(v.x, u.x), fmaxf(v.y, u.y), fmaxf(v.z, u.z), fmaxf(v.w, u.w));
    }
  out[i] = v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // (commutative steps: every lane ends with the same bits)
  return v;
}

// one tap: features of image n (ref) and n + N (pred), (2N,HW,C) NHWC; part[n * tiles + tile] = the workgroup's sum of d over its pixels
template <int CPL>
__global__ __launch_bounds__(256) void lpips_head_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int N, int HW, int C,
                                                         int tiles, float* __restrict__ part) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tile = blockIdx.x, n = blockIdx.y;
  const float* __restrict__ fr = feat + (size_t)n * HW * C;
  const float* __restrict__ fp = feat + (size_t)(n + N) * HW * C;
  float w[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) w[k] = (k * 64 + lane < C) ? lin[k * 64 + lane] : 0.f;
  float sum = 0.f;
  for (int i = 0; i < kHeadPix; ++i) {
    const int p = tile * kHeadTile + wv * kHeadPix + i;
    if (p >= HW) break;
    float r[CPL], q[CPL];
    float sr = 0.f, sp = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int c = k * 64 + lane;
      r[k] = c < C ? fr[(size_t)p * C + c] : 0.f;
      q[k] = c < C ? fp[(size_t)p * C + c] : 0.f;
      sr = fmaf(r[k], r[k], sr);
      sp = fmaf(q[k], q[k], sp);
    }
    const float nr = sqrtf(wave_sum(sr)) + 1e-10f, np = sqrtf(wave_sum(sp)) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const float e = r[k] / nr - q[k] / np;
      d = fmaf(w[k], e * e, d);
    }
    sum += wave_sum(d);
  }
  if (lane == 0) red[wv] = sum;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)n * tiles + tile] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct FinishArgs {
  const float* part[kTaps];
  int tiles[kTaps];
  double hw[kTaps];
  float* out;
};

__global__ void __launch_bounds__(64) lpips_finish_kernel(FinishArgs f) {
  __shared__ double v[kTaps];
  const int n = blockIdx.x, t = threadIdx.x;
  float* o = f.out + (size_t)n * (1 + kTaps);
  if (t < kTaps) {
    const float* p = f.part[t] + (size_t)n * f.tiles[t];
    double s = 0.0;
    for (int i = 0; i < f.tiles[t]; ++i) s += (double)p[i];
    s /= f.hw[t];
    v[t] = s;
    o[1 + t] = (float)s;
  }
  __syncthreads();
  if (t == 0) o[0] = (float)((((v[0] + v[1]) + v[2]) + v[3]) + v[4]);
}

// ---- sizes -----------------------------------------------------------------------------------------------------------------------
inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

struct Plan {
  int h[kTaps], w[kTaps];                    // tap sides: relu1, relu2, relu3 = relu4 = relu5
  int ph[2], pw[2];                          // pooled sides (pool1 = relu2's, pool2 = relu3's)
  size_t act[kTaps], pool[2], part[kTaps];   // byte offsets
  int tiles[kTaps];
  size_t bytes;
};

Plan plan(int N, int H, int W) {
  Plan p;
  p.h[0] = (H + 4 - 11) / 4 + 1;
  p.w[0] = (W + 4 - 11) / 4 + 1;
  p.ph[0] = (p.h[0] - 3) / 2 + 1;
  p.pw[0] = (p.w[0] - 3) / 2 + 1;
  p.h[1] = p.ph[0];
  p.w[1] = p.pw[0];
  p.ph[1] = (p.h[1] - 3) / 2 + 1;
  p.pw[1] = (p.w[1] - 3) / 2 + 1;
  for (int k = 2; k < kTaps; ++k) {
    p.h[k] = p.ph[1];
    p.w[k] = p.pw[1];
  }
  const size_t B = 2 * (size_t)N;
  size_t off = 0;
  for (int k = 0; k < kTaps; ++k) {
    p.act[k] = off;
    off += align256(B * p.h[k] * p.w[k] * kTapC[k] * sizeof(float));
    if (k < 2) {
      p.pool[k] = off;
      off += align256(B * p.ph[k] * p.pw[k] * kTapC[k] * sizeof(float));
    }
  }
  for (int k = 0; k < kTaps; ++k) {
    p.tiles[k] = (p.h[k] * p.w[k] + kHeadTile - 1) / kHeadTile;
    p.part[k] = off;
    off += align256((size_t)N * p.tiles[k] * sizeof(float));
  }
  p.bytes = off;
  return p;
}

// net buffer: conv1 and conv2 slabs (pack_kxk_kernel), conv3..5 (harp_conv3x3_pack_filters, HARP_CONV_F32), the five biases, the five
// lin weights; every block 256-B aligned
struct NetLayout {
  size_t w[kTaps], bias[kTaps], lin[kTaps], bytes;
};
constexpr int kCin[kTaps] = {3, 64, 192, 384, 256};
constexpr int kKS[kTaps] = {11, 5, 3, 3, 3};

NetLayout net_layout() {
  NetLayout l;
  size_t off = 0;
  l.w[0] = off;
  off += align256((size_t)1 * 11 * 12 * 1 * kCN * 16);                         // one output block, one chunk, 11 rows x 12 slots x 1 quad
  l.w[1] = off;
  off += align256((size_t)(192 / kCN) * (64 / 16) * 5 * 5 * 4 * kCN * 16);
  for (int k = 2; k < kTaps; ++k) {
    l.w[k] = off;
    off += align256(harp_conv3x3_filter_bytes(kTapC[k], kCin[k]));
  }
  for (int k = 0; k < kTaps; ++k) {
    l.bias[k] = off;
    off += align256(kTapC[k] * sizeof(float));
  }
  for (int k = 0; k < kTaps; ++k) {
    l.lin[k] = off;
    off += align256(kTapC[k] * sizeof(float));
  }
  l.bytes = off;
  return l;
}

template <int KS, int S, int Q, bool FIRST>
int launch_kxk(ConvArgs a, hipStream_t stream) {
  a.tiles_x = (a.Wo + kT - 1) / kT;
  a.tiles_y = (a.Ho + kT - 1) / kT;
  const size_t blocks = (size_t)a.tiles_x * a.tiles_y * a.B * (a.Cout / kCN);
  if (blocks == 0 || blocks > 0x7fffffffu) return HARP_ERR_ARG;
  hipLaunchKernelGGL((conv_kxk_kernel<KS, S, Q, FIRST>), dim3((unsigned)blocks), dim3(256), 0, stream, a);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

int launch_pool(const float* in, float* out, int B, int H, int W, int C, int Ho, int Wo, hipStream_t stream) {
  const size_t total = (size_t)B * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const float4*)in, (float4*)out, B, H, W, C / 4,
                     Ho, Wo);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

}  // namespace

extern "C" {

size_t harp_lpips_alex_net_bytes(void) { return net_layout().bytes; }

int harp_lpips_alex_pack(const float* const* w, const float* const* bias, const float* const* lin, void* net, hipStream_t stream) {
  if (!w || !bias || !lin || !net || ((size_t)net & 255)) return HARP_ERR_ARG;
  for (int k = 0; k < kTaps; ++k)
    if (!w[k] || !bias[k] || !lin[k]) return HARP_ERR_ARG;
  const NetLayout l = net_layout();
  char* base = (char*)net;
  const int ksp[2] = {12, 5}, q[2] = {1, 4};
  for (int k = 0; k < 2; ++k) {
    const size_t total = (size_t)((kTapC[k] + kCN - 1) / kCN) * kCN * ((kCin[k] + 4 * q[k] - 1) / (4 * q[k])) * kKS[k] * ksp[k] * q[k] * 4;
    hipLaunchKernelGGL(pack_kxk_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, w[k], kTapC[k], kCin[k], kKS[k], ksp[k], q[k],
                       (float*)(base + l.w[k]));
    HARP_CHECK_LAUNCH();
  }
  for (int k = 2; k < kTaps; ++k) {
    const int rc = harp_conv3x3_pack_filters(w[k], kTapC[k], kCin[k], 0, HARP_CONV_F32, base + l.w[k], stream);
    if (rc != HARP_OK) return rc;
  }
  for (int k = 0; k < kTaps; ++k) {
    if (hipMemcpyAsync(base + l.bias[k], bias[k], kTapC[k] * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) return HARP_ERR_LAUNCH;
    if (hipMemcpyAsync(base + l.lin[k], lin[k], kTapC[k] * sizeof(float), hipMemcpyDeviceToDevice, stream) != hipSuccess) return HARP_ERR_LAUNCH;
  }
  return HARP_OK;
}

size_t harp_lpips_alex_ws_bytes(int N, int H, int W) {
  if (N < 1 || N > 65535 || H < kMinSide || W < kMinSide) return 0;
  return plan(N, H, W).bytes;
}

int harp_lpips_alex(const void* net, const float* ref, const float* pred, long long sn, long long sc, long long sy, long long sx, int N, int H,
                    int W, int normalize, void* ws, float* out, hipStream_t stream) {
  if (!net || !ref || !pred || !ws || !out || ((size_t)net & 255) || ((size_t)ws & 255)) return HARP_ERR_ARG;
  if (N < 1 || N > 65535 || H < kMinSide || W < kMinSide) return HARP_ERR_ARG;
  const Plan p = plan(N, H, W);
  // 32-bit offsets inside one image (activations here and in harp_conv3x3) and in the head's pixel index
  for (int k = 0; k < kTaps; ++k)
    if ((size_t)p.h[k] * p.w[k] * 384 > 0x7fffffffu) return HARP_ERR_ARG;
  const NetLayout l = net_layout();
  const char* nb = (const char*)net;
  char* wb = (char*)ws;
  auto act = [&](int k) { return (float*)(wb + p.act[k]); };
  auto pool = [&](int k) { return (float*)(wb + p.pool[k]); };
  const int B = 2 * N;
  ConvArgs a = {};
  a.in = ref; a.in2 = pred; a.sn = sn; a.sc = sc; a.sy = sy; a.sx = sx; a.N = N;
  a.B = B; a.H = H; a.W = W; a.Cin = 3; a.Ho = p.h[0]; a.Wo = p.w[0]; a.Cout = 64; a.pad = 2;
  a.filters = (const float4*)(nb + l.w[0]); a.bias = (const float*)(nb + l.bias[0]); a.out = act(0); a.normalize = normalize != 0;
  int rc = launch_kxk<11, 4, 1, true>(a, stream);
  if (rc != HARP_OK) return rc;
  if ((rc = launch_pool(act(0), pool(0), B, p.h[0], p.w[0], 64, p.ph[0], p.pw[0], stream)) != HARP_OK) return rc;
  a = ConvArgs{};
  a.in = pool(0); a.B = B; a.H = p.ph[0]; a.W = p.pw[0]; a.Cin = 64; a.Ho = p.h[1]; a.Wo = p.w[1]; a.Cout = 192; a.pad = 2;
  a.filters = (const float4*)(nb + l.w[1]); a.bias = (const float*)(nb + l.bias[1]); a.out = act(1);
  if ((rc = launch_kxk<5, 1, 4, false>(a, stream)) != HARP_OK) return rc;
  if ((rc = launch_pool(act(1), pool(1), B, p.h[1], p.w[1], 192, p.ph[1], p.pw[1], stream)) != HARP_OK) return rc;
  for (int k = 2; k < kTaps; ++k) {
    harp_conv3x3_args c = {};
    c.in = k == 2 ? pool(1) : act(k - 1);
    c.filters = nb + l.w[k];
    c.bias = (const float*)(nb + l.bias[k]);
    c.out = act(k);
    c.N = B; c.H = p.h[k]; c.W = p.w[k]; c.Cin = kCin[k]; c.Cout = kTapC[k];
    c.precision = HARP_CONV_F32;
    c.epilogue = HARP_CONV_RELU;
    if ((rc = harp_conv3x3(&c, stream)) != HARP_OK) return rc;
  }
  FinishArgs f;
  for (int k = 0; k < kTaps; ++k) {
    const int HW = p.h[k] * p.w[k], C = kTapC[k];
    float* part = (float*)(wb + p.part[k]);
    const float* lin = (const float*)(nb + l.lin[k]);
    const dim3 grid((unsigned)p.tiles[k], (unsigned)N);
    switch ((C + 63) / 64) {
      case 1: hipLaunchKernelGGL(lpips_head_kernel<1>, grid, dim3(256), 0, stream, act(k), lin, N, HW, C, p.tiles[k], part); break;
      case 3: hipLaunchKernelGGL(lpips_head_kernel<3>, grid, dim3(256), 0, stream, act(k), lin, N, HW, C, p.tiles[k], part); break;
      case 4: hipLaunchKernelGGL(lpips_head_kernel<4>, grid, dim3(256), 0, stream, act(k), lin, N, HW, C, p.tiles[k], part); break;
      default: hipLaunchKernelGGL(lpips_head_kernel<6>, grid, dim3(256), 0, stream, act(k), lin, N, HW, C, p.tiles[k], part); break;
    }
    HARP_CHECK_LAUNCH();
    f.part[k] = part;
    f.tiles[k] = p.tiles[k];
    f.hw[k] = (double)HW;
  }
  f.out = out;
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)N), dim3(64), 0, stream, f);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

}  // extern "C"
