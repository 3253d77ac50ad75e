// Scene playback (harp_amd/playback.py ScenePlayer): several supersampled avatar layers with their view depth resolved
// into one finished 8-bit frame with depth-correct occlusion.  harp_resolve_u8 (csrc/playback.hip) knows "covered or not" of ONE render;
// this is the same box filter over the NEAREST of up to four renders per sub-sample, each optionally read mirrored in x (a left hand is a
// right-hand fit of mirrored frames), tested against an optional scene depth at output resolution (a cup in front of the hand hides it).
//
// harp_composite_layers_u8: layers l = 0..n-1 of rgb (B, S ss, S ss, 3) and zbuf (B, S ss, S ss) (view depth, > 0: covered), ss in 1..4
//   -> out (B,S,S,3|4) uint8 and optionally owner (B,S,S) uint8 = 1 + the layer that won most sub-samples of the pixel (0: none).
//   One lane per output pixel, as resolve_u8_kernel.  Per sub-row the lane walks the layers: the 4 ss bytes of depth first, and the 12 ss
//   bytes of colour only when that layer wins at least one of the sub-row's samples — a layer that is empty or hidden there costs its
//   depth alone.  Both are read as 8- / 16-byte words where ss and the address allow.  A flipped layer reads the span of the mirrored
//   pixel S - 1 - x (the same aligned words) and reverses it in registers.  No LDS, no atomics.
//   The layer table travels to the kernel BY VALUE (kernel arguments): nothing on the device points at host memory, and a captured graph
//   holds its own copy.  Every index is derived from (b, y, x) < (B, S, S), the mirrored column S - 1 - x, and a background / scene-depth
//   row checked against n_bg / n_scene: nothing is read or written out of bounds.
#include "harp_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "harp_hip.h"

namespace {

constexpr int kMaxLayers = 4;

struct LayerPack {
  const float* rgb[kMaxLayers];
  const float* z[kMaxLayers];
  int flip[kMaxLayers];
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }      // (NaN -> 0)
__device__ __forceinline__ unsigned quantise(float v) { return (unsigned)min(max((int)(255.0f * v + 0.5f), 0), 255); }

// N consecutive floats at p, as the widest words the address allows (N = ss or 3 ss; a sub-row starts on a multiple of ss elements)
template <int N, int VEC>
__device__ __forceinline__ void load_span(const float* p, float (&v)[N]) {
  if constexpr (VEC == 4) {
    if (((uintptr_t)p & 15) == 0) {
#pragma unroll
      for (int k = 0; k < N / 4; ++k) {
        const float4 w = ((const float4*)p)[k];
        v[4 * k] = w.x; v[4 * k + 1] = w.y; v[4 * k + 2] = w.z; v[4 * k + 3] = w.w;
      }
      return;
    }
  } else if constexpr (VEC == 2) {
    if (((uintptr_t)p & 7) == 0) {
#pragma unroll
      for (int k = 0; k < N / 2; ++k) {
        const float2 w = ((const float2*)p)[k];
        v[2 * k] = w.x; v[2 * k + 1] = w.y;
      }
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = p[k];
}

template <int SS, int CH>
__global__ void __launch_bounds__(256) composite_layers_u8_kernel(const LayerPack L, int n_layers, int B, int S,
                                                                  const float* __restrict__ scene_z, int n_scene,
                                                                  const int32_t* __restrict__ scene_rows, const unsigned char* __restrict__ bg,
                                                                  int n_bg, const int32_t* __restrict__ bg_rows,
                                                                  const float* __restrict__ bg_color, unsigned char* __restrict__ out,
                                                                  unsigned char* __restrict__ owner) {
  constexpr int kVec = SS == 4 ? 4 : (SS == 2 ? 2 : 1);
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)S * S;
  if (idx >= per * B) return;
  const int b = (int)(idx / per);
  const int rem = (int)(idx - (long long)b * per), y = rem / S, x = rem - y * S;
  // the background of this pixel: a byte triple of frame `row`, or the constant colour quantised like a pixel (as resolve_u8_kernel)
  unsigned bgb[3];
  const int row = bg_rows ? bg_rows[b] : (n_bg == B ? b : 0);
  if (bg && row >= 0 && row < n_bg) {
    const unsigned char* pb = bg + ((size_t)row * per + rem) * 3;
    bgb[0] = pb[0]; bgb[1] = pb[1]; bgb[2] = pb[2];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) bgb[c] = quantise(clamp01(bg_color[c]));
  }
  // the scene depth in front of this pixel; d > 0 is a measurement (0 and NaN: nothing in front)
  float d = 0.0f;
  const int srow = scene_rows ? scene_rows[b] : (n_scene == B ? b : 0);
  if (scene_z && srow >= 0 && srow < n_scene) d = scene_z[(size_t)srow * per + rem];
  const bool has_d = d > 0.0f;
  const size_t Sh = (size_t)S * SS;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  int n = 0;
  int won[kMaxLayers] = {0, 0, 0, 0};
#pragma unroll
  for (int sy = 0; sy < SS; ++sy) {
    const size_t r0 = ((size_t)b * Sh + (size_t)y * SS + sy) * Sh;
    float bz[SS], bc[SS * 3];
    int bl[SS];
#pragma unroll
    for (int sx = 0; sx < SS; ++sx) bl[sx] = -1;
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l) {
      if (l >= n_layers) break;
      const bool flip = L.flip[l] != 0;
      const size_t p0 = r0 + (size_t)(flip ? S - 1 - x : x) * SS;        // the mirrored pixel's span holds the mirrored sub-columns, reversed
      float z[SS];
      load_span<SS, kVec>(L.z[l] + p0, z);
      bool take[SS], any = false;
#pragma unroll
      for (int sx = 0; sx < SS; ++sx) {
        const float zl = flip ? z[SS - 1 - sx] : z[sx];
        // candidate: z > 0 (NaN and -1 are not), in front of a valid scene depth; it wins over a STRICTLY farther earlier layer only
        take[sx] = zl > 0.0f && (!has_d || zl < d) && (bl[sx] < 0 || zl < bz[sx]);
        any |= take[sx];
      }
      if (!any) continue;
      float c[SS * 3];
      load_span<SS * 3, kVec>(L.rgb[l] + p0 * 3, c);
#pragma unroll
      for (int sx = 0; sx < SS; ++sx) {
        const int kf = 3 * (SS - 1 - sx), ku = 3 * sx;                     // (static once unrolled: the arrays stay in registers)
        if (take[sx]) {
          bz[sx] = flip ? z[SS - 1 - sx] : z[sx]; bl[sx] = l;
          bc[ku] = flip ? c[kf] : c[ku]; bc[ku + 1] = flip ? c[kf + 1] : c[ku + 1]; bc[ku + 2] = flip ? c[kf + 2] : c[ku + 2];
        }
      }
    }
#pragma unroll
    for (int sx = 0; sx < SS; ++sx)
      if (bl[sx] >= 0) {
        ++n;
        sum[0] += clamp01(bc[3 * sx]); sum[1] += clamp01(bc[3 * sx + 1]); sum[2] += clamp01(bc[3 * sx + 2]);
#pragma unroll
        for (int l = 0; l < kMaxLayers; ++l) won[l] += bl[sx] == l ? 1 : 0;
      }
  }
  constexpr int kN = SS * SS;
  unsigned o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    o[c] = n == 0 ? bgb[c] : quantise((sum[c] + (float)(kN - n) * ((float)bgb[c] / 255.0f)) / (float)kN);
  unsigned char* po = out + (size_t)idx * CH;
  if (CH == 4) {
    const unsigned al = (unsigned)((255 * n + kN / 2) / kN);          // integers: 255 n / ss^2 sits ON .5 for (ss, n) = (2, 2), (4, 8)
    const unsigned word = o[0] | (o[1] << 8) | (o[2] << 16) | (al << 24);
    if (((uintptr_t)po & 3) == 0) {
      *(unsigned*)po = word;
    } else {
      po[0] = (unsigned char)o[0]; po[1] = (unsigned char)o[1]; po[2] = (unsigned char)o[2]; po[3] = (unsigned char)al;
    }
  } else {
    po[0] = (unsigned char)o[0]; po[1] = (unsigned char)o[1]; po[2] = (unsigned char)o[2];
  }
  if (owner) {
    int best = 0, who = 0;                                             // most sub-samples; a tie goes to the lower index
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l)
      if (won[l] > best) { best = won[l]; who = l + 1; }
    owner[idx] = (unsigned char)who;
  }
}

}  // namespace

extern "C" int harp_composite_layers_u8(const harp_layer* layers, int n_layers, int B, int S, int ss, const float* scene_z, int n_scene,
                                        const int32_t* scene_rows, const unsigned char* bg, int n_bg, const int32_t* bg_rows,
                                        const float* bg_color, int channels, unsigned char* out, unsigned char* owner, hipStream_t stream) {
  if (!layers || !out || !bg_color || n_layers < 1 || n_layers > kMaxLayers) return HARP_ERR_ARG;
  if (B <= 0 || S <= 0 || ss < 1 || ss > 4 || (channels != 3 && channels != 4)) return HARP_ERR_ARG;
  if (bg && (n_bg <= 0 || (!bg_rows && n_bg != 1 && n_bg != B))) return HARP_ERR_ARG;
  if (scene_z && (n_scene <= 0 || (!scene_rows && n_scene != 1 && n_scene != B))) return HARP_ERR_ARG;
  if ((long long)S * ss > 46340LL) return HARP_ERR_ARG;               // (S ss)^2 and S^2 fit an int
  const long long px = (long long)S * S * B;
  if (px > 0x7fffffffLL * 256) return HARP_ERR_ARG;
  LayerPack L = {};
  for (int l = 0; l < n_layers; ++l) {                                // the host array is read here and nowhere later
    if (!layers[l].rgb || !layers[l].zbuf || layers[l].reserved != 0) return HARP_ERR_ARG;
    L.rgb[l] = layers[l].rgb; L.z[l] = layers[l].zbuf; L.flip[l] = layers[l].flip_x != 0;
  }
  const dim3 grid((unsigned)((px + 255) / 256)), block(256);
  if (!bg) n_bg = 0;
  if (!scene_z) n_scene = 0;
#define HARP_COMPOSITE(SS, CH)                                                                                                          \
  hipLaunchKernelGGL((composite_layers_u8_kernel<SS, CH>), grid, block, 0, stream, L, n_layers, B, S, scene_z, n_scene, scene_rows, bg, \
                     n_bg, bg_rows, bg_color, out, owner)
#define HARP_COMPOSITE_SS(SS) do { if (channels == 4) HARP_COMPOSITE(SS, 4); else HARP_COMPOSITE(SS, 3); } while (0)
  switch (ss) {
    case 1: HARP_COMPOSITE_SS(1); break;
    case 2: HARP_COMPOSITE_SS(2); break;
    case 3: HARP_COMPOSITE_SS(3); break;
    default: HARP_COMPOSITE_SS(4); break;
  }
#undef HARP_COMPOSITE_SS
#undef HARP_COMPOSITE
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
