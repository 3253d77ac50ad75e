// Motion labels (harp_amd/playback/player.py flow): where the surface point that an output pixel of the composite shows
// lies in ANOTHER frame of the same meshes — optical flow, the change of view depth, and whether the point is still seen there and by
// what it is hidden.  include/harp_hip.h states the contract; tests/_flow_ref.py restates it in float64.
//
// harp_flow_layers: one lane per OUTPUT pixel.  The source point is harp_annotate_layers' — the composite's winner per sub-sample, the
//   owner, the part vote and the representative sub-sample.  THAT CODE BELONGS TO csrc/annotate.hip (annotate_layers_kernel, from the scene
//   depth down to the representative): the block marked below is a copy of it, word for word, and a change there is made here too.  It
//   is a copy and not a shared header because moving it out of annotate.hip changed that kernel's registers.
//   The at most 16 sub-samples stay in registers; the owner layer's table entries are taken by selects (pick).  Then per owned pixel
//   three face indices, nine source ndc floats (bary_fwd of csrc/shade_common.h at the centre of the source sub-pixel: the point `uv` is
//   taken at), nine target ndc floats, and at the landing sub-pixel one target depth per layer and one target scene depth
//   (harp_keypoint_visibility's test).  No LDS, no scratch, no atomics: the pixel groups go in plain order.
// The layer table travels BY VALUE.  Every index is derived from (b, y, x) < (B, S, S), the mirrored column, a scene-depth row checked
// against n_scene, a face id checked against F, vertex indices checked against V, and a landing sub-pixel checked against [0, S ss)^2
// before it is used.  Nothing is read or written out of bounds; all stores are per-lane vector stores.
#include "shade_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kMaxLayers = 4;

struct FlowPack {
  const int32_t* face[kMaxLayers];
  const float* z[kMaxLayers];
  const unsigned char* label[kMaxLayers];
  const float* ndc[kMaxLayers];
  const int32_t* faces[kMaxLayers];
  const float* ndc_to[kMaxLayers];
  const float* z_to[kMaxLayers];
  int V[kMaxLayers], F[kMaxLayers], flip[kMaxLayers];
};

// entry `l` of a four-entry kernel-argument table by selects: a per-lane index into the table would make a private copy of it
template <typename T>
__device__ __forceinline__ T pick(const T (&t)[kMaxLayers], int l) {
  return l == 0 ? t[0] : (l == 1 ? t[1] : (l == 2 ? t[2] : t[3]));
}

// N consecutive 32-bit words at p, as the widest words the address allows (composite.hip's load_span; a sub-row starts on a multiple of ss)
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

template <int SS>
__global__ void __launch_bounds__(256) flow_layers_kernel(const FlowPack L, int n_layers, int B, int S, const float* __restrict__ scene_z,
                                                          int n_scene, const int32_t* __restrict__ scene_rows,
                                                          const float* __restrict__ scene_z_to, int n_scene_to,
                                                          const int32_t* __restrict__ scene_rows_to, float tol, float* __restrict__ flow,
                                                          float* __restrict__ dz, unsigned char* __restrict__ status) {
  constexpr int kVec = SS == 4 ? 4 : (SS == 2 ? 2 : 1);
  constexpr int kN = SS * SS;
  const long long per = (long long)S * S, total = per * B;
  const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = at < total;
  const long long idx = live ? at : total - 1;       // a lane past the end works on the last pixel again and stores nothing
  const int b = (int)(idx / per);
  const int rem = (int)(idx - (long long)b * per), y = rem / S, x = rem - y * S;
  // ---- the source point: a copy of csrc/annotate.hip annotate_layers_kernel (see the head of this file) ----------------------------
  // the scene depth in front of this pixel; d > 0 is a measurement (0 and NaN: nothing in front)
  float d = 0.0f;
  const int srow = scene_rows ? scene_rows[b] : (n_scene == B ? b : 0);
  if (scene_z && srow >= 0 && srow < n_scene) d = scene_z[(size_t)srow * per + rem];
  const bool has_d = d > 0.0f;
  const int Shi = S * SS;
  const size_t Sh = (size_t)Shi;
  int key[kN], fc[kN];                                // per sub-sample: layer << 8 | label (-1: no winner), the winner's face id and depth
  float zz[kN];
#pragma unroll
  for (int sy = 0; sy < SS; ++sy) {
    const size_t r0 = ((size_t)b * Sh + (size_t)y * SS + sy) * Sh;
    float bz[SS];
    int bl[SS], bf[SS];
#pragma unroll
    for (int sx = 0; sx < SS; ++sx) { bl[sx] = -1; bz[sx] = 0.0f; bf[sx] = -1; }
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
        // the composite's rule: z > 0 (NaN and -1 are not), in front of a valid scene depth; it wins over a STRICTLY farther earlier layer only
        take[sx] = zl > 0.0f && (!has_d || zl < d) && (bl[sx] < 0 || zl < bz[sx]);
        any |= take[sx];
      }
      if (!any) continue;
      float f[SS];
      load_span<SS, kVec>((const float*)(L.face[l] + p0), f);
#pragma unroll
      for (int sx = 0; sx < SS; ++sx)
        if (take[sx]) {
          bz[sx] = flip ? z[SS - 1 - sx] : z[sx]; bl[sx] = l;
          bf[sx] = __float_as_int(flip ? f[SS - 1 - sx] : f[sx]);
        }
    }
#pragma unroll
    for (int sx = 0; sx < SS; ++sx) {
      const int i = sy * SS + sx;
      int k = -1;
      if (bl[sx] >= 0) {
        const unsigned char* lab = pick(L.label, bl[sx]);
        const int F = pick(L.F, bl[sx]);
        k = (bl[sx] << 8) | (bf[sx] >= 0 && bf[sx] < F ? (int)lab[bf[sx]] : 0);
      }
      key[i] = k; zz[i] = bz[sx]; fc[i] = bf[sx];
    }
  }
  // owner: the layer that won the most sub-samples, a tie to the lower index (composite.hip, bit for bit)
  int best = 0, who = 0;
#pragma unroll
  for (int l = 0; l < kMaxLayers; ++l) {
    int won = 0;
#pragma unroll
    for (int i = 0; i < kN; ++i) won += (key[i] >> 8) == l ? 1 : 0;    // (-1 >> 8 is -1: no layer)
    if (won > best) { best = won; who = l + 1; }
  }
  // part: among the owner's sub-samples the most frequent label, a tie to the lower label (equal keys: same layer, same label)
  int bc = 0, bkey = -1;
#pragma unroll
  for (int i = 0; i < kN; ++i) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < kN; ++j) c += key[j] == key[i] ? 1 : 0;
    const bool mine = key[i] >= 0 && (key[i] >> 8) == who - 1;
    if (mine && (c > bc || (c == bc && key[i] < bkey))) { bc = c; bkey = key[i]; }
  }
  // representative: of the owner's sub-samples with that label the nearest, a tie to the first in row-major order
  int ri = -1, rf = -1;
  float rz = 0.0f;
#pragma unroll
  for (int i = 0; i < kN; ++i)
    if (key[i] >= 0 && key[i] == bkey && (ri < 0 || zz[i] < rz)) { ri = i; rz = zz[i]; rf = fc[i]; }
  // ---- end of the copy -----------------------------------------------------------------------------------------------------------
  float fx = 0.0f, fy = 0.0f, dzo = 0.0f;
  unsigned char st = who ? 1 : 0, by = 0;              // an owned pixel is not trackable until everything below holds
  const int ol = who - 1;
  if (who && rf >= 0 && rf < pick(L.F, ol)) {
    const int32_t* fv = pick(L.faces, ol) + 3 * (size_t)rf;
    const int V = pick(L.V, ol);
    const int i0 = fv[0], i1 = fv[1], i2 = fv[2];
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
      // the centre of the SOURCE sub-pixel the layer was read at (the mirrored column of a flipped layer): the point uv is taken at
      const bool oflip = pick(L.flip, ol) != 0;
      const int sy = ri / SS, sx = ri - sy * SS;
      const int Xo = x * SS + sx, Xs = oflip ? Shi - 1 - Xo : Xo, Ys = y * SS + sy;
      const float* nb = pick(L.ndc, ol) + (size_t)b * V * 3;
      Tri t;
      t.x0 = nb[3 * i0]; t.y0 = nb[3 * i0 + 1]; t.z0 = nb[3 * i0 + 2];
      t.x1 = nb[3 * i1]; t.y1 = nb[3 * i1 + 1]; t.z1 = nb[3 * i1 + 2];
      t.x2 = nb[3 * i2]; t.y2 = nb[3 * i2 + 1]; t.z2 = nb[3 * i2 + 2];
      const Bary br = bary_fwd(t, pix_to_ndc(Xs, Shi), pix_to_ndc(Ys, Shi));
      // the same point of the face in the target frame (harp_texture_bake_accum's projection of a barycentric point)
      const float* nt = pick(L.ndc_to, ol) + (size_t)b * V * 3;
      const float z0 = nt[3 * i0 + 2], z1 = nt[3 * i1 + 2], z2 = nt[3 * i2 + 2];
      const float w0 = br.b0 * z0, w1 = br.b1 * z1, w2 = br.b2 * z2;
      const float Zp = w0 + w1 + w2;
      if (Zp > 1e-3f) {                                                   // (a NaN is not)
        const float xp = (w0 * nt[3 * i0] + w1 * nt[3 * i1] + w2 * nt[3 * i2]) / Zp;
        const float yp = (w0 * nt[3 * i0 + 1] + w1 * nt[3 * i1 + 1] + w2 * nt[3 * i2 + 1]) / Zp;
        const float lim = (float)Shi, half = 0.5f * lim;
        float cx = (1.0f - xp) * half;
        const float cy = (1.0f - yp) * half;
        if (oflip) cx = lim - cx;
        const float inf = __builtin_inff();
        if (Zp < inf && fabsf(cx) < inf && fabsf(cy) < inf) {             // (a NaN fails every comparison)
          fx = (cx - ((float)Xo + 0.5f)) / (float)SS;
          fy = (cy - ((float)Ys + 0.5f)) / (float)SS;
          dzo = Zp - rz;
          st = 2;
          if (cx >= 0.0f && cx < lim && cy >= 0.0f && cy < lim) {
            // harp_keypoint_visibility's test at the landing sub-pixel of the TARGET frame
            const int Xt = min((int)cx, Shi - 1), Yt = min((int)cy, Shi - 1);
            const int xo = Xt / SS, yo = Yt / SS;
            float dt = 0.0f;
            const int trow = scene_rows_to ? scene_rows_to[b] : (n_scene_to == B ? b : 0);
            if (scene_z_to && trow >= 0 && trow < n_scene_to) dt = scene_z_to[((size_t)trow * S + yo) * S + xo];
            const bool has_dt = dt > 0.0f;
            const size_t q0 = ((size_t)b * Sh + (size_t)Yt) * Sh;
            int nl = -1;
            float nz = 0.0f;
#pragma unroll
            for (int l = 0; l < kMaxLayers; ++l) {
              if (l >= n_layers) break;
              const float zl = L.z_to[l][q0 + (size_t)(L.flip[l] ? Shi - 1 - Xt : Xt)];
              if (zl > 0.0f && (!has_dt || zl < dt) && (nl < 0 || zl < nz)) { nz = zl; nl = l; }
            }
            const bool something = nl >= 0 || has_dt;
            const float near = nl >= 0 ? nz : dt;
            const bool visible = !something || near >= Zp - tol;
            st = visible ? 4 : 3;
            by = visible ? 0 : (unsigned char)(nl >= 0 ? 1 + nl : 255);
          }
        }
      }
    }
  }
  if (live) {
    flow[2 * (size_t)idx] = fx; flow[2 * (size_t)idx + 1] = fy;
    dz[idx] = dzo;
    status[2 * (size_t)idx] = st; status[2 * (size_t)idx + 1] = by;
  }
}

bool scene_ok(const float* scene_z, int n_scene, const int32_t* scene_rows, int B) {
  return !scene_z || (n_scene > 0 && (scene_rows || n_scene == 1 || n_scene == B));
}

}  // namespace

extern "C" int harp_flow_layers(const harp_flow_layer* layers, int n_layers, int B, int S, int ss, const float* scene_z, int n_scene,
                                const int32_t* scene_rows, const float* scene_z_to, int n_scene_to, const int32_t* scene_rows_to, float tol,
                                float* flow, float* dz, unsigned char* status, hipStream_t stream) {
  if (!layers || !flow || !dz || !status || n_layers < 1 || n_layers > kMaxLayers) return HARP_ERR_ARG;
  if (B <= 0 || S <= 0 || ss < 1 || ss > 4) return HARP_ERR_ARG;
  if (!scene_ok(scene_z, n_scene, scene_rows, B) || !scene_ok(scene_z_to, n_scene_to, scene_rows_to, B)) return HARP_ERR_ARG;
  if (!(tol >= 0.0f) || !(tol < __builtin_inff())) return HARP_ERR_ARG;      // (a NaN is neither)
  if ((long long)S * ss > 46340LL) return HARP_ERR_ARG;               // (S ss)^2 and S^2 fit an int
  const long long px = (long long)S * S * B;
  if (px > 0x7fffffffLL * 256) return HARP_ERR_ARG;
  FlowPack L = {};
  for (int l = 0; l < n_layers; ++l) {                                // the host array is read here and nowhere later
    const harp_flow_layer& a = layers[l];
    if (!a.face_id || !a.zbuf || !a.face_label || !a.ndc || !a.faces || !a.ndc_to || !a.zbuf_to) return HARP_ERR_ARG;
    if (a.V <= 0 || a.F <= 0 || a.reserved != 0) return HARP_ERR_ARG;
    L.face[l] = a.face_id; L.z[l] = a.zbuf; L.label[l] = a.face_label; L.ndc[l] = a.ndc; L.faces[l] = a.faces;
    L.ndc_to[l] = a.ndc_to; L.z_to[l] = a.zbuf_to; L.V[l] = a.V; L.F[l] = a.F; L.flip[l] = a.flip_x != 0;
  }
  const dim3 grid((unsigned)((px + 255) / 256)), block(256);
  if (!scene_z) n_scene = 0;
  if (!scene_z_to) n_scene_to = 0;
#define HARP_FLOW(SS)                                                                                                                   \
  hipLaunchKernelGGL((flow_layers_kernel<SS>), grid, block, 0, stream, L, n_layers, B, S, scene_z, n_scene, scene_rows, scene_z_to,     \
                     n_scene_to, scene_rows_to, tol, flow, dz, status)
  switch (ss) {
    case 1: HARP_FLOW(1); break;
    case 2: HARP_FLOW(2); break;
    case 3: HARP_FLOW(3); break;
    default: HARP_FLOW(4); break;
  }
#undef HARP_FLOW
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
