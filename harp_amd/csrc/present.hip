// What a fit is LOOKED at with (optimize_sequence.py:710-757, utils/visualize.py:145-228): the K-fragment normal image and the uint8
// panel strips, forward only, for gfx950.
//
// harp_normal_image = MeshRenderer(MeshRasterizer(K, blur 0), SoftPhongNormalShader) (renderer_helper.py:83-101, 216-301) in ONE pass:
//   rasterize_meshes (K nearest fragments) -> interpolate_face_attributes (vertex normals) -> [TexturesUV.sample_textures +
//   PBRMaterials.apply_normal_map] -> (x, -y, -z) -> (n + 1) / 2 -> softmax_rgb_blend.  No buffer with a K dimension exists: the K
//   candidates of a pixel (depth, face id) live in registers, and each kept fragment is shaded and blended as it is visited.
// Design: a workgroup of 256 lanes owns a 16 x 16 tile, one lane per pixel.  The face list of the tile's 64 x 64
//   super-tile (the rasteriser's workspace, as fragments_fwd_kernel walks it) is read in chunks of 256: every lane tests ONE face's box
//   against the tile, the survivors are compacted IN LIST ORDER (ballot + popcount) into LDS together with their 64-B records, and the
//   pixels then walk only those — LDS broadcast reads instead of each pixel walking the whole super-tile list in global memory.
//   The candidate test is the one of fragments_fwd_kernel with blur_radius = 0 (box, pz >= 0, b0, b1, b2 > 0) on the same float32
//   expressions, so the kept set is the fragment op's.  A cheap exact pre-test skips the divisions for most (pixel, face) pairs: if the
//   three depths are positive and an edge function has the sign opposite to the area's, that barycentric is <= 0 after the IEEE
//   divisions whatever their rounding, so the face is no candidate.
//   The K slots are sorted by a fully unrolled insert (compile-time register indices, no scratch); ties keep the lower face index
//   because faces arrive in ascending order and a new one only displaces strictly deeper ones.
// harp_panels_u8 = the numpy statement of optimize_sequence.py:744-755 (and the clip * 255 -> uint8 of utils/visualize.py:174-175) on
//   the device: only the final uint8 strip crosses to the host.
#include "shade_common.h"

int harp_detail_raster_setup(const float* ndc, const int32_t* faces, int B, int V, int F, int S, float r, void* ws, hipStream_t stream);

namespace {

constexpr int kMaxK = 16;
constexpr int kChunk = 256;

__device__ __forceinline__ float seg_d2(float px, float py, float ax, float ay, float bx, float by) {
  const float bax = bx - ax, bay = by - ay;
  const float l2 = bax * bax + bay * bay;
  if (l2 <= kEps) return (px - bx) * (px - bx) + (py - by) * (py - by);
  float t = (bax * (px - ax) + bay * (py - ay)) / l2;
  t = fminf(fmaxf(t, 0.f), 1.f);
  const float qx = ax + t * bax, qy = ay + t * bay;
  return (px - qx) * (px - qx) + (py - qy) * (py - qy);
}

struct Pair { float c0, c1, c2, pz; bool inside; };

// the (pixel, face) arithmetic of rasterize_meshes without blur, expression by expression that of fragments.hip:eval_pair (exact IEEE
// divisions, barycentrics not clipped)
__device__ __forceinline__ Pair eval_pair(const Tri& t, float px, float py) {
  Pair p;
  const float area = edge_fn(t.x2, t.y2, t.x0, t.y0, t.x1, t.y1) + kEps;
  const float w0 = edge_fn(px, py, t.x1, t.y1, t.x2, t.y2) / area;
  const float w1 = edge_fn(px, py, t.x2, t.y2, t.x0, t.y0) / area;
  const float w2 = edge_fn(px, py, t.x0, t.y0, t.x1, t.y1) / area;
  const float t0 = w0 * t.z1 * t.z2, t1 = t.z0 * w1 * t.z2, t2 = t.z0 * t.z1 * w2;
  const float den = fmaxf(t0 + t1 + t2, kEps);
  p.c0 = t0 / den; p.c1 = t1 / den; p.c2 = t2 / den;
  p.inside = p.c0 > 0.f && p.c1 > 0.f && p.c2 > 0.f;
  p.pz = p.c0 * t.z0 + p.c1 * t.z1 + p.c2 * t.z2;
  return p;
}

__device__ __forceinline__ float min_edge_d2(const Tri& t, float px, float py) {
  const float d01 = seg_d2(px, py, t.x0, t.y0, t.x1, t.y1);
  const float d02 = seg_d2(px, py, t.x0, t.y0, t.x2, t.y2);
  const float d12 = seg_d2(px, py, t.x1, t.y1, t.x2, t.y2);
  return fminf(d01, fminf(d02, d12));
}

// true: some barycentric comes out <= 0 for certain (see the header comment), false: evaluate the pair
__device__ __forceinline__ bool surely_outside(const Tri& t, float px, float py) {
  if (!(t.z0 > 0.f && t.z1 > 0.f && t.z2 > 0.f)) return false;
  const float area = edge_fn(t.x2, t.y2, t.x0, t.y0, t.x1, t.y1) + kEps;
  const float e0 = edge_fn(px, py, t.x1, t.y1, t.x2, t.y2), e1 = edge_fn(px, py, t.x2, t.y2, t.x0, t.y0),
              e2 = edge_fn(px, py, t.x0, t.y0, t.x1, t.y1);
  if (area > 0.f) return e0 < 0.f || e1 < 0.f || e2 < 0.f;
  if (area < 0.f) return e0 > 0.f || e1 > 0.f || e2 > 0.f;
  return false;
}

struct NormalArgs {
  const FaceRec* recs; const float4* bbs; const int32_t* bins; const int32_t* bin_count;
  const float* vnormals; const int32_t* faces; const float* nmap; const float* verts_uvs; const int32_t* faces_uvs;
  long long nmap_frame_stride;
  int B, V, F, S, nsx, K, Ht, Wt;
  float inv_sigma, inv_gamma, znear, zfar, bg0, bg1, bg2;
  float* out;
};

__global__ void __launch_bounds__(256) normal_image_kernel(NormalArgs A) {
  __shared__ float4 s_a[kChunk], s_b[kChunk], s_bb[kChunk];
  __shared__ float s_z2[kChunk];
  __shared__ int s_f[kChunk];
  __shared__ int s_wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = A.S, K = A.K, b = blockIdx.z;
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  const int xi = tx0 + (tid & 15), yi = ty0 + (tid >> 4);
  const bool valid = xi < S && yi < S;
  const float px = pix_to_ndc(xi, S), py = pix_to_ndc(yi, S);
  // NDC range of the tile's pixel centres (pix_to_ndc decreases with the index)
  const float txmax = pix_to_ndc(tx0, S), txmin = pix_to_ndc(min(tx0 + kTile - 1, S - 1), S);
  const float tymax = pix_to_ndc(ty0, S), tymin = pix_to_ndc(min(ty0 + kTile - 1, S - 1), S);
  const int nst = A.nsx * A.nsx;
  const int st = (ty0 / kSuper) * A.nsx + (tx0 / kSuper);
  const int n = A.bin_count[b * nst + st];
  const int32_t* list = A.bins + ((size_t)b * nst + st) * A.F;
  const FaceRec* rb = A.recs + (size_t)b * A.F;
  const float4* bbb = A.bbs + (size_t)b * A.F;

  const float kInf = __int_as_float(0x7f800000);
  float kz[kMaxK];
  int kf[kMaxK];
#pragma unroll
  for (int i = 0; i < kMaxK; ++i) { kz[i] = kInf; kf[i] = -1; }

  for (int e0 = 0; e0 < n; e0 += kChunk) {
    const int e = e0 + tid;
    bool hit = false;
    int f = 0;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < n) {
      f = list[e];
      q = bbb[f];
      hit = !(txmin > q.y || txmax < q.x || tymin > q.w || tymax < q.z);
    }
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int c = s_wcnt[w]; base += w < wave ? c : 0; total += c; }
    if (hit) {
      const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
      const FaceRec* r = rb + f;
      s_a[pos] = r->a; s_b[pos] = r->b; s_z2[pos] = r->c.x; s_bb[pos] = q; s_f[pos] = f;
    }
    __syncthreads();
    if (valid) {
      for (int j = 0; j < total; ++j) {
        const float4 bb = s_bb[j];
        if (px > bb.y || px < bb.x || py > bb.w || py < bb.z) continue;
        const float4 a = s_a[j], c = s_b[j];
        Tri t;
        t.x0 = a.x; t.y0 = a.y; t.z0 = a.z; t.x1 = a.w; t.y1 = c.x; t.z1 = c.y; t.x2 = c.z; t.y2 = c.w; t.z2 = s_z2[j];
        if (surely_outside(t, px, py)) continue;
        const Pair p = eval_pair(t, px, py);
        if (p.pz < 0.f || !p.inside) continue;
        // sorted insert into the first K slots: the new fragment goes in front of the first strictly deeper one, the rest move down
        // and the K-th falls out; slots K.. stay empty (+inf)
        float cz = p.pz;
        int cf = s_f[j];
        bool moving = false;
#pragma unroll
        for (int i = 0; i < kMaxK; ++i) {
          const bool sw = i < K && (moving || cz < kz[i]);
          const float oz = kz[i];
          const int of = kf[i];
          kz[i] = sw ? cz : oz; kf[i] = sw ? cf : of;
          cz = sw ? oz : cz; cf = sw ? of : cf;
          moving = moving || sw;
        }
      }
    }
    __syncthreads();
  }
  if (!valid) return;

  float* o = A.out + (((size_t)b * S + yi) * S + xi) * 4;
  if (kf[0] < 0) {                       // softmax_rgb_blend without a fragment: delta = 1, (0 + 1 * bg) / (0 + 1), alpha = 1 - 1
    *(float4*)o = make_float4(A.bg0, A.bg1, A.bg2, 0.f);
    return;
  }
  const float eps = 1e-10f;
  const float zspan = A.zfar - A.znear;
  // the slots ascend in depth, so the first one holds max z_inv (the empty slots' 0 never exceeds the clamp)
  const float zmax = fmaxf((A.zfar - kz[0]) / zspan, eps);
  const float delta = fmaxf(expf((eps - zmax) * A.inv_gamma), eps);
  float wsum = 0.f, r0 = 0.f, r1 = 0.f, r2 = 0.f, keep = 1.f;
  const float* vn = A.vnormals + (size_t)b * A.V * 3;
  const float* nmap = A.nmap ? A.nmap + (size_t)b * A.nmap_frame_stride : nullptr;
  for (int k = 0; k < K; ++k) {
    const int f = kf[0];
    if (f < 0) break;
    const float z = kz[0];
#pragma unroll
    for (int i = 0; i + 1 < kMaxK; ++i) { kz[i] = kz[i + 1]; kf[i] = kf[i + 1]; }     // next slot to the front: no dynamic register index
    kf[kMaxK - 1] = -1;
    const Tri t = load_tri(rb + f);
    const Pair p = eval_pair(t, px, py);
    const float d2 = min_edge_d2(t, px, py);              // inside the face: dists = -d2, prob = sigmoid(d2 / sigma)
    const int i0 = A.faces[3 * f], i1 = A.faces[3 * f + 1], i2 = A.faces[3 * f + 2];
    V3 nrm = ld(vn + 3 * i0) * p.c0 + ld(vn + 3 * i1) * p.c1 + ld(vn + 3 * i2) * p.c2;
    if (nmap) {
      const int u0 = A.faces_uvs[3 * f], u1 = A.faces_uvs[3 * f + 1], u2 = A.faces_uvs[3 * f + 2];
      const float u = p.c0 * A.verts_uvs[2 * u0] + p.c1 * A.verts_uvs[2 * u1] + p.c2 * A.verts_uvs[2 * u2];
      const float v = p.c0 * A.verts_uvs[2 * u0 + 1] + p.c1 * A.verts_uvs[2 * u1 + 1] + p.c2 * A.verts_uvs[2 * u2 + 1];
      const Bil bs = bil_setup(u, v, A.Wt, A.Ht);
      const V3 m = bil_sample(nmap, bs, A.Wt, A.Ht, nullptr, nullptr);
      // compute_tangent + apply_normal_map (pbr_materials.py:58-124)
      const float s = nrm.z >= 0.f ? 1.f : -1.f;
      const float a = -1.f / (s + nrm.z);
      const float bxy = nrm.x * nrm.y * a;
      const V3 tu = mk(1.f + s * nrm.x * nrm.x * a, s * bxy, -s * nrm.x);
      const V3 tv = mk(bxy, s + nrm.y * nrm.y * a, -nrm.y);
      const V3 np = tu * (-m.x) + tv * (-m.y) + nrm * m.z;
      nrm = np * (1.f / fmaxf(sqrtf(dot(np, np)), 1e-12f));
    }
    const float c0 = (nrm.x + 1.f) * 0.5f, c1 = (1.f - nrm.y) * 0.5f, c2 = (1.f - nrm.z) * 0.5f;
    const float prob = 1.f / (1.f + expf(-d2 * A.inv_sigma));
    const float w = prob * expf(((A.zfar - z) / zspan - zmax) * A.inv_gamma);
    wsum += w; r0 += w * c0; r1 += w * c1; r2 += w * c2;
    keep *= 1.f - prob;
  }
  const float inv = 1.f / (wsum + delta);
  *(float4*)o = make_float4((r0 + delta * A.bg0) * inv, (r1 + delta * A.bg1) * inv, (r2 + delta * A.bg2) * inv, 1.f - keep);
}

struct PanelArgs {
  const float* img[3];
  long long sn[3], sy[3], sx[3], sc[3];
  const float* mask_true; const float* mask_pred;
  int n_img, P, N, H, W;
  unsigned char* out;
};

__device__ __forceinline__ unsigned colour_u8(float x) {          // uint8(trunc(clip(x, 0, 1) * 255)), the product in float32
  return (unsigned)(int)__fmul_rn(fminf(fmaxf(x, 0.f), 1.f), 255.f);
}
__device__ __forceinline__ unsigned overlay_u8(float m) {         // uint8(trunc(float64(m) * 225)); outside [0, 255]: saturates
  const double v = (double)m * 225.0;
  return v >= 255.0 ? 255u : (v > 0.0 ? (unsigned)(int)v : 0u);
}

// one lane = 4 neighbouring pixels of one panel row = 12 output bytes (three aligned 32-bit stores when W is a multiple of 4)
__global__ void __launch_bounds__(256) panels_u8_kernel(PanelArgs A) {
  const int gpr = (A.W + 3) / 4;                                    // groups per panel row
  const long long total = (long long)A.N * A.H * A.P * gpr;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int g = (int)(i % gpr);
  const int p = (int)((i / gpr) % A.P);
  const int y = (int)((i / ((long long)gpr * A.P)) % A.H);
  const int nimg = (int)(i / ((long long)gpr * A.P * A.H));
  const int x0 = 4 * g, npx = min(4, A.W - x0);
  // (the panel's pointer and strides picked with constant indices: a run-time index into the argument arrays would go through scratch)
  const bool colour = p < A.n_img;
  const float* ip = p == 0 ? A.img[0] : p == 1 ? A.img[1] : A.img[2];
  const long long sn = p == 0 ? A.sn[0] : p == 1 ? A.sn[1] : A.sn[2], sy = p == 0 ? A.sy[0] : p == 1 ? A.sy[1] : A.sy[2];
  const long long sx = p == 0 ? A.sx[0] : p == 1 ? A.sx[1] : A.sx[2], sc = p == 0 ? A.sc[0] : p == 1 ? A.sc[1] : A.sc[2];
  unsigned v[12];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned c0 = 0, c1 = 0, c2 = 0;
    if (k < npx) {
      const int x = x0 + k;
      if (colour) {
        const float* s = ip + nimg * sn + y * sy + x * sx;
        c0 = colour_u8(s[0]); c1 = colour_u8(s[sc]); c2 = colour_u8(s[2 * sc]);
      } else {
        const size_t m = ((size_t)nimg * A.H + y) * A.W + x;
        c0 = overlay_u8(A.mask_true[m]); c2 = overlay_u8(A.mask_pred[m]);
      }
    }
    v[3 * k] = c0; v[3 * k + 1] = c1; v[3 * k + 2] = c2;
  }
  unsigned char* o = A.out + ((((size_t)nimg * A.H + y) * A.P + p) * A.W + x0) * 3;
  if ((A.W & 3) == 0) {
    unsigned* o4 = (unsigned*)o;
#pragma unroll
    for (int k = 0; k < 3; ++k) o4[k] = v[4 * k] | (v[4 * k + 1] << 8) | (v[4 * k + 2] << 16) | (v[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < 3 * npx) o[k] = (unsigned char)v[k];
  }
}

}  // namespace

extern "C" {

int harp_normal_image(const float* ndc, const float* vnormals, const int32_t* faces, int B, int V, int F, int S, int K, float sigma, float gamma,
                      float znear, float zfar, const float* background, const float* nmap, long long nmap_frame_stride, int Ht, int Wt,
                      const float* verts_uvs, const int32_t* faces_uvs, void* ws, float* out, hipStream_t stream) {
  if (!ndc || !vnormals || !faces || !background || !ws || !out || B <= 0 || B > 65535 || V <= 0 || F <= 0 || S <= 0 || K < 1 || K > kMaxK ||
      !(sigma > 0.f) || !(gamma > 0.f) || !(zfar > znear))
    return HARP_ERR_ARG;
  if (nmap && (!verts_uvs || !faces_uvs || Ht <= 0 || Wt <= 0 || nmap_frame_stride < 0)) return HARP_ERR_ARG;
  const int rc = harp_detail_raster_setup(ndc, faces, B, V, F, S, 0.f, ws, stream);
  if (rc != HARP_OK) return rc;
  const RasterWs W = raster_ws_split(ws, B, F, S);
  NormalArgs A;
  A.recs = W.recs; A.bbs = W.bbs; A.bins = W.bins; A.bin_count = W.cnt;
  A.vnormals = vnormals; A.faces = faces; A.nmap = nmap; A.verts_uvs = verts_uvs; A.faces_uvs = faces_uvs;
  A.nmap_frame_stride = nmap_frame_stride;
  A.B = B; A.V = V; A.F = F; A.S = S; A.nsx = W.nsx; A.K = K; A.Ht = Ht; A.Wt = Wt;
  A.inv_sigma = 1.f / sigma; A.inv_gamma = 1.f / gamma; A.znear = znear; A.zfar = zfar;
  A.bg0 = background[0]; A.bg1 = background[1]; A.bg2 = background[2];
  A.out = out;
  hipLaunchKernelGGL(normal_image_kernel, dim3((S + kTile - 1) / kTile, (S + kTile - 1) / kTile, B), dim3(256), 0, stream, A);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

int harp_panels_u8(const float* const* images, const long long* strides, int n_images, const float* mask_true, const float* mask_pred, int N,
                   int H, int W, unsigned char* out, hipStream_t stream) {
  if (!out || n_images < 0 || n_images > 3 || (n_images > 0 && (!images || !strides)) || (mask_true == nullptr) != (mask_pred == nullptr) ||
      N <= 0 || H <= 0 || W <= 0)
    return HARP_ERR_ARG;
  PanelArgs A;
  for (int k = 0; k < 3; ++k) {
    A.img[k] = nullptr; A.sn[k] = A.sy[k] = A.sx[k] = A.sc[k] = 0;
    if (k < n_images) {
      if (!images[k]) return HARP_ERR_ARG;
      A.img[k] = images[k];
      A.sn[k] = strides[4 * k]; A.sy[k] = strides[4 * k + 1]; A.sx[k] = strides[4 * k + 2]; A.sc[k] = strides[4 * k + 3];
      if (A.sn[k] < 0 || A.sy[k] < 0 || A.sx[k] < 0 || A.sc[k] < 0) return HARP_ERR_ARG;
    }
  }
  A.mask_true = mask_true; A.mask_pred = mask_pred;
  A.n_img = n_images; A.P = n_images + (mask_true ? 1 : 0); A.N = N; A.H = H; A.W = W; A.out = out;
  if (A.P == 0) return HARP_ERR_ARG;
  const long long total = (long long)N * H * A.P * ((W + 3) / 4);
  if ((total + 255) / 256 > 0x7fffffffLL) return HARP_ERR_ARG;
  hipLaunchKernelGGL(panels_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, A);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

}  // extern "C"
