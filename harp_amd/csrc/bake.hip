// The frames baked into UV space: a map from the atlas back to the video.  The reference starts every fit from one flat
// skin colour (optimize_sequence.py:234), writes the fitted texture multiplied by uv_mask (:627-654) and exports it as it is (:776-791);
// nothing there tells which texels a frame ever saw.  Four forward-only kernels, off the fitting step's path:
//
//   harp_uv_texel_map       the UV triangles rasterised at the texel centres of the atlas: owning face (lowest index) + barycentrics
//   harp_texture_bake_accum per covered texel and frame: where the texel is seen (perspective-correct from the vertex NDC alone), whether it
//                           is seen there (hard raster's face_id / zbuf, eroded mask, viewing angle), the target colour there (bilinear),
//                           divided by the Lambert shading; weighted sums in float64, frames added IN FRAME ORDER by the texel's one thread
//   harp_texture_bake_finish  mean, variance, seen
//   harp_texture_dilate     3 x 3 Jacobi fill of invalid texels from valid neighbours, one launch per pass
//
// Design: one thread per texel everywhere (68 k covered texels of a 512^2 hand atlas = about one wave per SIMD of the 256 CUs; the work is
// gathers, not arithmetic).  A texel's accumulators are read once, kept in registers over the B frames of the call and written once, so the
// sums do not depend on how a sequence is cut into calls and no atomics are needed.  Splitting the frames of a call over more threads would
// need a second ordered pass over partial sums for the same bits; at ~20 gathers per (texel, frame) against an epoch of renders it is not
// worth it.  The per-(texel, frame) arithmetic is float64: every accept / reject test is then decided far inside the
// margins the float64 restatement (tests/_bake_ref.py) treats as undecidable.
// The only atomic is the integer atomicMin of the texel map (order-independent).  Every index read from memory (texel list, face, vertex,
// target row) is range-checked before it is used as an address.
#include "harp_common.h"
#include "harp_hip.h"

namespace {

constexpr int kNoFace = 0x7fffffff;

struct UvTri { float x0, y0, x1, y1, x2, y2, area; bool ok; };

// texel-space corners of UV face f: tx = u (Wt - 1), ty = (1 - v) (Ht - 1) — where bil_setup (shade_common.h) puts an integer sample
__device__ __forceinline__ UvTri uv_tri(const float* __restrict__ verts_uvs, const int32_t* __restrict__ faces_uvs, int f, int VT, int Ht, int Wt) {
  UvTri t;
  t.ok = false;
  const int i0 = faces_uvs[3 * (size_t)f], i1 = faces_uvs[3 * (size_t)f + 1], i2 = faces_uvs[3 * (size_t)f + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= VT || i1 >= VT || i2 >= VT) return t;
  const float sx = (float)(Wt - 1), sy = (float)(Ht - 1);
  t.x0 = verts_uvs[2 * (size_t)i0] * sx; t.y0 = (1.0f - verts_uvs[2 * (size_t)i0 + 1]) * sy;
  t.x1 = verts_uvs[2 * (size_t)i1] * sx; t.y1 = (1.0f - verts_uvs[2 * (size_t)i1 + 1]) * sy;
  t.x2 = verts_uvs[2 * (size_t)i2] * sx; t.y2 = (1.0f - verts_uvs[2 * (size_t)i2 + 1]) * sy;
  t.area = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0);
  t.ok = fabsf(t.area) > 0.f && fabsf(t.area) < INFINITY;          // zero-area and non-finite faces own nothing
  return t;
}

// edge functions of texel centre (px, py), formed from the corner - centre differences: e_i / area = barycentric i
__device__ __forceinline__ void uv_edges(const UvTri& t, float px, float py, float& e0, float& e1, float& e2) {
  const float ax = t.x0 - px, ay = t.y0 - py, bx = t.x1 - px, by = t.y1 - py, cx = t.x2 - px, cy = t.y2 - py;
  e0 = bx * cy - by * cx;
  e1 = cx * ay - cy * ax;
  e2 = ax * by - ay * bx;
}

__global__ void __launch_bounds__(256) texel_map_clear_kernel(int32_t* __restrict__ texel_face, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) texel_face[i] = kNoFace;
}

// one wave per face: its lanes walk the texel centres of the face's bounding box, clipped to the atlas
__global__ void __launch_bounds__(256) texel_map_faces_kernel(const float* __restrict__ verts_uvs, const int32_t* __restrict__ faces_uvs, int F, int VT,
                                                              int Ht, int Wt, int32_t* __restrict__ texel_face) {
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (f >= F) return;
  const UvTri t = uv_tri(verts_uvs, faces_uvs, f, VT, Ht, Wt);
  if (!t.ok) return;
  const float xmin = fminf(t.x0, fminf(t.x1, t.x2)), xmax = fmaxf(t.x0, fmaxf(t.x1, t.x2));
  const float ymin = fminf(t.y0, fminf(t.y1, t.y2)), ymax = fmaxf(t.y0, fmaxf(t.y1, t.y2));
  if (!(xmax >= 0.f && ymax >= 0.f && xmin <= (float)(Wt - 1) && ymin <= (float)(Ht - 1))) return;
  const int x0 = (int)floorf(fmaxf(xmin, 0.f)), x1 = (int)ceilf(fminf(xmax, (float)(Wt - 1)));
  const int y0 = (int)floorf(fmaxf(ymin, 0.f)), y1 = (int)ceilf(fminf(ymax, (float)(Ht - 1)));
  const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
  const float sg = t.area > 0.f ? 1.f : -1.f;
  for (long long i = lane; i < (long long)bw * bh; i += 64) {
    const int y = y0 + (int)(i / bw), x = x0 + (int)(i % bw);
    float e0, e1, e2;
    uv_edges(t, (float)x, (float)y, e0, e1, e2);
    if (e0 * sg >= 0.f && e1 * sg >= 0.f && e2 * sg >= 0.f) atomicMin(&texel_face[(size_t)y * Wt + x], f);
  }
}

__global__ void __launch_bounds__(256) texel_map_bary_kernel(const float* __restrict__ verts_uvs, const int32_t* __restrict__ faces_uvs, int VT, int Ht,
                                                             int Wt, int32_t* __restrict__ texel_face, float* __restrict__ texel_bary) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Ht * Wt) return;
  const int f = texel_face[i];
  float b0 = 0.f, b1 = 0.f;
  if (f == kNoFace) {
    texel_face[i] = -1;
  } else {
    const UvTri t = uv_tri(verts_uvs, faces_uvs, f, VT, Ht, Wt);
    float e0, e1, e2;
    uv_edges(t, (float)(i % Wt), (float)(i / Wt), e0, e1, e2);
    b0 = __fdiv_rn(e0, t.area); b1 = __fdiv_rn(e1, t.area);
  }
  texel_bary[2 * (size_t)i] = b0; texel_bary[2 * (size_t)i + 1] = b1;
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ld3(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ D3 mix3(const D3& a, const D3& b, const D3& c, double b0, double b1, double b2) {
  return {b0 * a.x + b1 * b.x + b2 * c.x, b0 * a.y + b1 * b.y + b2 * c.y, b0 * a.z + b1 * b.z + b2 * c.z};
}
__device__ __forceinline__ double dot3(const D3& a, const D3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// a / max(|a|, 1e-6): the shader's normalisation (shade.hip)
__device__ __forceinline__ D3 unit3(const D3& a) {
  const double r = 1.0 / fmax(sqrt(dot3(a, a)), 1e-6);
  return {a.x * r, a.y * r, a.z * r};
}

__global__ void __launch_bounds__(256) bake_accum_kernel(harp_bake_args A) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= A.n) return;
  const int t = A.texel_idx ? A.texel_idx[j] : j;
  if (t < 0 || t >= A.Ht * A.Wt) return;
  const int f = A.texel_face[t];
  if (f < 0 || f >= A.F) return;
  const int i0 = A.faces[3 * (size_t)f], i1 = A.faces[3 * (size_t)f + 1], i2 = A.faces[3 * (size_t)f + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= A.V || i1 >= A.V || i2 >= A.V) return;
  const double b0 = (double)A.texel_bary[2 * (size_t)t], b1 = (double)A.texel_bary[2 * (size_t)t + 1], b2 = 1.0 - b0 - b1;
  const int S = A.S;
  const double half = 0.5 * (double)S;
  const bool angle = A.vnormals != nullptr, delight = A.light_pos != nullptr;

  double sw = A.sum_w[t];
  double sc[3], sc2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { sc[c] = A.sum_wc[3 * (size_t)t + c]; sc2[c] = A.sum_wc2[3 * (size_t)t + c]; }
  int cnt = A.count[t];
  float best = A.best_cos[t];

  for (int k = 0; k < A.B; ++k) {
    const int row = A.rows[k];
    if (row < 0 || row >= A.N) continue;
    const float* nd = A.ndc + (size_t)k * A.V * 3;
    const D3 p0 = ld3(nd + 3 * (size_t)i0), p1 = ld3(nd + 3 * (size_t)i1), p2 = ld3(nd + 3 * (size_t)i2);
    const double z = b0 * p0.z + b1 * p1.z + b2 * p2.z;
    if (!(z > 0.0)) continue;
    const double x = (b0 * p0.x * p0.z + b1 * p1.x * p1.z + b2 * p2.x * p2.z) / z;
    const double y = (b0 * p0.y * p0.z + b1 * p1.y * p1.z + b2 * p2.y * p2.z) / z;
    const double fx = (1.0 - x) * half, fy = (1.0 - y) * half;     // pixel i covers [i, i + 1): the inverse of pix_to_ndc
    if (!(fx >= 0.0 && fx < (double)S && fy >= 0.0 && fy < (double)S)) continue;
    const int ix = (int)floor(fx), iy = (int)floor(fy);
    const size_t pix = ((size_t)k * S + iy) * S + ix;
    if (A.face_id[pix] < 0) continue;
    if (!(z <= (double)A.zbuf[pix] * (1.0 + (double)A.depth_tol))) continue;
    if (!(A.y_mask[((size_t)row * S + iy) * S + ix] >= 0.5f)) continue;
    double cosv = 1.0, shade[3] = {1.0, 1.0, 1.0}, spec[3] = {0.0, 0.0, 0.0};
    if (angle) {
      const float* vn = A.vnormals + (size_t)k * A.V * 3;
      const float* vw = A.verts + (size_t)k * A.V * 3;
      const D3 nh = unit3(mix3(ld3(vn + 3 * (size_t)i0), ld3(vn + 3 * (size_t)i1), ld3(vn + 3 * (size_t)i2), b0, b1, b2));
      const D3 pw = mix3(ld3(vw + 3 * (size_t)i0), ld3(vw + 3 * (size_t)i1), ld3(vw + 3 * (size_t)i2), b0, b1, b2);
      const D3 cp = ld3(A.cam_pos + 3 * (size_t)k);
      cosv = dot3(nh, unit3({cp.x - pw.x, cp.y - pw.y, cp.z - pw.z}));
      if (!(cosv >= (double)A.cos_min)) continue;
      if (delight) {
        const D3 lp = ld3(A.light_pos + 3 * (size_t)k);
        const double cosl = fmax(dot3(nh, unit3({lp.x - pw.x, lp.y - pw.y, lp.z - pw.z})), 0.0);
        const float* col = A.colors + 9 * (size_t)k;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          shade[c] = fmax((double)col[c] + (double)col[3 + c] * cosl, (double)A.shade_floor);
          spec[c] = (double)col[6 + c];               // shininess 0: a constant (0 in the fit's shadow renderer)
        }
      }
    }
    const double cw = fmax(cosv, 0.0);
    const double w = !angle ? 1.0 : (A.cos_power == 2.0f ? cw * cw : pow(cw, (double)A.cos_power));
    // bilinear sample of the target at the continuous pixel coordinate, clamped to the image
    const double cx = fmin(fmax(fx - 0.5, 0.0), (double)(S - 1)), cy = fmin(fmax(fy - 0.5, 0.0), (double)(S - 1));
    const int x0 = (int)floor(cx), y0 = (int)floor(cy), x1 = min(x0 + 1, S - 1), y1 = min(y0 + 1, S - 1);
    const double wx = cx - (double)x0, wy = cy - (double)y0;
    const float* img = A.y_true + (size_t)row * S * S * 3;
    const float* q00 = img + ((size_t)y0 * S + x0) * 3; const float* q01 = img + ((size_t)y0 * S + x1) * 3;
    const float* q10 = img + ((size_t)y1 * S + x0) * 3; const float* q11 = img + ((size_t)y1 * S + x1) * 3;
    sw += w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double top = (1.0 - wx) * (double)q00[c] + wx * (double)q01[c], bot = (1.0 - wx) * (double)q10[c] + wx * (double)q11[c];
      const double v = ((1.0 - wy) * top + wy * bot - spec[c]) / shade[c];
      sc[c] += w * v; sc2[c] += w * v * v;
    }
    cnt += 1;
    best = fmaxf(best, (float)cosv);
  }

  A.sum_w[t] = sw;
#pragma unroll
  for (int c = 0; c < 3; ++c) { A.sum_wc[3 * (size_t)t + c] = sc[c]; A.sum_wc2[3 * (size_t)t + c] = sc2[c]; }
  A.count[t] = cnt;
  A.best_cos[t] = best;
}

__global__ void __launch_bounds__(256) bake_finish_kernel(const double* __restrict__ sum_w, const double* __restrict__ sum_wc,
                                                          const double* __restrict__ sum_wc2, const int32_t* __restrict__ count, int n, int min_count,
                                                          float* __restrict__ mean, float* __restrict__ var, unsigned char* __restrict__ seen) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const double w = sum_w[t];
  const bool ok = count[t] >= min_count && w > 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float m = 0.f, v = 0.f;
    if (ok) {
      const double mu = sum_wc[3 * (size_t)t + c] / w;
      m = (float)fmin(fmax(mu, 0.0), 1.0);
      v = (float)fmax(sum_wc2[3 * (size_t)t + c] / w - mu * mu, 0.0);
    }
    mean[3 * (size_t)t + c] = m;
    if (var) var[3 * (size_t)t + c] = v;
  }
  seen[t] = ok ? 1 : 0;
}

// one Jacobi pass src -> dst (never the same buffers)
__global__ void __launch_bounds__(256) dilate_pass_kernel(const float* __restrict__ src, const unsigned char* __restrict__ vsrc,
                                                          const unsigned char* __restrict__ allow, int Ht, int Wt, int C, float* __restrict__ dst,
                                                          unsigned char* __restrict__ vdst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Ht * Wt) return;
  const int y = i / Wt, x = i - y * Wt;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int n = 0;
  const bool was = vsrc[i] != 0;
  if (!was && (!allow || allow[i])) {
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if ((dy == 0 && dx == 0) || yy < 0 || yy >= Ht || xx < 0 || xx >= Wt) continue;
        const int q = yy * Wt + xx;
        if (!vsrc[q] || (allow && !allow[q])) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < C) acc[c] += src[(size_t)q * C + c];
        ++n;
      }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < C) dst[(size_t)i * C + c] = n > 0 ? __fdiv_rn(acc[c], (float)n) : src[(size_t)i * C + c];
  vdst[i] = (was || n > 0) ? 1 : 0;
}

size_t round256(size_t n) { return (n + 255) / 256 * 256; }
bool atlas_fits(int Ht, int Wt, int C) { return (long long)Ht * Wt * C <= 0x7fffffffLL - 256; }     // the kernels' int texel arithmetic

}  // namespace

extern "C" {

int harp_uv_texel_map(const float* verts_uvs, const int32_t* faces_uvs, int F, int VT, int Ht, int Wt, int32_t* texel_face, float* texel_bary,
                      hipStream_t stream) {
  if (!verts_uvs || !faces_uvs || !texel_face || !texel_bary || F < 1 || VT < 1 || Ht < 2 || Wt < 2 || !atlas_fits(Ht, Wt, 1)) return HARP_ERR_ARG;
  const int n = Ht * Wt;
  hipLaunchKernelGGL(texel_map_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, texel_face, n);
  HARP_CHECK_LAUNCH();
  hipLaunchKernelGGL(texel_map_faces_kernel, dim3((F + 3) / 4), dim3(256), 0, stream, verts_uvs, faces_uvs, F, VT, Ht, Wt, texel_face);
  HARP_CHECK_LAUNCH();
  hipLaunchKernelGGL(texel_map_bary_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, verts_uvs, faces_uvs, VT, Ht, Wt, texel_face, texel_bary);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

int harp_texture_bake_accum(const harp_bake_args* a, hipStream_t stream) {
  if (!a) return HARP_ERR_ARG;
  if (!a->texel_face || !a->texel_bary || !a->faces || !a->ndc || !a->face_id || !a->zbuf || !a->y_true || !a->y_mask || !a->rows || !a->sum_w ||
      !a->sum_wc || !a->sum_wc2 || !a->count || !a->best_cos)
    return HARP_ERR_ARG;
  if (a->n < 1 || a->Ht < 2 || a->Wt < 2 || a->F < 1 || a->V < 1 || a->B < 1 || a->S < 1 || a->N < 1 || !atlas_fits(a->Ht, a->Wt, 1)) return HARP_ERR_ARG;
  if (!a->texel_idx && a->n != a->Ht * a->Wt) return HARP_ERR_ARG;
  // the viewing angle needs normals, positions and the camera centre together; the de-lighting needs those and light + colours together
  const int n_angle = (a->verts != nullptr) + (a->vnormals != nullptr) + (a->cam_pos != nullptr);
  const int n_light = (a->light_pos != nullptr) + (a->colors != nullptr);
  if ((n_angle != 0 && n_angle != 3) || (n_light != 0 && n_light != 2) || (n_light == 2 && n_angle != 3)) return HARP_ERR_ARG;
  if (!(a->depth_tol >= 0.f) || !(a->shade_floor > 0.f) || !(a->cos_power >= 0.f) || !(a->cos_min >= -1.f)) return HARP_ERR_ARG;
  hipLaunchKernelGGL(bake_accum_kernel, dim3((a->n + 255) / 256), dim3(256), 0, stream, *a);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

int harp_texture_bake_finish(const double* sum_w, const double* sum_wc, const double* sum_wc2, const int32_t* count, int Ht, int Wt, int min_count,
                             float* mean, float* var, unsigned char* seen, hipStream_t stream) {
  if (!sum_w || !sum_wc || !sum_wc2 || !count || !mean || !seen || Ht < 1 || Wt < 1 || !atlas_fits(Ht, Wt, 3)) return HARP_ERR_ARG;
  const int n = Ht * Wt;
  hipLaunchKernelGGL(bake_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, sum_w, sum_wc, sum_wc2, count, n, min_count, mean, var, seen);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

size_t harp_texture_dilate_ws_bytes(int Ht, int Wt, int C) {
  if (Ht < 1 || Wt < 1 || C < 1 || C > 4 || !atlas_fits(Ht, Wt, C)) return 0;
  return 2 * round256((size_t)Ht * Wt * C * sizeof(float)) + 2 * round256((size_t)Ht * Wt);
}

int harp_texture_dilate(const float* tex, const unsigned char* valid, const unsigned char* allow, int Ht, int Wt, int C, int n_pass, float* out,
                        unsigned char* valid_out, void* ws, hipStream_t stream) {
  if (!tex || !valid || !out || Ht < 1 || Wt < 1 || C < 1 || C > 4 || n_pass < 0 || !atlas_fits(Ht, Wt, C)) return HARP_ERR_ARG;
  if (n_pass > 0 && !ws) return HARP_ERR_ARG;
  const size_t tb = (size_t)Ht * Wt * C * sizeof(float), vb = (size_t)Ht * Wt;
  const float* src = tex;
  const unsigned char* vsrc = valid;
  if (n_pass > 0) {
    // tex -> a -> b -> a ...: every pass reads one buffer and writes the other, so `out` may be `tex` (copied into at the end)
    float* buf[2] = {(float*)ws, (float*)((char*)ws + round256(tb))};
    unsigned char* vbuf[2] = {(unsigned char*)ws + 2 * round256(tb), (unsigned char*)ws + 2 * round256(tb) + round256(vb)};
    const dim3 grid((Ht * Wt + 255) / 256);
    for (int pass = 0; pass < n_pass; ++pass) {
      hipLaunchKernelGGL(dilate_pass_kernel, grid, dim3(256), 0, stream, src, vsrc, allow, Ht, Wt, C, buf[pass & 1], vbuf[pass & 1]);
      HARP_CHECK_LAUNCH();
      src = buf[pass & 1]; vsrc = vbuf[pass & 1];
    }
  }
  if (src != out) {
    const hipError_t e = hipMemcpyAsync(out, src, tb, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return HARP_ERR_LAUNCH + (int)e;
  }
  if (valid_out && vsrc != valid_out) {
    const hipError_t e = hipMemcpyAsync(valid_out, vsrc, vb, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return HARP_ERR_LAUNCH + (int)e;
  }
  return HARP_OK;
}

}  // extern "C"
