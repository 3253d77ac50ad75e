// Contact labels (harp_amd/playback/player.py ScenePlayer.contact): for every vertex of a QUERY mesh its unsigned distance
// to the surface of a TARGET mesh, the face that attains it and the generalised winding number of the target about it, per frame of a
// batch.  include/harp_hip.h states the contract; tests/_contact_ref.py restates it in float64.
//
// contact_setup_kernel: one lane per (frame, target face), one workgroup of kFaces lanes per chunk of kFaces faces.  It writes the face's
//   three view-space corners (after the flip) and a validity word as 12 floats into ws, and the chunk's bounding box over its valid faces
//   (an LDS min/max tree) as 8 floats.  A face with an index outside [0, V) or a non-finite corner is marked invalid and keeps out of
//   the box; its vertices are not read when an index is out of range.
// contact_kernel: one workgroup of four waves per tile of 64 query vertices of one frame; every wave holds the tile, one lane per vertex,
//   and takes every fourth chunk of the target (one wave per tile leaves a SIMD 1.5 waves: the dependent arithmetic of one pair is not
//   hidden).  Pass 1 walks the wave's chunks in ascending order.  A chunk is skipped when the gap between its box and the tile's box, less
//   a rounding margin, exceeds min(max_dist, the worst best distance of the wave's lanes); otherwise its 12-float records are copied into
//   the wave's 6 KiB of LDS and every lane runs the point-triangle distance on every valid face in registers: all lanes read the same
//   record, so the LDS reads are broadcasts.  A face replaces the lane's best only on a strictly smaller float32 distance; the four
//   waves' results meet in LDS, of equal distances the lower face: the lowest index wins a tie.  Pass 2, the winding sum, needs every
//   face: it runs over all chunks again, a quarter per wave, summed in a fixed order, and only for a tile where some lane's distance is
//   within max_dist (a workgroup-uniform branch).
// Point-triangle distance: the foot of the perpendicular when it falls inside the triangle (three edge-plane tests against the normal),
//   otherwise the nearest of the three point-segment distances.  Every term is built from differences against the face's own corners,
//   so a small triangle far from the point loses nothing; a zero-area face has a zero normal, fails the inside test and is measured as
//   its segments, a zero-length segment as its point.  No division by a zero is made.
// The cull is conservative: the boxes are exact float32 bounds of the very coordinates the distances are computed from, and the margin
//   (kCullMargin times the largest absolute box coordinate) is above the rounding of the gap and of a computed distance together, so a
//   skipped chunk holds no face that could have replaced, or tied with, any lane's result.  The outputs do not depend on the chunking.
// harp_mesh_contact_excl (self-contact) is the same two launches with contact_kernel<true>: a per-(query vertex, face) bit
//   table removes faces from a vertex's distance minimum; the winding sum stays over all faces.  The comment at the kernel says how.
// No atomics, no scratch, no allocation; every index is checked before it is used and all stores are per-lane vector stores.
#include "harp_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "harp_hip.h"

namespace {

constexpr int kFaces = 128;          // target faces per chunk: one box each, 128 * 48 B = 6 KiB of LDS when staged
constexpr int kRec = 12;             // floats per face record in ws and LDS: a, b, c, the validity word, two unused
constexpr int kBox = 8;              // floats per chunk box in ws: lo xyz, hi xyz, two unused
constexpr int kLanes = 64;            // query vertices per workgroup: one wave
// 64 * 2^-24: a computed distance is within 32 * 2^-24 M of the exact one (include/harp_hip.h) and the float32 gap between two boxes
// within a few 2^-24 M; M = the largest absolute coordinate of the two boxes
constexpr float kCullMargin = 3.8146973e-6f;
constexpr int kWaves = 4;            // waves per workgroup: all own the SAME 64 query vertices and share the target's chunks, wave w those with c % 4 == w
// below this a squared length (a segment's, or a face's normal's: 4 area^2) counts as zero, so that no reciprocal of a denormal is taken:
// the segment is measured as its first point, the face as its edges, either within 1e-15 m of the truth
constexpr float kTiny = 1e-30f;

// harp_project_fwd's view transform (csrc/mesh.hip) with the order of operations fixed, so that the query and the target side give the
// same bits for the same vertex; then the mirror
__device__ __forceinline__ void view_of(const float* __restrict__ p, const float* __restrict__ r, const float* __restrict__ t, bool flip,
                                        float& X, float& Y, float& Z) {
  const float x = p[0], y = p[1], z = p[2];
  X = __fmaf_rn(z, r[6], __fmaf_rn(y, r[3], __fmaf_rn(x, r[0], t[0])));
  Y = __fmaf_rn(z, r[7], __fmaf_rn(y, r[4], __fmaf_rn(x, r[1], t[1])));
  Z = __fmaf_rn(z, r[8], __fmaf_rn(y, r[5], __fmaf_rn(x, r[2], t[2])));
  if (flip) X = -X;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  const float inf = __builtin_inff();
  return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;          // (a NaN fails the comparison)
}

__global__ void __launch_bounds__(kFaces) contact_setup_kernel(const float* __restrict__ verts, const float* __restrict__ cam_R,
                                                               const float* __restrict__ cam_T, const int32_t* __restrict__ faces, int V,
                                                               int F, int n_chunks, int flip, float* __restrict__ boxes,
                                                               float* __restrict__ recs) {
  __shared__ float red[6][kFaces];
  const int b = blockIdx.x / n_chunks, c = blockIdx.x - b * n_chunks;
  const int f = c * kFaces + (int)threadIdx.x;
  const float inf = __builtin_inff();
  float v[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = 0.0f;
  bool ok = false;
  if (f < F) {
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
      const float* vb = verts + (size_t)b * V * 3;
      const float* r = cam_R + 9 * (size_t)b;
      const float* t = cam_T + 3 * (size_t)b;
      view_of(vb + 3 * (size_t)i0, r, t, flip != 0, v[0], v[1], v[2]);
      view_of(vb + 3 * (size_t)i1, r, t, flip != 0, v[3], v[4], v[5]);
      view_of(vb + 3 * (size_t)i2, r, t, flip != 0, v[6], v[7], v[8]);
      ok = finite3(v[0], v[1], v[2]) && finite3(v[3], v[4], v[5]) && finite3(v[6], v[7], v[8]);
    }
    float4* o = (float4*)(recs + ((size_t)b * F + f) * kRec);          // (ws is 16-byte aligned and the boxes in front are 32 B each)
    o[0] = make_float4(v[0], v[1], v[2], v[3]);
    o[1] = make_float4(v[4], v[5], v[6], v[7]);
    o[2] = make_float4(v[8], ok ? 1.0f : 0.0f, 0.0f, 0.0f);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    red[k][threadIdx.x] = ok ? fminf(v[k], fminf(v[3 + k], v[6 + k])) : inf;
    red[3 + k][threadIdx.x] = ok ? fmaxf(v[k], fmaxf(v[3 + k], v[6 + k])) : -inf;
  }
  __syncthreads();
  for (int s = kFaces / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + s]);
        red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < kBox) boxes[(size_t)blockIdx.x * kBox + threadIdx.x] = threadIdx.x < 6 ? red[threadIdx.x][0] : 0.0f;
}

__device__ __forceinline__ float wave_min(float x) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) x = fminf(x, __shfl_xor(x, s, 64));
  return x;
}

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) x = fmaxf(x, __shfl_xor(x, s, 64));
  return x;
}

// the same value in every lane, held in a scalar register: what a wave-uniform branch tests
__device__ __forceinline__ float uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

// squared distance from the point to the segment o + t d, t in [0, 1], given w = point - o; a zero-length segment is its point
__device__ __forceinline__ float seg_dist2(float wx, float wy, float wz, float dx, float dy, float dz) {
  const float dd = dx * dx + dy * dy + dz * dz;
  const float wd = wx * dx + wy * dy + wz * dz;
  // (v_rcp_f32, within 1 ulp: an error of t moves the foot ALONG the segment, which changes the distance in second order only)
  const float t = dd > kTiny ? fminf(fmaxf(wd * __builtin_amdgcn_rcpf(dd), 0.0f), 1.0f) : 0.0f;
  const float ex = wx - t * dx, ey = wy - t * dy, ez = wz - t * dz;
  return ex * ex + ey * ey + ez * ez;
}

// squared distance from p to the triangle (a, b, c)
__device__ __forceinline__ float tri_dist2(float px, float py, float pz, const float4 r0, const float4 r1, const float4 r2) {
  const float ax = r0.x, ay = r0.y, az = r0.z, bx = r0.w, by = r1.x, bz = r1.y, cx = r1.z, cy = r1.w, cz = r2.x;
  const float ux = bx - ax, uy = by - ay, uz = bz - az;               // ab
  const float vx = cx - ax, vy = cy - ay, vz = cz - az;               // ac
  const float ex = cx - bx, ey = cy - by, ez = cz - bz;               // bc
  const float wx = px - ax, wy = py - ay, wz = pz - az;               // ap
  const float qx = px - bx, qy = py - by, qz = pz - bz;               // bp
  // products rounded one by one (no fused multiply-add): equal corners give a normal that is exactly zero
  const float nx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
  const float ny = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
  const float nz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
  const float nn = nx * nx + ny * ny + nz * nz;
  // inside the three edge planes: n . (ab x ap), n . (bc x bp), n . (ca x cp) = n . (ap x ac), all >= 0
  const float s0 = nx * (uy * wz - uz * wy) + ny * (uz * wx - ux * wz) + nz * (ux * wy - uy * wx);
  const float s1 = nx * (ey * qz - ez * qy) + ny * (ez * qx - ex * qz) + nz * (ex * qy - ey * qx);
  const float s2 = nx * (wy * vz - wz * vy) + ny * (wz * vx - wx * vz) + nz * (wx * vy - wy * vx);
  const float h = nx * wx + ny * wy + nz * wz;
  float d2 = fminf(seg_dist2(wx, wy, wz, ux, uy, uz), fminf(seg_dist2(wx, wy, wz, vx, vy, vz), seg_dist2(qx, qy, qz, ex, ey, ez)));
  if (nn > kTiny && s0 >= 0.0f && s1 >= 0.0f && s2 >= 0.0f) d2 = fminf(d2, h * h * __builtin_amdgcn_rcpf(nn));      // (the plane is never farther than the edges)
  return d2;
}

// the signed solid angle of (a, b, c) about p over 2, van Oosterom-Strackee; exactly 0 for a face whose normal is exactly zero
__device__ __forceinline__ float tri_half_angle(float px, float py, float pz, const float4 r0, const float4 r1, const float4 r2) {
  const float ax = r0.x - px, ay = r0.y - py, az = r0.z - pz;
  const float bx = r0.w - px, by = r1.x - py, bz = r1.y - pz;
  const float cx = r1.z - px, cy = r1.w - py, cz = r2.x - pz;
  const float ux = r0.w - r0.x, uy = r1.x - r0.y, uz = r1.y - r0.z;   // ab, ac from the corners themselves: equal corners give exact zeros
  const float vx = r1.z - r0.x, vy = r1.w - r0.y, vz = r2.x - r0.z;
  // products rounded one by one (no fused multiply-add): u x u is exactly zero
  const float nx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
  const float ny = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
  const float nz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
  // det[a, b, c] from the corners minus p themselves: exactly zero when p IS a corner (a zero vector), where the denominator is zero too
  const float det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
  const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz), lc = sqrtf(cx * cx + cy * cy + cz * cz);
  const float ab = ax * bx + ay * by + az * bz, bc = bx * cx + by * cy + bz * cz, ca = cx * ax + cy * ay + cz * az;
  const float den = la * lb * lc + ab * lc + bc * la + ca * lb;
  const bool flat = nx == 0.0f && ny == 0.0f && nz == 0.0f;
  return flat ? 0.0f : atan2f(det, den);
}

// one wave copies a chunk's records into ITS part of the LDS; only that wave reads them, so a wave barrier orders the accesses
__device__ __forceinline__ void stage_chunk(float4* __restrict__ lds, const float* __restrict__ recs, int n, int lane) {
  const float4* src = (const float4*)recs;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");             // the previous chunk has been read
  __builtin_amdgcn_wave_barrier();
  for (int k = lane; k < n * (kRec / 4); k += kLanes) lds[k] = src[k];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// kMask (harp_mesh_contact_excl): excl holds, chunk-major, one uint4 = 128 bits per (chunk, query vertex); bit k of it set
//   means face c * kFaces + k does not count for that vertex's distance minimum.  A lane loads its word after the cull decision (a culled
//   chunk's words are never read) and before the chunk is staged, so the load is in flight during the copy; the 64 lanes of a tile read
//   64 consecutive 16-byte words.  The inner loop picks one of the four 32-bit words and one bit by the loop counter, which is
//   wave-uniform: selects and a shift by a scalar, no indexed register, no scratch.  The test only removes candidates: a lane with every
//   face of its chunks excluded keeps best = inf, which leaves the cull by `worst` at inf for the wave, so max_dist alone culls — the
//   cull stays conservative with no change.  Pass 2, the winding sum, is not masked.  Without kMask the kernel is the one before.
template <bool kMask>
__global__ void __launch_bounds__(kLanes* kWaves) contact_kernel(const float* __restrict__ verts, const float* __restrict__ cam_R,
                                                                 const float* __restrict__ cam_T, int V, int q_flip,
                                                                 const float* __restrict__ boxes, const float* __restrict__ recs, int F,
                                                                 int n_chunks, int n_tiles, int t_flip, float max_dist,
                                                                 const uint4* __restrict__ excl, float* __restrict__ dist,
                                                                 int32_t* __restrict__ face, float* __restrict__ wind) {
  __shared__ float4 stage[kWaves][kFaces * (kRec / 4)];
  __shared__ float part_d[kWaves][kLanes], part_w[kWaves][kLanes];
  __shared__ int part_f[kWaves][kLanes];
  const int b = blockIdx.x / n_tiles, tile = blockIdx.x - b * n_tiles;
  const int lane = (int)threadIdx.x & (kLanes - 1), wave = (int)threadIdx.x / kLanes;
  float4* lds = stage[wave];
  const int i = tile * kLanes + lane;
  const bool live = i < V;
  const float inf = __builtin_inff();
  float px, py, pz;
  view_of(verts + ((size_t)b * V + (live ? i : V - 1)) * 3, cam_R + 9 * (size_t)b, cam_T + 3 * (size_t)b, q_flip != 0, px, py, pz);
  const bool ok = live && finite3(px, py, pz);
  if (!ok) px = py = pz = 0.0f;                                       // (its results are dropped below)
  const float qlx = uniform(wave_min(ok ? px : inf)), qly = uniform(wave_min(ok ? py : inf)), qlz = uniform(wave_min(ok ? pz : inf));
  const float qhx = uniform(wave_max(ok ? px : -inf)), qhy = uniform(wave_max(ok ? py : -inf)), qhz = uniform(wave_max(ok ? pz : -inf));
  const float qm = fmaxf(fmaxf(fmaxf(fabsf(qlx), fabsf(qhx)), fmaxf(fabsf(qly), fabsf(qhy))), fmaxf(fabsf(qlz), fabsf(qhz)));
  float best = inf, w = 0.0f;
  int bf = -1;
  if (__ballot(ok) != 0ull) {                                         // (the same in the four waves: they hold the same vertices)
    const float* bx = boxes + (size_t)b * n_chunks * kBox;
    const float* rb = recs + (size_t)b * F * kRec;
    // pass 1, this wave's chunks in ascending order: best is the float32 distance, best2 the squared distance that a face has to beat
    float best2 = inf, worst = inf;
    for (int c = wave; c < n_chunks; c += kWaves) {
      const float* t = bx + (size_t)c * kBox;
      const float tlx = t[0], tly = t[1], tlz = t[2], thx = t[3], thy = t[4], thz = t[5];
      const float gx = fmaxf(0.0f, fmaxf(tlx - qhx, qlx - thx)), gy = fmaxf(0.0f, fmaxf(tly - qhy, qly - thy));
      const float gz = fmaxf(0.0f, fmaxf(tlz - qhz, qlz - thz));
      const float m = fmaxf(qm, fmaxf(fmaxf(fmaxf(fabsf(tlx), fabsf(thx)), fmaxf(fabsf(tly), fabsf(thy))), fmaxf(fabsf(tlz), fabsf(thz))));
      const float gap = uniform(sqrtf(gx * gx + gy * gy + gz * gz) - kCullMargin * m);
      if (gap > fminf(max_dist, worst)) continue;                     // (an empty box gives inf - inf = NaN or an infinite gap: the chunk has no valid face either way)
      const int n = min(kFaces, F - c * kFaces);
      uint4 ex = make_uint4(0u, 0u, 0u, 0u);
      if (kMask && live) ex = excl[(size_t)c * V + i];                // (c < n_chunks, i < V: inside the table of n_chunks * V words)
      stage_chunk(lds, rb + (size_t)c * kFaces * kRec, n, lane);
      for (int k = 0; k < n; ++k) {
        const float4 r0 = lds[3 * k], r1 = lds[3 * k + 1], r2 = lds[3 * k + 2];
        if (r2.y != 0.0f) {                                           // (the same record in every lane: wave-uniform)
          const float d2 = tri_dist2(px, py, pz, r0, r1, r2);
          bool counts = true;
          if (kMask) {                                                // (k is wave-uniform: the word by selects, the bit by a scalar shift)
            const int wsel = k >> 5;
            const uint32_t word = wsel == 0 ? ex.x : wsel == 1 ? ex.y : wsel == 2 ? ex.z : ex.w;
            counts = ((word >> (k & 31)) & 1u) == 0u;
          }
          if (d2 < best2 && counts) {                                 // a candidate; it replaces only on a strictly smaller float32 DISTANCE
            const float d = sqrtf(d2);
            if (d < best) { best = d; best2 = d2; bf = c * kFaces + k; }
          }
        }
      }
      worst = uniform(wave_max(ok ? best : 0.0f));
    }
    // the four waves' results in wave order; of equal distances the lower face
    part_d[wave][lane] = best;
    part_f[wave][lane] = bf;
    __syncthreads();
    best = inf; bf = -1;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const float d = part_d[k][lane];
      const int f = part_f[k][lane];
      if (f >= 0 && (d < best || (d == best && f < bf))) { best = d; bf = f; }
    }
    // (with the mask a lane can be left without a face although the target has valid ones: at max_dist = inf its best = inf is no contact)
    const bool near = ok && best <= max_dist && (!kMask || bf >= 0);
    if (wind && __ballot(near) != 0ull) {                             // (the same in the four waves)
      for (int c = wave; c < n_chunks; c += kWaves) {
        const int n = min(kFaces, F - c * kFaces);
        stage_chunk(lds, rb + (size_t)c * kFaces * kRec, n, lane);
        for (int k = 0; k < n; ++k) {
          const float4 r0 = lds[3 * k], r1 = lds[3 * k + 1], r2 = lds[3 * k + 2];
          if (r2.y != 0.0f) w += tri_half_angle(px, py, pz, r0, r1, r2);
        }
      }
      part_w[wave][lane] = w;
      __syncthreads();
      w = ((part_w[0][lane] + part_w[1][lane]) + (part_w[2][lane] + part_w[3][lane])) * (t_flip ? -0.15915494309189535f : 0.15915494309189535f);      // 2 / (4 pi), negated for a mirrored target
    }
    if (!near) { best = inf; bf = -1; w = 0.0f; }
  }
  if (live && wave == 0) {
    const size_t o = (size_t)b * V + i;
    if (dist) dist[o] = best;
    if (face) face[o] = bf;
    if (wind) wind[o] = w;
  }
}

size_t chunks_of(int F) { return (size_t)((F + kFaces - 1) / kFaces); }

bool mesh_ok(const harp_contact_mesh* m, bool target) {
  return m && m->verts && m->cam_R && m->cam_T && m->V > 0 && m->reserved == 0 && (!target || (m->faces && m->F > 0));
}

// the checks and the two launches of both entries; kMask: with the exclusion table
template <bool kMask>
int launch_contact(const harp_contact_mesh* query, const harp_contact_mesh* target, const uint32_t* excl, int B, float max_dist, float* ws,
                   float* dist, int32_t* face, float* wind, hipStream_t stream) {
  if (!mesh_ok(query, false) || !mesh_ok(target, true) || !ws || B <= 0) return HARP_ERR_ARG;
  if (kMask && (!excl || ((uintptr_t)excl & 15) != 0)) return HARP_ERR_ARG;
  if (!(max_dist >= 0.0f)) return HARP_ERR_ARG;                       // (a NaN is not)
  if (!dist && !face && !wind) return HARP_ERR_ARG;
  if (((uintptr_t)ws & 15) != 0) return HARP_ERR_ARG;
  const int V = query->V, F = target->F;
  const long long n_chunks = (long long)chunks_of(F), n_tiles = ((long long)V + kLanes - 1) / kLanes;
  if (n_chunks * B > 0x7fffffffLL || n_tiles * B > 0x7fffffffLL) return HARP_ERR_ARG;
  float* boxes = ws;
  float* recs = ws + (size_t)B * n_chunks * kBox;
  hipLaunchKernelGGL(contact_setup_kernel, dim3((unsigned)(n_chunks * B)), dim3(kFaces), 0, stream, target->verts, target->cam_R,
                     target->cam_T, target->faces, target->V, F, (int)n_chunks, target->flip_x != 0 ? 1 : 0, boxes, recs);
  HARP_CHECK_LAUNCH();
  hipLaunchKernelGGL(contact_kernel<kMask>, dim3((unsigned)(n_tiles * B)), dim3(kLanes * kWaves), 0, stream, query->verts, query->cam_R,
                     query->cam_T, V, query->flip_x != 0 ? 1 : 0, (const float*)boxes, (const float*)recs, F, (int)n_chunks, (int)n_tiles,
                     target->flip_x != 0 ? 1 : 0, max_dist, (const uint4*)excl, dist, face, wind);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

}  // namespace

extern "C" size_t harp_mesh_contact_ws_floats(int B, int F_target) {
  if (B <= 0 || F_target <= 0) return 0;
  return (size_t)B * (chunks_of(F_target) * kBox + (size_t)F_target * kRec);
}

extern "C" int harp_mesh_contact(const harp_contact_mesh* query, const harp_contact_mesh* target, int B, float max_dist, float* ws,
                                 float* dist, int32_t* face, float* wind, hipStream_t stream) {
  return launch_contact<false>(query, target, nullptr, B, max_dist, ws, dist, face, wind, stream);
}

extern "C" size_t harp_contact_excl_words(int V_query, int F_target) {
  if (V_query <= 0 || F_target <= 0) return 0;
  return chunks_of(F_target) * (size_t)V_query * 4;
}

extern "C" int harp_mesh_contact_excl(const harp_contact_mesh* query, const harp_contact_mesh* target, const uint32_t* excl, int B,
                                      float max_dist, float* ws, float* dist, int32_t* face, float* wind, hipStream_t stream) {
  return launch_contact<true>(query, target, excl, B, max_dist, ws, dist, face, wind, stream);
}
