// Taubin smoothing of the fitted meshes before they are exported (gfx950): optimize_sequence.py:780
// `taubin_smoothing(meshes)` = pytorch3d.ops.taubin_smoothing(lambd=0.53, mu=-0.53, num_iter=10), forward only.  PyTorch3D is not
// installed where this was written: the passes below are its v0.6.2 taubin_smoothing / norm_laplacian as recalled (include/harp_hip.h).
//
// 2 * num_iter dependent Jacobi passes over a 3093- or 4083-vertex mesh, every frame on its own.  A pass, with factor f:
//   w_ij = 1 / (|v_i - v_j| + 1e-12),   v_i' = (1 - f) v_i + f (sum_j w_ij v_j) / (sum_j w_ij)
// evaluated as v_i' = v_i + f (sum_j w_ij (v_j - v_i)) / (sum_j w_ij): the same value, and the differences v_j - v_i are already formed
// for the edge lengths (and are exact to the last bit or two for neighbours 2.5 mm apart at 0.5 m).
//
// LDS path: one workgroup of 1024 threads per frame, the positions of the whole mesh resident in LDS for all passes, one float4 slot per
// vertex (64 KiB for 4096 vertices: the static limit, no attribute to raise).  A thread owns vertices tid, tid + 1024, ... (4 at most),
// keeps their positions and CSR ranges in registers, and a pass is gather -> barrier -> write own slots -> barrier: the new positions wait
// in registers while the other waves still read the old ones, so ONE buffer holds the mesh (DESIGN.md §16 for the layout and the numbers).
// Global path: any V, one launch per pass, ping-pong through two workspace buffers.
#include "harp_common.h"
#include "harp_hip.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kPerThread = 4;
constexpr int kLdsMaxV = kThreads * kPerThread;        // 4096 vertices = 64 KiB of float4

// 1 / (|d| + 1e-12); the fused multiply-adds are spelled out here and below so that both kernels round alike whatever the compiler contracts
__device__ __forceinline__ float edge_weight(float dx, float dy, float dz) {
  return 1.0f / (sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx))) + 1e-12f);
}

// one vertex of one pass: the displacement f * sum_j w_ij (q_j - p) / sum_j w_ij; a vertex without neighbours stays (PyTorch3D: 0/0 = NaN)
template <typename Fetch>
__device__ __forceinline__ float3 taubin_step(float3 p, int lo, int hi, const int32_t* __restrict__ nbr_idx, float f, Fetch fetch) {
  float ax = 0.f, ay = 0.f, az = 0.f, W = 0.f;
  for (int e = lo; e < hi; ++e) {
    const float3 q = fetch(nbr_idx[e]);
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    const float w = edge_weight(dx, dy, dz);
    ax = fmaf(w, dx, ax); ay = fmaf(w, dy, ay); az = fmaf(w, dz, az);
    W += w;
  }
  if (W > 0.f) {
    const float r = f / W;
    p.x = fmaf(r, ax, p.x); p.y = fmaf(r, ay, p.y); p.z = fmaf(r, az, p.z);
  }
  return p;
}

__global__ void __launch_bounds__(kThreads) taubin_lds_kernel(const float* verts, const int32_t* __restrict__ nbr_off,
                                                              const int32_t* __restrict__ nbr_idx, int V, float lambd, float mu, int passes,
                                                              float* out) {   // out may be verts: no __restrict__
  __shared__ float4 pos[kLdsMaxV];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * V * 3;
  float3 mine[kPerThread];
  int lo[kPerThread], hi[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int i = tid + k * kThreads;
    mine[k] = make_float3(0.f, 0.f, 0.f);
    lo[k] = hi[k] = 0;
    if (i < V) {
      const float* s = verts + base + 3 * (size_t)i;
      mine[k] = make_float3(s[0], s[1], s[2]);
      pos[i] = make_float4(mine[k].x, mine[k].y, mine[k].z, 0.f);
      lo[k] = nbr_off[i];
      hi[k] = nbr_off[i + 1];
    }
  }
  int steps = 0;                                       // the longest of this lane's CSR rows
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) steps = max(steps, hi[k] - lo[k]);
  __syncthreads();
  for (int pass = 0; pass < passes; ++pass) {
    const float f = (pass & 1) ? mu : lambd;
    // the lane's (up to) four rows are walked in lockstep, the indices of step s + 1 fetched before step s is computed, so that four
    // independent L2 read -> LDS read -> sqrt / division chains are in flight per lane.  Per vertex the neighbours are still added in
    // CSR order with the same fused operations as taubin_step: both kernels give the same bits.  (Measured: no faster than walking the
    // rows one after the other, 155 against 146 us for 32 hand frames — DESIGN.md §16.)
    float ax[kPerThread], ay[kPerThread], az[kPerThread], W[kPerThread];
    int jn[kPerThread];
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      ax[k] = ay[k] = az[k] = W[k] = 0.f;
      jn[k] = lo[k] < hi[k] ? nbr_idx[lo[k]] : 0;
    }
    for (int s = 0; s < steps; ++s) {
      int j[kPerThread];
#pragma unroll
      for (int k = 0; k < kPerThread; ++k) {
        j[k] = jn[k];
        jn[k] = lo[k] + s + 1 < hi[k] ? nbr_idx[lo[k] + s + 1] : 0;
      }
#pragma unroll
      for (int k = 0; k < kPerThread; ++k) {
        const float4 q = pos[j[k]];                    // slot 0 for a row that has ended: read, not used
        const float dx = q.x - mine[k].x, dy = q.y - mine[k].y, dz = q.z - mine[k].z;
        const float w = edge_weight(dx, dy, dz);
        if (lo[k] + s < hi[k]) {
          ax[k] = fmaf(w, dx, ax[k]); ay[k] = fmaf(w, dy, ay[k]); az[k] = fmaf(w, dz, az[k]);
          W[k] += w;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kPerThread; ++k)
      if (W[k] > 0.f) {                                // no neighbour: the vertex stays
        const float r = f / W[k];
        mine[k].x = fmaf(r, ax[k], mine[k].x); mine[k].y = fmaf(r, ay[k], mine[k].y); mine[k].z = fmaf(r, az[k], mine[k].z);
      }
    if (pass + 1 == passes) break;
    __syncthreads();                                   // every wave has read the old positions
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      const int i = tid + k * kThreads;
      if (i < V) pos[i] = make_float4(mine[k].x, mine[k].y, mine[k].z, 0.f);
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int i = tid + k * kThreads;
    if (i < V) {
      float* d = out + base + 3 * (size_t)i;
      d[0] = mine[k].x; d[1] = mine[k].y; d[2] = mine[k].z;
    }
  }
}

// one pass from src to dst (never the same buffer), one thread per vertex, frames over grid.y (strided: any B)
__global__ void __launch_bounds__(256) taubin_pass_kernel(const float* __restrict__ src, const int32_t* __restrict__ nbr_off,
                                                          const int32_t* __restrict__ nbr_idx, int B, int V, float f, float* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  const int lo = nbr_off[i], hi = nbr_off[i + 1];
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const float* s = src + (size_t)b * V * 3;
    const float3 p = taubin_step(make_float3(s[3 * (size_t)i], s[3 * (size_t)i + 1], s[3 * (size_t)i + 2]), lo, hi, nbr_idx, f,
                                 [&](int j) { return make_float3(s[3 * (size_t)j], s[3 * (size_t)j + 1], s[3 * (size_t)j + 2]); });
    float* d = dst + ((size_t)b * V + i) * 3;
    d[0] = p.x; d[1] = p.y; d[2] = p.z;
  }
}

size_t round256(size_t n) { return (n + 255) / 256 * 256; }

}  // namespace

extern "C" {

size_t harp_taubin_ws_bytes(int B, int V) {
  if (B <= 0 || V <= 0) return 0;
  return 2 * round256((size_t)B * V * 3 * sizeof(float));
}

int harp_taubin_smooth(const float* verts, const int32_t* nbr_off, const int32_t* nbr_idx, int B, int V, float lambd, float mu, int num_iter,
                       int mode, float* out, void* ws, hipStream_t stream) {
  if (!verts || !nbr_off || !nbr_idx || !out || B <= 0 || V <= 0 || num_iter < 0 || mode < 0 || mode > 2) return HARP_ERR_ARG;
  if (mode == 1 && V > kLdsMaxV) return HARP_ERR_ARG;
  const bool lds = mode == 1 || (mode == 0 && V <= kLdsMaxV);
  if (num_iter > 0 && !lds && !ws) return HARP_ERR_ARG;
  const size_t bytes = (size_t)B * V * 3 * sizeof(float);
  if (num_iter == 0) {
    if (out != verts && hipMemcpyAsync(out, verts, bytes, hipMemcpyDeviceToDevice, stream) != hipSuccess) return HARP_ERR_LAUNCH;
    return HARP_OK;
  }
  const int passes = 2 * num_iter;
  if (lds) {
    hipLaunchKernelGGL(taubin_lds_kernel, dim3(B), dim3(kThreads), 0, stream, verts, nbr_off, nbr_idx, V, lambd, mu, passes, out);
    HARP_CHECK_LAUNCH();
    return HARP_OK;
  }
  // verts -> a -> b -> a ... -> out: `verts` is read by the first pass only and `out` written by the last, so they may be one buffer
  float* buf[2] = {(float*)ws, (float*)((char*)ws + round256(bytes))};
  const dim3 grid((V + 255) / 256, B < 65535 ? B : 65535);
  const float* src = verts;
  for (int pass = 0; pass < passes; ++pass) {
    float* dst = pass + 1 == passes ? out : buf[pass & 1];
    hipLaunchKernelGGL(taubin_pass_kernel, grid, dim3(256), 0, stream, src, nbr_off, nbr_idx, B, V, (pass & 1) ? mu : lambd, dst);
    HARP_CHECK_LAUNCH();
    src = dst;
  }
  return HARP_OK;
}

}  // extern "C"
