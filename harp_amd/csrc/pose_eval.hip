// Geometric accuracy of the post-fit evaluation (gfx950): batched Procrustes alignment, PCK counts and the point-set F-score.
//   harp_procrustes_align   utils/eval_util.py:212-235 (align_w_scale, scipy's orthogonal_procrustes inside) for N frames at once
//   harp_pck_counts         the counting half of utils/eval_util.py:103-163 (EvalUtil._get_pck / _get_epe / get_measures)
//   harp_point_set_fscore   precision / recall / F between two point sets at several distances (the mesh measure of the FreiHAND benchmark)
// All three are forward only, float64 inside, deterministic (no float atomics; every sum has a fixed order: a strided per-lane chain, a
// 64-lane butterfly, then the waves of the workgroup in index order), allocate nothing and need no workspace.
//
// Procrustes: one workgroup of 256 threads per frame and three passes over its K points (K is not bounded by the block: lanes stride).
//   pass 1  n_valid, sum gt, sum pred over the valid points                   -> t1, t2
//   pass 2  |a|_F^2, |b|_F^2 and the nine sums of a^T b of the centred sets   -> s1, s2, M = a^T b / (s1 s2)
//   lane 0  one-sided Jacobi SVD of the 3x3 M in float64: M V = U W, R = U V^T (NO determinant correction: a mirrored prediction is
//           aligned by a reflection, as scipy does), s = sum W.  Columns whose singular value vanishes (three points, coplanar sets)
//           are completed to an orthonormal U; the sign of a completed column does not reach `aligned` (b has no component along it).
//   pass 3  aligned = R (b / s2) s s1 + t1, err = |gt - aligned|, both rounded to float32 once.
// PCK: one workgroup per keypoint; its column of errors goes through LDS 256 frames at a time and lane j counts threshold j, j + 256, ...
// F-score: one workgroup of 512 threads per frame, all pairs, the other set tiled through LDS as doubles, two own points per lane.
#include "harp_common.h"
#include "harp_hip.h"

namespace {

constexpr int kProThreads = 256;
constexpr int kPckThreads = 256;
constexpr int kFsThreads = 512;
constexpr int kFsTile = 512;                               // points of the other set per LDS tile (12 KiB of doubles)

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sums of NV doubles over a workgroup of WAVES waves; every thread gets the totals (lds: WAVES * NV doubles, reusable after return)
template <int NV, int WAVES>
__device__ __forceinline__ void block_sum_d(double (&v)[NV], double* lds) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    v[c] = wave_sum_d(v[c]);
    if ((threadIdx.x & 63) == 0) lds[w * NV + c] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    double r = lds[c];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) r += lds[k * NV + c];
    v[c] = r;
  }
  __syncthreads();
}
template <int WAVES>
__device__ __forceinline__ int block_sum_i(int v, int* lds) {
  v = wave_sum_i(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int k = 0; k < WAVES; ++k) r += lds[k];
  __syncthreads();
  return r;
}

// R = U V^T and s = sum of the singular values of M = U W V^T (row-major 3x3), by one-sided Jacobi rotations of M's columns
// (also a host function: tests/test_pose_eval_cpu.py runs it against LAPACK without a GPU)
__host__ __device__ inline void polar_no_det_fix(const double* M, double* R, double& s) {
  double A[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { A[i][j] = M[3 * i + j]; V[i][j] = i == j ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) { al += A[i][p] * A[i][p]; be += A[i][q] * A[i][q]; ga += A[i][p] * A[i][q]; }
      if (fabs(ga) <= 2e-16 * sqrt(al * be) || ga == 0.0) continue;
      rotated = true;
      const double zeta = (be - al) / (2.0 * ga);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double ap = A[i][p], aq = A[i][q], vp = V[i][p], vq = V[i][q];
        A[i][p] = c * ap - sn * aq; A[i][q] = sn * ap + c * aq;
        V[i][p] = c * vp - sn * vq; V[i][q] = sn * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double sig[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) sig[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
  // columns by falling singular value
  int o0 = 0, o1 = 1, o2 = 2, tmp;
  if (sig[o1] > sig[o0]) { tmp = o0; o0 = o1; o1 = tmp; }
  if (sig[o2] > sig[o0]) { tmp = o0; o0 = o2; o2 = tmp; }
  if (sig[o2] > sig[o1]) { tmp = o1; o1 = o2; o2 = tmp; }
  const double tiny = 1e-12 * sig[o0];
  double U[3][3];                                            // U[j] = the left vector that belongs to column j of V
  if (sig[o0] > 0.0) {
    for (int i = 0; i < 3; ++i) U[o0][i] = A[i][o0] / sig[o0];
  } else {
    U[o0][0] = 1.0; U[o0][1] = 0.0; U[o0][2] = 0.0;
  }
  if (sig[o1] > tiny) {
    for (int i = 0; i < 3; ++i) U[o1][i] = A[i][o1] / sig[o1];
  } else {                                                   // any unit vector across U[o0]: its cross product with the axis it leans on least
    const double* u = U[o0];
    const double ax = fabs(u[0]), ay = fabs(u[1]), az = fabs(u[2]);
    double e[3] = {0.0, 0.0, 0.0};
    e[(ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2)] = 1.0;
    double w[3] = {u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0]};
    const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int i = 0; i < 3; ++i) U[o1][i] = w[i] / n;
  }
  if (sig[o2] > tiny) {
    for (int i = 0; i < 3; ++i) U[o2][i] = A[i][o2] / sig[o2];
  } else {
    const double *u = U[o0], *v = U[o1];
    U[o2][0] = u[1] * v[2] - u[2] * v[1]; U[o2][1] = u[2] * v[0] - u[0] * v[2]; U[o2][2] = u[0] * v[1] - u[1] * v[0];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = U[0][r] * V[c][0] + U[1][r] * V[c][1] + U[2][r] * V[c][2];
  s = sig[0] + sig[1] + sig[2];
}

__global__ void __launch_bounds__(kProThreads) procrustes_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                                const int32_t* __restrict__ pred_idx, const float* __restrict__ valid, int K,
                                                                int Kp, float* __restrict__ aligned, float* __restrict__ err,
                                                                double* __restrict__ trafo, int32_t* __restrict__ n_valid) {
  __shared__ double red[(kProThreads / 64) * 11];
  __shared__ int redi[kProThreads / 64];
  __shared__ double res[10];                                 // lane 0's R (9) and s for the third pass
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* g = gt + (size_t)n * K * 3;
  const float* p = pred + (size_t)n * Kp * 3;
  const float* vm = valid ? valid + (size_t)n * K : nullptr;
  // a point is used when its mask is non-zero and its gather index lies inside the prediction (an index outside never reads)
  auto src = [&](int k) -> int {
    if (vm && vm[k] == 0.0f) return -1;
    const int j = pred_idx ? pred_idx[k] : k;
    return (j >= 0 && j < Kp) ? j : -1;
  };
  double a1[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
  for (int k = tid; k < K; k += kProThreads) {
    const int j = src(k);
    if (j < 0) continue;
    ++cnt;
#pragma unroll
    for (int c = 0; c < 3; ++c) { a1[c] += (double)g[3 * (size_t)k + c]; a1[3 + c] += (double)p[3 * (size_t)j + c]; }
  }
  cnt = block_sum_i<kProThreads / 64>(cnt, redi);
  block_sum_d<6, kProThreads / 64>(a1, red);
  float* al = aligned ? aligned + (size_t)n * K * 3 : nullptr;
  float* er = err + (size_t)n * K;
  if (tid == 0) n_valid[n] = cnt;
  if (cnt < 3) {                                             // "invalid ground truth" (:204-207): NaN everywhere, the true count
    const float qnan = __int_as_float(0x7fc00000);
    for (int k = tid; k < K; k += kProThreads) {
      er[k] = qnan;
      if (al) { al[3 * (size_t)k] = qnan; al[3 * (size_t)k + 1] = qnan; al[3 * (size_t)k + 2] = qnan; }
    }
    if (trafo && tid < 14) trafo[(size_t)n * 14 + tid] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }
  double t1[3], t2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { t1[c] = a1[c] / (double)cnt; t2[c] = a1[3 + c] / (double)cnt; }
  double a2[11] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = tid; k < K; k += kProThreads) {
    const int j = src(k);
    if (j < 0) continue;
    double a[3], b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[c] = (double)g[3 * (size_t)k + c] - t1[c]; b[c] = (double)p[3 * (size_t)j + c] - t2[c]; }
    a2[0] += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    a2[1] += b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) a2[2 + 3 * r + c] += a[r] * b[c];
  }
  block_sum_d<11, kProThreads / 64>(a2, red);
  const double s1 = sqrt(a2[0]) + 1e-8, s2 = sqrt(a2[1]) + 1e-8;
  if (tid == 0) {
    double M[9], R[9], s;
    const double inv = 1.0 / (s1 * s2);
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = a2[2 + i] * inv;
    polar_no_det_fix(M, R, s);
#pragma unroll
    for (int i = 0; i < 9; ++i) res[i] = R[i];
    res[9] = s;
    if (trafo) {
      double* t = trafo + (size_t)n * 14;
#pragma unroll
      for (int i = 0; i < 9; ++i) t[i] = R[i];
      t[9] = s; t[10] = s1;
#pragma unroll
      for (int c = 0; c < 3; ++c) t[11 + c] = t1[c] - t2[c];
    }
  }
  __syncthreads();
  double R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = res[i];
  const double s = res[9];
  const float qnan = __int_as_float(0x7fc00000);
  for (int k = tid; k < K; k += kProThreads) {
    const int j = src(k);
    if (j < 0) {
      er[k] = qnan;
      if (al) { al[3 * (size_t)k] = qnan; al[3 * (size_t)k + 1] = qnan; al[3 * (size_t)k + 2] = qnan; }
      continue;
    }
    double b[3], d2 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = ((double)p[3 * (size_t)j + c] - t2[c]) / s2;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double x = (b[0] * R[3 * r] + b[1] * R[3 * r + 1] + b[2] * R[3 * r + 2]) * s * s1 + t1[r];
      const double d = (double)g[3 * (size_t)k + r] - x;
      d2 += d * d;
      if (al) al[3 * (size_t)k + r] = (float)x;
    }
    er[k] = (float)sqrt(d2);
  }
}

// one workgroup per keypoint k: counts[k][j] = #{n seen : err[n][k] <= thr[j]}, n_vis[k] = #{n seen}, err_sum[k] = sum of the seen errors;
// seen = mask non-zero and the error not NaN
__global__ void __launch_bounds__(kPckThreads) pck_kernel(const float* __restrict__ err, const float* __restrict__ valid,
                                                          const float* __restrict__ thr, int N, int K, int n_thr, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ n_vis, double* __restrict__ err_sum) {
  __shared__ float col[kPckThreads];
  __shared__ double red[kPckThreads / 64];
  __shared__ int redi[kPckThreads / 64];
  const int k = blockIdx.x, tid = threadIdx.x;
  const float qnan = __int_as_float(0x7fc00000);
  double sum[1] = {0.0};
  int vis = 0;
  // thresholds tid, tid + 256, ... : this lane's running counts live in the output, which no other lane touches
  for (int j = tid; j < n_thr; j += kPckThreads) counts[(size_t)k * n_thr + j] = 0;
  for (int n0 = 0; n0 < N; n0 += kPckThreads) {
    const int n = n0 + tid;
    float e = qnan;
    if (n < N && (!valid || valid[(size_t)n * K + k] != 0.0f)) e = err[(size_t)n * K + k];
    if (e == e) { ++vis; sum[0] += (double)e; }
    col[tid] = e;
    __syncthreads();
    const int m = min(kPckThreads, N - n0);
    for (int j = tid; j < n_thr; j += kPckThreads) {
      const float t = thr[j];
      int c = 0;
      for (int i = 0; i < m; ++i) c += col[i] <= t ? 1 : 0;   // NaN <= t is false
      counts[(size_t)k * n_thr + j] += c;
    }
    __syncthreads();
  }
  vis = block_sum_i<kPckThreads / 64>(vis, redi);
  block_sum_d<1, kPckThreads / 64>(sum, red);
  if (tid == 0) { n_vis[k] = vis; err_sum[k] = sum[0]; }
}

struct P3d { double x, y, z; };

// nearest squared distance from the points of `own` (Ko) to the set `oth` (Kt) of one frame; counts of the own points nearer than t2[j]
// land in cnt[wave][j] (written by lane 0 of each wave only, summed by the caller)
__device__ __forceinline__ void nearest_pass(const float* __restrict__ own, int Ko, const float* __restrict__ oth, int Kt, P3d* tile,
                                             const float* __restrict__ thr, int n_thr, float* __restrict__ nn, int* cnt) {
  const int tid = threadIdx.x, wave = tid >> 6;
  for (int j = tid; j < (kFsThreads / 64) * n_thr; j += kFsThreads) cnt[j] = 0;
  for (int i0 = 0; i0 < Ko; i0 += 2 * kFsThreads) {
    const int ia = i0 + tid, ib = i0 + kFsThreads + tid;
    const bool ha = ia < Ko, hb = ib < Ko;
    P3d a = {0.0, 0.0, 0.0}, b = {0.0, 0.0, 0.0};
    if (ha) { a.x = (double)own[3 * (size_t)ia]; a.y = (double)own[3 * (size_t)ia + 1]; a.z = (double)own[3 * (size_t)ia + 2]; }
    if (hb) { b.x = (double)own[3 * (size_t)ib]; b.y = (double)own[3 * (size_t)ib + 1]; b.z = (double)own[3 * (size_t)ib + 2]; }
    double ma = __longlong_as_double(0x7ff0000000000000LL), mb = ma;     // +inf
    for (int c0 = 0; c0 < Kt; c0 += kFsTile) {
      const int m = min(kFsTile, Kt - c0);
      __syncthreads();                                       // the previous tile (and cnt's clearing) is done with
      for (int q = tid; q < m; q += kFsThreads) {
        const float* s = oth + 3 * (size_t)(c0 + q);
        tile[q].x = (double)s[0]; tile[q].y = (double)s[1]; tile[q].z = (double)s[2];
      }
      __syncthreads();
      for (int q = 0; q < m; ++q) {
        const P3d t = tile[q];
        const double ax = a.x - t.x, ay = a.y - t.y, az = a.z - t.z, bx = b.x - t.x, by = b.y - t.y, bz = b.z - t.z;
        ma = fmin(ma, ax * ax + ay * ay + az * az);
        mb = fmin(mb, bx * bx + by * by + bz * bz);
      }
    }
    if (nn) {
      if (ha) nn[ia] = (float)sqrt(ma);
      if (hb) nn[ib] = (float)sqrt(mb);
    }
    for (int j = 0; j < n_thr; ++j) {
      const double t = (double)thr[j], t2 = t * t;
      const int c = __popcll(__ballot(ha && ma < t2)) + __popcll(__ballot(hb && mb < t2));
      if ((tid & 63) == 0) cnt[wave * n_thr + j] += c;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kFsThreads) fscore_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                            const float* __restrict__ thr, int Kg, int Kp, int n_thr, float* __restrict__ out,
                                                            float* __restrict__ nn_gt, float* __restrict__ nn_pred) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  P3d* tile = (P3d*)smem;
  int* cnt_g = (int*)(smem + sizeof(P3d) * kFsTile);
  int* cnt_p = cnt_g + (kFsThreads / 64) * n_thr;
  const int n = blockIdx.x;
  const float* g = gt + (size_t)n * Kg * 3;
  const float* p = pred + (size_t)n * Kp * 3;
  nearest_pass(g, Kg, p, Kp, tile, thr, n_thr, nn_gt ? nn_gt + (size_t)n * Kg : nullptr, cnt_g);
  nearest_pass(p, Kp, g, Kg, tile, thr, n_thr, nn_pred ? nn_pred + (size_t)n * Kp : nullptr, cnt_p);
  for (int j = threadIdx.x; j < n_thr; j += kFsThreads) {
    int cg = 0, cp = 0;
#pragma unroll
    for (int w = 0; w < kFsThreads / 64; ++w) { cg += cnt_g[w * n_thr + j]; cp += cnt_p[w * n_thr + j]; }
    const double pr = (double)cg / (double)Kg, rc = (double)cp / (double)Kp;
    float* o = out + ((size_t)n * n_thr + j) * 3;
    o[0] = (float)pr; o[1] = (float)rc;
    o[2] = pr + rc > 0.0 ? (float)(2.0 * pr * rc / (pr + rc)) : 0.0f;
  }
}

constexpr int kFsMaxThr = 512;                             // 2 * 8 * n_thr ints of LDS beside the 12 KiB tile: 44 KiB at 512

}  // namespace

extern "C" {

int harp_procrustes_align(const float* gt, const float* pred, const int32_t* pred_idx, const float* valid, int N, int K, int Kp,
                          float* aligned, float* err, double* trafo, int32_t* n_valid, hipStream_t stream) {
  if (!gt || !pred || !err || !n_valid || N <= 0 || K <= 0 || Kp <= 0) return HARP_ERR_ARG;
  if (!pred_idx && Kp != K) return HARP_ERR_ARG;
  hipLaunchKernelGGL(procrustes_kernel, dim3(N), dim3(kProThreads), 0, stream, gt, pred, pred_idx, valid, K, Kp, aligned, err, trafo, n_valid);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

int harp_pck_counts(const float* err, const float* valid, const float* thresholds, int N, int K, int n_thr, int32_t* counts, int32_t* n_vis,
                    double* err_sum, hipStream_t stream) {
  if (!err || !thresholds || !counts || !n_vis || !err_sum || N <= 0 || K <= 0 || n_thr < 1) return HARP_ERR_ARG;
  hipLaunchKernelGGL(pck_kernel, dim3(K), dim3(kPckThreads), 0, stream, err, valid, thresholds, N, K, n_thr, counts, n_vis, err_sum);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

int harp_point_set_fscore(const float* gt, const float* pred, const float* thresholds, int N, int Kg, int Kp, int n_thr, float* out,
                          float* nn_gt, float* nn_pred, hipStream_t stream) {
  if (!gt || !pred || !thresholds || !out || N <= 0 || Kg <= 0 || Kp <= 0 || n_thr < 1 || n_thr > kFsMaxThr) return HARP_ERR_ARG;
  const size_t lds = sizeof(P3d) * kFsTile + 2 * (kFsThreads / 64) * (size_t)n_thr * sizeof(int);
  hipLaunchKernelGGL(fscore_kernel, dim3(N), dim3(kFsThreads), lds, stream, gt, pred, thresholds, Kg, Kp, n_thr, out, nn_gt, nn_pred);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

}  // extern "C"
