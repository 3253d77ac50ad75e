// Temporal smoothing of a motion (harp_amd/playback.py Motion.smooth / smooth_keypoints): the one kernel that takes the
// jitter out of per-frame rows before they are retimed (harp_motion_resample) or solved (harp_mano_ik).  Nothing in the reference does
// this on the device: its preprocessing fixes one-frame jumps of `pose` on the host and otherwise runs an Adam loop over the sequence.
//
// harp_motion_filter: rows (T, W) = n_rot axis-angle triples | n_vec 3-vectors | n_lin scalars -> out (T, W), used (T, nch): a symmetric
//   window of taps[0..R] around every row, shrunk symmetrically at the ends of the clip and at a change of `segment`, weighted per row or
//   per (row, channel) by a confidence.  Vectors and scalars are the weighted mean; a rotation is the weighted GEODESIC mean of the
//   rotations (rot_offset + triple): a sign-aligned chordal start, then a fixed number of Karcher iterations — a triple and its 2 pi
//   complement are one sample, a window around pi averages to a rotation near pi.  An optional trimmed second pass leaves out what lies
//   farther than trim[channel] from the first estimate (a one-frame spike).  include/harp_hip.h states the contract in full.
//   One lane per (row, channel), as motion_resample_kernel: neighbouring lanes read neighbouring channels of the same 2 R + 1 rows (the
//   whole window of a hand's 20 channels is (2 R + 1) x 216 bytes, served by L1 / L2 after the first pass).  Every pass recomputes the
//   quaternions from the rows; which samples count is kept as bit masks in registers (centre, R to the left, R to the right), so there is
//   no private array, no scratch, no LDS, no atomics and no data-dependent exit: two calls give the same bits, one capturable launch.
//   Every gather is row t +- d with 0 <= t - d and t + d < T.
#include "harp_common.h"
#include "harp_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct Quat { float w, x, y, z; };
struct Vec3 { float x, y, z; };
// the samples of a window that count: the centre, rows t - d (bit d - 1 of l) and rows t + d (bit d - 1 of r), d <= 64
struct Mask { bool c; unsigned long long l, r; };

// axis-angle -> unit quaternion; sin(t/2)/t by its series below 1e-4 (playback.hip's quat_of)
__device__ __forceinline__ Quat quat_of(float ax, float ay, float az) {
  const float t2 = ax * ax + ay * ay + az * az, t = sqrtf(t2);
  const float s = t < 1e-4f ? 0.5f - t2 * (1.0f / 48.0f) : sinf(0.5f * t) / t;
  return Quat{cosf(0.5f * t), s * ax, s * ay, s * az};
}
// a b
__device__ __forceinline__ Quat qmul(const Quat& a, const Quat& b) {
  return Quat{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + b.w * a.x + (a.y * b.z - a.z * b.y),
              a.w * b.y + b.w * a.y + (a.z * b.x - a.x * b.z), a.w * b.z + b.w * a.z + (a.x * b.y - a.y * b.x)};
}
// a^-1 b for a unit a
__device__ __forceinline__ Quat qmul_conj(const Quat& a, const Quat& b) { return qmul(Quat{a.w, -a.x, -a.y, -a.z}, b); }
// rotation vector of q taken with w >= 0 (an angle in [0, pi]): 2 atan2(|v|, w) v / |v|, the resample kernel's back-conversion
__device__ __forceinline__ Vec3 log_of(Quat q) {
  if (q.w < 0.0f) { q.w = -q.w; q.x = -q.x; q.y = -q.y; q.z = -q.z; }
  const float vn = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z);
  const float g = vn < 1e-8f ? 2.0f : 2.0f * atan2f(vn, q.w) / vn;
  return Vec3{g * q.x, g * q.y, g * q.z};
}
__device__ __forceinline__ bool positive_finite(float v) { return v > 0.0f && v < INFINITY; }      // (false for a NaN)
__device__ __forceinline__ int count(const Mask& m) { return (m.c ? 1 : 0) + __popcll(m.l) + __popcll(m.r); }

// what one lane reads: its channel's nc columns of the rows of its window
struct Window {
  const float* __restrict__ rows;
  const float* __restrict__ taps;
  const float* __restrict__ weights;
  int w_stride, w_col;                                                // weight of row s: weights[s * w_stride + w_col]
  int W, c0, nc, t, Rt;
  float ox, oy, oz;                                                   // the rotation offset of the channel (0 for the others)

  // a_s = tap[d] c_s in float32; a tap, a weight or a product that is negative or not finite is 0
  __device__ __forceinline__ float weight(int s, int d) const {
    float a = taps[d];
    if (!positive_finite(a)) return 0.0f;
    if (weights) {
      const float c = weights[(size_t)s * w_stride + w_col];
      if (!positive_finite(c)) return 0.0f;
      a *= c;
    }
    return positive_finite(a) ? a : 0.0f;
  }
  __device__ __forceinline__ bool load(int s, float& x, float& y, float& z) const {
    const float* p = rows + (size_t)s * W + c0;
    x = p[0];
    y = nc == 3 ? p[1] : 0.0f;
    z = nc == 3 ? p[2] : 0.0f;
    return isfinite(x) && isfinite(y) && isfinite(z);
  }
  __device__ __forceinline__ Quat quat(int s) const {
    float x, y, z;
    load(s, x, y, z);
    return quat_of(x + ox, y + oy, z + oz);
  }
  // f(row, distance) for the samples of m in the contract's order: the centre, then d = 1 .. Rt with t - d before t + d
  template <class F>
  __device__ __forceinline__ void visit(const Mask& m, F f) const {
    if (m.c) f(t, 0);
    for (int d = 1; d <= Rt; ++d) {
      if ((m.l >> (d - 1)) & 1ull) f(t - d, d);
      if ((m.r >> (d - 1)) & 1ull) f(t + d, d);
    }
  }
  // the same with the mask still to be decided: keep(row, distance) -> the sample's bit
  template <class F>
  __device__ __forceinline__ Mask select(const Mask& m, F keep) const {
    Mask k{m.c && keep(t, 0), 0ull, 0ull};
    for (int d = 1; d <= Rt; ++d) {
      if (((m.l >> (d - 1)) & 1ull) && keep(t - d, d)) k.l |= 1ull << (d - 1);
      if (((m.r >> (d - 1)) & 1ull) && keep(t + d, d)) k.r |= 1ull << (d - 1);
    }
    return k;
  }

  // sum a_s v_s / sum a_s over the samples of m (not empty)
  __device__ __forceinline__ Vec3 mean(const Mask& m) const {
    float sa = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    visit(m, [&](int s, int d) {
      const float a = weight(s, d);
      float x, y, z;
      load(s, x, y, z);
      sa += a; sx += a * x; sy += a * y; sz += a * z;
    });
    return Vec3{sx / sa, sy / sa, sz / sa};
  }
  // the geodesic mean of the rotations of m (not empty): false when the chordal sum vanishes (|sum a q| < 1e-6 sum a)
  __device__ __forceinline__ bool rot_mean(const Mask& m, int iters, Quat& mu) const {
    bool have = false;
    Quat qf{1.0f, 0.0f, 0.0f, 0.0f};
    float sa = 0.0f, sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
    visit(m, [&](int s, int d) {
      const float a = weight(s, d);
      Quat q = quat(s);
      if (!have) { qf = q; have = true; }
      const float sg = qf.w * q.w + qf.x * q.x + qf.y * q.y + qf.z * q.z < 0.0f ? -a : a;      // q and -q are one rotation: the first one's side
      sa += a; sw += sg * q.w; sx += sg * q.x; sy += sg * q.y; sz += sg * q.z;
    });
    const float nrm = sqrtf(sw * sw + sx * sx + sy * sy + sz * sz);
    if (nrm < 1e-6f * sa) return false;
    const float inv = 1.0f / nrm;
    mu = Quat{sw * inv, sx * inv, sy * inv, sz * inv};
    for (int it = 0; it < iters; ++it) {
      float vx = 0.0f, vy = 0.0f, vz = 0.0f;
      const Quat m0 = mu;
      visit(m, [&](int s, int d) {
        const float a = weight(s, d);
        const Vec3 l = log_of(qmul_conj(m0, quat(s)));
        vx += a * l.x; vy += a * l.y; vz += a * l.z;
      });
      mu = qmul(m0, quat_of(vx / sa, vy / sa, vz / sa));
    }
    return true;
  }
};

__global__ void __launch_bounds__(256) motion_filter_kernel(const float* __restrict__ rows, int T, int n_rot, int n_vec, int n_lin,
                                                            const float* __restrict__ rot_offset, const float* __restrict__ taps, int R,
                                                            const float* __restrict__ weights, int w_cols, const int32_t* __restrict__ segment,
                                                            const float* __restrict__ trim, int iters, float* __restrict__ out,
                                                            int32_t* __restrict__ used) {
  const int n3 = n_rot + n_vec, nch = n3 + n_lin, W = 3 * n3 + n_lin;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)T * nch) return;
  const int t = (int)(idx / nch), j = (int)(idx - (long long)t * nch);
  const bool rot = j < n_rot;
  Window w;
  w.rows = rows; w.taps = taps; w.weights = weights;
  w.w_stride = w_cols; w.w_col = w_cols == 1 ? 0 : j;                 // (nch == 1: both readings of w_cols == 1 are column 0)
  w.W = W; w.nc = j < n3 ? 3 : 1; w.c0 = j < n3 ? 3 * j : 3 * n3 + (j - n3); w.t = t;
  w.ox = w.oy = w.oz = 0.0f;
  if (rot && rot_offset) { w.ox = rot_offset[w.c0]; w.oy = rot_offset[w.c0 + 1]; w.oz = rot_offset[w.c0 + 2]; }
  // the window: the largest d <= R with every row t +- d' (d' <= d) inside the clip and inside the centre's segment
  int Rt = 0;
  const int seg_t = segment ? segment[t] : 0;
  for (int d = 1; d <= R; ++d) {
    if (t - d < 0 || t + d >= T) break;
    if (segment && (segment[t - d] != seg_t || segment[t + d] != seg_t)) break;
    Rt = d;
  }
  w.Rt = Rt;
  Mask all{true, Rt > 0 ? ~0ull >> (64 - Rt) : 0ull, Rt > 0 ? ~0ull >> (64 - Rt) : 0ull};
  // used samples: a_s > 0 and finite values; nothing else is ever read again
  const Mask use = w.select(all, [&](int s, int d) {
    float x, y, z;
    return w.weight(s, d) > 0.0f && w.load(s, x, y, z);
  });
  const int n = count(use);
  const float* src = rows + (size_t)t * W + w.c0;
  float* o = out + (size_t)t * W + w.c0;
  int32_t* u = used + (size_t)t * nch + j;
  if (n == 0 || (n == 1 && use.c)) {                                  // nothing to average, or the centre alone: the input, bit for bit
    for (int c = 0; c < w.nc; ++c) o[c] = src[c];
    *u = n;
    return;
  }
  const float tr = trim ? trim[j] : 0.0f;
  int n_final = n;
  if (!rot) {
    Vec3 m = w.mean(use);
    if (tr > 0.0f) {
      const Mask keep = w.select(use, [&](int s, int) {
        float x, y, z;
        w.load(s, x, y, z);
        const float dx = x - m.x, dy = y - m.y, dz = z - m.z;
        const float dist = w.nc == 1 ? fabsf(dx) : sqrtf(dx * dx + dy * dy + dz * dz);
        return !(dist > tr);
      });
      const int nk = count(keep);
      if (nk > 0 && nk < n) { m = w.mean(keep); n_final = nk; }
    }
    o[0] = m.x;
    if (w.nc == 3) { o[1] = m.y; o[2] = m.z; }
    *u = n_final;
    return;
  }
  Quat mu{1.0f, 0.0f, 0.0f, 0.0f};
  bool ok = w.rot_mean(use, iters, mu);
  if (ok && tr > 0.0f) {
    const Quat m0 = mu;
    const Mask keep = w.select(use, [&](int s, int) {
      const Vec3 l = log_of(qmul_conj(m0, w.quat(s)));
      return !(sqrtf(l.x * l.x + l.y * l.y + l.z * l.z) > tr);
    });
    const int nk = count(keep);
    if (nk > 0 && nk < n) { ok = w.rot_mean(keep, iters, mu); n_final = nk; }
  }
  if (!ok) {                                                          // antipodal samples: no mean to speak of
    for (int c = 0; c < 3; ++c) o[c] = src[c];
    *u = -1;
    return;
  }
  const Vec3 l = log_of(mu);
  o[0] = l.x - w.ox; o[1] = l.y - w.oy; o[2] = l.z - w.oz;
  *u = n_final;
}

}  // namespace

extern "C" int harp_motion_filter(const float* rows, int T, int n_rot, int n_vec, int n_lin, const float* rot_offset, const float* taps, int R,
                                  const float* weights, int w_cols, const int32_t* segment, const float* trim, int iters, float* out,
                                  int32_t* used, hipStream_t stream) {
  if (!rows || !taps || !out || !used || T <= 0 || n_rot < 0 || n_vec < 0 || n_lin < 0) return HARP_ERR_ARG;
  if (R < 0 || R > HARP_FILTER_MAX_RADIUS || iters < 0 || iters > 8) return HARP_ERR_ARG;
  const long long nch = (long long)n_rot + n_vec + n_lin, W = 3LL * n_rot + 3LL * n_vec + n_lin;
  if (nch == 0 || W * T > 0x7fffffffLL) return HARP_ERR_ARG;          // (so T nch <= T W fits an int as well)
  if (weights ? (w_cols != 1 && w_cols != nch) : w_cols != 0) return HARP_ERR_ARG;
  const long long lanes = nch * T;
  hipLaunchKernelGGL(motion_filter_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, rows, T, n_rot, n_vec, n_lin, rot_offset,
                     taps, R, weights, w_cols, segment, trim, iters, out, used);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
