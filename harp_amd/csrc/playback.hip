// Playback of a fitted avatar (harp_amd/playback.py): the two kernels the forward-only player needs beside the fit's own
// front, rasterisers and shader.  The reference animates a fit by overwriting pose rows (utils/visualize.py:111-143 change_pose) and
// quantises its renders on the host (:258-320 followed by `(img * 255).astype(np.uint8)`).
//
// harp_motion_resample: key-frame rows (Tk, 3 n_rot + n_lin) -> rows at fractional times (Tn, 3 n_rot + n_lin).  The n_rot axis-angle
//   triples are interpolated as ROTATIONS (quaternion slerp along the shortest arc, nlerp when the two are closer than acos(0.9995)),
//   after rot_offset has been added and before it is subtracted again (MANO stores its finger joints relative to hands_mean, csrc/lbs.hip:35);
//   the n_lin channels behind them linearly.  A time is clamped to [0, Tk - 1] (NaN -> 0); a time ON a key copies that row bit for bit.
//   One lane per (output row, rotation or linear channel): at most two rows of 12 bytes in, 12 bytes out; no LDS, no atomics.
// harp_resolve_u8: a render supersampled ss x ss, rgb (B, S ss, S ss, 3) float32 with its coverage face_id (B, S ss, S ss) (>= 0: covered),
//   box-filtered over a uint8 background into finished (B,S,S,3|4) uint8 frames; alpha = the covered share, rounded in integers.
//   One lane per output pixel; a lane's ss sub-rows are 12 ss contiguous bytes of rgb and 4 ss of face_id each, read as 8- / 16-byte
//   words where ss and the address allow; neighbouring lanes read neighbouring words.  RGBA leaves as one 32-bit store per lane.
//   Every index is derived from (b, y, x) < (B, S, S) and a background row checked against n_bg: nothing is read or written out of bounds.
// Both are bound by memory traffic; both only enqueue on the caller's stream.
#include "harp_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct Quat { float w, x, y, z; };

// axis-angle -> unit quaternion; sin(t/2)/t by its series below 1e-4 (the quotient is 0/0 at the identity)
__device__ __forceinline__ Quat quat_of(float ax, float ay, float az) {
  const float t2 = ax * ax + ay * ay + az * az, t = sqrtf(t2);
  const float s = t < 1e-4f ? 0.5f - t2 * (1.0f / 48.0f) : sinf(0.5f * t) / t;
  return Quat{cosf(0.5f * t), s * ax, s * ay, s * az};
}

__global__ void __launch_bounds__(256) motion_resample_kernel(const float* __restrict__ keys, int Tk, int n_rot, int n_lin,
                                                              const float* __restrict__ rot_offset, const float* __restrict__ times, int Tn,
                                                              float* __restrict__ out) {
  const int nch = n_rot + n_lin, W = 3 * n_rot + n_lin;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)Tn * nch) return;
  const int i = (int)(idx / nch), j = (int)(idx - (long long)i * nch);
  const float t = fminf(fmaxf(times[i], 0.0f), (float)(Tk - 1));      // fmaxf(NaN, 0) = 0: a NaN time is row 0
  int k = min((int)t, Tk - 2);
  if (k < 0) k = 0;                                                   // (Tk == 1: t = 0, row 0)
  const float f = t - (float)k;
  const bool rot = j < n_rot;
  const int c0 = rot ? 3 * j : 3 * n_rot + (j - n_rot), nc = rot ? 3 : 1;
  float* o = out + (size_t)i * W + c0;
  if (f == 0.0f || f == 1.0f) {                                       // on a key: that row, bit for bit (row k + 1 exists when f == 1: Tk >= 2)
    const float* src = keys + (size_t)(f == 0.0f ? k : k + 1) * W + c0;
    for (int c = 0; c < nc; ++c) o[c] = src[c];
    return;
  }
  const float* a = keys + (size_t)k * W + c0;
  const float* b = a + W;
  if (!rot) {
    o[0] = (1.0f - f) * a[0] + f * b[0];
    return;
  }
  float off[3] = {0.0f, 0.0f, 0.0f};
  if (rot_offset) { off[0] = rot_offset[c0]; off[1] = rot_offset[c0 + 1]; off[2] = rot_offset[c0 + 2]; }
  const Quat q0 = quat_of(a[0] + off[0], a[1] + off[1], a[2] + off[2]);
  Quat q1 = quat_of(b[0] + off[0], b[1] + off[1], b[2] + off[2]);
  float d = q0.w * q1.w + q0.x * q1.x + q0.y * q1.y + q0.z * q1.z;
  if (d < 0.0f) { d = -d; q1.w = -q1.w; q1.x = -q1.x; q1.y = -q1.y; q1.z = -q1.z; }      // q and -q are one rotation: the shorter arc
  float s0 = 1.0f - f, s1 = f;                                        // nlerp: the two are within 1.8 degrees, sin(Omega) loses its digits
  if (d <= 0.9995f) {
    const float om = acosf(d), is = 1.0f / sinf(om);
    s0 = sinf((1.0f - f) * om) * is;
    s1 = sinf(f * om) * is;
  }
  float w = s0 * q0.w + s1 * q1.w, x = s0 * q0.x + s1 * q1.x, y = s0 * q0.y + s1 * q1.y, z = s0 * q0.z + s1 * q1.z;
  const float inv = 1.0f / sqrtf(w * w + x * x + y * y + z * z);
  w *= inv; x *= inv; y *= inv; z *= inv;
  if (w < 0.0f) { w = -w; x = -x; y = -y; z = -z; }                   // w >= 0: an angle in [0, pi]
  const float vn = sqrtf(x * x + y * y + z * z);
  const float g = vn < 1e-8f ? 2.0f : 2.0f * atan2f(vn, w) / vn;
  o[0] = g * x - off[0];
  o[1] = g * y - off[1];
  o[2] = g * z - off[2];
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }      // (NaN -> 0)
__device__ __forceinline__ unsigned quantise(float v) { return (unsigned)min(max((int)(255.0f * v + 0.5f), 0), 255); }

// SS * 3 floats / SS ints of one sub-row of a lane's pixel, as the widest words its address allows
template <int SS>
__device__ __forceinline__ void load_row(const float* p, const int32_t* q, float (&c)[SS * 3], int (&id)[SS]) {
  constexpr int kVec = SS == 4 ? 4 : (SS == 2 ? 2 : 1);              // floats / ints per word: a sub-row starts on a multiple of SS elements
  if constexpr (kVec == 4) {
    if ((((uintptr_t)p | (uintptr_t)q) & 15) == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float4 v = ((const float4*)p)[k];
        c[4 * k] = v.x; c[4 * k + 1] = v.y; c[4 * k + 2] = v.z; c[4 * k + 3] = v.w;
      }
      const int4 u = *(const int4*)q;
      id[0] = u.x; id[1] = u.y; id[2] = u.z; id[3] = u.w;
      return;
    }
  } else if constexpr (kVec == 2) {
    if ((((uintptr_t)p | (uintptr_t)q) & 7) == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float2 v = ((const float2*)p)[k];
        c[2 * k] = v.x; c[2 * k + 1] = v.y;
      }
      const int2 u = *(const int2*)q;
      id[0] = u.x; id[1] = u.y;
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < SS * 3; ++k) c[k] = p[k];
#pragma unroll
  for (int k = 0; k < SS; ++k) id[k] = q[k];
}

template <int SS, int CH>
__global__ void __launch_bounds__(256) resolve_u8_kernel(const float* __restrict__ rgb, const int32_t* __restrict__ face_id, int B, int S,
                                                         const unsigned char* __restrict__ bg, int n_bg, const int32_t* __restrict__ bg_rows,
                                                         const float* __restrict__ bg_color, unsigned char* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)S * S;
  if (idx >= per * B) return;
  const int b = (int)(idx / per);
  const int rem = (int)(idx - (long long)b * per), y = rem / S, x = rem - y * S;
  // the background of this pixel: a byte triple of frame `row`, or the constant colour quantised like a pixel
  unsigned bgb[3];
  const int row = bg_rows ? bg_rows[b] : (n_bg == B ? b : 0);
  if (bg && row >= 0 && row < n_bg) {
    const unsigned char* pb = bg + ((size_t)row * per + rem) * 3;
    bgb[0] = pb[0]; bgb[1] = pb[1]; bgb[2] = pb[2];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) bgb[c] = quantise(clamp01(bg_color[c]));
  }
  const size_t Sh = (size_t)S * SS;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  int n = 0;
#pragma unroll
  for (int sy = 0; sy < SS; ++sy) {
    const size_t p0 = ((size_t)b * Sh + (size_t)y * SS + sy) * Sh + (size_t)x * SS;
    float c[SS * 3];
    int id[SS];
    load_row<SS>(rgb + p0 * 3, face_id + p0, c, id);
#pragma unroll
    for (int sx = 0; sx < SS; ++sx)
      if (id[sx] >= 0) {
        ++n;
        sum[0] += clamp01(c[3 * sx]); sum[1] += clamp01(c[3 * sx + 1]); sum[2] += clamp01(c[3 * sx + 2]);
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
}

}  // namespace

extern "C" int harp_motion_resample(const float* keys, int Tk, int n_rot, int n_lin, const float* rot_offset, const float* times, int Tn,
                                    float* out, hipStream_t stream) {
  if (!keys || !times || !out || Tk <= 0 || Tn <= 0 || n_rot < 0 || n_lin < 0 || (long long)n_rot + n_lin == 0) return HARP_ERR_ARG;
  // the 1-D grid, the kernel's int row width and (int) time -> key index: all far below 2^31
  const long long nch = (long long)n_rot + n_lin, W = 3LL * n_rot + n_lin, lanes = nch * Tn;
  if (W > 0x7fffffffLL || Tk > (1 << 24) || lanes > 0x7fffffffLL * 256) return HARP_ERR_ARG;
  hipLaunchKernelGGL(motion_resample_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, keys, Tk, n_rot, n_lin, rot_offset,
                     times, Tn, out);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

extern "C" int harp_resolve_u8(const float* rgb, const int32_t* face_id, int B, int S, int ss, const unsigned char* bg, int n_bg,
                               const int32_t* bg_rows, const float* bg_color, int channels, unsigned char* out, hipStream_t stream) {
  if (!rgb || !face_id || !out || !bg_color || B <= 0 || S <= 0 || ss < 1 || ss > 4 || (channels != 3 && channels != 4)) return HARP_ERR_ARG;
  if (bg && (n_bg <= 0 || (!bg_rows && n_bg != 1 && n_bg != B))) return HARP_ERR_ARG;
  if ((long long)S * ss > 46340LL) return HARP_ERR_ARG;               // (S ss)^2 and S^2 fit an int
  const long long px = (long long)S * S * B;
  if (px > 0x7fffffffLL * 256) return HARP_ERR_ARG;
  const dim3 grid((unsigned)((px + 255) / 256)), block(256);
  if (!bg) n_bg = 0;
#define HARP_RESOLVE(SS, CH) hipLaunchKernelGGL((resolve_u8_kernel<SS, CH>), grid, block, 0, stream, rgb, face_id, B, S, bg, n_bg, bg_rows, bg_color, out)
#define HARP_RESOLVE_SS(SS) do { if (channels == 4) HARP_RESOLVE(SS, 4); else HARP_RESOLVE(SS, 3); } while (0)
  switch (ss) {
    case 1: HARP_RESOLVE_SS(1); break;
    case 2: HARP_RESOLVE_SS(2); break;
    case 3: HARP_RESOLVE_SS(3); break;
    default: HARP_RESOLVE_SS(4); break;
  }
#undef HARP_RESOLVE_SS
#undef HARP_RESOLVE
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
