// Image metrics of the post-fit evaluation (optimize_sequence.py:595-816 -> utils/eval_util.py:10-60): MS-SSIM with the semantics of
// pytorch_msssim 0.2.1 (MS_SSIM(data_range=1, size_average=True, channel=3), eval_util.py:8, 56-60), plus the silhouette IoU counts
// (:41-49) and the L1 sum (:34-38) read in the same level-0 pass.
//
// One launch per pyramid level, then one finish launch:
//   level kernel — one workgroup per (32 x 32 output tile of the valid map, image); for each channel it stages the (32+10)^2 input patch
//     of X and Y in LDS, runs the horizontal 11-tap pass into five LDS moment planes and the vertical pass in registers (4 outputs per
//     thread), and writes the tile's sums of the ssim and cs maps into its own record.  While the patch is staged it also writes the
//     2x2 average pool of the pixels it owns for the next level (avg_pool2d(2, stride 2, padding (H%2, W%2)), count_include_pad) and, at
//     level 0, the |X - Y| sum and the >= 0.5 mask counts of the pixels it owns (the tiles' owned ranges partition the FULL image).
//   finish kernel — one wave per image: sums the tile records in a fixed order in float64, forms the per-level means, relu, the weight
//     powers and the channel mean.
// No atomics anywhere: every workgroup writes its own slot, so two calls give bit-identical results.
//
// Accuracy: E[x^2] - mu^2 cancels in float32 wherever the window is nearly flat (a rendered frame's background, a constant image), where
// an error of one ulp of x^2 is a large fraction of C2 = 9e-4.  So every moment is taken about the window's own centre pixel: the
// horizontal pass forms sums of (x - c) with c = the centre of its 11-pixel row segment, and the vertical pass moves each row's sums to
// the centre pixel C of the 11 x 11 window before adding them (sum w (x - C)^2 = q + 2 d a + S d^2 with d = c - C, S = sum of the taps).
// The package's variance  sum w x^2 - mu^2  then follows without cancellation as  E' - u^2 - C^2 k  with E' = sum w (x - C)^2,
// u = mu - C = m + C k, m = sum w (x - C) and k = S^2 - 1 (-6.1e-8 for the float32 taps of sigma 1.5: the window does not sum to exactly
// 1, and the package's formula is not shift-invariant by that much).  An identical pair gives exactly cs = ssim = 1.
#include <math.h>
#include "harp_common.h"
#include "harp_hip.h"

namespace {

constexpr int kT = 32;                 // output tile side
constexpr int kWin = 11;               // Gaussian window (pytorch_msssim default; the only size supported)
constexpr int kP = kT + kWin - 1;      // staged patch side
constexpr int kThreads = 256;
constexpr int kMaxLevels = 5;
constexpr int kMaxC = 3;
constexpr int kRec = 16;               // floats per tile record: ssim sums [0,3), cs sums [3,6), l1 [6], inter [7], union [8]
constexpr int kMinSide = (kWin - 1) * 16;   // pytorch_msssim asserts min(H, W) > (win_size - 1) * 2^4

struct Taps {
  float w[kWin];
};

struct LevelArgs {
  const float* x;
  const float* y;
  long long sn, sc, sy, sx;            // element strides of x and y
  int H, W, C;
  const float* mx;                     // level 0 only: (N,H,W) masks, NULL = no IoU
  const float* my;
  float* px;                           // pooled next level (N,C,ph,pw), NULL at the last level
  float* py;
  int ph, pw;
  float* part;                         // (N, tiles_y * tiles_x) records of kRec floats
  int tiles_x, tiles_y;
  float C1, C2, S, k;                  // S = sum of the taps, k = S^2 - 1 (formed in float64)
  int level0;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// fixed-order sum over the workgroup; every thread gets the result
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int wid = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wid] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(kThreads) ssim_level_kernel(LevelArgs a, Taps tp) {
  __shared__ float X[kP * kP];
  __shared__ float Y[kP * kP];
  __shared__ float mom[5][kP * kT];    // horizontal pass: sum w dx, w dy, w dx^2, w dy^2, w dx dy per (staged row, output column)
  __shared__ float red[2][4];

  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int tile = blockIdx.x;
  const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
  const int oy = ty * kT, ox = tx * kT;
  const int Ho = a.H - (kWin - 1), Wo = a.W - (kWin - 1);
  // input pixels this tile owns (for the pool, L1 and IoU): its own 32 rows / columns, the last tile also the 10-pixel tail
  const int own_y0 = oy, own_y1 = (ty == a.tiles_y - 1) ? a.H : oy + kT;
  const int own_x0 = ox, own_x1 = (tx == a.tiles_x - 1) ? a.W : ox + kT;
  // pooled outputs i owned: input row 2i - pad in [own_y0, own_y1) (row -1 of the zero padding goes with row 0)
  const int pady = a.H & 1, padx = a.W & 1;
  const int pi0 = own_y0 == 0 ? 0 : (own_y0 + pady + 1) >> 1, pi1 = (own_y1 + pady + 1) >> 1;
  const int pj0 = own_x0 == 0 ? 0 : (own_x0 + padx + 1) >> 1, pj1 = (own_x1 + padx + 1) >> 1;
  const float S = a.S, kk = a.k;

  float l1 = 0.f, inter = 0.f, uni = 0.f;
  const long long nbase = (long long)n * a.sn;

  for (int c = 0; c < a.C; ++c) {
    const long long cbase = nbase + (long long)c * a.sc;
    __syncthreads();                                   // the previous channel's readers are done with X / Y / mom
    for (int idx = tid; idx < kP * kP; idx += kThreads) {
      const int r = idx / kP, q = idx - r * kP;
      const int gy = oy + r, gx = ox + q;
      float xv = 0.f, yv = 0.f;
      if (gy < a.H && gx < a.W) {
        const long long off = cbase + (long long)gy * a.sy + (long long)gx * a.sx;
        xv = a.x[off];
        yv = a.y[off];
        if (a.level0 && gy < own_y1 && gx < own_x1) {    // (gy >= own_y0 = oy and gx >= own_x0 = ox always)
          l1 += fabsf(xv - yv);
          if (c == 0 && a.mx) {
            const long long mo = ((long long)n * a.H + gy) * a.W + gx;
            const bool rb = a.mx[mo] >= 0.5f, pb = a.my[mo] >= 0.5f;
            inter += (rb && pb) ? 1.f : 0.f;
            uni += (rb || pb) ? 1.f : 0.f;
          }
        }
      }
      X[idx] = xv;
      Y[idx] = yv;
    }
    __syncthreads();

    if (a.px) {                                        // next pyramid level, from the staged (exact) values
      const int pw_ = pj1 - pj0, cnt = (pi1 - pi0) * pw_;
      const long long pbase = ((long long)n * a.C + c) * a.ph * a.pw;
      for (int idx = tid; idx < cnt; idx += kThreads) {
        const int i = pi0 + idx / pw_, j = pj0 + idx % pw_;
        if (i >= a.ph || j >= a.pw) continue;
        const int r0 = 2 * i - pady - oy, c0 = 2 * j - padx - ox;      // local rows r0, r0+1 and columns c0, c0+1 (r0 or c0 may be -1: padding)
        float sxv = 0.f, syv = 0.f;                     // avg_pool2d's order: rows outer, columns inner, padded taps skipped, / 4
        for (int dr = 0; dr < 2; ++dr) {
          const int r = r0 + dr;
          if (r + oy < 0) continue;
          for (int dc = 0; dc < 2; ++dc) {
            const int q = c0 + dc;
            if (q + ox < 0) continue;
            sxv += X[r * kP + q];
            syv += Y[r * kP + q];
          }
        }
        a.px[pbase + (long long)i * a.pw + j] = sxv / 4.f;
        a.py[pbase + (long long)i * a.pw + j] = syv / 4.f;
      }
    }

    // horizontal pass about each row segment's centre pixel
    for (int idx = tid; idx < kP * kT; idx += kThreads) {
      const int r = idx >> 5, j = idx & (kT - 1);
      const float* xr = X + r * kP + j;
      const float* yr = Y + r * kP + j;
      const float cx = xr[kWin / 2], cy = yr[kWin / 2];
      float sa = 0.f, sb = 0.f, sq = 0.f, sqy = 0.f, sp = 0.f;
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const float dx = xr[k] - cx, dy = yr[k] - cy;
        const float t = tp.w[k] * dx, u = tp.w[k] * dy;
        sa += t;
        sb += u;
        sq = fmaf(t, dx, sq);
        sqy = fmaf(u, dy, sqy);
        sp = fmaf(t, dy, sp);
      }
      mom[0][idx] = sa;
      mom[1][idx] = sb;
      mom[2][idx] = sq;
      mom[3][idx] = sqy;
      mom[4][idx] = sp;
    }
    __syncthreads();

    // vertical pass: column j, output rows 4g .. 4g+3, about each window's centre pixel
    const int j = tid & (kT - 1), g = tid >> 5;
    float mx[4], my[4], exx[4], eyy[4], exy[4], Cx[4], Cy[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      mx[o] = my[o] = exx[o] = eyy[o] = exy[o] = 0.f;
      Cx[o] = X[(4 * g + o + kWin / 2) * kP + j + kWin / 2];
      Cy[o] = Y[(4 * g + o + kWin / 2) * kP + j + kWin / 2];
    }
#pragma unroll
    for (int rr = 0; rr < kWin + 3; ++rr) {
      const int r = 4 * g + rr;
      const float ra = mom[0][r * kT + j], rb = mom[1][r * kT + j], rq = mom[2][r * kT + j], rqy = mom[3][r * kT + j], rp = mom[4][r * kT + j];
      const float cx = X[r * kP + j + kWin / 2], cy = Y[r * kP + j + kWin / 2];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int k = rr - o;
        if (k < 0 || k >= kWin) continue;
        const float w = tp.w[k];
        const float dx = cx - Cx[o], dy = cy - Cy[o];
        mx[o] = fmaf(w, fmaf(S, dx, ra), mx[o]);
        my[o] = fmaf(w, fmaf(S, dy, rb), my[o]);
        // sum w (x-C)(y-D) = p + dx (b + S dy) + dy a; the squares in the same form, so an identical pair gives exy == exx bit for bit
        exx[o] = fmaf(w, fmaf(dx, ra, fmaf(dx, fmaf(S, dx, ra), rq)), exx[o]);
        eyy[o] = fmaf(w, fmaf(dy, rb, fmaf(dy, fmaf(S, dy, rb), rqy)), eyy[o]);
        exy[o] = fmaf(w, fmaf(dy, ra, fmaf(dx, fmaf(S, dy, rb), rp)), exy[o]);
      }
    }
    float ssum = 0.f, csum = 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int gi = oy + 4 * g + o, gj = ox + j;
      if (gi < Ho && gj < Wo) {
#pragma clang fp contract(off)
        const float u = mx[o] + Cx[o] * kk, v = my[o] + Cy[o] * kk;     // mu - C
        const float s1 = (exx[o] - u * u) - (Cx[o] * Cx[o]) * kk;
        const float s2 = (eyy[o] - v * v) - (Cy[o] * Cy[o]) * kk;
        const float s12 = (exy[o] - u * v) - (Cx[o] * Cy[o]) * kk;
        const float mu1 = Cx[o] + u, mu2 = Cy[o] + v;
        const float cs = (2.f * s12 + a.C2) / ((s1 + s2) + a.C2);
        const float lum = (2.f * (mu1 * mu2) + a.C1) / ((mu1 * mu1 + mu2 * mu2) + a.C1);
        ssum += lum * cs;
        csum += cs;
      }
    }
    ssum = block_sum(ssum, red[0]);
    csum = block_sum(csum, red[1]);
    if (tid == 0) {
      float* rec = a.part + ((long long)n * a.tiles_x * a.tiles_y + tile) * kRec;
      rec[c] = ssum;
      rec[kMaxC + c] = csum;
    }
  }
  if (a.level0) {
    l1 = block_sum(l1, red[0]);
    inter = block_sum(inter, red[1]);
    uni = block_sum(uni, red[0]);
    if (tid == 0) {
      float* rec = a.part + ((long long)n * a.tiles_x * a.tiles_y + tile) * kRec;
      rec[6] = l1;
      rec[7] = inter;
      rec[8] = uni;
    }
  }
}

struct FinishArgs {
  const float* part[kMaxLevels];
  int tiles[kMaxLevels];
  double count[kMaxLevels];            // valid-map pixels per level
  float w[kMaxLevels];
  int L, C;
  float* out;
};

__global__ void __launch_bounds__(64) ssim_finish_kernel(FinishArgs f) {
  __shared__ double ss[kMaxLevels * kMaxC], cc[kMaxLevels * kMaxC];
  const int n = blockIdx.x, t = threadIdx.x;
  const int LC = f.L * f.C, stride = 4 + 2 * LC;
  float* o = f.out + (long long)n * stride;
  if (t < LC) {
    const int l = t / f.C, c = t % f.C;
    const float* p = f.part[l] + (long long)n * f.tiles[l] * kRec;
    double s = 0.0, cs = 0.0;
    for (int i = 0; i < f.tiles[l]; ++i) {
      s += (double)p[i * kRec + c];
      cs += (double)p[i * kRec + kMaxC + c];
    }
    s /= f.count[l];
    cs /= f.count[l];
    ss[t] = s;
    cc[t] = cs;
    o[4 + t] = (float)s;
    o[4 + LC + t] = (float)cs;
  } else if (t >= 32 && t < 35) {                      // 6: l1, 7: inter, 8: union of level 0
    const float* p = f.part[0] + (long long)n * f.tiles[0] * kRec;
    double s = 0.0;
    for (int i = 0; i < f.tiles[0]; ++i) s += (double)p[i * kRec + 6 + (t - 32)];
    o[(t == 32) ? 2 : (t == 33 ? 0 : 1)] = (float)s;
  }
  __syncthreads();
  if (t == 0) {
    double ms = 0.0;
    for (int c = 0; c < f.C; ++c) {
      double prod = 1.0;
      for (int l = 0; l < f.L - 1; ++l) prod *= pow(fmax(cc[l * f.C + c], 0.0), (double)f.w[l]);
      prod *= pow(fmax(ss[(f.L - 1) * f.C + c], 0.0), (double)f.w[f.L - 1]);
      ms += prod;
    }
    o[3] = (float)(ms / f.C);
  }
}

struct Plan {
  int h[kMaxLevels], w[kMaxLevels], tx[kMaxLevels], ty[kMaxLevels];
  size_t pyr_x[kMaxLevels], pyr_y[kMaxLevels], part[kMaxLevels];
  size_t bytes;
};

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// workspace: for levels 1..4 the pooled X and Y (N, 3, h_l, w_l) float32, then for levels 0..4 the tile records (N, tiles_l, 16) float32;
// every block 256-B aligned; h_{l+1} = (h_l + 1) / 2, tiles_l = ceil((h_l - 10) / 32) * ceil((w_l - 10) / 32)
Plan plan(int N, int H, int W) {
  Plan p;
  size_t off = 0;
  for (int l = 0; l < kMaxLevels; ++l) {
    p.h[l] = l == 0 ? H : (p.h[l - 1] + 1) / 2;
    p.w[l] = l == 0 ? W : (p.w[l - 1] + 1) / 2;
    p.ty[l] = (p.h[l] - (kWin - 1) + kT - 1) / kT;
    p.tx[l] = (p.w[l] - (kWin - 1) + kT - 1) / kT;
  }
  for (int l = 1; l < kMaxLevels; ++l) {
    const size_t b = align256((size_t)N * kMaxC * p.h[l] * p.w[l] * sizeof(float));
    p.pyr_x[l] = off;
    off += b;
    p.pyr_y[l] = off;
    off += b;
  }
  for (int l = 0; l < kMaxLevels; ++l) {
    p.part[l] = off;
    off += align256((size_t)N * p.tx[l] * p.ty[l] * kRec * sizeof(float));
  }
  p.bytes = off;
  return p;
}

}  // namespace

extern "C" size_t harp_image_metrics_ws_bytes(int N, int H, int W) {
  if (N < 1 || H <= kMinSide || W <= kMinSide) return 0;
  return plan(N, H, W).bytes;
}

extern "C" int harp_image_metrics(const float* ref, const float* pred, const float* ref_mask, const float* pred_mask, long long sn,
                                  long long sc, long long sy, long long sx, int N, int C, int H, int W, float data_range,
                                  const float* weights, int n_levels, float K1, float K2, float sigma, void* ws, float* out,
                                  hipStream_t stream) {
  if (!ref || !pred || !ws || !out || !weights || ((ref_mask == nullptr) != (pred_mask == nullptr))) return HARP_ERR_ARG;
  if (N < 1 || N > 65535 || C < 1 || C > kMaxC || H <= kMinSide || W <= kMinSide || n_levels < 1 || n_levels > kMaxLevels) return HARP_ERR_ARG;
  if (!(sigma > 0.f) || !isfinite(data_range) || ((size_t)ws & 15)) return HARP_ERR_ARG;
  const Plan p = plan(N, H, W);
  char* base = (char*)ws;
  Taps tp;                                             // pytorch_msssim _fspecial_gauss_1d, in float32
  float tsum = 0.f;
  for (int i = 0; i < kWin; ++i) {
    const float c = (float)(i - kWin / 2);
    tp.w[i] = expf(-(c * c) / (2.f * sigma * sigma));
    tsum += tp.w[i];
  }
  for (int i = 0; i < kWin; ++i) tp.w[i] /= tsum;
  double Sd = 0.0;
  for (int i = 0; i < kWin; ++i) Sd += (double)tp.w[i];
  const double r = (double)data_range;
  const float C1 = (float)((K1 * r) * (K1 * r)), C2 = (float)((K2 * r) * (K2 * r));
  for (int l = 0; l < n_levels; ++l) {
    LevelArgs a;
    if (l == 0) {
      a.x = ref;
      a.y = pred;
      a.sn = sn; a.sc = sc; a.sy = sy; a.sx = sx;
    } else {
      a.x = (const float*)(base + p.pyr_x[l]);
      a.y = (const float*)(base + p.pyr_y[l]);
      a.sx = 1; a.sy = p.w[l]; a.sc = (long long)p.h[l] * p.w[l]; a.sn = a.sc * C;
    }
    a.H = p.h[l];
    a.W = p.w[l];
    a.C = C;
    a.level0 = l == 0;
    a.mx = l == 0 ? ref_mask : nullptr;
    a.my = l == 0 ? pred_mask : nullptr;
    const bool pool = l + 1 < n_levels;
    a.px = pool ? (float*)(base + p.pyr_x[l + 1]) : nullptr;
    a.py = pool ? (float*)(base + p.pyr_y[l + 1]) : nullptr;
    a.ph = pool ? p.h[l + 1] : 0;
    a.pw = pool ? p.w[l + 1] : 0;
    a.part = (float*)(base + p.part[l]);
    a.tiles_x = p.tx[l];
    a.tiles_y = p.ty[l];
    a.C1 = C1;
    a.C2 = C2;
    a.S = (float)Sd;
    a.k = (float)(Sd * Sd - 1.0);
    ssim_level_kernel<<<dim3((unsigned)(p.tx[l] * p.ty[l]), (unsigned)N), kThreads, 0, stream>>>(a, tp);
    HARP_CHECK_LAUNCH();
  }
  FinishArgs f;
  for (int l = 0; l < kMaxLevels; ++l) {
    f.part[l] = (const float*)(base + p.part[l]);
    f.tiles[l] = p.tx[l] * p.ty[l];
    f.count[l] = (double)(p.h[l] - (kWin - 1)) * (double)(p.w[l] - (kWin - 1));
    f.w[l] = l < n_levels ? weights[l] : 0.f;
  }
  f.L = n_levels;
  f.C = C;
  f.out = out;
  ssim_finish_kernel<<<N, 64, 0, stream>>>(f);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
