// Second half of the texel gradient of the shader backward (harp_shade_args.trec, include/harp_hip.h): the backward of
// TexturesUV.sample_textures / F.grid_sample(bilinear, align_corners=True) (renderer/renderer_helper.py:472-523,
// renderer/pbr_materials.py:82-124) as "emit, then reduce by owner".
//
// Why: scattered from the pixel side, the 4 corners x 6 channels of every shaded pixel cost the shader backward a 6.3-KB LDS table per
// wave, its flush and 11.8 M memory-side float atomics per launch (C3) — while the 1.39 M shaded pixels of the 32 frames of a step land
// on only ~44 k distinct texels (all frames show the same chart of the same atlas).  The pixel pass now appends one 36-byte record per
// pixel to the list of the 32x32-texel UV tile its footprint starts in (coalesced 4-byte planes); here a workgroup owns one chunk of
// one tile's list, accumulates the footprints in a (33 x 33 texel) x 6 channel 64-bit fixed-point table in LDS (ds_add_u64, one
// scale per map and chunk: order-independent sums) and adds the table to the maps with row-contiguous memory atomics:
// ~0.3 M atomics per tile chunk set instead of 11.8 M, and the kernel feeds nothing but the optimiser — it runs beside the mesh / hand
// backward tail, off the step's critical path.
#include <stdlib.h>
#include "harp_common.h"
#include "harp_hip.h"

namespace {

constexpr int kBin = 32;                       // texels per tile side
constexpr int kAcc = kBin + 1;                 // + the row / column the last footprints reach into
constexpr int kChunk = 2048;                   // records per workgroup pass
constexpr int kThreads = 512;
constexpr int kMaxBins = 1024;                 // (1024 x 1024 texels)

// power-of-two scale s with |x| * s < 2^40 for every |x| <= m; inv = 1 / s exactly
__device__ __forceinline__ void fixed_scale40(float m, double& s, double& inv) {
  int e = ((__float_as_int(m) >> 23) & 0xff) - 126;          // m < 2^e
  e = min(max(e, -100), 100);
  s = __longlong_as_double((long long)(1023 + 40 - e) << 52);
  inv = __longlong_as_double((long long)(1023 - 40 + e) << 52);
}
// rint(x) for |x| < 2^51 as a 64-bit integer: the integer sits in the low mantissa bits of x + 1.5 * 2^52 (gfx950 has no f64 -> i64 convert)
__device__ __forceinline__ long long to_fixed(double x) {
  return __double_as_longlong(x + 6755399441055744.0) - 0x4338000000000000ll;
}

// One map's share of a thread's four consecutive records: every corner contribution in fixed point exactly as a record on its own would add it
// (same product, same scale, same to_fixed, same guards), but records j, j + 1 of one texel row whose footprints start on the same texel or on
// x-neighbouring ones (dx = 0, +1, -1) name the same table cells in the columns they share: those integers are added in registers first and
// the cell gets ONE ds_add_u64.  The pending footprint `pa` hands the shared columns on to the next record and adds the others to the table; integer
// addition is associative, so the table is bit-identical to one atomic per record, corner and channel.  (Of the pixels of a frame row, half share
// their top-left texel with the next and more their column x0 + 1: ~4 distinct columns per thread instead of 8.)
template <int M>
__device__ __forceinline__ void add_records(long long* __restrict__ acc, const float (&rv)[4][9], int t, int n, int Wt, int Ht, double s) {
  long long pa[2][2][3];                       // pending footprint [column][row][channel]
  int px = 0, py = 0;
  auto flush = [&](int c) {                    // column c of the pending footprint -> table
    const int o = ((py & (kBin - 1)) * kAcc + (px & (kBin - 1)) + c) * 3;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        atomicAdd((unsigned long long*)&acc[o + r * kAcc * 3 + ch], (unsigned long long)pa[c][r][ch]);   // (a corner off the map or of weight 0 adds 0)
  };
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (4 * t + j < n) {
      const int key = __float_as_int(rv[j][0]);
      const int x0 = key & 0xffff, y0 = (int)((unsigned)key >> 16);
      const float wx = rv[j][1], wy = rv[j][2];
      const float ax = 1.f - wx, ay = 1.f - wy;
      const float cw[4] = {ax * ay, wx * ay, ax * wy, wx * wy};
      long long cur[2][2][3];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int cx = x0 + (k & 1), cy = y0 + (k >> 1);
        const bool on = cx < Wt && cy < Ht && cw[k] != 0.f;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) cur[k & 1][k >> 1][ch] = on ? to_fixed((double)(rv[j][3 + 3 * M + ch] * cw[k]) * s) : 0;
      }
      if (j > 0) {
        const int dx = x0 - px;
        const bool row = y0 == py, same = row && dx == 0, right = row && dx == 1, left = row && dx == -1;
        if (!(same || left)) flush(0);         // (column 0 goes on into the new column 0 when dx = 0, into its column 1 when dx = -1)
        if (!(same || right)) flush(1);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const long long a = pa[0][r][ch], b = pa[1][r][ch];
            cur[0][r][ch] += same ? a : right ? b : 0;
            cur[1][r][ch] += same ? b : left ? a : 0;
          }
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) pa[c][r][ch] = cur[c][r][ch];
      px = x0; py = y0;
    }
  }
  if (4 * t < n) { flush(0); flush(1); }
}

// kHalves = 2: a workgroup of 1024 threads whose halves each own a table and reduce a chunk of their own at the same time (nothing but the prefix
// at the top and the barriers is shared) — the launch shape of the small job, see harp_texel_reduce
template <int kHalves>
__global__ void __launch_bounds__(kThreads * kHalves) texel_reduce_kernel(const float* __restrict__ rec, int32_t* __restrict__ cnt, int cap, int nbins, int nbx,
                                                                          int Wt, int Ht, double* __restrict__ g_tex, double* __restrict__ g_nmap) {
  __shared__ long long acc[kHalves][2][kAcc * kAcc * 3];   // [half][map][(ly * 33 + lx) * 3 + channel], 64-bit fixed point (see the scales below)
  __shared__ float wmax[kHalves][2][kThreads / 64];
  __shared__ int pre[kMaxBins];                // inclusive prefix of the tiles' chunk counts
  __shared__ int cl[kMaxBins];                 // the tiles' record counts
  __shared__ int wsum[kHalves * kThreads / 64];
  constexpr int kAll = kThreads * kHalves;
  const int half = threadIdx.x / kThreads, t = threadIdx.x % kThreads, lane = t & 63, w = t >> 6;
  // ---- chunk counts of all tiles -> inclusive prefix (every workgroup forms it: nbins loads)
  int carry = 0;
  for (int b0 = 0; b0 < nbins; b0 += kAll) {
    const int b = b0 + (int)threadIdx.x, wa = (int)threadIdx.x >> 6;
    const int c = b < nbins ? min(cnt[16 * b], cap) : 0;
    int v = (c + kChunk - 1) / kChunk;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
    if (lane == 63) wsum[wa] = v;
    __syncthreads();
    int off = carry;
    for (int i = 0; i < wa; ++i) off += wsum[i];
    if (b < nbins) { pre[b] = v + off; cl[b] = c; }
    int tot = 0;
    for (int i = 0; i < kAll / 64; ++i) tot += wsum[i];
    carry += tot;
    __syncthreads();
  }
  const int total = carry;
  // thread t owns records 4 t .. 4 t + 3 of the chunk: one 16-byte load per plane, and — what matters — the lanes of a wave instruction
  // are then 4 records apart: x-neighbouring pixels of a frame that share a texel (half of 64 consecutive records are such duplicates,
  // up to 9 lanes on one texel) meet in ONE thread, one after the other, instead of in one LDS atomic instruction
  float rv[kChunk / kThreads][9];
  static_assert(kChunk / kThreads == 4, "one float4 per plane and thread");
  int next_bin = 0, next_n = 0;
  // tile and length of this half's chunk of the pass that starts at chunk c0, and its records on their way into rv.  Half h takes chunk
  // c0 + h * gridDim.x: the two chunks of a workgroup are a grid apart (mostly other tiles: their flushes do not meet in memory); the halves
  // share the barriers, so a half without a chunk walks an empty one (n = 0)
  auto fetch = [&](int c0) {
    const int chunk = c0 + half * (int)gridDim.x;
    // tile of this chunk: first b with pre[b] > chunk
    int lo = 0, hi = nbins - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (pre[mid] > chunk) hi = mid; else lo = mid + 1; }
    const int first = (chunk - (lo ? pre[lo - 1] : 0)) * kChunk;
    next_bin = lo;
    next_n = chunk < total ? min(cl[lo] - first, kChunk) : 0;
    const float* r0 = rec + (size_t)lo * 9 * (size_t)cap + (size_t)first;
    const size_t capz = (size_t)cap;
    const int i = 4 * t;
    if (i < next_n) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const float4 q = *(const float4*)(r0 + k * capz + i);   // (slots past n: stale, never used)
        rv[0][k] = q.x; rv[1][k] = q.y; rv[2][k] = q.z; rv[3][k] = q.w;
      }
    }
  };
  if ((int)blockIdx.x < total) fetch(blockIdx.x);
  for (int c0 = blockIdx.x; c0 < total; c0 += gridDim.x * kHalves) {
    const int bin = next_bin, n = next_n;
    for (int i = t; i < 2 * kAcc * kAcc * 3; i += kThreads) (&acc[half][0][0])[i] = 0;
    // 64-bit FIXED-POINT accumulators (ds_add_u64: 6.9 clk per wave instruction on gfx950 against 8.7 for ds_add_f64, which also pays ~11 clk
    // for every further lane on the same address — and neighbouring pixels of a frame DO share texels): one power-of-two scale per map and
    // chunk from the chunk's largest gradient component, |x| * s < 2^40; a texel takes at most one corner of each of the <= 2048 records
    // (weight <= 1): |sum| < 2^51.  Resolution 2^-40 of the chunk's largest component: every contribution down to 2^-16 of it keeps its whole
    // float mantissa, and the sum is independent of the order of the records (a 32-bit table at 2^-20 was measured first: its rounding of the
    // small contributions depends on what else is in the chunk, which Adam's sign-like first steps turned into visible differences between a
    // 2-rank and a 1-rank fit of the same frames).
    float m0 = 0.f, m1 = 0.f;
#pragma unroll
    for (int j = 0; j < kChunk / kThreads; ++j) {
      if (4 * t + j < n) {
        m0 = fmaxf(m0, fmaxf(fabsf(rv[j][3]), fmaxf(fabsf(rv[j][4]), fabsf(rv[j][5]))));
        m1 = fmaxf(m1, fmaxf(fabsf(rv[j][6]), fmaxf(fabsf(rv[j][7]), fabsf(rv[j][8]))));
      }
    }
    m0 = wave_max_u(m0); m1 = wave_max_u(m1);
    if (lane == 0) { wmax[half][0][w] = m0; wmax[half][1][w] = m1; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) { m0 = fmaxf(m0, wmax[half][0][i]); m1 = fmaxf(m1, wmax[half][1][i]); }
    double s0, i0, s1, i1;
    fixed_scale40(m0, s0, i0);
    fixed_scale40(m1, s1, i1);
    if (g_tex) add_records<0>(&acc[half][0][0], rv, t, n, Wt, Ht, s0);
    if (g_nmap) add_records<1>(&acc[half][1][0], rv, t, n, Wt, Ht, s1);
    __syncthreads();
    // the records of the next pass set out now (rv is free): their way from memory lies under the flush instead of in front of the next table phase
    if (c0 + (int)gridDim.x * kHalves < total) fetch(c0 + (int)gridDim.x * kHalves);
    // flush, lanes = (texel, channel) along a tile row: 99 consecutive floats per row
    const int bx = bin % nbx, by = bin / nbx;
    for (int i = t; i < kAcc * kAcc * 3; i += kThreads) {
      const int ly = i / (kAcc * 3), q = i - ly * (kAcc * 3);
      const int gx3 = bx * kBin * 3 + q, gy = by * kBin + ly;
      if (gy < Ht && gx3 < Wt * 3) {
        const size_t o = (size_t)gy * Wt * 3 + gx3;
        const long long a0 = acc[half][0][i], a1 = acc[half][1][i];
        if (g_tex && a0 != 0) atomicAdd(g_tex + o, (double)a0 * i0);          // (exact product: |a0| < 2^51, i0 a power of two)
        if (g_nmap && a1 != 0) atomicAdd(g_nmap + o, (double)a1 * i1);
      }
    }
    __syncthreads();
  }
}

// acc (n_texels, 3) doubles -> g (+=, float), acc cleared; with nmap_raw the normal map's chain rule rides along: acc is the gradient of the
// NORMALISED map F.normalize(nmap_raw, dim=-1) (utils/visualize.py:99) and g that of the raw one (harp_normalize3_bwd's arithmetic)
__global__ void __launch_bounds__(256) texel_finish_kernel(double* __restrict__ acc_tex, float* __restrict__ g_tex, double* __restrict__ acc_nmap,
                                                           float* __restrict__ g_nmap, const float* __restrict__ nmap_raw, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (acc_tex) {
    const double a = acc_tex[3 * (size_t)i], b = acc_tex[3 * (size_t)i + 1], c = acc_tex[3 * (size_t)i + 2];
    if (a != 0.0 || b != 0.0 || c != 0.0) {
      g_tex[3 * (size_t)i] += (float)a; g_tex[3 * (size_t)i + 1] += (float)b; g_tex[3 * (size_t)i + 2] += (float)c;
      acc_tex[3 * (size_t)i] = 0.0; acc_tex[3 * (size_t)i + 1] = 0.0; acc_tex[3 * (size_t)i + 2] = 0.0;
    }
  }
  if (acc_nmap) {
    const double a = acc_nmap[3 * (size_t)i], b = acc_nmap[3 * (size_t)i + 1], c = acc_nmap[3 * (size_t)i + 2];
    if (a != 0.0 || b != 0.0 || c != 0.0) {
      acc_nmap[3 * (size_t)i] = 0.0; acc_nmap[3 * (size_t)i + 1] = 0.0; acc_nmap[3 * (size_t)i + 2] = 0.0;
      if (nmap_raw) {
        normalize3_bwd_vals(nmap_raw, (float)a, (float)b, (float)c, g_nmap, (size_t)i);
      } else {
        g_nmap[3 * (size_t)i] += (float)a; g_nmap[3 * (size_t)i + 1] += (float)b; g_nmap[3 * (size_t)i + 2] += (float)c;
      }
    }
  }
}

__global__ void texel_counters_clear_kernel(int32_t* __restrict__ cnt, int nbins) {
  for (int b = threadIdx.x; b < nbins; b += blockDim.x) cnt[16 * b] = 0;
}

// half the compute units of the current device (hipDeviceProp_t::multiProcessorCount / 2), asked once per device
unsigned half_the_cus() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cached[dev] == 0) {
    hipDeviceProp_t prop;
    cached[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount >= 2) ? prop.multiProcessorCount / 2 : 128;
    (void)hipGetLastError();
  }
  return (unsigned)cached[dev];
}

}  // namespace

extern "C" {

int harp_texel_bins(int Ht, int Wt) { return (Ht <= 0 || Wt <= 0) ? 0 : ((Ht + kBin - 1) / kBin) * ((Wt + kBin - 1) / kBin); }

int harp_texel_reduce(const float* trec, int32_t* trec_cnt, int trec_cap, int Ht, int Wt, double* acc_tex, double* acc_nmap, int expected_records,
                      hipStream_t stream) {
  const int nbins = harp_texel_bins(Ht, Wt);
  if (!trec || !trec_cnt || trec_cap <= 0 || (trec_cap & 3) || ((size_t)trec & 15) || nbins <= 0 || nbins > kMaxBins || Wt > 65535 || Ht > 65535) return HARP_ERR_ARG;
  // Launch shape.  The kernel runs beside the depth backward and the mesh / hand backward tail, which are the step's critical path; it is bound by the
  // LDS pipe, and so are the tail's kernels (126 random LDS reads per vertex).
  //   small job (expected_records <= 2 M, or unknown: the C3 step's 1.4 M records are ~680 chunks): HALF the CUs, one 1024-thread workgroup of two
  //     tables on each, and nothing else on those CUs while it runs.  Its 112 928 B of static LDS leave 50 912 B of a CU's 160 KB: a chain_wide_bwd_b / c
  //     workgroup (74 232 B for the hand, 98 KB for the arm) does not fit, whatever the dispatcher prefers, and neither does a second reducer; its
  //     16 waves x 127 VGPRs (a 128-register allocation) take the whole register file of the four SIMDs, which keeps the kernels that need little LDS
  //     (depth backward, chain_wide_bwd_a, hand_back, lbs_*) off as well.  The reducers start first, right behind the shader backward, so the 128
  //     chain workgroups of a 32-frame step go to the other half, one per CU.  In the graph (profiles/r08_ab_record.txt): depth backward 28.6 -> 21.6 us,
  //     chain_wide_bwd_a 15.6 -> 6.4, _c 14.3 -> 11.6, the reduce 55 -> 68 ... 71 us, step -17 us.  One 512-thread table per CU on every CU (the shape
  //     before) shared each chain workgroup's LDS pipe with a reducer; 512-thread workgroups on half the CUs behind a 32-KB pad keep the chain
  //     workgroups away as well but take 86 us, and the maps' branch then ends behind the main stream.  The price: where nothing runs beside the
  //     reduce (an appearance-only stage without the mesh tail) half the chip is 7 - 13 us slower than all of it.
  //   large job (C5: 4.9 M records, ~2 600 chunks): 512 workgroups of one table, two per CU (12 KB pad: a third does not fit)
  const bool small_job = expected_records <= 2000000;
  const int nbx = (Wt + kBin - 1) / kBin;
  if (small_job)
    hipLaunchKernelGGL(texel_reduce_kernel<2>, dim3(half_the_cus()), dim3(2 * kThreads), 0, stream, trec, trec_cnt, trec_cap, nbins, nbx, Wt, Ht, acc_tex, acc_nmap);
  else
    hipLaunchKernelGGL(texel_reduce_kernel<1>, dim3(512), dim3(kThreads), 12288, stream, trec, trec_cnt, trec_cap, nbins, nbx, Wt, Ht, acc_tex, acc_nmap);
  // (a "last workgroup clears" ticket was measured first: the 512 same-address returning atomics put ~15 us under every workgroup's record loads;
  //  every reducer reads all counters, and this call has no other launch behind them that the clear could ride on)
  hipLaunchKernelGGL(texel_counters_clear_kernel, dim3(1), dim3(256), 0, stream, trec_cnt, nbins);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

int harp_texel_finish(double* acc_tex, float* g_tex, double* acc_nmap, float* g_nmap, const float* nmap_raw, int n_texels, hipStream_t stream) {
  if (n_texels <= 0 || (acc_tex && !g_tex) || (acc_nmap && !g_nmap) || (!acc_tex && !acc_nmap)) return HARP_ERR_ARG;
  hipLaunchKernelGGL(texel_finish_kernel, dim3((n_texels + 255) / 256), dim3(256), 0, stream, acc_tex, g_tex, acc_nmap, g_nmap, nmap_raw, n_texels);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}

}  // extern "C"
