// Batched fit of the MANO hand to mesh vertices for gfx950 (ops.mano_vertex_fit; hand_utils.optimize_for_mano_param(method="lm");
// playback Motion.from_vertices): 778 target vertices per frame -> the rows [rot | pose | betas | trans] that
// harp_lbs_mano_fwd turns back into those vertices.  The reference does this with 500 + 700 Adam iterations
// (metro_modifications/hand_utils.py:16-131); the model inverted is csrc/lbs.hip's, with rodrigues_fwd, rodrigues_jvp, parent_of, skin_weights
// and skin_T of lbs_body.h, so the solver and the renderer cannot disagree.
//
// harp_mano_vertex_fit: T independent Levenberg-Marquardt solves in ONE launch, one workgroup of four waves per frame.  Per frame 61
// unknowns x = [rot 3 | pose 45 | betas 10 | trans 3] and 2334 residuals (include/harp_hip.h states the contract).
//
//   set-up       the chain at x as lbs_joints_kernel does it (16 Rodrigues, rest joints at this shape, five finger chains, A_j =
//                [G_j | t_j - G_j J_j]); with the Jacobian also the chain TANGENTS, stored compactly because the Jacobian is structured:
//                a root column moves all 16 transforms (3 x 16 x 12 floats), a finger column the at most three transforms below its
//                joint (45 x 3 x 12), a shape column only the 16 translations (10 x 16 x 3, through J_dirs), trans is the identity.
//                One thread per (column, finger) walks a chain: 45 + 15 + 50 threads in three waves.
//   forward      one lane per vertex in four rounds: v_posed q (coalesced posedirs_T / shapedirs_T reads; kept in LDS for the Jacobian),
//                T_v = sum_j w_vj A_j, the residual and the cost; a fixed-order sum over the workgroup.  The candidate of an iteration is
//                evaluated by this alone.
//   Jacobian     tiles of 64 vertices, a lane per vertex and the 61 columns split over the four waves by KIND, so that no wave diverges:
//                wave 0 the root, shape and trans columns and the residual, waves 1..3 the fingers (2, 2, 1).  A finger column is
//                T_v[:3,:3] (posedirs[v, :, its joint's 9 entries] . dR) + sum over the moved joints of w_vj dA_j [q; 1].  The tile
//                (192 rows x 64 columns, column 61 = the residual, row stride 65: lane v writes rows 3v.., 195 floats apart = no bank
//                conflict) lives in LDS.
//   J^T W J      v_mfma_f32_32x32x2_f32 (exact float32): every wave takes 48 rows of the tile (its K slice) into three 32 x 32
//                accumulators - blocks (0,0), (1,0), (1,1) of the 64 x 64 product; the lower triangle is all Cholesky reads - that
//                live in registers across the 13 tiles and meet in LDS at the end, wave after wave (fixed order).  Row 61 of the
//                product is g = J^T W r.
//   solve        lm_solve_body.h on wave 0 (Jacobi scaling, the in-place Cholesky of the scaled system in LDS with lane i = row i, both
//                triangular solves in registers), accept iff C(x') < C(x).
// `iters` iterations whatever happens; every branch is uniform over the workgroup.  No workspace, no allocation, no synchronisation, no
// atomics: the launch can be captured and a repeated call gives the same bits.
#include "lbs_body.h"
#include "lm_gram_body.h"
#include "lm_solve_body.h"
#include "harp_hip.h"

#include <math.h>

namespace {

using namespace lb;

using lm::f32x16;

constexpr int NX = 61;                  // unknowns per frame
constexpr int NXP = 64;                 // ... padded to the matrix cores' 2 x 32; column 61 carries the residual
constexpr int LD = 65;                  // row stride of the tile and of the normal matrix in LDS
constexpr int TV = 64;                  // vertices per tile
constexpr int NT = (NV + TV - 1) / TV;  // 13 tiles, the last with 10 vertices
constexpr int kThreads = 256;
constexpr int kVfFramesPerBlock = 1;
constexpr int XB = 48, XT = 58;         // first shape / trans column

struct VfLds {                          // (the small tables first: their addresses then fit the 16-bit offset of an LDS instruction)
  float dAr[3][NJ][12];                 // d A_j / d rot[c]
  float dAf[45][3][12];                 // d A_{joint + s} / d pose[i], s = 0..2 down the finger (unused slots zero)
  float dAs[NB][NJ][3];                 // d (A_j's translation) / d betas[k]
  float dR[45][9];                      // d R_joint / d pose[i]: the tangent of the pose correctives
  float q[NV][3];                       // v_posed at the last evaluated point
  float x[NXP];                         // the point being evaluated
  float R[NJ][9], G[NJ][12], Aj[NJ][12], Jr[NJ][3], pm[NP];
  float wt[TV];                         // the tile's vertex weights (0 = unused)
  float prior[48];
  float red[4];
  int flag;
  union {
    float J[3 * TV][LD];                // a tile of d v (metres) / d x, column 61 = the residual
    float A[NXP][LD];                   // the normal matrix (lower triangle; row 61 = g), then its scaled Cholesky factor
  } u;
};
static_assert(sizeof(VfLds) == 75148, "two workgroups on a CU rest on this size (DESIGN.md §27)");

__device__ __forceinline__ void joint_aa(const harp_mano_model& M, const VfLds& S, int j, float aa[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p = S.x[3 * j + c];
    aa[c] = (j == 0) ? p : (M.hands_mean[3 * (j - 1) + c] + p);       // (csrc/lbs.hip:35)
  }
}

// dA (3 x 4) = [dG | dt - dG J]
__device__ __forceinline__ void store_dA(float* dA, const float dG[9], const float dt[3], const float J[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    dA[r * 4] = dG[r * 3]; dA[r * 4 + 1] = dG[r * 3 + 1]; dA[r * 4 + 2] = dG[r * 3 + 2];
    dA[r * 4 + 3] = dt[r] - (dG[r * 3] * J[0] + dG[r * 3 + 1] * J[1] + dG[r * 3 + 2] * J[2]);
  }
}

// one level down a chain: the child's (dG, dt) from the parent's, in place
__device__ __forceinline__ void tangent_down(const VfLds& S, int j, float dG[9], float dt[3]) {
  const int p = parent_of(j);
  const float rel[3] = {S.Jr[j][0] - S.Jr[p][0], S.Jr[j][1] - S.Jr[p][1], S.Jr[j][2] - S.Jr[p][2]};
  float nG[9], nt[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) nG[r * 3 + c] = dG[r * 3] * S.R[j][c] + dG[r * 3 + 1] * S.R[j][3 + c] + dG[r * 3 + 2] * S.R[j][6 + c];
    nt[r] = dG[r * 3] * rel[0] + dG[r * 3 + 1] * rel[1] + dG[r * 3 + 2] * rel[2] + dt[r];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) dG[k] = nG[k];
  dt[0] = nt[0]; dt[1] = nt[1]; dt[2] = nt[2];
}

// The chain at S.x (every thread of the workgroup calls this; S.x is visible).  JAC: also the tangents.
__device__ void vf_setup(const harp_mano_model& M, VfLds& S, int tid, bool JAC) {
  if (tid < NJ) {
    float aa[3], R[9];
    joint_aa(M, S, tid, aa);
    rodrigues_fwd(aa, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      S.R[tid][k] = R[k];
      if (tid > 0) S.pm[(tid - 1) * 9 + k] = R[k] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
    }
  } else if (tid >= 64 && tid < 64 + NJ * 3) {                         // rest joints at this shape (csrc/lbs.hip:43-48)
    const int l = tid - 64;
    float acc = M.J_template[l];
    for (int k = 0; k < NB; ++k) acc += M.J_dirs[l * NB + k] * S.x[XB + k];
    S.Jr[l / 3][l % 3] = acc;
  } else if (JAC && tid >= 128 && tid < 128 + 45) {
    const int i = tid - 128;
    float aa[3], dR[9];
    joint_aa(M, S, i / 3 + 1, aa);
    rodrigues_jvp(aa, i % 3, dR);
#pragma unroll
    for (int k = 0; k < 9; ++k) S.dR[i][k] = dR[k];
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 0; k < 9; ++k) S.G[0][(k / 3) * 4 + (k % 3)] = S.R[0][k];
    for (int r = 0; r < 3; ++r) S.G[0][r * 4 + 3] = S.Jr[0][r];
  }
  __syncthreads();
  if (tid < 5) {                                                       // one finger per lane, as lbs_joints_kernel
    for (int lev = 0; lev < 3; ++lev) {
      const int j = 3 * tid + 1 + lev, p = parent_of(j);
      const float rel[3] = {S.Jr[j][0] - S.Jr[p][0], S.Jr[j][1] - S.Jr[p][1], S.Jr[j][2] - S.Jr[p][2]};
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
          S.G[j][r * 4 + c] = S.G[p][r * 4] * S.R[j][c] + S.G[p][r * 4 + 1] * S.R[j][3 + c] + S.G[p][r * 4 + 2] * S.R[j][6 + c];
        S.G[j][r * 4 + 3] = S.G[p][r * 4] * rel[0] + S.G[p][r * 4 + 1] * rel[1] + S.G[p][r * 4 + 2] * rel[2] + S.G[p][r * 4 + 3];
      }
    }
  }
  __syncthreads();
  if (tid < NJ * 12) {                                                 // A_j = [G_j | t_j - G_j J_j]
    const int j = tid / 12, e = tid % 12, r = e / 4, c = e % 4;
    S.Aj[j][e] = (c < 3) ? S.G[j][e]
                         : S.G[j][r * 4 + 3] - (S.G[j][r * 4] * S.Jr[j][0] + S.G[j][r * 4 + 1] * S.Jr[j][1] + S.G[j][r * 4 + 2] * S.Jr[j][2]);
  }
  if (JAC) {
    if (tid < 45) {                                                    // a finger column: G_q = G_p R_q, so d G_q = G_p dR and the position stays
      const int jq = tid / 3 + 1, lev = (jq - 1) % 3, p = parent_of(jq);
      float dG[9], dt[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          dG[r * 3 + c] = S.G[p][r * 4] * S.dR[tid][c] + S.G[p][r * 4 + 1] * S.dR[tid][3 + c] + S.G[p][r * 4 + 2] * S.dR[tid][6 + c];
      store_dA(S.dAf[tid][0], dG, dt, S.Jr[jq]);
      for (int s = 1; s < 3; ++s) {
        if (lev + s < 3) {
          tangent_down(S, jq + s, dG, dt);
          store_dA(S.dAf[tid][s], dG, dt, S.Jr[jq + s]);
        } else {
          for (int k = 0; k < 12; ++k) S.dAf[tid][s][k] = 0.f;
        }
      }
    } else if (tid >= 64 && tid < 64 + 15) {                           // a root column down one finger: d G_0 = dR, the root joint stays
      const int i = tid - 64, c = i / 5, f = i % 5;
      float aa[3], dG[9], dt[3] = {0.f, 0.f, 0.f};
      joint_aa(M, S, 0, aa);
      rodrigues_jvp(aa, c, dG);
      if (f == 0) store_dA(S.dAr[c][0], dG, dt, S.Jr[0]);
      for (int lev = 0; lev < 3; ++lev) {
        const int j = 3 * f + 1 + lev;
        tangent_down(S, j, dG, dt);
        store_dA(S.dAr[c][j], dG, dt, S.Jr[j]);
      }
    } else if (tid >= 128 && tid < 128 + 50) {                         // a shape column down one finger: only positions move, through J_dirs
      const int i = tid - 128, k = i / 5, f = i % 5;
      float dJp[3], dt[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) { dJp[r] = M.J_dirs[r * NB + k]; dt[r] = dJp[r]; }
      if (f == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) S.dAs[k][0][r] = dt[r] - (S.G[0][r * 4] * dJp[0] + S.G[0][r * 4 + 1] * dJp[1] + S.G[0][r * 4 + 2] * dJp[2]);
      }
      for (int lev = 0; lev < 3; ++lev) {
        const int j = 3 * f + 1 + lev, p = parent_of(j);
        float dJ[3], nt[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) dJ[r] = M.J_dirs[(3 * j + r) * NB + k];
        const float dr[3] = {dJ[0] - dJp[0], dJ[1] - dJp[1], dJ[2] - dJp[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          nt[r] = S.G[p][r * 4] * dr[0] + S.G[p][r * 4 + 1] * dr[1] + S.G[p][r * 4 + 2] * dr[2] + dt[r];
          S.dAs[k][j][r] = nt[r] - (S.G[j][r * 4] * dJ[0] + S.G[j][r * 4 + 1] * dJ[1] + S.G[j][r * 4 + 2] * dJ[2]);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) { dJp[r] = dJ[r]; dt[r] = nt[r]; }
      }
    }
  }
  __syncthreads();
}

// what a vertex contributes: its weight (0 = unused) and, when used, its target
__device__ __forceinline__ float vertex_target(const float* __restrict__ tg, const float* __restrict__ wts, int v, float t[3]) {
  const float w = wts ? wts[v] : 1.0f;
  t[0] = tg[3 * v]; t[1] = tg[3 * v + 1]; t[2] = tg[3 * v + 2];
  const bool used = (w > 0.f) && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
  return used ? w : 0.f;
}

// skinned position (metres, trans included) of posed vertex q
__device__ __forceinline__ void skin_pos(const VfLds& S, const float Tm[12], const float q[3], float pos[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) pos[r] = Tm[r * 4] * q[0] + Tm[r * 4 + 1] * q[1] + Tm[r * 4 + 2] * q[2] + Tm[r * 4 + 3] + S.x[XT + r];
}

// All vertices at S.x after vf_setup: S.q, optionally verts (mm), and C(x) (the same bits in every thread)
__device__ float vf_forward(const harp_mano_model& M, VfLds& S, int tid, const float* __restrict__ tg, const float* __restrict__ wts,
                            float pose_w, float shape_w, float* __restrict__ verts) {
  float part = 0.f;
#pragma unroll 1
  for (int v = tid; v < NV; v += kThreads) {
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = M.v_template[3 * v + c];
    for (int k = 0; k < NB; ++k) {
      const float b = S.x[XB + k];
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c] += M.shapedirs_T[(size_t)k * NV * 3 + 3 * v + c] * b;
    }
    // (the kernel is a chain of L2 round trips, not arithmetic: 45 rows = 135 loads are in flight per trip, three trips per vertex)
#pragma unroll 1
    for (int k0 = 0; k0 < NP; k0 += 45) {
      const float* pT = M.posedirs_T;
      float pd[45][3];
#pragma unroll
      for (int k = 0; k < 45; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) pd[k][c] = pT[(size_t)(k0 + k) * NV * 3 + 3 * v + c];
#pragma unroll
      for (int k = 0; k < 45; ++k) {
        const float p = S.pm[k0 + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] += pd[k][c] * p;
      }
    }
    S.q[v][0] = q[0]; S.q[v][1] = q[1]; S.q[v][2] = q[2];
    float4 w4s[4];
    float Tm[12], pos[3], t[3];
    skin_weights(M, v, w4s);
    skin_T(w4s, &S.Aj[0][0], Tm);
    skin_pos(S, Tm, q, pos);
    const float w = vertex_target(tg, wts, v, t);
    if (w > 0.f) {
      const float d0 = pos[0] - t[0], d1 = pos[1] - t[1], d2 = pos[2] - t[2];
      part += w * (d0 * d0 + d1 * d1 + d2 * d2);
    }
    if (verts) { verts[3 * v] = pos[0] * 1000.0f; verts[3 * v + 1] = pos[1] * 1000.0f; verts[3 * v + 2] = pos[2] * 1000.0f; }
  }
  if (tid >= 3 && tid < 48) {
    const float d = S.x[tid] - S.prior[tid - 3];
    part += pose_w * d * d;
  } else if (tid >= XB && tid < XT) {
    part += shape_w * S.x[tid] * S.x[tid];
  }
  part = wave_sum(part);
  if ((tid & 63) == 0) S.red[tid >> 6] = part;
  __syncthreads();
  // (uniform, and told so: the costs, lambda and the verdict then live in scalar registers)
  const float total = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(((S.red[0] + S.red[1]) + S.red[2]) + S.red[3])));
  __syncthreads();
  return total;
}

// A (lower triangle) = J^T W J and g = J^T W r at S.x after vf_setup (with the tangents) and vf_forward; optionally the Jacobian (2334,61) itself
__device__ void vf_normal(const harp_mano_model& M, VfLds& S, int tid, const float* __restrict__ tg, const float* __restrict__ wts,
                          float* __restrict__ jac) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;          // (wave-uniform for the compiler, unlike the caller's tid)
  f32x16 acc00, acc10, acc11;
#pragma unroll
  for (int k = 0; k < 16; ++k) { acc00[k] = 0.f; acc10[k] = 0.f; acc11[k] = 0.f; }
#pragma unroll 1
  for (int tile = 0; tile < NT; ++tile) {
    const int v = tile * TV + lane;
    const int vc = min(v, NV - 1);                                     // (a lane past the last vertex computes vertex 777 again with weight 0)
    float* row = &S.u.J[3 * lane][0];
    const float q[3] = {S.q[vc][0], S.q[vc][1], S.q[vc][2]};
    float4 w4s[4];
    float Tm[12];
    skin_weights(M, vc, w4s);
    skin_T(w4s, &S.Aj[0][0], Tm);
    if (wave == 0) {
      const float* sT = M.shapedirs_T;
      float pos[3], t[3], sd[NB][3];                                   // (the ten shape rows: one round trip, ahead of the root columns)
#pragma unroll
      for (int k = 0; k < NB; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) sd[k][c] = sT[(size_t)k * NV * 3 + 3 * vc + c];
      skin_pos(S, Tm, q, pos);
      const float w = (v < NV) ? vertex_target(tg, wts, vc, t) : 0.f;
      S.wt[lane] = w;
      const float wj[NJ] = {w4s[0].x, w4s[0].y, w4s[0].z, w4s[0].w, w4s[1].x, w4s[1].y, w4s[1].z, w4s[1].w,
                            w4s[2].x, w4s[2].y, w4s[2].z, w4s[2].w, w4s[3].x, w4s[3].y, w4s[3].z, w4s[3].w};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        row[r * LD + 61] = (w > 0.f) ? pos[r] - t[r] : 0.f;
        row[r * LD + 62] = 0.f; row[r * LD + 63] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) row[r * LD + XT + c] = (r == c) ? 1.f : 0.f;
      }
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {                                    // the root: every transform moves
        float d[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const float* dA = S.dAr[c][j];
#pragma unroll
          for (int r = 0; r < 3; ++r) d[r] += wj[j] * (dA[r * 4] * q[0] + dA[r * 4 + 1] * q[1] + dA[r * 4 + 2] * q[2] + dA[r * 4 + 3]);
        }
        row[c] = d[0]; row[LD + c] = d[1]; row[2 * LD + c] = d[2];
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {                                   // the shape: the vertex's own blend shape and the 16 translations
        const float* ds = sd[k];
        float d[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = Tm[r * 4] * ds[0] + Tm[r * 4 + 1] * ds[1] + Tm[r * 4 + 2] * ds[2];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
          for (int r = 0; r < 3; ++r) d[r] += wj[j] * S.dAs[k][j][r];
        }
        row[XB + k] = d[0]; row[LD + XB + k] = d[1]; row[2 * LD + XB + k] = d[2];
      }
    } else {
      const int f0 = 2 * (wave - 1), f1 = min(f0 + 2, 5);              // fingers 0 1 | 2 3 | 4
#pragma unroll 1
      for (int f = f0; f < f1; ++f) {
        const float* pT = M.posedirs_T;
        float pd3[27][3], w3[3];                                       // (the finger's 81 corrective entries and three weights: one round trip)
#pragma unroll
        for (int m = 0; m < 27; ++m)
#pragma unroll
          for (int c = 0; c < 3; ++c) pd3[m][c] = pT[(size_t)(f * 27 + m) * NV * 3 + 3 * vc + c];
#pragma unroll
        for (int s = 0; s < 3; ++s) w3[s] = M.weights[(size_t)vc * NJ + 3 * f + 1 + s];
#pragma unroll
        for (int lev = 0; lev < 3; ++lev) {
          const int jq = 3 * f + 1 + lev;
          const float (*pd)[3] = &pd3[9 * lev];
          const float* wj = &w3[lev];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int i = (jq - 1) * 3 + c;
            float dv[3] = {0.f, 0.f, 0.f}, d[3];
#pragma unroll
            for (int m = 0; m < 9; ++m) {
              const float dr = S.dR[i][m];
              dv[0] += pd[m][0] * dr; dv[1] += pd[m][1] * dr; dv[2] += pd[m][2] * dr;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) d[r] = Tm[r * 4] * dv[0] + Tm[r * 4 + 1] * dv[1] + Tm[r * 4 + 2] * dv[2];
#pragma unroll
            for (int s = 0; s < 3 - lev; ++s) {
              const float* dA = S.dAf[i][s];
#pragma unroll
              for (int r = 0; r < 3; ++r) d[r] += wj[s] * (dA[r * 4] * q[0] + dA[r * 4 + 1] * q[1] + dA[r * 4 + 2] * q[2] + dA[r * 4 + 3]);
            }
            row[3 + i] = d[0]; row[LD + 3 + i] = d[1]; row[2 * LD + 3 + i] = d[2];
          }
        }
      }
    }
    __syncthreads();
    if (jac) {
      const int n = min(TV, NV - tile * TV) * 3 * NX;                  // rows of real vertices only
      float* jo = jac + (size_t)tile * TV * 3 * NX;
      for (int i = tid; i < n; i += kThreads) jo[i] = S.u.J[i / NX][i % NX];
    }
    lm::gram_accumulate(S.u.J, S.wt, wave, lane, acc00, acc10, acc11);
    __syncthreads();
  }
  for (int w = 0; w < 4; ++w) {                                        // the four K slices meet, wave after wave
    if (wave == w) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int r = (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5), c = lane & 31;
        if (w == 0) { S.u.A[r][c] = acc00[k]; S.u.A[32 + r][c] = acc10[k]; S.u.A[32 + r][32 + c] = acc11[k]; }
        else { S.u.A[r][c] += acc00[k]; S.u.A[32 + r][c] += acc10[k]; S.u.A[32 + r][32 + c] += acc11[k]; }
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kThreads, 2) mano_vertex_fit_kernel(const harp_mano_model M, const float* __restrict__ targets,
                                                                   const float* __restrict__ weights, const float* __restrict__ prior, int iters,
                                                                   float lambda, float pose_w, float shape_w, int solve_shape,
                                                                   int betas_per_frame, float* __restrict__ pose48, float* __restrict__ betas,
                                                                   float* __restrict__ trans, float* __restrict__ cost,
                                                                   int32_t* __restrict__ status, float* __restrict__ verts,
                                                                   float* __restrict__ jac, float* __restrict__ Aout, float* __restrict__ gout) {
  extern __shared__ float s_raw[];
  int lds0 = 0;                                                        // (see below)
  asm volatile("" : "+v"(lds0));
  VfLds& S0 = *reinterpret_cast<VfLds*>(s_raw + lds0);
  const int t = blockIdx.x, wave = threadIdx.x >> 6;                   // (the grid is exactly T workgroups)
  int tid = threadIdx.x;
  const float* tg = targets + (size_t)t * NV * 3;
  const float* wts = weights ? weights + (size_t)t * NV : nullptr;
  const size_t brow = (solve_shape || betas_per_frame) ? (size_t)t * NB : 0;
  float xl = 0.f;                                                      // wave 0, lane l: unknown l
  if (tid < 48) xl = pose48[(size_t)t * 48 + tid];
  else if (tid < XT) xl = betas[brow + (tid - XB)];
  else if (tid < NX) xl = trans[(size_t)t * 3 + (tid - XT)];
  if (tid < NXP) S0.x[tid] = xl;
  if (tid < 48) S0.prior[tid] = (prior && tid < 45) ? prior[(size_t)t * 45 + tid] : 0.f;
  int n_used = 0;
  for (int r = 0; r < (NV + kThreads - 1) / kThreads; ++r) {
    const int v = tid + r * kThreads;
    float tt[3];
    n_used += __syncthreads_count(v < NV && vertex_target(tg, wts, min(v, NV - 1), tt) > 0.f);
  }
  const bool solve = n_used >= 21;                                     // 3 * 21 >= 61
  const bool frozen = (tid >= XB && tid < XT && !solve_shape);         // (of wave 0's lanes)

  // Evaluations alternate: an even one is at x with the tangents, the normal equations and the solve for the candidate x', an odd one is
  // the candidate's cost and the verdict.  One more even one at the end serves the optional outputs (and the cost when iters == 0).
  float C = 0.f, C0 = 0.f, xn = 0.f;
  int n_acc = 0;
  bool ok = false;
  const bool outputs = verts || jac || Aout || gout;
  const int n_eval = 2 * iters + ((outputs || iters == 0) ? 1 : 0);
#pragma unroll 1
  for (int e = 0; e < n_eval; ++e) {
    asm volatile("" : "+v"(tid));                                      // (nothing per lane is carried across evaluations in registers)
    // ... and the LDS base is taken afresh: every table is then base + a 16-bit instruction offset; with a constant base the compiler
    // builds each address as a constant of its own, hoists some 400 of them out of this loop and spills them
    asm volatile("" : "+v"(lds0));
    VfLds& S = *reinterpret_cast<VfLds*>(s_raw + lds0);
    const bool at_x = !(e & 1), last = e == 2 * iters;
    if (at_x && tid < NXP) S.x[tid] = xl;
    __syncthreads();
    vf_setup(M, S, tid, at_x);
    const float Ce = vf_forward(M, S, tid, tg, wts, pose_w, shape_w, (last && verts) ? verts + (size_t)t * NV * 3 : nullptr);
    if (!at_x) {
      const bool accept = ok && solve && (Ce < C);                     // (a NaN is not less; uniform over the workgroup)
      if (accept) {
        xl = xn;
        C = Ce;
        ++n_acc;
      }
      lambda = lm::damped(lambda, accept);
      continue;
    }
    if (e == 0) C0 = C = Ce;
    vf_normal(M, S, tid, tg, wts, (last && jac) ? jac + (size_t)t * NV * 3 * NX : nullptr);
    // priors, frozen columns, g
    float g = 0.f, diag = 1.f;
    if (tid < NX) {
      g = S.u.A[61][tid];
      diag = S.u.A[tid][tid];
      if (tid >= 3 && tid < 48) { g += pose_w * (xl - S.prior[tid - 3]); diag += pose_w; }
      else if (tid >= XB && tid < XT) { g += shape_w * xl; diag += shape_w; }
      if (frozen) { g = 0.f; diag = 1.f; }
    }
    __syncthreads();
    if (tid < NX) S.u.A[tid][tid] = diag;
    if (!solve_shape)
      for (int i = tid; i < NX * NB; i += kThreads) {
        const int r = i / NB, c = XB + i % NB;
        if (r != c) S.u.A[max(r, c)][min(r, c)] = 0.f;
      }
    __syncthreads();
    if (last) {
      if (Aout)
        for (int i = tid; i < NX * NX; i += kThreads) Aout[(size_t)t * NX * NX + i] = S.u.A[max(i / NX, i % NX)][min(i / NX, i % NX)];
      if (gout && tid < NX) gout[(size_t)t * NX + tid] = g;
      break;
    }
    bool okw;                                                          // (wave 0's verdict counts)
    const float s = lm::jacobi_scale<NX>(tid, diag, lambda, okw);
    const float z = lm::solve<NX, LD, 1, 8>(S.u.A, tid, s, -g * s, wave == 0, okw);
    if (wave == 0) {
      xn = (tid < NX) ? xl + z * s : 0.f;
      S.x[tid] = xn;
      if (tid == 0) S.flag = okw ? 1 : 0;
    }
    __syncthreads();
    ok = __builtin_amdgcn_readfirstlane(S.flag) != 0;
  }

  if (solve && iters > 0) {
    if (tid < 48) pose48[(size_t)t * 48 + tid] = xl;
    else if (tid < XT) { if (solve_shape) betas[brow + (tid - XB)] = xl; }
    else if (tid < NX) trans[(size_t)t * 3 + (tid - XT)] = xl;
  }
  if (tid == 0) {
    cost[2 * (size_t)t] = C0;
    cost[2 * (size_t)t + 1] = C;
    status[t] = solve ? n_acc : -1;
  }
}

}  // namespace

extern "C" int harp_mano_vertex_fit_frames_per_block(void) { return kVfFramesPerBlock; }

extern "C" int harp_mano_vertex_fit(const harp_mano_model* m, const float* targets, const float* weights, const float* prior, int T,
                                    const harp_vertex_fit_options* opt, float* pose48, float* betas, float* trans, float* cost, int32_t* status,
                                    float* verts, float* jac, float* A, float* g, hipStream_t stream) {
  if (!m || !opt || !targets || !pose48 || !betas || !trans || !cost || !status || T <= 0 || opt->iters < 0) return HARP_ERR_ARG;
  if (!(opt->lambda0 >= 0.f) || !(opt->pose_prior_weight >= 0.f) || !(opt->shape_prior_weight >= 0.f) || isinf(opt->lambda0) ||
      isinf(opt->pose_prior_weight) || isinf(opt->shape_prior_weight))
    return HARP_ERR_ARG;
  // dynamic LDS above 64 KB has to be requested; per-device attribute, set on every call
  if (hipFuncSetAttribute((const void*)mano_vertex_fit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(VfLds)) != hipSuccess)
    return HARP_ERR_ARG;
  hipLaunchKernelGGL(mano_vertex_fit_kernel, dim3((unsigned)T), dim3(kThreads), sizeof(VfLds), stream, *m, targets, weights, prior, opt->iters,
                     opt->lambda0, opt->pose_prior_weight, opt->shape_prior_weight, opt->solve_shape != 0, opt->betas_per_frame != 0, pose48, betas,
                     trans, cost, status, verts, jac, A, g);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
