// Batched fit of the SMPL-X right arm to mesh vertices for gfx950 (ops.arm_vertex_fit; hand_utils.optimize_for_mano_arm_param(method="lm");
// playback Motion.from_arm_vertices): n_t target vertices per frame (all 1026 of the arm, or the 778 of the hand through
// right_mano_idx) -> the rows [rot | wrist | pose | betas | trans] that harp_lbs_tree_fwd turns back into those vertices.  The reference does
// this with 500 + 700 Adam iterations (metro_modifications/hand_utils.py:134-240).  The sibling of csrc/vertex_fit.hip (MANO):
// the iteration and the tile are that file's, the solve is lm_solve_body.h's, the tree's slot tables are tree_slots_body.h's (shared with
// csrc/arm_ik.hip); the forward is csrc/lbs_tree.hip's (lt::rod_fwd, lt::rod_jvp, the level-parallel chain), so the solver and the renderer
// cannot disagree.
//
// harp_arm_vertex_fit: T independent Levenberg-Marquardt solves in ONE launch, one workgroup of four waves per frame, 64 unknowns
// x = [rot 3 | wrist 3 | pose 45 | betas 10 | trans 3] (include/harp_hip.h states the contract).
//
//   prologue     once per workgroup, what no unknown moves: the tree and its slot tables (tree_slots_body.h: 16 slots for the wrist,
//                3 + 2 + 1 per finger = 46 in all), the ten
//                solved columns of J_dirs, the rotations of the joints nothing drives, and q0 = v_template + their pose correctives:
//                constant rows (the real model's left hand: pose_src < 0 with a non-zero pose_mean) that are NOT zero, summed here once
//                instead of in each of the 2 iters + 1 evaluations; a row whose R - I is exactly zero (rod_fwd(0) = I exactly) is skipped.
//   set-up       the chain at x: 17 Rodrigues, the rest joints at this shape, 11 levels, A_j = [G_j | t_j - G_j J_j], the posed centre
//                joint.  With the Jacobian also the TANGENTS, stored by structure: a wrist or finger column (row, axis) walks its slots
//                ([dG | dt] of every joint below, parents before children); a shape column moves only translations (dt_j through J_dirs,
//                level by level beside the chain itself); the root column needs no table at all (below).
//   forward      one lane per TARGET vertex i (model vertex vert_idx[i]): q = q0 + 10 shape rows + the 16 x 9 corrective rows that move,
//                T_v = sum_j w_vj A_j, v = T_v [q; 1] - centre + trans, the cost; a fixed-order sum.  A candidate is evaluated by this alone.
//   Jacobian     tiles of 64 target vertices, a lane per vertex, the 64 columns split over the four waves by KIND (no divergence):
//                wave 0 root, shape, trans and the residual; waves 1..3 the wrist and the five fingers.
//                  root    rotation about the pelvis followed by the subtraction of the posed wrist is a rotation of the wrist-relative
//                          mesh: dv = (dR_0 R_0^T) (v - trans) — no 55-joint sum (the skin weights of a vertex sum to one)
//                  wrist,  T_v[:3,:3] (posedirs[v, the joint's 9 rows] . dR) + sum over its slots of w_vj (dG_j (q - J_j) + dt_j)
//                  finger  - d(posed centre), which is zero when the centre is the wrist itself or above it
//                  shape   T_v[:3,:3] shapedirs[v, k] + sum_j w_vj (dt_j - G_j dJ_j) - d(posed centre)
//                The tile (192 rows x 64 columns, row stride 65: lane v writes rows 3v.., 195 floats apart = no bank conflict) is in LDS.
//   J^T W J      v_mfma_f32_32x32x2_f32 (exact float32) as csrc/vertex_fit.hip: every wave takes 48 rows of the tile into three 32 x 32
//                accumulators (blocks (0,0), (1,0), (1,1)), live across the tiles, meeting in LDS wave after wave.
//   g = J^T W r  64 unknowns leave the tile no column for the residual: thread (column c, wave p) adds J[k][c] w_k r_k over the wave's 48
//                rows of every tile in a register, and the four partial sums meet in fixed order.
//   solve        lm_solve_body.h with all 64 lanes of wave 0.
// `iters` iterations whatever happens; every branch is uniform over the workgroup.  No workspace, no allocation, no synchronisation, no
// atomics: the launch can be captured and a repeated call gives the same bits.
#include "lm_gram_body.h"
#include "lm_solve_body.h"
#include "tree_slots_body.h"

#include <math.h>

namespace {

using namespace lt;

using lm::f32x16;

constexpr int NX = 64;                  // unknowns per frame = the matrix cores' 2 x 32
constexpr int LD = 65;                  // row stride of the tile and of the normal matrix in LDS
constexpr int TV = 64;                  // target vertices per tile
constexpr int kThreads = 256;
constexpr int kAfFramesPerBlock = 1;
constexpr int XW = 3, XP = 6, XB = 51, XT = 61;       // first wrist / finger / shape / trans column
constexpr int NSB = 10;                 // shape coefficients solved (the model's other NB - 10 are zero)
constexpr int MAXV = HARP_ARM_VERTEX_FIT_MAX_VERTS;
constexpr int MIN_USED = 22;            // 3 x 22 >= 64

struct AfLds : TreeTables {            // (the small tables first; the tree and its slot tables: the prologue's, tree_slots_body.h)
  int flag;
  // the point and its chain (every evaluation)
  float x[NX];
  float prior[NX];                      // by column (zero outside the finger columns)
  float pmv[NIN][9];                    // R - I of a driven joint: the corrective rows that move
  float cen[3], red[4];
  float R[MAXJ][9], G[MAXJ][12], Aj[MAXJ][12], Jr[MAXJ][3];
  // the tangents (evaluations at x)
  float Om[3][9];                       // dR_0/d rot[c] R_0^T
  float dR[NIN * 3][9];
  float dcen[NX][3];                    // d (posed centre) / d x[col], wrist, finger and shape columns
  float dGt[MAXSLOT][3][12];            // [dG_j | dt_j] of a slot's joint by the column's three axes
  float dJ[NSB][MAXJ][3];               // J_dirs, the solved columns (prologue)
  float dAs[NSB][MAXJ][3];              // d t_j / d betas[k], then dt_j - G_j dJ_j
  float res[3 * TV], wt[TV];            // the tile's residual rows and vertex weights (0 = unused)
  float gp[4][NX];
  float sW[TV][MAXJ + 1];               // the tile's skin weights (odd stride: conflict-free rows)
  float q0[MAXV][3];                    // v_template + the constant correctives, by MODEL vertex
  float q[MAXV][3];                     // v_posed at the last evaluated point, by TARGET vertex
  union {
    float J[3 * TV][LD];                // a tile of d v (metres) / d x
    float A[NX][LD];                    // the normal matrix (lower triangle), then its scaled Cholesky factor
  } u;
};
static_assert(sizeof(AfLds) == 132272, "the dynamic LDS of a workgroup (DESIGN.md §28)");

__device__ __forceinline__ void joint_aa(const harp_tree_model& M, const AfLds& S, int row, float aa[3]) {
  const int j = S.drv[row];
#pragma unroll
  for (int c = 0; c < 3; ++c) aa[c] = M.pose_mean[3 * j + c] + S.x[3 * row + c];            // (lbs_tree_body.h, joints_body)
}

__device__ __forceinline__ int target_vertex(const harp_tree_model& M, const int32_t* __restrict__ idx, int i) {
  return idx ? min(max(idx[i], 0), M.NV - 1) : i;
}

// Once per workgroup.  Sets S.bad when the model is not of the shape this kernel's tables hold.
__device__ void af_prologue(const harp_tree_model& M, AfLds& S, int tid) {
  const int NJ = M.NJ, NB = M.NB, NV = M.NV;
  for (int i = tid; i < NSB * NJ * 3; i += kThreads) {
    const int k = i / (NJ * 3), l = i % (NJ * 3);
    S.dJ[k][l / 3][l % 3] = M.J_dirs[(size_t)l * NB + k];
  }
  tree_tables<kThreads>(M, S, tid);
  if (S.bad) return;
  undriven_rotation(M, S, tid - 64, S.R);
  __syncthreads();
  for (int v = tid; v < NV; v += kThreads) {                           // q0: the template and the constant corrective rows
    float q[3] = {M.v_template[3 * v], M.v_template[3 * v + 1], M.v_template[3 * v + 2]};
    for (int j = 1; j < NJ; ++j) {
      if (S.driven[j]) continue;
#pragma unroll 1
      for (int k = 0; k < 9; ++k) {
        const float p = S.R[j][k] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
        if (p == 0.f) continue;                                        // (uniform: the same LDS word in every lane)
        const float* pd = M.posedirs_T + (size_t)((j - 1) * 9 + k) * NV * 3 + 3 * v;
        q[0] += pd[0] * p; q[1] += pd[1] * p; q[2] += pd[2] * p;
      }
    }
    S.q0[v][0] = q[0]; S.q0[v][1] = q[1]; S.q0[v][2] = q[2];
  }
  __syncthreads();
}

// The chain at S.x (every thread of the workgroup calls this; S.x is visible).  JAC: also the tangents.
__device__ void af_setup(const harp_tree_model& M, AfLds& S, int tid, bool JAC) {
  const int NJ = M.NJ, cj = M.center_joint;
  if (tid < NIN) {
    const int j = S.drv[tid];
    float aa[3], R[9];
    joint_aa(M, S, tid, aa);
    rod_fwd(aa, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      S.R[j][k] = R[k];
      S.pmv[tid][k] = R[k] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
    }
  } else if (tid >= 64 && tid < 64 + NJ * 3) {                         // rest joints at this shape (lbs_tree_body.h, joints_body)
    const int l = tid - 64, j = l / 3, r = l % 3;
    float acc = M.J_template[l];
#pragma unroll
    for (int k = 0; k < NSB; ++k) acc += S.dJ[k][j][r] * S.x[XB + k];
    S.Jr[j][r] = acc;
  }
  if (JAC && tid >= 128 && tid < 128 + NIN * 3) {
    const int i = tid - 128;
    float aa[3], dR[9];
    joint_aa(M, S, i / 3, aa);
    rod_jvp(aa, i % 3, dR);
#pragma unroll
    for (int k = 0; k < 9; ++k) S.dR[i][k] = dR[k];
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 0; k < 9; ++k) S.G[0][(k / 3) * 4 + (k % 3)] = S.R[0][k];
    for (int r = 0; r < 3; ++r) S.G[0][r * 4 + 3] = S.Jr[0][r];
  } else if (JAC && tid >= 64 && tid < 64 + NSB) {
    for (int r = 0; r < 3; ++r) S.dAs[tid - 64][0][r] = S.dJ[tid - 64][0][r];
  }
  // batch_rigid_transform level by level (lbs_tree_body.h, joints_body); beside it the shape tangents of the posed joint positions
  const int maxd = S.maxd;
  for (int d = 1; d <= maxd; ++d) {
    __syncthreads();
    if (tid < NJ) {
      const int j = tid;
      if (S.depth[j] == d) {
        const int p = S.par[j];
        const float rel[3] = {S.Jr[j][0] - S.Jr[p][0], S.Jr[j][1] - S.Jr[p][1], S.Jr[j][2] - S.Jr[p][2]};
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c)
            S.G[j][r * 4 + c] = S.G[p][r * 4] * S.R[j][c] + S.G[p][r * 4 + 1] * S.R[j][3 + c] + S.G[p][r * 4 + 2] * S.R[j][6 + c];
          S.G[j][r * 4 + 3] = S.G[p][r * 4] * rel[0] + S.G[p][r * 4 + 1] * rel[1] + S.G[p][r * 4 + 2] * rel[2] + S.G[p][r * 4 + 3];
        }
      }
    } else if (JAC && tid >= 64) {
      for (int i = tid - 64; i < NSB * NJ; i += kThreads - 64) {
        const int k = i / NJ, j = i % NJ;
        if (S.depth[j] != d) continue;
        const int p = S.par[j];
        const float dr[3] = {S.dJ[k][j][0] - S.dJ[k][p][0], S.dJ[k][j][1] - S.dJ[k][p][1], S.dJ[k][j][2] - S.dJ[k][p][2]};
        for (int r = 0; r < 3; ++r)
          S.dAs[k][j][r] = S.G[p][r * 4] * dr[0] + S.G[p][r * 4 + 1] * dr[1] + S.G[p][r * 4 + 2] * dr[2] + S.dAs[k][p][r];
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < NJ * 12; i += kThreads) {                      // A_j = [G_j | t_j - G_j J_j]
    const int j = i / 12, e = i % 12, r = e / 4, c = e % 4;
    S.Aj[j][e] = (c < 3) ? S.G[j][e]
                         : S.G[j][r * 4 + 3] - (S.G[j][r * 4] * S.Jr[j][0] + S.G[j][r * 4 + 1] * S.Jr[j][1] + S.G[j][r * 4 + 2] * S.Jr[j][2]);
  }
  if (tid < 3) S.cen[tid] = S.G[cj][tid * 4 + 3];
  if (JAC) {
    if (tid >= 64 && tid < 67) {                                       // the root: Omega_c = dR_0 R_0^T
      const int c = tid - 64;
      for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k)
          S.Om[c][r * 3 + k] = S.dR[c][r * 3] * S.R[0][k * 3] + S.dR[c][r * 3 + 1] * S.R[0][k * 3 + 1] + S.dR[c][r * 3 + 2] * S.R[0][k * 3 + 2];
    } else if (tid >= 128 && tid < 128 + (NIN - 1) * 3) {              // a wrist or finger column down its slots
      const int i = 3 + (tid - 128), row = i / 3, c = i % 3;
      float dc[3] = {0.f, 0.f, 0.f};
      for (int s = S.soff[row]; s < S.soff[row + 1]; ++s) {
        const int j = S.sj[s], ps = S.sp[s], p = S.par[j];
        float* o = S.dGt[s][c];
        if (ps < 0) {                                                  // G_q = G_p [R_q | .]: d G_q = G_p dR, the joint's position stays
          for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k)
              o[r * 4 + k] = S.G[p][r * 4] * S.dR[i][k] + S.G[p][r * 4 + 1] * S.dR[i][3 + k] + S.G[p][r * 4 + 2] * S.dR[i][6 + k];
            o[r * 4 + 3] = 0.f;
          }
        } else {
          const float* pg = S.dGt[ps][c];
          const float rel[3] = {S.Jr[j][0] - S.Jr[p][0], S.Jr[j][1] - S.Jr[p][1], S.Jr[j][2] - S.Jr[p][2]};
          for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) o[r * 4 + k] = pg[r * 4] * S.R[j][k] + pg[r * 4 + 1] * S.R[j][3 + k] + pg[r * 4 + 2] * S.R[j][6 + k];
            o[r * 4 + 3] = pg[r * 4] * rel[0] + pg[r * 4 + 1] * rel[1] + pg[r * 4 + 2] * rel[2] + pg[r * 4 + 3];
          }
        }
        if (j == cj) { dc[0] = o[3]; dc[1] = o[7]; dc[2] = o[11]; }
      }
      S.dcen[i][0] = dc[0]; S.dcen[i][1] = dc[1]; S.dcen[i][2] = dc[2];
    } else if (tid >= 192 && tid < 192 + NSB) {
      for (int r = 0; r < 3; ++r) S.dcen[XB + tid - 192][r] = S.dAs[tid - 192][cj][r];
    }
    __syncthreads();
    for (int i = tid; i < NSB * NJ; i += kThreads) {                   // a shape column: d (A_j's translation) = dt_j - G_j dJ_j
      const int k = i / NJ, j = i % NJ;
      for (int r = 0; r < 3; ++r)
        S.dAs[k][j][r] -= S.G[j][r * 4] * S.dJ[k][j][0] + S.G[j][r * 4 + 1] * S.dJ[k][j][1] + S.G[j][r * 4 + 2] * S.dJ[k][j][2];
    }
  }
  __syncthreads();
}

// what a target contributes: its weight (0 = unused) and, when used, its position
__device__ __forceinline__ float vertex_target(const float* __restrict__ tg, const float* __restrict__ wts, int i, float t[3]) {
  const float w = wts ? wts[i] : 1.0f;
  t[0] = tg[3 * i]; t[1] = tg[3 * i + 1]; t[2] = tg[3 * i + 2];
  const bool used = (w > 0.f) && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
  return used ? w : 0.f;
}

// v_posed of model vertex v at S.x: q0 + the ten shape rows + the corrective rows that move
__device__ __forceinline__ void posed_vertex(const harp_tree_model& M, const AfLds& S, int v, float q[3]) {
  const size_t NV3 = (size_t)M.NV * 3;
  q[0] = S.q0[v][0]; q[1] = S.q0[v][1]; q[2] = S.q0[v][2];
  {
    float sd[NSB][3];
#pragma unroll
    for (int k = 0; k < NSB; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) sd[k][c] = M.shapedirs_T[k * NV3 + 3 * v + c];
#pragma unroll
    for (int k = 0; k < NSB; ++k) {
      const float b = S.x[XB + k];
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c] += sd[k][c] * b;
    }
  }
#pragma unroll 2
  for (int row = 1; row < NIN; ++row) {                                // (27 loads in flight per joint)
    const float* pT = M.posedirs_T + (size_t)(S.drv[row] - 1) * 9 * NV3 + 3 * v;
    float pd[9][3];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) pd[k][c] = pT[k * NV3 + c];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float p = S.pmv[row][k];
#pragma unroll
      for (int c = 0; c < 3; ++c) q[c] += pd[k][c] * p;
    }
  }
}

// T_v = sum_j w_vj A_j, joints in order (w: the vertex's NJ weights, in memory or in LDS)
__device__ __forceinline__ void skin_T(const AfLds& S, const float* w, int NJ, float Tm[12]) {
#pragma unroll
  for (int k = 0; k < 12; ++k) Tm[k] = 0.f;
#pragma unroll 5
  for (int j = 0; j < NJ; ++j) {
    const float wj = w[j];
#pragma unroll
    for (int k = 0; k < 12; ++k) Tm[k] += wj * S.Aj[j][k];
  }
}

// skinned position (metres, centred, trans included) of posed vertex q
__device__ __forceinline__ void skin_pos(const AfLds& S, const float Tm[12], const float q[3], float pos[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) pos[r] = (Tm[r * 4] * q[0] + Tm[r * 4 + 1] * q[1] + Tm[r * 4 + 2] * q[2] + Tm[r * 4 + 3]) - S.cen[r] + S.x[XT + r];
}

// The target vertices at S.x after af_setup: S.q and C(x) (the same bits in every thread); optionally ALL model vertices to verts (mm)
__device__ float af_forward(const harp_tree_model& M, AfLds& S, int tid, const int32_t* __restrict__ idx, int n_t, const float* __restrict__ tg,
                            const float* __restrict__ wts, float pose_w, float wrist_w, float shape_w, float* __restrict__ verts) {
  const int NJ = M.NJ;
  float part = 0.f;
#pragma unroll 1
  for (int i = tid; i < n_t; i += kThreads) {
    const int v = target_vertex(M, idx, i);
    float q[3], Tm[12], pos[3], t[3];
    posed_vertex(M, S, v, q);
    S.q[i][0] = q[0]; S.q[i][1] = q[1]; S.q[i][2] = q[2];
    skin_T(S, M.weights + (size_t)v * NJ, NJ, Tm);
    skin_pos(S, Tm, q, pos);
    const float w = vertex_target(tg, wts, i, t);
    if (w > 0.f) {
      const float d0 = pos[0] - t[0], d1 = pos[1] - t[1], d2 = pos[2] - t[2];
      part += w * (d0 * d0 + d1 * d1 + d2 * d2);
    }
  }
  if (verts) {
#pragma unroll 1
    for (int v = tid; v < M.NV; v += kThreads) {
      float q[3], Tm[12], pos[3];
      posed_vertex(M, S, v, q);
      skin_T(S, M.weights + (size_t)v * NJ, NJ, Tm);
      skin_pos(S, Tm, q, pos);
      verts[3 * v] = pos[0] * 1000.0f; verts[3 * v + 1] = pos[1] * 1000.0f; verts[3 * v + 2] = pos[2] * 1000.0f;
    }
  }
  if (tid >= XP && tid < XB) {
    const float d = S.x[tid] - S.prior[tid];
    part += pose_w * d * d;
  } else if (tid >= XW && tid < XP) {
    part += wrist_w * S.x[tid] * S.x[tid];
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

// A (lower triangle) = J^T W J and S.gp = the four partial sums of J^T W r at S.x after af_setup (with the tangents) and af_forward;
// optionally the Jacobian (3 n_t, 64) itself
__device__ void af_normal(const harp_tree_model& M, AfLds& S, int tid, const int32_t* __restrict__ idx, int n_t, const float* __restrict__ tg,
                          const float* __restrict__ wts, float* __restrict__ jac) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;          // (wave-uniform for the compiler, unlike the caller's tid)
  const int NJ = M.NJ;
  const size_t NV3 = (size_t)M.NV * 3;
  const int n_tiles = (n_t + TV - 1) / TV;
  f32x16 acc00, acc10, acc11;
#pragma unroll
  for (int k = 0; k < 16; ++k) { acc00[k] = 0.f; acc10[k] = 0.f; acc11[k] = 0.f; }
  float gacc = 0.f;
#pragma unroll 1
  for (int tile = 0; tile < n_tiles; ++tile) {
    for (int i = tid; i < TV * NJ; i += kThreads) {                    // the tile's weight rows (a slot past the last target repeats it)
      const int l = i / NJ, j = i % NJ;
      S.sW[l][j] = M.weights[(size_t)target_vertex(M, idx, min(tile * TV + l, n_t - 1)) * NJ + j];
    }
    __syncthreads();
    const int it = tile * TV + lane, ic = min(it, n_t - 1);
    const int vc = target_vertex(M, idx, ic);
    float* row = &S.u.J[3 * lane][0];
    const float q[3] = {S.q[ic][0], S.q[ic][1], S.q[ic][2]};
    const float* wv = &S.sW[lane][0];
    float Tm[12];
    skin_T(S, wv, NJ, Tm);
    if (wave == 0) {
      float pos[3], t[3], sd[NSB][3];                                  // (the ten shape rows: one round trip, ahead of the sums)
#pragma unroll
      for (int k = 0; k < NSB; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) sd[k][c] = M.shapedirs_T[k * NV3 + 3 * vc + c];
      skin_pos(S, Tm, q, pos);
      const float w = (it < n_t) ? vertex_target(tg, wts, ic, t) : 0.f;
      S.wt[lane] = w;
      const float u[3] = {pos[0] - S.x[XT], pos[1] - S.x[XT + 1], pos[2] - S.x[XT + 2]};        // the wrist-relative vertex
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        S.res[3 * lane + r] = (w > 0.f) ? pos[r] - t[r] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          row[r * LD + XT + c] = (r == c) ? 1.f : 0.f;
          row[r * LD + c] = S.Om[c][r * 3] * u[0] + S.Om[c][r * 3 + 1] * u[1] + S.Om[c][r * 3 + 2] * u[2];
        }
      }
      float d[NSB][3];                                                 // the shape: the vertex's own blend shape and the joints' translations
#pragma unroll
      for (int k = 0; k < NSB; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) d[k][r] = (Tm[r * 4] * sd[k][0] + Tm[r * 4 + 1] * sd[k][1] + Tm[r * 4 + 2] * sd[k][2]);
#pragma unroll 1
      for (int j = 0; j < NJ; ++j) {
        const float wj = wv[j];
#pragma unroll
        for (int k = 0; k < NSB; ++k)
#pragma unroll
          for (int r = 0; r < 3; ++r) d[k][r] += wj * S.dAs[k][j][r];
      }
#pragma unroll
      for (int k = 0; k < NSB; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) row[r * LD + XB + k] = d[k][r] - S.dcen[XB + k][r];
    } else {
      const int r0 = (wave == 1) ? 1 : (wave == 2 ? 5 : 11), r1 = (wave == 1) ? 5 : (wave == 2 ? 11 : NIN);   // wrist + finger 0 | 1 2 | 3 4
#pragma unroll 1
      for (int rw = r0; rw < r1; ++rw) {
        const float* pT = M.posedirs_T + (size_t)(S.drv[rw] - 1) * 9 * NV3 + 3 * vc;
        float pd[9][3];                                                // (the joint's 27 corrective entries: one round trip)
#pragma unroll
        for (int m = 0; m < 9; ++m)
#pragma unroll
          for (int c = 0; c < 3; ++c) pd[m][c] = pT[m * NV3 + c];
        const int s0 = S.soff[rw], s1 = S.soff[rw + 1];
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
          const int i = 3 * rw + c;
          float dv[3] = {0.f, 0.f, 0.f}, d[3];
#pragma unroll
          for (int m = 0; m < 9; ++m) {
            const float dr = S.dR[i][m];
            dv[0] += pd[m][0] * dr; dv[1] += pd[m][1] * dr; dv[2] += pd[m][2] * dr;
          }
#pragma unroll
          for (int r = 0; r < 3; ++r) d[r] = Tm[r * 4] * dv[0] + Tm[r * 4 + 1] * dv[1] + Tm[r * 4 + 2] * dv[2];
#pragma unroll 1
          for (int s = s0; s < s1; ++s) {
            const int j = S.sj[s];
            const float wj = wv[j];
            const float* dG = S.dGt[s][c];
            const float p[3] = {q[0] - S.Jr[j][0], q[1] - S.Jr[j][1], q[2] - S.Jr[j][2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) d[r] += wj * (dG[r * 4] * p[0] + dG[r * 4 + 1] * p[1] + dG[r * 4 + 2] * p[2] + dG[r * 4 + 3]);
          }
          row[i] = d[0] - S.dcen[i][0]; row[LD + i] = d[1] - S.dcen[i][1]; row[2 * LD + i] = d[2] - S.dcen[i][2];
        }
      }
    }
    __syncthreads();
    if (jac) {
      const int n = min(TV, n_t - tile * TV) * 3 * NX;                 // rows of real targets only
      float* jo = jac + (size_t)tile * TV * 3 * NX;
      for (int i = tid; i < n; i += kThreads) jo[i] = S.u.J[i / NX][i % NX];
    }
    lm::gram_accumulate(S.u.J, S.wt, wave, lane, acc00, acc10, acc11);
    {
#pragma unroll 4
      for (int kk = 0; kk < 48; ++kk) {                                // g: column `lane`, this wave's 48 rows, in order
        const int k = 48 * wave + kk;
        gacc += S.u.J[k][lane] * (S.wt[k / 3] * S.res[k]);
      }
    }
    __syncthreads();
  }
  S.gp[wave][lane] = gacc;
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

__device__ __forceinline__ bool frozen_col(int c, int solve_shape, int solve_wrist) {
  return (c >= XB && c < XT && !solve_shape) || (c >= XW && c < XP && !solve_wrist);
}

__global__ void __launch_bounds__(kThreads, 1)
arm_vertex_fit_kernel(const harp_tree_model M, const int32_t* __restrict__ vert_idx, int n_t, const float* __restrict__ targets,
                      const float* __restrict__ weights, const float* __restrict__ prior, int iters, float lambda, float pose_w, float wrist_w,
                      float shape_w, int solve_shape, int solve_wrist, int betas_per_frame, float* __restrict__ in_pose,
                      float* __restrict__ betas, float* __restrict__ trans, float* __restrict__ cost, int32_t* __restrict__ status,
                      float* __restrict__ verts, float* __restrict__ jac, float* __restrict__ Aout, float* __restrict__ gout) {
  extern __shared__ float s_raw[];
  int lds0 = 0;                                                        // (see csrc/vertex_fit.hip: the LDS base is taken afresh per evaluation)
  asm volatile("" : "+v"(lds0));
  AfLds& S0 = *reinterpret_cast<AfLds*>(s_raw + lds0);
  const int t = blockIdx.x, wave = threadIdx.x >> 6;                   // (the grid is exactly T workgroups)
  int tid = threadIdx.x;
  const float* tg = targets + (size_t)t * n_t * 3;
  const float* wts = weights ? weights + (size_t)t * n_t : nullptr;
  const size_t brow = (solve_shape || betas_per_frame) ? (size_t)t * NSB : 0;
  float xl = 0.f;                                                      // wave 0, lane l: unknown l
  if (tid < XB) xl = in_pose[(size_t)t * XB + tid];
  else if (tid < XT) xl = betas[brow + (tid - XB)];
  else if (tid < NX) xl = trans[(size_t)t * 3 + (tid - XT)];
  if (tid < NX) {
    S0.x[tid] = xl;
    S0.prior[tid] = (prior && tid >= XP && tid < XB) ? prior[(size_t)t * 45 + (tid - XP)] : 0.f;
  }
  int n_used = 0;
  for (int r = 0; r < (n_t + kThreads - 1) / kThreads; ++r) {
    const int i = tid + r * kThreads;
    float tt[3];
    n_used += __syncthreads_count(i < n_t && vertex_target(tg, wts, min(i, n_t - 1), tt) > 0.f);
  }
  af_prologue(M, S0, tid);
  if (S0.bad) {                                                        // a tree these tables do not hold: nothing is solved or written
    if (tid == 0) { cost[2 * (size_t)t] = 0.f; cost[2 * (size_t)t + 1] = 0.f; status[t] = -2; }
    return;
  }
  const bool solve = n_used >= MIN_USED;
  const bool frozen = frozen_col(tid, solve_shape, solve_wrist);       // (of wave 0's lanes)

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
    asm volatile("" : "+v"(lds0));
    AfLds& S = *reinterpret_cast<AfLds*>(s_raw + lds0);
    const bool at_x = !(e & 1), last = e == 2 * iters;
    if (at_x && tid < NX) S.x[tid] = xl;
    __syncthreads();
    af_setup(M, S, tid, at_x);
    const float Ce = af_forward(M, S, tid, vert_idx, n_t, tg, wts, pose_w, wrist_w, shape_w,
                                (last && verts) ? verts + (size_t)t * M.NV * 3 : nullptr);
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
    af_normal(M, S, tid, vert_idx, n_t, tg, wts, (last && jac) ? jac + (size_t)t * n_t * 3 * NX : nullptr);
    // priors, frozen columns, g
    float g = 0.f, diag = 1.f;
    if (tid < NX) {
      g = ((S.gp[0][tid] + S.gp[1][tid]) + S.gp[2][tid]) + S.gp[3][tid];
      diag = S.u.A[tid][tid];
      if (tid >= XP && tid < XB) { g += pose_w * (xl - S.prior[tid]); diag += pose_w; }
      else if (tid >= XW && tid < XP) { g += wrist_w * xl; diag += wrist_w; }
      else if (tid >= XB && tid < XT) { g += shape_w * xl; diag += shape_w; }
      if (frozen) { g = 0.f; diag = 1.f; }
    }
    __syncthreads();
    if (tid < NX) S.u.A[tid][tid] = diag;
    if (!solve_shape || !solve_wrist)
      for (int i = tid; i < NX * NX; i += kThreads) {
        const int r = i / NX, c = i % NX;
        if (r > c && (frozen_col(r, solve_shape, solve_wrist) || frozen_col(c, solve_shape, solve_wrist))) S.u.A[r][c] = 0.f;
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
      xn = xl + z * s;
      S.x[tid] = xn;
      if (tid == 0) S.flag = okw ? 1 : 0;
    }
    __syncthreads();
    ok = __builtin_amdgcn_readfirstlane(S.flag) != 0;
  }

  if (solve && iters > 0 && tid < NX && !frozen) {
    if (tid < XB) in_pose[(size_t)t * XB + tid] = xl;
    else if (tid < XT) betas[brow + (tid - XB)] = xl;
    else trans[(size_t)t * 3 + (tid - XT)] = xl;
  }
  if (tid == 0) {
    cost[2 * (size_t)t] = C0;
    cost[2 * (size_t)t + 1] = C;
    status[t] = solve ? n_acc : -1;
  }
}

}  // namespace

extern "C" int harp_arm_vertex_fit_frames_per_block(void) { return kAfFramesPerBlock; }

extern "C" int harp_arm_vertex_fit(const harp_tree_model* m, const int32_t* vert_idx, int n_t, const float* targets, const float* weights,
                                   const float* prior, int T, const harp_arm_vertex_fit_options* opt, float* in_pose, float* betas, float* trans,
                                   float* cost, int32_t* status, float* verts, float* jac, float* A, float* g, hipStream_t stream) {
  if (!m || !opt || !targets || !in_pose || !betas || !trans || !cost || !status || T <= 0 || opt->iters < 0) return HARP_ERR_ARG;
  if (m->n_pose_in != NIN || m->NB < NSB || m->NB > MAXB || m->NJ < 1 || m->NJ > MAXJ || m->NV < 1 || m->NV > MAXV) return HARP_ERR_ARG;
  if (m->center_joint < 0 || m->center_joint >= m->NJ) return HARP_ERR_ARG;
  if (n_t < 1 || n_t > m->NV || (!vert_idx && n_t != m->NV)) return HARP_ERR_ARG;
  const float nonneg[4] = {opt->lambda0, opt->pose_prior_weight, opt->wrist_prior_weight, opt->shape_prior_weight};
  for (float v : nonneg)
    if (!(v >= 0.f) || isinf(v)) return HARP_ERR_ARG;
  // dynamic LDS above 64 KB has to be requested; per-device attribute, set on every call
  if (hipFuncSetAttribute((const void*)arm_vertex_fit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AfLds)) != hipSuccess)
    return HARP_ERR_ARG;
  hipLaunchKernelGGL(arm_vertex_fit_kernel, dim3((unsigned)T), dim3(kThreads), sizeof(AfLds), stream, *m, vert_idx, n_t, targets, weights, prior,
                     opt->iters, opt->lambda0, opt->pose_prior_weight, opt->wrist_prior_weight, opt->shape_prior_weight, opt->solve_shape != 0,
                     opt->solve_wrist != 0, opt->betas_per_frame != 0, in_pose, betas, trans, cost, status, verts, jac, A, g);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
