// Batched 2.5-D reprojection inverse kinematics of the SMPL-X right arm for gfx950 (ops.arm_reproj_ik; playback
// Motion.from_arm_image_keypoints): up to 22 image keypoints per problem (the wrist, the five fingers root to tip, the
// elbow), in pixels, optionally with a wrist-relative depth per joint -> the rows [rot | wrist | pose | trans] that harp_lbs_tree_fwd and
// the player's camera turn back into those pixels.  Nothing in the reference does this.  Two files own the mathematics and this one
// repeats both: csrc/arm_ik.hip (§29) the joints of the tree and their derivative — the prologue, the level-parallel chain, the skinned
// vertex rows, the slot recursion, the root and elbow structure — and csrc/reproj_ik.hip (§30) the camera, the rows (u, v, d), which
// entries are used, and the guard against a joint behind the camera.  The forward is written out here rather than shared with
// arm_ik.hip because every fold of a one-wave kernel's forward into a header cost that kernel 0.3-1.6 % (§31), and this file was to
// change no existing code object; a later change may fold the two arm forwards under §31's procedure.  The slot tables are
// tree_slots_body.h's, the solve is lm_solve_body.h's (lm::jacobi_scale, lm::solve, lm::damped), the rotations lbs_tree_body.h's
// (lt::rod_fwd, lt::rod_jvp), so the solver and the renderer cannot disagree.
//
// harp_arm_reproj_ik: N independent Levenberg-Marquardt solves in ONE launch, one wave (= one workgroup) per problem, 54 unknowns
// x = [rot 3 | wrist 3 | pose 45 | trans 3] and 3 n_out <= 66 rows (include/harp_hip.h states the contract):
//   Z_k = j_k.z + t_z, u_k = S/2 + focal (j_k.x + cam1) / Z_k, v_k = S/2 + focal (j_k.y + cam2) / Z_k, d_k = j_k.z - j_0.z
// with j(x) the n_out joints of harp_arm_ik in metres.
//
//   prologue     csrc/arm_ik.hip's: the tree's tables, the rotations nothing drives, the rest joints at this shape, the vertex rows' q0.
//   forward      csrc/arm_ik.hip's up to the 3 n_out joint coordinates; then lane k < n_out projects joint k: its Z, its three rows, their
//                residuals and its share of the cost (a butterfly sum, fixed order), and for the Jacobian focal / Z_k and
//                focal (j + cam) / Z_k^2, kept in the first floats of the normal matrix's storage, which is dead then.
//   Jacobian     lane i < 54 owns column i: first the 3-D entries as csrc/arm_ik.hip writes them (the elbow's rows in the 48 wrist and
//                finger columns exactly 0), then the same lane turns its own column into (u, v, d) rows in place, as csrc/reproj_ik.hip:
//                du = focal/Z dj.x - focal (j.x + cam1)/Z^2 dj.z, dd = dj_k.z - dj_0.z.  0 - 0 stays 0: the elbow's zeros and
//                d d / d trans = 0 survive the conversion bit for bit.
//   normal eqs., solve, accept: csrc/arm_ik.hip's with the row weights (w_k, w_k, wz_k), the three priors on the diagonal, a frozen wrist
//                column as there; a candidate with a used pixel joint at Z_k <= 1e-3 is a rejection.
// `iters` iterations whatever happens: no early exit, every branch that holds a barrier is uniform over the wave.  No workspace, no
// allocation, no synchronisation, no atomics: the launch can be captured and a repeated call gives the same bits.
#include "lm_solve_body.h"
#include "tree_slots_body.h"                                           // (NIN, MAXSLOT, NOSLOT, TreeTables; lbs_tree_body.h)

#include <math.h>

namespace {

using namespace lt;

constexpr int NX = 54;                  // unknowns per problem
constexpr int NO = HARP_ARM_IK_MAX_JOINTS;
constexpr int NR = 3 * NO;              // rows held (those past 3 n_joints_out stay zero)
constexpr int LD = 55;                  // row stride of J and A in LDS (odd)
constexpr int XW = 3, XP = 6, XT = 51;  // first wrist / finger / trans column
constexpr int NSB = 10;                 // shape coefficients given (the model's other NB - 10 are zero)
constexpr int kFramesPerBlock = 1;      // one wave per workgroup: LDS (48.3 KiB a problem: three on a CU) bounds the problems in flight
constexpr float kZMin = 1e-3f;          // a used joint nearer than this (metres along the view axis) is behind the camera

struct ArLds {
  // the model's structure and what no unknown moves (prologue)
  TreeTables t;
  int jsrc[NO];                         // the model's joint_src
  int vrow[NO], nv;                     // the output rows that are skinned vertices, in order
  float beta[NSB];
  float W[NR], tgt[NR];                 // the row weights (w_k, w_k, wz_k) and targets, both zero for an unused row
  float cam[3];                         // (t_z, cam1, cam2)
  float q0[NO][3];                      // a vertex row's rest position at this shape with the constant correctives
  float sW[NO][MAXJ + 1];               // a vertex row's skin weights (odd stride)
  // the point and its chain (every evaluation)
  float x[NX];
  float R[MAXJ][9], G[MAXJ][12], Aj[MAXJ][12], Jr[MAXJ][3];
  float pmv[NIN][9];                    // R - I of a driven joint: the corrective rows that move
  float cen[3];
  float q[NO][3], Tm[NO][12];           // a vertex row's posed position and blended transform
  float jnt[NR];                        // the joints, metres
  // at x only
  float res[NR], prj[NR];
  float dR[NIN * 3][9], Om[3][9];       // d R / d x[col];  dR_0/d rot[c] R_0^T
  float J[NR][LD];                      // d joints (metres, output order) / d x while the columns are pushed, then d (u, v, d) rows / d x
  union {                               // (an evaluation is over before the normal matrix is formed, and begins after the solves)
    float A[NX][LD];                    // normal matrix, then its scaled Cholesky factor in the lower triangle
    struct {
      float iz[NO], px[NO], py[NO];     // focal / Z_k, focal (j_k.x + cam1) / Z_k^2, focal (j_k.y + cam2) / Z_k^2: projecting -> column lanes
      float dGt[MAXSLOT][3][12];        // [dG_j | dt_j] of a slot's joint by the column's three axes
      float qp[NO * 3][NIN - 1];        // a vertex row's corrective sum joint by joint (one lane per (coordinate, joint): one round trip)
    } e;
  } u;
};
static_assert(sizeof(ArLds) == 49452, "three problems on a CU rest on this size: at most 54608 (DESIGN.md §35)");
static_assert(sizeof(ArLds) <= 54608, "three problems on a CU");

__device__ __forceinline__ void joint_aa(const harp_tree_model& M, const ArLds& S, int row, float aa[3]) {
  const int j = S.t.drv[row];
#pragma unroll
  for (int c = 0; c < 3; ++c) aa[c] = M.pose_mean[3 * j + c] + S.x[3 * row + c];            // (lbs_tree_body.h:90)
}

// the model vertex of output row k (joint_src[k] < 0), held inside the model
__device__ __forceinline__ int row_vertex(const harp_tree_model& M, int src) { return min(max(-src - 1, 0), M.NV - 1); }

// Once per problem.  Sets S.t.bad when the model is not of the shape the tables hold.
__device__ void ar_prologue(const harp_tree_model& M, ArLds& S, int l, const float* __restrict__ beta_row, int n_out) {
  const int NJ = M.NJ, NB = M.NB, NP = (NJ - 1) * 9;
  if (l < NSB) S.beta[l] = beta_row[l];
  if (l < NO) S.jsrc[l] = (l < n_out) ? M.joint_src[l] : 0;
  for (int i = l; i < NR * LD; i += 64) (&S.J[0][0])[i] = 0.f;
  for (int i = l; i < NR; i += 64) { S.res[i] = 0.f; S.jnt[i] = 0.f; S.prj[i] = 0.f; }
  tree_tables<64>(M, S.t, l);                                          // (its first barrier orders the lines above)
  if (S.t.bad) return;
  if (l == 0) {
    int nv = 0;
    for (int k = 0; k < n_out; ++k)
      if (S.jsrc[k] < 0) S.vrow[nv++] = k;
    S.nv = nv;
  }
  __syncthreads();
  for (int i = l; i < S.nv * NJ; i += 64) {                            // the vertex rows' skin weights
    const int k = S.vrow[i / NJ], j = i % NJ;
    S.sW[k][j] = M.weights[(size_t)row_vertex(M, S.jsrc[k]) * NJ + j];
  }
  undriven_rotation(M, S.t, l, S.R);                                   // the joints nothing drives: their rotation is the model's
  for (int i = l; i < NJ * 3; i += 64) {                               // rest joints at this shape (lbs_tree_body.h:100-112)
    float acc = M.J_template[i];
#pragma unroll
    for (int k = 0; k < NSB; ++k) acc += M.J_dirs[(size_t)i * NB + k] * S.beta[k];
    S.Jr[i / 3][i % 3] = acc;
  }
  __syncthreads();
  for (int i = l; i < S.nv * 3; i += 64) {                             // q0 of the vertex rows
    const int k = S.vrow[i / 3], c = i % 3, src = S.jsrc[k];
    const size_t e = (size_t)row_vertex(M, src) * 3 + c;
    float q = M.v_template[e];
#pragma unroll
    for (int b = 0; b < NSB; ++b) q += M.shapedirs_T[(size_t)b * M.NV * 3 + e] * S.beta[b];
    for (int j = 1; j < NJ; ++j) {
      if (S.t.driven[j]) continue;
      for (int m = 0; m < 9; ++m) {
        const float p = S.R[j][m] - ((m == 0 || m == 4 || m == 8) ? 1.f : 0.f);
        if (p != 0.f) q += M.posedirs[e * NP + (j - 1) * 9 + m] * p;   // (rod_fwd(0) = I exactly: a zero mean costs no load)
      }
    }
    S.q0[k][c] = q;
  }
  __syncthreads();
}

// The joints, projected rows and cost at xl (lane l's unknown); JAC: also S.res, S.prj and the Jacobian S.J.  Returns C(x), the same bits
// in every lane; behind: a used pixel joint at Z <= kZMin (uniform over the wave).  pw, pc: this lane's diagonal of P (the wrist prior's
// weight in lanes 3..5, the pose prior's in 6..50, trans_z's in lane 53, else 0) and what it pulls towards.
template <bool JAC>
__device__ float ar_eval(const harp_tree_model& M, ArLds& S, int l, float xl, float pw, float pc, int n_out, float focal, float half,
                         bool& behind) {
  const int NJ = M.NJ, NP = (NJ - 1) * 9, cj = M.center_joint;
  const TreeTables& T = S.t;
  if (l < NX) S.x[l] = xl;
  __syncthreads();
  if (l < NIN) {
    float aa[3], R[9];
    joint_aa(M, S, l, aa);
    rod_fwd(aa, R);
    const int j = T.drv[l];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      S.R[j][k] = R[k];
      S.pmv[l][k] = R[k] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
    }
  }
  if (JAC && l < NIN * 3) {
    float aa[3], dR[9];
    joint_aa(M, S, l / 3, aa);
    rod_jvp(aa, l % 3, dR);
#pragma unroll
    for (int k = 0; k < 9; ++k) S.dR[l][k] = dR[k];
  }
  __syncthreads();
  if (l == 0) {
    for (int k = 0; k < 9; ++k) S.G[0][(k / 3) * 4 + (k % 3)] = S.R[0][k];
    for (int r = 0; r < 3; ++r) S.G[0][r * 4 + 3] = S.Jr[0][r];
  }
  // batch_rigid_transform level by level (lbs_tree_body.h:114-139)
  const int maxd = T.maxd;
  for (int d = 1; d <= maxd; ++d) {
    __syncthreads();
    if (l < NJ && T.depth[l] == d) {
      const int j = l, p = T.par[j];
      const float rel[3] = {S.Jr[j][0] - S.Jr[p][0], S.Jr[j][1] - S.Jr[p][1], S.Jr[j][2] - S.Jr[p][2]};
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
          S.G[j][r * 4 + c] = S.G[p][r * 4] * S.R[j][c] + S.G[p][r * 4 + 1] * S.R[j][3 + c] + S.G[p][r * 4 + 2] * S.R[j][6 + c];
        S.G[j][r * 4 + 3] = S.G[p][r * 4] * rel[0] + S.G[p][r * 4 + 1] * rel[1] + S.G[p][r * 4 + 2] * rel[2] + S.G[p][r * 4 + 3];
      }
    }
  }
  __syncthreads();
  for (int i = l; i < NJ * 12; i += 64) {                              // A_j = [G_j | t_j - G_j J_j]
    const int j = i / 12, e = i % 12, r = e / 4, c = e % 4;
    S.Aj[j][e] = (c < 3) ? S.G[j][e]
                         : S.G[j][r * 4 + 3] - (S.G[j][r * 4] * S.Jr[j][0] + S.G[j][r * 4 + 1] * S.Jr[j][1] + S.G[j][r * 4 + 2] * S.Jr[j][2]);
  }
  if (l < 3) S.cen[l] = S.G[cj][l * 4 + 3];
  const int nv = S.nv;
  for (int p = l; p < nv * 3 * (NIN - 1); p += 64) {                   // posed vertex rows: the corrective rows that move, joint by joint
    const int i = p / (NIN - 1), row = p % (NIN - 1) + 1, k = S.vrow[i / 3], c = i % 3;
    const float* pj = M.posedirs + ((size_t)row_vertex(M, S.jsrc[k]) * 3 + c) * NP + (T.drv[row] - 1) * 9;
    float pd[9], acc = 0.f;
#pragma unroll
    for (int m = 0; m < 9; ++m) pd[m] = pj[m];
#pragma unroll
    for (int m = 0; m < 9; ++m) acc += pd[m] * S.pmv[row][m];
    S.u.e.qp[i][row - 1] = acc;
  }
  __syncthreads();
  for (int i = l; i < nv * 3; i += 64) {                               // ... q0 + the joints' sums in order
    const int k = S.vrow[i / 3], c = i % 3;
    float acc = S.q0[k][c];
#pragma unroll
    for (int r = 0; r < NIN - 1; ++r) acc += S.u.e.qp[i][r];
    S.q[k][c] = acc;
  }
  for (int i = l; i < nv * 12; i += 64) {                              // T_k = sum_j w_kj A_j, all NJ joints in order
    const int k = S.vrow[i / 12], e = i % 12;
    float acc = 0.f;
    for (int j = 0; j < NJ; ++j) acc += S.sW[k][j] * S.Aj[j][e];
    S.Tm[k][e] = acc;
  }
  __syncthreads();
  for (int i = l; i < n_out * 3; i += 64) {
    const int k = i / 3, c = i % 3, src = S.jsrc[k];
    float v;
    if (src >= 0) {
      v = S.G[min(src, NJ - 1)][c * 4 + 3];
    } else {
      const float* Tm = S.Tm[k];
      const float* q = S.q[k];
      v = Tm[c * 4] * q[0] + Tm[c * 4 + 1] * q[1] + Tm[c * 4 + 2] * q[2] + Tm[c * 4 + 3];
    }
    S.jnt[i] = (v - S.cen[c]) + S.x[XT + c];
  }
  __syncthreads();
  float part = 0.f;
  bool bad = false;
  if (l < n_out) {                                                     // joint l through the camera: its rows (u, v, d)
    const float jx = S.jnt[3 * l] + S.cam[1], jy = S.jnt[3 * l + 1] + S.cam[2], jz = S.jnt[3 * l + 2];
    const float Z = jz + S.cam[0];
    const float wp = S.W[3 * l], wz = S.W[3 * l + 2];                  // (0 for an unused row; S.tgt too)
    const bool front = Z > kZMin;
    bad = (wp > 0.f) && !front;
    const bool proj = front || (wp > 0.f);                             // neither used nor in front: nothing to divide by, rows of zeros
    const float iz = proj ? focal / Z : 0.f;
    const float u = proj ? half + iz * jx : 0.f, v = proj ? half + iz * jy : 0.f, d = jz - S.jnt[2];
    const float ru = (wp > 0.f) ? (u - S.tgt[3 * l]) : 0.f, rv = (wp > 0.f) ? (v - S.tgt[3 * l + 1]) : 0.f;
    const float rd = (wz > 0.f) ? (d - S.tgt[3 * l + 2]) : 0.f;
    part = wp * ru * ru + wp * rv * rv + wz * rd * rd;
    if (JAC) {
      S.prj[3 * l] = u; S.prj[3 * l + 1] = v; S.prj[3 * l + 2] = d;
      S.res[3 * l] = ru; S.res[3 * l + 1] = rv; S.res[3 * l + 2] = rd;
      S.u.e.iz[l] = iz; S.u.e.px[l] = proj ? iz * jx / Z : 0.f; S.u.e.py[l] = proj ? iz * jy / Z : 0.f;
    }
  }
  part += pw * (xl - pc) * (xl - pc);
  behind = __any(bad) != 0;
  const float cost = __shfl(wave_sum(part), 0, 64);
  if (!JAC) return cost;

  // ---- Jacobian columns, 3-D entries first
  if (l < 3) {                                                         // the root: Omega_c = dR_0 R_0^T
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k)
        S.Om[l][r * 3 + k] = S.dR[l][r * 3] * S.R[0][k * 3] + S.dR[l][r * 3 + 1] * S.R[0][k * 3 + 1] + S.dR[l][r * 3 + 2] * S.R[0][k * 3 + 2];
  } else if (l < XT) {                                                 // a wrist or finger column down its slots
    const int row = l / 3, c = l % 3;
    for (int s = T.soff[row]; s < T.soff[row + 1]; ++s) {
      const int j = T.sj[s], ps = T.sp[s], p = T.par[j];
      float* o = S.u.e.dGt[s][c];
      if (ps < 0) {                                                    // G_q = G_p [R_q | .]: d G_q = G_p dR, the joint's position stays
        for (int r = 0; r < 3; ++r) {
          for (int k = 0; k < 3; ++k)
            o[r * 4 + k] = S.G[p][r * 4] * S.dR[l][k] + S.G[p][r * 4 + 1] * S.dR[l][3 + k] + S.G[p][r * 4 + 2] * S.dR[l][6 + k];
          o[r * 4 + 3] = 0.f;
        }
      } else {
        const float* pg = S.u.e.dGt[ps][c];
        const float rel[3] = {S.Jr[j][0] - S.Jr[p][0], S.Jr[j][1] - S.Jr[p][1], S.Jr[j][2] - S.Jr[p][2]};
        for (int r = 0; r < 3; ++r) {
          for (int k = 0; k < 3; ++k) o[r * 4 + k] = pg[r * 4] * S.R[j][k] + pg[r * 4 + 1] * S.R[j][3 + k] + pg[r * 4 + 2] * S.R[j][6 + k];
          o[r * 4 + 3] = pg[r * 4] * rel[0] + pg[r * 4 + 1] * rel[1] + pg[r * 4 + 2] * rel[2] + pg[r * 4 + 3];
        }
      }
    }
  }
  __syncthreads();
  if (l < 3) {
#pragma unroll 1
    for (int k = 0; k < n_out; ++k) {
      const float u[3] = {S.jnt[3 * k] - S.x[XT], S.jnt[3 * k + 1] - S.x[XT + 1], S.jnt[3 * k + 2] - S.x[XT + 2]};   // centre-relative
      for (int r = 0; r < 3; ++r) S.J[3 * k + r][l] = S.Om[l][r * 3] * u[0] + S.Om[l][r * 3 + 1] * u[1] + S.Om[l][r * 3 + 2] * u[2];
    }
  } else if (l < XT) {
    const int row = l / 3, c = l % 3, s0 = T.soff[row], s1 = T.soff[row + 1];
    const int sc = T.spos[row][cj];
    float dc[3] = {0.f, 0.f, 0.f};                                     // d (posed centre): zero when the centre is the column's joint or above it
    if (sc != NOSLOT) { dc[0] = S.u.e.dGt[sc][c][3]; dc[1] = S.u.e.dGt[sc][c][7]; dc[2] = S.u.e.dGt[sc][c][11]; }
#pragma unroll 1
    for (int k = 0; k < n_out; ++k) {
      const int src = S.jsrc[k];
      float d[3] = {0.f, 0.f, 0.f};
      if (src >= 0) {
        const int s = T.spos[row][min(src, NJ - 1)];
        if (s != NOSLOT) { d[0] = S.u.e.dGt[s][c][3]; d[1] = S.u.e.dGt[s][c][7]; d[2] = S.u.e.dGt[s][c][11]; }
      } else {
        const int v = row_vertex(M, src);
        const float* Tm = S.Tm[k];
        const float* q = S.q[k];
        float dv[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {                               // the row's correctives of this joint's 9 pose_map entries
          const float* pd = M.posedirs + ((size_t)v * 3 + cc) * NP + (T.drv[row] - 1) * 9;
          float acc = 0.f;
#pragma unroll
          for (int m = 0; m < 9; ++m) acc += pd[m] * S.dR[l][m];
          dv[cc] = acc;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = Tm[r * 4] * dv[0] + Tm[r * 4 + 1] * dv[1] + Tm[r * 4 + 2] * dv[2];
#pragma unroll 1
        for (int s = s0; s < s1; ++s) {
          const int j = T.sj[s];
          const float wj = S.sW[k][j];
          const float* dG = S.u.e.dGt[s][c];
          const float p[3] = {q[0] - S.Jr[j][0], q[1] - S.Jr[j][1], q[2] - S.Jr[j][2]};
#pragma unroll
          for (int r = 0; r < 3; ++r) d[r] += wj * (dG[r * 4] * p[0] + dG[r * 4 + 1] * p[1] + dG[r * 4 + 2] * p[2] + dG[r * 4 + 3]);
        }
      }
      S.J[3 * k][l] = d[0] - dc[0]; S.J[3 * k + 1][l] = d[1] - dc[1]; S.J[3 * k + 2][l] = d[2] - dc[2];
    }
  } else if (l < NX) {
    for (int i = 0; i < n_out * 3; ++i) S.J[i][l] = (i % 3 == l - XT) ? 1.f : 0.f;
  }
  // ---- this lane's own column: 3-D entries -> (u, v, d) rows, in place (iz, px, py were written before the barrier above)
  if (l < NX) {
    const float dz0 = S.J[2][l];                                       // (the wrist is output joint 0)
#pragma unroll 1
    for (int k = 0; k < n_out; ++k) {
      const float dx = S.J[3 * k][l], dy = S.J[3 * k + 1][l], dz = S.J[3 * k + 2][l];
      S.J[3 * k][l] = S.u.e.iz[k] * dx - S.u.e.px[k] * dz;
      S.J[3 * k + 1][l] = S.u.e.iz[k] * dy - S.u.e.py[k] * dz;
      S.J[3 * k + 2][l] = dz - dz0;
    }
  }
  __syncthreads();
  return cost;
}

struct ArInputs {
  const float *betas, *cam, *targets, *weights, *depth_weights, *prior, *wrist_prior, *z_prior;
};

__global__ void __launch_bounds__(64) arm_reproj_ik_kernel(const harp_tree_model M, const ArInputs in, const harp_arm_reproj_ik_options opt,
                                                           float* __restrict__ in_pose, float* __restrict__ trans, float* __restrict__ cost,
                                                           int32_t* __restrict__ status, float* __restrict__ proj, float* __restrict__ jac) {
  __shared__ ArLds S;
  const int t = blockIdx.x, l = threadIdx.x;                           // (the grid is exactly N workgroups of one wave)
  const int n_out = M.n_joints_out, nr = 3 * n_out;
  const int lc = min(l, NX - 1);
  const int iters = opt.iters;
  const float focal = opt.focal, half = 0.5f * (float)opt.S;
  float lambda = opt.lambda0;
  float xl = 0.f;
  if (l < XT) xl = in_pose[(size_t)t * XT + l];
  else if (l < NX) xl = trans[(size_t)t * 3 + (l - XT)];
  if (l == 63) {
    const float* c = in.cam + (opt.cam_per_frame ? (size_t)t * 3 : 0);
    S.cam[0] = 2.0f * focal / ((float)opt.S * c[0] + 1e-9f);           // t_z
    S.cam[1] = c[1]; S.cam[2] = c[2];
  }
  bool used = false;
  if (l < NO) {
    float w = 0.f, wz = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (l < n_out) {
      w = in.weights ? in.weights[(size_t)t * n_out + l] : 1.0f;
      wz = (in.depth_weights && l > 0) ? in.depth_weights[(size_t)t * n_out + l] : 0.f;
      const float* tg = in.targets + ((size_t)t * n_out + l) * 3;
      t0 = tg[0]; t1 = tg[1]; t2 = tg[2];
      used = (w > 0.f) && isfinite(t0) && isfinite(t1);
    }
    const bool used_z = (wz > 0.f) && isfinite(t2);
    S.W[3 * l] = S.W[3 * l + 1] = used ? w : 0.f;
    S.W[3 * l + 2] = used_z ? wz : 0.f;
    S.tgt[3 * l] = used ? t0 : 0.f; S.tgt[3 * l + 1] = used ? t1 : 0.f; S.tgt[3 * l + 2] = used_z ? t2 : 0.f;
  }
  const bool enough = __popcll(__ballot(used)) >= 4;
  ar_prologue(M, S, l, in.betas + (opt.betas_per_frame ? (size_t)t * NSB : 0), n_out);
  if (S.t.bad) {                                                       // a tree the tables do not hold: nothing is solved or written
    if (l == 0) { cost[2 * (size_t)t] = 0.f; cost[2 * (size_t)t + 1] = 0.f; status[t] = -2; }
    return;
  }

  const bool pose_lane = l >= XP && l < XT, wrist_lane = l >= XW && l < XP, z_lane = l == XT + 2;
  const bool frozen = wrist_lane && !opt.solve_wrist;
  const float pw = pose_lane ? opt.pose_prior_weight : (wrist_lane ? opt.wrist_prior_weight : (z_lane ? opt.z_prior_weight : 0.f));
  float pc = 0.f;                                                      // what this lane's prior pulls towards
  if (pose_lane && in.prior) pc = in.prior[(size_t)t * 45 + (l - XP)];
  if (wrist_lane && in.wrist_prior) pc = in.wrist_prior[(size_t)t * 3 + (l - XW)];
  if (z_lane && in.z_prior) pc = in.z_prior[t];
  bool behind0, behind;
  float C = ar_eval<true>(M, S, l, xl, pw, pc, n_out, focal, half, behind0);
  const float C0 = C;
  const bool solve = enough && !behind0;
  int n_acc = 0;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // this lane's weighted column, gradient entry and row of A
    float Jw[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) Jw[k] = S.W[k] * S.J[k][lc];
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < NR; ++k) g += Jw[k] * S.res[k];
    g += pw * (xl - pc);
    if (frozen) g = 0.f;
    float diag = 1.f;
#pragma unroll 1
    for (int j = 0; j < NX; ++j) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < NR; ++k) a += Jw[k] * S.J[k][j];
      const bool fj = !opt.solve_wrist && j >= XW && j < XP;
      if (j == l) {
        a = frozen ? 1.f : a + pw;
        diag = a;
      } else if (frozen || fj) {
        a = 0.f;
      }
      if (l < NX) S.u.A[l][j] = a;
    }
    bool ok;
    const float s = lm::jacobi_scale<NX>(l, diag, lambda, ok);
    __syncthreads();
    const float z = lm::solve<NX, LD, 1, 6>(S.u.A, l, s, -g * s, true, ok);
    const float xn = (l < NX) ? xl + z * s : 0.f;
    const float Cn = ar_eval<false>(M, S, l, xn, pw, pc, n_out, focal, half, behind);
    const bool accept = __builtin_amdgcn_readfirstlane((int)(ok && solve && !behind && (Cn < C))) != 0;       // (a NaN is not less)
    if (accept) {
      xl = xn;
      lambda = lm::damped(lambda, true);
      ++n_acc;
      C = ar_eval<true>(M, S, l, xl, pw, pc, n_out, focal, half, behind);
    } else {
      lambda = lm::damped(lambda, false);
    }
  }

  if (solve && iters > 0 && !frozen) {
    if (l < XT) in_pose[(size_t)t * XT + l] = xl;
    else if (l < NX) trans[(size_t)t * 3 + (l - XT)] = xl;
  }
  if (l == 0) {
    cost[2 * (size_t)t] = C0;
    cost[2 * (size_t)t + 1] = C;
    status[t] = !enough ? -1 : (behind0 ? -3 : n_acc);
  }
  if (proj)
    for (int i = l; i < nr; i += 64) proj[(size_t)t * nr + i] = S.prj[i];
  if (jac && l < NX)
    for (int r = 0; r < nr; ++r) jac[((size_t)t * nr + r) * NX + l] = S.J[r][l];
}

}  // namespace

extern "C" int harp_arm_reproj_ik_frames_per_block(void) { return kFramesPerBlock; }

extern "C" int harp_arm_reproj_ik(const harp_tree_model* m, const float* betas, const float* cam, const float* targets, const float* weights,
                                  const float* depth_weights, const float* prior, const float* wrist_prior, const float* z_prior, int N,
                                  const harp_arm_reproj_ik_options* opt, float* in_pose, float* trans, float* cost, int32_t* status,
                                  float* proj, float* jac, hipStream_t stream) {
  if (!m || !opt || !betas || !cam || !targets || !in_pose || !trans || !cost || !status || N <= 0 || opt->iters < 0) return HARP_ERR_ARG;
  if (m->n_pose_in != NIN || m->NB < NSB || m->NB > MAXB || m->NJ < 1 || m->NJ > MAXJ || m->NV < 1) return HARP_ERR_ARG;
  if (m->n_joints_out < 1 || m->n_joints_out > NO || m->center_joint < 0 || m->center_joint >= m->NJ) return HARP_ERR_ARG;
  const float nonneg[4] = {opt->lambda0, opt->pose_prior_weight, opt->wrist_prior_weight, opt->z_prior_weight};
  for (float v : nonneg)
    if (!(v >= 0.f) || isinf(v)) return HARP_ERR_ARG;
  if (!(opt->focal > 0.f) || isinf(opt->focal) || opt->S <= 0) return HARP_ERR_ARG;
  if (!z_prior && opt->z_prior_weight != 0.f) return HARP_ERR_ARG;
  const ArInputs in = {betas, cam, targets, weights, depth_weights, prior, wrist_prior, z_prior};
  hipLaunchKernelGGL(arm_reproj_ik_kernel, dim3((unsigned)N), dim3(64), 0, stream, *m, in, *opt, in_pose, trans, cost, status, proj, jac);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
