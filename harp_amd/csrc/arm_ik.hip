// Batched inverse kinematics of the SMPL-X right arm for gfx950 (ops.arm_ik; playback Motion.from_arm_keypoints): up to 22 3-D
// keypoints per frame (the wrist, the five fingers root to tip, the elbow) -> the rows [rot | wrist | pose | trans] that harp_lbs_tree_fwd
// turns back into those joints.  Nothing in the reference does this.  The keypoint counterpart of csrc/arm_vertex_fit.hip (§28) and the tree
// counterpart of csrc/ik.hip (§24): the iteration is csrc/ik.hip's, the slot tables of the tree are tree_slots_body.h's and the solve is
// lm_solve_body.h's, both written out here because this kernel measured slower through either shared routine, beyond its run-to-run
// spread; the forward is csrc/lbs_tree.hip's (lt::rod_fwd, its tangent lt::rod_jvp, the level-parallel chain), so the
// solver and the renderer cannot disagree.
//
// harp_arm_ik: T independent Levenberg-Marquardt solves in ONE launch, one wave (= one workgroup) per frame, 54 unknowns
// x = [rot 3 | wrist 3 | pose 45 | trans 3] and 3 n_out <= 66 residuals (include/harp_hip.h states the contract).
//
//   prologue     once per frame, what no unknown moves: the tree (parents, depths, the joint each input row drives), for every driven joint
//                but the root the list of joints below it ("slots", parents before children; spos[row][joint] finds a joint's slot), the
//                rotations of the joints nothing drives (their pose mean is NOT zero in general: the wrist's own ancestors 17 and 19 turn the
//                elbow), the rest joints at this shape, and for every output row that is a skinned vertex q0 = v_template + its shape rows +
//                the constant corrective rows of the undriven joints.
//   forward      lanes 0..16 one Rodrigues each, the chain level by level (lane = joint), A_j = [G_j | t_j - G_j J_j], the posed vertex
//                rows (q0 + the 16 x 9 driven corrective rows: a lane per (coordinate, joint), so the 144 loads of a coordinate are one
//                round trip, then summed joint by joint), their blended 3x4 transforms over ALL NJ joints (the rows' skin weights are
//                staged in LDS by the prologue), then lane i < 3 n_out one output coordinate (rows from the model's joint_src), its
//                residual and its share of the cost; a butterfly sum (fixed order).
//   Jacobian     lane i < 54 owns column i.
//                  root    rotation about the pelvis followed by the subtraction of the posed centre is a rotation of the centre-relative
//                          output: dj = (dR_0 R_0^T)(j - trans) for every row, tips and elbow included
//                  wrist,  the column walks its slots ([dG | dt] of every joint below, kept in LDS); a tree row takes its joint's dt, a
//                  finger  vertex row T_v[:3,:3] (posedirs[v, the joint's 9 rows] . dR) + sum over the slots of w_vj (dG_j (q - J_j) + dt_j);
//                          minus d(posed centre).  A row whose joint is in none of the column's slots (the elbow: an ancestor of the
//                          centre) gets exactly 0.
//                  trans   the identity.
//                J (66 x 54, rows past 3 n_out zero, row stride 55: consecutive lanes and consecutive rows fall in different banks) in LDS.
//   normal eqs., solve, accept: csrc/ik.hip's (lm::jacobi_scale, lm::damped), lane i = row i; a frozen wrist column has A_ii = 1, zeros elsewhere, g_i = 0.
// `iters` iterations whatever happens: no early exit, every branch that holds a barrier is uniform over the wave.  No workspace, no
// allocation, no synchronisation, no atomics: the launch can be captured and a repeated call gives the same bits.
#include "lm_solve_body.h"
#include "tree_slots_body.h"                                           // (NIN, MAXSLOT, NOSLOT, UNSET; lbs_tree_body.h)

#include <math.h>

namespace {

using namespace lt;

constexpr int NX = 54;                  // unknowns per frame
constexpr int NO = HARP_ARM_IK_MAX_JOINTS;
constexpr int NR = 3 * NO;              // residual rows held (those past 3 n_joints_out stay zero)
constexpr int LD = 55;                  // row stride of J and A in LDS (odd)
constexpr int XW = 3, XP = 6, XT = 51;  // first wrist / finger / trans column
constexpr int NSB = 10;                 // shape coefficients given (the model's other NB - 10 are zero)
constexpr int kAkFramesPerBlock = 1;    // one wave per workgroup, as csrc/ik.hip: LDS (48 KiB a frame: three on a CU) bounds the frames in flight on a CU

struct AkLds {
  // the model's structure and what no unknown moves (prologue)
  int par[MAXJ], depth[MAXJ], drv[NIN]; // drv[row] = the joint that row of in_pose drives
  int soff[NIN + 1];                    // row's slots: soff[row] .. soff[row + 1] (row 0 has none)
  int sj[MAXSLOT], sp[MAXSLOT];         // a slot's joint; its parent's slot, or -1 for the column's own joint
  int jsrc[NO];                         // the model's joint_src
  int vrow[NO], nv;                     // the output rows that are skinned vertices, in order
  int maxd, bad;
  unsigned char spos[NIN][MAXJ], driven[MAXJ];      // spos[row][j]: the slot of joint j among the row's, or NOSLOT
  float beta[NSB], prior[NX];           // prior by column (zero outside the wrist and finger columns)
  float w[NO], tgt[NR];                 // zero for an unused joint
  float q0[NO][3];                      // a vertex row's rest position at this shape with the constant correctives
  float sW[NO][MAXJ + 1];               // a vertex row's skin weights (odd stride)
  // the point and its chain (every evaluation)
  float x[NX];
  float R[MAXJ][9], G[MAXJ][12], Aj[MAXJ][12], Jr[MAXJ][3];
  float pmv[NIN][9];                    // R - I of a driven joint: the corrective rows that move
  float cen[3];
  float q[NO][3], Tm[NO][12];           // a vertex row's posed position and blended transform
  // at x only
  float res[NR], jnt[NR];
  float dR[NIN * 3][9], Om[3][9];       // d R / d x[col];  dR_0/d rot[c] R_0^T
  float J[NR][LD];                      // d joints (metres, output order) / d x
  union {                               // (an evaluation is over before the normal matrix is formed, and begins after the solves)
    float A[NX][LD];                    // normal matrix, then its scaled Cholesky factor in the lower triangle
    struct {
      float dGt[MAXSLOT][3][12];        // [dG_j | dt_j] of a slot's joint by the column's three axes
      float qp[NO * 3][NIN - 1];        // a vertex row's corrective sum joint by joint (one lane per (coordinate, joint): one round trip)
    } e;
  } u;
};
static_assert(sizeof(AkLds) == 49216, "three frames on a CU rest on this size (DESIGN.md §29)");

__device__ __forceinline__ void joint_aa(const harp_tree_model& M, const AkLds& S, int row, float aa[3]) {
  const int j = S.drv[row];
#pragma unroll
  for (int c = 0; c < 3; ++c) aa[c] = M.pose_mean[3 * j + c] + S.x[3 * row + c];            // (lbs_tree_body.h:90)
}

// the model vertex of output row k (joint_src[k] < 0), held inside the model
__device__ __forceinline__ int row_vertex(const harp_tree_model& M, int src) { return min(max(-src - 1, 0), M.NV - 1); }

// Once per frame.  Sets S.bad when the model is not of the shape this kernel's tables hold.
__device__ void ak_prologue(const harp_tree_model& M, AkLds& S, int l, const float* __restrict__ beta_row, int n_out) {
  const int NJ = M.NJ, NB = M.NB, NP = (NJ - 1) * 9;
  if (l < NJ) S.par[l] = min(M.parents[l], l - 1);                     // (parents[j] < j: every walk up the tree ends)
  if (l < NIN) S.drv[l] = -1;
  if (l < NSB) S.beta[l] = beta_row[l];
  if (l < NO) S.jsrc[l] = (l < n_out) ? M.joint_src[l] : 0;
  for (int i = l; i < NIN * MAXJ; i += 64) (&S.spos[0][0])[i] = NOSLOT;
  for (int i = l; i < NR * LD; i += 64) (&S.J[0][0])[i] = 0.f;
  for (int i = l; i < NR; i += 64) { S.res[i] = 0.f; S.jnt[i] = 0.f; }
  if (l == 0) S.bad = 0;
  __syncthreads();
  if (l < NJ) {
    const int src = M.pose_src[l];
    const bool drn = src >= 0 && src < NIN;
    S.driven[l] = drn ? 1 : 0;
    if (drn) S.drv[src] = l;
    int d = 0;
    for (int q = S.par[l]; q >= 0; q = S.par[q]) ++d;
    S.depth[l] = d;
  }
  __syncthreads();
  if (l == 0) {
    int md = 0, bad = (S.drv[0] != 0);
    for (int j = 0; j < NJ; ++j) md = max(md, S.depth[j]);
    for (int r = 1; r < NIN; ++r) bad |= (S.drv[r] <= 0);
    S.maxd = md;
    S.bad = bad;
    int nv = 0;
    for (int k = 0; k < n_out; ++k)
      if (S.jsrc[k] < 0) S.vrow[nv++] = k;
    S.nv = nv;
  }
  __syncthreads();
  if (S.bad) return;
  for (int i = l; i < S.nv * NJ; i += 64) {                            // the vertex rows' skin weights
    const int k = S.vrow[i / NJ], j = i % NJ;
    S.sW[k][j] = M.weights[(size_t)row_vertex(M, S.jsrc[k]) * NJ + j];
  }
  if (l < NJ)                                                          // is joint l a row's joint or below it
    for (int row = 1; row < NIN; ++row) {
      const int jq = S.drv[row];
      int a = l;
      while (a > jq) a = S.par[a];
      if (a == jq) S.spos[row][l] = UNSET;
    }
  __syncthreads();
  if (l == 0) {
    int n = 0;
    S.soff[0] = 0;
    for (int row = 0; row < NIN; ++row) {
      for (int j = 0; j < NJ; ++j) n += (S.spos[row][j] == UNSET);
      S.soff[row + 1] = n;
    }
    if (n > MAXSLOT) S.bad = 1;
  }
  __syncthreads();
  if (S.bad) return;
  if (l >= 1 && l < NIN) {                                             // the row's slots, parents before children (parents[j] < j)
    const int jq = S.drv[l];
    int s = S.soff[l];
    for (int j = jq; j < NJ; ++j) {
      if (S.spos[l][j] != UNSET) continue;
      S.sj[s] = j;
      S.sp[s] = (j == jq) ? -1 : (int)S.spos[l][S.par[j]];
      S.spos[l][j] = (unsigned char)s;
      ++s;
    }
  }
  if (l < NJ && !S.driven[l]) {                                        // the joints nothing drives: their rotation is the model's
    const float aa[3] = {M.pose_mean[3 * l], M.pose_mean[3 * l + 1], M.pose_mean[3 * l + 2]};
    float R[9];
    rod_fwd(aa, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) S.R[l][k] = R[k];
  }
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
      if (S.driven[j]) continue;
      for (int m = 0; m < 9; ++m) {
        const float p = S.R[j][m] - ((m == 0 || m == 4 || m == 8) ? 1.f : 0.f);
        if (p != 0.f) q += M.posedirs[e * NP + (j - 1) * 9 + m] * p;   // (rod_fwd(0) = I exactly: a zero mean costs no load)
      }
    }
    S.q0[k][c] = q;
  }
  __syncthreads();
}

// The joints, residuals and cost at xl (lane l's unknown); JAC: also S.jnt, S.res and the Jacobian S.J.  Returns C(x), the same bits in every lane.
__device__ float ak_eval(const harp_tree_model& M, AkLds& S, int l, float xl, bool JAC, int n_out, float pose_w, float wrist_w) {
  const int NJ = M.NJ, NP = (NJ - 1) * 9, cj = M.center_joint;
  if (l < NX) S.x[l] = xl;
  __syncthreads();
  if (l < NIN) {
    float aa[3], R[9];
    joint_aa(M, S, l, aa);
    rod_fwd(aa, R);
    const int j = S.drv[l];
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
  const int maxd = S.maxd;
  for (int d = 1; d <= maxd; ++d) {
    __syncthreads();
    if (l < NJ && S.depth[l] == d) {
      const int j = l, p = S.par[j];
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
    const float* pj = M.posedirs + ((size_t)row_vertex(M, S.jsrc[k]) * 3 + c) * NP + (S.drv[row] - 1) * 9;
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
  float part = 0.f;
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
    v = (v - S.cen[c]) + S.x[XT + c];
    const float wk = S.w[k];
    const float r = (wk > 0.f) ? (v - S.tgt[i]) : 0.f;                 // (S.tgt is 0 for an unused joint, S.w too)
    part += wk * r * r;
    if (JAC) { S.jnt[i] = v; S.res[i] = r; }
  }
  if (l >= XP && l < XT) {
    const float d = xl - S.prior[l];
    part += pose_w * d * d;
  } else if (l >= XW && l < XP) {
    const float d = xl - S.prior[l];
    part += wrist_w * d * d;
  }
  const float cost = __shfl(wave_sum(part), 0, 64);
  if (!JAC) return cost;

  // ---- Jacobian columns
  if (l < 3) {                                                         // the root: Omega_c = dR_0 R_0^T
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k)
        S.Om[l][r * 3 + k] = S.dR[l][r * 3] * S.R[0][k * 3] + S.dR[l][r * 3 + 1] * S.R[0][k * 3 + 1] + S.dR[l][r * 3 + 2] * S.R[0][k * 3 + 2];
  } else if (l < XT) {                                                 // a wrist or finger column down its slots
    const int row = l / 3, c = l % 3;
    for (int s = S.soff[row]; s < S.soff[row + 1]; ++s) {
      const int j = S.sj[s], ps = S.sp[s], p = S.par[j];
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
    const int row = l / 3, c = l % 3, s0 = S.soff[row], s1 = S.soff[row + 1];
    const int sc = S.spos[row][cj];
    float dc[3] = {0.f, 0.f, 0.f};                                     // d (posed centre): zero when the centre is the column's joint or above it
    if (sc != NOSLOT) { dc[0] = S.u.e.dGt[sc][c][3]; dc[1] = S.u.e.dGt[sc][c][7]; dc[2] = S.u.e.dGt[sc][c][11]; }
#pragma unroll 1
    for (int k = 0; k < n_out; ++k) {
      const int src = S.jsrc[k];
      float d[3] = {0.f, 0.f, 0.f};
      if (src >= 0) {
        const int s = S.spos[row][min(src, NJ - 1)];
        if (s != NOSLOT) { d[0] = S.u.e.dGt[s][c][3]; d[1] = S.u.e.dGt[s][c][7]; d[2] = S.u.e.dGt[s][c][11]; }
      } else {
        const int v = row_vertex(M, src);
        const float* Tm = S.Tm[k];
        const float* q = S.q[k];
        float dv[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {                               // the row's correctives of this joint's 9 pose_map entries
          const float* pd = M.posedirs + ((size_t)v * 3 + cc) * NP + (S.drv[row] - 1) * 9;
          float acc = 0.f;
#pragma unroll
          for (int m = 0; m < 9; ++m) acc += pd[m] * S.dR[l][m];
          dv[cc] = acc;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) d[r] = Tm[r * 4] * dv[0] + Tm[r * 4 + 1] * dv[1] + Tm[r * 4 + 2] * dv[2];
#pragma unroll 1
        for (int s = s0; s < s1; ++s) {
          const int j = S.sj[s];
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
  __syncthreads();
  return cost;
}

__global__ void __launch_bounds__(64) arm_ik_kernel(const harp_tree_model M, const float* __restrict__ betas, int betas_per_frame,
                                                    const float* __restrict__ targets, const float* __restrict__ weights,
                                                    const float* __restrict__ prior, const float* __restrict__ wrist_prior, int iters,
                                                    float lambda, float pose_w, float wrist_w, int solve_wrist, float* __restrict__ in_pose,
                                                    float* __restrict__ trans, float* __restrict__ cost, int32_t* __restrict__ status,
                                                    float* __restrict__ joints, float* __restrict__ jac) {
  __shared__ AkLds S;
  const int t = blockIdx.x, l = threadIdx.x;                           // (the grid is exactly T workgroups of one wave)
  const int n_out = M.n_joints_out, nr = 3 * n_out;
  const int lc = min(l, NX - 1);
  float xl = 0.f;
  if (l < XT) xl = in_pose[(size_t)t * XT + l];
  else if (l < NX) xl = trans[(size_t)t * 3 + (l - XT)];
  if (l < NX) {
    float p = 0.f;
    if (l >= XP && l < XT) p = prior ? prior[(size_t)t * 45 + (l - XP)] : 0.f;
    else if (l >= XW && l < XP) p = wrist_prior ? wrist_prior[(size_t)t * 3 + (l - XW)] : 0.f;
    S.prior[l] = p;
  }
  bool used = false;
  if (l < NO) {
    float w = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (l < n_out) {
      w = weights ? weights[(size_t)t * n_out + l] : 1.0f;
      const float* tg = targets + ((size_t)t * n_out + l) * 3;
      t0 = tg[0]; t1 = tg[1]; t2 = tg[2];
      used = (w > 0.f) && isfinite(t0) && isfinite(t1) && isfinite(t2);
    }
    S.w[l] = used ? w : 0.f;
    S.tgt[3 * l] = used ? t0 : 0.f; S.tgt[3 * l + 1] = used ? t1 : 0.f; S.tgt[3 * l + 2] = used ? t2 : 0.f;
  }
  const bool solve = __popcll(__ballot(used)) >= 3;
  ak_prologue(M, S, l, betas + (betas_per_frame ? (size_t)t * NSB : 0), n_out);
  if (S.bad) {                                                         // a tree these tables do not hold: nothing is solved or written
    if (l == 0) { cost[2 * (size_t)t] = 0.f; cost[2 * (size_t)t + 1] = 0.f; status[t] = -2; }
    return;
  }

  const bool pose_lane = l >= XP && l < XT, wrist_lane = l >= XW && l < XP;
  const bool frozen = wrist_lane && !solve_wrist;
  const float pw = pose_lane ? pose_w : (wrist_lane ? wrist_w : 0.f);  // this lane's prior weight
  float C = 0.f, C0 = 0.f;
  int n_acc = 0;
  bool fresh = true;                                                   // J and the residual are to be evaluated at xl
#pragma unroll 1
  for (int it = 0;; ++it) {
    if (fresh) {
      C = ak_eval(M, S, l, xl, true, n_out, pose_w, wrist_w);
      if (it == 0) C0 = C;
      fresh = false;
    }
    if (it == iters) break;
    // this lane's weighted column, gradient entry and row of A
    float Jw[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) Jw[k] = S.w[k / 3] * S.J[k][lc];
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < NR; ++k) g += Jw[k] * S.res[k];
    g += pw * (xl - S.prior[lc]);
    if (frozen) g = 0.f;
    float diag = 1.f;
#pragma unroll 1
    for (int j = 0; j < NX; ++j) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < NR; ++k) a += Jw[k] * S.J[k][j];
      const bool fj = !solve_wrist && j >= XW && j < XP;
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
#pragma unroll 1
    for (int j = 0; j < NX; ++j) {                                     // lm::solve's factorisation, column j
      const float sj = __shfl(s, j, 64);
      float v = 0.f;
      if (l >= j && l < NX) {
        v = (l == j) ? 1.0f : S.u.A[l][j] * s * sj;
#pragma unroll 6
        for (int c = 0; c < j; ++c) v -= S.u.A[l][c] * S.u.A[j][c];
      }
      const float piv = __shfl(v, j, 64);
      ok = ok && (piv > 0.f) && isfinite(piv);
      const float ljj = sqrtf(piv);
      if (l >= j && l < NX) S.u.A[l][j] = (l == j) ? ljj : v / ljj;
      __syncthreads();
    }
    float b = (l < NX) ? -g * s : 0.f, y = 0.f, z = 0.f;
#pragma unroll 1
    for (int j = 0; j < NX; ++j) {                                     // L y = b
      const float yj = __shfl(b, j, 64) / S.u.A[j][j];
      if (l == j) y = yj;
      if (l > j && l < NX) b -= S.u.A[l][j] * yj;
    }
#pragma unroll 1
    for (int j = NX - 1; j >= 0; --j) {                                // L^T z = y
      const float zj = __shfl(y, j, 64) / S.u.A[j][j];
      if (l == j) z = zj;
      if (l < j) y -= S.u.A[j][l] * zj;
    }
    const float xn = (l < NX) ? xl + z * s : 0.f;
    const float Cn = ak_eval(M, S, l, xn, false, n_out, pose_w, wrist_w);
    const bool accept = __builtin_amdgcn_readfirstlane((int)(ok && solve && (Cn < C))) != 0;       // (a NaN is not less)
    if (accept) {
      xl = xn;
      lambda = lm::damped(lambda, true);
      ++n_acc;
      fresh = true;
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
    status[t] = solve ? n_acc : -1;
  }
  if (joints)
    for (int i = l; i < nr; i += 64) joints[(size_t)t * nr + i] = S.jnt[i] * 1000.0f;
  if (jac && l < NX)
    for (int r = 0; r < nr; ++r) jac[((size_t)t * nr + r) * NX + l] = S.J[r][l];
}

}  // namespace

extern "C" int harp_arm_ik_frames_per_block(void) { return kAkFramesPerBlock; }

extern "C" int harp_arm_ik(const harp_tree_model* m, const float* betas, const float* targets, const float* weights, const float* prior,
                           const float* wrist_prior, int T, const harp_arm_ik_options* opt, float* in_pose, float* trans, float* cost,
                           int32_t* status, float* joints, float* jac, hipStream_t stream) {
  if (!m || !opt || !betas || !targets || !in_pose || !trans || !cost || !status || T <= 0 || opt->iters < 0) return HARP_ERR_ARG;
  if (m->n_pose_in != NIN || m->NB < NSB || m->NB > MAXB || m->NJ < 1 || m->NJ > MAXJ || m->NV < 1) return HARP_ERR_ARG;
  if (m->n_joints_out < 1 || m->n_joints_out > NO || m->center_joint < 0 || m->center_joint >= m->NJ) return HARP_ERR_ARG;
  const float nonneg[3] = {opt->lambda0, opt->pose_prior_weight, opt->wrist_prior_weight};
  for (float v : nonneg)
    if (!(v >= 0.f) || isinf(v)) return HARP_ERR_ARG;
  hipLaunchKernelGGL(arm_ik_kernel, dim3((unsigned)T), dim3(64), 0, stream, *m, betas, opt->betas_per_frame != 0, targets, weights, prior,
                     wrist_prior, opt->iters, opt->lambda0, opt->pose_prior_weight, opt->wrist_prior_weight, opt->solve_wrist != 0, in_pose,
                     trans, cost, status, joints, jac);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
