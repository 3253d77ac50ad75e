// Batched 2.5-D reprojection inverse kinematics of the MANO hand for gfx950 (harp_amd/playback/motion.py Motion.from_image_keypoints,
// DESIGN.md §30): 21 image keypoints per problem, in pixels, optionally with a wrist-relative depth per joint -> the rows
// [rot | pose | trans] that harp_lbs_mano_fwd and the player's camera turn back into those pixels.  Nothing in the reference does this
// (its change_pose takes another sequence's parameters), so this header cites the model it inverts: csrc/lbs.hip, csrc/lbs_body.h and
// the camera of utils/visualize.py:268-271 (R = diag(-1,-1,1), T = (-cam1, -cam2, 2 focal / (S cam0 + 1e-9))) seen through the
// rasteriser's pixel centres (column i has its centre at u = i + 0.5).
//
// harp_mano_reproj_ik: N independent Levenberg-Marquardt solves in ONE launch, one wave (= one workgroup) per problem; the iteration is
// harp_mano_ik's (csrc/ik.hip): the same joints forward and tangent push, and lm_solve_body.h's solve, written out in both files because
// either kernel measured slower through shared routines, beyond its run-to-run spread.  Per problem 51
// unknowns x = [rot 3 | pose 45 | trans 3] and 63 rows (u_k, v_k, d_k):
//   Z_k = j_k.z + t_z, u_k = S/2 + focal (j_k.x + cam1) / Z_k, v_k = S/2 + focal (j_k.y + cam2) / Z_k, d_k = j_k.z - j_0.z
// with j(x) the 21 joints of harp_lbs_mano_fwd in metres (rodrigues_fwd, rodrigues_jvp, parent_of, c_tips, c_reorder from lbs_body.h), and the cost
//   C = sum_k w_k [(u_k - u^_k)^2 + (v_k - v^_k)^2] + sum_{k>=1} wz_k (d_k - d^_k)^2 + w_pose sum_i (pose_i - prior_i)^2 + w_z (trans_z - z_prior)^2.
//
//   forward      as csrc/ik.hip up to the 63 joint coordinates; then lane k < 21 projects joint k: its Z, its three rows, their residuals
//                and its share of the cost (a butterfly sum over the wave, fixed order), and for the Jacobian focal / Z_k and
//                focal (j + cam) / Z_k^2.  A used joint at Z_k <= 1e-3 marks the point as behind the camera.
//   Jacobian     lane i < 48 pushes the tangent of ITS axis-angle component into all 21 joints (as csrc/ik.hip; dense in the tips), lanes
//                48..50 hold the identity columns of trans; every lane then turns the 63 3-D entries of its own column into (u, v, d) rows
//                — du = focal/Z dj.x - focal (j.x + cam1)/Z^2 dj.z, dd = dj_k.z - dj_0.z with its own wrist entry — in place in LDS.
//   normal eqs., solve, accept: csrc/ik.hip's (lm::jacobi_scale, lm::damped), with the row weights (w_k, w_k, wz_k) and the two priors on the diagonal; a candidate
//                behind the camera is a rejection.
// `iters` iterations whatever happens: no early exit, every branch is uniform over the wave.  No workspace, no allocation, no
// synchronisation, no atomics: the launch can be captured and a repeated call gives the same bits.
// A problem with fewer than 4 used pixel joints (status -1) or with a used joint behind the camera at its input (status -2) runs the same
// instructions and writes nothing back but cost, status and the optional proj / jac at its input.  An unused target is tested and never
// enters arithmetic; a joint that is not pixel-used AND at Z_k <= 1e-3 gets u = v = 0 and zero u / v rows in jac (nothing to divide by).
#include "lbs_body.h"
#include "lm_solve_body.h"
#include "harp_hip.h"

#include <math.h>

namespace {

using namespace lb;

constexpr int NX = 51;                 // unknowns per frame
constexpr int NR = 63;                 // residuals per frame
constexpr int kFramesPerBlock = 1;     // one wave per workgroup: LDS (26.7 KiB a problem), not registers, bounds the problems in flight on a
                                       // CU, and single-problem workgroups waste none of it
constexpr float kZMin = 1e-3f;         // a used joint nearer than this (metres along the view axis) is behind the camera

struct RpLds {
  float J[NR][NX];                     // d joints (metres, output order) / d x while a column is pushed, then d (u, v, d) rows / d x
  float A[NX][NX];                     // normal matrix, then its scaled Cholesky factor in the lower triangle
  float x[NX + 1];                     // the point being evaluated
  float R[NJ][9], G[NJ][12], Jr[NJ][3];
  float vs[5][3], vp[5][3], Tk[5][12], pm[NP];
  float W[NR], res[NR], jnt[NR], prj[NR], tgt[NR], beta[NB];       // W: the row weights (w_k, w_k, wz_k), 0 for an unused row
  float cam[3];                        // (t_z, cam1, cam2)
  int inv[21];                         // inverse of c_reorder: model joint / tip -> output joint
  // What an evaluation WITH the Jacobian hands from its projecting lanes to its column lanes lives in A's first 63 floats: A is dead then
  // (every iteration rebuilds it from J before it reads it; such an evaluation runs before the first iteration or after a step's solves).
  // Those 252 bytes, and the priors' centres kept in their lanes' registers, keep six problems within a CU's 160 KiB.
  __device__ float* iz() { return &A[0][0]; }              // [21] focal / Z_k
  __device__ float* px() { return &A[0][0] + 21; }         // [21] focal (j_k.x + cam1) / Z_k^2
  __device__ float* py() { return &A[0][0] + 42; }         // [21] focal (j_k.y + cam2) / Z_k^2
};
static_assert(sizeof(RpLds) == 27296, "six problems within a CU's 160 KiB rest on this size (DESIGN.md §30)");

__device__ __forceinline__ void joint_aa(const harp_mano_model& M, const RpLds& S, int j, float aa[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p = S.x[3 * j + c];
    aa[c] = (j == 0) ? p : (M.hands_mean[3 * (j - 1) + c] + p);       // (csrc/lbs.hip:35)
  }
}

// The joints, projected rows and cost at xl (lane l's unknown); JAC: also S.res, S.prj and the Jacobian S.J.  Returns C(x), the same bits
// in every lane; behind: a used pixel joint at Z <= kZMin (uniform over the wave).  pw, pc: this lane's diagonal of P (the pose prior's
// weight in lanes 3..47, trans_z's in lane 50, else 0) and what it pulls towards.
template <bool JAC>
__device__ float rp_eval(const harp_mano_model& M, RpLds& S, int l, float xl, float pw, float pc, float focal, float half, bool& behind) {
  if (l < NX) S.x[l] = xl;
  __syncthreads();
  if (l < NJ) {
    float aa[3], R[9];
    joint_aa(M, S, l, aa);
    rodrigues_fwd(aa, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      S.R[l][k] = R[k];
      if (l > 0) S.pm[(l - 1) * 9 + k] = R[k] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
    }
  }
  __syncthreads();
  if (l == 0) {
    for (int k = 0; k < 9; ++k) S.G[0][(k / 3) * 4 + (k % 3)] = S.R[0][k];
    for (int r = 0; r < 3; ++r) S.G[0][r * 4 + 3] = S.Jr[0][r];
  }
  __syncthreads();
  if (l < 5) {                                                         // one finger per lane, as lbs_joints_kernel
    for (int lev = 0; lev < 3; ++lev) {
      const int j = 3 * l + 1 + lev, p = parent_of(j);
      const float rel[3] = {S.Jr[j][0] - S.Jr[p][0], S.Jr[j][1] - S.Jr[p][1], S.Jr[j][2] - S.Jr[p][2]};
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
          S.G[j][r * 4 + c] = S.G[p][r * 4] * S.R[j][c] + S.G[p][r * 4 + 1] * S.R[j][3 + c] + S.G[p][r * 4 + 2] * S.R[j][6 + c];
        S.G[j][r * 4 + 3] = S.G[p][r * 4] * rel[0] + S.G[p][r * 4 + 1] * rel[1] + S.G[p][r * 4 + 2] * rel[2] + S.G[p][r * 4 + 3];
      }
    }
  }
  if (l < 15) {                                                        // posed tip coordinates: rest + pose correctives
    const int k = l / 3, c = l % 3;
    const float* pd = M.posedirs + ((size_t)c_tips[k] * 3 + c) * NP;
    float acc = S.vs[k][c];
    for (int m = 0; m < NP; ++m) acc += pd[m] * S.pm[m];
    S.vp[k][c] = acc;
  }
  __syncthreads();
  if (l < 60) {                                                        // T_k = sum_j w_kj [G_j | t_j - G_j J_j]
    const int k = l / 12, e = l % 12, r = e / 4, c = e % 4;
    const float* wk = M.weights + (size_t)c_tips[k] * NJ;
    float acc = 0.f;
    for (int j = 0; j < NJ; ++j) {
      const float a = (c < 3) ? S.G[j][e]
                              : S.G[j][r * 4 + 3] - (S.G[j][r * 4] * S.Jr[j][0] + S.G[j][r * 4 + 1] * S.Jr[j][1] + S.G[j][r * 4 + 2] * S.Jr[j][2]);
      acc += wk[j] * a;
    }
    S.Tk[k][e] = acc;
  }
  __syncthreads();
  float part = 0.f;
  if (l < NR) {
    const int k = l / 3, c = l % 3, src = c_reorder[k];
    float v;
    if (src < NJ) {
      v = S.G[src][c * 4 + 3];
    } else {
      const float* Tm = S.Tk[src - NJ];
      const float* q = S.vp[src - NJ];
      v = Tm[c * 4] * q[0] + Tm[c * 4 + 1] * q[1] + Tm[c * 4 + 2] * q[2] + Tm[c * 4 + 3];
    }
    S.jnt[l] = v + S.x[48 + c];
  }
  __syncthreads();
  bool bad = false;
  if (l < 21) {                                                        // joint l through the camera: its rows (u, v, d)
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
      S.iz()[l] = iz; S.px()[l] = proj ? iz * jx / Z : 0.f; S.py()[l] = proj ? iz * jy / Z : 0.f;
    }
  }
  part += pw * (xl - pc) * (xl - pc);
  behind = __any(bad) != 0;
  const float cost = __shfl(wave_sum(part), 0, 64);
  if (!JAC) return cost;

  // ---- Jacobian columns
  if (l < 48) {
    const int q = l / 3, c = l % 3;
    float aa[3], dR[9];
    joint_aa(M, S, q, aa);
    rodrigues_jvp(aa, c, dR);
    float dtip[5][3];
#pragma unroll
    for (int k = 0; k < 5; ++k) dtip[k][0] = dtip[k][1] = dtip[k][2] = 0.f;
    if (q > 0) {                                                       // the tips' pose correctives of this joint's 9 pose_map entries
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        float dv[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
          const float* pd = M.posedirs + ((size_t)c_tips[k] * 3 + cc) * NP + (q - 1) * 9;
          float acc = 0.f;
#pragma unroll
          for (int m = 0; m < 9; ++m) acc += pd[m] * dR[m];
          dv[cc] = acc;
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) dtip[k][r] += S.Tk[k][r * 4] * dv[0] + S.Tk[k][r * 4 + 1] * dv[1] + S.Tk[k][r * 4 + 2] * dv[2];
      }
    } else {                                                           // the root's own skinning share: d A_0 = [dR | -dR J_0]
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float wk = M.weights[(size_t)c_tips[k] * NJ];
        const float d[3] = {S.vp[k][0] - S.Jr[0][0], S.vp[k][1] - S.Jr[0][1], S.vp[k][2] - S.Jr[0][2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) dtip[k][r] += wk * (dR[r * 3] * d[0] + dR[r * 3 + 1] * d[1] + dR[r * 3 + 2] * d[2]);
      }
    }
    {
      const int o = S.inv[0] * 3;                                      // the root joint's position is the rest joint: no derivative
      S.J[o][l] = 0.f; S.J[o + 1][l] = 0.f; S.J[o + 2][l] = 0.f;
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      float pG[9], pt[3] = {0.f, 0.f, 0.f};
      bool pact = (q == 0);
#pragma unroll
      for (int m = 0; m < 9; ++m) pG[m] = dR[m];
#pragma unroll
      for (int lev = 0; lev < 3; ++lev) {
        const int j = 3 * f + 1 + lev, p = parent_of(j);
        float cG[9], ct[3] = {0.f, 0.f, 0.f};
        bool act = false;
#pragma unroll
        for (int m = 0; m < 9; ++m) cG[m] = 0.f;
        if (j == q) {                                                  // G_q = G_p R_q: d = G_p dR, the position does not move
          act = true;
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc)
              cG[r * 3 + cc] = S.G[p][r * 4] * dR[cc] + S.G[p][r * 4 + 1] * dR[3 + cc] + S.G[p][r * 4 + 2] * dR[6 + cc];
        } else if (pact) {                                             // below the moved joint: d G_j = d G_p R_j, d t_j = d G_p rel_j + d t_p
          act = true;
          const float rel[3] = {S.Jr[j][0] - S.Jr[p][0], S.Jr[j][1] - S.Jr[p][1], S.Jr[j][2] - S.Jr[p][2]};
#pragma unroll
          for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc)
              cG[r * 3 + cc] = pG[r * 3] * S.R[j][cc] + pG[r * 3 + 1] * S.R[j][3 + cc] + pG[r * 3 + 2] * S.R[j][6 + cc];
            ct[r] = pG[r * 3] * rel[0] + pG[r * 3 + 1] * rel[1] + pG[r * 3 + 2] * rel[2] + pt[r];
          }
        }
        const int o = S.inv[j] * 3;
        S.J[o][l] = ct[0]; S.J[o + 1][l] = ct[1]; S.J[o + 2][l] = ct[2];
        if (act) {                                                     // d A_j = [dG | dt - dG J_j] weighted into every tip
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            const float wk = M.weights[(size_t)c_tips[k] * NJ + j];
            const float d[3] = {S.vp[k][0] - S.Jr[j][0], S.vp[k][1] - S.Jr[j][1], S.vp[k][2] - S.Jr[j][2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) dtip[k][r] += wk * (cG[r * 3] * d[0] + cG[r * 3 + 1] * d[1] + cG[r * 3 + 2] * d[2] + ct[r]);
          }
        }
#pragma unroll
        for (int m = 0; m < 9; ++m) pG[m] = cG[m];
        pt[0] = ct[0]; pt[1] = ct[1]; pt[2] = ct[2];
        pact = act;
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int o = S.inv[NJ + k] * 3;
      S.J[o][l] = dtip[k][0]; S.J[o + 1][l] = dtip[k][1]; S.J[o + 2][l] = dtip[k][2];
    }
  } else if (l < NX) {
    for (int r = 0; r < NR; ++r) S.J[r][l] = (r % 3 == l - 48) ? 1.f : 0.f;
  }
  __syncthreads();                                                     // (S.iz, S.px, S.py of the projecting lanes)
  if (l < NX) {                                                        // this lane's own column: 3-D entries -> (u, v, d) rows, in place
    const float dz0 = S.J[2][l];                                       // (the wrist is output joint 0)
    for (int k = 0; k < 21; ++k) {
      const float dx = S.J[3 * k][l], dy = S.J[3 * k + 1][l], dz = S.J[3 * k + 2][l];
      S.J[3 * k][l] = S.iz()[k] * dx - S.px()[k] * dz;
      S.J[3 * k + 1][l] = S.iz()[k] * dy - S.py()[k] * dz;
      S.J[3 * k + 2][l] = dz - dz0;
    }
  }
  __syncthreads();
  return cost;
}

struct RpInputs {
  const float *betas, *cam, *targets, *weights, *depth_weights, *prior, *z_prior;
};

__global__ void __launch_bounds__(64, 2) mano_reproj_ik_kernel(const harp_mano_model M, const RpInputs in, const harp_reproj_ik_options opt,
                                                            float* __restrict__ pose48, float* __restrict__ trans, float* __restrict__ cost,
                                                            int32_t* __restrict__ status, float* __restrict__ proj, float* __restrict__ jac) {
  __shared__ RpLds S;
  const int t = blockIdx.x, l = threadIdx.x;                           // (the grid is exactly N workgroups of one wave)
  const int lc = min(l, NX - 1);
  const int iters = opt.iters;
  const float prior_w = opt.pose_prior_weight, z_w = opt.z_prior_weight, focal = opt.focal, half = 0.5f * (float)opt.S;
  float lambda = opt.lambda0;
  float xl = 0.f;
  if (l < 48) xl = pose48[(size_t)t * 48 + l];
  else if (l < NX) xl = trans[(size_t)t * 3 + (l - 48)];
  if (l < NB) S.beta[l] = in.betas[(opt.betas_per_frame ? (size_t)t * NB : 0) + l];
  if (l == 48) {
    const float* c = in.cam + (opt.cam_per_frame ? (size_t)t * 3 : 0);
    S.cam[0] = 2.0f * focal / ((float)opt.S * c[0] + 1e-9f);           // t_z (utils/visualize.py:268)
    S.cam[1] = c[1]; S.cam[2] = c[2];
  }
  bool used = false;
  if (l < 21) {
    S.inv[c_reorder[l]] = l;
    const float w = in.weights ? in.weights[(size_t)t * 21 + l] : 1.0f;
    const float wz = (in.depth_weights && l > 0) ? in.depth_weights[(size_t)t * 21 + l] : 0.f;
    const float* tg = in.targets + ((size_t)t * 21 + l) * 3;
    const float t0 = tg[0], t1 = tg[1], t2 = tg[2];
    used = (w > 0.f) && isfinite(t0) && isfinite(t1);
    const bool used_z = (wz > 0.f) && isfinite(t2);
    S.W[3 * l] = S.W[3 * l + 1] = used ? w : 0.f;
    S.W[3 * l + 2] = used_z ? wz : 0.f;
    S.tgt[3 * l] = used ? t0 : 0.f; S.tgt[3 * l + 1] = used ? t1 : 0.f; S.tgt[3 * l + 2] = used_z ? t2 : 0.f;
  }
  const bool enough = __popcll(__ballot(used)) >= 4;
  __syncthreads();
  if (l < NJ * 3) {                                                    // rest joints at this shape (csrc/lbs.hip:43-48)
    float acc = M.J_template[l];
    for (int k = 0; k < NB; ++k) acc += M.J_dirs[l * NB + k] * S.beta[k];
    S.Jr[l / 3][l % 3] = acc;
  }
  if (l < 15) {                                                        // the tips' rest coordinates at this shape
    const int i = c_tips[l / 3] * 3 + l % 3;
    float acc = M.v_template[i];
    for (int k = 0; k < NB; ++k) acc += M.shapedirs_T[(size_t)k * NV * 3 + i] * S.beta[k];
    S.vs[l / 3][l % 3] = acc;
  }
  __syncthreads();

  const bool pose_lane = l >= 3 && l < 48;
  const float pw = pose_lane ? prior_w : (l == 50 ? z_w : 0.f);         // this lane's diagonal of P ...
  float pc = 0.f;                                                       // ... and what it pulls towards
  if (pose_lane && in.prior) pc = in.prior[(size_t)t * 45 + (l - 3)];
  if (l == 50 && in.z_prior) pc = in.z_prior[t];
  bool behind0, behind;
  float C = rp_eval<true>(M, S, l, xl, pw, pc, focal, half, behind0);
  const float C0 = C;
  const bool solve = enough && !behind0;
  int n_acc = 0;
  for (int it = 0; it < iters; ++it) {
    // this lane's weighted column, gradient entry and row of A
    float Jw[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) Jw[k] = S.W[k] * S.J[k][lc];
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < NR; ++k) g += Jw[k] * S.res[k];
    g += pw * (xl - pc);
    float diag = 1.f;
    for (int j = 0; j < NX; ++j) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < NR; ++k) a += Jw[k] * S.J[k][j];
      if (j == l) {
        a += pw;
        diag = a;
      }
      if (l < NX) S.A[l][j] = a;
    }
    bool ok;
    const float s = lm::jacobi_scale<NX>(l, diag, lambda, ok);
    __syncthreads();
    for (int j = 0; j < NX; ++j) {                                     // lm::solve's factorisation, column j
      const float sj = __shfl(s, j, 64);
      float v = 0.f;
      if (l >= j && l < NX) {
        v = (l == j) ? 1.0f : S.A[l][j] * s * sj;
        for (int c = 0; c < j; ++c) v -= S.A[l][c] * S.A[j][c];
      }
      const float piv = __shfl(v, j, 64);
      ok = ok && (piv > 0.f) && isfinite(piv);
      const float ljj = sqrtf(piv);
      if (l >= j && l < NX) S.A[l][j] = (l == j) ? ljj : v / ljj;
      __syncthreads();
    }
    float b = (l < NX) ? -g * s : 0.f, y = 0.f, z = 0.f;
    for (int j = 0; j < NX; ++j) {                                     // L y = b
      const float yj = __shfl(b, j, 64) / S.A[j][j];
      if (l == j) y = yj;
      if (l > j && l < NX) b -= S.A[l][j] * yj;
    }
    for (int j = NX - 1; j >= 0; --j) {                                // L^T z = y
      const float zj = __shfl(y, j, 64) / S.A[j][j];
      if (l == j) z = zj;
      if (l < j) y -= S.A[j][l] * zj;
    }
    const float xn = (l < NX) ? xl + z * s : 0.f;
    const float Cn = rp_eval<false>(M, S, l, xn, pw, pc, focal, half, behind);
    const bool accept = __builtin_amdgcn_readfirstlane((int)(ok && solve && !behind && (Cn < C))) != 0;       // (a NaN is not less)
    if (accept) {
      xl = xn;
      lambda = lm::damped(lambda, true);
      ++n_acc;
      C = rp_eval<true>(M, S, l, xl, pw, pc, focal, half, behind);
    } else {
      lambda = lm::damped(lambda, false);
    }
  }

  if (solve && iters > 0) {
    if (l < 48) pose48[(size_t)t * 48 + l] = xl;
    else if (l < NX) trans[(size_t)t * 3 + (l - 48)] = xl;
  }
  if (l == 0) {
    cost[2 * (size_t)t] = C0;
    cost[2 * (size_t)t + 1] = C;
    status[t] = !enough ? -1 : (behind0 ? -2 : n_acc);
  }
  if (proj && l < NR) proj[(size_t)t * NR + l] = S.prj[l];
  if (jac && l < NX)
    for (int r = 0; r < NR; ++r) jac[((size_t)t * NR + r) * NX + l] = S.J[r][l];
}

}  // namespace

extern "C" int harp_mano_reproj_ik_frames_per_block(void) { return kFramesPerBlock; }

extern "C" int harp_mano_reproj_ik(const harp_mano_model* m, const float* betas, const float* cam, const float* targets, const float* weights,
                                   const float* depth_weights, const float* prior, const float* z_prior, int N,
                                   const harp_reproj_ik_options* opt, float* pose48, float* trans, float* cost, int32_t* status, float* proj,
                                   float* jac, hipStream_t stream) {
  if (!m || !opt || !betas || !cam || !targets || !pose48 || !trans || !cost || !status || N <= 0 || opt->iters < 0) return HARP_ERR_ARG;
  const float nonneg[3] = {opt->lambda0, opt->pose_prior_weight, opt->z_prior_weight};
  for (float v : nonneg)
    if (!(v >= 0.f) || isinf(v)) return HARP_ERR_ARG;
  if (!(opt->focal > 0.f) || isinf(opt->focal) || opt->S <= 0) return HARP_ERR_ARG;
  if (!z_prior && opt->z_prior_weight != 0.f) return HARP_ERR_ARG;
  const RpInputs in = {betas, cam, targets, weights, depth_weights, prior, z_prior};
  hipLaunchKernelGGL(mano_reproj_ik_kernel, dim3((unsigned)N), dim3(64), 0, stream, *m, in, *opt, pose48, trans, cost, status, proj, jac);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
