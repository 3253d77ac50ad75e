// Batched inverse kinematics of the MANO hand for gfx950 (harp_amd/playback.py Motion.from_keypoints): 21 3-D keypoints per
// frame -> the rows [rot | pose | trans] that harp_lbs_mano_fwd turns back into those joints.  Nothing in the reference does this (its
// change_pose takes another sequence's parameters), so this header cites the model it inverts: csrc/lbs.hip and csrc/lbs_body.h.
//
// harp_mano_ik: T independent Levenberg-Marquardt solves in ONE launch, one wave (= one workgroup) per frame.  Per frame 51 unknowns
// x = [rot 3 | pose 45 | trans 3] and 63 residuals; cost C(x) = sum_k w_k |j_k(x) - t_k|^2 + w_prior sum_i (pose_i - prior_i)^2 with j(x)
// the 21 joints of harp_lbs_mano_fwd in metres (16 chain joints, 5 tip vertices with shape blend, pose correctives and skinning, trans,
// c_reorder's order; rodrigues_fwd and its tangent rodrigues_jvp, parent_of, c_tips, c_reorder from lbs_body.h).
//
//   forward      lanes 0..15 one Rodrigues each, lanes 0..4 one finger chain each (as lbs_joints_kernel), lanes 0..14 the posed tip
//                coordinates (135-long dot with the tips' posedirs rows), lanes 0..59 the tips' blended 3x4 transforms, lanes 0..62 one
//                joint coordinate, its residual and its share of the cost; the cost is a butterfly sum over the wave (fixed order).
//   Jacobian     lane i < 48 owns column i (joint i / 3, axis-angle component i % 3): the forward-mode tangent dR of ITS rotation (the
//                derivative of rodrigues_fwd itself, 1e-8 inside the norm included, so it holds at aa = 0), pushed down its finger
//                (the root: all five) and into ALL five tips: through the skinning weights of the joints it moves and through the tips'
//                pose correctives.  Lanes 48..50: the identity columns of trans.  J (63 x 51) lives in LDS.
//   normal eqs.  A = J^T W J + P (lane i: row i, its own weighted column in 63 registers, the other column a broadcast LDS read),
//                g = J^T W r + P (x - prior); the Jacobi scale of lm_solve_body.h (lm::jacobi_scale).
//   solve        the factorisation and both triangular solves of lm_solve_body.h, written out here: this kernel measured 0.3 % slower
//                through lm::solve, beyond its run-to-run spread.  x' = x + s z.
//   accept       C(x') < C(x) (a NaN is not less): x = x', lambda down, J re-evaluated; else lambda up (lm::damped).
// `iters` iterations whatever happens: no early exit, every branch is uniform over the wave.  No workspace, no allocation, no
// synchronisation, no atomics: the launch can be captured and a repeated call gives the same bits.
// A frame with fewer than 3 used joints (w_k > 0 and a finite target) runs the same instructions and writes nothing back but cost, status
// -1 and the optional joints / jac at its input.  An unused joint's target is tested for finiteness and never enters arithmetic.
#include "lbs_body.h"
#include "lm_solve_body.h"
#include "harp_hip.h"

#include <math.h>

namespace {

using namespace lb;

constexpr int NX = 51;                 // unknowns per frame
constexpr int NR = 63;                 // residuals per frame
constexpr int kIkFramesPerBlock = 1;   // one wave per workgroup: LDS (26.4 KiB a frame), not registers, bounds the frames in flight on a CU,
                                       // and single-frame workgroups waste none of it

struct IkLds {
  float J[NR][NX];                     // d joints (metres, output order) / d x
  float A[NX][NX];                     // normal matrix, then its scaled Cholesky factor in the lower triangle
  float x[NX + 1];                     // the point being evaluated
  float R[NJ][9], G[NJ][12], Jr[NJ][3];
  float vs[5][3], vp[5][3], Tk[5][12], pm[NP];
  float w[21], res[NR], jnt[NR], tgt[NR], beta[NB], prior[48];
  int inv[21];                         // inverse of c_reorder: model joint / tip -> output joint
};
static_assert(sizeof(IkLds) == 27056, "the frames in flight on a CU rest on this size (DESIGN.md §24)");

__device__ __forceinline__ void joint_aa(const harp_mano_model& M, const IkLds& S, int j, float aa[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p = S.x[3 * j + c];
    aa[c] = (j == 0) ? p : (M.hands_mean[3 * (j - 1) + c] + p);       // (csrc/lbs.hip:35)
  }
}

// The joints, residuals and cost at xl (lane l's unknown); JAC: also S.jnt, S.res and the Jacobian S.J.  Returns C(x), the same bits in every lane.
template <bool JAC>
__device__ float ik_eval(const harp_mano_model& M, IkLds& S, int l, float xl, float prior_w) {
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
    v += S.x[48 + c];
    const float wk = S.w[k];
    const float r = (wk > 0.f) ? (v - S.tgt[l]) : 0.f;               // (S.tgt is 0 for an unused joint, S.w too)
    part = wk * r * r;
    if (JAC) { S.jnt[l] = v; S.res[l] = r; }
  }
  if (l >= 3 && l < 48) {
    const float d = xl - S.prior[l - 3];
    part += prior_w * d * d;
  }
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
  __syncthreads();
  return cost;
}

__global__ void __launch_bounds__(64, 2) mano_ik_kernel(const harp_mano_model M, const float* __restrict__ betas, int betas_per_frame,
                                                     const float* __restrict__ targets, const float* __restrict__ weights,
                                                     const float* __restrict__ prior, int iters, float lambda, float prior_w,
                                                     float* __restrict__ pose48, float* __restrict__ trans, float* __restrict__ cost,
                                                     int32_t* __restrict__ status, float* __restrict__ joints, float* __restrict__ jac) {
  __shared__ IkLds S;
  const int t = blockIdx.x, l = threadIdx.x;                           // (the grid is exactly T workgroups of one wave)
  const int lc = min(l, NX - 1);
  float xl = 0.f;
  if (l < 48) xl = pose48[(size_t)t * 48 + l];
  else if (l < NX) xl = trans[(size_t)t * 3 + (l - 48)];
  if (l < NB) S.beta[l] = betas[(betas_per_frame ? (size_t)t * NB : 0) + l];
  if (l < 48) S.prior[l] = (prior && l < 45) ? prior[(size_t)t * 45 + l] : 0.f;
  bool used = false;
  if (l < 21) {
    S.inv[c_reorder[l]] = l;
    const float w = weights ? weights[(size_t)t * 21 + l] : 1.0f;
    const float* tg = targets + ((size_t)t * 21 + l) * 3;
    const float t0 = tg[0], t1 = tg[1], t2 = tg[2];
    used = (w > 0.f) && isfinite(t0) && isfinite(t1) && isfinite(t2);
    S.w[l] = used ? w : 0.f;
    S.tgt[3 * l] = used ? t0 : 0.f; S.tgt[3 * l + 1] = used ? t1 : 0.f; S.tgt[3 * l + 2] = used ? t2 : 0.f;
  }
  const bool solve = __popcll(__ballot(used)) >= 3;
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

  float C = ik_eval<true>(M, S, l, xl, prior_w);
  const float C0 = C;
  int n_acc = 0;
  const bool pose_lane = l >= 3 && l < 48;
  for (int it = 0; it < iters; ++it) {
    // this lane's weighted column, gradient entry and row of A
    float Jw[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) Jw[k] = S.w[k / 3] * S.J[k][lc];
    float g = 0.f;
#pragma unroll
    for (int k = 0; k < NR; ++k) g += Jw[k] * S.res[k];
    if (pose_lane) g += prior_w * (xl - S.prior[l - 3]);
    float diag = 1.f;
    for (int j = 0; j < NX; ++j) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < NR; ++k) a += Jw[k] * S.J[k][j];
      if (j == l) {
        if (pose_lane) a += prior_w;
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
    const float Cn = ik_eval<false>(M, S, l, xn, prior_w);
    const bool accept = __builtin_amdgcn_readfirstlane((int)(ok && solve && (Cn < C))) != 0;       // (a NaN is not less)
    if (accept) {
      xl = xn;
      lambda = lm::damped(lambda, true);
      ++n_acc;
      C = ik_eval<true>(M, S, l, xl, prior_w);
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
    status[t] = solve ? n_acc : -1;
  }
  if (joints && l < NR) joints[(size_t)t * NR + l] = S.jnt[l] * 1000.0f;
  if (jac && l < NX)
    for (int r = 0; r < NR; ++r) jac[((size_t)t * NR + r) * NX + l] = S.J[r][l];
}

}  // namespace

extern "C" int harp_mano_ik_frames_per_block(void) { return kIkFramesPerBlock; }

extern "C" int harp_mano_ik(const harp_mano_model* m, const float* betas, const float* targets, const float* weights, const float* prior, int T,
                            const harp_ik_options* opt, float* pose48, float* trans, float* cost, int32_t* status, float* joints, float* jac,
                            hipStream_t stream) {
  if (!m || !opt || !betas || !targets || !pose48 || !trans || !cost || !status || T <= 0 || opt->iters < 0) return HARP_ERR_ARG;
  if (!(opt->lambda0 >= 0.f) || !(opt->prior_weight >= 0.f) || isinf(opt->lambda0) || isinf(opt->prior_weight)) return HARP_ERR_ARG;
  hipLaunchKernelGGL(mano_ik_kernel, dim3((unsigned)T), dim3(64), 0, stream, *m, betas, opt->betas_per_frame != 0, targets, weights, prior,
                     opt->iters, opt->lambda0, opt->prior_weight, pose48, trans, cost, status, joints, jac);
  HARP_CHECK_LAUNCH();
  return HARP_OK;
}
