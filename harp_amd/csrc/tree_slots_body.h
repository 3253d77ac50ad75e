// The structural tables of a kinematic tree whose 17 input rows [rot | wrist | pose(15)] drive 17 of its joints, as the arm's two pose
// solvers need them (arm_vertex_fit.hip, DESIGN.md §28, builds them here; arm_ik.hip, §29, carries the same routine written out for one wave,
// because it measured slower through this one: §31): what no unknown moves and a solve builds once in its prologue.
//   par, depth, maxd   the tree (par[j] < j, so every walk up ends) and its levels
//   drv, driven        the joint an input row drives; whether anything drives a joint
//   slots              for every driven joint but the root the joints at or below it, parents before children: row's slots are
//                      soff[row] .. soff[row + 1], slot s holds joint sj[s], sp[s] is its parent's slot (-1: the row's own joint), and
//                      spos[row][j] finds joint j's slot among the row's (NOSLOT: j is not below the row's joint).  The column of a wrist or
//                      finger unknown walks its row's slots to push its tangent down the tree.
#pragma once
#include "lbs_tree_body.h"

namespace lt {

constexpr int NIN = 17;                 // rows of in_pose
constexpr int MAXSLOT = 48;             // (row's joint, joint at or below it) pairs: the arm has 16 + 5 x 6 = 46
constexpr int NOSLOT = 255, UNSET = 254;

struct TreeTables {
  int par[MAXJ], depth[MAXJ], drv[NIN];
  int soff[NIN + 1];
  int sj[MAXSLOT], sp[MAXSLOT];
  int maxd, bad;
  unsigned char spos[NIN][MAXJ], driven[MAXJ];
};

// By a workgroup of T threads, every one of which must call.  Sets S.bad when the model is not of the shape these tables hold (then returns
// early, right after a barrier).  NO barrier follows the last step: a caller places a __syncthreads() before anything reads sj / sp / spos.
template <int T>
__device__ __forceinline__ void tree_tables(const harp_tree_model& M, TreeTables& S, int tid) {
  const int NJ = M.NJ;
  if (tid < NJ) S.par[tid] = min(M.parents[tid], tid - 1);             // (parents[j] < j: every walk up the tree ends)
  if (tid < NIN) S.drv[tid] = -1;
  for (int i = tid; i < NIN * MAXJ; i += T) (&S.spos[0][0])[i] = NOSLOT;
  if (tid == 0) S.bad = 0;
  __syncthreads();
  if (tid < NJ) {
    const int src = M.pose_src[tid];
    const bool drn = src >= 0 && src < NIN;
    S.driven[tid] = drn ? 1 : 0;
    if (drn) S.drv[src] = tid;
    int d = 0;
    for (int q = S.par[tid]; q >= 0; q = S.par[q]) ++d;
    S.depth[tid] = d;
  }
  __syncthreads();
  if (tid == 0) {
    int md = 0, bad = (S.drv[0] != 0);
    for (int j = 0; j < NJ; ++j) md = max(md, S.depth[j]);
    for (int r = 1; r < NIN; ++r) bad |= (S.drv[r] <= 0);
    S.maxd = md;
    S.bad = bad;
  }
  __syncthreads();
  if (S.bad) return;
  for (int i = tid; i < (NIN - 1) * NJ; i += T) {                      // is joint j the row's joint or below it (the root row has no slots)
    const int row = 1 + i / NJ, j = i % NJ, jq = S.drv[row];
    int a = j;
    while (a > jq) a = S.par[a];
    if (a == jq) S.spos[row][j] = UNSET;
  }
  __syncthreads();
  if (tid == 0) {
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
  if (tid >= 1 && tid < NIN) {                                         // the row's slots, parents before children (par[j] < j)
    const int jq = S.drv[tid];
    int s = S.soff[tid];
    for (int j = jq; j < NJ; ++j) {
      if (S.spos[tid][j] != UNSET) continue;
      S.sj[s] = j;
      S.sp[s] = (j == jq) ? -1 : (int)S.spos[tid][S.par[j]];
      S.spos[tid][j] = (unsigned char)s;
      ++s;
    }
  }
}

// The rotation of joint j when nothing drives it: the model's pose mean, which is NOT zero in general, constant over the solve.
__device__ __forceinline__ void undriven_rotation(const harp_tree_model& M, const TreeTables& S, int j, float (*Rj)[9]) {
  if (j >= 0 && j < M.NJ && !S.driven[j]) {
    const float aa[3] = {M.pose_mean[3 * j], M.pose_mean[3 * j + 1], M.pose_mean[3 * j + 2]};
    float R[9];
    rod_fwd(aa, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) Rj[j][k] = R[k];
  }
}

}  // namespace lt
