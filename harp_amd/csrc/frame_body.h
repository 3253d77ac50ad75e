// Per-frame set-up, table scatter and step book-keeping shared by the fused front / back kernels of a fitting step (hand_front.hip,
// hand_back.hip, arm_front.hip) and the stand-alone glue kernels (glue.hip): the pieces that do not depend on the skinning model.
// The lane or wave a piece runs in differs between the kernels: it is a template argument or the caller's `if (tid == ...)`.
//   reference: the row gathers params[...][fid] (utils/visualize.py:26-27, 37-40), the camera convention (:268-271), shared light +
//   ambient ratio (optimize_sequence.py:453-456, 478-480; renderer_helper.py:435-441) and their autograd.
#pragma once
#include "chain_body.h"

namespace fb {

// ---- step prologue (harp_step_frame)
// target-local id of frame f, entry i = row * B + b of the schedule
__device__ __forceinline__ int step_tfid(const int32_t* tschedule, size_t i, int f, int target_offset) {
  return tschedule ? tschedule[i] : f - target_offset;
}

// Frame of batch slot b: fid[b], or — with a device schedule — the slot's entry of the current row (the row counter is bumped by the step
// epilogue, a later launch).  `write` (one lane per slot): publishes it in fid[b] / tfid_out[b], what schedule_next_kernel does as a launch.
__device__ __forceinline__ int step_frame_of(const harp_step_frame& E, const int32_t* fid, int b, int B, bool write) {
  if (!E.schedule) return fid[b];
  const int row = (int)((unsigned)E.sched_row[0] % (unsigned)E.n_rows);
  const int f = E.schedule[(size_t)row * B + b];
  if (write) {
    const_cast<int32_t*>(fid)[b] = f;
    if (E.tfid_out) E.tfid_out[b] = step_tfid(E.tschedule, (size_t)row * B + b, f, E.target_offset);
  }
  return f;
}

// Clear of frame b's slices of the two gradient segments the key-point / mesh terms accumulate into (inputs of the backward launch of the
// same struct), by part `part` of `parts` workgroups of `threads` threads
__device__ __forceinline__ void clear_mesh_grads(const harp_mesh_chain& A, int b, int part, int parts, int tid, int threads) {
  const int n = (A.V0 + A.E0) * 3, per = (n + parts - 1) / parts;
  float* gv = const_cast<float*>(A.g_vd) + (size_t)b * n;
  for (int k = part * per + tid; k < min((part + 1) * per, n); k += threads) gv[k] = 0.f;
  if (part == 0 && tid < A.NJ * 3) const_cast<float*>(A.g_joints_m)[(size_t)b * A.NJ * 3 + tid] = 0.f;
}

// ---- frame set-up: a frame's rows of the parameter tables
// camera row (scale, tx, ty) -> PyTorch3D R (row-major 9), T
__device__ __forceinline__ void cam_from_row(const float* cam_row, float focal, int S, float R[9], float T[3]) {
  const float c0 = cam_row[0], c1 = cam_row[1], c2 = cam_row[2];
  T[0] = -c1; T[1] = -c2; T[2] = 2.0f * focal / ((float)S * c0 + 1e-9f);
  const float I[9] = {-1.f, 0.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.f, 1.f};
  for (int k = 0; k < 9; ++k) R[k] = I[k];
}
// dL/d cam_row[k] from dL/dT
__device__ __forceinline__ float cam_row_bwd(const float* cam_row, float focal, int S, const float* g_T, int k) {
  if (k > 0) return -g_T[k - 1];
  const float c0 = cam_row[0];
  const float den = (float)S * c0 + 1e-9f;
  return g_T[2] * (-2.0f * focal * (float)S / (den * den));
}

// ambient / diffuse / specular colours (3 x rgb)
__device__ __forceinline__ void light_colors(int self_shadow, const float* amb_ratio, float* colors) {
  if (self_shadow) {
    const float amb = 1.0f / (1.0f + expf(-amb_ratio[0]));            // nn.Sigmoid()(params['amb_ratio'])
    for (int c = 0; c < 3; ++c) { colors[c] = amb; colors[3 + c] = 1.0f - amb; colors[6 + c] = 0.f; }
  } else {
    for (int c = 0; c < 3; ++c) { colors[c] = 0.5f; colors[3 + c] = 0.4f; colors[6 + c] = 0.1f; }   // renderer_helper.py:70-73
  }
}
// dL/d amb_ratio from dL/d colours
__device__ __forceinline__ float amb_ratio_bwd(const float* amb_ratio, const float* g_colors) {
  const float amb = 1.0f / (1.0f + expf(-amb_ratio[0]));
  const float g_amb = (g_colors[0] + g_colors[1] + g_colors[2]) - (g_colors[3] + g_colors[4] + g_colors[5]);
  return g_amb * amb * (1.0f - amb);
}

// Row gather of frame f into batch slot b of the front struct H (harp_hand_front / harp_arm_front) by one workgroup: lanes [0, ps) the
// pose row [rot(3), wrist_pose(3) if kWrist, pose(45)] -> pose_out, [64, 64 + nbo) the shape coefficients (padded with zeros), [128, 131)
// translation and light position, 192 the camera, kColorLane of frame 0 the colours.  `lead` guards the global writes (one workgroup of
// the frame); the LDS copies are made by every caller, a null one is not wanted.
template <bool kWrist, int kColorLane, class Front>
__device__ __forceinline__ void frame_rows(const Front& H, float* pose_out, int ps, int nbo, int f, int b, int tid, bool lead, float* s_pose,
                                           float* s_beta, float* s_tr, float* s_cam, float* s_lpos) {
  const harp_frame_tables& T = H.tables;
  if (tid < ps) {
    const float p = (tid < 3) ? T.rot[f * 3 + tid] : (kWrist && tid < 6) ? T.wrist_pose[f * 3 + tid - 3] : T.pose[f * 45 + tid - (kWrist ? 6 : 3)];
    s_pose[tid] = p;
    if (lead) pose_out[b * ps + tid] = p;
  } else if (tid >= 64 && tid < 64 + nbo) {
    const int k = tid - 64;
    const float v = (k < 10) ? T.shape[k] : 0.f;
    s_beta[k] = v;
    if (lead) H.betas[b * nbo + k] = v;
  } else if (tid >= 128 && tid < 131) {
    const int k = tid - 128;
    const float v = T.trans[f * 3 + k];
    if (s_tr) s_tr[k] = v;
    if (lead) {
      H.trans_b[b * 3 + k] = v;
      const int lf = T.share_light ? 0 : f;
      const float lp = T.light_positions[lf * 3 + k];
      if (s_lpos) s_lpos[k] = lp;
      H.light_pos[b * 3 + k] = lp;
    }
  } else if (tid == 192 && lead) {
    float R[9], ct[3];
    cam_from_row(T.cam + f * 3, H.chain.focal, H.chain.S, R, ct);
    for (int k = 0; k < 9; ++k) { if (s_cam) s_cam[k] = R[k]; H.cam_R[b * 9 + k] = R[k]; }
    for (int k = 0; k < 3; ++k) { if (s_cam) s_cam[9 + k] = ct[k]; H.cam_T[b * 3 + k] = ct[k]; }
  } else if (tid == kColorLane && lead && b == 0) {
    light_colors(H.self_shadow, T.amb_ratio, H.colors);
  }
}

// ---- scatter of what the mesh-chain backward leaves final into the gradient rows of the parameter tables; duplicates of a frame in one
//      batch are legal and the shared light is summed over the frames -> atomics.  Lane k < 3 of frame b (row f); the flags say which parts
//      this workgroup owns (`light`: there is an appearance gradient and the workgroup leads its frame)
__device__ __forceinline__ void tables_scatter(const harp_frame_tables& T, const harp_mesh_chain& A, int f, int b, int k, float g_trans,
                                               bool trans, bool cam, bool light) {
  if (T.g_trans && trans) atomicAdd(T.g_trans + f * 3 + k, g_trans);
  if (T.g_cam && cam) atomicAdd(T.g_cam + f * 3 + k, cam_row_bwd(T.cam + f * 3, A.focal, A.S, A.g_cam_T + b * 3, k));
  if (light && A.g_light_pos && T.g_light_positions) {
    const int lf = T.share_light ? 0 : f;
    atomicAdd(T.g_light_positions + lf * 3 + k, A.g_light_pos[b * 3 + k]);
  }
}
// the ambient lane (one of the whole grid)
__device__ __forceinline__ void amb_scatter(const harp_frame_tables& T, int self_shadow, const float* g_colors) {
  if (self_shadow && g_colors && T.g_amb_ratio) atomicAdd(T.g_amb_ratio, amb_ratio_bwd(T.amb_ratio, g_colors));
}

// ---- step epilogue (harp_step_frame), by ONE workgroup of the grid: every kernel that reads the schedule row, adds to the loss vector or
//      reads the draw counter is an EARLIER launch of the step (stream order / joins), so the three are turned over for the next step here.
//      Wave kWave, whole (the wave sum needs every lane): the loss vector, n_loss <= 64 (checked by the launchers); the two lanes behind
//      it: the schedule row and the draw counter.
template <int kWave>
__device__ __forceinline__ void step_epilogue(const harp_step_frame& E, int tid) {
  if ((tid >> 6) == kWave) {
    const int k = tid - kWave * 64;
    const bool on = E.loss && k < E.n_loss;
    const float v = on ? E.loss[k] : 0.f;
    if (on) {
      if (E.loss_out) E.loss_out[k] = v;
      E.loss[k] = 0.f;
    }
    if (E.loss_w && E.loss_total) {
      const float tot = wave_sum_u(on ? E.loss_w[k] * v : 0.f);
      if (k == 0) E.loss_total[0] += tot;
    }
  } else if (tid == (kWave + 1) * 64 && E.schedule) {
    E.sched_row[0] = (int)((unsigned)E.sched_row[0] % (unsigned)E.n_rows) + 1;
  } else if (tid == (kWave + 1) * 64 + 1 && E.draw_counter) {
    E.draw_counter[0] += 1;
  }
}

// ---- host side: the argument checks of the fused entry points (the size limits of a form and what only one form needs stay with it)
// mesh inputs and outputs of the chain forward
inline bool chain_fwd_ok(const harp_mesh_chain& a) {
  return a.edges0 && a.vf_off && a.vf_tri && a.disp && a.verts_mm && a.joints_mm && a.joints_m && a.vs && a.n1 && a.il1 && a.vd && a.n2 &&
         a.il2 && a.ndc_c && (!a.shadow || (a.centroid && a.light_R && a.light_T && a.ndc_l));
}
// mesh inputs, saved forward rows and gradient rows of the chain backward
inline bool chain_bwd_ok(const harp_mesh_chain& a) {
  return a.vf_off && a.vf_tri && a.disp && a.sub_off && a.sub_idx && a.vd && a.vs && a.n1 && a.il1 && a.cam_R && a.cam_T && a.g_vd &&
         a.g_ndc_c && a.g_joints_m && a.g_joints_mm && a.g_v0 && a.g_cam_T && a.g_disp && (!a.has_normal_grad || (a.n2 && a.il2 && a.g_n2)) &&
         (!a.shadow || (a.light_pos && a.centroid && a.light_R && a.light_T && a.g_ndc_l && a.g_light_R && a.g_light_T && a.g_light_pos));
}
// step prologue (schedule, clear of the mesh gradients) and, need_loss, the epilogue's loss vector
inline bool step_ok(const harp_step_frame& s, const harp_mesh_chain& a, bool need_loss) {
  return !(s.schedule && (!s.sched_row || s.n_rows <= 0)) && !(s.clear_mesh_grads && (!a.g_vd || !a.g_joints_m)) &&
         !(need_loss && s.loss && (s.n_loss < 0 || s.n_loss > 64));
}

}  // namespace fb
