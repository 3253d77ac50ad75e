"""Playback of a fitted avatar: drive it with a motion it was not fitted on, at an output frame rate of the caller's choice, and composite
it over a video or a plain background as finished 8-bit frames.  Stands in for the reference's `change_pose`
(utils/visualize.py:111-143) and the render calls of :258-320 followed by the host-side `(img * 255).astype(np.uint8)`.

The package in six modules, each importing only those before it:

  keypoints  the float64 host side of the keypoint solve: rest joints, bone-length scale, Kabsch start, `ik_inputs`; `vertex_start`, the
             batched rigid start of the vertex fit; `rest_arm_joints`, `match_arm_lengths`, `arm_palm_start` for the SMPL-X arm's keypoints; `planar_palm_starts`, `project_pixels`, `image_ik_inputs` for image keypoints, `arm_image_ik_inputs`, `arm_image_starts` for the arm's; and `checked`, the one coercion of a caller's tensor or array-like
  motion     `Motion` (the per-frame rows), `RowLayout` (their one packed table), `Motion.resample` (ops.motion_resample),
             `Motion.from_keypoints` (ops.mano_ik), `Motion.from_image_keypoints` (ops.mano_reproj_ik), `Motion.from_arm_image_keypoints` (ops.arm_reproj_ik), `Motion.from_vertices` (ops.mano_vertex_fit), `Motion.from_arm_vertices` (ops.arm_vertex_fit), `Motion.from_arm_keypoints` (ops.arm_ik), `Motion.smooth` / `smooth_keypoints` (ops.motion_filter), `motion_jitter`
  labels     `face_part_labels`, `part_names`: the part of the hand every face belongs to, from the skinning weights (host integers)
  selfcontact  `geodesic_exclusion`, `pack_exclusion`, `unpack_exclusion`: which faces of a mesh do not count for which of its own vertices
             (an edge-path radius on the rest geometry) and the bit table harp_mesh_contact_excl reads; torch, any device
  player     `AvatarPlayer`, the forward-only renderer — the fit's own fused front, rasterisers and shader without a backward, then
             harp_resolve_u8: six calls of the C ABI per batch of frames, in order on one stream, captured into a graph — and `ScenePlayer`,
             several such avatars in one frame through ONE harp_composite_layers_u8 per batch; both on `_Player`, which owns the
             staging table (`_Stage`), the graphs, each pass's buffers and the way to disk.  A call is one pass — frames, labels, flow,
             contact or self-contact — under a graph of its own: `annotate` of either says what the frames show (harp_annotate_layers,
             harp_keypoint_visibility), `flow` where each pixel's surface point lies in another frame (harp_flow_layers), both written
             once over the player's layers (an avatar is a scene of one); `ScenePlayer.contact` where the avatars touch: per vertex
             the signed distance to the nearest other avatar, its face and part (harp_mesh_contact); `self_contact` of either where
             an avatar touches ITSELF — a pinch, a fist — per vertex the signed distance to the nearest face of its own surface beyond
             a geodesic radius, which parts touch which (harp_mesh_contact_excl)
  cli        `main`:

    python -m harp_amd.playback --config CFG (--motion MOTION.npz | --keypoints KP.npz | --keypoints2d KP.npz | --vertices V.npz) --out DIR [--fps-scale X] [--ss 2] [--background DIR] [--alpha]
                                [--flip] [--also CFG:MOTION[:flip]]... [--scene-depth DIR] [--masks]
                                [--smooth SIGMA [--smooth-trim RAD]] [--smooth-keypoints SIGMA] [--labels [--label-tol M]]
                                [--flow {fw,bw,both} [--flow-tol M]] [--contacts [--contact-dist M]]
                                [--self-contacts [--self-contact-dist M] [--self-geodesic M]]

Importing the package needs neither the built library nor a device.
"""
from .cli import main
from .keypoints import (ARM_JOINT_IDX, CHAIN_BONES, ELBOW, JOINT_REORDER, PALM, arm_image_ik_inputs, arm_image_starts, arm_palm_start, axis_angle_of, bone_length_scale,
                        kabsch_rotation, match_arm_lengths, palm_start, planar_palm_starts, project_pixels, rest_arm_joints, rest_chain_joints,
                        vertex_start)
from .labels import face_part_labels, part_names
from .motion import Motion, motion_jitter, pose_mean_rows, smooth_keypoints
from .selfcontact import geodesic_exclusion, pack_exclusion, unpack_exclusion
from .player import (BG_WHITE, CONTACT_DIST, FLOW_TOL, LABEL_TOL, SELF_CONTACT_DIST, SELF_GEODESIC, Annotation, Contact, Flow, SelfContact, AvatarPlayer,
                     ScenePlayer, load_backgrounds, load_scene_depth)

__all__ = ["Motion", "AvatarPlayer", "ScenePlayer", "smooth_keypoints", "motion_jitter", "pose_mean_rows", "rest_chain_joints",
           "bone_length_scale", "kabsch_rotation", "axis_angle_of", "palm_start", "JOINT_REORDER", "PALM", "CHAIN_BONES", "load_backgrounds",
           "load_scene_depth", "main", "BG_WHITE", "vertex_start", "arm_palm_start", "rest_arm_joints", "match_arm_lengths", "ARM_JOINT_IDX", "ELBOW",
           "planar_palm_starts", "project_pixels", "face_part_labels", "part_names", "Annotation", "LABEL_TOL", "Flow", "FLOW_TOL", "arm_image_ik_inputs",
           "arm_image_starts", "Contact", "CONTACT_DIST", "SelfContact", "SELF_CONTACT_DIST", "SELF_GEODESIC", "geodesic_exclusion", "pack_exclusion",
           "unpack_exclusion"]
