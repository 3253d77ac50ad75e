"""ctypes binding of the C-ABI library (include/harp_hip.h).  No CPU fallback: if the library is missing
or a call fails, raise — the product path must never silently run anything else."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HARP_LIB_PATH") or os.path.join(_HERE, "csrc", "libharp_hip.so")   # override: A/B of kernel variants

_vp, _i, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t

# name -> (restype, argtypes); must list every symbol include/harp_hip.h declares (tests/test_abi.py checks)
SIGNATURES = {
    "harp_rasterize_ws_bytes": (_sz, [_i, _i, _i]),
    "harp_rasterize_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "harp_silhouette_bwd": (_i, [_vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"HIP library not built: {LIB_PATH} (run `python -m harp_amd.build`); "
                               "harp_amd has no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def ptr(t):
    """Raw device pointer of a contiguous CUDA(HIP) tensor, or NULL for None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError("harp_amd ops need contiguous tensors")
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(code, what):
    if code != 0:
        raise RuntimeError(f"{what} failed with status {code}")


class ShadeArgs(ctypes.Structure):
    """mirror of `harp_shade_args` (include/harp_hip.h)"""
    _fields_ = ([(n, _vp) for n in ("face_id", "recs", "faces", "faces_uvs", "verts_uvs", "verts", "vnormals", "tex", "nmap",
                                    "light_pos", "colors", "zl", "light_R", "light_T")] +
                [(n, _i) for n in ("B", "V", "F", "S", "Ht", "Wt")] +
                [(n, _f) for n in ("focal", "ppx", "ppy")] + [("bg", _f * 3)] +
                [(n, _vp) for n in ("rgb", "g_rgb", "g_tex", "g_nmap", "g_verts", "g_vnormals", "g_ndc", "g_zl", "g_light_pos",
                                    "g_colors", "g_light_R", "g_light_T")] + [("debug_skip", _i)] +
                [(n, _vp) for n in ("l1_target", "l1_mask", "l1_fid", "l1_w", "l1_loss", "l1_grad")] + [("l1_inv", _f), ("texnm", _vp), ("l1_bg_sums", _vp), ("g_zl_tiles", _vp),
                 ("trec", _vp), ("trec_cnt", _vp), ("trec_cap", _i), ("trec_acc_tex", _vp), ("trec_acc_nmap", _vp), ("g_vert9", _vp)])


SIGNATURES.update({
    "harp_depth_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "harp_depth_bwd_consume": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "harp_shade_fwd": (_i, [ctypes.POINTER(ShadeArgs), _vp]),
    "harp_shade_bwd": (_i, [ctypes.POINTER(ShadeArgs), _vp]),
    "harp_texel_bins": (_i, [_i, _i]),
    "harp_texel_reduce": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp]),
    "harp_texel_finish": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "harp_pack_texels": (_i, [_vp, _vp, _i, _vp, _vp]),
    "harp_normalize3_pack": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "harp_depth_nmap_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "harp_depth_bwd_tiles": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "harp_depth_bwd_riders": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "harp_vert9_unpack": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "harp_subdivide_fwd": (_i, [_vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "harp_subdivide_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "harp_vertex_normals_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "harp_vertex_normals_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "harp_displace_bwd": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "harp_project_fwd": (_i, [_vp, _vp, _vp, _i, _i, _f, _f, _f, _i, _vp, _vp]),
    "harp_project_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp]),
    "harp_centroid": (_i, [_vp, _i, _i, _vp, _vp]),
})


class ManoModel(ctypes.Structure):
    """mirror of `harp_mano_model` (include/harp_hip.h)"""
    _fields_ = [(n, _vp) for n in ("v_template", "shapedirs_T", "posedirs_T", "posedirs", "J_template", "J_dirs", "weights", "hands_mean")]


_mp = ctypes.POINTER(ManoModel)
SIGNATURES.update({
    "harp_lbs_mano_ws_floats": (_sz, [_i]),
    "harp_lbs_mano_fwd": (_i, [_mp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "harp_lbs_mano_bwd": (_i, [_mp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "harp_image_l1": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "harp_kps_loss": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "harp_mesh_regularizers": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "harp_sum_squares": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "harp_mse": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "harp_texture_smooth_reg": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "harp_mesh_kps_terms": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "harp_texture_terms": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "harp_close_to_z_reg": (_i, [_vp, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "harp_normalize3_fwd": (_i, [_vp, _i, _vp, _vp]),
    "harp_normalize3_bwd": (_i, [_vp, _vp, _i, _vp, _vp]),
    "harp_adam_step": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _i, _f, _vp]),
})


class FrameTables(ctypes.Structure):
    """mirror of `harp_frame_tables` (include/harp_hip.h)"""
    _fields_ = ([(n, _vp) for n in ("pose", "rot", "trans", "cam", "shape", "light_positions", "amb_ratio", "g_pose", "g_rot", "g_trans",
                                    "g_cam", "g_shape", "g_light_positions", "g_amb_ratio")] + [("share_light", _i)] +
                [("wrist_pose", _vp), ("g_wrist_pose", _vp), ("n_betas_out", _i)])


_tp = ctypes.POINTER(FrameTables)
SIGNATURES.update({
    "harp_frame_setup_fwd": (_i, [_tp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "harp_frame_setup_bwd": (_i, [_tp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "harp_light_setup_fwd": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "harp_light_setup_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "harp_scale": (_i, [_vp, _f, _i, _vp, _vp]),
    "harp_schedule_next": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "harp_schedule_next_rows": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
})

SIGNATURES.update({
    "harp_adam_tick": (_i, [_vp, _i, _vp]),
    "harp_step_prologue": (_i, [_vp, _sz, _vp, _i, ctypes.c_uint, _vp, _i, _i, _f, _vp, _f, _vp, _vp]),
    "harp_adam_apply": (_i, [_vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "harp_adam_apply2": (_i, [_vp, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp, _vp]),
})


class TreeModel(ctypes.Structure):
    """mirror of `harp_tree_model` (include/harp_hip.h)"""
    _fields_ = ([(n, _i) for n in ("NV", "NJ", "NB")] +
                [(n, _vp) for n in ("v_template", "shapedirs_T", "posedirs_T", "posedirs", "J_template", "J_dirs", "weights", "pose_mean", "parents",
                                    "pose_src")] + [("n_pose_in", _i), ("center_joint", _i), ("n_joints_out", _i), ("joint_src", _vp)])


_trp = ctypes.POINTER(TreeModel)
SIGNATURES.update({
    "harp_lbs_tree_ws_floats": (_sz, [_trp, _i]),
    "harp_lbs_tree_fwd": (_i, [_trp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "harp_lbs_tree_bwd": (_i, [_trp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
})


class MeshChain(ctypes.Structure):
    """mirror of `harp_mesh_chain` (include/harp_hip.h)"""
    _fields_ = ([(n, _vp) for n in ("edges0", "vf_off", "vf_tri", "sub_off", "sub_idx", "disp")] +
                [(n, _i) for n in ("B", "V0", "E0", "NJ", "S")] + [("focal", _f), ("shadow", _i), ("has_normal_grad", _i), ("light_only", _i)] +
                [(n, _vp) for n in ("verts_mm", "joints_mm", "cam_R", "cam_T", "light_pos",
                                    "joints_m", "vs", "n1", "il1", "vd", "n2", "il2", "ndc_c", "centroid", "light_R", "light_T", "ndc_l",
                                    "g_ndc_c", "g_ndc_l", "g_n2", "g_joints_m", "g_vd", "g_light_R", "g_light_T",
                                    "g_v0", "g_joints_mm", "g_light_pos", "g_cam_T", "g_disp")])


SIGNATURES["harp_mesh_chain_max_vertices"] = (_i, [])
SIGNATURES["harp_mesh_chain_fwd"] = (_i, [ctypes.POINTER(MeshChain), _vp])
SIGNATURES["harp_mesh_chain_bwd"] = (_i, [ctypes.POINTER(MeshChain), _vp])
SIGNATURES["harp_mesh_chain_wide_ws_floats"] = (_sz, [_i, _i])
SIGNATURES["harp_mesh_chain_bwd_wide"] = (_i, [ctypes.POINTER(MeshChain), _vp, _vp])
SIGNATURES["harp_mesh_chain_fwd_wide"] = (_i, [ctypes.POINTER(MeshChain), _i, _vp, _vp])
SIGNATURES["harp_draw_texture_offsets"] = (_i, [ctypes.c_uint, _vp, _i, _i, _f, _vp, _f, _vp, _vp])
SIGNATURES["harp_raster_setup_pair"] = (_i, [_vp, _f, _vp, _vp, _f, _vp, _vp, _i, _i, _i, _i, _vp])
SIGNATURES["harp_rasterize_fwd_keep"] = (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp])
SIGNATURES["harp_rasterize_l1_fwd"] = (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
SIGNATURES["harp_sil_records_bytes"] = (_sz, [_i, _i, _i])
SIGNATURES["harp_sil_records_bind"] = (_i, [_vp, _vp, _i, _i, _i, _i])
SIGNATURES["harp_rasterize_l1_fwd_bwd"] = (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])

# data-parallel exchange (csrc/comm.hip): RCCL bound at run time, all-reduce enqueued on the caller's stream
SIGNATURES.update({
    "harp_comm_unique_id": (_i, [_vp]),
    "harp_comm_create": (_i, [_vp, _i, _i, ctypes.POINTER(_vp)]),
    "harp_comm_destroy": (_i, [_vp]),
    "harp_allreduce_flat": (_i, [_vp, _vp, _sz, _vp]),
})
COMM_ID_BYTES = 128
SIGNATURES.update({
    "harp_rasterize_fragments_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "harp_rasterize_fragments_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _vp]),
})
SIGNATURES["harp_shade_sil_bwd"] = (_i, [ctypes.POINTER(ShadeArgs), _f, _f, _vp, _vp, _vp])


class StepFrame(ctypes.Structure):
    """mirror of `harp_step_frame` (include/harp_hip.h)"""
    _fields_ = [("schedule", _vp), ("tschedule", _vp), ("sched_row", _vp), ("n_rows", _i), ("target_offset", _i), ("tfid_out", _vp), ("clear_mesh_grads", _i),
                ("loss", _vp), ("loss_out", _vp), ("n_loss", _i), ("draw_counter", _vp), ("loss_w", _vp), ("loss_total", _vp)]


class HandFront(ctypes.Structure):
    """mirror of `harp_hand_front` (include/harp_hip.h)"""
    _fields_ = ([("chain", MeshChain), ("mano", ManoModel), ("tables", FrameTables), ("fid", _vp)] +
                [(n, _vp) for n in ("pose48", "betas", "trans_b", "cam_R", "cam_T", "light_pos", "colors", "lbs_ws")] + [("self_shadow", _i),
                 ("step", StepFrame)])


SIGNATURES["harp_hand_front_fwd"] = (_i, [ctypes.POINTER(HandFront), _vp])
SIGNATURES["harp_hand_front_wide_fwd"] = (_i, [ctypes.POINTER(HandFront), _vp, _vp])
SIGNATURES["harp_hand_front_hybrid_fwd"] = (_i, [ctypes.POINTER(HandFront), _vp])
SIGNATURES["harp_hand_back_bwd"] = (_i, [ctypes.POINTER(HandFront), _vp, _vp, _vp])
SIGNATURES["harp_hand_back_wide_bwd"] = (_i, [ctypes.POINTER(HandFront), _vp, _vp, _vp, _vp])


class ArmFront(ctypes.Structure):
    """mirror of `harp_arm_front` (include/harp_hip.h)"""
    _fields_ = ([("chain", MeshChain), ("tree", TreeModel), ("tables", FrameTables), ("fid", _vp)] +
                [(n, _vp) for n in ("pose_in", "betas", "trans_b", "cam_R", "cam_T", "light_pos", "colors", "lbs_ws", "weights_T")] +
                [("self_shadow", _i), ("step", StepFrame)])


SIGNATURES["harp_arm_front_fwd"] = (_i, [ctypes.POINTER(ArmFront), _vp])
SIGNATURES["harp_arm_back_bwd"] = (_i, [ctypes.POINTER(ArmFront), _vp, _vp, _vp, _vp])
SIGNATURES["harp_arm_front_wide_fwd"] = (_i, [ctypes.POINTER(ArmFront), _vp, _vp])
SIGNATURES["harp_arm_back_wide_bwd"] = (_i, [ctypes.POINTER(ArmFront), _vp, _vp, _vp, _vp, _vp])


class Conv3x3Args(ctypes.Structure):
    """mirror of `harp_conv3x3_args` (include/harp_hip.h)"""
    _fields_ = ([(n, _vp) for n in ("in_", "filters", "bias", "out", "pooled", "target", "target_row", "g_tap", "loss", "gate")] +
                [(n, _i) for n in ("N", "H", "W", "Cin", "Cout", "precision", "epilogue", "in_channels")] + [("tap_scale", _f)] +
                [("tile_list", _vp), ("tile_count", _vp), ("max_tiles", _i), ("in_valid_shift", _i), ("in_valid", _vp), ("in_alt", _vp),
                 ("out_valid", _vp), ("tile_origin", _vp), ("in_valid_origin", _vp), ("out_valid_origin", _vp), ("tile_pitch", _i),
                 ("in_valid_pitch", _i), ("out_valid_pitch", _i), ("tile_side", _i), ("in_valid_cell", _i), ("out_valid_cell", _i),
                 ("in_amax", _vp), ("in_exp", _i)])


SIGNATURES.update({
    "harp_conv3x3_filter_bytes": (_sz, [_i, _i]),
    "harp_conv3x3_pack_filters": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "harp_conv3x3": (_i, [ctypes.POINTER(Conv3x3Args), _vp]),
})


class Vgg16(ctypes.Structure):
    """mirror of `harp_vgg16` (include/harp_hip.h)"""
    _fields_ = [("filters", _vp * 10), ("filters_t", _vp * 10), ("bias", _vp * 10), ("w0t", _vp), ("layer_w", _f * 5), ("precision", _i)]


class Vgg16TermArgs(ctypes.Structure):
    """mirror of `harp_vgg16_term_args` (include/harp_hip.h)"""
    _fields_ = [("rgb", _vp), ("y_true", _vp), ("mask", _vp), ("rows", _vp), ("target", _vp * 4), ("target_by_row", _i), ("covered", _vp),
                ("g_rgb", _vp), ("weight", _f), ("loss", _vp), ("N", _i), ("S", _i), ("ws", _vp), ("target_in", _vp * 10), ("tiles", _vp * 4),
                ("tile_list", _vp * 4), ("tile_count", _vp * 4), ("max_tiles", _i * 4), ("tile_origin", _vp * 4), ("tile_pitch", _i * 4), ("tile_side", _i * 4), ("side_streams", _vp * 3)]


SIGNATURES.update({
    "harp_vgg16_ws_bytes": (_sz, [_i, _i, _i]),
    "harp_vgg16_features": (_i, [ctypes.POINTER(Vgg16), _vp, _vp, _vp, _i, _i, _vp, ctypes.POINTER(_vp), _vp]),
    "harp_vgg16_term": (_i, [ctypes.POINTER(Vgg16), ctypes.POINTER(Vgg16TermArgs), _vp]),
})

# post-fit evaluation metrics (csrc/metrics.hip)
_ll = ctypes.c_longlong
SIGNATURES.update({
    "harp_image_metrics_ws_bytes": (_sz, [_i, _i, _i]),
    "harp_image_metrics": (_i, [_vp, _vp, _vp, _vp, _ll, _ll, _ll, _ll, _i, _i, _i, _i, _f, ctypes.POINTER(_f), _i, _f, _f, _f, _vp, _vp, _vp]),
})

# LPIPS v0.1 / AlexNet of the post-fit evaluation (csrc/lpips.hip)
SIGNATURES.update({
    "harp_lpips_alex_net_bytes": (_sz, []),
    "harp_lpips_alex_pack": (_i, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp), _vp, _vp]),
    "harp_lpips_alex_ws_bytes": (_sz, [_i, _i, _i]),
    "harp_lpips_alex": (_i, [_vp, _vp, _vp, _ll, _ll, _ll, _ll, _i, _i, _i, _i, _vp, _vp, _vp]),
})

# normal image and uint8 panel strips of the post-fit pass (csrc/present.hip)
SIGNATURES.update({
    "harp_normal_image": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, ctypes.POINTER(_f), _vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "harp_panels_u8": (_i, [ctypes.POINTER(_vp), ctypes.POINTER(_ll), _i, _vp, _vp, _i, _i, _i, _vp, _vp]),
})

# uint8 contact sheets of the in-fit monitor (csrc/sheet.hip)
SIGNATURES["harp_sheet_u8"] = (_i, [_i, _vp, ctypes.POINTER(_ll), _vp, ctypes.POINTER(_ll), _vp, ctypes.POINTER(_ll), _i, _i, _i, _i, _i, _i, _vp, _vp])

# Taubin smoothing of the exported meshes (csrc/smooth.hip)
SIGNATURES.update({
    "harp_taubin_ws_bytes": (_sz, [_i, _i]),
    "harp_taubin_smooth": (_i, [_vp, _vp, _vp, _i, _i, _f, _f, _i, _i, _vp, _vp, _vp]),
})

# geometric accuracy of the post-fit evaluation (csrc/pose_eval.hip)
SIGNATURES.update({
    "harp_procrustes_align": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "harp_pck_counts": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "harp_point_set_fscore": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
})

# decoded uint8 frames -> the resident float32 targets (csrc/ingest.hip)
SIGNATURES["harp_targets_from_u8"] = (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp])


class BakeArgs(ctypes.Structure):
    """mirror of `harp_bake_args` (include/harp_hip.h)"""
    _fields_ = ([(n, _vp) for n in ("texel_idx", "texel_face", "texel_bary", "faces", "ndc", "face_id", "zbuf", "y_true", "y_mask", "rows",
                                    "verts", "vnormals", "cam_pos", "light_pos", "colors", "sum_w", "sum_wc", "sum_wc2", "count", "best_cos")] +
                [(n, _i) for n in ("n", "Ht", "Wt", "F", "V", "B", "S", "N")] +
                [(n, _f) for n in ("depth_tol", "cos_min", "cos_power", "shade_floor")])


# the frames baked into UV space (csrc/bake.hip)
SIGNATURES.update({
    "harp_uv_texel_map": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "harp_texture_bake_accum": (_i, [ctypes.POINTER(BakeArgs), _vp]),
    "harp_texture_bake_finish": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "harp_texture_dilate_ws_bytes": (_sz, [_i, _i, _i]),
    "harp_texture_dilate": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
})

# playback of a fitted avatar (csrc/playback.hip)
SIGNATURES.update({
    "harp_motion_resample": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "harp_resolve_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp]),
})


class Layer(ctypes.Structure):
    """mirror of `harp_layer` (include/harp_hip.h)"""
    _fields_ = [("rgb", _vp), ("zbuf", _vp), ("flip_x", ctypes.c_int32), ("reserved", ctypes.c_int32)]


# several avatars in one frame (csrc/composite.hip)
SIGNATURES["harp_composite_layers_u8"] = (_i, [ctypes.POINTER(Layer), _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp])


class LabelLayer(ctypes.Structure):
    """mirror of `harp_label_layer` (include/harp_hip.h)"""
    _fields_ = ([(n, _vp) for n in ("face_id", "zbuf", "face_label", "ndc", "faces", "verts_uvs", "faces_uvs")] +
                [(n, ctypes.c_int32) for n in ("V", "F", "Vt", "flip_x", "reserved")])


# what the frames show (csrc/annotate.hip)
_llp = ctypes.POINTER(LabelLayer)
SIGNATURES["harp_annotate_layers"] = (_i, [_llp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
SIGNATURES["harp_keypoint_visibility"] = (_i, [_vp, _vp, _vp, _i, _i, _f, _i, _i, _i, _llp, _i, _vp, _i, _vp, _f, _vp, _vp, _vp])


class FlowLayer(ctypes.Structure):
    """mirror of `harp_flow_layer` (include/harp_hip.h)"""
    _fields_ = ([(n, _vp) for n in ("face_id", "zbuf", "face_label", "ndc", "faces", "ndc_to", "zbuf_to")] +
                [(n, ctypes.c_int32) for n in ("V", "F", "flip_x", "reserved")])


# where the surface points of a frame are in another frame (csrc/flow.hip)
SIGNATURES["harp_flow_layers"] = (_i, [ctypes.POINTER(FlowLayer), _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _f, _vp, _vp, _vp, _vp])


class ContactMesh(ctypes.Structure):
    """mirror of `harp_contact_mesh` (include/harp_hip.h)"""
    _fields_ = ([(n, _vp) for n in ("verts", "cam_R", "cam_T", "faces")] + [(n, ctypes.c_int32) for n in ("V", "F", "flip_x", "reserved")])


# per-vertex distance, nearest face and winding number between two meshes (csrc/contact.hip)
SIGNATURES["harp_mesh_contact_ws_floats"] = (_sz, [_i, _i])
SIGNATURES["harp_mesh_contact"] = (_i, [ctypes.POINTER(ContactMesh), ctypes.POINTER(ContactMesh), _i, _f, _vp, _vp, _vp, _vp, _vp])
# the same with a per-(query vertex, target face) exclusion table (self-contact)
SIGNATURES["harp_contact_excl_words"] = (_sz, [_i, _i])
SIGNATURES["harp_mesh_contact_excl"] = (_i, [ctypes.POINTER(ContactMesh), ctypes.POINTER(ContactMesh), _vp, _i, _f, _vp, _vp, _vp, _vp, _vp])


class IkOptions(ctypes.Structure):
    """mirror of `harp_ik_options` (include/harp_hip.h)"""
    _fields_ = [("iters", _i), ("lambda0", _f), ("prior_weight", _f), ("betas_per_frame", _i)]


# batched MANO inverse kinematics (csrc/ik.hip)
SIGNATURES["harp_mano_ik_frames_per_block"] = (_i, [])
SIGNATURES["harp_mano_ik"] = (_i, [_mp, _vp, _vp, _vp, _vp, _i, ctypes.POINTER(IkOptions), _vp, _vp, _vp, _vp, _vp, _vp, _vp])

# motion smoothing: the confidence-weighted rotation-aware window filter (csrc/filter.hip)
FILTER_MAX_RADIUS = 64                                     # HARP_FILTER_MAX_RADIUS
SIGNATURES["harp_motion_filter"] = (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp])


class VertexFitOptions(ctypes.Structure):
    """mirror of `harp_vertex_fit_options` (include/harp_hip.h)"""
    _fields_ = [("iters", _i), ("lambda0", _f), ("pose_prior_weight", _f), ("shape_prior_weight", _f), ("solve_shape", _i), ("betas_per_frame", _i)]


# batched MANO vertex fit (csrc/vertex_fit.hip)
SIGNATURES["harp_mano_vertex_fit_frames_per_block"] = (_i, [])
SIGNATURES["harp_mano_vertex_fit"] = (_i, [_mp, _vp, _vp, _vp, _i, ctypes.POINTER(VertexFitOptions), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])


class ArmVertexFitOptions(ctypes.Structure):
    """mirror of `harp_arm_vertex_fit_options` (include/harp_hip.h)"""
    _fields_ = [("iters", _i), ("lambda0", _f), ("pose_prior_weight", _f), ("wrist_prior_weight", _f), ("shape_prior_weight", _f),
                ("solve_shape", _i), ("solve_wrist", _i), ("betas_per_frame", _i)]


# batched SMPL-X arm vertex fit (csrc/arm_vertex_fit.hip)
ARM_VERTEX_FIT_MAX_VERTS = 1088                            # HARP_ARM_VERTEX_FIT_MAX_VERTS
SIGNATURES["harp_arm_vertex_fit_frames_per_block"] = (_i, [])
SIGNATURES["harp_arm_vertex_fit"] = (_i, [_trp, _vp, _i, _vp, _vp, _vp, _i, ctypes.POINTER(ArmVertexFitOptions), _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp])


class ArmIkOptions(ctypes.Structure):
    """mirror of `harp_arm_ik_options` (include/harp_hip.h)"""
    _fields_ = [("iters", _i), ("lambda0", _f), ("pose_prior_weight", _f), ("wrist_prior_weight", _f), ("solve_wrist", _i), ("betas_per_frame", _i)]


# batched SMPL-X arm inverse kinematics (csrc/arm_ik.hip)
ARM_IK_MAX_JOINTS = 22                                     # HARP_ARM_IK_MAX_JOINTS
SIGNATURES["harp_arm_ik_frames_per_block"] = (_i, [])
SIGNATURES["harp_arm_ik"] = (_i, [_trp, _vp, _vp, _vp, _vp, _vp, _i, ctypes.POINTER(ArmIkOptions), _vp, _vp, _vp, _vp, _vp, _vp, _vp])


class ReprojIkOptions(ctypes.Structure):
    """mirror of `harp_reproj_ik_options` (include/harp_hip.h)"""
    _fields_ = [("iters", _i), ("lambda0", _f), ("pose_prior_weight", _f), ("z_prior_weight", _f), ("betas_per_frame", _i), ("cam_per_frame", _i),
                ("focal", _f), ("S", _i)]


# batched 2.5-D reprojection inverse kinematics of the MANO hand (csrc/reproj_ik.hip)
SIGNATURES["harp_mano_reproj_ik_frames_per_block"] = (_i, [])
SIGNATURES["harp_mano_reproj_ik"] = (_i, [_mp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, ctypes.POINTER(ReprojIkOptions), _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp])


class ArmReprojIkOptions(ctypes.Structure):
    """mirror of `harp_arm_reproj_ik_options` (include/harp_hip.h)"""
    _fields_ = [("iters", _i), ("lambda0", _f), ("pose_prior_weight", _f), ("wrist_prior_weight", _f), ("z_prior_weight", _f), ("solve_wrist", _i),
                ("betas_per_frame", _i), ("cam_per_frame", _i), ("focal", _f), ("S", _i)]


# batched 2.5-D reprojection inverse kinematics of the SMPL-X arm (csrc/arm_reproj_ik.hip)
SIGNATURES["harp_arm_reproj_ik_frames_per_block"] = (_i, [])
SIGNATURES["harp_arm_reproj_ik"] = (_i, [_trp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, ctypes.POINTER(ArmReprojIkOptions), _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp])
