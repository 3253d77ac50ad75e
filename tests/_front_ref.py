"""Plain float64, differentiable torch reference of the fused per-frame front of a fitting step, MANO path (include/harp_hip.h:
harp_hand_front): from the parameter tables down to what the rasteriser set-up reads.  Nothing is computed here that is not computed by a
piece the suite already holds: the row gathers, the camera row and the colours are `_definition` of tests/test_gpu_frame_glue.py, the hand
layer is oracle.harp_ref.mano_forward, the mesh chain is tests/_chain_ref.chain.  Because every piece is differentiable torch,
torch.autograd.grad on the tables is the reference of every gradient row the fused back (harp_hand_back_bwd) adds to.
The SMPL-X arm path (harp_arm_front, harp_arm_back_bwd) is the same composition with tests/_tree_ref.tree_forward as the skinning layer:
arm_case_tables, arm_rows, arm_front below; total and table_grads serve both."""
import numpy as np
import torch

from oracle import harp_ref as H
from tests import _chain_ref as C
from tests.test_gpu_frame_glue import FOCAL, S, _definition

TABLE_KEYS = ("pose", "rot", "trans", "cam", "shape", "light_positions", "amb_ratio")
ROW_KEYS = ("pose48", "betas", "trans_b", "cam_R", "cam_T", "light_pos", "colors")


def mano_model(model, dtype=torch.float64):
    """the arrays of synth.make_mano_model as oracle.harp_ref.mano_forward wants them: the float32 values the device model holds, in `dtype`"""
    m = {k: torch.from_numpy(np.asarray(model[k], np.float32)).to(dtype) for k in ("v_template", "J_regressor", "weights", "hands_mean")}
    m["v_template"] = m["v_template"].reshape(778, 3)
    m["J_regressor"] = m["J_regressor"].reshape(16, 778)
    m["weights"] = m["weights"].reshape(778, 16)
    m["hands_mean"] = m["hands_mean"].reshape(45)
    m["shapedirs"] = torch.from_numpy(np.asarray(model["shapedirs"], np.float32)).to(dtype).reshape(778, 3, 10)
    m["posedirs"] = torch.from_numpy(np.asarray(model["posedirs"], np.float32)).to(dtype).reshape(778, 3, 135)
    return m


def case_tables(model, T=7):
    """float32 tables of T rows at the rotation edges of the skinning tests: every (row, joint) takes an angle of `_rotations`
    (tests/test_gpu_geometry_terms.py: 0, 1e-7 ... about pi, 2 pi, 3 pi, 10 rad), the assignment shifted per TABLE ROW so that a row mix-up
    changes the answer; where the angle is exactly 0 the finger pose is -hands_mean.  Every row has its own cam, trans and light position;
    the shape has components at +3 and -3."""
    from tests.test_gpu_geometry_terms import _rotations
    g = torch.Generator().manual_seed(41)
    hm = torch.from_numpy(np.asarray(model["hands_mean"], np.float32)).reshape(15, 3)
    aa = _rotations(T, 16, g)
    pose = aa.clone()
    pose[:, 1:] -= hm.double()
    pose = pose.float()
    zero = (aa == 0).all(-1)
    pose[:, 1:][zero[:, 1:]] = -hm.expand(T, 15, 3)[zero[:, 1:]]
    shape = torch.randn(10, generator=g).float()
    shape[0], shape[3] = 3.0, -3.0
    return dict(pose=pose[:, 1:].reshape(T, 45).contiguous(), rot=pose[:, 0].contiguous(), trans=(torch.randn(T, 3, generator=g) * 0.05).float(),
                cam=torch.tensor([1.1, 0.02, -0.03]) + torch.randn(T, 3, generator=g) * 0.05, shape=shape,
                light_positions=(torch.randn(T, 3, generator=g) * 0.5 + torch.tensor([0.2, -0.9, -0.4])).float(), amb_ratio=torch.tensor([0.3]))


def rows(tb, fid, share_light, self_shadow):
    """stage 1, the frame set-up: `_definition` + the constant camera rotation diag(-1, -1, 1) of the camera convention"""
    r = _definition(tb, fid, False, share_light, self_shadow)
    B = fid.shape[0]
    r["cam_R"] = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=r["cam_T"].dtype)).repeat(B, 1, 1)
    return r


def front(tb, fid, disp, edges0, faces, model, share_light, self_shadow, mm=1e-3, centroid_value=None):
    """tb: the tables (TABLE_KEYS), fid (B,) integer, disp (V,), edges0 (E0,2) / faces (F,3) long of the subdivided template, model: mano_model().
    Returns the gathered rows (ROW_KEYS), verts_mm (B,778,3), joints_mm (B,21,3) and every output of the mesh chain (C.FWD_KEYS).
    S and FOCAL are those of `_definition`; mm and centroid_value as in tests/_chain_ref.chain."""
    out = rows(tb, fid, share_light, self_shadow)
    out["verts_mm"], out["joints_mm"] = H.mano_forward(model, out["pose48"], out["betas"], out["trans_b"])
    out.update(C.chain(out["verts_mm"], out["joints_mm"], out["cam_R"], out["cam_T"], out["light_pos"], disp, edges0, faces, S, FOCAL, mm=mm,
                       centroid_value=centroid_value))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# SMPL-X arm path (include/harp_hip.h: harp_arm_front): the same composition with the kinematic-tree layer tests/_tree_ref.tree_forward
# ----------------------------------------------------------------------------------------------------------------------------------
ARM_TABLE_KEYS = TABLE_KEYS + ("wrist_pose",)
ARM_ROW_KEYS = ("pose_in", "betas", "trans_b", "cam_R", "cam_T", "light_pos", "colors")
# seed and finger assignment of arm_case_tables per model.  The production arm's are chosen so that the clamp-margin condition of
# tests/test_front_ref_cpu.py holds on all seven rows (one pair of some 600 x 15 tried does); the mesh of a synthetic tree is nowhere near it
ARM_CASE = dict(arm=dict(seed=650, finger_shift=6), twig=dict(seed=41, finger_shift=0), crown=dict(seed=41, finger_shift=0))


def arm_case_tables(host, T=7, seed=41, finger_shift=0):
    """case_tables for a tree model (tests/_tree_ref.py host model): the rotation edges of `_rotations` on the 17 driven joints, shifted per
    table ROW; in_pose = -pose_mean where the angle is exactly 0; every row its own cam / trans / light / wrist_pose; shape at +-3.
    finger_shift rotates the assignment of the angles among the 15 finger rows (2..16)."""
    from tests.test_gpu_geometry_terms import _rotations
    g = torch.Generator().manual_seed(seed)
    src = host["pose_src"]
    joint_of_row = [src.index(r) for r in range(17)]
    pm = torch.from_numpy(host["pose_mean"])[joint_of_row]                 # (17,3) float32
    aa = _rotations(T, 17, g)
    aa = torch.cat([aa[:, :2], torch.roll(aa[:, 2:], finger_shift, 1)], 1)
    in_pose = (aa - pm.double()).float()
    zero = (aa == 0).all(-1)
    in_pose[zero] = -pm.expand(T, 17, 3)[zero]
    shape = torch.randn(10, generator=g).float()
    shape[0], shape[3] = 3.0, -3.0
    return dict(pose=in_pose[:, 2:].reshape(T, 45).contiguous(), rot=in_pose[:, 0].contiguous(), wrist_pose=in_pose[:, 1].contiguous(),
                trans=(torch.randn(T, 3, generator=g) * 0.05).float(), cam=torch.tensor([1.1, 0.02, -0.03]) + torch.randn(T, 3, generator=g) * 0.05,
                shape=shape, light_positions=(torch.randn(T, 3, generator=g) * 0.5 + torch.tensor([0.2, -0.9, -0.4])).float(),
                amb_ratio=torch.tensor([0.3]))


def arm_rows(tb, fid, NB, share_light, self_shadow):
    """`_definition` of the arm rows + the constant camera rotation: pose_in (B,51) = [rot, wrist_pose, pose], betas (B,NB) = shape padded
    with zeros"""
    r = _definition(tb, fid, True, share_light, self_shadow)
    B = fid.shape[0]
    r["pose_in"] = r.pop("pose48")
    r["betas"] = torch.cat([r["betas"][:, :10], r["betas"].new_zeros(B, NB - 10)], 1)
    r["cam_R"] = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=r["cam_T"].dtype)).repeat(B, 1, 1)
    return r


def arm_front(tb, fid, disp, edges0, faces, model, share_light, self_shadow, mm=1e-3, centroid_value=None):
    """`front` for the arm path: model is tests/_tree_ref.model64(host); returns ARM_ROW_KEYS, verts_mm (B,NV,3), joints_mm (B,n_out,3) and
    the mesh chain's outputs"""
    from tests import _tree_ref as TR
    out = arm_rows(tb, fid, model["shapedirs"].shape[-1], share_light, self_shadow)
    out["verts_mm"], out["joints_mm"] = TR.tree_forward(model, out["pose_in"].view(fid.shape[0], 17, 3), out["betas"], out["trans_b"])
    out.update(C.chain(out["verts_mm"], out["joints_mm"], out["cam_R"], out["cam_T"], out["light_pos"], disp, edges0, faces, S, FOCAL, mm=mm,
                       centroid_value=centroid_value))
    return out


def total(out, cot, g_colors=None, shadow=True, normal_grad=True):
    """sum of <cotangent, output> over the outputs the fused back differentiates: cot has g_ndc_c, g_vd, g_joints_m and, shadow, g_ndc_l,
    g_light_R, g_light_T, normal_grad, g_n2 (the names of harp_mesh_chain); g_colors (9,) is the shader's dL/d colours"""
    pairs = [("ndc_c", "g_ndc_c"), ("vd", "g_vd"), ("joints_m", "g_joints_m")]
    if shadow:
        pairs += [("ndc_l", "g_ndc_l"), ("light_R", "g_light_R"), ("light_T", "g_light_T")]
    if normal_grad:
        pairs += [("n2", "g_n2")]
    t = sum((out[a].reshape(cot[b].shape) * cot[b].to(out[a].dtype)).sum() for a, b in pairs)
    if g_colors is not None:
        t = t + (out["colors"] * g_colors.to(out["colors"].dtype)).sum()
    return t


def table_grads(tb, disp, fn):
    """autograd of the scalar fn(leaves, disp_leaf) with respect to every table and disp: dict g_<table> / g_disp, zeros where unused"""
    leaves = {k: v.detach().clone().requires_grad_() for k, v in tb.items()}
    dl = disp.detach().clone().requires_grad_()
    gr = torch.autograd.grad(fn(leaves, dl), list(leaves.values()) + [dl], allow_unused=True)
    out = {"g_" + k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(leaves.items(), gr[:-1])}
    out["g_disp"] = torch.zeros_like(dl) if gr[-1] is None else gr[-1]
    return out
