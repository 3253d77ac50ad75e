"""TEST INFRASTRUCTURE ONLY — CPU oracle, part 2: restatement of HARP's render-and-compare path.

Only `tests/`, `__graft_entry__.smoke()` and `bench.py`'s `cpu_baseline` leg may import this.
Each function cites the reference file:line it follows (paths relative to /root/reference).
Same structure as the reference: materialised (B,S,S,K) fragments (oracle.p3d_like), torch autograd
for the backward pass, torch.optim.Adam for the update.

Pinning status:
  * mano_forward / batch_rodrigues, kps_loss, arap_loss, albedo_reg / normal_reg are PINNED against
    the reference itself (imported in the build container by tests/golden/make_golden.py; vectors in
    tests/golden/*.npz; checked by tests/test_oracle_golden.py).
  * everything that goes through PyTorch3D (rasteriser, blending, texture sampling, shading, shadow,
    laplacian, normal consistency) is PARITY UNPINNED (see oracle/p3d_like.py header).
"""
import math

import torch
import torch.nn.functional as F

from . import p3d_like as P


# ----------------------------------------------------------------------------------------------
# MANO layer  (manopth/manolayer.py:108-296, rodrigues_layer.py:15-54, tensutils.py:6-42)
# ----------------------------------------------------------------------------------------------
def quat2mat(quat):
    """rodrigues_layer.py:15-40"""
    nq = quat / quat.norm(p=2, dim=1, keepdim=True)
    w, x, y, z = nq[:, 0], nq[:, 1], nq[:, 2], nq[:, 3]
    w2, x2, y2, z2 = w.pow(2), x.pow(2), y.pow(2), z.pow(2)
    wx, wy, wz = w * x, w * y, w * z
    xy, xz, yz = x * y, x * z, y * z
    return torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
                        2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
                        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], dim=1).view(-1, 3, 3)


def batch_rodrigues(axisang):
    """rodrigues_layer.py:43-54 (note norm(axisang + 1e-8))."""
    n = torch.norm(axisang + 1e-8, p=2, dim=1)
    ang = n.unsqueeze(-1)
    axis = axisang / ang
    ang = ang * 0.5
    quat = torch.cat([torch.cos(ang), torch.sin(ang) * axis], dim=1)
    return quat2mat(quat).view(-1, 9)


MANO_TIPS_RIGHT = [745, 317, 444, 556, 673]                              # manolayer.py:270
MANO_JOINT_REORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]  # :279


def _with_zeros(t):
    pad = t.new_tensor([0.0, 0.0, 0.0, 1.0]).view(1, 1, 4).repeat(t.shape[0], 1, 1)
    return torch.cat([t, pad], 1)


def mano_forward(model, pose_coeffs, betas, trans):
    """ManoLayer(use_pca=False, flat_hand_mean=False, side='right').forward (manolayer.py:108-296).
    model: dict of v_template (778,3), shapedirs (778,3,10), posedirs (778,3,135), J_regressor (16,778),
    weights (778,16), hands_mean (45,).  Returns verts (B,778,3) mm, joints (B,21,3) mm."""
    B = pose_coeffs.shape[0]
    full_pose = torch.cat([pose_coeffs[:, :3], model["hands_mean"][None] + pose_coeffs[:, 3:48]], 1)  # :139-143
    rot_map = batch_rodrigues(full_pose.contiguous().view(-1, 3)).view(B, 16 * 9)                   # tensutils.py:6-12
    pose_map = rot_map - torch.eye(3, dtype=rot_map.dtype).view(1, 9).repeat(B, 16)
    root_rot = rot_map[:, :9].view(B, 3, 3)                                                          # :150-153
    rot_map, pose_map = rot_map[:, 9:], pose_map[:, 9:]
    v_shaped = torch.matmul(model["shapedirs"], betas.transpose(1, 0)).permute(2, 0, 1) + model["v_template"][None]  # :185-187
    th_j = torch.matmul(model["J_regressor"], v_shaped)                                              # :188
    v_posed = v_shaped + torch.matmul(model["posedirs"], pose_map.transpose(0, 1)).permute(2, 0, 1)  # :191-192
    root_j = th_j[:, 0, :].contiguous().view(B, 3, 1)
    root_trans = _with_zeros(torch.cat([root_rot, root_j], 2))                                       # :202
    all_rots = rot_map.view(B, 15, 3, 3)
    l1, l2, l3 = [1, 4, 7, 10, 13], [2, 5, 8, 11, 14], [3, 6, 9, 12, 15]
    r1, r2, r3 = all_rots[:, [i - 1 for i in l1]], all_rots[:, [i - 1 for i in l2]], all_rots[:, [i - 1 for i in l3]]
    j1, j2, j3 = th_j[:, l1], th_j[:, l2], th_j[:, l3]
    transforms = [root_trans.unsqueeze(1)]
    j1_rel = j1 - root_j.transpose(1, 2)
    t1 = _with_zeros(torch.cat([r1, j1_rel.unsqueeze(3)], 3).view(-1, 3, 4))
    root_flt = root_trans.unsqueeze(1).repeat(1, 5, 1, 1).view(B * 5, 4, 4)
    lev1 = torch.matmul(root_flt, t1)
    transforms.append(lev1.view(B, 5, 4, 4))
    t2 = _with_zeros(torch.cat([r2, (j2 - j1).unsqueeze(3)], 3).view(-1, 3, 4))
    lev2 = torch.matmul(lev1, t2)
    transforms.append(lev2.view(B, 5, 4, 4))
    t3 = _with_zeros(torch.cat([r3, (j3 - j2).unsqueeze(3)], 3).view(-1, 3, 4))
    lev3 = torch.matmul(lev2, t3)
    transforms.append(lev3.view(B, 5, 4, 4))
    reorder = [0, 1, 6, 11, 2, 7, 12, 3, 8, 13, 4, 9, 14, 5, 10, 15]                                  # :241
    results = torch.cat(transforms, 1)[:, reorder]
    joint_js = torch.cat([th_j, th_j.new_zeros(B, 16, 1)], 2)
    tmp2 = torch.matmul(results, joint_js.unsqueeze(3))
    results2 = (results - torch.cat([tmp2.new_zeros(B, 16, 4, 3), tmp2], 3)).permute(0, 2, 3, 1)    # :247
    th_T = torch.matmul(results2, model["weights"].transpose(0, 1))                                  # :251
    rest_h = torch.cat([v_posed.transpose(2, 1), v_posed.new_ones(B, 1, v_posed.shape[1])], 1)
    verts = (th_T * rest_h.unsqueeze(1)).sum(2).transpose(2, 1)[:, :, :3]                            # :260-261
    jtr = results[:, :, :3, 3]
    jtr = torch.cat([jtr, verts[:, MANO_TIPS_RIGHT]], 1)[:, MANO_JOINT_REORDER]
    if not bool(torch.norm(trans) == 0):                                                             # :281
        jtr = jtr + trans.unsqueeze(1)
        verts = verts + trans.unsqueeze(1)
    return verts * 1000, jtr * 1000


# ----------------------------------------------------------------------------------------------
# Scene assembly (utils/visualize.py:16-108)
# ----------------------------------------------------------------------------------------------
def prepare_mesh(params, fid, model, topo, use_arm=False):
    """utils/visualize.py:16-88 (MANO branch :42-44 or SMPL-X arm branch :37-40), with subdivision + normal displacement.
    topo: dict with edges0 (E0,2), faces (F,3) long (subdivided). Returns joints (B,21|22,3) m, verts (B,V,3) m."""
    B = fid.shape[0]
    pose_b, rot_b = params["pose"][fid], params["rot"][fid]                                          # :26-27
    if use_arm:
        verts, joints = smplxarm_forward(model, params["shape"].repeat([B, 1]), rot_b, params["trans"][fid], pose_b,
                                         params["wrist_pose"][fid])                                  # :37-40
    else:
        verts, joints = mano_forward(model, torch.cat((rot_b, pose_b), 1), params["shape"].repeat([B, 1]),
                                     params["trans"][fid])                                           # :42-44
    verts, joints = verts / 1000.0, joints / 1000.0                                                  # :45-46
    e = topo["edges0"]
    verts = torch.cat([verts, verts[:, e].mean(2)], 1)                                               # SubdivideMeshes (:52)
    n = P.verts_normals(verts, topo["faces"])
    verts = verts + n * params["verts_disps"].repeat(B, 1, 1)                                        # :58-64
    return joints, verts


def camera_RT(cam, S, focal):
    """utils/visualize.py:268-271 / renderer_helper.py:455-459."""
    T = torch.stack([-cam[:, 1], -cam[:, 2], 2 * focal / (S * cam[:, 0] + 1e-9)], dim=1)
    R = torch.tensor([[-1., 0., 0.], [0., -1., 0.], [0., 0., 1.]], dtype=cam.dtype).repeat(cam.shape[0], 1, 1)
    return R, T


def render_silhouette(verts, faces, cam, S, focal, sigma=1e-7, K=50):
    """render_image(..., silhouette=True) (utils/visualize.py:258-285) with the silhouette renderer of
    renderer_helper.py:33-58. Returns alpha (B,S,S)."""
    R, T = camera_RT(cam, S, focal)
    _, ndc = P.world_to_ndc(verts, R, T, focal, (S / 2.0, S / 2.0), S)
    blur = math.log(1.0 / 1e-4 - 1.0) * sigma
    p2f, zbuf, bary, dists = P.rasterize_meshes(ndc, faces, S, blur, K)
    return P.sigmoid_alpha_blend(p2f, dists, sigma)


def process_info_for_shadow(cam, light_positions, center, S, focal):
    """renderer_helper.py:454-468."""
    cam_R, cam_T = camera_RT(cam, S, focal)
    radius = 1.5
    d = light_positions - center
    pos = center + d * (radius / torch.linalg.norm(d, dim=1, keepdim=True))
    up = torch.tensor([[0.0, 1.0, 0.0]], dtype=cam.dtype)
    light_R = P.look_at_rotation(pos, center, up)
    light_T = -torch.bmm(light_R.transpose(1, 2), pos[:, :, None])[:, :, 0]
    return light_R, light_T, cam_R, cam_T


def _depth_tie(p2f2, zbuf2, tol=1e-5):
    """(test infrastructure) pixels whose nearest and second-nearest face are closer in depth than float32 can order (K=2 fragments)"""
    return (p2f2[..., 1] >= 0) & ((zbuf2[..., 1] - zbuf2[..., 0]).abs() < tol * zbuf2[..., 0].abs())


def compute_tangent(normals):
    """pbr_materials.py:58-77."""
    x, y, z = normals[..., 0], normals[..., 1], normals[..., 2]
    s = (2 * (z >= 0)) - 1.0
    a = -1 / (s + z)
    b = x * y * a
    uv = torch.stack((1 + s * x * x * a, s * b, -s * x, b, s + y * y * a, -y), dim=-1)
    return uv.view(uv.shape[:-1] + (2, 3))


def apply_normal_map(pixel_normals, nm):
    """pbr_materials.py:82-124; nm = sampled normal-map texels (N,H,W,K,3)."""
    tangent = compute_tangent(pixel_normals)
    TBN = torch.cat([-tangent, pixel_normals.unsqueeze(4)], dim=4)
    out = torch.matmul(TBN.transpose(-1, -2).reshape(-1, 3, 3), nm.reshape(-1, 3, 1)).reshape(pixel_normals.shape)
    return F.normalize(out, dim=-1)


def render_rgb(verts, topo, params, cam, S, focal, self_shadow=True, light_positions=None, return_aux=False, flag_ambiguous=False):
    """RGB pass. self_shadow=True: render_image_with_RT + MeshRendererShadow.forward + SoftPhongShaderShadow
    (utils/visualize.py:288-319, renderer_helper.py:331-412, 472-523, 565-592). self_shadow=False: render_image
    with the phong renderer (renderer_helper.py:60-81, 106-190). Returns (B,S,S,3)."""
    B = verts.shape[0]
    dt = verts.dtype
    faces = topo["faces"]
    Fn = faces.shape[0]
    pp = (S / 2.0, S / 2.0)
    if light_positions is None:
        light_positions = params["light_positions"][0].repeat(B, 1)                                 # optimize_sequence.py:453-454
    texture = params["texture"][None, 0].repeat(B, 1, 1, 1)                                          # visualize.py:81
    nmap = F.normalize(params["normal_map"][None, 0].repeat(B, 1, 1, 1), dim=-1)                     # visualize.py:94-99
    vn = P.verts_normals(verts, faces)                                                               # renderer_helper.py:495
    fverts = verts[:, faces].reshape(B * Fn, 3, 3)
    fnorm = vn[:, faces].reshape(B * Fn, 3, 3)
    if self_shadow:
        light_R, light_T, cam_R, cam_T = process_info_for_shadow(cam, light_positions, verts.mean(1), S, focal)
        _, ndc_l = P.world_to_ndc(verts, light_R, light_T, focal, pp, S)
        rl = P.rasterize_meshes(ndc_l, faces, S, 0.0, 2 if flag_ambiguous else 1, return_ambiguous=flag_ambiguous, flag_slivers=False)   # :344 (K=1; K=2 only to see depth ties)
        zbuf_l = rl[1][..., :1]
        amb_l = (rl[4] | _depth_tie(rl[0], rl[1])) if flag_ambiguous else None
        amb = torch.sigmoid(params["amb_ratio"])                                                     # optimize_sequence.py:480
        ambient = amb * torch.ones(1, 3, dtype=dt)                                                   # :435-441
        diffuse_c = 1.0 - ambient
        specular = torch.zeros(1, 3, dtype=dt)
    else:
        cam_R, cam_T = camera_RT(cam, S, focal)
        ambient = torch.full((1, 3), 0.5, dtype=dt)                                                  # :70-73
        diffuse_c = torch.full((1, 3), 0.4, dtype=dt)
        specular = torch.full((1, 3), 0.1, dtype=dt)   # shininess=0 -> pow(.,0)=1 -> constant
    _, ndc = P.world_to_ndc(verts, cam_R, cam_T, focal, pp, S)
    rc = P.rasterize_meshes(ndc, faces, S, 0.0, 2 if flag_ambiguous else 1, return_ambiguous=flag_ambiguous)     # :353
    p2f, zbuf, bary, dists = rc[0][..., :1], rc[1][..., :1], rc[2][..., :1, :], rc[3][..., :1]
    amb_c = (rc[4] | _depth_tie(rc[0], rc[1])) if flag_ambiguous else None
    pix_pos = P.interpolate_face_attributes(p2f, bary, fverts)                                       # :364 / :498
    if self_shadow:
        N_, H, W, Kk, _ = pix_pos.shape
        flat = pix_pos.reshape(N_, H * W * Kk, 3)
        in_light = torch.bmm(flat, light_R) + light_T[:, None, :]                                   # :379-380
        xs, ys = P.view_to_screen_xy(in_light, focal, pp, S)                                         # :382
        xk = xs.round().long().reshape(-1)                                                           # :385
        yk = ys.round().long().reshape(-1)
        bk = torch.arange(B).repeat_interleave(H * W * Kk)
        vis = torch.zeros_like(zbuf_l)
        for ii in (-1, 0, 1):                                                                        # :394-406
            for jj in (-1, 0, 1):
                d_at = zbuf_l[bk, (yk + ii).clamp(0, S - 1), (xk + jj).clamp(0, S - 1), 0].reshape(N_, H, W, Kk)
                aa = in_light.reshape(N_, H, W, Kk, 3)[..., 2] - 0.008
                vis = vis + torch.sigmoid((d_at - aa) * 1000.0)
        vis = vis / 9.0                                                                              # :408
        if flag_ambiguous:
            # (test infrastructure) camera pixels whose colour is not decided at float32 precision: own coverage ambiguous, a shadow tap
            # on a light-view pixel with ambiguous coverage, or a hit point within 2e-3 px of the .round() boundary of the tap index
            fx, fy = xs.detach() - torch.floor(xs.detach()), ys.detach() - torch.floor(ys.detach())
            amb = ((fx - 0.5).abs() < 2e-3) | ((fy - 0.5).abs() < 2e-3)
            for ii in (-1, 0, 1):
                for jj in (-1, 0, 1):
                    amb = amb | amb_l[bk, (yk + ii).clamp(0, S - 1), (xk + jj).clamp(0, S - 1)].reshape(N_, -1)
            amb_c = amb_c | amb.reshape(N_, H, W)
    texels = P.sample_textures_uv(texture, params["verts_uvs"], params["faces_uvs"], p2f, bary, Fn)  # :572
    pix_n = P.interpolate_face_attributes(p2f, bary, fnorm)                                          # :501-503
    nm = P.sample_textures_uv(nmap, params["verts_uvs"], params["faces_uvs"], p2f, bary, Fn)         # pbr_materials.py:110
    if flag_ambiguous:
        with torch.no_grad():
            # branch of the tangent frame (pbr_materials.py:68: s = sign(z), z >= 0 -> +1) on the un-normalised interpolated normal
            amb_c = amb_c | (pix_n[..., 0, 2].abs() < 1e-5 * pix_n[..., 0, :].norm(dim=-1).clamp(min=1e-12))
            # texel boundary of the bilinear footprint: the texture VALUE is continuous there, its derivative w.r.t. uv (hence every
            # geometry gradient of the photometric term) is not
            puv = P.interpolate_face_attributes(p2f, bary, params["verts_uvs"][params["faces_uvs"]].repeat(B, 1, 1))[..., 0, :]
            Ht, Wt = texture.shape[1:3]
            tx, ty = puv[..., 0] * (Wt - 1), (1 - puv[..., 1]) * (Ht - 1)
            amb_c = amb_c | ((tx - tx.round()).abs() < 1e-3) | ((ty - ty.round()).abs() < 1e-3)
    pix_n = apply_normal_map(pix_n, nm)                                                              # :505-511
    diff = P.point_light_diffuse(pix_pos, pix_n, light_positions[:, None, None, None, :], diffuse_c[:, None, None, None, :])
    if flag_ambiguous:
        with torch.no_grad():      # kink of relu(n^ . l^)
            lh = F.normalize(light_positions[:, None, None, None, :] - pix_pos, dim=-1, eps=1e-6)
            amb_c = amb_c | ((F.normalize(pix_n, dim=-1, eps=1e-6) * lh).sum(-1)[..., 0].abs() < 1e-5)
    amb_b = ambient[:, None, None, None, :]
    if self_shadow:
        colors = (amb_b + diff * vis[..., None]) * texels + specular[:, None, None, None, :]        # :517-518
    else:
        colors = (amb_b + diff) * texels + specular[:, None, None, None, :]                          # :188
    img = P.softmax_rgb_blend(colors, p2f, zbuf, dists)                                              # :589-591
    if return_aux:
        aux = {"pix_to_face": p2f, "zbuf": zbuf, "bary": bary}
        if flag_ambiguous:
            aux["ambiguous"] = amb_c
        if self_shadow:
            aux.update(zbuf_light=zbuf_l, vis=vis, light_R=light_R, light_T=light_T)
        return img[..., :3], aux
    return img[..., :3]


# ----------------------------------------------------------------------------------------------
# Losses (loss/*.py, optimize_sequence.py:517-553)
# ----------------------------------------------------------------------------------------------
def kps_loss(gt_kps, pred_kps, use_arm=False):
    """loss/kps_loss.py:4-17."""
    if use_arm:
        pred_kps = pred_kps[:, :21, :]
    gt = gt_kps - gt_kps[:, 0, None, :]
    pr = (pred_kps - pred_kps[:, 0, None, :]) * 1000.0
    return torch.mean((torch.norm(gt - pr, dim=2) / 100.0) ** 2.0)


def arap_loss(verts, ref_verts, edges):
    """loss/arap.py:4-57 on (B,V,3) verts, (1,V,3) reference verts, (E,2) edges."""
    N = verts.shape[0]
    e = edges.long()
    v0, v1 = verts[:, e[:, 0]], verts[:, e[:, 1]]
    r0, r1 = ref_verts[:, e[:, 0]], ref_verts[:, e[:, 1]]
    loss = ((v0 - v1).norm(dim=-1, p=2) * 1000.0 - (r0 - r1).norm(dim=-1, p=2) * 1000.0) ** 2.0
    return (loss * (1.0 / e.shape[0])).sum() / N


def _smooth_reg(tex, dist, uv_mask):
    """loss/texture_reg.py:11-30 / 48-66 with the random integer offsets passed in."""
    t = tex.squeeze(0)
    H, W = t.shape[:2]
    gx, gy = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tx = torch.clamp(gx + dist[:, :, 0], 0, H - 1)
    ty = torch.clamp(gy + dist[:, :, 1], 0, W - 1)
    diff = torch.norm(t - t[tx, ty], p=1, dim=2) / 3.0
    if uv_mask is not None:
        diff = diff * uv_mask.to(diff.dtype)
    return diff.mean()


def albedo_reg(uv_texture, dist, uv_mask=None):
    """loss/texture_reg.py:5-30; dist = torch.normal(0,std,(H,W,2)).to(torch.int)."""
    return _smooth_reg(uv_texture, dist, uv_mask)


def close_to_z_reg(normal_map):
    """loss/texture_reg.py:40-45 (norm over dim=2 of the un-squeezed (1,H,W,3) tensor: SURVEY Appendix C.2)."""
    diff = torch.norm(normal_map - torch.tensor([0.0, 0.0, 1.0], dtype=normal_map.dtype), p=2, dim=2) / 3.0
    return diff.mean()


def normal_reg(normal_map, dist, uv_mask=None):
    """loss/texture_reg.py:33-37."""
    return 0.2 * close_to_z_reg(normal_map) + _smooth_reg(normal_map, dist, uv_mask)


LOSS_WEIGHTS = {"silhouette": 7.0, "kps_anchor": 10.0, "vert_disp_reg": 2.0, "normal": 0.1, "laplacian": 4.0,
                "arap": 0.2, "photo": 1.0, "albedo": 0.5, "normal_reg": 0.1}       # optimize_sequence.py:411-422 (vgg excluded)


def step_losses(params, fid, model, topo, targets, S, focal, ref_verts, dist_albedo, dist_normal,
                coarse=True, app=True, self_shadow=True, use_arm=False, mask_from_render=None):
    """Loop body optimize_sequence.py:446-558 (VGG term excluded: SURVEY §8(f)). Returns (dict, weighted sum,
    aux dict with images)."""
    y_true, y_sil_true, y_sil_col = targets["y_true"][fid], targets["y_sil"][fid], targets["y_sil_col"][fid]
    joints, verts = prepare_mesh(params, fid, model, topo, use_arm=use_arm)
    cam = params["cam"][fid]
    y_sil_pred = render_silhouette(verts, topo["faces"], cam, S, focal)
    raux = None
    if mask_from_render is not None:
        # (tests: the photometric mask of this evaluation is decided from the SAME render — the float32-undecidable pixels the render flags —
        #  instead of by a second, gradient-free render in front of it: mask_from_render(y_pred, render aux, y_sil_col) -> y_sil_col)
        y_pred, raux = render_rgb(verts, topo, params, cam, S, focal, self_shadow=self_shadow, return_aux=True, flag_ambiguous=True)
        y_sil_col = mask_from_render(y_pred.detach(), raux, y_sil_col)
    else:
        y_pred = render_rgb(verts, topo, params, cam, S, focal, self_shadow=self_shadow)
    loss = {}
    if coarse:
        loss["silhouette"] = F.l1_loss(y_sil_true, y_sil_pred)                                      # :519
        loss["kps_anchor"] = kps_loss(params["init_joints"][fid], joints, use_arm=use_arm)          # :524
        loss["vert_disp_reg"] = torch.sum(params["verts_disps"] ** 2.0)                             # :533
        loss["laplacian"] = P.mesh_laplacian_smoothing_uniform(verts, topo["nbr_off"], topo["nbr_idx"])   # :536
        loss["normal"] = P.mesh_normal_consistency(verts, topo["nc_pairs"])                         # :537
        loss["arap"] = arap_loss(verts, ref_verts, topo["edges"])                                   # :539
    if app:
        loss["photo"] = F.l1_loss(y_true * y_sil_col.unsqueeze(-1), y_pred * y_sil_col.unsqueeze(-1))  # :543
        loss["albedo"] = albedo_reg(params["texture"], dist_albedo, params["uv_mask"])              # :552
        loss["normal_reg"] = normal_reg(params["normal_map"], dist_normal, params["uv_mask"])       # :553
    total = sum(l * LOSS_WEIGHTS[k] for k, l in loss.items())                                        # :556-558
    return loss, total, {"y_sil_pred": y_sil_pred, "y_pred": y_pred, "verts": verts, "joints": joints, "render_aux": raux}


# ----------------------------------------------------------------------------------------------
# Perceptual term  (model/vgg.py:10-56, optimize_sequence.py:405, 546-547).  torchvision and the pretrained
# VGG16 file are absent from the build image -> PARITY UNPINNED; restated from the published VGG16 "D"
# configuration (torchvision vgg16.features[0:23]: 3x3 conv pad 1 + ReLU, 2x2/2 max-pool at 4, 9, 16).
# ----------------------------------------------------------------------------------------------
VGG16_CONV_AT = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)
VGG16_TAPS = (3, 8, 15, 22)                 # relu1_2, relu2_2, relu3_3, relu4_3 = last layer of slice1..4


def vgg16_features(filters, x, layers_weights):
    """filters: {layer index: (weight (O,I,3,3), bias (O,))}; x (N,3,H,W) -> (N, L) concatenation of the weighted flattened
    input and tap activations (model/vgg.py:38-56)."""
    rows = [layers_weights[0] * x.flatten(start_dim=1)]
    h, tap = x, 1
    for ix in range(23):
        if ix in VGG16_CONV_AT:
            h = F.conv2d(h, filters[ix][0], filters[ix][1], padding=1)
        elif ix in (4, 9, 16):
            h = F.max_pool2d(h, 2, 2)
        else:
            h = F.relu(h)
        if ix in VGG16_TAPS:
            rows.append(layers_weights[tap] * h.flatten(start_dim=1))
            tap += 1
    return torch.cat(rows, 1)


def perceptual_loss(filters, layers_weights, y_pred, y_true, y_sil_col):
    """optimize_sequence.py:546-547 (weight 1.0, :419)."""
    m = y_sil_col.unsqueeze(-1)
    return F.l1_loss(vgg16_features(filters, (y_pred * m).permute(0, 3, 1, 2), layers_weights),
                     vgg16_features(filters, (y_true * m).permute(0, 3, 1, 2), layers_weights))


# ----------------------------------------------------------------------------------------------
# SMPL-X right-arm layer  (hand_models_harp/body_models.py:2163-2390; smplx.lbs is un-vendored -> PARITY UNPINNED,
# restated from the published smplx/lbs.py algorithm)
# ----------------------------------------------------------------------------------------------
SMPLX_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15, 20, 25, 26, 20, 28, 29, 20, 31, 32,
                 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]
ARM_JOINT_IDX = [21, 52, 53, 54, 71, 40, 41, 42, 72, 43, 44, 45, 73, 49, 50, 51, 74, 46, 47, 48, 75, 19]   # smplx_arm_corr.pkl['mano_joint']


def smplx_batch_rodrigues(rot_vecs):
    """smplx.lbs.batch_rodrigues: I + sin K + (1-cos) K^2 with angle = |r + 1e-8|."""
    angle = torch.norm(rot_vecs + 1e-8, dim=1, keepdim=True)
    rot_dir = rot_vecs / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    rx, ry, rz = torch.split(rot_dir, 1, dim=1)
    zeros = torch.zeros_like(rx)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view(-1, 3, 3)
    ident = torch.eye(3, dtype=rot_vecs.dtype)[None]
    return ident + sin * K + (1 - cos) * torch.bmm(K, K)


def smplxarm_forward(model, betas, global_orient, transl, right_hand_pose, right_wrist_pose, expression=None):
    """SMPLXARM.forward(..., return_type='mano_w_arm') on an ARM-SLICED model dict (the LBS of the other ~9400 body vertices is
    discarded by the reference's final slice, body_models.py:2383-2390, and the joint regressor is folded into J_template /
    J_shapedirs): v_template (Va,3), shapedirs (Va,3,20), posedirs (486, Va*3), J_template (55,3), J_shapedirs (55,3,20),
    weights (Va,55), pose_mean (165,), tip_verts (5,) arm-local ids of the right thumb..pinky tips.
    expression (B,10): the last 10 shape coefficients (None: zeros, as SMPLXARM.forward passes).
    Returns verts (B,Va,3) mm, joints (B,22,3) mm."""
    B = betas.shape[0]
    dt = betas.dtype
    full_pose = torch.zeros(B, 55, 3, dtype=dt)
    full_pose[:, 0] = global_orient                                                   # :2304
    full_pose[:, 21] = right_wrist_pose                                               # body_pose[:, 60:63], :2299-2301
    full_pose[:, 40:55] = right_hand_pose.reshape(B, 15, 3)
    full_pose = full_pose.reshape(B, 165) + model["pose_mean"][None]                  # :2315
    expr = torch.zeros(B, 10, dtype=dt) if expression is None else expression
    shape_components = torch.cat([betas, expr], dim=-1)                               # expression defaults to zeros, :2323
    v_shaped = model["v_template"][None] + torch.einsum("bl,mkl->bmk", shape_components, model["shapedirs"])
    J = model["J_template"][None] + torch.einsum("bl,jkl->bjk", shape_components, model["J_shapedirs"])
    rot_mats = smplx_batch_rodrigues(full_pose.view(-1, 3)).view(B, 55, 3, 3)
    pose_feature = (rot_mats[:, 1:] - torch.eye(3, dtype=dt)).view(B, -1)
    v_posed = v_shaped + torch.matmul(pose_feature, model["posedirs"]).view(B, -1, 3)
    parents = SMPLX_PARENTS
    rel = J.clone()
    rel[:, 1:] = J[:, 1:] - J[:, parents[1:]]
    tm = torch.cat([torch.cat([rot_mats, rel[..., None]], -1), torch.tensor([0., 0., 0., 1.], dtype=dt).expand(B, 55, 1, 4)], -2)
    chain = [tm[:, 0]]
    for i in range(1, 55):
        chain.append(torch.matmul(chain[parents[i]], tm[:, i]))
    transforms = torch.stack(chain, dim=1)
    posed_joints = transforms[:, :, :3, 3]
    jh = torch.cat([J, torch.zeros(B, 55, 1, dtype=dt)], -1)[..., None]
    rel_t = transforms - torch.nn.functional.pad(torch.matmul(transforms, jh), [3, 0])
    T = torch.matmul(model["weights"][None].expand(B, -1, -1), rel_t.view(B, 55, 16)).view(B, -1, 4, 4)
    vh = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1, dtype=dt)], -1)
    verts = torch.matmul(T, vh[..., None])[:, :, :3, 0]
    wrist = posed_joints[:, None, 21, :]
    verts, joints = verts - wrist, posed_joints - wrist                                # :2342-2343
    tips = verts[:, model["tip_verts"].long()]                                         # vertex_joint_selector: joints 71..75
    allj = torch.cat([joints, torch.zeros(B, 16, 3, dtype=dt), tips], 1)               # 55..70 are not selected by ARM_JOINT_IDX
    verts, allj = verts + transl[:, None], allj + transl[:, None]                      # :2378-2380
    return verts * 1000.0, allj[:, ARM_JOINT_IDX] * 1000.0                             # :2383-2390


# ---------------------------------------------------------------------------------------------------------------
# temporal smoothness terms (reference loss/smooth.py:29-131; not called by the main loop — SURVEY.md §8f rank 4).
# Pinned by tests/golden/smooth.npz (generated by importing the reference).
def _neighbour_frames(fid, n_frames):
    """loss/smooth.py:38-39: previous / next frame id, clamped at the boundaries of each n_frames-long sequence"""
    fid_r = torch.where(fid % n_frames == n_frames - 1, fid, fid + 1)
    fid_l = torch.where(fid % n_frames == 0, fid, fid - 1)
    return fid_l, fid_r


def smooth_pose_loss(params, fid, model, n_frames):
    """LossSmoothPoses.smooth_pose (loss/smooth.py:35-73), MANO branch: root-aligned joints (mm) vs the detached mean of the
    (previous, current, next) frames' root-aligned joints, sum of squares / N."""
    N = len(fid)
    fl, fr = _neighbour_frames(fid, n_frames)
    J = []
    for f in (fl, fid, fr):
        _, j = mano_forward(model, torch.cat((params["rot"][f], params["pose"][f]), 1), params["shape"].repeat(N, 1), params["trans"][f])
        J.append(j - j[:, 0:1])
    interp = ((J[0] + J[1] + J[2]) / 3.0).detach()
    return torch.sum((J[1] - interp) ** 2) / N


def smooth_root_loss(params, fid, model, n_frames, focal_length, res):
    """LossSmoothRoots.smooth_root (loss/smooth.py:86-131): camera translation (visualize.py convention without the sign flips) plus
    the DETACHED root joint in metres, vs the detached 3-frame mean."""
    N = len(fid)
    fl, fr = _neighbour_frames(fid, n_frames)
    R = []
    for f in (fl, fid, fr):
        _, j = mano_forward(model, torch.cat((params["rot"][f], params["pose"][f]), 1), params["shape"].repeat(N, 1), params["trans"][f])
        cam = params["cam"][f]
        t = torch.stack([cam[:, 1], cam[:, 2], 2 * focal_length / (res * cam[:, 0] + 1e-9)], dim=1)
        R.append(t + j[:, 0].detach() / 1000.0)
    interp = ((R[0] + R[1] + R[2]) / 3.0).detach()
    return torch.sum((R[1] - interp) ** 2) / N
