"""Mirror of utils/visualize.py: the scene assembly (prepare_mesh :16-88, prepare_materials :91-108, render_image :258-285,
render_image_with_RT :288-319) and the playback helpers of the post-fit pass (change_pose :111-142, render_360 :145-196,
render_360_light :199-228, concat_image_in_dir :322-345, save_gif :349-355) with the reference's signatures, directory and file names.
A turntable is rendered as ONE batch of 72 (or 40) views and quantised on the device (ops.panels_u8); the helpers also return the uint8
stack they wrote (the reference returns None).  `render_with_rotation` is left out: the reference marks it "Currently not used" and it
reads an undefined `idx`."""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..renderer.pbr_materials import PBRMaterials
from ..structures import Meshes, TexturesUV
from ..topology import subdivide_topology  # noqa: F401  (re-export)


class MeshSubdivider:
    """What `get_mesh_subdivider` returns (optimize_sequence.py:67-89): the static topology of the 4-way subdivided template,
    computed ONCE (SubdivideMeshes precomputes the face table too; PyTorch3D still rebuilds edges per call)."""

    def __init__(self, faces0, n_verts0, device):
        from ..synth import build_topology
        import numpy as np
        t = build_topology(np.asarray(faces0.detach().cpu() if torch.is_tensor(faces0) else faces0), n_verts0)
        self.topo = ops.DeviceTopology(t, torch.zeros(1, 2), torch.zeros(t["faces"].shape[0], 3, dtype=torch.int32), device)
        self.faces = self.topo.faces.long()

    def __call__(self, verts_mm_or_m):
        raise TypeError("call prepare_mesh(..., mesh_subdivider=this) — subdivision is fused into the mesh-prep kernels")


def get_mesh_subdivider(hand_layer, use_arm=False, device="cuda"):
    """optimize_sequence.py:67-89"""
    if use_arm:
        return MeshSubdivider(hand_layer.right_arm_faces_tensor, 1026, device)
    return MeshSubdivider(hand_layer.th_faces, 778, device)


def params_on(params, device):
    """the parameter dict with every tensor detached and on `device` (the rest as it is): what prepare_mesh and the renders read under no_grad"""
    return {k: (v.detach().to(device) if torch.is_tensor(v) else v) for k, v in params.items()}


_RAW_TOPO = {}


def raw_topology(mesh_faces, n_verts, device):
    """static tables of the UN-subdivided template (prepare_mesh with mesh_subdivider=None, utils/visualize.py:51-56), built once"""
    import hashlib
    f = torch.as_tensor(mesh_faces).detach().cpu().reshape(-1, 3).contiguous()
    # keyed on the CONTENT of the face table (18 KB for MANO): an address can be reused by another tensor after this one is freed
    key = (hashlib.sha1(f.numpy().tobytes()).hexdigest(), int(n_verts), str(device))
    if key not in _RAW_TOPO:
        from ..synth import build_raw_topology
        if len(_RAW_TOPO) >= 8:                           # a handful of templates at most (hand, arm): bounded
            _RAW_TOPO.pop(next(iter(_RAW_TOPO)))
        t = build_raw_topology(f.numpy(), int(n_verts))
        _RAW_TOPO[key] = ops.DeviceTopology(t, torch.zeros(1, 2), torch.zeros(t["faces"].shape[0], 3, dtype=torch.int32), device)
    return _RAW_TOPO[key]


def prepare_mesh(params, fid, mano_layer, verts_textures, mesh_subdivider, global_pose, configs, device="cuda", vis_normal=False,
                 shared_texture=True, use_arm=False):
    """utils/visualize.py:16-88 for the MANO + UV-texture path HARP runs (verts_textures=False, shared_texture=True, model_type
    'harp').  Returns (hand_joints (B,21,3) m, hand_verts (B,V,3) m, faces (B,F,3), textures)."""
    if configs.get("model_type", "harp") != "harp" or verts_textures:
        raise NotImplementedError("the 'harp' model type with UV textures is the path in scope (SURVEY.md §8)")
    fid = torch.as_tensor(fid).long()
    B = fid.shape[0]
    pose_batch, rot_batch = params["pose"][fid.to(params["pose"].device)], params["rot"][fid.to(params["rot"].device)]   # :26-27 (global_pose forced False, :20)
    trans_batch = params["trans"][fid.to(params["trans"].device)].to(device)
    if use_arm:
        hand_verts, hand_joints = mano_layer(betas=params["shape"].repeat([B, 1]).to(device), global_orient=rot_batch.to(device),
                                             transl=trans_batch, right_hand_pose=pose_batch.to(device),
                                             right_wrist_pose=params["wrist_pose"][fid.to(params["wrist_pose"].device)].to(device),
                                             return_type="mano_w_arm")                                                   # :37-40
    else:
        hand_verts, hand_joints = mano_layer(torch.cat((rot_batch, pose_batch), 1).to(device), params["shape"].repeat([B, 1]).to(device),
                                             trans_batch)                                                                # :42-44
    hand_joints = hand_joints / 1000.0                                                                                   # :46
    if mesh_subdivider is None:                                                                                          # :51-56: the raw template mesh (config C1)
        topo = raw_topology(params["mesh_faces"], hand_verts.shape[1], device)
        vs = hand_verts / 1000.0                                                                                         # :45
    else:
        topo = mesh_subdivider.topo
        vs = ops.subdivide(hand_verts, topo, 1.0 / 1000.0)                                                              # :45, :50-52
    disp = params["verts_disps"]
    if disp is not None:
        if disp.shape[1] != 1:
            raise NotImplementedError("VERT_DISPS_NORMALS=True in the reference (optimize_sequence.py:326): displacement along normals")
        _, hand_verts = ops.normals_displace(vs, disp.to(device), topo)                                                  # :58-64
    else:
        hand_verts = vs
    faces = topo.faces.long()[None].expand(B, -1, -1)
    faces._harp_topo = topo
    uv_map = params["texture"][None, 0].repeat(B, 1, 1, 1).to(device) if shared_texture else params["texture"].to(device)   # :81-83
    textures = TexturesUV(maps=uv_map, faces_uvs=params["faces_uvs"], verts_uvs=params["verts_uvs"])
    return hand_joints, hand_verts, faces, textures


def prepare_materials(params, batch_size, shared_texture=True, device="cuda"):
    """utils/visualize.py:91-108"""
    normal_maps = None
    if "normal_map" in params:
        nm = params["normal_map"][None, 0].repeat(batch_size, 1, 1, 1).to(device) if shared_texture else params["normal_map"].to(device)
        nm = F.normalize(nm, dim=-1)
        normal_maps = TexturesUV(maps=nm, faces_uvs=params["faces_uvs"], verts_uvs=params["verts_uvs"])
    return {"normal_maps": normal_maps}


def _cam_RT(cam, batch_size, img_size, focal_length, device):
    camera_t = torch.stack([-cam[:, 1], -cam[:, 2], 2 * focal_length / (img_size * cam[:, 0] + 1e-9)], dim=1).to(device)   # :268
    R = torch.tensor([[-1., 0., 0.], [0., -1., 0.], [0., 0., 1.]], device=device).repeat(batch_size, 1, 1)                    # :271
    return R, camera_t


def render_image(mesh, cam, batch_size, renderer, img_size, focal_length, silhouette=False, device="cuda", materials_properties=dict()):
    """utils/visualize.py:258-285"""
    materials = PBRMaterials(device=device, shininess=0.0, **materials_properties)
    R, T = _cam_RT(cam, batch_size, img_size, focal_length, device)
    img = renderer(mesh, principal_point=torch.Tensor([(img_size / 2., img_size / 2.)]), focal_length=focal_length, T=T, R=R,
                   materials=materials, image_size=torch.Tensor([(img_size, img_size)]))
    return img[:, :, :, 3] if silhouette else img[:, :, :, 0:3]


def render_image_with_RT(mesh, light_t, light_r, cam_t, cam_r, batch_size, renderer, img_size, focal_length, silhouette=False,
                         materials_properties=dict(), device="cuda"):
    """utils/visualize.py:288-319"""
    materials = PBRMaterials(device=device, shininess=0.0, **materials_properties)
    img = renderer(mesh, principal_point=torch.Tensor([(img_size / 2., img_size / 2.)]), focal_length=focal_length, T=light_t.to(device),
                   R=light_r.to(device), cam_T=cam_t.to(device), cam_R=cam_r.to(device), materials=materials,
                   image_size=torch.Tensor([(img_size, img_size)]))
    return img[:, :, :, 3] if silhouette else img[:, :, :, 0:3]


# the demo pose of change_pose (utils/visualize.py:117-140): 15 joints x 3 axis-angle components, index, middle, pinky, ring, thumb
DEMO_POSE = (0.0, -0.3, 0.7, 0.0, 0.0, -0.1, 0.0, 0.0, 0.0,
             0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0,
             0.0, 0.0, 0.0, 0.2, 0.0, -0.6, -0.0, 0.0, 0.0,
             0.0, -0.2, 0.8, 0.0, 0.0, 0.8, 0.0, 0.0, 0.0,
             0.5, 0.5, 0.1, 0.6, -0.7, 1.0, 0.0, -1.0, 0.1)


def change_pose(params, idx):
    """utils/visualize.py:111-142: frame 0's 45 finger-pose numbers become the demo pose (`idx` is unused there too)"""
    with torch.no_grad():
        params["pose"][0][0:45] = torch.tensor(DEMO_POSE, dtype=params["pose"].dtype, device=params["pose"].device)
    return params


def _axis_rotation(axis, degrees, device):
    """RotateAxisAngle(degrees, axis).get_matrix()[:, :3, :3] of pytorch3d (row vectors: p' = p @ M), float32"""
    a = torch.tensor(float(degrees), dtype=torch.float32, device=device) / 180.0 * np.pi
    c, s, one, zero = torch.cos(a), torch.sin(a), torch.ones((), device=device), torch.zeros((), device=device)
    rows = {"X": (one, zero, zero, zero, c, -s, zero, s, c), "Y": (c, zero, s, zero, one, zero, -s, zero, c),
            "Z": (c, -s, zero, s, c, zero, zero, zero, one)}[axis]
    return torch.stack(rows).reshape(3, 3).t()


def turntable_vertices(hand_verts):
    """The 36 + 36 vertex sets of render_360 (:164-194) for the first mesh of `hand_verts` (B,V,3) -> (72,V,3): 10 degrees about Y applied
    cumulatively to the already rotated vertices in float32, about the centroid of the UNROTATED mesh, then 10 degrees about X continuing
    from where the Y sweep ended."""
    v = hand_verts[0:1].detach().float()
    center = v.mean(dim=1, keepdim=True)
    out = []
    for axis in ("Y", "X"):
        M = _axis_rotation(axis, 10, v.device)
        for _ in range(36):
            v = torch.matmul(v - center, M) + center
            out.append(v[0])
    return torch.stack(out)


def _write_frames(u8, out_dir, names):
    from PIL import Image
    frames = u8.cpu().numpy()
    for img, name in zip(frames, names):
        Image.fromarray(img).save(os.path.join(out_dir, name))
    return frames


def _first_light(renderer, n):
    """the turntable renders n views of ONE frame: a renderer built for a batch keeps its first frame's light"""
    lp = torch.as_tensor(getattr(renderer, "light_posi", ((0.0, 0.0, 0.0),)), dtype=torch.float32).reshape(-1, 3)
    if lp.shape[0] in (1, n) or not hasattr(renderer, "light_posi"):
        return renderer
    import copy
    r = copy.copy(renderer)
    r.light_posi = lp[0:1]
    return r


def render_360(params, fid, renderer, img_size, focal_length, mano_layer, configs, render_normal=False, verts_textures=True,
               mesh_subdivider=None, global_pose=False, global_betas=True, device="cuda", save_img_dir=None, use_arm=False):
    """utils/visualize.py:145-196: frame fid[0] turned about its centroid, 36 views about Y (`%04d.jpg`) then 36 about X (`h_%04d.jpg`)
    plus out.gif, under save_img_dir/render_360 (render_360_normal with render_normal).  All 72 views go through `renderer` as one batch.
    Returns the (72,S,S,3) uint8 stack that was written."""
    fid = torch.as_tensor(fid).long().reshape(-1)
    out_dir = os.path.join(save_img_dir, "render_360_normal" if render_normal else "render_360")
    os.makedirs(out_dir, exist_ok=True)
    with torch.no_grad():
        _, hand_verts, faces, textures = prepare_mesh(params, fid[0:1], mano_layer, verts_textures, mesh_subdivider, global_pose, configs=configs,
                                                      device=device, use_arm=use_arm)
        materials_properties = prepare_materials(params, 1, device=device)
        verts = turntable_vertices(hand_verts)
        n = verts.shape[0]
        cam = params["cam"][fid[0:1].to(params["cam"].device)].to(device).expand(n, -1)
        img = render_image(Meshes(verts, faces, textures), cam, n, _first_light(renderer, n), img_size, focal_length, device=device,
                           materials_properties=materials_properties)
        u8 = ops.panels_u8(img)
    frames = _write_frames(u8, out_dir, ["%04d.jpg" % i for i in range(36)] + ["h_%04d.jpg" % i for i in range(36)])
    save_gif(out_dir, os.path.join(out_dir, "out.gif"))
    return frames


def light_sweep_positions(num=40, start=-5.0, end=5.0):
    """the light positions (1, 1, z_k), z_k = start + (end - start) / num * k, of render_360_light (:208-214)"""
    return torch.tensor([(1.0, 1.0, start + (end - start) / num * k) for k in range(num)], dtype=torch.float32)


def render_360_light(params, fid, hand_verts, faces, textures, img_size, focal_length, save_img_dir=None, device="cuda"):
    """utils/visualize.py:199-228: 40 phong renders (no shadow pass, no normal map, as in the reference) of the first mesh with the light
    swept from z = -5 towards +5, `%04d.jpg` + out.gif under save_img_dir/render_360_light, rendered as one batch.  Returns the
    (40,S,S,3) uint8 stack that was written."""
    from ..renderer import renderer_helper
    fid = torch.as_tensor(fid).long().reshape(-1)
    out_dir = os.path.join(save_img_dir, "render_360_light")
    os.makedirs(out_dir, exist_ok=True)
    lights = light_sweep_positions()
    n = lights.shape[0]
    with torch.no_grad():
        cam = params["cam"][fid[0:1].to(params["cam"].device)].to(device).expand(n, -1)
        phong_renderer, _, _ = renderer_helper.get_renderers(image_size=img_size, light_posi=lights, silh_sigma=1e-7, silh_gamma=1e-1,
                                                             silh_faces_per_pixel=50, device=device)
        topo = getattr(faces, "_harp_topo", None)
        mesh = Meshes(hand_verts[0:1].detach().float().expand(n, -1, -1).contiguous(), faces, textures, topo)
        u8 = ops.panels_u8(render_image(mesh, cam, n, phong_renderer, img_size, focal_length, device=device))
    frames = _write_frames(u8, out_dir, ["%04d.jpg" % i for i in range(n)])
    save_gif(out_dir, os.path.join(out_dir, "out.gif"))
    return frames


def _images_in(d):
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".png") or f.endswith(".jpg"))


def concat_image_in_dir(dir1, dir2, out_dir):
    """utils/visualize.py:322-345: the sorted .png / .jpg files of two directories side by side, pair by pair (the longer directory's
    surplus is ignored), as `%04d.jpg` + out.gif under out_dir.  Returns the list of uint8 strips."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    strips = []
    for idx, (f1, f2) in enumerate(zip(_images_in(dir1), _images_in(dir2))):
        strip = np.concatenate([np.asarray(Image.open(f1).convert("RGB")), np.asarray(Image.open(f2).convert("RGB"))], axis=1).astype(np.uint8)
        Image.fromarray(strip).save(os.path.join(out_dir, "%04d.jpg" % idx))
        strips.append(strip)
    save_gif(out_dir, os.path.join(out_dir, "out.gif"))
    return strips


def save_gif(in_dir, outname):
    """utils/visualize.py:349-355 (imageio.mimsave(duration=0.1)) with PIL: the sorted *.jpg of in_dir, 100 ms per frame"""
    from PIL import Image
    frames = [Image.open(f).convert("RGB") for f in sorted(glob.glob(os.path.join(in_dir, "*.jpg")))]
    if not frames:
        raise ValueError(f"no *.jpg under {in_dir}")
    frames[0].save(outname, save_all=True, append_images=frames[1:], duration=100, loop=0)
    return len(frames)
