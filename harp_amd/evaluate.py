"""Everything that looks at a fit: the forward pass through the reference-API mirror (`mirror_render`) and the post-fit evaluation of the
reference's optimize_sequence.py:595-816 (`evaluate_sequence`).  The evaluation is a short driver over a list of parts.  A part owns its
state, sees every batch of frames together with its render (`batch`) and adds its lines to the result once the frames are through
(`finish`); the parts share nothing but that batch and that render, so a switch that is off leaves every other number and file as it is."""
import os
import warnings
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from . import ops
from .bake import bake_texture, pad_texture as pad_map
from .io import encode_png, save_obj
from .renderer import renderer_helper
from .structures import Meshes
from .utils.data_util import _ingest_paths, decode_u8
from .utils.eval_util import EvalUtil, align_w_scale, load_gt_vert, sil_iou
from .utils.visualize import (concat_image_in_dir, get_mesh_subdivider, params_on, prepare_materials, prepare_mesh, render_360, render_360_light,
                              render_image, render_image_with_RT)


def mirror_render(configs, P, fid, hand_layer, sub, device="cuda"):
    """One forward pass of frames `fid` through the reference-API mirror, as the loop body (optimize_sequence.py:452-488), visualize_val
    (:110-154) and the evaluation (:680-708) run it: get_renderers(silh_sigma=1e-7, silh_faces_per_pixel=50), prepare_mesh,
    prepare_materials, the silhouette render, and the image through get_shadow_renderers + render_image_with_RT with self_shadow, else
    render_image with the phong renderer.  P: the parameter dict on `device`.  Call under torch.no_grad().  Returns a namespace with
    y_sil_pred (B,S,S), y_pred (B,S,S,3) float32 and the intermediates (hand_verts, hand_joints (m), faces, textures, meshes, cam, light_positions,
    materials_properties, normal_renderer)."""
    S, focal = int(configs["img_size"]), configs["focal_length"]
    use_arm = bool(configs["use_arm"])
    B = fid.shape[0]
    fd = fid.to(device)
    if configs["share_light_position"]:
        light_positions = P["light_positions"][0].repeat(B, 1)
    else:
        light_positions = P["light_positions"][fd]
    phong_renderer, silhouette_renderer, normal_renderer = renderer_helper.get_renderers(
        image_size=S, light_posi=light_positions, silh_sigma=1e-7, silh_gamma=1e-1, silh_faces_per_pixel=50, device=device)
    hand_joints, hand_verts, faces, textures = prepare_mesh(P, fid, hand_layer, False, sub, False, configs, device=device, use_arm=use_arm)
    materials_properties = prepare_materials(P, B, device=device)
    meshes = Meshes(hand_verts, faces, textures)
    cam = P["cam"][fd]
    y_sil_pred = render_image(meshes, cam, B, silhouette_renderer, S, focal, silhouette=True, device=device)
    if configs["self_shadow"]:
        light_R, light_T, cam_R, cam_T = renderer_helper.process_info_for_shadow(cam, light_positions, hand_verts.mean(1), image_size=S,
                                                                                 focal_length=focal, device=device)
        shadow_renderer = renderer_helper.get_shadow_renderers(image_size=S, light_posi=light_positions, silh_sigma=1e-7, silh_gamma=1e-1,
                                                               silh_faces_per_pixel=50, amb_ratio=torch.sigmoid(P["amb_ratio"]), device=device)
        y_pred = render_image_with_RT(meshes, light_T, light_R, cam_T, cam_R, B, shadow_renderer, S, focal, silhouette=False,
                                      materials_properties=materials_properties, device=device)
    else:
        y_pred = render_image(meshes, cam, B, phong_renderer, S, focal, silhouette=False, materials_properties=materials_properties,
                              device=device)
    return SimpleNamespace(y_sil_pred=y_sil_pred, y_pred=y_pred.float(), hand_verts=hand_verts, hand_joints=hand_joints, faces=faces, textures=textures, meshes=meshes,
                           cam=cam, light_positions=light_positions, materials_properties=materials_properties, normal_renderer=normal_renderer)


EVAL_CHUNK = 64                  # optimize_sequence.py:716: image_eval runs on every 64 frames; the final stats are means of the chunk means


def chunk_mean(values, n, per_frame=None):
    """The reference's averaging of a per-frame metric (image_eval per 64-frame chunk, :713-731, then np.mean over the chunks, :733-738):
    the mean over the EVAL_CHUNK-frame chunks of `n` frames (the last, partial chunk included) of each chunk's mean.  values: (n,) float64
    tensor.  per_frame: None, or for a metric that arrives as per-frame SUMS (L1) the number of elements behind each sum — a chunk's mean
    is then its sum divided by (frames in the chunk * per_frame), one division per chunk as the reference's mean over the chunk's pixels."""
    chunks = [slice(c, min(n, c + EVAL_CHUNK)) for c in range(0, n, EVAL_CHUNK)]
    if per_frame is None:
        return float(np.mean([values[c].mean().item() for c in chunks]))
    return float(np.mean([values[c].sum().item() / ((c.stop - c.start) * per_frame) for c in chunks]))


def write_stats(stats, path):
    """:808-816: the ` %s: %.5f` lines, printed and written to `path` in the dict's order"""
    print("  -- Evaluation --")
    for k, v in stats.items():
        print(" %s: %.5f" % (k, v))
    with open(path, "w") as f_out:
        for k, v in stats.items():
            f_out.write(" %s: %.5f\n" % (k, v))


def write_uv_maps(P, uv_mask, uv_out_dir):
    """:627-654: uv_out/texture.png and uv_out/normal_map.png, both multiplied by the UV mask.  Returns that mask as the (Ht,Wt) float64
    array the files were made with (ones without a mask): the mesh export and the coverage pass use the same one."""
    os.makedirs(uv_out_dir, exist_ok=True)
    tex = P["texture"].cpu().numpy()[0]
    uvm = np.ones(tex.shape[:2]) if uv_mask is None else np.asarray(torch.as_tensor(uv_mask).detach().cpu(), dtype=np.float64)
    Image.fromarray(np.uint8(tex.clip(0, 1) * np.expand_dims(uvm, 2) * 255)).save(os.path.join(uv_out_dir, "texture.png"))
    if "normal_map" in P:
        nm = F.normalize(P["normal_map"], dim=-1).cpu().numpy()
        nm = (nm / 2.0 + 0.5) * np.expand_dims(uvm, 2)
        Image.fromarray(np.uint8(nm[0].clip(0, 1) * 255)).save(os.path.join(uv_out_dir, "normal_map.png"))
    return uvm


Batch = namedtuple("Batch", "fid y_true y_sil_true")          # fid (B,) long on the host; y_true (B,S,S,3), y_sil_true (B,S,S) float32 on the device


def frame_batches(images_dataset, batch_size, S, device="cuda", device_ingest=False):
    """The dataset's items in order, `batch_size` at a time (the last batch may be short), as Batch tuples.  The ground truth comes from
    `images_dataset[i]` -> (fid, y_true (S,S,3), y_sil (S,S,1), ...), or with device_ingest=True from utils.data_util.decode_u8 and
    ops.targets_from_u8(eroded=False) — the same bits, each file decoded once and no erosion computed.  That path needs a dataset with
    paths: the ValueError for one without is raised here, by the call, before the first batch is asked for."""
    n = len(images_dataset)
    spans = [range(lo, min(n, lo + batch_size)) for lo in range(0, n, batch_size)]
    if device_ingest:
        return _batches_from_files(images_dataset, spans, _ingest_paths(images_dataset)[2], device)
    return _batches_from_items(images_dataset, spans, S, device)


def _batches_from_items(images_dataset, spans, S, device):
    for span in spans:
        items = [images_dataset[i] for i in span]
        fid = torch.as_tensor([int(it[0]) for it in items], dtype=torch.long)
        y_true = torch.stack([torch.as_tensor(it[1]) for it in items]).to(device=device, dtype=torch.float32)
        y_sil_true = torch.stack([torch.as_tensor(it[2]) for it in items]).reshape(len(items), S, S).to(device=device, dtype=torch.float32)
        yield Batch(fid, y_true, y_sil_true)


def _batches_from_files(images_dataset, spans, d, device):
    for span in spans:
        fid = torch.arange(span.start, span.stop, dtype=torch.long)                     # ImagesDataset: the item's index is its fid
        rgb_u8, mask_u8 = (torch.from_numpy(a).to(device) for a in decode_u8(images_dataset, fid.tolist()))
        y_true, y_sil_true, _ = ops.targets_from_u8(rgb_u8, mask_u8, d=d, eroded=False)
        yield Batch(fid, y_true, y_sil_true)


def lpips_for(configs, lpips_fn, S, device):
    """The LPIPS module of the evaluation, or None: `lpips_fn` as given, else harp_amd.lpips.LPIPS on configs["lpips_weights"] (a combined
    lpips.LPIPS state-dict path, or a (torchvision alexnet, lpips v0.1 head) path pair); without either there is no LPIPS line (the
    weights cannot be shipped).  Left out with a warning when the image side is below what AlexNet needs."""
    if lpips_fn is None and configs.get("lpips_weights"):
        from .lpips import LPIPS
        lw = configs["lpips_weights"]
        lpips_fn = LPIPS(weights=tuple(lw) if isinstance(lw, (list, tuple)) else lw).to(device)
    if lpips_fn is not None and S < ops.LPIPS_MIN_SIDE:
        warnings.warn(f"LPIPS left out of the evaluation: {S} px images (AlexNet needs a side >= {ops.LPIPS_MIN_SIDE})")
        return None
    return lpips_fn


class ImageMetrics:
    """`Silhouette IoU`, `L1`, `LPIPS`, `MS_SSIM` — the reference's key order, which is why LPIPS lives here.  Per batch one
    ops.image_metrics (csrc/metrics.hip) on y_true / y_pred and the two silhouettes; MS_SSIM is left out with a warning when the image
    side is <= ops.MS_SSIM_MIN_SIDE (the reference would fail pytorch_msssim's assertion there), and then no metrics kernel runs: sil_iou
    and the absolute difference per frame.  LPIPS (harp_amd.lpips, csrc/lpips.hip; utils/eval_util.py:51-53) per frame on the same images,
    [0, 1] without `normalize` as the reference passes them, when lpips_for finds a module.  All four averaged by chunk_mean."""

    def __init__(self, configs, S, lpips_fn=None, device="cuda"):
        self.per_pixel = float(S * S * 3)
        self.with_ms = S > ops.MS_SSIM_MIN_SIDE
        if not self.with_ms:
            warnings.warn(f"MS_SSIM left out of the evaluation: {S} px images (pytorch_msssim needs a side > {ops.MS_SSIM_MIN_SIDE})")
        self.lpips_fn = lpips_for(configs, lpips_fn, S, device)
        self.iou, self.l1, self.ms, self.lp = [], [], [], []

    def batch(self, b, r):
        B = b.fid.shape[0]
        if self.with_ms:
            m = ops.image_metrics(b.y_true, r.y_pred, b.y_sil_true, r.y_sil_pred)
            self.iou.append(m["iou"].cpu())
            self.l1.append(m["l1_sum"].double().cpu())
            self.ms.append(m["ms_ssim"].double().cpu())
        else:
            self.iou.append(torch.stack([torch.as_tensor(sil_iou(b.y_sil_true[i:i + 1], r.y_sil_pred[i:i + 1])) for i in range(B)]).cpu())
            self.l1.append((b.y_true - r.y_pred).abs().double().sum((1, 2, 3)).cpu())
        if self.lpips_fn is not None:
            self.lp.append(self.lpips_fn(b.y_true.permute(0, 3, 1, 2), r.y_pred.permute(0, 3, 1, 2)).reshape(B).double().cpu())

    def finish(self, stats):
        iou = torch.cat(self.iou).double()
        n = iou.shape[0]
        stats["Silhouette IoU"] = chunk_mean(iou, n)
        stats["L1"] = chunk_mean(torch.cat(self.l1), n, per_frame=self.per_pixel)
        if self.lpips_fn is not None:
            stats["LPIPS"] = chunk_mean(torch.cat(self.lp), n)
        if self.with_ms:
            stats["MS_SSIM"] = chunk_mean(torch.cat(self.ms), n)


def load_pose_eval(pose_eval, configs):
    """`pose_eval`, else configs["pose_eval"]: None, the path of an .npz or a dict with any of gt_joints (T,21,3) mm, gt_joint_valid (T,21)
    and gt_verts (T,778,3) m, rows indexed by fid -> None or a dict of host tensors with those keys"""
    pe = pose_eval if pose_eval is not None else configs.get("pose_eval")
    if isinstance(pe, (str, os.PathLike)):
        with np.load(pe) as z:
            pe = {k: z[k] for k in z.files}
    if pe is None:
        return None
    return {k: torch.as_tensor(np.asarray(v)) for k, v in pe.items() if k in ("gt_joints", "gt_joint_valid", "gt_verts")}


class PoseAccuracy:
    """The geometric accuracy on the device (csrc/pose_eval.hip; :760-774 and utils/eval_util.py:166-209) against the ground truth `pe` of
    load_pose_eval.  Per batch one ops.procrustes_align of the first 21 joints (mm, both sets root-aligned, only the valid joints), one of
    the vertices (gathered by right_mano_idx on the arm, else the first 778; with configs["eval_mesh"] and no gt_verts they still come from
    load_gt_vert) and one ops.point_set_fscore of the aligned vertices.  Adds whichever the ground truth allows of `Procrustes-aligned
    joint error (mm)`, `Joint AUC 0-50 mm` (100 thresholds), `Procrustes-aligned vertex error (mm)`, `Vertex AUC 0-50 mm`, `F@5mm`,
    `F@15mm` and writes eval_joint_mm[_test].txt / eval_vert_mm[_test].txt with the per-frame means.  Frames with fewer than 3 valid joints
    are left out of the joint lines."""

    def __init__(self, ctx, pe):
        self.ctx, self.pe = ctx, pe
        self.with_joints = "gt_joints" in pe
        self.with_verts = "gt_verts" in pe or bool(ctx.configs["eval_mesh"])
        self.joint_err, self.vert_err, self.f_scores = [], [], []
        self.joint_pck, self.vert_pck = EvalUtil(21), EvalUtil(778)
        idx = torch.as_tensor(np.asarray(ctx.hand_layer.right_mano_idx)) if ctx.use_arm else torch.arange(778)
        self.vert_idx = idx.to(device=ctx.device, dtype=torch.int32)
        self.f_thr = torch.tensor([0.005, 0.015], dtype=torch.float32, device=ctx.device)        # metres

    def batch(self, b, r):
        if self.with_joints:
            self._joints(b.fid, r.hand_joints)
        if self.with_verts:
            self._verts(b.fid, r.hand_verts)

    def _joints(self, fid, hand_joints):
        pe, device, B = self.pe, self.ctx.device, fid.shape[0]
        gt_j = pe["gt_joints"][fid].to(device=device, dtype=torch.float32)
        gt_j = gt_j - gt_j[:, :1]
        pred_j = hand_joints[:, :21].float() * 1000.0
        pred_j = pred_j - pred_j[:, :1]
        vis = (pe["gt_joint_valid"][fid] == 1).to(device) if "gt_joint_valid" in pe else torch.ones(B, 21, dtype=torch.bool, device=device)
        al_j, err_j, nv = ops.procrustes_align(gt_j, pred_j, valid=vis.float())
        ok = nv >= 3
        self.joint_err.append((torch.nan_to_num(err_j.double()).sum(1) / nv.clamp(min=1))[ok].cpu())
        self.joint_pck.feed_batch(gt_j, vis & ok[:, None], al_j)

    def _verts(self, fid, hand_verts):
        configs, device, B = self.ctx.configs, self.ctx.device, fid.shape[0]
        if "gt_verts" in self.pe:
            gt_v = self.pe["gt_verts"][fid].to(device=device, dtype=torch.float32)
        else:
            gt_v = torch.as_tensor(np.stack([load_gt_vert(fid[i:i + 1], configs["gt_mesh_dir"], dataset="synthetic", start_from_one=True,
                                                          idx_offset=500) for i in range(B)]), dtype=torch.float32).to(device)
        al_v, err_v, _ = ops.procrustes_align(gt_v, hand_verts, pred_idx=self.vert_idx)
        self.vert_err.extend((err_v.double().mean(1) * 1000.0).cpu().tolist())
        self.vert_pck.feed_batch(gt_v * 1000.0, torch.ones(B, 778, device=device), al_v * 1000.0)
        self.f_scores.append(ops.point_set_fscore(gt_v, al_v, self.f_thr)[0][:, :, 2].double().cpu())

    def finish(self, stats):
        joint_err = torch.cat(self.joint_err).tolist() if self.with_joints else []
        if joint_err:
            stats["Procrustes-aligned joint error (mm)"] = float(np.mean(joint_err))
            stats["Joint AUC 0-50 mm"] = float(self.joint_pck.get_measures(0.0, 50.0, 100)[2])
            np.savetxt(os.path.join(self.ctx.base, "eval_joint_mm" + self.ctx.test_name + ".txt"), joint_err)
        if self.vert_err:
            f = torch.cat(self.f_scores).mean(0)
            stats["Procrustes-aligned vertex error (mm)"] = float(np.mean(self.vert_err))
            np.savetxt(os.path.join(self.ctx.base, "eval_vert_mm" + self.ctx.test_name + ".txt"), self.vert_err)
            stats["Vertex AUC 0-50 mm"] = float(self.vert_pck.get_measures(0.0, 50.0, 100)[2])
            stats["F@5mm"], stats["F@15mm"] = float(f[0]), float(f[1])


class HostMeshError:
    """configs["eval_mesh"] without pose ground truth: the reference's per-frame host loop (:760-774), the Procrustes-aligned vertex error
    against `<gt_mesh_dir>/<500 + fid + 1>_manov.xyz` through align_w_scale, also written to eval_vert_mm[_test].txt"""

    def __init__(self, ctx):
        self.ctx, self.vert_err = ctx, []

    def batch(self, b, r):
        ctx = self.ctx
        for i in range(b.fid.shape[0]):
            gt = load_gt_vert(b.fid[i:i + 1], ctx.configs["gt_mesh_dir"], dataset="synthetic", start_from_one=True, idx_offset=500)
            pred = r.hand_verts[i, ctx.hand_layer.right_mano_idx] if ctx.use_arm else r.hand_verts[i, :778]
            err = gt - align_w_scale(gt, pred.detach().cpu().numpy())
            self.vert_err.append(float(np.linalg.norm(err, axis=1).mean()) * 1000.0)

    def finish(self, stats):
        if self.vert_err:
            stats["Procrustes-aligned vertex error (mm)"] = float(np.mean(self.vert_err))
            np.savetxt(os.path.join(self.ctx.base, "eval_vert_mm" + self.ctx.test_name + ".txt"), self.vert_err)


class Panels:
    """panels=True (:710-714, :742-757): per batch one more prepare_mesh(vis_normal=True) + normal render, one ops.panels_u8 and one
    `true | pred | normal | overlay` JPEG per frame, rendered_after_opt[_test]/<fid %04d>.jpg; panel_hook(fid, strip), if given, sees every
    (S, 4S, 3) uint8 strip before it is encoded."""

    def __init__(self, ctx, panel_hook=None):
        self.ctx, self.hook = ctx, panel_hook
        self.dir = os.path.join(ctx.base, "rendered_after_opt" + ctx.test_name)
        os.makedirs(self.dir, exist_ok=True)                       # :660

    def batch(self, b, r):
        c, B = self.ctx, b.fid.shape[0]
        _, verts_n, faces_n, textures_n = prepare_mesh(c.P, b.fid, c.hand_layer, False, c.sub, False, c.configs, device=c.device, vis_normal=True,
                                                       use_arm=c.use_arm)
        y_pred_normal = render_image(Meshes(verts_n, faces_n, textures_n), r.cam, B, r.normal_renderer, c.S, c.focal, silhouette=False,
                                     materials_properties=r.materials_properties, device=c.device)
        strips = ops.panels_u8([b.y_true, r.y_pred, y_pred_normal], b.y_sil_true, r.y_sil_pred).cpu().numpy()
        for i in range(B):
            if self.hook is not None:
                self.hook(int(b.fid[i]), strips[i])
            Image.fromarray(strips[i]).save(os.path.join(self.dir, "%04d.jpg" % int(b.fid[i])))

    def finish(self, stats):
        pass


class Turntable:
    """turntable=True (:716-727): the dataset item whose fid is 0 turned through 360 degrees with the phong and the normal renderer
    (render_360), concat_image_in_dir into render_360_combine, and lit from 40 positions (render_360_light), each with its out.gif."""

    def __init__(self, ctx):
        self.ctx = ctx

    def batch(self, b, r):
        if not bool((b.fid == 0).any()):
            return
        c = self.ctx
        i0 = int((b.fid == 0).nonzero()[0])
        f0 = b.fid[i0:i0 + 1]
        phong0, _, normal0 = renderer_helper.get_renderers(image_size=c.S, light_posi=r.light_positions[i0:i0 + 1], silh_sigma=1e-7,
                                                           silh_gamma=1e-1, silh_faces_per_pixel=50, device=c.device)
        kw360 = dict(configs=c.configs, use_arm=c.use_arm, verts_textures=False, mesh_subdivider=c.sub, global_pose=False, save_img_dir=c.base,
                     device=c.device)
        render_360(c.P, f0, phong0, c.S, c.focal, c.hand_layer, **kw360)
        render_360(c.P, f0, normal0, c.S, c.focal, c.hand_layer, render_normal=True, **kw360)
        concat_image_in_dir(os.path.join(c.base, "render_360"), os.path.join(c.base, "render_360_normal"), os.path.join(c.base, "render_360_combine"))
        render_360_light(c.P, f0, r.hand_verts[i0:i0 + 1], r.faces, r.textures, c.S, c.focal, save_img_dir=c.base, device=c.device)

    def finish(self, stats):
        pass


class MeshExport:
    """export_mesh=True (the reference's constant EXPORT_MESH, :776-791): per batch one ops.taubin_smoothing(meshes) (csrc/smooth.hip) and
    one device -> host copy, then per frame mesh/<fid %04d>.obj, .mtl and .png through harp_amd.io.save_obj with the reference's arguments —
    smoothed vertices, the faces of the unsmoothed mesh, the textures' verts_uvs / faces_uvs and maps_padded()[0].clamp(0, 1).  prepare_mesh
    repeats ONE texture over every frame of every batch, so its PNG is encoded once.  pad_texture=k: that PNG is dilated by k 3 x 3 passes
    from uv_mask > 0.5 into the rest (harp_amd.bake.pad_texture), which removes the dark band a viewer's bilinear lookup pulls across the
    chart borders; 0: the reference's bytes."""

    def __init__(self, ctx, uvm, pad_texture=0):
        self.uvm, self.pad, self.png = uvm, pad_texture, None
        self.dir = os.path.join(ctx.base, "mesh")
        os.makedirs(self.dir, exist_ok=True)                       # :783

    def batch(self, b, r):
        meshes = r.meshes
        smoothed = ops.taubin_smoothing(meshes).verts_padded().cpu()
        faces_cpu = meshes.faces_padded()[0].cpu()
        verts_uvs = meshes.textures.verts_uvs_padded()[0].detach().cpu()
        faces_uvs = meshes.textures.faces_uvs_padded()[0].detach().cpu()
        if self.png is None:
            self.png = encode_png(pad_map(meshes.textures.maps_padded()[0].detach(), self.uvm, self.pad).cpu().clamp(0, 1))
        for i in range(b.fid.shape[0]):
            save_obj(os.path.join(self.dir, "%04d.obj" % int(b.fid[i])), verts=smoothed[i], faces=faces_cpu, verts_uvs=verts_uvs,
                     faces_uvs=faces_uvs, texture_png=self.png)

    def finish(self, stats):
        pass


class Coverage:
    """coverage=True: which texels did the video ever see — one harp_amd.bake.bake_texture pass over the dataset with the fitted parameters
    and delight=True (csrc/bake.hip), after the frames are through.  Writes uv_out/coverage.png (8-bit, min(count, 255): in how many frames
    a texel was observed), uv_out/baked_texture.png (the projective albedo, filled inside the charts) and uv_out/texture_std.png (the
    weighted standard deviation of the observed colours), and adds ` Texel coverage` (the share of uv_mask & covered texels seen at least
    once) as the last line."""

    def __init__(self, ctx, uvm, images_dataset, device_ingest=False):
        self.ctx, self.uvm, self.dataset, self.device_ingest = ctx, uvm, images_dataset, device_ingest

    def batch(self, b, r):
        pass

    def finish(self, stats):
        c, out = self.ctx, os.path.join(self.ctx.base, "uv_out")
        baked = bake_texture(c.configs, dict(c.P, uv_mask=torch.as_tensor(self.uvm)), self.dataset, c.hand_layer, delight=True, device=c.device,
                             device_ingest=self.device_ingest)
        u8 = lambda t: t.detach().float().clamp(0, 1).mul(255).to(torch.uint8).cpu().numpy()      # noqa: E731
        Image.fromarray(baked["count"].clamp(max=255).to(torch.uint8).cpu().numpy()).save(os.path.join(out, "coverage.png"))
        Image.fromarray(u8(baked["texture"][0])).save(os.path.join(out, "baked_texture.png"))
        Image.fromarray(u8(baked["variance"].sqrt())).save(os.path.join(out, "texture_std.png"))
        stats["Texel coverage"] = baked["coverage"]


def evaluate_sequence(configs, params, images_dataset, hand_layer, device="cuda", batch_size=32, uv_mask=None, lpips_fn=None, panels=False,
                      turntable=False, panel_hook=None, export_mesh=False, pose_eval=None, device_ingest=False, coverage=False, pad_texture=0):
    """The post-fit evaluation of optimize_sequence.py:595-816: every dataset item in order, `batch_size` frames per call, re-rendered with
    the fitted `params` through mirror_render and handed to the parts the switches ask for.  Returns the stats dict, prints it and writes
    it as ` %s: %.5f` lines to eval_results[_test].txt under configs["base_output_dir"] (_test: configs["known_appearance"]).
    Always: uv_out/texture.png, uv_out/normal_map.png (write_uv_maps) and `Silhouette IoU`, `L1`, `MS_SSIM` (ImageMetrics).  The rest is
    off by default and leaves every other number and file as it is when off:
    lpips_fn / configs["lpips_weights"]: `LPIPS` (lpips_for, ImageMetrics).
    pose_eval / configs["pose_eval"]: joint and vertex errors, their AUC, `F@5mm`, `F@15mm`; eval_joint_mm[_test].txt, eval_vert_mm[_test].txt
    (load_pose_eval, PoseAccuracy).  Without it configs["eval_mesh"]: the vertex error and eval_vert_mm[_test].txt (HostMeshError).
    panels, panel_hook: rendered_after_opt[_test]/<fid>.jpg (Panels).  turntable: render_360*/ of fid 0 (Turntable).
    export_mesh, pad_texture: mesh/<fid>.obj, .mtl, .png (MeshExport).
    coverage: uv_out/coverage.png, baked_texture.png, texture_std.png and `Texel coverage` (Coverage).
    device_ingest: the ground truth is decoded from the dataset's files (frame_batches); ValueError for a dataset without paths."""
    S, base, use_arm = int(configs["img_size"]), configs["base_output_dir"], bool(configs["use_arm"])
    P = params_on(params, device)
    ctx = SimpleNamespace(configs=configs, P=P, hand_layer=hand_layer, device=device, S=S, focal=configs["focal_length"], use_arm=use_arm, base=base,
                          test_name="_test" if configs["known_appearance"] else "",
                          sub=get_mesh_subdivider(hand_layer, use_arm=use_arm, device=device))
    uvm = write_uv_maps(P, params.get("uv_mask") if uv_mask is None else uv_mask, os.path.join(base, "uv_out"))
    pe = load_pose_eval(pose_eval, configs)
    batches = frame_batches(images_dataset, batch_size, S, device, device_ingest)
    parts = [                                         # this order is the order of the lines
        ImageMetrics(configs, S, lpips_fn, device),
        PoseAccuracy(ctx, pe) if pe is not None else HostMeshError(ctx) if configs["eval_mesh"] else None,
        Panels(ctx, panel_hook) if panels else None,
        Turntable(ctx) if turntable else None,
        MeshExport(ctx, uvm, pad_texture) if export_mesh else None,
        Coverage(ctx, uvm, images_dataset, device_ingest) if coverage else None,
    ]
    parts = [part for part in parts if part is not None]
    with torch.no_grad():
        for batch in batches:
            r = mirror_render(configs, P, batch.fid, hand_layer, ctx.sub, device=device)
            for part in parts:
                part.batch(batch, r)
    stats = {}
    for part in parts:
        part.finish(stats)
    write_stats(stats, os.path.join(base, "eval_results" + ctx.test_name + ".txt"))
    return stats
