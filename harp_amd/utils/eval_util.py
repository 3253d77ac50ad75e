"""Evaluation metrics of the reference's utils/eval_util.py: silhouette IoU, masked-free L1, white-background
fill, Procrustes alignment, MS-SSIM (harp_amd.pytorch_msssim: the HIP kernels of csrc/metrics.hip, so it needs a HIP device) and the
ground-truth vertex loader, and LPIPS (harp_amd.lpips: csrc/lpips.hip) when an `lpips_fn` is given — its pretrained AlexNet + head weights
cannot be shipped, so without one `image_eval` reports LPIPS as None.  IoU and L1 run on whatever device the tensors live on."""
import warnings

import numpy as np
import torch

from .. import ops


def fill_bg(img, mask):
    """utils/eval_util.py:29-32: composite (N,H,W,3) over a white background with a (N,H,W) mask"""
    m = mask.unsqueeze(-1)
    return img * m + (m - 1) * -1.0


def l1_diff(ref_image, ref_mask, pred_image, pred_mask):
    """utils/eval_util.py:35-39: mean |ref - pred| over everything, images in [0,1] (the masks are accepted and ignored, as upstream)"""
    return torch.mean(torch.abs(ref_image - pred_image)).detach().cpu().numpy()


def sil_iou(ref_masks, pred_masks):
    """utils/eval_util.py:42-50: per-image IoU of the >= 0.5 masks, averaged over the batch"""
    r, p = ref_masks >= 0.5, pred_masks >= 0.5
    union = torch.logical_or(r, p).sum([1, 2])
    inter = torch.logical_and(r, p).sum([1, 2])
    return torch.mean(inter / union).detach().cpu().numpy()


def ms_ssim_diff(ref_images, pred_images):
    """utils/eval_util.py:56-60: MS_SSIM(data_range=1, size_average=True, channel=3) of (N,H,W,3) images (HIP tensors; the permuted
    views are read in place)"""
    from ..pytorch_msssim import MS_SSIM
    with torch.no_grad():
        diff = MS_SSIM(data_range=1, size_average=True, channel=3)(ref_images.permute(0, 3, 1, 2), pred_images.permute(0, 3, 1, 2))
    return torch.mean(diff).cpu().numpy()


def lpips_diff(ref_images, pred_images, lpips_fn=None):
    """utils/eval_util.py:51-53: the batch mean of lpips_fn(ref, pred) over (N,H,W,3) images (permuted views, read in place).  As in the
    reference the [0, 1] images go in without `normalize`, so LPIPS reads them as if they were in [-1, 1] (kept on purpose: the numbers stay
    comparable with the reference's eval_results.txt).  lpips_fn: a harp_amd.lpips.LPIPS(net='alex', ...) with its weights."""
    if lpips_fn is None:
        raise ValueError("lpips_diff needs lpips_fn = harp_amd.lpips.LPIPS(net='alex', ...) with pretrained weights (none ship here)")
    with torch.no_grad():
        diff = lpips_fn(ref_images.permute(0, 3, 1, 2), pred_images.permute(0, 3, 1, 2))
    return torch.mean(diff).cpu().numpy()


def image_eval(images_for_eval, device=None, lpips_fn=None):
    """utils/eval_util.py:10-26: dict of lists of (n,H,W[,3]) tensors -> {"Silhouette IoU", "L1", "LPIPS", "MS_SSIM"}.
    MS_SSIM is computed when the images are HIP tensors or `device` names a HIP device (they are copied there); on CPU tensors without
    a device it is None.  Images whose smaller side is <= 160 px (pytorch_msssim asserts there) also give None, with a warning.
    LPIPS (lpips_diff) only with an `lpips_fn`, on `device`, the images' HIP device or else the module's; None without one."""
    ev = {k: torch.vstack(v) for k, v in images_for_eval.items()}
    stat = {"Silhouette IoU": sil_iou(ev["ref_mask"], ev["pred_mask"]),
            "L1": l1_diff(ev["ref_image"], ev["ref_mask"], ev["pred_image"], ev["pred_mask"]),
            "LPIPS": None, "MS_SSIM": None}
    ref, pred = ev["ref_image"], ev["pred_image"]
    dev = torch.device(device) if device is not None else (ref.device if ref.is_cuda else None)
    if dev is not None and dev.type == "cuda":
        if min(ref.shape[1:3]) <= ops.MS_SSIM_MIN_SIDE:
            warnings.warn(f"MS_SSIM left out: images of {ref.shape[1]} x {ref.shape[2]} px (pytorch_msssim needs both sides > {ops.MS_SSIM_MIN_SIDE})")
        else:
            stat["MS_SSIM"] = ms_ssim_diff(ref.to(dev, torch.float32), pred.to(dev, torch.float32))
    if lpips_fn is not None:
        ldev = dev if dev is not None else next(lpips_fn.parameters()).device
        stat["LPIPS"] = lpips_diff(ref.to(ldev, torch.float32), pred.to(ldev, torch.float32), lpips_fn)
    return stat


def load_gt_vert(fid, gt_mesh_dir, dataset="synthetic", start_from_one=False, idx_offset=0):
    """utils/eval_util.py:63-70: the ground-truth MANO vertices (mm, `<num>_manov.xyz`) of frame fid[0], in metres"""
    if dataset != "synthetic":
        raise NotImplementedError("only the 'synthetic' ground-truth layout (as in the reference)")
    num = idx_offset + int(fid[0]) + (1 if start_from_one else 0)
    mano_verts = np.loadtxt("{:s}/{:d}_manov.xyz".format(gt_mesh_dir, num))
    return mano_verts / 1000.0


def align_w_scale(mtx1, mtx2, return_trafo=False):
    """utils/eval_util.py:212-235 (FreiHAND-style Procrustes): align mtx2 (K,3) to mtx1 (K,3) by translation, scale and rotation"""
    from scipy.linalg import orthogonal_procrustes
    mtx1, mtx2 = np.asarray(mtx1, dtype=np.float64), np.asarray(mtx2, dtype=np.float64)
    t1, t2 = mtx1.mean(0), mtx2.mean(0)
    a, b = mtx1 - t1, mtx2 - t2
    s1, s2 = np.linalg.norm(a) + 1e-8, np.linalg.norm(b) + 1e-8
    a, b = a / s1, b / s2
    R, s = orthogonal_procrustes(a, b)
    if return_trafo:
        return R, s, s1, t1 - t2
    return np.dot(b, R.T) * s * s1 + t1
