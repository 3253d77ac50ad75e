"""Evaluation metrics of the reference's utils/eval_util.py: silhouette IoU, masked-free L1, white-background
fill, Procrustes alignment, EvalUtil (PCK / AUC / end-point error) and eval_procrustes, MS-SSIM (harp_amd.pytorch_msssim: the HIP kernels of csrc/metrics.hip, so it needs a HIP device) and the
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
    """utils/eval_util.py:212-235 (FreiHAND-style Procrustes): align mtx2 (K,3) to mtx1 (K,3) by translation, scale and rotation.
    HIP tensors, (K,3) or a batch (N,K,3), go through ops.procrustes_align (csrc/pose_eval.hip) and come back as float32 tensors; with
    return_trafo the reference's tuple (R, s, s1, t1 - t2) of float64 tensors — for a batch a list of one tuple per frame."""
    if torch.is_tensor(mtx1) and mtx1.is_cuda:
        out = ops.procrustes_align(mtx1, torch.as_tensor(mtx2).to(mtx1.device), return_trafo=return_trafo)
        if not return_trafo:
            return out[0]
        tr = out[3]
        unpack = lambda t: (t[:9].reshape(3, 3), t[9], t[10], t[11:14])
        return unpack(tr) if tr.dim() == 1 else [unpack(t) for t in tr]
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


def align_by_trafo(mtx, trafo):
    """utils/eval_util.py:238-242: apply the tuple of align_w_scale(..., return_trafo=True) to another point set (K,3) — NumPy arrays, or
    tensors (float64 arithmetic on the tensor's device; a batch (N,K,3) takes the list of per-frame tuples)"""
    if torch.is_tensor(mtx):
        m = mtx.double()
        if m.dim() == 3:
            R, s, s1, t1 = (torch.stack([torch.as_tensor(t[i], dtype=torch.float64).to(m.device) for t in trafo]) for i in range(4))
            s, s1, t1 = s[:, None, None], s1[:, None, None], t1[:, None, :]
        else:
            R, s, s1, t1 = (torch.as_tensor(x, dtype=torch.float64).to(m.device) for x in trafo)
        t2 = m.mean(-2, keepdim=True)
        return torch.matmul(m - t2, R.transpose(-1, -2)) * s * s1 + t1 + t2
    t2 = mtx.mean(0)
    mtx_t = mtx - t2
    R, s, s1, t1 = trafo
    return np.dot(mtx_t, R.T) * s * s1 + t1 + t2


def _trapezoid(y, x):
    """np.trapz as the reference calls it (the name left NumPy in 2.x)"""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return float(np.sum((y[1:] + y[:-1]) * 0.5 * np.diff(x)))


class EvalUtil:
    """utils/eval_util.py:73-163: collects per-keypoint end-point errors and reports their mean, median, PCK curve and its AUC.
    `feed` is the reference's (one frame, NumPy, kept on the host).  `feed_batch` takes (n,K,3) / (n,K) / (n,K,3) tensors, forms the
    distances where the tensors live and keeps them there; on a HIP device get_measures then counts through ops.pck_counts
    (csrc/pose_eval.hip) and sorts for the median on the device.  One instance holds host data or device data, not both."""

    def __init__(self, num_kp=21):
        self.num_kp = num_kp
        self.data = [list() for _ in range(num_kp)]
        self._batches = []                                   # (dist (n,K) float32, vis (n,K) bool) on one HIP device

    def feed(self, keypoint_gt, keypoint_vis, keypoint_pred, skip_check=False):
        """:83-101: stores the euclidean distance between gt and pred of every visible keypoint of one frame"""
        if self._batches:
            raise RuntimeError("this EvalUtil already holds device data (feed_batch): use one kind of feeding")
        if not skip_check:
            keypoint_gt = np.squeeze(keypoint_gt)
            keypoint_pred = np.squeeze(keypoint_pred)
            keypoint_vis = np.squeeze(keypoint_vis).astype("bool")
            assert len(keypoint_gt.shape) == 2
            assert len(keypoint_pred.shape) == 2
            assert len(keypoint_vis.shape) == 1
        diff = keypoint_gt - keypoint_pred
        euclidean_dist = np.sqrt(np.sum(np.square(diff), axis=1))
        for i in range(keypoint_gt.shape[0]):
            if keypoint_vis[i]:
                self.data[i].append(euclidean_dist[i])

    def feed_batch(self, gt, vis, pred):
        """n frames at once: gt / pred (n,K,3), vis (n,K) (non-zero = visible).  A NaN distance is never counted."""
        gt, pred, vis = torch.as_tensor(gt), torch.as_tensor(pred), torch.as_tensor(vis)
        if gt.dim() != 3 or gt.shape != pred.shape or gt.shape[1] != self.num_kp or tuple(vis.shape) != tuple(gt.shape[:2]):
            raise ValueError(f"feed_batch takes (n,{self.num_kp},3), (n,{self.num_kp}), (n,{self.num_kp},3), got {tuple(gt.shape)}, "
                             f"{tuple(vis.shape)}, {tuple(pred.shape)}")
        with torch.no_grad():
            d = gt.detach().float() - pred.detach().float().to(gt.device)
            dist = (d * d).sum(-1).sqrt()
            seen = (vis.to(gt.device) != 0) & ~torch.isnan(dist)
        if not gt.is_cuda:
            if self._batches:
                raise RuntimeError("this EvalUtil already holds device data: feed it tensors of that device")
            dist, seen = dist.numpy(), seen.numpy()
            for i in range(self.num_kp):
                self.data[i].extend(dist[seen[:, i], i].tolist())
            return
        if any(self.data) or (self._batches and self._batches[0][0].device != dist.device):
            raise RuntimeError("this EvalUtil already holds data of another device")
        self._batches.append((dist, seen))

    def _get_pck(self, kp_id, threshold):
        if len(self.data[kp_id]) == 0:
            return None
        data = np.array(self.data[kp_id])
        return np.mean((data <= threshold).astype("float"))

    def _get_epe(self, kp_id):
        if len(self.data[kp_id]) == 0:
            return None, None
        data = np.array(self.data[kp_id])
        return np.mean(data), np.median(data)

    def get_measures(self, val_min, val_max, steps):
        """:122-163: (epe_mean_all, epe_median_all, auc_all, pck_curve_all, thresholds) over np.linspace(val_min, val_max, steps); a
        keypoint that was never visible is skipped.  steps < 2 raises (the reference divides by a zero span there)."""
        if int(steps) < 2:
            raise ValueError("get_measures needs at least 2 thresholds (the AUC is normalised by their span)")
        thresholds = np.array(np.linspace(val_min, val_max, steps))
        norm_factor = _trapezoid(np.ones_like(thresholds), thresholds)
        if self._batches:
            epe_mean, epe_median, curves = self._device_measures(thresholds)
        else:
            epe_mean, epe_median, curves = [], [], []
            for part_id in range(self.num_kp):
                mean, median = self._get_epe(part_id)
                if mean is None:
                    continue
                epe_mean.append(mean)
                epe_median.append(median)
                curves.append(np.array([self._get_pck(part_id, t) for t in thresholds]))
        auc_all = [_trapezoid(c, thresholds) / norm_factor for c in curves]
        return (np.mean(np.array(epe_mean)), np.mean(np.array(epe_median)), np.mean(np.array(auc_all)), np.mean(np.array(curves), 0),
                thresholds)

    def _device_measures(self, thresholds):
        dist = torch.cat([b[0] for b in self._batches])
        seen = torch.cat([b[1] for b in self._batches])
        thr = torch.as_tensor(thresholds, dtype=torch.float32, device=dist.device)
        counts, n_vis, err_sum = ops.pck_counts(dist, seen.float(), thr)
        # median (NumPy's rule: the mean of the two middle values) from one sort per column, unseen entries pushed to the end
        srt, _ = torch.sort(torch.where(seen, dist, torch.full_like(dist, float("inf"))), dim=0)
        nv = n_vis.long().clamp(min=1)
        lo, hi = srt.gather(0, ((nv - 1) // 2)[None]), srt.gather(0, (nv // 2)[None])
        median = ((lo.double() + hi.double()) * 0.5)[0].cpu().numpy()
        counts, n_vis, err_sum = counts.cpu().numpy().astype(np.float64), n_vis.cpu().numpy(), err_sum.cpu().numpy()
        keep = n_vis > 0
        n = n_vis[keep].astype(np.float64)
        return list(err_sum[keep] / n), list(median[keep]), list(counts[keep] / n[:, None])


def eval_procrustes(images_dataset, params, input_params, mano_layer, global_pose=False, average_pose=False, device="cuda", batch_size=32):
    """What utils/eval_util.py:166-209 set out to do: the mean Procrustes-aligned joint error (mm) of the fitted hand against
    input_params["gt_joints"] (T,21,3) mm with input_params["gt_joint_valid"] (T,21), `batch_size` frames per hand-layer call and one
    ops.procrustes_align (csrc/pose_eval.hip) per batch.  global_pose uses pose row 0 for every frame, average_pose the mean pose.  Joints
    (mm) come from the hand layer; both sets are root-aligned; only joints with gt_joint_valid == 1 enter the alignment and the error;
    frames with fewer than 3 such joints are left out.  Returns {"mean_mm", "per_frame_mm", "n_frames"} and prints the reference's line.
    Two defects of the reference are not reproduced: it reads `root_aligned_pred` before ever defining it (:198), and it unpacks three
    items from a dataset that yields four (:169), so it cannot run as shipped."""
    gt_all = torch.as_tensor(input_params["gt_joints"], dtype=torch.float32)
    valid_all = torch.as_tensor(input_params["gt_joint_valid"])
    per_frame = []
    n = len(images_dataset)
    with torch.no_grad():
        for lo in range(0, n, batch_size):
            fid = torch.as_tensor([int(images_dataset[i][0]) for i in range(lo, min(n, lo + batch_size))], dtype=torch.long)
            B = fid.shape[0]
            pose, rot, trans = params["pose"].detach(), params["rot"].detach(), params["trans"].detach()
            if global_pose:
                pose_batch = pose[0].repeat(B, 1)
            elif average_pose:
                pose_batch = pose.mean(dim=0).repeat(B, 1)
            else:
                pose_batch = pose[fid.to(pose.device)]
            _, hand_joints = mano_layer(torch.cat((rot[fid.to(rot.device)].to(device), pose_batch.to(device)), 1),
                                        params["shape"].detach().repeat([B, 1]).to(device), trans[fid.to(trans.device)].to(device))
            target = gt_all[fid].to(device)
            target = target - target[:, :1]
            pred = hand_joints[:, :21].float()
            pred = pred - pred[:, :1]
            valid = (valid_all[fid] == 1).to(device)
            _, err, n_valid = ops.procrustes_align(target, pred, valid=valid.float())
            frame = torch.nan_to_num(err.double()).sum(1) / n_valid.clamp(min=1)
            per_frame.extend(frame[n_valid >= 3].cpu().tolist())
    mean = float(np.mean(per_frame)) if per_frame else float("nan")
    print("Mean Procrustes-aligned joint error of %d samples: %.3f mm" % (len(per_frame), mean))
    return {"mean_mm": mean, "per_frame_mm": per_frame, "n_frames": len(per_frame)}
