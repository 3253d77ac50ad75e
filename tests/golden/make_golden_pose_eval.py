"""Generate the golden vectors of the geometric evaluation by IMPORTING THE REFERENCE's utils/eval_util.py in the build container.

    python tests/golden/make_golden_pose_eval.py          # needs /root/reference (absent on the GPU box), numpy and scipy

The reference module imports `lpips` and `pytorch_msssim` at the top and builds an LPIPS network on 'cuda' (:3-8); neither package is
needed for what is recorded here, so both are stubbed before the import.  Writes pose_eval_ref.npz (data only) next to this script:
  seeded float32 inputs (stored as float32; the reference is fed their float64 values, so that every recorded output is the float64
  arithmetic of the reference on exactly the numbers the tests feed), and per case `<name>_*`
    gt, pred            the inputs, mm
    aligned             align_w_scale(gt, pred)                          (:212-235)
    R, s, s1, t         align_w_scale(gt, pred, return_trafo=True)
    by_trafo            align_by_trafo(pred, that tuple)                 (:238-242)
  cases: K = 21 at noise 0.5, 3 and 8 mm; a mirrored prediction; K = 4; K = 3; K = 778 translated by (5, -7, 300) and scaled by 1.2
  pck_gt, pck_vis, pck_pred (7,21,3) / (7,21) and the tuple of EvalUtil.get_measures(0, 50, 20) after 7 feeds with about 20 % of the joints
  invisible and joint 13 never visible: pck_epe_mean, pck_epe_median, pck_auc, pck_curve, pck_thresholds."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def import_reference():
    class _Anything:
        def __init__(self, *a, **k):
            pass

        def to(self, *a, **k):
            return self
    lp = types.ModuleType("lpips")
    lp.LPIPS = _Anything
    ms = types.ModuleType("pytorch_msssim")
    ms.ssim = ms.ms_ssim = ms.SSIM = ms.MS_SSIM = _Anything
    sys.modules["lpips"], sys.modules["pytorch_msssim"] = lp, ms
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    sys.path.insert(0, "/root/reference")
    import utils.eval_util as RE
    return RE


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def make_case(rng, K, noise_mm, mirror=False, shift=(0.0, 0.0, 0.0), scale=1.0):
    """a hand-sized point cloud (mm) and a rotated, scaled, shifted, noisy copy of it, both float32"""
    gt = rng.normal(size=(K, 3)) * np.array([40.0, 25.0, 15.0])
    pred = gt @ rotation(rng).T
    if mirror:
        pred = pred * np.array([-1.0, 1.0, 1.0])
    pred = pred * scale + np.asarray(shift) + rng.normal(size=(K, 3)) * noise_mm
    return gt.astype(np.float32), pred.astype(np.float32)


CASES = [("k21_n05", dict(K=21, noise_mm=0.5)), ("k21_n3", dict(K=21, noise_mm=3.0)), ("k21_n8", dict(K=21, noise_mm=8.0)),
         ("k21_mirror", dict(K=21, noise_mm=0.5, mirror=True)), ("k4", dict(K=4, noise_mm=3.0)), ("k3", dict(K=3, noise_mm=3.0)),
         ("k778", dict(K=778, noise_mm=3.0, shift=(5.0, -7.0, 300.0), scale=1.2))]


def main():
    RE = import_reference()
    rng = np.random.default_rng(20240607)
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, kw in CASES:
        while True:                                   # K > 3: redrawn until M = a^T b is well away from rank 2 (sigma3 / sigma1 >= 0.02)
            gt, pred = make_case(rng, **kw)
            g64, p64 = gt.astype(np.float64), pred.astype(np.float64)
            a, b = g64 - g64.mean(0), p64 - p64.mean(0)
            w = np.linalg.svd((a / np.linalg.norm(a)).T @ (b / np.linalg.norm(b)), compute_uv=False)
            if kw["K"] == 3 or w[2] / w[0] >= 0.02:
                break
        out[name + "_sigma"] = w
        out[name + "_gt"], out[name + "_pred"] = gt, pred
        out[name + "_aligned"] = RE.align_w_scale(g64.copy(), p64.copy())          # (the reference divides its arguments in place)
        R, s, s1, t = RE.align_w_scale(g64.copy(), p64.copy(), return_trafo=True)
        out[name + "_R"], out[name + "_s"], out[name + "_s1"], out[name + "_t"] = R, np.float64(s), np.float64(s1), t
        out[name + "_by_trafo"] = RE.align_by_trafo(p64.copy(), (R, s, s1, t))
    n, K = 7, 21
    gt = (rng.normal(size=(n, K, 3)) * 40.0).astype(np.float32)
    pred = (gt + rng.normal(size=(n, K, 3)) * rng.uniform(1.0, 25.0, size=(n, K, 1))).astype(np.float32)
    vis = (rng.uniform(size=(n, K)) > 0.2).astype(np.float32)
    vis[:, 13] = 0.0
    vis[0, 0] = 1.0
    ev = RE.EvalUtil(num_kp=K)
    for i in range(n):
        ev.feed(gt[i].astype(np.float64), vis[i], pred[i].astype(np.float64))
    mean, median, auc, curve, thr = ev.get_measures(0, 50, 20)
    out.update(pck_gt=gt, pck_vis=vis, pck_pred=pred, pck_epe_mean=np.float64(mean), pck_epe_median=np.float64(median), pck_auc=np.float64(auc),
               pck_curve=np.asarray(curve), pck_thresholds=np.asarray(thr))
    path = os.path.join(HERE, "pose_eval_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
