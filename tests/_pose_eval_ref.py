"""Float64 NumPy restatement of the three contracts of csrc/pose_eval.hip (include/harp_hip.h), own code written from the header's formulas:
the reference of tests/test_gpu_pose_eval.py, itself checked against the reference project's recorded outputs (tests/golden/
pose_eval_ref.npz) in tests/test_pose_eval_cpu.py.  Inputs are the float32 arrays the kernels get, widened to float64; nothing here is
rounded to float32, the tests do that where the contract says so."""
import numpy as np


def ulp32(x):
    """the spacing of float32 at magnitude |x|"""
    return float(np.spacing(np.float32(abs(x))))


def procrustes(gt, pred, valid=None, pred_idx=None):
    """gt (N,K,3), pred (N,Kp,3) float32 -> dict of float64 aligned (N,K,3), err (N,K), trafo (N,14), int n_valid (N), sigma (N,3) (the
    singular values of M, falling).  np.linalg.svd, no determinant correction.  NaN at points not used and in frames with < 3 of them."""
    gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    N, K = gt.shape[:2]
    if pred_idx is not None:
        pred = pred[:, np.asarray(pred_idx)]
    use = np.ones((N, K), dtype=bool) if valid is None else np.asarray(valid).reshape(N, K) != 0
    aligned, err = np.full((N, K, 3), np.nan), np.full((N, K), np.nan)
    trafo, sigma = np.full((N, 14), np.nan), np.full((N, 3), np.nan)
    n_valid = use.sum(1).astype(np.int32)
    for n in range(N):
        u = use[n]
        if n_valid[n] < 3:
            continue
        g, p = gt[n, u], pred[n, u]
        t1, t2 = g.mean(0), p.mean(0)
        a, b = g - t1, p - t2
        s1, s2 = np.sqrt((a * a).sum()) + 1e-8, np.sqrt((b * b).sum()) + 1e-8
        a, b = a / s1, b / s2
        U, W, Vt = np.linalg.svd(a.T @ b)
        R, s = U @ Vt, W.sum()
        al = (b @ R.T) * s * s1 + t1
        aligned[n, u], err[n, u] = al, np.sqrt(((g - al) ** 2).sum(1))
        trafo[n], sigma[n] = np.concatenate([R.ravel(), [s, s1], t1 - t2]), W
    return {"aligned": aligned, "err": err, "trafo": trafo, "n_valid": n_valid, "sigma": sigma}


def pck_counts(err, valid, thresholds):
    """err (N,K) float32, valid (N,K) or None, thresholds (n_thr) float32 -> counts (K,n_thr) int, n_vis (K) int, err_sum (K) float64;
    seen = visible and not NaN; the comparison is the float32 one"""
    err, thr = np.asarray(err, dtype=np.float32), np.asarray(thresholds, dtype=np.float32)
    seen = ~np.isnan(err)
    if valid is not None:
        seen &= np.asarray(valid).reshape(err.shape) != 0
    with np.errstate(invalid="ignore"):
        le = err[:, :, None] <= thr[None, None, :]
    counts = (le & seen[:, :, None]).sum(0).astype(np.int32)
    return counts, seen.sum(0).astype(np.int32), np.where(seen, err.astype(np.float64), 0.0).sum(0)


def fscore(gt, pred, thresholds):
    """gt (N,Kg,3), pred (N,Kp,3), thresholds (n_thr) float32 -> float64 out (N,n_thr,3) = precision, recall, F; the nearest SQUARED
    distances d2_gt (N,Kg), d2_pred (N,Kp) and the squared thresholds t2 (n_thr)"""
    gt, pred = np.asarray(gt, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    t2 = np.asarray(thresholds, dtype=np.float32).astype(np.float64) ** 2
    N = gt.shape[0]
    d2_gt, d2_pred = np.empty(gt.shape[:2]), np.empty(pred.shape[:2])
    for n in range(N):
        d = gt[n][:, None, :] - pred[n][None, :, :]
        d2 = d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2
        d2_gt[n], d2_pred[n] = d2.min(1), d2.min(0)
    p = (d2_gt[:, None, :] < t2[None, :, None]).mean(2)
    r = (d2_pred[:, None, :] < t2[None, :, None]).mean(2)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(p + r > 0, 2 * p * r / (p + r), 0.0)
    return {"out": np.stack([p, r, f], -1), "d2_gt": d2_gt, "d2_pred": d2_pred, "t2": t2}


def measures(err, seen, val_min, val_max, steps):
    """EvalUtil.get_measures from an (N,K) float64 error table and its (N,K) bool mask (include/harp_hip.h and utils/eval_util.py:122-163)"""
    thr = np.linspace(val_min, val_max, steps)
    means, medians, aucs, curves = [], [], [], []
    for k in range(err.shape[1]):
        d = err[seen[:, k], k]
        if d.size == 0:
            continue
        c = np.array([(d <= t).mean() for t in thr])
        means.append(d.mean()); medians.append(np.median(d)); curves.append(c)
        aucs.append(np.sum((c[1:] + c[:-1]) * 0.5 * np.diff(thr)) / (thr[-1] - thr[0]))
    return np.mean(means), np.mean(medians), np.mean(aucs), np.mean(np.array(curves), 0), thr
