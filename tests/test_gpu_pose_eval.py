"""-m gpu: the geometric evaluation kernels of csrc/pose_eval.hip — harp_procrustes_align, harp_pck_counts, harp_point_set_fscore — through
the raw C entry points and through harp_amd.ops, against the float64 restatement tests/_pose_eval_ref.py on the same float32 inputs
(itself checked against the reference project's recorded outputs in tests/test_pose_eval_cpu.py); EvalUtil on the device against the
recorded tuple; evaluate_sequence(pose_eval=...).  Every kernel case runs twice and must give the same bits.

Bounds (include/harp_hip.h; none comes from the kernels' output):
  aligned, err   4 ulp32(max |gt coordinate|): the kernel rounds its float64 result once (<= 0.5 ulp32 of the value, which is about the
                 size of the ground truth it is aligned to); the rest is margin for float64 sums taken in another order
  trafo          1e-8 absolute, where the reference's own sigma3 / sigma1 >= 1e-3 (asserted on the reference; scenes are redrawn until it
                 holds); with three points sigma3 = 0, R is free along the lost direction and only aligned / err are compared
  PCK            counts and n_vis exact, err_sum 1e-12 relative (float64 sums of at most 257 float32 values in another order)
  F-score        precondition on the reference alone: no nearest d2 within 1e-9 relative of a squared threshold; then the counts, and
                 so precision and recall, are exact, F within 1 ulp32 (the last division), the nearest distances within 1 ulp32
Measured maxima (MI355X) are printed by every test and recorded in DESIGN.md §18."""
import os

import numpy as np
import pytest
import torch

from tests import _pose_eval_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_eval_ref.npz"))


def _lib():
    from harp_amd import _lib as L
    return L


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


# ---------------------------------------------------------------------------------------------------------------- Procrustes
def _scene(seed, N, K, Kp=None, noise=2.0, mirror=False, mask=None, few=()):
    """root-aligned ground truth (mm) and a rotated, scaled prediction 300 mm away; redrawn (reference only) until every frame that is
    aligned has sigma3 / sigma1 >= 1e-3 (K > 3) or sigma2 / sigma1 >= 1e-3 (K = 3).  mask: share of points switched off at random;
    few: {frame: number of valid points} for frames with fewer than 3."""
    for attempt in range(100):
        rng = np.random.default_rng(1000 * seed + attempt)
        gt = rng.normal(size=(N, K, 3)) * 40.0
        gt -= gt[:, :1]
        src = np.stack([(gt[n] @ _rotation(rng).T) * rng.uniform(0.8, 1.3) for n in range(N)])
        if mirror:
            src = src * np.array([-1.0, 1.0, 1.0])
        src = src + np.array([5.0, -7.0, 300.0]) + rng.normal(size=(N, K, 3)) * noise
        idx = None
        if Kp is not None:
            idx = rng.permutation(Kp)[:K].astype(np.int32)
            pred = rng.normal(size=(N, Kp, 3)) * 500.0
            pred[:, idx] = src
        else:
            pred = src
        valid = None
        if mask is not None or few:
            valid = (rng.uniform(size=(N, K)) >= (mask or 0.0)).astype(np.float32)
            valid *= rng.choice([1.0, 2.0, -1.0, 0.5], size=(N, K)).astype(np.float32)          # any non-zero value counts
            for n, m in dict(few).items():
                valid[n] = 0.0
                valid[n, rng.permutation(K)[:m]] = 1.0
        gt, pred = gt.astype(np.float32), pred.astype(np.float32)
        ref = PR.procrustes(gt, pred, valid, idx)
        sg = ref["sigma"][ref["n_valid"] >= 3]
        if np.all(sg[:, 2 if K > 3 else 1] / sg[:, 0] >= 1e-3):
            return dict(gt=gt, pred=pred, idx=idx, valid=valid, ref=ref, N=N, K=K, Kp=Kp or K, noise=noise)
    raise AssertionError("no well-conditioned scene in 100 draws")


PRO_CASES = {
    "n1_k3": dict(N=1, K=3), "n3_k4": dict(N=3, K=4), "n2_k21": dict(N=2, K=21), "n5_k64_mask": dict(N=5, K=64, mask=0.2),
    "n5_k65_few": dict(N=5, K=65, mask=0.1, few={1: 2, 3: 0}), "n2_k778": dict(N=2, K=778), "n2_k1026_of_4083": dict(N=2, K=1026, Kp=4083),
    "n2_k21_mirror": dict(N=2, K=21, mirror=True, noise=0.5), "n3_k257_mask": dict(N=3, K=257, mask=0.3),
}


def _pro_raw(c):
    L = _lib()
    t = lambda a, dt=torch.float32: None if a is None else torch.as_tensor(a, dtype=dt, device=DEV).contiguous()
    gt, pred, idx, valid = t(c["gt"]), t(c["pred"]), t(c["idx"], torch.int32), t(c["valid"])
    N, K = c["N"], c["K"]
    al = torch.full((N, K, 3), 7.0, device=DEV)
    er = torch.full((N, K), 7.0, device=DEV)
    tr = torch.full((N, 14), 7.0, dtype=torch.float64, device=DEV)
    nv = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    rc = L.lib().harp_procrustes_align(L.ptr(gt), L.ptr(pred), L.ptr(idx), L.ptr(valid), N, K, c["Kp"], L.ptr(al), L.ptr(er), L.ptr(tr), L.ptr(nv),
                                       L.stream())
    torch.cuda.synchronize()
    assert rc == 0
    return al, er, nv, tr


@pytest.mark.parametrize("name", list(PRO_CASES))
def test_procrustes_against_float64(name):
    from harp_amd import ops
    c = _scene(sum(map(ord, name)), **PRO_CASES[name])
    ref, N, K = c["ref"], c["N"], c["K"]
    raw, raw2 = _pro_raw(c), _pro_raw(c)
    assert _same_bits(raw, raw2)
    d = lambda a, dt=torch.float32: None if a is None else torch.as_tensor(a, dtype=dt, device=DEV)
    via_ops = ops.procrustes_align(d(c["gt"]), d(c["pred"]), valid=d(c["valid"]), pred_idx=d(c["idx"], torch.int32), return_trafo=True)
    assert _same_bits(raw, via_ops)
    al, er, nv, tr = (x.cpu().numpy() for x in raw)
    assert np.array_equal(nv, ref["n_valid"])
    used = ~np.isnan(ref["err"])
    assert np.array_equal(np.isnan(er), ~used) and np.array_equal(np.isnan(al), np.isnan(ref["aligned"]))
    bound = 4 * PR.ulp32(np.abs(c["gt"]).max())
    e_al = np.abs(al.astype(np.float64) - ref["aligned"])[used].max()
    e_er = np.abs(er.astype(np.float64) - ref["err"])[used].max()
    ok = ref["n_valid"] >= 3
    assert np.isnan(tr[~ok]).all() and np.isnan(er[~ok]).all()
    e_tr = np.abs(tr[ok] - ref["trafo"][ok])
    e_tr = e_tr.max() if K > 3 else e_tr[:, 9:].max()          # K = 3: R is free along the lost direction; s, s1, t are not
    print(f"[procrustes {name}] aligned {e_al:.3e}, err {e_er:.3e} (bound {bound:.3e}), trafo {e_tr:.3e} (bound 1e-8), "
          f"sigma3/sigma1 >= {np.nanmin(ref['sigma'][:, 2] / ref['sigma'][:, 0]):.2e}")
    assert e_al <= bound and e_er <= bound
    assert e_tr <= 1e-8
    R = tr[ok, :9].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
    if PRO_CASES[name].get("mirror"):
        assert np.all(np.linalg.det(R) < -0.999)
        assert np.nanmean(er) < 3 * c["noise"]                   # a reflection was used: the error is the noise, not a proper rotation's
        proper = PR.procrustes(c["gt"], c["pred"] * np.array([-1, 1, 1], dtype=np.float32))["err"].mean()
        assert np.nanmean(er) < 1.5 * proper                     # and as small as aligning the un-mirrored copy
    elif K > 3:
        assert np.all(np.linalg.det(R) > 0.999)


def test_procrustes_fixture_cases_and_wrappers():
    """the reference project's recorded cases through align_w_scale / align_by_trafo on HIP tensors; optional outputs left out; refusals"""
    from harp_amd import ops
    from harp_amd.utils.eval_util import align_by_trafo, align_w_scale
    for name in [str(x) for x in G["cases"]]:
        gt, pred = torch.from_numpy(G[name + "_gt"]).to(DEV), torch.from_numpy(G[name + "_pred"]).to(DEV)
        bound = 4 * PR.ulp32(np.abs(G[name + "_gt"]).max())
        got = align_w_scale(gt, pred)
        assert got.shape == gt.shape and got.dtype == torch.float32
        e = np.abs(got.cpu().numpy().astype(np.float64) - G[name + "_aligned"]).max()
        batch = align_w_scale(torch.stack([gt, gt]), torch.stack([pred, pred]))
        assert torch.equal(batch[0], got) and torch.equal(batch[1], got)
        R, s, s1, t = align_w_scale(gt, pred, return_trafo=True)
        e_t = max(abs(float(s) - G[name + "_s"]), abs(float(s1) - G[name + "_s1"]), np.abs(t.cpu().numpy() - G[name + "_t"]).max())
        if name != "k3":
            e_t = max(e_t, np.abs(R.cpu().numpy() - G[name + "_R"]).max())
            moved = align_by_trafo(pred, (R, s, s1, t)).cpu().numpy()
            assert np.abs(moved - G[name + "_by_trafo"]).max() <= 1e-8 * np.abs(G[name + "_by_trafo"]).max()
        print(f"[procrustes fixture {name}] aligned {e:.3e} (bound {bound:.3e}), trafo {e_t:.3e}")
        assert e <= bound and e_t <= 1e-8
        lst = align_w_scale(torch.stack([gt, gt]), torch.stack([pred, pred]), return_trafo=True)
        assert len(lst) == 2 and torch.equal(lst[1][0], R) and lst[0][3].shape == (3,)
    # aligned and trafo are optional in the C interface
    L = _lib()
    gt, pred = torch.from_numpy(G["k21_n3_gt"]).to(DEV)[None].contiguous(), torch.from_numpy(G["k21_n3_pred"]).to(DEV)[None].contiguous()
    er, nv = torch.empty(1, 21, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    assert L.lib().harp_procrustes_align(L.ptr(gt), L.ptr(pred), None, None, 1, 21, 21, None, L.ptr(er), None, L.ptr(nv), L.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(er[0], ops.procrustes_align(gt[0], pred[0])[1]) and int(nv[0]) == 21
    with pytest.raises(NotImplementedError):
        ops.procrustes_align(gt.clone().requires_grad_(), pred)
    with pytest.raises(RuntimeError):
        ops.procrustes_align(gt.cpu(), pred.cpu())
    with pytest.raises(ValueError):
        ops.procrustes_align(gt, pred[:, :20])


# ---------------------------------------------------------------------------------------------------------------- PCK
def _pck_scene(N, K, n_thr, seed):
    rng = np.random.default_rng(seed)
    thr = np.linspace(0.0, 50.0, n_thr).astype(np.float32)
    err = rng.uniform(0.0, 60.0, size=(N, K)).astype(np.float32)
    flat = err.reshape(-1)
    pick = rng.permutation(flat.size)[:max(3, flat.size // 4)]
    t = thr[rng.integers(0, n_thr, size=pick.size)]
    kind = rng.integers(0, 3, size=pick.size)                      # exactly a threshold, one float32 below it, one above it
    flat[pick] = np.where(kind == 0, t, np.where(kind == 1, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(100))))
    nan = rng.uniform(size=(N, K)) < 0.05
    err[nan] = np.nan
    valid = (rng.uniform(size=(N, K)) > 0.2).astype(np.float32) * rng.choice([1.0, 3.0], size=(N, K)).astype(np.float32)
    if K > 1:
        valid[:, K // 2] = 0.0                                     # a keypoint that is never visible
    return err, valid, thr


@pytest.mark.parametrize("N", [1, 64, 257])
@pytest.mark.parametrize("K,n_thr", [(1, 20), (21, 20), (778, 20), (21, 300)])
def test_pck_counts_exact(N, K, n_thr):
    from harp_amd import ops
    L = _lib()
    err, valid, thr = _pck_scene(N, K, n_thr, 7 * N + K + n_thr)
    e, v, t = (torch.from_numpy(x).to(DEV) for x in (err, valid, thr))
    for mask, vd in ((valid, v), (None, None)):
        want = PR.pck_counts(err, mask, thr)

        def raw():
            c = torch.full((K, n_thr), -7, dtype=torch.int32, device=DEV)
            n = torch.full((K,), -7, dtype=torch.int32, device=DEV)
            s = torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
            assert L.lib().harp_pck_counts(L.ptr(e), L.ptr(vd), L.ptr(t), N, K, n_thr, L.ptr(c), L.ptr(n), L.ptr(s), L.stream()) == 0
            torch.cuda.synchronize()
            return c, n, s
        a, b = raw(), raw()
        assert _same_bits(a, b) and _same_bits(a, ops.pck_counts(e, vd, t))
        assert np.array_equal(a[0].cpu().numpy(), want[0]) and np.array_equal(a[1].cpu().numpy(), want[1])
        rel = np.abs(a[2].cpu().numpy() - want[2]).max() / max(np.abs(want[2]).max(), 1e-300)
        print(f"[pck N={N} K={K} n_thr={n_thr} mask={mask is not None}] counts exact, err_sum {rel:.2e} relative")
        assert rel <= 1e-12
    if K > 1:
        assert int(a[1].sum()) > 0 and PR.pck_counts(err, valid, thr)[1][K // 2] == 0


def test_eval_util_on_the_device_against_the_fixture():
    from harp_amd.utils.eval_util import EvalUtil
    gt, vis, pred = G["pck_gt"], G["pck_vis"], G["pck_pred"]
    d64 = np.linalg.norm(gt.astype(np.float64) - pred.astype(np.float64), axis=2)
    thr = G["pck_thresholds"]
    near = np.abs(d64[:, :, None] - thr[None, None, 1:]) / thr[None, None, 1:]
    assert near.min() > 1e-6                                       # on the reference alone: no distance sits on a threshold
    ev = EvalUtil(21)
    ev.feed_batch(torch.from_numpy(gt[:4]).to(DEV), torch.from_numpy(vis[:4]).to(DEV), torch.from_numpy(pred[:4]).to(DEV))
    ev.feed_batch(torch.from_numpy(gt[4:]).to(DEV), torch.from_numpy(vis[4:]).to(DEV), torch.from_numpy(pred[4:]).to(DEV))
    mean, median, auc, curve, got_thr = ev.get_measures(0, 50, 20)
    rel = [abs(mean - G["pck_epe_mean"]) / G["pck_epe_mean"], abs(median - G["pck_epe_median"]) / G["pck_epe_median"],
           abs(auc - G["pck_auc"]) / G["pck_auc"]]
    print(f"[EvalUtil device] mean {rel[0]:.2e}, median {rel[1]:.2e}, auc {rel[2]:.2e} relative; curve exact: {np.array_equal(curve, G['pck_curve'])}")
    assert max(rel) <= 1e-6
    assert np.array_equal(curve, G["pck_curve"]) and np.array_equal(got_thr, thr)
    with pytest.raises(ValueError):
        ev.get_measures(0, 50, 1)
    with pytest.raises(RuntimeError):
        ev.feed(gt[0], vis[0], pred[0])


# ---------------------------------------------------------------------------------------------------------------- F-score
THR_MM = np.array([5.0, 15.0], dtype=np.float32)


def _fs_scene(N, Kg, Kp, seed, same=False):
    for attempt in range(100):
        rng = np.random.default_rng(100 * seed + attempt)
        gt = (rng.normal(size=(N, Kg, 3)) * 30.0 + np.array([5.0, -7.0, 300.0])).astype(np.float32)
        if same:
            pred = gt.copy()
        else:
            pick = rng.integers(0, Kg, size=(N, Kp))
            pred = (np.take_along_axis(gt, pick[:, :, None], 1) + rng.normal(size=(N, Kp, 3)) * rng.uniform(1.0, 12.0, size=(N, Kp, 1))).astype(np.float32)
        if Kg >= 3:
            gt[:, 2] = gt[:, 0]                                     # duplicated points
        if Kp >= 2 and not same:
            pred[:, 1] = pred[:, 0]
        if same:
            pred = gt.copy()
        ref = PR.fscore(gt, pred, THR_MM)
        d2 = np.concatenate([ref["d2_gt"].ravel(), ref["d2_pred"].ravel()])
        if np.all(np.abs(d2[:, None] - ref["t2"][None]) > 1e-9 * ref["t2"][None]):       # the precondition, on the reference alone
            return gt, pred, ref
    raise AssertionError("no scene clear of the thresholds in 100 draws")


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("Kg,Kp", [(1, 1), (3, 5), (64, 65), (778, 778), (778, 3093)])
def test_fscore_against_float64(N, Kg, Kp):
    from harp_amd import ops
    L = _lib()
    gt, pred, ref = _fs_scene(N, Kg, Kp, 13 * Kg + Kp + N)
    g, p, t = (torch.from_numpy(x).to(DEV) for x in (gt, pred, THR_MM))

    def raw(with_nn=True):
        out = torch.full((N, 2, 3), 7.0, device=DEV)
        ng, npd = torch.full((N, Kg), 7.0, device=DEV), torch.full((N, Kp), 7.0, device=DEV)
        rc = L.lib().harp_point_set_fscore(L.ptr(g), L.ptr(p), L.ptr(t), N, Kg, Kp, 2, L.ptr(out), L.ptr(ng) if with_nn else None,
                                           L.ptr(npd) if with_nn else None, L.stream())
        torch.cuda.synchronize()
        assert rc == 0
        return out, ng, npd
    a, b = raw(), raw()
    assert _same_bits(a, b) and _same_bits(a, ops.point_set_fscore(g, p, t))
    assert torch.equal(raw(False)[0], a[0])                          # the nearest distances are optional
    out, ng, npd = (x.cpu().numpy() for x in a)
    want = ref["out"].astype(np.float32)
    assert np.array_equal(out[..., :2], want[..., :2])               # exact counts: precision and recall to the bit
    e_f = np.abs(out[..., 2].astype(np.float64) - ref["out"][..., 2]).max()
    wg, wp = np.sqrt(ref["d2_gt"]), np.sqrt(ref["d2_pred"])
    e_n = max((np.abs(ng - wg) / np.maximum(np.spacing(wg.astype(np.float32)), 1e-45)).max(),
              (np.abs(npd - wp) / np.maximum(np.spacing(wp.astype(np.float32)), 1e-45)).max())
    print(f"[fscore N={N} {Kg}x{Kp}] P/R exact, F {e_f:.2e} (bound {PR.ulp32(1.0):.2e}), nearest {e_n:.2f} ulp32; F@5 {out[0, 0, 2]:.3f} F@15 {out[0, 1, 2]:.3f}")
    assert e_f <= PR.ulp32(1.0) and e_n <= 1.0
    if Kg >= 64:
        assert 0.0 < out[..., 0, 2].min() and out[..., 0, 2].max() < out[..., 1, 2].max() <= 1.0      # the thresholds are told apart


def test_fscore_identical_sets_and_far_sets():
    from harp_amd import ops
    gt, pred, ref = _fs_scene(2, 65, 65, 5, same=True)
    out, ng, npd = ops.point_set_fscore(torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV), torch.from_numpy(THR_MM).to(DEV))
    assert bool((out == 1.0).all()) and bool((ng == 0).all()) and bool((npd == 0).all())
    out, _, _ = ops.point_set_fscore(torch.from_numpy(gt[0]).to(DEV), torch.from_numpy(gt[0] + 100.0).to(DEV), torch.from_numpy(THR_MM).to(DEV))
    assert out.shape == (2, 3) and bool((out == 0.0).all())         # p + r = 0: F = 0, not NaN
    with pytest.raises(ValueError):
        ops.point_set_fscore(torch.from_numpy(gt).to(DEV), torch.from_numpy(pred).to(DEV), torch.zeros(0, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- evaluate_sequence
def _setup(T, S, seed, tmp_path, **cfg_kw):
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.optimize_sequence import init_params
    from harp_amd.utils.config_utils import get_config
    from tests._scene import make_scene
    sc = make_scene(T=T, S=S, seed=seed)
    cfg = get_config(write_yaml=False, use_arm=False, img_size=S, focal_length=sc["focal"], base_output_dir=str(tmp_path) + "/", **cfg_kw)
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=sc["model_np"], device=DEV)
    params = init_params(sc["seq"], True, True, None, layer.th_faces, False, torch.from_numpy(sc["tpl"]["verts_uvs"])[None],
                         torch.from_numpy(sc["tpl"]["faces_uvs"])[None], configs=cfg, device=DEV, uv_mask=sc["uv_mask"])
    tg = sc["targets"]
    ds = [(i, tg["y_true"][i], tg["y_sil"][i][..., None], tg["y_sil_col"][i][..., None]) for i in range(T)]
    return cfg, layer, params, ds


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.filterwarnings("ignore:MS_SSIM left out")
def test_evaluate_sequence_pose_eval(tmp_path):
    """3 frames of 96 px (the smallest scene of tests/test_gpu_evaluate.py), synthetic ground truth = a similarity transform of the fitted
    joints / vertices plus noise.  Without pose_eval: the host loop, the files and lines of before.  With it: the new lines in order, the
    vertex error equal to the host loop's, the joint error equal to the float64 restatement's, frame 1 (2 valid joints) left out."""
    from harp_amd.optimize_sequence import evaluate_sequence, get_mesh_subdivider
    from harp_amd.utils.eval_util import align_w_scale
    from harp_amd.utils.visualize import prepare_mesh
    T = 3
    old_dir, new_dir, gt_dir = tmp_path / "old", tmp_path / "new", tmp_path / "gt"
    for d in (old_dir, new_dir, gt_dir):
        d.mkdir()
    cfg, layer, params, ds = _setup(T, 96, 24, old_dir, eval_mesh=True, gt_mesh_dir=str(gt_dir))
    with torch.no_grad():
        j, v, _, _ = prepare_mesh(params, torch.arange(T), layer, False, get_mesh_subdivider(layer, device=DEV), False, cfg, device=DEV)
    rng = np.random.default_rng(3)
    q = _rotation(rng)
    gt_v = 1.3 * v[:, :778].double().cpu().numpy() @ q.T + np.array([0.02, -0.01, 0.3]) + rng.normal(size=(T, 778, 3)) * 2e-3
    for i in range(T):
        np.savetxt(gt_dir / f"{500 + i + 1}_manov.xyz", gt_v[i] * 1000.0)
    gt_j = (1.1 * (j[:, :21].double().cpu().numpy() * 1000.0) @ q.T + np.array([3.0, 4.0, -50.0]) + rng.normal(size=(T, 21, 3)) * 2.0).astype(np.float32)
    jv = np.ones((T, 21), dtype=np.float32)
    jv[0, [3, 17]] = 0.0
    jv[1] = 0.0
    jv[1, [4, 9]] = 1.0                                              # frame 1: two valid joints, left out
    # ---- as before
    old = evaluate_sequence(cfg, params, ds, layer, device=DEV)
    host = [float(np.linalg.norm(np.loadtxt(gt_dir / f"{501 + i}_manov.xyz") / 1000.0 -
                                 align_w_scale(np.loadtxt(gt_dir / f"{501 + i}_manov.xyz") / 1000.0, v[i, :778].cpu().numpy()), axis=1).mean()) * 1000.0
            for i in range(T)]
    assert list(old) == ["Silhouette IoU", "L1", "Procrustes-aligned vertex error (mm)"]
    text = "".join(" %s: %.5f\n" % (k, x) for k, x in [("Silhouette IoU", old["Silhouette IoU"]), ("L1", old["L1"]),
                                                        ("Procrustes-aligned vertex error (mm)", float(np.mean(host)))])
    assert open(old_dir / "eval_results.txt").read() == text         # byte for byte the host loop's file
    assert _files(old_dir) == ["eval_results.txt", "eval_vert_mm.txt", os.path.join("uv_out", "normal_map.png"), os.path.join("uv_out", "texture.png")]
    assert np.array_equal(np.loadtxt(old_dir / "eval_vert_mm.txt"), host) and old["Procrustes-aligned vertex error (mm)"] == float(np.mean(host))
    # ---- with ground-truth joints: the device path
    cfg["base_output_dir"] = str(new_dir) + "/"
    new = evaluate_sequence(cfg, params, ds, layer, device=DEV, pose_eval={"gt_joints": gt_j, "gt_joint_valid": jv})
    keys = ["Silhouette IoU", "L1", "Procrustes-aligned joint error (mm)", "Joint AUC 0-50 mm", "Procrustes-aligned vertex error (mm)",
            "Vertex AUC 0-50 mm", "F@5mm", "F@15mm"]
    assert list(new) == keys
    lines = open(new_dir / "eval_results.txt").read().splitlines()
    assert [ln.split(":")[0][1:] for ln in lines] == keys and lines == [" %s: %.5f" % (k, new[k]) for k in keys]
    assert new["Silhouette IoU"] == old["Silhouette IoU"] and new["L1"] == old["L1"]
    rel_v = abs(new["Procrustes-aligned vertex error (mm)"] - old["Procrustes-aligned vertex error (mm)"]) / old["Procrustes-aligned vertex error (mm)"]
    # the joints as evaluate_sequence forms them (float32, mm, root-aligned), through the float64 restatement
    g32 = torch.from_numpy(gt_j).to(DEV)
    g32 = (g32 - g32[:, :1]).cpu().numpy()
    p32 = j[:, :21].float() * 1000.0
    p32 = (p32 - p32[:, :1]).cpu().numpy()
    ref = PR.procrustes(g32, p32, jv)
    frames = [np.nanmean(ref["err"][i]) for i in (0, 2)]
    rel_j = abs(new["Procrustes-aligned joint error (mm)"] - np.mean(frames)) / np.mean(frames)
    auc = PR.measures(np.nan_to_num(ref["err"][[0, 2]]), jv[[0, 2]] != 0, 0.0, 50.0, 100)[2]
    print(f"[evaluate_sequence pose_eval] vertex {new['Procrustes-aligned vertex error (mm)']:.5f} mm against the host loop: {rel_v:.2e} relative; "
          f"joint {new['Procrustes-aligned joint error (mm)']:.5f} mm: {rel_j:.2e}; joint AUC {new['Joint AUC 0-50 mm']:.5f} (float64 {auc:.5f}); "
          f"vertex AUC {new['Vertex AUC 0-50 mm']:.5f}, F@5mm {new['F@5mm']:.4f}, F@15mm {new['F@15mm']:.4f}")
    assert rel_v <= 1e-6 and rel_j <= 1e-6
    assert abs(new["Joint AUC 0-50 mm"] - auc) <= 1e-6
    assert np.loadtxt(new_dir / "eval_joint_mm.txt").shape == (2,) and np.loadtxt(new_dir / "eval_vert_mm.txt").shape == (T,)
    assert np.allclose(np.loadtxt(new_dir / "eval_joint_mm.txt"), frames, rtol=1e-6)
    assert 0.9 < new["Vertex AUC 0-50 mm"] < 1.0 and 0.0 < new["F@5mm"] < new["F@15mm"] <= 1.0
    # ground-truth vertices passed in, no joints; read from an .npz through the configuration
    np.savez(tmp_path / "pe.npz", gt_verts=gt_v.astype(np.float32))
    cfg["eval_mesh"], cfg["pose_eval"] = False, str(tmp_path / "pe.npz")
    third = evaluate_sequence(cfg, params, ds, layer, device=DEV)
    assert list(third) == ["Silhouette IoU", "L1"] + keys[4:]
    assert abs(third["Procrustes-aligned vertex error (mm)"] - new["Procrustes-aligned vertex error (mm)"]) <= 1e-4      # float32 storage of the .npz


def test_eval_procrustes(tmp_path, capsys):
    """utils/eval_util.py:166-209 as it was meant: ground-truth joints = a similarity transform of the layer's joints plus 2 mm of noise;
    the mean equals the float64 restatement's on the same float32 joints, a frame with two valid joints is left out, and the pose
    switches change what is evaluated"""
    from harp_amd.utils.eval_util import eval_procrustes
    T = 3
    cfg, layer, params, ds = _setup(T, 96, 24, tmp_path)
    with torch.no_grad():
        _, joints = layer(torch.cat((params["rot"], params["pose"]), 1).to(DEV), params["shape"].repeat([T, 1]).to(DEV), params["trans"].to(DEV))
    rng = np.random.default_rng(11)
    gt = (1.2 * joints[:, :21].double().cpu().numpy() @ _rotation(rng).T + np.array([10.0, 20.0, -400.0]) + rng.normal(size=(T, 21, 3)) * 2.0)
    valid = np.ones((T, 21), dtype=np.int64)
    valid[0, [2, 5, 11]] = 0
    valid[2] = 0
    valid[2, [0, 7]] = 1
    inp = {"gt_joints": torch.from_numpy(gt.astype(np.float32)), "gt_joint_valid": torch.from_numpy(valid)}
    out = eval_procrustes(ds, params, inp, layer, device=DEV, batch_size=2)
    g32 = inp["gt_joints"] - inp["gt_joints"][:, :1]
    p32 = (joints[:, :21].float() - joints[:, :1].float()).cpu()
    ref = PR.procrustes(g32.numpy(), p32.numpy(), valid)
    want = [np.nanmean(ref["err"][i]) for i in (0, 1)]
    rel = abs(out["mean_mm"] - np.mean(want)) / np.mean(want)
    print(f"[eval_procrustes] {out['mean_mm']:.5f} mm over {out['n_frames']} frames, {rel:.2e} relative to float64")
    assert out["n_frames"] == 2 and len(out["per_frame_mm"]) == 2 and rel <= 1e-6
    assert 0.5 < out["mean_mm"] < 6.0                                  # 2 mm of noise per axis
    assert "Mean Procrustes-aligned joint error of 2 samples: %.3f mm" % out["mean_mm"] in capsys.readouterr().out
    with torch.no_grad():
        params["pose"][1:] += 0.3                                     # now frame 0's pose, or the mean pose, is not every frame's pose
    per_frame = eval_procrustes(ds, params, inp, layer, device=DEV)
    first = eval_procrustes(ds, params, inp, layer, global_pose=True, device=DEV)
    mean_pose = eval_procrustes(ds, params, inp, layer, average_pose=True, device=DEV)
    assert len({round(r["mean_mm"], 6) for r in (per_frame, first, mean_pose)}) == 3
    assert first["per_frame_mm"][0] == per_frame["per_frame_mm"][0]                                # frame 0 under its own pose either way
    assert abs(first["per_frame_mm"][0] - out["per_frame_mm"][0]) <= 1e-6 * out["per_frame_mm"][0]
    assert first["per_frame_mm"][1] != per_frame["per_frame_mm"][1] and mean_pose["per_frame_mm"][0] != out["per_frame_mm"][0]
