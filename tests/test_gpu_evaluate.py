"""-m gpu: the post-fit evaluation `evaluate_sequence` (optimize_sequence.py:595-816) on a synthetic 70-frame scene (two chunks of the
reference's 64-frame averaging: 64 + 6), recomputed here from the same mirror renders with float64 metrics; the eval_mesh path; the
`evaluate=True` flag of the fit; small images (no MS_SSIM line)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _msssim_ref as R
from tests._scene import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _setup(T, S, seed, tmp_path, **cfg_kw):
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.optimize_sequence import init_params
    from harp_amd.utils.config_utils import get_config
    sc = make_scene(T=T, S=S, seed=seed)
    cfg = get_config(write_yaml=False, use_arm=False, img_size=S, focal_length=sc["focal"], base_output_dir=str(tmp_path) + "/", **cfg_kw)
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=sc["model_np"], device=DEV)
    params = init_params(sc["seq"], True, True, None, layer.th_faces, False, torch.from_numpy(sc["tpl"]["verts_uvs"])[None],
                         torch.from_numpy(sc["tpl"]["faces_uvs"])[None], configs=cfg, device=DEV, uv_mask=sc["uv_mask"])
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        params["texture"].copy_(torch.rand(1, 512, 512, 3, generator=g) * 0.5 + 0.3)
        params["trans"].copy_(torch.randn(T, 3, generator=g) * 0.01)
        params["light_positions"].copy_(params["light_positions"] + 0.1 * torch.randn(T, 3, generator=g).to(DEV))
    tg = sc["targets"]
    ds = [(i, tg["y_true"][i], tg["y_sil"][i][..., None], tg["y_sil_col"][i][..., None]) for i in range(T)]
    return sc, cfg, layer, params, ds


def _recompute(cfg, params, ds, layer):
    """the same mirror renders (all frames in one call), float64 metrics, then the mean of the 64-frame chunk means"""
    from harp_amd.optimize_sequence import get_mesh_subdivider
    from harp_amd.renderer import renderer_helper
    from harp_amd.structures import Meshes
    from harp_amd.utils.visualize import prepare_materials, prepare_mesh, render_image, render_image_with_RT
    S, focal, T = cfg["img_size"], cfg["focal_length"], len(ds)
    fid = torch.arange(T)
    with torch.no_grad():
        lp = params["light_positions"][0].repeat(T, 1) if cfg["share_light_position"] else params["light_positions"][fid.to(DEV)]
        phong, sil, _ = renderer_helper.get_renderers(image_size=S, light_posi=lp, silh_sigma=1e-7, silh_faces_per_pixel=50, device=DEV)
        _, v, f, t = prepare_mesh(params, fid, layer, False, get_mesh_subdivider(layer, device=DEV), False, cfg, device=DEV)
        mesh, cam, mat = Meshes(v, f, t), params["cam"][fid.to(DEV)], prepare_materials(params, T, device=DEV)
        y_sil = render_image(mesh, cam, T, sil, S, focal, silhouette=True, device=DEV).cpu().double()
        if cfg["self_shadow"]:
            lR, lT, cR, cT = renderer_helper.process_info_for_shadow(cam, lp, v.mean(1), image_size=S, focal_length=focal, device=DEV)
            shadow = renderer_helper.get_shadow_renderers(image_size=S, light_posi=lp, amb_ratio=torch.sigmoid(params["amb_ratio"]), device=DEV)
            y = render_image_with_RT(mesh, lT, lR, cT, cR, T, shadow, S, focal, materials_properties=mat, device=DEV)
        else:
            y = render_image(mesh, cam, T, phong, S, focal, materials_properties=mat, device=DEV)
    y = y.cpu().double()
    y_true = torch.stack([d[1] for d in ds]).double()
    m_true = torch.stack([d[2][..., 0] for d in ds]).double()
    r, p = m_true >= 0.5, y_sil >= 0.5
    iou = (r & p).sum((1, 2)).double() / (r | p).sum((1, 2)).double()
    l1 = (y_true - y).abs().mean((1, 2, 3))
    ms = R.ms_ssim(y_true.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2))["ms_ssim"] if S > 160 else None
    chunks = [slice(c, min(T, c + 64)) for c in range(0, T, 64)]
    out = {"Silhouette IoU": np.mean([iou[c].mean().item() for c in chunks]), "L1": np.mean([l1[c].mean().item() for c in chunks])}
    if ms is not None:
        out["MS_SSIM"] = np.mean([ms[c].mean().item() for c in chunks])
    return out


def _read(path):
    lines = open(path).read().splitlines()
    for ln in lines:
        assert re.fullmatch(r" [A-Za-z0-9_ ()-]+: -?\d+\.\d{5}", ln), ln
    return {ln.split(":")[0][1:]: float(ln.split(":")[1]) for ln in lines}


@pytest.mark.parametrize("shadow,known", [(True, False), (False, True)])
def test_evaluate_sequence_two_chunks(tmp_path, shadow, known):
    from PIL import Image
    from harp_amd.optimize_sequence import evaluate_sequence
    sc, cfg, layer, params, ds = _setup(70, 176, 21, tmp_path, self_shadow=shadow, known_appearance=known, share_light_position=shadow)
    stats = evaluate_sequence(cfg, params, ds, layer, device=DEV, batch_size=32)
    want = _recompute(cfg, params, ds, layer)
    print(f"[evaluate_sequence] shadow={shadow}: " + ", ".join(f"{k} {stats[k]:.6f} (float64 {want[k]:.6f})" for k in want))
    assert list(stats) == ["Silhouette IoU", "L1", "MS_SSIM"]
    for k in want:
        assert abs(stats[k] - want[k]) <= 1e-5, (k, stats[k], want[k])
    name = "eval_results_test.txt" if known else "eval_results.txt"
    assert not os.path.exists(tmp_path / ("eval_results.txt" if known else "eval_results_test.txt"))
    got = _read(tmp_path / name)
    assert list(got) == ["Silhouette IoU", "L1", "MS_SSIM"] and all(abs(got[k] - stats[k]) <= 5e-6 for k in got)
    for f in ("texture.png", "normal_map.png"):
        im = Image.open(tmp_path / "uv_out" / f)
        assert im.size == (512, 512) and im.mode == "RGB"


def test_evaluate_sequence_eval_mesh(tmp_path):
    """GT vertices = a known similarity transform of the fitted mesh (mm, <500 + fid + 1>_manov.xyz): Procrustes error ~ 0"""
    from harp_amd.optimize_sequence import evaluate_sequence, get_mesh_subdivider
    from harp_amd.utils.visualize import prepare_mesh
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    sc, cfg, layer, params, ds = _setup(5, 176, 22, tmp_path, eval_mesh=True, gt_mesh_dir=str(gt_dir))
    with torch.no_grad():
        _, v, _, _ = prepare_mesh(params, torch.arange(5), layer, False, get_mesh_subdivider(layer, device=DEV), False, cfg, device=DEV)
    rng = np.random.default_rng(0)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    for i in range(5):
        gt = 1.3 * v[i, :778].double().cpu().numpy() @ q.T + np.array([0.02, -0.01, 0.3])
        np.savetxt(gt_dir / f"{500 + i + 1}_manov.xyz", gt * 1000.0)
    stats = evaluate_sequence(cfg, params, ds, layer, device=DEV)
    err = stats["Procrustes-aligned vertex error (mm)"]
    print(f"[evaluate_sequence] Procrustes error of a similarity-transformed mesh: {err:.2e} mm")
    assert err < 1e-3
    assert "Procrustes-aligned vertex error (mm)" in _read(tmp_path / "eval_results.txt")
    assert np.loadtxt(tmp_path / "eval_vert_mm.txt").shape == (5,)


def test_fit_with_evaluate_flag(tmp_path):
    from harp_amd.optimize_sequence import optimize_hand_sequence
    sc, cfg, layer, params, ds = _setup(4, 176, 23, tmp_path, total_epoch=2, training_stage=[1, 1, 0])
    optimize_hand_sequence(cfg, sc["seq"], ds, None, None, layer, torch.from_numpy(sc["tpl"]["verts_uvs"])[None],
                           torch.from_numpy(sc["tpl"]["faces_uvs"])[None], device=DEV, uv_mask=sc["uv_mask"], batch_size=2, evaluate=True)
    got = _read(tmp_path / "eval_results.txt")
    assert list(got) == ["Silhouette IoU", "L1", "MS_SSIM"] and 0 <= got["Silhouette IoU"] <= 1
    assert (tmp_path / "uv_out" / "texture.png").exists()


def test_small_images_leave_out_ms_ssim(tmp_path):
    from harp_amd.optimize_sequence import evaluate_sequence
    sc, cfg, layer, params, ds = _setup(3, 96, 24, tmp_path)
    with pytest.warns(UserWarning, match="MS_SSIM"):
        stats = evaluate_sequence(cfg, params, ds, layer, device=DEV)
    want = _recompute(cfg, params, ds, layer)
    got = _read(tmp_path / "eval_results.txt")
    assert list(got) == ["Silhouette IoU", "L1"] and list(stats) == ["Silhouette IoU", "L1"]
    for k in want:
        assert abs(stats[k] - want[k]) <= 1e-5, (k, stats[k], want[k])
