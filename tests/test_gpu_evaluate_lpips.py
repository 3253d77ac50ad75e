"""-m gpu: LPIPS in the post-fit evaluation — evaluate_sequence with seeded LPIPS weights on a 70-frame scene (two chunks of the reference's
64-frame averaging), recomputed from the same mirror renders with the float64 restatement (tests/_lpips_ref.py); the reference's key order
and the eval_results.txt line; configs["lpips_weights"] as a file through optimize_hand_sequence(evaluate=True) and --lpips-weights."""
import numpy as np
import pytest
import torch

from tests import _lpips_ref as LR
from tests.test_gpu_evaluate import _read, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _renders(cfg, params, ds, layer):
    """the mirror renders of every frame in one call (phong, no shadow: the configs below), y_true and y_pred as (T,S,S,3)"""
    from harp_amd.optimize_sequence import get_mesh_subdivider
    from harp_amd.renderer import renderer_helper
    from harp_amd.structures import Meshes
    from harp_amd.utils.visualize import prepare_materials, prepare_mesh, render_image
    S, focal, T = cfg["img_size"], cfg["focal_length"], len(ds)
    fid = torch.arange(T)
    with torch.no_grad():
        lp = params["light_positions"][fid.to(DEV)]
        phong, _, _ = renderer_helper.get_renderers(image_size=S, light_posi=lp, silh_sigma=1e-7, silh_faces_per_pixel=50, device=DEV)
        _, v, f, t = prepare_mesh(params, fid, layer, False, get_mesh_subdivider(layer, device=DEV), False, cfg, device=DEV)
        y = render_image(Meshes(v, f, t), params["cam"][fid.to(DEV)], T, phong, S, focal, materials_properties=prepare_materials(params, T, device=DEV),
                         device=DEV)
    return torch.stack([d[1] for d in ds]).float(), y.float().cpu()


def test_evaluate_sequence_with_lpips_two_chunks(tmp_path):
    from harp_amd.lpips import LPIPS
    from harp_amd.optimize_sequence import evaluate_sequence
    sc, cfg, layer, params, ds = _setup(70, 176, 31, tmp_path, self_shadow=False, share_light_position=False)
    fn = LPIPS(weights="random", seed=4).to(DEV)
    stats = evaluate_sequence(cfg, params, ds, layer, device=DEV, batch_size=32, lpips_fn=fn)
    assert list(stats) == ["Silhouette IoU", "L1", "LPIPS", "MS_SSIM"]
    y_true, y_pred = _renders(cfg, params, ds, layer)
    # the float64 restatement on the first and last frame of each chunk; the kernel's per-frame values for the chunk means
    with torch.no_grad():
        per = fn(y_true.permute(0, 3, 1, 2).to(DEV), y_pred.permute(0, 3, 1, 2).to(DEV)).view(-1).double().cpu()
    idx = [0, 63, 64, 69]
    want = LR.lpips(y_true[idx].permute(0, 3, 1, 2), y_pred[idx].permute(0, 3, 1, 2), fn.state_dict())["total"]
    assert (per[idx] - want).abs().max() <= 2e-5 + 1e-4 * want.abs().max(), (per[idx], want)
    chunk_mean = float(np.mean([per[:64].mean().item(), per[64:].mean().item()]))
    print(f"[evaluate_sequence] LPIPS {stats['LPIPS']:.6f} (per-frame recomputation {chunk_mean:.6f})")
    assert abs(stats["LPIPS"] - chunk_mean) <= 1e-5 and stats["LPIPS"] > 0
    got = _read(tmp_path / "eval_results.txt")
    assert list(got) == ["Silhouette IoU", "L1", "LPIPS", "MS_SSIM"] and abs(got["LPIPS"] - stats["LPIPS"]) <= 5e-6


def test_lpips_weights_file_through_the_fit(tmp_path):
    """configs["lpips_weights"] = a combined state-dict file (what --lpips-weights sets), passed through optimize_hand_sequence(evaluate=True)"""
    from harp_amd.lpips import random_alex_weights
    from harp_amd.optimize_sequence import lpips_weights_arg, optimize_hand_sequence
    path = str(tmp_path / "lpips_alex.pth")
    torch.save(random_alex_weights(5), path)
    assert lpips_weights_arg([path]) == path and lpips_weights_arg(["a", "b"]) == ("a", "b")
    sc, cfg, layer, params, ds = _setup(4, 176, 32, tmp_path, total_epoch=2, training_stage=[1, 1, 0], lpips_weights=lpips_weights_arg([path]))
    optimize_hand_sequence(cfg, sc["seq"], ds, None, None, layer, torch.from_numpy(sc["tpl"]["verts_uvs"])[None],
                           torch.from_numpy(sc["tpl"]["faces_uvs"])[None], device=DEV, uv_mask=sc["uv_mask"], batch_size=2, evaluate=True)
    got = _read(tmp_path / "eval_results.txt")
    assert list(got) == ["Silhouette IoU", "L1", "LPIPS", "MS_SSIM"] and got["LPIPS"] > 0
