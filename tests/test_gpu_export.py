"""-m gpu: evaluate_sequence(export_mesh=True) (optimize_sequence.py:776-791) on the small synthetic scene of the evaluation tests: one
Taubin-smoothed textured OBJ per dataset frame under mesh/, every other output of the evaluation as without the switch."""
import os

import numpy as np
import pytest
import torch

from tests._scene import make_scene
from tests.test_io_cpu import read_obj

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, S = 4, 96                           # the smallest image the evaluation tests use (no MS_SSIM line at this size)
FIDS = (3, 0, 2)                       # the dataset: three of the four fitted frames, out of order, two batches of batch_size 2


@pytest.fixture(scope="module")
def scene():
    from harp_amd.manopth.manolayer import ManoLayer
    sc = make_scene(T=T, S=S, seed=31)
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=sc["model_np"], device=DEV)
    tg = sc["targets"]
    ds = [(i, tg["y_true"][i], tg["y_sil"][i][..., None], tg["y_sil_col"][i][..., None]) for i in FIDS]
    return sc, layer, ds


def _params(sc, layer, cfg):
    from harp_amd.optimize_sequence import init_params
    params = init_params(sc["seq"], True, True, None, layer.th_faces, False, torch.from_numpy(sc["tpl"]["verts_uvs"])[None],
                         torch.from_numpy(sc["tpl"]["faces_uvs"])[None], configs=cfg, device=DEV, uv_mask=sc["uv_mask"])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        params["texture"].copy_(torch.rand(1, 512, 512, 3, generator=g) * 1.2 - 0.1)          # leaves [0, 1]: the export clamps
        params["verts_disps"].copy_(torch.randn(3093, 1, generator=g) * 5e-4)                 # a rough surface for the smoothing to act on
        params["trans"].copy_(torch.randn(T, 3, generator=g) * 0.01)
    return params


@pytest.mark.filterwarnings("ignore:MS_SSIM left out")
def test_export_mesh_writes_the_smoothed_textured_meshes(tmp_path, scene):
    from PIL import Image
    from harp_amd import ops
    from harp_amd.optimize_sequence import evaluate_sequence, get_mesh_subdivider
    from harp_amd.structures import Meshes
    from harp_amd.utils.config_utils import get_config
    from harp_amd.utils.visualize import prepare_mesh
    sc, layer, ds = scene
    on, off = tmp_path / "on", tmp_path / "off"
    stats, text = {}, {}
    for d, flag in ((on, True), (off, False)):
        d.mkdir()
        cfg = get_config(write_yaml=False, use_arm=False, img_size=S, focal_length=sc["focal"], base_output_dir=str(d) + "/")
        params = _params(sc, layer, cfg)
        stats[flag] = evaluate_sequence(cfg, params, ds, layer, device=DEV, batch_size=2, export_mesh=flag)
        text[flag] = open(d / "eval_results.txt", "rb").read()
    # ---- everything else is as without the switch, and without it there is no mesh/
    assert stats[True] == stats[False] and list(stats[True]) == ["Silhouette IoU", "L1"]
    assert text[True] == text[False]
    assert not (off / "mesh").exists()
    assert sorted(os.listdir(off)) == sorted(set(os.listdir(on)) - {"mesh"})
    for f in ("texture.png", "normal_map.png"):
        assert open(on / "uv_out" / f, "rb").read() == open(off / "uv_out" / f, "rb").read()
    # ---- one .obj / .mtl / .png per dataset frame, named by its fid
    assert sorted(os.listdir(on / "mesh")) == sorted("%04d.%s" % (f, e) for f in FIDS for e in ("obj", "mtl", "png"))
    fid = torch.tensor(FIDS)
    with torch.no_grad():
        _, verts, faces, textures = prepare_mesh(params, fid, layer, False, get_mesh_subdivider(layer, device=DEV), False, cfg, device=DEV)
        want = ops.taubin_smoothing(Meshes(verts, faces, textures)).verts_padded().cpu()
    moved = (want - verts.cpu()).abs().max().item()
    print(f"[export] the smoothing moved the vertices by up to {moved * 1e3:.3f} mm")
    assert moved > 1e-4                                                    # the files hold the SMOOTHED mesh: 1e-6 below tells them apart
    topo = faces._harp_topo
    tex_u8 = (params["texture"][0].detach().cpu().clamp(0, 1) * 255.0).to(torch.uint8).numpy()
    png0 = open(on / "mesh" / ("%04d.png" % FIDS[0]), "rb").read()
    for b, f in enumerate(FIDS):
        o = read_obj(on / "mesh" / ("%04d.obj" % f))
        assert o["mtllib"] == ["%04d.mtl" % f] and o["usemtl"] == ["mesh"]
        assert (torch.tensor(o["v"], dtype=torch.float64) - want[b].double()).abs().max().item() <= 1e-6
        assert (torch.tensor(o["f"]) - 1).equal(topo.faces.cpu().long())
        assert (torch.tensor(o["ft"]) - 1).equal(torch.from_numpy(sc["tpl"]["faces_uvs"]).long().reshape(-1, 3))
        assert (torch.tensor(o["vt"], dtype=torch.float64) - torch.from_numpy(sc["tpl"]["verts_uvs"]).double().reshape(-1, 2)).abs().max() <= 5e-7
        assert "map_Kd %04d.png" % f in open(on / "mesh" / ("%04d.mtl" % f)).read()
        assert open(on / "mesh" / ("%04d.png" % f), "rb").read() == png0   # one shared texture, encoded once
    assert np.array_equal(np.asarray(Image.open(on / "mesh" / ("%04d.png" % FIDS[0]))), tex_u8)


@pytest.mark.filterwarnings("ignore:MS_SSIM left out")
def test_fit_passes_export_mesh_through(tmp_path, scene):
    from harp_amd.optimize_sequence import optimize_hand_sequence
    from harp_amd.utils.config_utils import get_config
    sc, layer, _ = scene
    tg = sc["targets"]
    ds = [(i, tg["y_true"][i], tg["y_sil"][i][..., None], tg["y_sil_col"][i][..., None]) for i in range(T)]
    cfg = get_config(write_yaml=False, use_arm=False, img_size=S, focal_length=sc["focal"], base_output_dir=str(tmp_path) + "/", total_epoch=1,
                     training_stage=[1, 0, 0])
    optimize_hand_sequence(cfg, sc["seq"], ds, None, None, layer, torch.from_numpy(sc["tpl"]["verts_uvs"])[None],
                           torch.from_numpy(sc["tpl"]["faces_uvs"])[None], device=DEV, uv_mask=sc["uv_mask"], batch_size=2, evaluate=True,
                           export_mesh=True)
    assert sorted(os.listdir(tmp_path / "mesh")) == sorted("%04d.%s" % (f, e) for f in range(T) for e in ("obj", "mtl", "png"))
    assert len(read_obj(tmp_path / "mesh" / "0003.obj")["v"]) == 3093
