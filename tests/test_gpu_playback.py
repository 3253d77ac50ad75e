"""-m gpu: the playback half of the post-fit pass on the synthetic hand at S = 128 — render_360 / render_360_light / concat_image_in_dir
(utils/visualize.py:145-228, 322-355) rendered as one batch against the per-view path (render_image at batch 1 + ops.panels_u8), a
full turn against the unrotated mesh, and evaluate_sequence's `panels` / `turntable` switches (optimize_sequence.py:710-757)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.test_gpu_evaluate import _read, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 128

# share of pixels with a channel more than 2 levels off between view 35 (36 x 10 degrees = a full turn, 36 float32 rotations of rounding)
# and the render of the unrotated mesh, MEASURED on MI355X (profiles/normal_image_errors.txt); the test asserts 2 x these, and < 2 %
# whatever was measured, so that a wrong axis, angle or centre cannot pass
FULL_TURN_SHARE = {"phong": 0.0, "normal": 0.0}


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from harp_amd.optimize_sequence import get_mesh_subdivider
    sc, cfg, layer, params, ds = _setup(3, S, 11, tmp_path_factory.mktemp("playback"), self_shadow=False)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        params["normal_map"].copy_(torch.tensor([0., 0., 1.]).repeat(1, 512, 512, 1) + torch.randn(1, 512, 512, 3, generator=g) * 0.15)
    return dict(cfg=cfg, layer=layer, params=params, ds=ds, sub=get_mesh_subdivider(layer, device=DEV), focal=sc["focal"])


def _renderers(params, i=0):
    from harp_amd.renderer import renderer_helper
    return renderer_helper.get_renderers(image_size=S, light_posi=params["light_positions"][i:i + 1], silh_sigma=1e-7, silh_faces_per_pixel=50, device=DEV)


def _single_view(sc, renderer, verts, materials=True):
    """the per-view path: render_image at batch 1 on one vertex set -> (S,S,3) uint8"""
    from harp_amd import ops
    from harp_amd.structures import Meshes
    from harp_amd.utils.visualize import prepare_materials, prepare_mesh, render_image
    params = sc["params"]
    fid = torch.tensor([0])
    with torch.no_grad():
        _, _, faces, textures = prepare_mesh(params, fid, sc["layer"], False, sc["sub"], False, sc["cfg"], device=DEV)
        mat = prepare_materials(params, 1, device=DEV) if materials else dict()
        img = render_image(Meshes(verts[None].contiguous(), faces, textures), params["cam"][0:1], 1, renderer, S, sc["focal"], device=DEV,
                           materials_properties=mat)
        return ops.panels_u8(img)[0].cpu().numpy()


@pytest.mark.parametrize("kind", ["phong", "normal"])
def test_render_360_is_the_per_view_path_in_one_batch(scene, tmp_path, kind):
    from harp_amd.utils.visualize import prepare_mesh, render_360, turntable_vertices
    params = scene["params"]
    phong, _, normal = _renderers(params)
    renderer = phong if kind == "phong" else normal
    out = str(tmp_path) + "/"
    frames = render_360(params, torch.tensor([0]), renderer, S, scene["focal"], scene["layer"], configs=scene["cfg"], render_normal=kind == "normal",
                        verts_textures=False, mesh_subdivider=scene["sub"], save_img_dir=out, device=DEV)
    assert frames.shape == (72, S, S, 3) and frames.dtype == np.uint8
    d = os.path.join(out, "render_360_normal" if kind == "normal" else "render_360")
    names = ["%04d.jpg" % i for i in range(36)] + ["h_%04d.jpg" % i for i in range(36)]
    assert sorted(os.listdir(d)) == sorted(names + ["out.gif"])
    for nme in names:
        assert Image.open(os.path.join(d, nme)).size == (S, S)
    gif = Image.open(os.path.join(d, "out.gif"))
    assert gif.n_frames == 72 and gif.size == (S, S)
    with torch.no_grad():
        _, hand_verts, _, _ = prepare_mesh(params, torch.tensor([0]), scene["layer"], False, scene["sub"], False, scene["cfg"], device=DEV)
    verts = turntable_vertices(hand_verts)
    assert verts.shape == (72, hand_verts.shape[1], 3)
    differing = 0
    for k in range(72):
        differing += int((_single_view(scene, renderer, verts[k]) != frames[k]).sum())
    print(f"[turntable batch vs per-view] {kind}: {differing} differing uint8 values of {frames.size}")
    assert differing == 0
    assert (frames[0] != frames[18]).mean() > 0.01 and (frames[36] != frames[54]).mean() > 0.01      # the views do turn
    # a known answer: 36 x 10 degrees about Y is the unrotated mesh again
    still = _single_view(scene, renderer, hand_verts[0])
    share = float((np.abs(frames[35].astype(np.int32) - still.astype(np.int32)).max(-1) > 2).mean())
    half = float((np.abs(frames[17].astype(np.int32) - still.astype(np.int32)).max(-1) > 2).mean())
    print(f"[turntable full turn] {kind}: share of pixels more than 2 levels off after 360 degrees {share:.3e} (after 180: {half:.3e})")
    assert half > 0.02                                     # (half a turn is a different picture)
    assert share < 0.02
    rec = FULL_TURN_SHARE[kind]
    assert rec is not None, f"no recorded share for {kind!r} (measured now: {share:.3e})"
    assert share <= 2.0 * rec + 1e-12, (share, rec)


def test_concat_of_the_two_turntables(scene, tmp_path):
    from harp_amd.utils.visualize import concat_image_in_dir, render_360
    params = scene["params"]
    phong, _, normal = _renderers(params)
    out = str(tmp_path) + "/"
    kw = dict(configs=scene["cfg"], verts_textures=False, mesh_subdivider=scene["sub"], save_img_dir=out, device=DEV)
    render_360(params, torch.tensor([0]), phong, S, scene["focal"], scene["layer"], **kw)
    render_360(params, torch.tensor([0]), normal, S, scene["focal"], scene["layer"], render_normal=True, **kw)
    strips = concat_image_in_dir(out + "render_360", out + "render_360_normal", out + "render_360_combine")
    assert len(strips) == 72 and all(s.shape == (S, 2 * S, 3) for s in strips)
    assert sorted(os.listdir(out + "render_360_combine")) == ["%04d.jpg" % i for i in range(72)] + ["out.gif"]
    assert Image.open(out + "render_360_combine/0071.jpg").size == (2 * S, S)
    assert Image.open(out + "render_360_combine/out.gif").n_frames == 72


def test_render_360_light(scene, tmp_path):
    from harp_amd.renderer import renderer_helper
    from harp_amd.utils.visualize import prepare_mesh, render_360_light
    params = scene["params"]
    out = str(tmp_path) + "/"
    with torch.no_grad():
        _, hand_verts, faces, textures = prepare_mesh(params, torch.arange(2), scene["layer"], False, scene["sub"], False, scene["cfg"], device=DEV)
    frames = render_360_light(params, torch.tensor([0]), hand_verts[0:1], faces, textures, S, scene["focal"], save_img_dir=out, device=DEV)
    assert frames.shape == (40, S, S, 3) and frames.dtype == np.uint8
    d = out + "render_360_light"
    assert sorted(os.listdir(d)) == ["%04d.jpg" % i for i in range(40)] + ["out.gif"]
    assert Image.open(d + "/0039.jpg").size == (S, S) and Image.open(d + "/out.gif").n_frames == 40
    for k in range(40):
        phong, _, _ = renderer_helper.get_renderers(image_size=S, light_posi=torch.Tensor(((1.0, 1.0, -5.0 + k / 4.0),)), device=DEV)
        assert np.array_equal(_single_view(scene, phong, hand_verts[0], materials=False), frames[k]), k
    assert (frames[0] != frames[39]).mean() > 0.01         # the sweep does something


def _tree(base):
    return sorted(os.path.relpath(os.path.join(d, f), base) for d, _, fs in os.walk(base) for f in fs)


def test_evaluate_sequence_panels_and_turntable(scene, tmp_path):
    from harp_amd import ops
    from harp_amd.optimize_sequence import evaluate_sequence
    from harp_amd.renderer import renderer_helper
    from harp_amd.structures import Meshes
    from harp_amd.utils.visualize import prepare_materials, prepare_mesh, render_image
    params, ds, layer = scene["params"], scene["ds"], scene["layer"]
    T = len(ds)
    runs = {}
    for tag, kw in (("off", dict()), ("panels", dict(panels=True)), ("both", dict(panels=True, turntable=True))):
        base = tmp_path / tag
        base.mkdir()
        cfg = dict(scene["cfg"], base_output_dir=str(base) + "/")
        seen = {}
        with pytest.warns(UserWarning, match="MS_SSIM left out"):
            stats = evaluate_sequence(cfg, params, ds, layer, device=DEV, panel_hook=lambda fid, strip: seen.__setitem__(fid, strip.copy()), **kw)
        runs[tag] = (str(base), stats, seen, open(str(base / "eval_results.txt")).read())
    # flags off: exactly today's files
    assert _tree(runs["off"][0]) == ["eval_results.txt", "uv_out/normal_map.png", "uv_out/texture.png"] and not runs["off"][2]
    # the metrics do not depend on the flags
    assert runs["off"][3] == runs["panels"][3] == runs["both"][3] and runs["off"][1] == runs["panels"][1] == runs["both"][1]
    assert set(_read(os.path.join(runs["off"][0], "eval_results.txt"))) == {"Silhouette IoU", "L1"}
    # panels: one S x 4S JPEG per dataset item, named by its fid
    assert _tree(runs["panels"][0]) == ["eval_results.txt"] + ["rendered_after_opt/%04d.jpg" % i for i in range(T)] + ["uv_out/normal_map.png", "uv_out/texture.png"]
    for i in range(T):
        assert Image.open(os.path.join(runs["panels"][0], "rendered_after_opt/%04d.jpg" % i)).size == (4 * S, S)
    # ... of the four images rendered by hand through the mirror API
    cfgd = scene["cfg"]
    fid = torch.arange(T)
    with torch.no_grad():
        lp = params["light_positions"][0].repeat(T, 1) if cfgd["share_light_position"] else params["light_positions"][fid.to(DEV)]
        phong, sil, normal = renderer_helper.get_renderers(image_size=S, light_posi=lp, silh_sigma=1e-7, silh_faces_per_pixel=50, device=DEV)
        _, v, f, t = prepare_mesh(params, fid, layer, False, scene["sub"], False, cfgd, device=DEV)
        mesh, cam, mat = Meshes(v, f, t), params["cam"][fid.to(DEV)], prepare_materials(params, T, device=DEV)
        y_sil = render_image(mesh, cam, T, sil, S, scene["focal"], silhouette=True, device=DEV)
        y = render_image(mesh, cam, T, phong, S, scene["focal"], materials_properties=mat, device=DEV)
        y_n = render_image(mesh, cam, T, normal, S, scene["focal"], materials_properties=mat, device=DEV)
        y_true = torch.stack([d[1] for d in ds]).to(DEV).float()
        m_true = torch.stack([d[2][..., 0] for d in ds]).to(DEV).float()
        want = ops.panels_u8([y_true, y, y_n], m_true, y_sil).cpu().numpy()
    assert want.shape == (T, S, 4 * S, 3)
    for tag in ("panels", "both"):
        assert sorted(runs[tag][2]) == list(range(T))
        for i in range(T):
            assert np.array_equal(runs[tag][2][i], want[i]), (tag, i)
    assert (want[:, :, 2 * S:3 * S] != 255).mean() > 0.02 and want[:, :, 3 * S:, 1].max() == 0 and want[:, :, 3 * S:, 0].max() == 225
    # turntable: the reference's four directories next to the panels
    tree = _tree(runs["both"][0])
    for d, n in (("render_360", 72), ("render_360_normal", 72), ("render_360_combine", 72), ("render_360_light", 40)):
        got = [p for p in tree if p.startswith(d + "/")]
        assert len(got) == n + 1 and d + "/out.gif" in got and d + "/0000.jpg" in got, (d, len(got))
    assert "render_360/h_0035.jpg" in tree and "render_360_normal/h_0035.jpg" in tree
    assert Image.open(os.path.join(runs["both"][0], "render_360_combine/0000.jpg")).size == (2 * S, S)
