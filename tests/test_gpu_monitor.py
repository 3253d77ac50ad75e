"""-m gpu: the in-fit monitor (harp_amd/monitor.py) on a synthetic 6-frame 96 x 96 scene: back-pressure and error hand-over of the writer
thread; show_img_pair / visualize_val against the numpy restatement of their sheets and an independent mirror render over the merged
parameter dict; optimize_hand_sequence(monitor=...) end to end."""
import json
import os
import re
import threading

import numpy as np
import pytest
import torch

from tests._sheet_ref import normal_levels_f64, numpy_sheet
from tests.test_gpu_evaluate import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, S = 6, 96
SHEET = re.compile(r"^(|sil_|loss_|val_|uv_|normal_)\d{4}\.jpg$")


def _val_params(sc, seed=5):
    """a validation track whose cam, trans and rot all differ from the fit's"""
    g = torch.Generator().manual_seed(seed)
    seq = sc["seq"]
    cam = seq["cam"].clone().float()
    cam[:, 0] *= 0.9
    cam[:, 1:] += 0.03 * torch.randn(cam.shape[0], 2, generator=g)
    return {"cam": cam, "trans": seq["trans"].float() + 0.004 * torch.randn(seq["trans"].shape, generator=g),
            "rot": seq["rot"].float() + 0.1 * torch.randn(seq["rot"].shape, generator=g)}


def test_backpressure_and_writer_errors(tmp_path):
    from harp_amd import ops
    from harp_amd.monitor import FitMonitor, encode_jpeg
    gate = threading.Event()

    def gated(path, u8):
        assert gate.wait(30), "the gate never opened"
        encode_jpeg(path, u8)

    base = str(tmp_path) + "/"
    mon = FitMonitor(base, slots=4, encode_fn=gated)
    imgs = torch.rand(3, 9, S, S, 3, device=DEV)
    try:
        for k in range(3):
            mon.submit("s%d.jpg" % k, ops.sheet_u8(imgs[k]))
        assert mon.pending == 3 and mon.waits == 0 and not gate.is_set()     # three of four slots taken, nobody waited for the encoder
    finally:
        gate.set()
        mon.close()
    assert mon.pending == 0 and mon.submitted == 3
    from PIL import Image
    for k in range(3):
        assert Image.open(base + "s%d.jpg" % k).size == (3 * S, 3 * S)
    assert len(mon.timings) == 3 and all(t["copy_ms"] >= 0 and t["encode_ms"] >= 0 for t in mon.timings)

    def broken(path, u8):
        raise OSError("disk full: " + os.path.basename(path))

    mon = FitMonitor(base, slots=2, encode_fn=broken)
    mon.submit("bad.jpg", ops.sheet_u8(imgs[0]))
    with pytest.raises(OSError, match="disk full: bad.jpg"):
        mon.close()
    mon.close()                                                              # raised once; closing again is a no-op


def _independent_render(cfg, P, fid, layer):
    """the mirror render of visualize_val (optimize_sequence.py:110-154) written out here, not through the package's helper"""
    from harp_amd.optimize_sequence import get_mesh_subdivider
    from harp_amd.renderer import renderer_helper
    from harp_amd.structures import Meshes
    from harp_amd.utils.visualize import prepare_materials, prepare_mesh, render_image, render_image_with_RT
    n, focal = fid.shape[0], cfg["focal_length"]
    with torch.no_grad():
        lp = P["light_positions"][0].repeat(n, 1) if cfg["share_light_position"] else P["light_positions"][fid.to(DEV)]
        phong, _, _ = renderer_helper.get_renderers(image_size=S, light_posi=lp, silh_sigma=1e-7, silh_faces_per_pixel=50, device=DEV)
        _, v, f, t = prepare_mesh(P, fid, layer, False, get_mesh_subdivider(layer, device=DEV), False, cfg, device=DEV)
        mesh, cam, mat = Meshes(v, f, t), P["cam"][fid.to(DEV)], prepare_materials(P, n, device=DEV)
        if cfg["self_shadow"]:
            lR, lT, cR, cT = renderer_helper.process_info_for_shadow(cam, lp, v.mean(1), image_size=S, focal_length=focal, device=DEV)
            shadow = renderer_helper.get_shadow_renderers(image_size=S, light_posi=lp, amb_ratio=torch.sigmoid(P["amb_ratio"]), device=DEV)
            return render_image_with_RT(mesh, lT, lR, cT, cR, n, shadow, S, focal, materials_properties=mat, device=DEV).float()
        return render_image(mesh, cam, n, phong, S, focal, materials_properties=mat, device=DEV).float()


@pytest.mark.parametrize("shadow", [True, False])
def test_show_img_pair_and_visualize_val(tmp_path, shadow):
    from harp_amd.optimize_sequence import get_mesh_subdivider, show_img_pair, visualize_val
    sc, cfg, layer, params, ds = _setup(T, S, 41, tmp_path, self_shadow=shadow, share_light_position=shadow)
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        params["normal_map"].add_(0.2 * torch.randn(1, 512, 512, 3, generator=g).to(DEV))
    val = _val_params(sc)
    fid = torch.tensor([4, 0, 2])
    batch = (fid, torch.stack([ds[i][1] for i in fid]), torch.stack([ds[i][2] for i in fid]), torch.stack([ds[i][3] for i in fid]))
    seen = {}
    hook = lambda name, u8, sources: seen.__setitem__(name, (u8, {k: v.detach().cpu().numpy() for k, v in sources.items()}))
    visualize_val([batch], 20, DEV, params, val, cfg, layer, get_mesh_subdivider(layer, device=DEV), None, False, False, True, sheet_hook=hook)
    assert sorted(seen) == ["normal_0020.jpg", "uv_0020.jpg", "val_0020.jpg"]
    assert sorted(f for f in os.listdir(tmp_path) if SHEET.match(f)) == sorted(seen)
    u8, src = seen["val_0020.jpg"]
    assert u8.shape == (3 * S, 3 * S, 3) and np.array_equal(u8, numpy_sheet(0, src["y_pred"], grid=(3, 3), d=1))
    assert (u8[S:] == 255).all() and (u8[:S] != 255).any()                  # three frames: the lower two rows of cells are empty
    # the sources against an independent render over the merged dict: the fit's shape / pose / appearance under the validation cam, trans, rot
    merged = dict(params)
    merged.update({k: v.to(DEV) for k, v in val.items()})
    want = _independent_render(cfg, merged, fid, layer).cpu().numpy()
    own_cam = _independent_render(cfg, params, fid, layer).cpu().numpy()
    diff = float(np.abs(src["y_pred"] - want).max())
    print(f"[monitor] visualize_val sources vs independent mirror render, shadow={shadow}: max |diff| = {diff:.3e} "
          f"(against the fit's own cam / trans / rot: {float(np.abs(src['y_pred'] - own_cam).max()):.3e})")
    assert np.abs(src["y_pred"] - own_cam).max() > 0.05                     # a wrong merge would be seen
    assert np.array_equal(src["y_pred"], want)                              # two runs of the same deterministic forward kernels
    u8, src = seen["uv_0020.jpg"]
    assert u8.shape == (512, 512, 3) and np.array_equal(u8, numpy_sheet(0, src["texture"], grid=(1, 1), d=1))
    assert np.array_equal(src["texture"], params["texture"].detach().cpu().numpy())
    u8, src = seen["normal_0020.jpg"]
    v = normal_levels_f64(src["normal_map"])[0]
    frac = v - np.floor(v)
    decided = (frac >= 0.01) & (frac <= 0.99)
    lvl = u8.astype(np.int64)
    assert np.abs(lvl - np.floor(v)).max() <= 1 and np.array_equal(lvl[decided], np.floor(v)[decided].astype(np.int64)) and decided.mean() > 0.9

    # show_img_pair: numpy input is uploaded; without save_img_dir the sheet comes back
    tg = sc["targets"]
    sil_true, sil_pred = tg["y_sil"].numpy(), tg["y_sil_col"][..., None].numpy()
    got = show_img_pair(sil_pred, sil_true, step=7, silhouette=True, sheet_hook=hook)
    assert np.array_equal(got, numpy_sheet(1, sil_true, sil_pred[..., 0], grid=(3, 3), d=1)) and np.array_equal(seen["sil_0007.jpg"][0], got)
    assert show_img_pair(tg["y_true"].to(DEV), None, step=7, save_img_dir=str(tmp_path) + "/", prefix="loss_", sheet_hook=hook) is None
    assert np.array_equal(seen["loss_0007.jpg"][0], numpy_sheet(0, tg["y_true"].numpy(), grid=(3, 3), d=1))
    from PIL import Image
    assert Image.open(tmp_path / "loss_0007.jpg").size == (3 * S, 3 * S)
    big = torch.rand(2, 512, 512, 3)
    assert np.array_equal(show_img_pair(big, None), numpy_sheet(0, big.numpy(), grid=(3, 3), d=2))          # 512 px: box factor 2, 768 px


def _fit(tmp_path, monitor, with_val=True, **kw):
    from harp_amd.optimize_sequence import optimize_hand_sequence
    sc, cfg, layer, params, ds = _setup(T, S, 42, tmp_path, total_epoch=21, training_stage=[7, 7, 7])
    val, val_ds = (_val_params(sc), ds[:3]) if with_val else (None, None)
    optimize_hand_sequence(cfg, sc["seq"], ds, val, val_ds, layer, torch.from_numpy(sc["tpl"]["verts_uvs"])[None],
                           torch.from_numpy(sc["tpl"]["faces_uvs"])[None], device=DEV, uv_mask=sc["uv_mask"], batch_size=2, monitor=monitor, **kw)
    return sorted(f for f in os.listdir(tmp_path) if SHEET.match(f) or f.endswith(".jsonl"))


def test_fit_with_monitor(tmp_path):
    from PIL import Image
    seen = []
    files = _fit(tmp_path, dict(sheet_hook=lambda name, u8, sources: seen.append((name, u8, sources))))
    want = [p + "%04d.jpg" % e for p in ("", "sil_", "loss_") for e in (0, 10, 20)] + [p + "%04d.jpg" % e for p in ("val_", "uv_", "normal_") for e in (0, 20)]
    assert files == sorted(want + ["monitor_log.jsonl"])
    for f in want:
        im = Image.open(tmp_path / f)
        assert im.mode == "RGB" and im.size == ((512, 512) if f.startswith(("uv_", "normal_")) else (3 * S, 3 * S)), f
    lines = [json.loads(ln) for ln in open(tmp_path / "monitor_log.jsonl")]
    assert [ln["epoch"] for ln in lines] == list(range(21))
    for ln in lines:
        assert np.isfinite(ln["total_loss_epoch"]) and ln["lr_coarse"] > 0
        assert (ln["coarse"], ln["app"]) == (ln["epoch"] < 14, ln["epoch"] >= 7)
        assert ("val_iou" in ln) == ("val_l1" in ln) == (ln["epoch"] in (0, 20))
    for ln in (lines[0], lines[20]):
        assert 0.0 <= ln["val_iou"] <= 1.0 and np.isfinite(ln["val_l1"]) and ln["val_l1"] >= 0
    # what the writer thread saw: every sheet is the restatement of its own sources; two frames of the batch, seven empty cells
    assert sorted(n for n, _, _ in seen) == sorted(want)
    for name, u8, src in seen:
        src = {k: v.cpu().numpy() for k, v in src.items()}
        if name.startswith("sil_"):
            assert np.array_equal(u8, numpy_sheet(1, src["y_sil_true"], src["y_sil_pred"].reshape(src["y_sil_true"].shape))), name
        elif name.startswith("loss_"):
            assert np.array_equal(u8, numpy_sheet(2, src["y_true"], src["y_pred"], src["y_sil_true_col"])), name
        elif name.startswith("uv_"):
            assert np.array_equal(u8, numpy_sheet(0, src["texture"], grid=(1, 1))), name
        elif not name.startswith("normal_"):
            assert np.array_equal(u8, numpy_sheet(0, src["y_pred"])), name
            assert src["y_pred"].shape[0] == (3 if name.startswith("val_") else 2)
    first = dict((n, u) for n, u, _ in seen)
    assert not np.array_equal(first["0000.jpg"], first["0020.jpg"])         # the fit moved between the sheets


def test_writer_thread_calls_the_runtime_only_under_the_lock(tmp_path, monkeypatch):
    """A step graph is captured in the mode in which an event call from ANY thread fails and invalidates the capture (seen on the MI355X:
    elapsed_time on the writer thread during a capture -> hipErrorStreamCaptureUnsupported, the step's launch status 903).  The contract
    that excludes it: the writer thread's event calls happen under FitMonitor.hip_lock, never as a blocking synchronize, and the fit
    holds that lock whenever it captures."""
    from harp_amd.monitor import FitMonitor
    mon = FitMonitor(str(tmp_path) + "/")
    calls, captures = [], []
    for name in ("query", "elapsed_time", "synchronize"):
        def spy(self, *a, _orig=getattr(torch.cuda.Event, name), _name=name):
            if threading.current_thread().name == "harp-fit-monitor":
                calls.append((_name, mon.hip_lock.locked()))
            return _orig(self, *a)
        monkeypatch.setattr(torch.cuda.Event, name, spy)
    begin = torch.cuda.CUDAGraph.capture_begin

    def spy_begin(self, *a, **k):
        captures.append(mon.hip_lock.locked())
        return begin(self, *a, **k)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "capture_begin", spy_begin)
    files = _fit(tmp_path, mon)
    assert len(files) == 16 and len(mon.timings) == 15
    assert len(captures) >= 3 and all(captures)                             # one graph per stage at least, each captured under the lock
    assert {n for n, _ in calls} == {"query", "elapsed_time"} and all(held for _, held in calls)


def test_fit_without_monitor_writes_nothing_new(tmp_path):
    assert _fit(tmp_path, False) == []


def test_monitor_without_validation_set(tmp_path):
    files = _fit(tmp_path, True, with_val=False)
    assert files == sorted([p + "%04d.jpg" % e for p in ("", "sil_", "loss_") for e in (0, 10, 20)] + ["monitor_log.jsonl"])
    lines = [json.loads(ln) for ln in open(tmp_path / "monitor_log.jsonl")]
    assert len(lines) == 21 and not any("val_iou" in ln for ln in lines)


def test_validation_fid_outside_the_pose_table(tmp_path):
    from harp_amd.optimize_sequence import optimize_hand_sequence
    sc, cfg, layer, params, ds = _setup(T, S, 42, tmp_path, total_epoch=1, training_stage=[1, 0, 0])
    val_ds = [(T + 1,) + tuple(ds[0][1:])]
    with pytest.raises(ValueError, match="validation frame ids"):
        optimize_hand_sequence(cfg, sc["seq"], ds, _val_params(sc), val_ds, layer, torch.from_numpy(sc["tpl"]["verts_uvs"])[None],
                               torch.from_numpy(sc["tpl"]["faces_uvs"])[None], device=DEV, uv_mask=sc["uv_mask"], batch_size=2, monitor=True)
