"""The pure parts of the in-fit monitor (harp_amd/monitor.py): box factor, cadence, the dict merge of visualize_val, and the command
line's --monitor switch reaching optimize_hand_sequence.  No GPU."""
import inspect

import pytest
import torch


def test_box_factor():
    from harp_amd.monitor import box_factor
    # the smallest d with 3 * ceil(S / d) <= 1024
    assert [box_factor(S) for S in (96, 341, 342, 512, 1024)] == [1, 1, 2, 2, 4]
    assert [3 * -(-S // box_factor(S)) for S in (96, 341, 342, 512, 1024)] == [288, 1023, 513, 768, 768]
    for S in range(1, 1400, 7):
        d = box_factor(S)
        assert 3 * -(-S // d) <= 1024 and (d == 1 or 3 * -(-S // (d - 1)) > 1024), S
    assert box_factor(512, max_side=512, cells=1) == 1 and box_factor(512, max_side=300) == 6


def test_cadence():
    from harp_amd.monitor import FitMonitor, due
    mon = FitMonitor("unused/")
    assert (mon.train_every, mon.val_every, mon.max_side) == (10, 20, 1024)
    assert [e for e in range(21) if due(e, mon.train_every)] == [0, 10, 20]
    assert [e for e in range(21) if due(e, mon.val_every)] == [0, 20]
    assert [e for e in range(301) if due(e, 20)][-1] == 300 and not any(due(e, 0) for e in range(5))
    assert mon.pending == 0
    mon.close()                                                  # never started: nothing to join


def test_merge_takes_camera_and_root_from_the_validation_track():
    from harp_amd.monitor import merge_val_params
    fit = {k: torch.full((2, 3), 1.0) for k in ("cam", "trans", "rot", "pose", "light_positions")}
    fit["texture"] = torch.zeros(1, 4, 4, 3)
    val = {k: torch.full((5, 3), 2.0, dtype=torch.float64) for k in ("cam", "trans", "rot", "pose")}
    out = merge_val_params(fit, val, "cpu")
    assert all(out[k].shape == (5, 3) and out[k].dtype == torch.float32 and (out[k] == 2).all() for k in ("cam", "trans", "rot"))
    assert all(out[k] is fit[k] for k in ("pose", "light_positions", "texture"))
    assert (fit["cam"] == 1).all() and val["cam"].dtype == torch.float64                  # neither input is written


def test_reference_signatures():
    from harp_amd import optimize_sequence as O
    assert list(inspect.signature(O.show_img_pair).parameters)[:6] == ["ypred_np", "ytrue_np", "step", "silhouette", "save_img_dir", "prefix"]
    assert list(inspect.signature(O.visualize_val).parameters)[:12] == [
        "val_images_dataloader", "epoch_id", "device", "params", "val_params", "configs", "hand_layer", "mesh_subdivider", "opt_app",
        "use_verts_textures", "GLOBAL_POSE", "SHARED_TEXTURE"]
    assert inspect.signature(O.optimize_hand_sequence).parameters["monitor"].default is False


@pytest.mark.parametrize("flag", [True, False])
def test_main_passes_the_monitor_switch(tmp_path, monkeypatch, flag):
    from harp_amd import optimize_sequence as O
    from harp_amd.utils import data_util, hand_model_utils
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("use_arm: false\nimg_size: 96\nbase_output_dir: %s/\n" % tmp_path)
    got = {}
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda configs: ("layer", "uvs", "fuvs", None))
    monkeypatch.setattr(data_util, "load_multiple_sequences", lambda *a, **k: ("mano", "images", "val_mano", "val_images"))
    monkeypatch.setattr(O, "optimize_hand_sequence", lambda *a, **k: got.update(args=a, kw=k) or "params")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert O.main(["--config", str(cfg)] + (["--monitor"] if flag else [])) == "params"
    assert got["kw"]["monitor"] is flag and got["args"][3:5] == ("val_mano", "val_images")
    assert got["args"][0]["img_size"] == 96
