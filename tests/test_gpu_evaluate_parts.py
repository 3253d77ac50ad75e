"""-m gpu: the parts of the post-fit evaluation (harp_amd/evaluate.py) share nothing but the batch and its render — a run with every
switch on (the turntable aside: tests/test_gpu_playback.py has it) gives, number for number and byte for byte, what the runs with one
switch each give.  5 frames of 176 px (the smallest side that keeps MS_SSIM) in batches of 2: three batches, the last one short, fid 0 in
the first.  The renders and metrics are deterministic, so every comparison is `==`."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_evaluate import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, S = 5, 176
IMAGE, LPIPS_KEY, COVERAGE = ["Silhouette IoU", "L1", "MS_SSIM"], ["LPIPS"], ["Texel coverage"]
POSE = ["Procrustes-aligned joint error (mm)", "Joint AUC 0-50 mm", "Procrustes-aligned vertex error (mm)", "Vertex AUC 0-50 mm", "F@5mm", "F@15mm"]
KEYS = ["Silhouette IoU", "L1", "LPIPS", "MS_SSIM"] + POSE + COVERAGE


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _pose_ground_truth(cfg, layer, params):
    """as tests/test_gpu_pose_eval.py builds it: a similarity transform of the fitted joints (mm) / vertices (m) plus noise; frame 1 with
    two valid joints only, which leaves it out of the joint lines"""
    from harp_amd.optimize_sequence import get_mesh_subdivider
    from harp_amd.utils.visualize import prepare_mesh
    with torch.no_grad():
        j, v, _, _ = prepare_mesh(params, torch.arange(T), layer, False, get_mesh_subdivider(layer, device=DEV), False, cfg, device=DEV)
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    gt_v = 1.3 * v[:, :778].double().cpu().numpy() @ q.T + np.array([0.02, -0.01, 0.3]) + rng.normal(size=(T, 778, 3)) * 2e-3
    gt_j = 1.1 * (j[:, :21].double().cpu().numpy() * 1000.0) @ q.T + np.array([3.0, 4.0, -50.0]) + rng.normal(size=(T, 21, 3)) * 2.0
    jv = np.ones((T, 21), dtype=np.float32)
    jv[0, [3, 17]] = 0.0
    jv[1] = 0.0
    jv[1, [4, 9]] = 1.0
    return {"gt_joints": gt_j.astype(np.float32), "gt_joint_valid": jv, "gt_verts": gt_v.astype(np.float32)}


def test_all_switches_equal_each_switch_alone(tmp_path):
    from harp_amd.evaluate import evaluate_sequence
    from harp_amd.lpips import LPIPS
    sc, cfg, layer, params, ds = _setup(T, S, 21, tmp_path)
    single = {"nothing": {},
              "lpips": {"lpips_fn": LPIPS(weights="random", seed=4).to(DEV)},
              "pose": {"pose_eval": _pose_ground_truth(cfg, layer, params)},
              "panels": {"panels": True},
              "export": {"export_mesh": True, "pad_texture": 2},
              "coverage": {"coverage": True}}
    runs = dict(single, all={k: v for kw in single.values() for k, v in kw.items()})
    stats, files = {}, {}
    for name in ["all"] + list(single):
        out = tmp_path / name
        out.mkdir()
        stats[name] = evaluate_sequence(dict(cfg, base_output_dir=str(out) + "/"), params, ds, layer, device=DEV, batch_size=2, **runs[name])
        files[name] = {f: open(out / f, "rb").read() for f in _files(out)}
    # ---- the lines and their order
    assert list(stats["all"]) == KEYS
    own = {"nothing": IMAGE, "lpips": ["Silhouette IoU", "L1", "LPIPS", "MS_SSIM"], "pose": IMAGE + POSE, "coverage": IMAGE + COVERAGE}
    for name in single:
        assert list(stats[name]) == own.get(name, IMAGE), name
        for k, x in stats[name].items():
            assert stats["all"][k] == x, (name, k, stats["all"][k], x)
    assert np.loadtxt(tmp_path / "all" / "eval_joint_mm.txt").shape == (T - 1,) and np.loadtxt(tmp_path / "all" / "eval_vert_mm.txt").shape == (T,)
    # ---- the files: the union of the single runs', byte for byte
    assert set(files["all"]) == set().union(*(files[name] for name in single))
    assert set(files["export"]) - set(files["nothing"]) == {os.path.join("mesh", "%04d.%s" % (i, e)) for i in range(T) for e in ("obj", "mtl", "png")}
    assert set(files["panels"]) - set(files["nothing"]) == {os.path.join("rendered_after_opt", "%04d.jpg" % i) for i in range(T)}
    assert set(files["pose"]) - set(files["nothing"]) == {"eval_joint_mm.txt", "eval_vert_mm.txt"}
    assert set(files["coverage"]) - set(files["nothing"]) == {os.path.join("uv_out", f) for f in ("coverage.png", "baked_texture.png", "texture_std.png")}
    assert set(files["lpips"]) == set(files["nothing"]) == {"eval_results.txt", os.path.join("uv_out", "texture.png"), os.path.join("uv_out", "normal_map.png")}
    for name in single:
        for f, data in files[name].items():
            if f != "eval_results.txt":
                assert files["all"][f] == data, (name, f)
    # ---- eval_results.txt: the union of the single runs' lines, in key order
    lines = {ln for name in single for ln in files[name]["eval_results.txt"].decode().splitlines()}
    assert len(lines) == len(KEYS)
    assert files["all"]["eval_results.txt"].decode().splitlines() == sorted(lines, key=lambda ln: KEYS.index(ln.split(":")[0][1:]))
