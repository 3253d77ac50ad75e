"""MANO-to-METRO preprocessing fits (harp_amd/metro_modifications/hand_utils.py) against the oracle restatement (oracle/metro_fit.py).
CPU: loss classes, spike filter, pickle helpers.  GPU: the native two-stage vertex fit (hipGraph replay vs eager vs oracle's
torch.optim.Adam), its full-length convergence, the arm variant and the sequence smoothing."""
import os

import numpy as np
import pytest
import torch

from tests._scene import make_scene

DEV = "cuda"
ARM_CORR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "harp_amd", "assets", "arm_corr.npz")


def test_loss_terms_and_spike_filter():
    from harp_amd.metro_modifications import hand_utils as hu
    from oracle import metro_fit as M
    g = torch.Generator().manual_seed(0)
    est = torch.randn(9, 21, 3, generator=g, dtype=torch.float64).float().requires_grad_()
    anchor = torch.randn(9, 21, 3, generator=g)
    for mine, ref in ((hu.LossAnchor(anchor, device="cpu").loss_func(est), M.keypoint_term(est, anchor)),
                      (hu.LossKeypoints3D(anchor, device="cpu").loss_func(est), M.keypoint_term(est, anchor - anchor[:, :1])),
                      (hu.LossSmoothPoses(1, 9).poses(est), M.window_term(est, 9)),
                      (hu.LossSmoothBodyMean().body(est), M.midpoint_term(est)),
                      (hu.LossSmoothCam().body(est), M.midpoint_term(est))):
        assert abs(mine.item() - ref.item()) <= 1e-6 * abs(ref.item())
        ga, gb = torch.autograd.grad(mine, est), torch.autograd.grad(ref, est)
        assert torch.allclose(ga[0], gb[0], rtol=1e-5, atol=1e-7)
    # two views: each half is smoothed on its own
    two = torch.randn(12, 5, 3, generator=g)
    assert abs(hu.LossSmoothPoses(2, 6).poses(two).item() - (M.window_term(two[:6], 6) + M.window_term(two[6:], 6)).item() / 2) < 1e-5
    li = hu.LossInit({"poses": np.ones((4, 45)), "shapes": np.zeros((4, 10))}, device="cpu")
    assert abs(li.init_poses(torch.zeros(4, 45)).item() - 45.0) < 1e-5 and li.init_shapes(torch.ones(4, 10)).item() == 10.0
    # spikes: isolated jumps in both directions are replaced, a step (one-sided jump) and the end frames are not
    pose = torch.randn(12, 45, generator=g) * 0.01
    pose[3] += 0.5; pose[7:] += 0.4; pose[10] -= 0.6
    out = hu.remove_spike({"pose": pose.clone()})["pose"]
    assert torch.equal(out, M.remove_spike(pose))
    assert not torch.equal(out[3], pose[3]) and torch.equal(out[7], pose[7]) and not torch.equal(out[10], pose[10])


def test_pickle_helpers_round_trip(tmp_path):
    from harp_amd.metro_modifications import hand_utils as hu
    g = torch.Generator().manual_seed(1)
    N = 4
    params = {"joints": torch.randn(N, 21, 3, generator=g), "verts": torch.randn(N, 778, 3, generator=g), "rot": torch.randn(N, 3, generator=g),
              "pose": torch.randn(N, 45, generator=g), "shape": torch.randn(N, 10, generator=g), "trans": torch.randn(N, 3, generator=g),
              "cam": torch.randn(N, 3, generator=g)}
    hu.write_pkl(params, str(tmp_path))
    import os, pickle
    names = sorted(os.listdir(tmp_path))
    assert names == ["%04d_mano.pkl" % i for i in range(1, N + 1)]                     # unscreen frames are numbered from 1
    with open(tmp_path / names[0], "rb") as f:
        rec = pickle.load(f)
    assert rec["pose"].shape == (1, 45) and rec["cam"].shape == (3,) and rec["joints"].shape == (1, 21, 3)
    back = hu.load_params(str(tmp_path))
    for k, v in params.items():
        assert torch.equal(back[k], v), k
    hu.write_pkl(params, str(tmp_path), unscreen=False)
    assert "0000_mano.pkl" in os.listdir(tmp_path)


def _targets(sc, B, seed):
    from oracle import harp_ref as H
    g = torch.Generator().manual_seed(seed)
    rot, pose = torch.randn(B, 3, generator=g) * 0.4, torch.randn(B, 45, generator=g) * 0.25
    shape, trans = torch.randn(B, 10, generator=g) * 0.5, torch.randn(B, 3, generator=g) * 0.05 + torch.tensor([0.0, 0.0, 0.6])
    with torch.no_grad():
        verts, _ = H.mano_forward(sc["model"], torch.cat((rot, pose), 1), shape, trans)
    return verts / 1000.0                                                               # METRO vertices are in metres


@pytest.mark.gpu
def test_vertex_fit_native_loop_vs_oracle(monkeypatch, capsys):
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.metro_modifications import hand_utils as hu
    from oracle import metro_fit as M
    sc = make_scene(T=2, S=32, seed=2)
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=sc["model_np"], device=DEV)
    pred = _targets(sc, 3, seed=5)
    monkeypatch.setattr(hu, "EPOCH_COARSE", 40)
    monkeypatch.setattr(hu, "EPOCH_FINE", 60)
    ref, ref_losses = M.fit_mano_to_vertices(sc["model"], pred, 40, 60)
    outs = {}
    for graph in (True, False):
        outs[graph] = hu.optimize_for_mano_param(pred, layer, use_graph=graph)
        printed = capsys.readouterr().out
        coarse, fine = (float(l.split(":")[1]) for l in printed.splitlines()[:2])
        assert abs(coarse - ref_losses[0]) <= 2e-3 * ref_losses[0] and abs(fine - ref_losses[1]) <= 2e-3 * ref_losses[1], (printed, ref_losses)
    for k in ("rot", "pose", "shape", "trans", "joints", "verts"):
        assert outs[True][k].dtype == np.float32 and outs[True][k].shape == tuple(ref[k].shape)
        # replayed graph == eager launches up to the order of the float atomics in the LBS backward
        assert np.abs(outs[True][k] - outs[False][k]).max() <= 1e-5 * max(1.0, np.abs(outs[True][k]).max()), k
    # 100 Adam steps on fp32: trajectories stay together to ~1e-3 of the parameter scale
    for k, tol in (("rot", 2e-3), ("pose", 2e-3), ("shape", 2e-3), ("trans", 2e-4)):
        assert np.abs(outs[True][k] - ref[k].numpy()).max() < tol, (k, np.abs(outs[True][k] - ref[k].numpy()).max())
    assert np.abs(outs[True]["verts"] - ref["verts"].numpy()).max() < 0.05               # mm


@pytest.mark.gpu
def test_vertex_fit_full_length_converges(capsys):
    """the reference's schedule (500 + 700 iterations) on 64 frames at once: every frame ends within the reference's acceptance
    threshold (MSE 10.0 mm^2, hand_utils.py:106-111) — here far below it"""
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.metro_modifications import hand_utils as hu
    sc = make_scene(T=2, S=32, seed=3)
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=sc["model_np"], device=DEV)
    pred = _targets(sc, 64, seed=9)
    out = hu.optimize_for_mano_param(pred, layer)
    assert "ERROR TOO HIGH" not in capsys.readouterr().out
    err = ((torch.from_numpy(out["verts"]) - pred * 1000.0) ** 2).mean((1, 2))
    assert err.max() < 1.0, err.max()
    assert all(np.isfinite(v).all() for v in out.values())


@pytest.mark.gpu
def test_arm_vertex_fit_runs(monkeypatch, capsys):
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    from harp_amd.metro_modifications import hand_utils as hu
    from harp_amd import synth
    model = synth.make_smplx_arm_model(seed=0)
    corr = np.load(ARM_CORR)
    layer = SMPLXARM(model, model["faces"], corr["mano_vert_from_arm"], device=DEV)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        verts, _ = layer(betas=torch.randn(2, 10, generator=g).to(DEV) * 0.3, global_orient=torch.randn(2, 3, generator=g).to(DEV) * 0.2,
                         transl=torch.randn(2, 3, generator=g).to(DEV) * 0.02, right_hand_pose=torch.randn(2, 45, generator=g).to(DEV) * 0.2,
                         return_type="mano")
    monkeypatch.setattr(hu, "EPOCH_COARSE", 60)
    monkeypatch.setattr(hu, "EPOCH_FINE", 150)
    out = hu.optimize_for_mano_arm_param(verts.cpu() / 1000.0, layer)
    coarse, fine = (float(l.split(":")[1]) for l in capsys.readouterr().out.splitlines()[:2])
    assert fine < coarse and np.isfinite(fine)
    assert out["verts"].shape == (2, 778, 3) and out["pose"].shape == (2, 45)


@pytest.mark.gpu
def test_sequence_smoothing_vs_oracle():
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.metro_modifications import hand_utils as hu
    from oracle import metro_fit as M
    sc = make_scene(T=8, S=32, seed=6)
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=sc["model_np"], device=DEV)
    seq = sc["seq"]
    g = torch.Generator().manual_seed(8)
    params = {"joints": seq["joints"].float(), "rot": seq["rot"].float(), "pose": (seq["pose"] + torch.randn(8, 45, generator=g) * 0.05).float(),
              "shape": seq["shape"].float(), "trans": seq["trans"].float(), "cam": seq["cam"].float()}
    ref = M.smooth_sequence(sc["model"], {k: v.clone() for k, v in params.items()}, img_res=224, total_iter_pose=12, total_iter_cam=12)
    out = hu.optimize_smooth_seq({k: v.clone() for k, v in params.items()}, layer, img_res=224, total_iter_pose=12, total_iter_cam=12)
    assert set(out) == set(ref) and out["cam"].shape == (8, 3) and not out["cam"].is_cuda
    for k in ("rot", "pose", "shape", "cam"):
        moved = (ref[k] - params[k]).abs().max().item()
        assert moved > 0 and (out[k] - ref[k]).abs().max().item() <= 0.05 * moved + 1e-6, (k, moved, (out[k] - ref[k]).abs().max().item())
    assert (out["verts"] - ref["verts"]).abs().max() < 0.05 and torch.equal(out["trans"], params["trans"])
