"""What the batched inverse kinematics of the SMPL-X arm costs (csrc/arm_ik.hip): ops.arm_ik with 15 iterations at T = 256 and
T = 4096 frames of the synthetic arm (wrist and pose sigma 0.3, root rotations up to 3.1 rad, trans within 0.3 m) from the layer's start,
22 keypoints with the wrist solved and 21 with it held, beside its two siblings on the same frame counts — ops.mano_ik (the synthetic hand,
15 iterations from the palm start) and ops.arm_vertex_fit (778 targets, wrist held, 10 iterations from the rigid start) — and beside what
the solved rows are for: AvatarPlayer on a use_arm fit at 512 x 512, ss = 1.  No route from keypoints to arm rows existed before, so there
is no baseline to divide by; the one expectation to confirm or refute is that the solve stays faster than the arm player.

Method (tools/dev/gpu_ik_time.py's): warm-up, then device events around one call, median [min .. max] over `--repeats` calls, one process.
Also the wall-clock time of Motion.from_arm_keypoints as a whole, host-side start and uploads included.

    python tools/dev/gpu_arm_ik_time.py [--repeats 7] [--out profiles/arm_ik_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gpu_ik_time import event_ms  # noqa: E402
from gpu_playback_time import stats  # noqa: E402


def arm_fit(T, S, dev, seed=3):
    """a synthetic use_arm fit: (configs, layer, params, model)"""
    from harp_amd import synth
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    from harp_amd.optimize_sequence import init_params
    from harp_amd.utils.config_utils import get_config
    tpl = synth.load_template("arm")
    m = synth.make_smplx_arm_model(tpl, seed=seed)
    corr = np.load(os.path.join(os.path.dirname(os.path.abspath(synth.__file__)), "assets", "arm_corr.npz"))
    layer = SMPLXARM(m, m["faces"], corr["mano_vert_from_arm"], device=dev)
    focal = 1000.0 * S / 224.0
    g = torch.Generator().manual_seed(seed)
    c = m["v_template"].mean(0)
    seq = dict(pose=torch.randn(T, 45, generator=g) * 0.15, rot=torch.randn(T, 3, generator=g) * 0.2, trans=torch.randn(T, 3, generator=g) * 0.01,
               shape=torch.randn(T, 10, generator=g) * 0.3, joints=torch.zeros(T, 21, 3),
               cam=torch.tensor([[2 * focal / (S * 1.6), -float(c[0]), -float(c[1])]]).repeat(T, 1))
    cfg = get_config(write_yaml=False, use_arm=True, img_size=S, focal_length=focal, self_shadow=True, base_output_dir="unused/")
    params = init_params(seq, True, True, None, layer.right_arm_faces_tensor, False, torch.from_numpy(tpl["verts_uvs"])[None],
                         torch.from_numpy(tpl["faces_uvs"])[None], use_arm=True, configs=cfg, device=dev,
                         uv_mask=torch.from_numpy(tpl["uv_mask"]).double() / 255)
    with torch.no_grad():
        params["texture"].copy_(torch.rand(1, 512, 512, 3, generator=g) * 0.5 + 0.3)
        params["wrist_pose"].copy_(torch.randn(T, 3, generator=g) * 0.2)
    return cfg, layer, params, m


def main():
    from harp_amd import ops, playback, synth
    from harp_amd.manopth.manolayer import ManoLayer
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    res = {"iters": 15, "pose_prior_weight": 1e-5, "wrist_prior_weight": 1e-4, "repeats": a.repeats, "device": torch.cuda.get_device_name(),
           "frames_per_block": ops.arm_ik_frames_per_block()}

    # what the rows are for: the arm player
    B, Tp = 32, 256
    cfg, layer, params, model = arm_fit(Tp, a.size, dev)
    player = playback.AvatarPlayer(cfg, params, layer, batch_size=B, ss=1, device=dev)
    player.load_motion(playback.Motion.from_params(params))
    rows = [np.arange(i, i + B) for i in range(0, Tp, B)]

    def one_pass():
        for r in rows:
            player.render(r)

    p = event_ms(one_pass, 3, a.repeats)
    res["arm_player_ss1_graph"] = dict(size=a.size, batch=B, frames=Tp, pass_ms=p, frames_per_s=Tp / (p["median"] * 1e-3))
    dm = layer.device_model
    mano_idx = layer.right_mano_idx.to(dev).to(torch.int32)
    hand_model = synth.make_mano_model()
    hand = ManoLayer(flat_hand_mean=False, use_pca=False, model=hand_model, device=dev)

    for T in a.frames:
        rng = np.random.default_rng(T)
        u = rng.normal(size=(T, 3))
        rot = rng.uniform(0.0, 3.1, size=(T, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)
        wrist, pose = rng.normal(size=(T, 3)) * 0.3, rng.normal(size=(T, 45)) * 0.3
        trans = rng.uniform(-0.3, 0.3, size=(T, 3))
        shape = up(rng.normal(size=10) * 0.5)
        with torch.no_grad():
            verts, joints = layer(betas=shape.expand(T, 10).contiguous(), global_orient=up(rot), transl=up(trans), right_hand_pose=up(pose),
                                  right_wrist_pose=up(wrist))
        kp = (joints / 1000.0).contiguous()
        kp64 = kp.cpu().numpy().astype(np.float64)
        z = lambda *s: torch.zeros(*s, device=dev)
        for name, held in (("22_wrist_solved", False), ("21_wrist_held", True)):
            rows0 = np.zeros((T, 17, 3))
            w = torch.ones(T, 22, device=dev)
            if held:
                rows0[:, 1] = wrist
                w[:, 21] = 0.0
            j0 = ops.arm_ik(dm, shape, kp, up(rows0), z(T, 3), iters=0, joints=True).joints.cpu().numpy().astype(np.float64) / 1000.0
            n = 21 if held else 22
            r0, t0 = playback.arm_palm_start(kp64[:, :n], np.ones((T, n), bool), j0)
            rows0[:, 0] = r0
            x0, tr0 = up(rows0), up(t0)
            kw = dict(weights=w, wrist_prior=up(rows0[:, 1]), solve_wrist=not held, iters=15, pose_prior_weight=1e-5, wrist_prior_weight=1e-4,
                      joints=True)
            out = ops.arm_ik(dm, shape, kp, x0, tr0, **kw)
            solve = event_ms(lambda: ops.arm_ik(dm, shape, kp, x0, tr0, out=out, **kw), 3, a.repeats)
            err = (out.joints - joints).norm(dim=-1)[:, :n]
            solve.update(frames_per_s=T / (solve["median"] * 1e-3), joint_error_mm_mean=float(err.mean()), joint_error_mm_max=float(err.max()),
                         accepted_min=int(out.status.min()), accepted_max=int(out.status.max()), launches=1)
            res[f"arm_ik_{name}_T{T}"] = solve
            kw0 = dict(kw, iters=0)
            out0 = ops.arm_ik(dm, shape, kp, x0, tr0, **kw0)
            res[f"arm_ik_{name}_iters0_T{T}"] = event_ms(lambda: ops.arm_ik(dm, shape, kp, x0, tr0, out=out0, **kw0), 3, a.repeats)
        fit_params = {"shape": shape, "cam": torch.zeros(1, 3)}
        for name, tg, extra in (("22", kp, {}), ("21", kp[:, :21], dict(wrist_pose=wrist))):
            wall = []
            for _ in range(3):
                torch.cuda.synchronize()
                t_a = time.perf_counter()
                playback.Motion.from_arm_keypoints(tg, fit_params, layer, match_bone_lengths=False, **extra)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t_a) * 1e3)
            res[f"from_arm_keypoints_{name}_wall_T{T}"] = stats(wall)

        # the siblings on the same frame count
        tg778 = (verts[:, layer.right_mano_idx.to(dev)] / 1000.0).contiguous()
        rows0 = np.zeros((T, 17, 3))
        rows0[:, 1] = wrist
        zero = ops.arm_vertex_fit(dm, tg778, up(rows0), shape, z(T, 3), vert_idx=mano_idx, solve_shape=False, iters=0, verts=True).verts
        r0, t0 = playback.vertex_start(tg778.cpu().numpy().astype(np.float64), np.ones((T, 778)),
                                       zero[:, mano_idx.long()].cpu().numpy().astype(np.float64) / 1000.0, np.zeros(3))
        rows0[:, 0] = r0
        x0, tr0 = up(rows0), up(t0)
        kwv = dict(vert_idx=mano_idx, solve_shape=False, solve_wrist=False, iters=10)
        outv = ops.arm_vertex_fit(dm, tg778, x0, shape, tr0, **kwv)
        fit = event_ms(lambda: ops.arm_vertex_fit(dm, tg778, x0, shape, tr0, out=outv, **kwv), 3, a.repeats)
        fit.update(frames_per_s=T / (fit["median"] * 1e-3), iters=10)
        res[f"arm_vertex_fit_mano778_wrist_held_T{T}"] = fit

        pose48 = up(np.concatenate([rot, pose], 1))
        hshape = up(rng.normal(size=10) * 0.5)
        with torch.no_grad():
            _, hj = hand(pose48, hshape.expand(T, 10).contiguous(), up(trans))
        hkp = (hj / 1000.0).contiguous()
        r0, t0 = playback.palm_start(hkp.cpu().numpy().astype(np.float64), np.ones((T, 21), bool),
                                     playback.rest_chain_joints(hand_model, hshape.cpu().numpy()))
        hx0, htr0 = up(np.concatenate([r0, np.zeros((T, 45))], 1)), up(t0)
        hdm = hand.device_model
        outh = ops.mano_ik(hdm, hshape, hkp, hx0, htr0, iters=15, prior_weight=1e-5, joints=True)
        mik = event_ms(lambda: ops.mano_ik(hdm, hshape, hkp, hx0, htr0, iters=15, prior_weight=1e-5, joints=True, out=outh), 3, a.repeats)
        mik.update(frames_per_s=T / (mik["median"] * 1e-3))
        res[f"mano_ik_T{T}"] = mik
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
