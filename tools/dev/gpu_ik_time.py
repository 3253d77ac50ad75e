"""What the batched inverse kinematics costs (csrc/ik.hip): ops.mano_ik with 15 iterations at T = 256 and T = 4096 frames of the
synthetic hand (pose sigma 0.3, root rotations up to 3.1 rad, trans within 0.3 m) from the palm start, next to what the tree offered for
the same job before: optimize_for_mano_param on the same frames' 778 vertices at its 500 + 700 Adam iterations of seven launches each.

Method (tools/dev/gpu_playback_time.py's): warm-up, then device events around one call, median [min .. max] over `--repeats` calls (the
baseline over `--baseline-repeats`: one call is 8 400 launches).  Also the wall-clock time of Motion.from_keypoints as a whole, host-side
palm start and uploads included.

    python tools/dev/gpu_ik_time.py [--repeats 7] [--baseline-repeats 3] [--out profiles/ik_time.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gpu_playback_time import stats  # noqa: E402

PLAYER_FPS = 81e3                                          # AvatarPlayer at 512 x 512, ss = 1


def event_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out)


def main():
    from harp_amd import ops, playback, synth
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.metro_modifications.hand_utils import optimize_for_mano_param
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--baseline-repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    model = synth.make_mano_model()
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=model, device=dev)
    res = {"iters": 15, "prior_weight": 1e-5, "repeats": a.repeats, "baseline_repeats": a.baseline_repeats, "device": torch.cuda.get_device_name(),
           "player_frames_per_s": PLAYER_FPS}
    for T in a.frames:
        rng = np.random.default_rng(T)
        u = rng.normal(size=(T, 3))
        rot = rng.uniform(0.0, 3.1, size=(T, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)
        pose48 = torch.as_tensor(np.concatenate([rot, rng.normal(size=(T, 45)) * 0.3], 1), dtype=torch.float32, device=dev)
        trans = torch.as_tensor(rng.uniform(-0.3, 0.3, size=(T, 3)), dtype=torch.float32, device=dev)
        shape = torch.as_tensor(rng.normal(size=10) * 0.5, dtype=torch.float32, device=dev)
        with torch.no_grad():
            verts, joints = layer(pose48, shape.expand(T, 10).contiguous(), trans)
        kp = (joints / 1000.0).contiguous()
        rest = playback.rest_chain_joints(model, shape.cpu().numpy())
        r0, t0 = playback.palm_start(kp.cpu().numpy().astype(np.float64), np.ones((T, 21), bool), rest)
        x0 = torch.as_tensor(np.concatenate([r0, np.zeros((T, 45))], 1), dtype=torch.float32, device=dev)
        tr0 = torch.as_tensor(t0, dtype=torch.float32, device=dev)
        dm = layer.device_model
        out = ops.mano_ik(dm, shape, kp, x0, tr0, iters=15, prior_weight=1e-5, joints=True)
        solve = event_ms(lambda: ops.mano_ik(dm, shape, kp, x0, tr0, iters=15, prior_weight=1e-5, joints=True, out=out), 3, a.repeats)
        err = (out.joints - joints).norm(dim=-1)
        solve.update(frames_per_s=T / (solve["median"] * 1e-3), joint_error_mm_mean=float(err.mean()), joint_error_mm_max=float(err.max()),
                     accepted_min=int(out.status.min()), accepted_max=int(out.status.max()))
        res[f"mano_ik_T{T}"] = solve
        params = {"shape": shape, "cam": torch.zeros(1, 3)}
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t_a = time.perf_counter()
            playback.Motion.from_keypoints(kp, params, layer, match_bone_lengths=False)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t_a) * 1e3)
        res[f"from_keypoints_wall_T{T}"] = stats(wall)

        def baseline():
            with contextlib.redirect_stdout(io.StringIO()):
                return optimize_for_mano_param(verts / 1000.0, layer)

        fit = baseline()                                   # (also the warm-up)
        base = event_ms(baseline, 0, a.baseline_repeats)
        berr = np.linalg.norm(fit["joints"] - joints.cpu().numpy(), axis=-1)
        base.update(frames_per_s=T / (base["median"] * 1e-3), joint_error_mm_mean=float(berr.mean()), joint_error_mm_max=float(berr.max()),
                    launches=(500 + 700) * 7)
        res[f"vertex_fit_T{T}"] = base
        res[f"speedup_T{T}"] = base["median"] / solve["median"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
