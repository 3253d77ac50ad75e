"""What the batched reprojection inverse kinematics costs (csrc/reproj_ik.hip): ops.mano_reproj_ik with 20 iterations beside
ops.mano_ik with 15 in the same run, at 256 and 4096 problems of the synthetic hand (pose sigma 0.3, root rotations up to 3.1 rad, trans
within 0.05 m, cam (8.9, 0.01, -0.02), focal 2000, 448 px), the reprojection solve with depth rows from the first planar start, the 3-D
solve from the palm start.  The yardstick is mano_ik on this tree: per problem and iteration the two build the same J (63 x 51) and
A (51 x 51).

Method (tools/dev/gpu_ik_time.py's): warm-up, then device events around one call, median [min .. max] over `--repeats` calls.  Also the
wall-clock time of Motion.from_image_keypoints as a whole (N / 2 frames: two candidates each), host-side planar starts and uploads included.

    python tools/dev/gpu_reproj_ik_time.py [--repeats 7] [--out profiles/reproj_ik_time.json]"""
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

CAM, FOCAL, S = (8.9, 0.01, -0.02), 2000.0, 448
ITERS, IK_ITERS = 20, 15


def main():
    from harp_amd import ops, playback, synth
    from harp_amd.manopth.manolayer import ManoLayer
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--problems", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    model = synth.make_mano_model()
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=model, device=dev)
    dm = layer.device_model
    res = {"iters": ITERS, "mano_ik_iters": IK_ITERS, "repeats": a.repeats, "device": torch.cuda.get_device_name(), "cam": CAM, "focal": FOCAL, "S": S}
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)      # noqa: E731
    for N in a.problems:
        rng = np.random.default_rng(N)
        u = rng.normal(size=(N, 3))
        rot = rng.uniform(0.0, 3.1, size=(N, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)
        pose48 = up(np.concatenate([rot, rng.normal(size=(N, 45)) * 0.3], 1))
        trans = up(rng.uniform(-0.05, 0.05, size=(N, 3)))
        shape_np = rng.normal(size=10) * 0.5
        shape = up(shape_np)
        with torch.no_grad():
            _, joints = layer(pose48, shape.expand(N, 10).contiguous(), trans)
        kp3 = (joints / 1000.0).contiguous()
        rows = playback.project_pixels(kp3.cpu().double().numpy(), np.array(CAM), FOCAL, S)
        rest = playback.rest_chain_joints(model, shape_np)
        used = np.ones((N, 21), bool)
        rot0, tr0, zbar = playback.planar_palm_starts(rows[..., :2], used, rest, np.array(CAM), FOCAL, S)
        x0, t0 = up(np.concatenate([rot0[:, 0], np.zeros((N, 45))], 1)), up(tr0[:, 0])
        scale = (FOCAL / zbar) ** 2
        kw = dict(depth_weights=up(np.broadcast_to(scale[:, None], (N, 21))), z_prior=t0[:, 2].contiguous(), iters=ITERS,
                  pose_prior_weight=float(1e-5 * np.median(scale)), z_prior_weight=float(2.5e-5 * np.median(scale)), proj=True)
        targets, cam = up(rows), up(CAM)
        out = ops.mano_reproj_ik(dm, shape, targets, x0, t0, cam, FOCAL, S, **kw)
        solve = event_ms(lambda: ops.mano_reproj_ik(dm, shape, targets, x0, t0, cam, FOCAL, S, out=out, **kw), 3, a.repeats)
        err = (out.proj[..., :2] - targets[..., :2]).norm(dim=-1).amax(1)
        solve.update(problems_per_s=N / (solve["median"] * 1e-3), us_per_problem_iteration=solve["median"] * 1e3 / (N * ITERS),
                     pixel_error_median=float(err.median()), pixel_error_max=float(err.max()), accepted_min=int(out.status.min()),
                     accepted_max=int(out.status.max()))
        res[f"mano_reproj_ik_N{N}"] = solve

        r3, t3 = playback.palm_start(kp3.cpu().double().numpy(), used, rest)
        x3, tr3 = up(np.concatenate([r3, np.zeros((N, 45))], 1)), up(t3)
        out3 = ops.mano_ik(dm, shape, kp3, x3, tr3, iters=IK_ITERS, prior_weight=1e-5, joints=True)
        ik = event_ms(lambda: ops.mano_ik(dm, shape, kp3, x3, tr3, iters=IK_ITERS, prior_weight=1e-5, joints=True, out=out3), 3, a.repeats)
        ik.update(problems_per_s=N / (ik["median"] * 1e-3), us_per_problem_iteration=ik["median"] * 1e3 / (N * IK_ITERS))
        res[f"mano_ik_N{N}"] = ik
        res[f"per_iteration_ratio_N{N}"] = solve["us_per_problem_iteration"] / ik["us_per_problem_iteration"]

        n_frames = N // 2                                  # the layer solves two candidates a frame
        params = {"shape": shape, "cam": up(CAM)[None]}
        cfg = {"focal_length": FOCAL, "img_size": S}
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t_a = time.perf_counter()
            playback.Motion.from_image_keypoints(rows[:n_frames, :, :2], params, layer, depth=rows[:n_frames, :, 2], configs=cfg)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t_a) * 1e3)
        res[f"from_image_keypoints_wall_frames{n_frames}"] = stats(wall)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
