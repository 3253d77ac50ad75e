"""What the batched reprojection inverse kinematics of the SMPL-X arm costs (csrc/arm_reproj_ik.hip): ops.arm_reproj_ik with
20 iterations at N = 256 and N = 4096 problems of the synthetic arm (wrist and pose sigma 0.3, root rotations up to 3.1 rad, trans within
0.05 m, the camera of the tests) from the first planar start, 22 image keypoints with depth rows and the wrist solved and 21 with it held,
beside ops.arm_ik (15 iterations from the layer's 3-D start) on the same problem counts in the same run.  The one expectation to confirm
or refute (§30 found 1.0 x for the hand): per problem and iteration within about 1.1 x of ops.arm_ik.

Method (tools/dev/gpu_arm_ik_time.py's): warm-up, then device events around one call, median [min .. max] over `--repeats` calls, one
process.  Also the wall-clock time of Motion.from_arm_image_keypoints as a whole (2 T problems; host-side starts and uploads included) at
`--layer-frames` frames.

    python tools/dev/gpu_arm_reproj_ik_time.py [--repeats 7] [--out profiles/arm_reproj_ik_time.json]"""
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
ITERS, ITERS_3D = 20, 15


def main():
    import harp_amd
    from harp_amd import ops, playback, synth
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--problems", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--layer-frames", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    model = synth.make_smplx_arm_model(seed=0)
    corr = np.load(os.path.join(os.path.dirname(os.path.abspath(harp_amd.__file__)), "assets", "arm_corr.npz"))
    layer = SMPLXARM(model, model["faces"], corr["mano_vert_from_arm"], device=dev)
    dm = layer.device_model
    res = {"iters": ITERS, "arm_ik_iters": ITERS_3D, "repeats": a.repeats, "device": torch.cuda.get_device_name(),
           "frames_per_block": ops.arm_reproj_ik_frames_per_block()}
    z = lambda *s: torch.zeros(*s, device=dev)

    def scene(N):
        rng = np.random.default_rng(N)
        u = rng.normal(size=(N, 3))
        rows = np.zeros((N, 17, 3))
        rows[:, 0] = rng.uniform(0.0, 3.1, size=(N, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)
        rows[:, 1:] = rng.normal(size=(N, 16, 3)) * 0.3
        trans = rng.uniform(-0.05, 0.05, size=(N, 3))
        shape = up(rng.normal(size=10) * 0.5)
        kp = ops.arm_ik(dm, shape, z(N, 22, 3), up(rows), up(trans), iters=0, joints=True).joints / 1000.0
        px = playback.project_pixels(kp.cpu().double().numpy(), np.array(CAM), FOCAL, S)
        return rows, shape, kp.contiguous(), px

    for N in a.problems:
        rows, shape, kp, px = scene(N)
        params = {"shape": shape, "cam": up(np.array(CAM))[None]}
        for name, held in (("22_wrist_solved", False), ("21_wrist_held", True)):
            n = 21 if held else 22
            inp = playback.arm_image_ik_inputs(px[:, :n, :2], None, px[:, :n, 2], None, None, rows[:, 1] if held else None, params)
            j0 = ops.arm_ik(dm, shape, z(N, 22, 3), up(inp["in_pose"]), z(N, 3), iters=0, joints=True).joints.cpu().numpy().astype(np.float64) / 1000.0
            in_pose, trans, zbar = playback.arm_image_starts(inp, j0, None, FOCAL, S)
            scale = (FOCAL / zbar) ** 2
            med = float(np.median(scale))
            x0, t0 = up(in_pose[:, 0]), up(trans[:, 0])
            args = (dm, shape, up(inp["targets"]), x0, t0, up(np.array(CAM)), FOCAL, S)
            kw = dict(weights=up(inp["weights"]), depth_weights=up(np.broadcast_to(scale[:, None], (N, 22))), wrist_prior=up(inp["wrist"]),
                      z_prior=t0[:, 2].contiguous(), solve_wrist=not held, iters=ITERS, pose_prior_weight=1e-5 * med,
                      wrist_prior_weight=1e-4 * med, z_prior_weight=2.5e-5 * med, proj=True)
            out = ops.arm_reproj_ik(*args, **kw)
            solve = event_ms(lambda: ops.arm_reproj_ik(*args, out=out, **kw), 3, a.repeats)
            err = np.linalg.norm(out.proj.cpu().numpy()[:, :n, :2] - px[:, :n, :2], axis=-1).max(1)
            solve.update(problems_per_s=N / (solve["median"] * 1e-3), us_per_problem_iteration=solve["median"] * 1e3 / (N * ITERS),
                         pixel_error_median=float(np.median(err)), pixel_error_max=float(err.max()), accepted_min=int(out.status.min()),
                         accepted_max=int(out.status.max()), launches=1)
            res[f"arm_reproj_ik_{name}_N{N}"] = solve
            kw0 = dict(kw, iters=0)
            out0 = ops.arm_reproj_ik(*args, **kw0)
            res[f"arm_reproj_ik_{name}_iters0_N{N}"] = event_ms(lambda: ops.arm_reproj_ik(*args, out=out0, **kw0), 3, a.repeats)

            # the 3-D sibling on the same poses, in the same run
            kp64 = kp.cpu().numpy().astype(np.float64)
            rows0 = inp["in_pose"].copy()
            r0, tr0 = playback.arm_palm_start(kp64[:, :n], np.ones((N, n), bool), j0)
            rows0[:, 0] = r0
            w3 = torch.ones(N, 22, device=dev)
            if held:
                w3[:, 21] = 0.0
            a3 = (dm, shape, kp, up(rows0), up(tr0))
            kw3 = dict(weights=w3, wrist_prior=up(inp["wrist"]), solve_wrist=not held, iters=ITERS_3D, pose_prior_weight=1e-5,
                       wrist_prior_weight=1e-4, joints=True)
            out3 = ops.arm_ik(*a3, **kw3)
            ik = event_ms(lambda: ops.arm_ik(*a3, out=out3, **kw3), 3, a.repeats)
            ik.update(problems_per_s=N / (ik["median"] * 1e-3), us_per_problem_iteration=ik["median"] * 1e3 / (N * ITERS_3D))
            res[f"arm_ik_{name}_N{N}"] = ik
            res[f"per_problem_iteration_over_arm_ik_{name}_N{N}"] = solve["us_per_problem_iteration"] / ik["us_per_problem_iteration"]

    for T in a.layer_frames:
        rows, shape, kp, px = scene(T)
        params = {"shape": shape, "cam": up(np.array(CAM))[None]}
        cfg = dict(focal_length=FOCAL, img_size=S)
        for name, n, extra in (("22", 22, {}), ("21", 21, dict(wrist_pose=rows[:, 1]))):
            wall = []
            for _ in range(3):
                torch.cuda.synchronize()
                t_a = time.perf_counter()
                playback.Motion.from_arm_image_keypoints(px[:, :n, :2], params, layer, depth=px[:, :n, 2], configs=cfg, **extra)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t_a) * 1e3)
            res[f"from_arm_image_keypoints_{name}_wall_T{T}"] = stats(wall)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
