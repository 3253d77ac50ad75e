"""What the batched SMPL-X arm vertex fit costs (csrc/arm_vertex_fit.hip): ops.arm_vertex_fit with 10 iterations and the
shape solved at T = 256 and T = 4096 frames of the synthetic arm (pose sigma 0.3, root rotations up to 3.1 rad, trans within 0.3 m,
per-frame betas sigma 0.5) from the rigid start, for both target sets — all 1026 arm vertices with the wrist solved (true wrist sigma 0.3),
and the 778 hand vertices through right_mano_idx with the wrist held at zero (true wrist zero: the reference's parameter set) — next to the
tree's other route from hand vertices to arm rows: optimize_for_mano_arm_param(method="adam") on the frames of the second set at its
500 + 700 Adam iterations through torch.autograd and torch.optim.Adam — all in one process.

Method (tools/dev/gpu_vertex_fit_time.py's): warm-up, then device events around one call, median [min .. max] over `--repeats` calls (the
baseline over `--baseline-repeats`: one call is 1 200 iterations of a dozen launches and a host-side optimiser step).  Also the final mean /
largest vertex error of both methods, and the wall-clock time of optimize_for_mano_arm_param(method="lm") as a whole, host-side rigid start
and copies included.

    python tools/dev/gpu_arm_vertex_fit_time.py [--repeats 7] [--baseline-repeats 3] [--out profiles/arm_vertex_fit_time.json]"""
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
from gpu_ik_time import event_ms  # noqa: E402
from gpu_playback_time import stats  # noqa: E402

ITERS = 10


def main():
    import harp_amd
    from harp_amd import ops, playback, synth
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    from harp_amd.metro_modifications.hand_utils import optimize_for_mano_arm_param
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--baseline-repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    model = synth.make_smplx_arm_model(seed=0)
    corr = np.load(os.path.join(os.path.dirname(os.path.abspath(harp_amd.__file__)), "assets", "arm_corr.npz"))
    layer = SMPLXARM(model, model["faces"], corr["mano_vert_from_arm"], device=dev)
    dm, mano = layer.device_model, layer.right_mano_idx.to(dev)
    vi = mano.to(torch.int32).contiguous()
    res = {"iters": ITERS, "repeats": a.repeats, "baseline_repeats": a.baseline_repeats, "device": torch.cuda.get_device_name(),
           "frames_per_block": ops.arm_vertex_fit_frames_per_block()}
    f32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    with torch.no_grad():
        rest = layer(betas=z(1, 10), global_orient=z(1, 3), transl=z(1, 3), right_hand_pose=z(1, 45))[0][0].cpu().numpy().astype(np.float64) / 1000.0
    for T in a.frames:
        rng = np.random.default_rng(T)
        u = rng.normal(size=(T, 3))
        rot = f32(rng.uniform(0.0, 3.1, size=(T, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True))
        wrist, pose = f32(rng.normal(size=(T, 3)) * 0.3), f32(rng.normal(size=(T, 45)) * 0.3)
        trans, betas = f32(rng.uniform(-0.3, 0.3, size=(T, 3))), f32(rng.normal(size=(T, 10)) * 0.5)
        for name, idx, true_wrist in (("all1026_wrist_solved", None, wrist), ("mano778_wrist_held", vi, z(T, 3))):
            with torch.no_grad():
                verts = layer(betas=betas, global_orient=rot, transl=trans, right_hand_pose=pose, right_wrist_pose=true_wrist)[0]
            sel = (lambda v: v) if idx is None else (lambda v: v[:, mano])
            targets = (sel(verts) / 1000.0).contiguous()
            n = targets.shape[1]
            r0, t0 = playback.vertex_start(targets.cpu().numpy().astype(np.float64), np.ones((T, n), bool),
                                           rest if idx is None else rest[mano.cpu().numpy()], np.zeros(3))
            x0 = z(T, 17, 3)
            x0[:, 0] = f32(r0)
            b0, tr0 = z(T, 10), f32(t0)
            kw = dict(vert_idx=idx, solve_wrist=idx is None, iters=ITERS, verts=True)
            out = ops.arm_vertex_fit(dm, targets, x0, b0, tr0, **kw)
            solve = event_ms(lambda: ops.arm_vertex_fit(dm, targets, x0, b0, tr0, out=out, **kw), 3, a.repeats)
            err = (sel(out.verts) - sel(verts)).norm(dim=-1)
            solve.update(frames_per_s=T / (solve["median"] * 1e-3), vertex_error_mm_mean=float(err.mean()), vertex_error_mm_max=float(err.max()),
                         accepted_min=int(out.status.min()), accepted_max=int(out.status.max()), launches=1)
            res[f"arm_vertex_fit_{name}_T{T}"] = solve
            one = ops.arm_vertex_fit(dm, targets, x0, b0, tr0, vert_idx=idx, solve_wrist=idx is None, iters=0)
            ev0 = event_ms(lambda: ops.arm_vertex_fit(dm, targets, x0, b0, tr0, vert_idx=idx, solve_wrist=idx is None, iters=0, out=one), 3, a.repeats)
            res[f"arm_vertex_fit_{name}_iters0_T{T}"] = ev0  # the prologue, one evaluation with the tangents and the normal equations

        def fit(method):
            with contextlib.redirect_stdout(io.StringIO()):
                return optimize_for_mano_arm_param(targets, layer, method=method)

        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t_a = time.perf_counter()
            fit("lm")
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t_a) * 1e3)
        res[f"optimize_lm_wall_T{T}"] = stats(wall)
        got = fit("adam")                                  # (also the warm-up)
        base = event_ms(lambda: fit("adam"), 0, a.baseline_repeats)
        berr = np.linalg.norm(got["verts"] - sel(verts).cpu().numpy(), axis=-1)
        base.update(frames_per_s=T / (base["median"] * 1e-3), vertex_error_mm_mean=float(berr.mean()), vertex_error_mm_max=float(berr.max()),
                    iterations=500 + 700)
        res[f"optimize_adam_T{T}"] = base
        res[f"speedup_mano778_T{T}"] = base["median"] / res[f"arm_vertex_fit_mano778_wrist_held_T{T}"]["median"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
