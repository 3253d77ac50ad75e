"""What the batched vertex fit costs (csrc/vertex_fit.hip): ops.mano_vertex_fit with 10 iterations and the shape solved at
T = 256 and T = 4096 frames of the synthetic hand (pose sigma 0.3, root rotations up to 3.1 rad, trans within 0.3 m, per-frame betas sigma
0.5) from the rigid start, next to the tree's other route from vertices to MANO rows: optimize_for_mano_param(method="adam") on the same
frames at its 500 + 700 Adam iterations of seven launches each — both in one process.

Method (tools/dev/gpu_ik_time.py's): warm-up, then device events around one call, median [min .. max] over `--repeats` calls (the baseline
over `--baseline-repeats`: one call is 8 400 launches).  Also the final mean / largest vertex error of both methods, and the wall-clock
time of optimize_for_mano_param(method="lm") as a whole, host-side rigid start and copies included.

    python tools/dev/gpu_vertex_fit_time.py [--repeats 7] [--baseline-repeats 3] [--out profiles/vertex_fit_time.json]"""
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
    dm = layer.device_model
    res = {"iters": ITERS, "repeats": a.repeats, "baseline_repeats": a.baseline_repeats, "device": torch.cuda.get_device_name(),
           "frames_per_block": ops.mano_vertex_fit_frames_per_block()}
    f32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)
    with torch.no_grad():
        rest_v, rest_j = layer(torch.zeros(1, 48, device=dev), torch.zeros(1, 10, device=dev), torch.zeros(1, 3, device=dev))
    rest_v, rest_j = rest_v[0].cpu().numpy().astype(np.float64) / 1000.0, rest_j[0, 0].cpu().numpy().astype(np.float64) / 1000.0
    for T in a.frames:
        rng = np.random.default_rng(T)
        u = rng.normal(size=(T, 3))
        rot = rng.uniform(0.0, 3.1, size=(T, 1)) * u / np.linalg.norm(u, axis=1, keepdims=True)
        pose48, trans = f32(np.concatenate([rot, rng.normal(size=(T, 45)) * 0.3], 1)), f32(rng.uniform(-0.3, 0.3, size=(T, 3)))
        betas = f32(rng.normal(size=(T, 10)) * 0.5)
        with torch.no_grad():
            verts, _ = layer(pose48, betas, trans)
        targets = (verts / 1000.0).contiguous()
        r0, t0 = playback.vertex_start(targets.cpu().numpy().astype(np.float64), np.ones((T, 778), bool), rest_v, rest_j)
        x0, b0, tr0 = f32(np.concatenate([r0, np.zeros((T, 45))], 1)), torch.zeros(T, 10, device=dev), f32(t0)
        out = ops.mano_vertex_fit(dm, targets, x0, b0, tr0, iters=ITERS, verts=True)
        solve = event_ms(lambda: ops.mano_vertex_fit(dm, targets, x0, b0, tr0, iters=ITERS, verts=True, out=out), 3, a.repeats)
        err = (out.verts - verts).norm(dim=-1)
        solve.update(frames_per_s=T / (solve["median"] * 1e-3), vertex_error_mm_mean=float(err.mean()), vertex_error_mm_max=float(err.max()),
                     accepted_min=int(out.status.min()), accepted_max=int(out.status.max()), launches=1)
        res[f"mano_vertex_fit_T{T}"] = solve

        def fit(method):
            with contextlib.redirect_stdout(io.StringIO()):
                return optimize_for_mano_param(targets, layer, method=method)

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
        berr = np.linalg.norm(got["verts"] - verts.cpu().numpy(), axis=-1)
        base.update(frames_per_s=T / (base["median"] * 1e-3), vertex_error_mm_mean=float(berr.mean()), vertex_error_mm_max=float(berr.max()),
                    launches=(500 + 700) * 7)
        res[f"optimize_adam_T{T}"] = base
        res[f"speedup_T{T}"] = base["median"] / solve["median"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
