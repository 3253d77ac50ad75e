"""Time the Taubin smoothing of the mesh export (ops.taubin_smooth, csrc/smooth.hip) at the sizes the evaluation runs it — the subdivided
hand (3093 vertices) at B = 32, the arm (4083) at B = 8, num_iter = 10 — in both modes, next to the same 20 passes written with torch ops on
the device (index_add over the unique edge list).  Device events around each call, or, for per-kernel durations and launch counts:

    python tools/taubin_time.py --mesh hand [--reps 20] [--out profiles/taubin_time_hand.json]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/taubin_time.py --mesh hand --reps 5
    python tools/rocpd_stats.py DIR/.../run_results.db

One mesh per run: the kernels carry the same names for both."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_passes(v, edges, lambd, mu, num_iter):
    a, b = edges[:, 0], edges[:, 1]
    for _ in range(num_iter):
        for f in (lambd, mu):
            w = 1.0 / ((v[:, a] - v[:, b]).norm(dim=-1) + 1e-12)
            num = torch.zeros_like(v).index_add_(1, a, w[..., None] * v[:, b]).index_add_(1, b, w[..., None] * v[:, a])
            den = torch.zeros(v.shape[:2], device=v.device).index_add_(1, a, w).index_add_(1, b, w)
            v = (1.0 - f) * v + f * num / den[..., None]
    return v


def main():
    from harp_amd import ops, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", choices=("hand", "arm"), default="hand")
    ap.add_argument("--batch", type=int, default=None, help="frames per call (default: hand 32, arm 8)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B = args.batch or (32 if args.mesh == "hand" else 8)
    tpl = synth.load_template(args.mesh)
    n0 = tpl["base_verts"].shape[0]
    t = synth.build_topology(tpl["faces0"], n0)
    topo = ops.DeviceTopology(t, tpl["verts_uvs"], tpl["faces_uvs"], "cuda")
    rng = np.random.default_rng(0)
    v0 = tpl["base_verts"].astype(np.float64)[None] + rng.standard_normal((B, n0, 3)) * 3e-4
    v = np.concatenate([v0, 0.5 * (v0[:, t["edges0"][:, 0]] + v0[:, t["edges0"][:, 1]])], 1) + np.array([0.02, -0.01, 0.45])
    verts = torch.from_numpy(v.astype(np.float32)).cuda()
    edges = topo.edges.long()
    runs = {"hip_lds": lambda: ops.taubin_smooth(verts, topo, mode=1), "hip_global": lambda: ops.taubin_smooth(verts, topo, mode=2),
            "torch_ops": lambda: torch_passes(verts, edges, 0.53, -0.53, 10)}
    outs, res = {}, {"mesh": args.mesh, "B": B, "V": topo.V, "num_iter": 10, "reps": args.reps, "warmup": args.warmup}
    for name, fn in runs.items():
        for _ in range(args.warmup):
            outs[name] = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res[name + "_ms"] = {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}
    res["max_abs_lds_vs_global"] = float((outs["hip_lds"] - outs["hip_global"]).abs().max())
    res["max_abs_lds_vs_torch"] = float((outs["hip_lds"] - outs["torch_ops"]).abs().max())
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
