"""Time ops.image_metrics (csrc/metrics.hip) against a float32 torch restatement of pytorch_msssim 0.2.1's ms_ssim (grouped F.conv2d +
avg_pool2d, the package's algorithm) on N frames of S x S x 3, alternating the two in one run, warmed up, with device events.

    python tools/dev/gpu_metrics_time.py [--n 256] [--size 512] [--reps 10] [--out profiles/metrics_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -o metrics -- python tools/dev/gpu_metrics_time.py --reps 3 --profile

Achieved bytes/s counts one read of each image pair per level (level 0: both images; levels 1..4: both pooled images), over the
measured call time."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from harp_amd import ops  # noqa: E402

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def torch_ms_ssim(X, Y, data_range=1.0, K=(0.01, 0.03)):
    """pytorch_msssim 0.2.1 ms_ssim(size_average=False) in float32 torch ops (X, Y: (N,C,H,W) on the device)"""
    c = torch.arange(11, dtype=torch.float32, device=X.device) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).view(1, 1, 1, -1).repeat(X.shape[1], 1, 1, 1)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2

    def filt(t):
        return F.conv2d(F.conv2d(t, g, groups=t.shape[1]), g.transpose(2, 3), groups=t.shape[1])
    mcs = []
    for lvl in range(5):
        mu1, mu2 = filt(X), filt(Y)
        s1, s2, s12 = filt(X * X) - mu1 ** 2, filt(Y * Y) - mu2 ** 2, filt(X * Y) - mu1 * mu2
        cs = (2 * s12 + C2) / (s1 + s2 + C2)
        ssim = ((2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1)) * cs
        if lvl < 4:
            mcs.append(torch.relu(cs.flatten(2).mean(-1)))
            pad = (X.shape[2] % 2, X.shape[3] % 2)
            X, Y = F.avg_pool2d(X, 2, padding=pad), F.avg_pool2d(Y, 2, padding=pad)
    w = torch.tensor(WEIGHTS, device=X.device).view(-1, 1, 1)
    return torch.prod(torch.stack(mcs + [torch.relu(ssim.flatten(2).mean(-1))]) ** w, 0).mean(1)


def level_bytes(N, S):
    b, s = 0, S
    for _ in range(5):
        b += 2 * N * 3 * s * s * 4
        s = (s + 1) // 2
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--profile", action="store_true", help="only a few calls of ops.image_metrics (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    N, S = a.n, a.size
    ref = torch.rand(N, S, S, 3, device="cuda")
    pred = (ref + 0.1 * torch.rand(N, S, S, 3, device="cuda")).clamp(0, 1)
    mref, mpred = (torch.rand(N, S, S, device="cuda") > 0.5).float(), (torch.rand(N, S, S, device="cuda") > 0.5).float()
    Xc, Yc = ref.permute(0, 3, 1, 2).contiguous(), pred.permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        if a.profile:
            for _ in range(a.reps):
                ops.image_metrics(ref, pred, mref, mpred)
            torch.cuda.synchronize()
            return
        run = {"hip": lambda: ops.image_metrics(ref, pred, mref, mpred), "torch_f32": lambda: torch_ms_ssim(Xc, Yc)}
        for f in run.values():                       # warm-up: code objects, cuDNN/MIOpen algorithm choice
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in run}
        for _ in range(a.reps):
            for k, f in run.items():                 # alternating in one run
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        diff = (run["hip"]()["ms_ssim"] - run["torch_f32"]()).abs().max().item()
    b = level_bytes(N, S)
    res = {"n": N, "size": S, "reps": a.reps, "bytes_one_read_per_level": b, "max_abs_diff_ms_ssim_vs_torch_f32": diff}
    for k, v in times.items():
        v = sorted(v)
        res[k] = {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "GB_per_s_median": b / (v[len(v) // 2] * 1e-3) / 1e9}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
