"""Time ops.lpips_alex (csrc/lpips.hip) against a float32 torch restatement of LPIPS v0.1 / AlexNet on the device (F.conv2d / max_pool2d,
the library path) on N (ref, pred) pairs of S x S x 3 on seeded weights, alternating the two in one run, warmed up, with device events.

    python tools/dev/gpu_lpips_time.py [--n 64] [--size 512] [--reps 10] [--out profiles/lpips_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -o lpips -- python tools/dev/gpu_lpips_time.py --reps 3 --profile

Executed-convolution TFLOP/s counts 2 x MACs of the five convolutions at their output sizes for 2N images (7.30 GFLOP per image at 512²)
over the measured call time."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from harp_amd import ops  # noqa: E402
from harp_amd.lpips import LPIPS  # noqa: E402

KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")


def torch_lpips(X, Y, sd):
    """LPIPS v0.1 / alex in float32 torch ops, (N,3,H,W) -> (N,)"""
    shift = torch.tensor([-0.030, -0.088, -0.188], device=X.device).view(1, 3, 1, 1)
    scale = torch.tensor([0.458, 0.448, 0.450], device=X.device).view(1, 3, 1, 1)
    w = [(sd[k + ".weight"], sd[k + ".bias"]) for k in KEYS]
    h = (torch.cat([X, Y]) - shift) / scale
    taps = [F.relu(F.conv2d(h, *w[0], stride=4, padding=2))]
    taps.append(F.relu(F.conv2d(F.max_pool2d(taps[-1], 3, 2), *w[1], padding=2)))
    taps.append(F.relu(F.conv2d(F.max_pool2d(taps[-1], 3, 2), *w[2], padding=1)))
    taps.append(F.relu(F.conv2d(taps[-1], *w[3], padding=1)))
    taps.append(F.relu(F.conv2d(taps[-1], *w[4], padding=1)))
    N, total = X.shape[0], 0
    for k, f in enumerate(taps):
        f = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + F.conv2d((f[:N] - f[N:]) ** 2, sd[f"lin{k}.model.1.weight"]).mean((1, 2, 3))
    return total


def conv_flops(H, W):
    h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return 2 * (h1 * w1 * 64 * 363 + h2 * w2 * 192 * 1600 + h3 * w3 * (384 * 1728 + 256 * 3456 + 256 * 2304))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--profile", action="store_true", help="only a few calls of ops.lpips_alex (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    N, S = a.n, a.size
    m = LPIPS(weights="random", seed=0).to("cuda")
    sd = {k: v.to("cuda") for k, v in m.state_dict().items()}
    net = m._packed(torch.device("cuda"))
    ref = torch.rand(N, S, S, 3, device="cuda")
    pred = (ref + 0.1 * torch.rand(N, S, S, 3, device="cuda")).clamp(0, 1)
    Xc, Yc = ref.permute(0, 3, 1, 2).contiguous(), pred.permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        if a.profile:
            for _ in range(a.reps):
                ops.lpips_alex(ref, pred, net)
            torch.cuda.synchronize()
            return
        run = {"hip": lambda: ops.lpips_alex(ref, pred, net), "torch_f32": lambda: torch_lpips(Xc, Yc, sd)}
        for f in run.values():                       # warm-up: code objects, MIOpen algorithm choice
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
        diff = (run["hip"]()[:, 0] - run["torch_f32"]()).abs().max().item()
    fl = conv_flops(S, S) * 2 * N
    res = {"n_pairs": N, "size": S, "reps": a.reps, "conv_flop": fl, "gflop_per_image": conv_flops(S, S) / 1e9,
           "max_abs_diff_lpips_vs_torch_f32": diff, "device": torch.cuda.get_device_name()}
    for k, v in times.items():
        v = sorted(v)
        res[k] = {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "conv_TFLOP_per_s_median": fl / (v[len(v) // 2] * 1e-3) / 1e12}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
