"""What the motion filter costs (csrc/filter.hip): ops.motion_filter on 256 and 4 096 frames of the hand's table (16
rotations, 1 vector, 3 scalars: 54 columns) with a Gaussian window of sigma 2, R = 6, two geodesic iterations and the trimmed second pass
on, next to ops.motion_resample of the same table to as many rows (the neighbour kernel: at most two rows in, one out).  Both calls include
what the binding does around the launch (the taps' upload, the output allocation); the entry point alone, on buffers made beforehand, is
timed as `--burst` launches back to back between one pair of events, divided by their number.

Method (tools/dev/gpu_ik_time.py's): warm-up, then device events around one call, median [min .. max] over `--repeats` calls.

    python tools/dev/gpu_filter_time.py [--repeats 7] [--out profiles/filter_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gpu_ik_time import event_ms  # noqa: E402


def main():
    from harp_amd import _lib, ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--radius", type=int, default=6)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    n_rot, n_vec, n_lin, R = 16, 1, 3, a.radius
    nch = n_rot + n_vec + n_lin
    taps = ops.gaussian_taps(2.0, R)
    res = {"n_rot": n_rot, "n_vec": n_vec, "n_lin": n_lin, "radius": R, "sigma": 2.0, "iters": 2, "trim_rot": 0.5, "repeats": a.repeats, "burst": a.burst,
           "device": torch.cuda.get_device_name()}
    for T in a.frames:
        rng = np.random.default_rng(T)
        t = np.arange(T)[:, None]
        rows = np.concatenate([0.4 * np.sin(t / 20.0 + rng.uniform(0, 6.28, size=(1, 48))) + rng.normal(size=(T, 48)) * 0.02,
                               rng.normal(size=(T, 6)) * 0.01], 1)
        rows = torch.as_tensor(rows, dtype=torch.float32, device=dev)
        off = torch.as_tensor(rng.normal(size=48) * 0.2, dtype=torch.float32, device=dev)
        w = torch.as_tensor(rng.uniform(0.2, 1.0, size=T), dtype=torch.float32, device=dev)
        trim = torch.tensor([0.5] * n_rot + [0.05] * n_vec + [0.0] * n_lin, device=dev)
        times = torch.linspace(0.25, T - 1.25, T, device=dev)
        filt = event_ms(lambda: ops.motion_filter(rows, n_rot, n_vec, taps, weights=w, trim=trim, rot_offset=off, iters=2), 3, a.repeats)
        plain = event_ms(lambda: ops.motion_filter(rows, n_rot, n_vec, taps, rot_offset=off, iters=2), 3, a.repeats)
        resample = event_ms(lambda: ops.motion_resample(rows, times, n_rot, off), 3, a.repeats)
        out, used = ops.motion_filter(rows, n_rot, n_vec, taps, weights=w, trim=trim, rot_offset=off, iters=2)
        d_taps, p = torch.tensor(taps, device=dev), _lib.ptr

        def burst():
            for _ in range(a.burst):
                rc = _lib.lib().harp_motion_filter(p(rows), T, n_rot, n_vec, n_lin, p(off), p(d_taps), R, p(w), 1, None, p(trim), 2, p(out), p(used),
                                                   _lib.stream())
                assert rc == 0

        def burst_resample():
            for _ in range(a.burst):
                rc = _lib.lib().harp_motion_resample(p(rows), T, n_rot, 3 * n_vec + n_lin, p(off), p(times), T, p(out), _lib.stream())
                assert rc == 0

        per_launch = lambda r: {k: (v / a.burst if k != "n" else v) for k, v in r.items()}      # noqa: E731
        res[f"entry_point_per_launch_T{T}"] = per_launch(event_ms(burst, 3, a.repeats))
        res[f"resample_entry_point_per_launch_T{T}"] = per_launch(event_ms(burst_resample, 3, a.repeats))
        filt.update(frames_per_s=T / (filt["median"] * 1e-3), lanes=T * nch, used_min=int(used.min()), used_max=int(used.max()))
        res[f"motion_filter_T{T}"] = filt
        res[f"motion_filter_no_trim_no_weights_T{T}"] = plain
        res[f"motion_resample_T{T}"] = resample
        res[f"ratio_T{T}"] = filt["median"] / resample["median"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
