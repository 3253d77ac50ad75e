"""What preparing a fit's targets from JPEG files costs: 256 synthetic 512 x 512 frames and masks (quality 95), written
once; then `ResidentTargets(...)` + `FitEngine.set_targets`, synchronised, with ingest="host" (the path before csrc/ingest.hip) and with
ingest="device", alternating, each in a fresh process.  For the device path also every chunk's copies and kernel (device events) and the
host's time in the decoder and waiting for a staging buffer.

    python tools/dev/gpu_ingest_time.py [--pairs 3] [--out profiles/ingest_time.json]

The parent never opens the GPU; every child runs under its own time limit, one at a time, and the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
T, S, B = 256, 512, 32


def write_frames(folder):
    """smooth colours over a noisy background and a blob mask, like a segmented hand crop: (image_paths, mask_paths)"""
    import numpy as np
    from PIL import Image
    g = np.random.default_rng(0)
    yy, xx = np.mgrid[:S, :S].astype(np.float32)
    ips, mps = [], []
    for t in range(T):
        cy, cx = S / 2 + 40 * np.sin(t / 9.0), S / 2 + 40 * np.cos(t / 7.0)
        blob = ((yy - cy) / 150) ** 2 + ((xx - cx) / 110) ** 2 < 1
        rgb = np.stack([128 + 100 * np.sin(xx / 37 + t / 5.0), 128 + 100 * np.cos(yy / 29), 128 + 90 * np.sin((xx + yy) / 53)], -1)
        rgb = np.clip(rgb * blob[..., None] + g.normal(0, 6, (S, S, 3)), 0, 255).astype(np.uint8)
        ips.append(os.path.join(folder, "%04d.jpg" % t))
        mps.append(os.path.join(folder, "%04d_mask.jpg" % t))
        Image.fromarray(rgb, "RGB").save(ips[-1], quality=95)
        Image.fromarray((blob * 255).astype(np.uint8), "L").save(mps[-1], quality=95)
    return ips, mps


def child(mode, folder):
    import torch
    from harp_amd import synth
    from harp_amd.engine import FitEngine
    from harp_amd.utils.data_util import ImagesDataset, ResidentTargets, default_workers
    dev = "cuda"
    tpl = synth.load_template("hand")
    model_np = synth.make_mano_model(tpl, seed=0)
    seq, focal = synth.make_sequence(model_np, T, S, seed=0)
    seq["joints"] = torch.zeros(T, 21, 3)
    eng = FitEngine(model_np, synth.build_topology(tpl["faces0"], 778), tpl["verts_uvs"], tpl["faces_uvs"],
                    (torch.from_numpy(tpl["uv_mask"]).double() / 255).float(), seq, S, focal, B, device=dev)
    ds = ImagesDataset([os.path.join(folder, "%04d.jpg" % t) for t in range(T)], [os.path.join(folder, "%04d_mask.jpg" % t) for t in range(T)], 1)
    warm = torch.empty(1 << 20, dtype=torch.uint8).pin_memory().to(dev, non_blocking=True)       # the pinned allocator's and the copy engine's first use
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rt = ResidentTargets(ds, device=eng.dev, ingest="device") if mode == "device" else ResidentTargets(ds)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    eng.set_targets(*rt.tensors())
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = {"ingest": mode, "resident_targets_s": t1 - t0, "set_targets_s": t2 - t1, "total_s": t2 - t0, "workers": default_workers(),
           "device": torch.cuda.get_device_name(), "checksum": float(eng.y_true.double().sum() + eng.y_sil.double().sum() + eng.y_sil_col.double().sum())}
    if mode == "device":
        st = rt.ingest_stats()
        res.update(chunks=st["chunks"], host_decode_s=st["decode_s"], host_wait_s=st["wait_s"], copy_ms=st["copy_ms"], kernel_ms=st["kernel_ms"],
                   copy_ms_total=sum(st["copy_ms"]), kernel_ms_total=sum(st["kernel_ms"]))
    del warm
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_time.json"))
    ap.add_argument("--child", choices=["host", "device"], default=None)
    ap.add_argument("--frames", default=None, help="(child) the folder the parent wrote")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames)
    runs = []
    with tempfile.TemporaryDirectory() as folder:
        t0 = time.perf_counter()
        write_frames(folder)
        print("wrote %d frames and masks in %.1f s" % (T, time.perf_counter() - t0), flush=True)
        for i in range(2 * a.pairs):
            mode = "device" if i % 2 else "host"
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--frames", folder],
                               capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"child {i} (ingest {mode}) ended with status {p.returncode}: nothing more is started")
            runs.append(json.loads(line[-1][7:]))
            print(json.dumps({k: v for k, v in runs[-1].items() if not isinstance(v, list)}), flush=True)
    host, devr = [r for r in runs if r["ingest"] == "host"], [r for r in runs if r["ingest"] == "device"]
    if len({r["checksum"] for r in runs}) != 1:
        raise SystemExit("the two paths left different targets in the engine: " + str([r["checksum"] for r in runs]))
    vals = lambda rs, k: [r[k] for r in rs]
    out = {"scene": {"frames": T, "size": S, "jpeg_quality": 95, "chunk": 32, "workers": runs[0]["workers"]}, "device": runs[0]["device"], "runs": runs}
    for name, rs in (("host", host), ("device", devr)):
        for k in ("resident_targets_s", "set_targets_s", "total_s"):
            out[f"{name}_{k}"] = {"median": statistics.median(vals(rs, k)), "all": vals(rs, k)}
    for k in ("host_decode_s", "host_wait_s", "copy_ms_total", "kernel_ms_total"):
        out["device_" + k] = {"median": statistics.median(vals(devr, k)), "all": vals(devr, k)}
    out["speedup_total"] = out["host_total_s"]["median"] / out["device_total_s"]["median"]
    out["fit_for_scale"] = {"source": "profiles/monitor_time.json (DESIGN.md §17), targets handed over as device tensors", "call_s": 3.05,
                            "epochs_1_to_300_s": 1.15}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))


if __name__ == "__main__":
    main()
