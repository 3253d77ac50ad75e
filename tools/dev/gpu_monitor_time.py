"""What in-fit monitoring costs: the fit of the bench scene — 256 frames, 512 x 512, 32 frames per step, 301 epochs, no
perceptual term — through optimize_hand_sequence with monitor=False and monitor=True, alternating, each in a fresh process; and per
monitor event the mirror render, harp_sheet_u8 and the device-to-host copy (device events), the encoder's time on the writer thread and
the back-pressure waits of the enqueueing thread.

    python tools/dev/gpu_monitor_time.py [--pairs 2] [--out profiles/monitor_time.json]

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
T, S, B, EPOCHS = 256, 512, 32, 301


def child(monitor_on):
    import torch
    from harp_amd import synth
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.monitor import FitMonitor
    from harp_amd.optimize_sequence import optimize_hand_sequence
    from harp_amd.utils.config_utils import get_config
    from tests._scene import make_fit_case
    dev = "cuda"
    case = make_fit_case("hand", T=T, S=S, B=B, seed=0, device=dev)          # targets rendered by the engine, as bench.py's
    tg, tpl = case["targets"], case["tpl"]
    model_np = synth.make_mano_model(tpl, seed=0)
    seq, focal = synth.make_sequence(model_np, T, S, seed=0)
    seq["joints"] = case["init_joints"]
    del case
    torch.cuda.empty_cache()
    ds = [(i, tg["y_true"][i], tg["y_sil"][i][..., None], tg["y_sil_col"][i][..., None]) for i in range(T)]
    g = torch.Generator().manual_seed(1)
    val = {"cam": seq["cam"].float() + 0.01 * torch.randn(T, 3, generator=g), "trans": seq["trans"].float() + 0.003 * torch.randn(T, 3, generator=g),
           "rot": seq["rot"].float() + 0.05 * torch.randn(T, 3, generator=g)}
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=model_np, device=dev)
    uvs, fuvs = torch.from_numpy(tpl["verts_uvs"])[None], torch.from_numpy(tpl["faces_uvs"])[None]
    uv_mask = torch.from_numpy(tpl["uv_mask"]).double() / 255
    stamps = []
    with tempfile.TemporaryDirectory() as tmp:
        cfg = get_config(write_yaml=False, use_arm=False, img_size=S, focal_length=focal, base_output_dir=tmp + "/", total_epoch=EPOCHS,
                         training_stage=[100, 100, 101])
        mon = FitMonitor(tmp + "/") if monitor_on else False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        optimize_hand_sequence(cfg, seq, ds, val, ds[:16], layer, uvs, fuvs, device=dev, uv_mask=uv_mask, batch_size=B, monitor=mon,
                               log_fn=lambda e, loss, eng: stamps.append(time.perf_counter()))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        n_files = len([f for f in os.listdir(tmp) if f.endswith(".jpg")])
    res = {"monitor": bool(monitor_on), "fit_wall_s": wall, "epochs_1_to_300_s": stamps[-1] - stamps[0], "files": n_files,
           "device": torch.cuda.get_device_name()}
    if monitor_on:
        per = {}
        for t in mon.timings:
            kind = t["name"].rstrip("0123456789.jpg") or "pred_"
            for k, v in t.items():
                if k.endswith("_ms"):
                    per.setdefault(kind, {}).setdefault(k, []).append(v)
        res["sheets"] = {kind: {k: {"n": len(v), "median": statistics.median(v), "max": max(v)} for k, v in d.items()} for kind, d in per.items()}
        for k in ("render_ms", "sheet_ms", "copy_ms", "encode_ms"):
            res["total_" + k] = sum(t.get(k, 0.0) for t in mon.timings)
        renders = [t["render_ms"] for t in mon.timings if "render_ms" in t]
        res["first_render_ms"], res["total_render_ms_after_first"] = renders[0], sum(renders[1:])
        res.update(sheets_written=len(mon.timings), backpressure_waits=mon.waits, backpressure_wait_s=mon.wait_s)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="time limit of one child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor_time.json"))
    ap.add_argument("--child", choices=["on", "off"], default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child == "on")
    runs = []
    for i in range(2 * a.pairs):
        mode = "on" if i % 2 else "off"
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], capture_output=True, text=True, timeout=a.limit)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"child {i} (monitor {mode}) ended with status {p.returncode}: nothing more is started")
        runs.append(json.loads(line[-1][7:]))
        print(json.dumps(runs[-1]), flush=True)
    off, on = [r for r in runs if not r["monitor"]], [r for r in runs if r["monitor"]]
    med = lambda rs, k: statistics.median(r[k] for r in rs)
    out = {"scene": {"frames": T, "size": S, "frames_per_step": B, "epochs": EPOCHS, "perceptual": False}, "runs": runs,
           "fit_wall_s_monitor_off": med(off, "fit_wall_s"), "fit_wall_s_monitor_on": med(on, "fit_wall_s"),
           "epochs_1_to_300_s_monitor_off": med(off, "epochs_1_to_300_s"), "epochs_1_to_300_s_monitor_on": med(on, "epochs_1_to_300_s")}
    out["overhead_s"] = out["fit_wall_s_monitor_on"] - out["fit_wall_s_monitor_off"]
    out["overhead_epochs_1_to_300_s"] = out["epochs_1_to_300_s_monitor_on"] - out["epochs_1_to_300_s_monitor_off"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}))


if __name__ == "__main__":
    main()
