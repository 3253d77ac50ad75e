"""Where the time of evaluate_sequence(panels=True) goes: the whole pass with and without the panels on a synthetic 64-frame 512 x 512
sequence (wall clock, synchronised), and the added steps one by one for one batch of 32 frames — the extra prepare_mesh + normal render,
ops.panels_u8, the device-to-host copy of the uint8 strips, and the JPEG encoding on the host.

    python tools/dev/gpu_panels_time.py [--frames 64] [--size 512] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from harp_amd import ops  # noqa: E402
from tests.test_gpu_evaluate import _setup  # noqa: E402


def wall(f, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    from PIL import Image
    from harp_amd.evaluate import evaluate_sequence
    from harp_amd.renderer import renderer_helper
    from harp_amd.structures import Meshes
    from harp_amd.utils.visualize import get_mesh_subdivider, prepare_materials, prepare_mesh, render_image
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, S, dev = a.frames, a.size, "cuda"
    warnings.simplefilter("ignore")
    with tempfile.TemporaryDirectory() as tmp:
        sc, cfg, layer, params, ds = _setup(T, S, 21, tmp, self_shadow=True)
        res = {"frames": T, "size": S, "device": torch.cuda.get_device_name()}
        evaluate_sequence(cfg, params, ds, layer, device=dev, panels=True)            # warm-up
        res["evaluate_ms_panels_off"] = wall(lambda: evaluate_sequence(cfg, params, ds, layer, device=dev))
        res["evaluate_ms_panels_on"] = wall(lambda: evaluate_sequence(cfg, params, ds, layer, device=dev, panels=True))
        B = min(32, T)
        fid = torch.arange(B)
        sub = get_mesh_subdivider(layer, device=dev)
        y_true = torch.stack([d[1] for d in ds[:B]]).to(dev).float()
        m = torch.stack([d[2][..., 0] for d in ds[:B]]).to(dev).float()
        with torch.no_grad():
            _, _, normal = renderer_helper.get_renderers(image_size=S, device=dev)
            mat = prepare_materials(params, B, device=dev)
            cam = params["cam"][fid.to(dev)]

            def normal_render():
                _, v, f, t = prepare_mesh(params, fid, layer, False, sub, False, cfg, device=dev, vis_normal=True)
                return render_image(Meshes(v, f, t), cam, B, normal, S, sc["focal"], materials_properties=mat, device=dev)
            y_n = normal_render()
            res["batch"] = B
            res["normal_render_ms"] = wall(normal_render)
            res["panels_u8_ms"] = wall(lambda: ops.panels_u8([y_true, y_true, y_n], m, m))
            u8 = ops.panels_u8([y_true, y_true, y_n], m, m)
            res["d2h_uint8_ms"] = wall(lambda: u8.cpu())
            res["d2h_float_images_ms"] = wall(lambda: (y_true.cpu(), y_true.cpu(), y_n.cpu(), m.cpu(), m.cpu()))      # what the reference copies
            host = u8.cpu().numpy()

            def encode():
                for b in range(B):
                    Image.fromarray(host[b]).save(os.path.join(tmp, "enc_%04d.jpg" % b))
            res["jpeg_encode_ms"] = wall(encode)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
