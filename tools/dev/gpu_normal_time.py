"""Time the fused normal renderer (ops.normal_image, csrc/present.hip) against the torch chain over the fragment-level rasteriser (what
NormalRenderer runs when an autograd graph is needed, and all it ran before), each with and without a normal map, on the bench scenes
(same generator as bench.py): alternating calls in one run, warmed up, with device events; peak memory of each from max_memory_allocated.

    python tools/dev/gpu_normal_time.py [--reps 10] [--out profiles/normal_image_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -o normal -- python tools/dev/gpu_normal_time.py --reps 3 --profile

Algorithmic bytes of the fused kernel: NDC vertices and normals (2 x B V 12), face table (F 12), one 64-B record + 16-B box per (frame,
face) written and read once, 16 B per pixel out; with a map the uv tables and at most 4 texels x 12 B per covered pixel and kept
fragment (an upper bound: neighbouring pixels share texels).  The share of the 8 TB/s roofline is those bytes over the measured time."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bench  # noqa: E402
from harp_amd import ops  # noqa: E402
from harp_amd.renderer import renderer_helper as RH  # noqa: E402
from harp_amd.structures import TexturesUV  # noqa: E402

K = 10
SHAPES = (("hand", 512, 8), ("hand", 512, 32), ("arm", 1024, 8))
HBM_BYTES_PER_S = 8e12


def torch_chain(ndc, vn, faces, S, nmap, vuv, fuv):
    B, Fn = ndc.shape[0], faces.shape[0]
    fr = RH.Fragments(*ops.rasterize_fragments(ndc, faces, S, 0.0, K))
    pix_n = RH.interpolate_face_attributes(fr.pix_to_face, fr.bary_coords, vn[:, faces.long()].reshape(B * Fn, 3, 3))
    if nmap is not None:
        pix_n = RH.apply_normal_map(pix_n, RH.sample_textures_uv(TexturesUV(nmap[None].expand(B, -1, -1, -1), fuv.long(), vuv), fr, Fn))
    pix_n = pix_n * torch.tensor([1.0, -1.0, -1.0], device=pix_n.device)
    return RH.softmax_rgb_blend((pix_n + 1.0) / 2.0, fr)


def scene(kind, S, B, dev):
    eng, _ = bench.build_engine(0, 1, dev, T=B, img=S, B=B, kind=kind)
    eng.fid.copy_(torch.arange(B, dtype=torch.int32, device=dev))
    eng.tfid.zero_()
    eng.forward_backward(True, True)
    torch.cuda.synchronize()
    out = (eng.s["ndc_c"][:B].clone(), eng.s["n2"][:B].clone(), eng.topo.faces, eng.topo.verts_uvs, eng.topo.faces_uvs)
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--profile", action="store_true", help="only a few calls of ops.normal_image per shape (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(9)
    nmap = torch.nn.functional.normalize(torch.tensor([0., 0., 1.]).repeat(512, 512, 1) + torch.randn(512, 512, 3, generator=g) * 0.2, dim=-1).to(dev)
    res = {"K": K, "reps": a.reps, "device": torch.cuda.get_device_name(), "shapes": []}
    for kind, S, B in SHAPES:
        ndc, vn, faces, vuv, fuv = scene(kind, S, B, dev)
        V, Fn = ndc.shape[1], faces.shape[0]
        with torch.no_grad():
            for use_map in (False, True):
                m = nmap if use_map else None
                run = {"fused": lambda: ops.normal_image(ndc, vn, faces, S, K, nmap=m, verts_uvs=vuv, faces_uvs=fuv, check_uvs=False)}
                if not a.profile:
                    run["torch"] = lambda: torch_chain(ndc, vn, faces, S, m, vuv, fuv)
                for f in run.values():
                    for _ in range(2):
                        f()
                torch.cuda.synchronize()
                times, peak = {k: [] for k in run}, {}
                for _ in range(a.reps):
                    for k, f in run.items():                 # alternating in one run
                        torch.cuda.reset_peak_memory_stats()
                        base = torch.cuda.memory_allocated()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        img = f()
                        e1.record()
                        torch.cuda.synchronize()
                        times[k].append(e0.elapsed_time(e1))
                        peak[k] = torch.cuda.max_memory_allocated() - base
                        del img
                if a.profile:
                    continue
                covered = float((run["fused"]()[..., 3] > 0).float().mean())
                diff = float((run["fused"]() - run["torch"]()).abs().max())
                nbytes = 2 * B * V * 12 + Fn * 12 + 2 * B * Fn * 80 + B * S * S * 16
                if use_map:
                    nbytes += vuv.numel() * 4 + Fn * 12 + int(covered * B * S * S) * 48
                row = {"kind": kind, "S": S, "B": B, "V": V, "F": Fn, "normal_map": use_map, "covered_share": covered, "max_abs_diff": diff,
                       "algorithmic_bytes": nbytes}
                for k, v in times.items():
                    v = sorted(v)
                    row[k] = {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "peak_bytes": peak[k]}
                row["fused"]["roofline_share"] = nbytes / (row["fused"]["ms_median"] * 1e-3) / HBM_BYTES_PER_S
                row["speedup_median"] = row["torch"]["ms_median"] / row["fused"]["ms_median"]
                res["shapes"].append(row)
                print(json.dumps(row), flush=True)
        del ndc, vn
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    if a.out and not a.profile:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
