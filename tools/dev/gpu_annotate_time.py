"""What the labels cost: ops.annotate_layers with every output, and ops.keypoint_visibility, beside ops.composite_layers_u8
in the same run on the same buffers — B = 32 frames of the bench scene's synthetic hand at 512 x 512, ss = 1 and 2, L = 1 and 2 layers (the
second shown flipped), the players' own buffers of one batch (a hand covers about a seventh of the frame) and layers covered everywhere
with random depths and faces (every sub-sample has a winner).  Device events around 10 calls in a row after 3 warm-up calls, per call:
median [min ... max] of `--repeats` (7).  The expectation to test: the map kernel reads 8 bytes per sub-sample and layer where the composite
reads 4 to 16, and evaluates one barycentric triple per pixel, so it should cost about what the composite does.
Then play(labels=True) against play() without, frames per second of a whole motion to disk (host-clock, files included).

    python tools/dev/gpu_annotate_time.py [--frames 64] [--size 512] [--batch 32] [--repeats 7] [--out profiles/annotate_time.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gpu_playback_time import scene  # noqa: E402
from gpu_scene_time import kernel_ms  # noqa: E402
from harp_amd import _lib, ops  # noqa: E402


def main():
    from harp_amd.playback import AvatarPlayer, Motion, ScenePlayer
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, S, B, dev = a.frames, a.size, a.batch, "cuda"
    cfg, params, layer = scene(T, S, dev)
    res = {"frames": T, "size": S, "batch": B, "warmup_calls": 3, "repeats": a.repeats, "device": torch.cuda.get_device_name()}
    m0 = Motion.from_params(params)
    m1 = Motion.from_params(params, rows=np.arange(T)[::-1].copy())
    cam = m1.cam.clone()
    cam[:, 0] *= 0.7                                       # farther away, and 60 px to the side at its depth (tools/dev/gpu_scene_time.py's scene)
    cam[:, 1] += 60.0 * 2.0 / (S * cam[:, 0])
    m1.cam = cam.contiguous()
    g = torch.Generator().manual_seed(3)
    rows = np.arange(B)
    for ss in (1, 2):
        Sh = S * ss
        kept = [AvatarPlayer(cfg, params, layer, batch_size=B, ss=ss, device=dev, keep_depth=True) for _ in range(2)]
        sc = ScenePlayer(kept, flip=[False, True])
        sc.load_motions([m0, m1])
        sc.render(rows)                                    # the players' buffers of one batch, colour included
        tp = kept[0].topo
        real = [dict(face_id=pl.s["face_c"], zbuf=pl.s["z_c"], face_label=pl._part_table(), flip=f, ndc=pl.s["ndc_c"], faces=tp.faces,
                     verts_uvs=tp.verts_uvs, faces_uvs=tp.faces_uvs) for pl, f in zip(kept, (False, True))]
        dense = [dict(real[k], face_id=torch.randint(0, tp.F, (B, Sh, Sh), generator=g, dtype=torch.int32).to(dev),
                      zbuf=(0.2 + 0.8 * torch.rand(B, Sh, Sh, generator=g)).to(dev)) for k in range(2)]
        rgb = [pl.s["rgb"] for pl in kept]
        new = lambda dt, *shape: torch.empty(B, *shape, dtype=dt, device=dev)      # noqa: E731
        o_own, o_part, o_depth, o_face = new(torch.uint8, S, S), new(torch.uint8, S, S), new(torch.float32, S, S), new(torch.int32, S, S)
        o_uv, o_box, out3, white = new(torch.float32, S, S, 2), torch.zeros(B, 2, 4, dtype=torch.int32, device=dev), new(torch.uint8, S, S, 3), torch.ones(3, device=dev)
        L_, p, st = _lib.lib(), _lib.ptr, _lib.stream()
        for tag, lay in (("real", real), ("dense", dense)):
            for L in (1, 2):
                res[f"annotate_{tag}_L{L}_ss{ss}"] = kernel_ms(lambda: ops.annotate_layers(lay[:L], ss, uv=True), a.repeats)
                res[f"annotate_nouv_{tag}_L{L}_ss{ss}"] = kernel_ms(lambda: ops.annotate_layers(lay[:L], ss), a.repeats)
                res[f"composite_{tag}_L{L}_ss{ss}"] = kernel_ms(
                    lambda: ops.composite_layers_u8([(c, d["zbuf"], d["flip"]) for c, d in zip(rgb[:L], lay[:L])], ss, owner=True), a.repeats)
                res[f"keypoints_{tag}_L{L}_ss{ss}"] = kernel_ms(
                    lambda: ops.keypoint_visibility(kept[0].s["joints_m"], kept[0].s["cam_R"], kept[0].s["cam_T"], cfg["focal_length"], S, lay[:L], 0, ss),
                    a.repeats)
                # the C entries themselves on the same buffers (the wrappers above allocate their outputs and check their arguments per call)
                arr, keep, _, _ = ops._label_layers("time", lay[:L], ss, True)
                comp = (_lib.Layer * L)(*[_lib.Layer(p(c), p(d["zbuf"]), int(d["flip"]), 0) for c, d in zip(rgb[:L], lay[:L])])
                res[f"entry_annotate_{tag}_L{L}_ss{ss}"] = kernel_ms(
                    lambda: L_.harp_annotate_layers(arr, L, B, S, ss, None, 0, None, p(o_own), p(o_part), p(o_depth), p(o_face), p(o_uv), p(o_box), st), a.repeats)
                res[f"entry_composite_{tag}_L{L}_ss{ss}"] = kernel_ms(
                    lambda: L_.harp_composite_layers_u8(comp, L, B, S, ss, None, 0, None, None, 0, None, p(white), 3, p(out3), p(o_own), st), a.repeats)
        own = ops.annotate_layers(real, ss).owner
        res[f"owned_share_ss{ss}"] = [float((own == k).float().mean()) for k in (0, 1, 2)]
        # a whole motion to disk, with and without the label files (host clock around play: encoding and files included)
        one = kept[0]
        tmp = tempfile.mkdtemp()
        try:
            for tag, kw in (("play", {}), ("play_labels", dict(labels=True))):
                fps = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    one.play(m0, os.path.join(tmp, tag), fmt="jpg", **kw)
                    torch.cuda.synchronize()
                    fps.append(T / (time.perf_counter() - t0))
                res[f"{tag}_ss{ss}_frames_per_s"] = {"median": sorted(fps)[1], "min": min(fps), "max": max(fps), "n": 3}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        del sc, kept, one
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
