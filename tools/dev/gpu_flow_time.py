"""What the motion labels cost: harp_flow_layers beside harp_annotate_layers with uv in the same run on the same buffers —
B = 32 frames of the bench scene's synthetic hand at 512 x 512, ss = 1 and 2, L = 1 and 2 layers (the second shown flipped), the players'
own buffers of one batch of flow(rows, rows + 1) ("real") and layers covered everywhere with random depths and faces on both sides
("dense").  Device events around 10 calls in a row after 3 warm-up calls, per call: median [min ... max] of `--repeats` (7).  The
expectation to test: about the annotate call with uv plus one more 9-float gather per owned pixel.
Then play(flow="fw") against play() without, frames per second of a whole motion to disk (host clock, files included).

    python tools/dev/gpu_flow_time.py [--frames 64] [--size 512] [--batch 32] [--repeats 7] [--out profiles/flow_time.json]"""
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
        got = sc.flow(rows, rows + 1)                      # the players' buffers of one batch: the source frames' and the copies of the target frames'
        st = got.status[..., 0]
        res[f"status_share_ss{ss}"] = [float((st == k).float().mean()) for k in range(5)]
        res[f"flow_px_ss{ss}"] = {"mean": float(got.flow[st >= 2].norm(dim=-1).mean()), "max": float(got.flow[st >= 2].norm(dim=-1).max())}
        tp = kept[0].topo
        real = [dict(face_id=pl.s["face_c"], zbuf=pl.s["z_c"], face_label=pl._part_table(), flip=f, ndc=pl.s["ndc_c"], faces=tp.faces,
                     verts_uvs=tp.verts_uvs, faces_uvs=tp.faces_uvs) for pl, f in zip(kept, (False, True))]
        real_to = [dict(ndc=pl.s_to["ndc"], zbuf=pl.s_to["z"]) for pl in kept]
        rnd_z = lambda: (0.2 + 0.8 * torch.rand(B, Sh, Sh, generator=g)).to(dev)      # noqa: E731
        dense = [dict(real[k], face_id=torch.randint(0, tp.F, (B, Sh, Sh), generator=g, dtype=torch.int32).to(dev), zbuf=rnd_z()) for k in range(2)]
        dense_to = [dict(real_to[k], zbuf=rnd_z()) for k in range(2)]
        new = lambda dt, *shape: torch.empty(B, *shape, dtype=dt, device=dev)      # noqa: E731
        o_own, o_part, o_depth, o_face = new(torch.uint8, S, S), new(torch.uint8, S, S), new(torch.float32, S, S), new(torch.int32, S, S)
        o_uv, o_box = new(torch.float32, S, S, 2), torch.zeros(B, 2, 4, dtype=torch.int32, device=dev)
        o_flow, o_dz, o_st = new(torch.float32, S, S, 2), new(torch.float32, S, S), new(torch.uint8, S, S, 2)
        L_, p, stream = _lib.lib(), _lib.ptr, _lib.stream()
        for tag, lay, to in (("real", real, real_to), ("dense", dense, dense_to)):
            for L in (1, 2):
                res[f"flow_{tag}_L{L}_ss{ss}"] = kernel_ms(lambda: ops.flow_layers(lay[:L], to[:L], ss), a.repeats)
                res[f"annotate_{tag}_L{L}_ss{ss}"] = kernel_ms(lambda: ops.annotate_layers(lay[:L], ss, uv=True), a.repeats)
                # the C entries themselves on the same buffers (the wrappers above allocate their outputs and check their arguments per call)
                arr, keep, _, _ = ops._label_layers("time", lay[:L], ss, True)
                fl = (_lib.FlowLayer * L)(*[_lib.FlowLayer(face_id=p(d["face_id"]), zbuf=p(d["zbuf"]), face_label=p(d["face_label"]), ndc=p(d["ndc"]),
                                                           faces=p(d["faces"]), ndc_to=p(t["ndc"]), zbuf_to=p(t["zbuf"]), V=tp.V, F=tp.F,
                                                           flip_x=int(d["flip"]), reserved=0) for d, t in zip(lay[:L], to[:L])])
                res[f"entry_flow_{tag}_L{L}_ss{ss}"] = kernel_ms(
                    lambda: L_.harp_flow_layers(fl, L, B, S, ss, None, 0, None, None, 0, None, ops.FLOW_TOL, p(o_flow), p(o_dz), p(o_st), stream), a.repeats)
                res[f"entry_annotate_{tag}_L{L}_ss{ss}"] = kernel_ms(
                    lambda: L_.harp_annotate_layers(arr, L, B, S, ss, None, 0, None, p(o_own), p(o_part), p(o_depth), p(o_face), p(o_uv), p(o_box), stream), a.repeats)
        # a whole motion to disk, with and without the flow files (host clock around play: encoding and files included)
        one = kept[0]
        tmp = tempfile.mkdtemp()
        try:
            for tag, kw in (("play", {}), ("play_flow", dict(flow="fw"))):
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
