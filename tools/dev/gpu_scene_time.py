"""What ScenePlayer.render costs on the bench scene (256 frames of the synthetic hand at 512 x 512, batches of 32, self shadow on) with two
avatars — the fit itself and the same fit on a second motion, farther away, shifted and shown flipped — next to what the tree could do
before: two AvatarPlayer.render calls in sequence (which cannot occlude each other); and the composite kernel alone for 1, 2 and 4 layers
next to harp_resolve_u8 alone on the same buffers.

Per ss = 1 and 2, after 3 warm-up batches: device-event time per batch of 32 frames, medians over `--repeats` passes with their spread
(tools/dev/gpu_playback_time.py's method).  The kernels alone: device events around 10 launches in a row, per launch, on (i) the players'
own buffers of the last batch (a hand covers about a seventh of the frame) and (ii) layers that are covered everywhere with random depths,
the composite's worst case: every layer's colour is read wherever it wins.  `bound` is the issue's yardstick: 1.25 x the byte ratio
(16 ss^2 L + 3) / (16 ss^2 + 3) (3: the output bytes; no background image here) x the resolve's time.

    python tools/dev/gpu_scene_time.py [--frames 256] [--size 512] [--batch 32] [--repeats 7] [--out profiles/scene_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gpu_playback_time import scene, stats, timed_passes  # noqa: E402
from harp_amd import _lib  # noqa: E402


def kernel_ms(fn, repeats, inner=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return stats(out)


def main():
    from harp_amd.playback import AvatarPlayer, Motion, ScenePlayer
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, S, B, dev = a.frames, a.size, a.batch, "cuda"
    cfg, params, layer = scene(T, S, dev)
    batches = [np.arange(lo, min(T, lo + B)) for lo in range(0, T, B)]
    res = {"frames": T, "size": S, "batch": B, "self_shadow": True, "warmup_batches": 3, "repeats": a.repeats, "device": torch.cuda.get_device_name()}
    m0 = Motion.from_params(params)
    m1 = Motion.from_params(params, rows=np.arange(T)[::-1].copy())
    cam = m1.cam.clone()
    cam[:, 0] *= 0.7                                       # farther away, and 60 px to the side at its depth
    cam[:, 1] += 60.0 * 2.0 / (S * cam[:, 0])
    m1.cam = cam.contiguous()
    g = torch.Generator().manual_seed(3)
    for ss in (1, 2):
        make = lambda keep: [AvatarPlayer(cfg, params, layer, batch_size=B, ss=ss, device=dev, keep_depth=keep) for _ in range(2)]
        # (a) what the tree could do before: two players, one after the other
        plain = make(False)
        for p, m in zip(plain, (m0, m1)):
            p.load_motion(m)

        def two(rows):
            plain[0].render(rows)
            plain[1].render(rows)

        res[f"two_players_ss{ss}"] = timed_passes(two, batches, 3, a.repeats)
        res[f"one_player_ss{ss}"] = timed_passes(plain[0].render, batches, 3, a.repeats)
        del plain
        # (b) the scene
        kept = make(True)
        sc = ScenePlayer(kept, flip=[False, True])
        sc.load_motions([m0, m1])
        res[f"scene_ss{ss}"] = timed_passes(sc.render, batches, 3, a.repeats)
        own = sc.render(batches[0], owner=True)[1]
        res[f"scene_ss{ss}_owned_share"] = [float((own == k).float().mean()) for k in (0, 1, 2)]
        # (c) the kernels alone on the last batch's buffers, and on layers covered everywhere
        Sh = S * ss
        real = [(p.s["rgb"], p.s["z_c"]) for p in kept]
        dense = [(torch.rand(B, Sh, Sh, 3, generator=g).to(dev), (0.2 + 0.8 * torch.rand(B, Sh, Sh, generator=g)).to(dev)) for _ in range(4)]
        out3, fid_dense = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev), torch.zeros(B, Sh, Sh, dtype=torch.int32, device=dev)
        white, L_, p, st = torch.ones(3, device=dev), _lib.lib(), _lib.ptr, _lib.stream()
        for tag, lay, fid in (("real", [real[0], real[1], real[0], real[1]], kept[0].s["face_c"]), ("dense", dense, fid_dense)):
            # (the C entry points themselves: the ops wrappers' argument checks cost as much host time as these kernels take)
            r = kernel_ms(lambda: L_.harp_resolve_u8(p(lay[0][0]), p(fid), B, S, ss, None, 0, None, p(white), 3, p(out3), st), a.repeats)
            res[f"resolve_{tag}_ss{ss}"] = r
            for L in (1, 2, 4):
                arr = (_lib.Layer * L)(*[_lib.Layer(p(c), p(z), int(f), 0) for (c, z), f in zip(lay[:L], [False, True, False, True])])
                k = kernel_ms(lambda: L_.harp_composite_layers_u8(arr, L, B, S, ss, None, 0, None, None, 0, None, p(white), 3, p(out3), None, st), a.repeats)
                k["bound_ms"] = 1.25 * (16 * ss * ss * L + 3) / (16 * ss * ss + 3) * r["median"]
                res[f"composite_{tag}_L{L}_ss{ss}"] = k
        del sc, kept
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
