"""What the contact labels cost: ScenePlayer.contact on one batch of B = 32 frames of two hand avatars (the bench scene's
synthetic hand twice, the second playing the motion backwards) with the hands touching (the second 4 cm to the side) and
apart (0.5 m), beside annotate on the same batch for scale; the two harp_mesh_contact calls alone on the players' buffers, with
max_dist = CONTACT_DIST and without a limit (nothing culled by max_dist, the winding pass in every wave).  Device events around 10 calls
in a row after 3 warm-up calls, per call: median [min ... max] of `--repeats` (7).
Then, on the host in float64 from the same buffers, the share of (tile of 64 query vertices, chunk of 128 target faces) pairs that
survive the kernel's cull in the touching case: its loop restated wave by wave (four running worst distances per tile, one per wave's
chunks) with the brute-force distances (tests/_contact_ref.py) of two frames.

    python tools/dev/gpu_contact_time.py [--frames 64] [--size 512] [--batch 32] [--repeats 7] [--out profiles/contact_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from gpu_playback_time import scene  # noqa: E402
from gpu_scene_time import kernel_ms  # noqa: E402
from harp_amd import ops  # noqa: E402
from tests import _contact_ref as CR  # noqa: E402

TILE, CHUNK, WAVES, MARGIN = 64, 128, 4, 64.0 * 2.0 ** -24      # csrc/contact.hip: kLanes, kFaces, kWaves, kCullMargin


def surviving_pairs(q, t, max_dists, frames):
    """the kernel's pass 1 restated on the host, wave by wave: each of a tile's WAVES waves walks the chunks c = w, w + WAVES, ... with a
    running worst best-distance of its own -> per max_dist [staged, all] (tile, chunk) pairs"""
    count = {md: [0, 0] for md in max_dists}
    for b in frames:
        one = lambda d: {k: (v[b:b + 1] if k in ("verts", "cam_R", "cam_T") else v) for k, v in d.items()}      # noqa: E731
        qv = CR.view_space(q["verts"][b:b + 1], q["cam_R"][b:b + 1], q["cam_T"][b:b + 1], q["flip"])[0]
        tv = CR.view_space(t["verts"][b:b + 1], t["cam_R"][b:b + 1], t["cam_T"][b:b + 1], t["flip"])[0]
        F = t["faces"].shape[0]
        D = np.concatenate([CR.mesh_contact(dict(one(q), verts=q["verts"][b:b + 1, lo:lo + 512]), one(t))["D"][0] for lo in range(0, qv.shape[0], 512)])
        n_chunks = -(-F // CHUNK)
        Dc = np.stack([D[:, c * CHUNK:(c + 1) * CHUNK].min(1) for c in range(n_chunks)], 1)
        corners = tv[t["faces"]]                                                  # (F,3,3)
        lo_t = np.stack([corners[c * CHUNK:(c + 1) * CHUNK].min((0, 1)) for c in range(n_chunks)])
        hi_t = np.stack([corners[c * CHUNK:(c + 1) * CHUNK].max((0, 1)) for c in range(n_chunks)])
        for md in max_dists:
            for v0 in range(0, qv.shape[0], TILE):
                p = qv[v0:v0 + TILE]
                lo_q, hi_q = p.min(0), p.max(0)
                best = np.full((WAVES, p.shape[0]), np.inf)
                for c in range(n_chunks):
                    gap = np.linalg.norm(np.maximum(0.0, np.maximum(lo_t[c] - hi_q, lo_q - hi_t[c])))
                    m = max(np.abs(lo_q).max(), np.abs(hi_q).max(), np.abs(lo_t[c]).max(), np.abs(hi_t[c]).max())
                    count[md][1] += 1
                    if gap - MARGIN * m > min(md, best[c % WAVES].max()):
                        continue
                    count[md][0] += 1
                    best[c % WAVES] = np.minimum(best[c % WAVES], Dc[v0:v0 + TILE, c])
    return count


def main():
    from harp_amd.playback import CONTACT_DIST, AvatarPlayer, Motion, ScenePlayer
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, S, B, dev = a.frames, a.size, a.batch, "cuda"
    cfg, params, layer = scene(T, S, dev)
    res = {"frames": T, "size": S, "batch": B, "warmup_calls": 3, "repeats": a.repeats, "device": torch.cuda.get_device_name(), "max_dist": CONTACT_DIST}
    m0 = Motion.from_params(params)
    rows = np.arange(B)
    players = [AvatarPlayer(cfg, params, layer, batch_size=B, ss=1, device=dev, keep_depth=True) for _ in range(2)]
    sc = ScenePlayer(players, flip=[False, False])
    res["V"], res["F"] = players[0].topo.V, players[0].topo.F
    for tag, dx in (("touching", 0.04), ("apart", 0.5)):
        m1 = Motion.from_params(params, rows=np.arange(T)[::-1].copy())
        cam = m1.cam.clone()
        cam[:, 1] += dx
        m1.cam = cam.contiguous()
        sc.load_motions([m0, m1])
        c = sc.contact(rows)
        res[f"{tag}_in_contact_share"] = float(np.mean([float((o > 0).float().mean()) for o in c.other]))
        res[f"{tag}_inside_share"] = float(np.mean([float((d < 0).float().mean()) for d in c.dist]))
        res[f"{tag}_min_dist"] = float(c.min_dist.min())
        res[f"{tag}_max_penetration"] = float(c.max_penetration.max())
        res[f"contact_{tag}"] = kernel_ms(lambda: sc.contact(rows), a.repeats)
        res[f"annotate_{tag}"] = kernel_ms(lambda: sc.annotate(rows), a.repeats)
        sc.contact(rows)                                   # the players hold the batch's geometry again
        side = [ops.ContactMesh(pl.s["vd"], pl.s["cam_R"], pl.s["cam_T"], pl.topo.faces, f) for pl, f in zip(players, sc.flip)]
        for name, md in (("contact_dist", CONTACT_DIST), ("no_limit", float("inf"))):
            res[f"op_pair_{tag}_{name}"] = kernel_ms(lambda: (ops.mesh_contact(side[0], side[1], md), ops.mesh_contact(side[1], side[0], md)), a.repeats)
            res[f"op_pair_{tag}_{name}_dist_only"] = kernel_ms(lambda: (ops.mesh_contact(side[0], side[1], md, want=("dist", "face")),
                                                                        ops.mesh_contact(side[1], side[0], md, want=("dist", "face"))), a.repeats)
        if tag == "touching":
            host = [dict(verts=s.verts.cpu().numpy(), cam_R=s.cam_R.cpu().numpy(), cam_T=s.cam_T.cpu().numpy(), faces=s.faces.cpu().numpy(), flip=s.flip)
                    for s in side]
            count = surviving_pairs(host[0], host[1], (CONTACT_DIST, float("inf")), (0, B // 2))
            for name, md in (("contact_dist", CONTACT_DIST), ("no_limit", float("inf"))):
                res[f"surviving_tile_chunk_pairs_{name}"] = {"staged": count[md][0], "of": count[md][1], "share": count[md][0] / count[md][1]}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
