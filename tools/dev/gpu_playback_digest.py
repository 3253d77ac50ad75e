"""One sha256 per output of the playback package (harp_amd/playback/) on a small scene, as JSON: run it over two trees with the same built
library and compare — a change of host code that enqueues the same launches gives the same bytes.  Only the package's public names are
used, so the same file runs against a tree from before the package was split.

The scene: the synthetic hand of bench.py at 64 x 64, 5 frames, batches of 2 (2, 2, 1: the last is padded).  The items: Motion.resample
at linspace(0, 4, 9); Motion.smooth(sigma 1, trim_rot 0.5); Motion.from_keypoints of the fit's own joints; AvatarPlayer.render for ss 1, 2 x
self shadow on / off, each plain, over a background with bg_rows reversed, and with alpha; ScenePlayer.render of two players, one flipped,
at ss 2 with background, scene depth, alpha and owner; every file AvatarPlayer.play (jpg) and ScenePlayer.play(masks, alpha) (png) write.
The label passes: AvatarPlayer.annotate(uv=True) and .flow of a keep_depth player; ScenePlayer.annotate(uv=True) and .flow with the scene
depth under distinct depth_rows / depth_to_rows; ScenePlayer.contact; every file AvatarPlayer.play(labels, flow="both") and
ScenePlayer.play(labels, flow="both", contacts, masks) write (of an .npz its arrays: the archive itself carries the time of writing).

    python tools/dev/gpu_playback_digest.py [--tree DIR] [--out digests.json]      (--tree: the tree whose harp_amd is imported)"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def sha(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().contiguous().numpy()
    return hashlib.sha256(x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes()).hexdigest()


def motion_sha(m):
    return {k: None if getattr(m, k) is None else sha(getattr(m, k)) for k in ("pose", "rot", "trans", "cam", "wrist_pose", "light_positions")}


def files_sha(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".npz"):
            with np.load(os.path.join(d, f)) as z:
                out[f] = {k: sha(z[k]) for k in sorted(z.files)}
            continue
        with open(os.path.join(d, f), "rb") as h:
            out[f] = sha(h.read())
    return out


def fields_sha(t):
    """a namedtuple of tensors, tuples of tensors and Nones -> {field: sha, list of shas, or None}"""
    one = lambda x: None if x is None else sha(x) if torch.is_tensor(x) else [sha(y) for y in x]      # noqa: E731
    return {k: one(getattr(t, k)) for k in t._fields}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(HERE, "..", ".."))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.abspath(a.tree))
    import harp_amd                                        # noqa: F401  (this tree's, before gpu_playback_time puts its own tree in front)
    print("harp_amd of", os.path.dirname(os.path.abspath(harp_amd.__file__)), file=sys.stderr)
    from gpu_playback_time import scene
    from harp_amd.playback import AvatarPlayer, Motion, ScenePlayer
    T, S, B, dev = 5, 64, 2, "cuda"
    cfg, params, layer = scene(T, S, dev)
    g = torch.Generator().manual_seed(11)
    motion = Motion.from_params(params)
    res = {}
    res["resample"] = motion_sha(motion.resample(np.linspace(0, 4, 9), layer, device=dev))
    res["smooth"] = motion_sha(motion.smooth(layer, sigma=1.0, trim_rot=0.5, device=dev))
    with torch.no_grad():
        betas = params["shape"].detach().reshape(1, -1).expand(T, -1).contiguous()
        joints = layer(torch.cat([motion.rot, motion.pose], 1).to(dev), betas, motion.trans.to(dev))[1] / 1000.0      # (mm -> m: the fit's `joints`)
    res["from_keypoints"] = motion_sha(Motion.from_keypoints(joints, params, layer, device=dev))
    bg = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    rows = np.arange(T)
    for ss in (1, 2):
        for shadow in (True, False):
            p = AvatarPlayer(dict(cfg, self_shadow=shadow), params, layer, batch_size=B, ss=ss, device=dev)
            p.load_motion(motion)
            tag = f"avatar_ss{ss}_{'shadow' if shadow else 'plain'}"
            res[tag] = sha(p.render(rows))
            res[tag + "_bg_reversed"] = sha(p.render(rows, bg, rows[::-1].copy()))
            res[tag + "_alpha"] = sha(p.render(rows, alpha=True))
    m1 = Motion.from_params(params, rows=rows[::-1].copy())
    cam = m1.cam.clone()
    cam[:, 0] *= 0.7
    m1.cam = cam.contiguous()
    depth = (0.3 + 0.4 * torch.rand(T, S, S, generator=g)).to(dev)
    depth[:, :, : S // 2] = 0.0                          # no measurement on the left half
    players = [AvatarPlayer(cfg, params, layer, batch_size=B, ss=2, device=dev, keep_depth=True) for _ in range(2)]
    sc = ScenePlayer(players, flip=[False, True])
    sc.load_motions([motion, m1])
    frames, owner = sc.render(rows, bg, None, True, depth, None, owner=True)
    res["scene_frames"], res["scene_owner"] = sha(frames), sha(owner)
    with tempfile.TemporaryDirectory() as d:
        p = AvatarPlayer(cfg, params, layer, batch_size=B, ss=1, device=dev)
        p.play(motion, os.path.join(d, "avatar"), backgrounds=bg, fmt="jpg")
        res["avatar_play_jpg"] = files_sha(os.path.join(d, "avatar"))
        sc.play([motion, m1], os.path.join(d, "scene"), backgrounds=bg, scene_depth=depth, fmt="png", alpha=True, masks=True)
        res["scene_play_png"] = files_sha(os.path.join(d, "scene"))
        to = (rows + 2) % T
        p = AvatarPlayer(cfg, params, layer, batch_size=B, ss=2, device=dev, keep_depth=True)
        p.load_motion(motion)
        res["avatar_annotate_uv"], res["avatar_flow"] = fields_sha(p.annotate(rows, uv=True)), fields_sha(p.flow(rows, to))
        res["scene_annotate_uv"] = fields_sha(sc.annotate(rows, uv=True, scene_depth=depth, depth_rows=rows[::-1].copy()))
        res["scene_flow"] = fields_sha(sc.flow(rows, to, scene_depth=depth, depth_rows=rows[::-1].copy(), depth_to_rows=(rows + 1) % T))
        res["scene_contact"] = fields_sha(sc.contact(rows, 1.0))
        p.play(motion, os.path.join(d, "avatar_labels"), backgrounds=bg, fmt="png", labels=True, flow="both")
        res["avatar_play_labels"] = files_sha(os.path.join(d, "avatar_labels"))
        sc.play([motion, m1], os.path.join(d, "scene_labels"), backgrounds=bg, scene_depth=depth, fmt="png", masks=True, labels=True, flow="both",
                contacts=True, contact_dist=1.0)
        res["scene_play_labels"] = files_sha(os.path.join(d, "scene_labels"))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
