"""What the self-contact labels cost: one batch of B = 32 frames of one hand avatar (the bench scene's synthetic hand, 3093
vertices / 6152 faces) against ITSELF under its exclusion table of SELF_GEODESIC, as an open hand (every finger rotation zero) and as a
fist (every finger joint flexed by 1.2 rad), at max_dist = SELF_CONTACT_DIST (0.004) and CONTACT_DIST (0.02), with and without the
winding pass: ops.mesh_contact(..., exclude=) on the player's buffers, and the player's own self_contact (front, kernel, composition).
Beside them, for scale, the code before this label existed: ops.mesh_contact of the open hand against a second one 4 cm to the side.
Device events around 10 calls in a row after 3 warm-up calls, per call: median [min ... max] of `--repeats` (7).

Every step is a fresh process under a time limit of its own, started by this one (which does not touch the device) only after the step
before it has ended well; a step that fails, faults or runs out of time ends the run.

    python tools/dev/gpu_self_contact_time.py [--batch 32] [--size 128] [--repeats 7] [--out profiles/self_contact_time.json]"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = (("open", 300), ("fist", 300), ("pair", 300))                          # (step, its time limit in seconds)
FIST = 1.2                                                                      # rad about z on every finger joint


def _motion(params, layer, B, flex, dx=0.0):
    """B rows of the fit's first frame with every finger joint rotated by `flex` about z, the camera moved dx metres to the side"""
    import numpy as np
    import torch
    from harp_amd.playback import Motion
    m = Motion.from_params(params, rows=np.zeros(B, np.int64))
    pose = torch.zeros(B, 15, 3)
    pose[:, :, 2] = flex
    hm = torch.from_numpy(np.asarray(layer._model_np["hands_mean"], np.float32)).reshape(1, 45)
    m.pose = (pose.reshape(B, 45) - hm).to(m.pose.device).contiguous()
    cam = m.cam.clone()
    cam[:, 1] += dx
    m.cam = cam.contiguous()
    return m


def step(name, a):
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "..", ".."))
    from gpu_playback_time import scene
    from gpu_scene_time import kernel_ms
    from harp_amd import ops
    from harp_amd.playback import CONTACT_DIST, SELF_CONTACT_DIST, SELF_GEODESIC, AvatarPlayer
    B, dev = a.batch, "cuda"
    cfg, params, layer = scene(B, a.size, dev)
    rows = np.arange(B)
    res = {}
    pl = AvatarPlayer(cfg, params, layer, batch_size=B, ss=1, device=dev)
    side = lambda p: ops.ContactMesh(p.s["vd"], p.s["cam_R"], p.s["cam_T"], p.topo.faces, False)      # noqa: E731
    if name == "pair":                                                          # the code before: one hand against another, no table
        other = AvatarPlayer(cfg, params, layer, batch_size=B, ss=1, device=dev)
        pl.load_motion(_motion(params, layer, B, 0.0))
        other.load_motion(_motion(params, layer, B, 0.0, dx=0.04))
        pl.render(rows)                                                         # (the players hold the batch's geometry)
        other.render(rows)
        q, t = side(pl), side(other)
        for md in (SELF_CONTACT_DIST, CONTACT_DIST):
            c = ops.mesh_contact(q, t, md)
            res[f"pair_{md:g}_near_share"] = float(torch.isfinite(c.dist).float().mean())
            res[f"pair_{md:g}"] = kernel_ms(lambda: ops.mesh_contact(q, t, md), a.repeats)
            res[f"pair_{md:g}_dist_only"] = kernel_ms(lambda: ops.mesh_contact(q, t, md, want=("dist", "face")), a.repeats)
        return res
    pl.load_motion(_motion(params, layer, B, FIST if name == "fist" else 0.0))
    c = pl.self_contact(rows)
    table = pl._exclusion_table(SELF_GEODESIC)
    res.update(V=pl.topo.V, F=pl.topo.F, device=torch.cuda.get_device_name(), geodesic=SELF_GEODESIC,
               table_bytes=table.numel() * 4, excluded_share=float(torch.cat([(table >> k) & 1 for k in range(32)]).float().mean()))
    s = side(pl)
    for md in (SELF_CONTACT_DIST, CONTACT_DIST):
        c = pl.self_contact(rows, md)
        res[f"{name}_{md:g}_near_share"] = float(torch.isfinite(c.dist).float().mean())
        res[f"{name}_{md:g}_inside_share"] = float((c.dist < 0).float().mean())
        res[f"{name}_{md:g}_self_contact"] = kernel_ms(lambda: pl.self_contact(rows, md), a.repeats)
        pl.self_contact(rows, md)                                               # (the player holds the batch's geometry again)
        res[f"{name}_{md:g}_op"] = kernel_ms(lambda: ops.mesh_contact(s, s, md, exclude=table), a.repeats)
        res[f"{name}_{md:g}_op_dist_only"] = kernel_ms(lambda: ops.mesh_contact(s, s, md, want=("dist", "face"), exclude=table), a.repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(what a child process runs: one of %s)" % ", ".join(s for s, _ in STEPS))
    a = ap.parse_args()
    if a.step is not None:
        print("RESULT " + json.dumps(step(a.step, a)))
        return 0
    res = {"batch": a.batch, "size": a.size, "warmup_calls": 3, "repeats": a.repeats, "fist_flexion_rad": FIST}
    for name, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--batch", str(a.batch), "--size", str(a.size),
               "--repeats", str(a.repeats)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:                                                # nothing more is started on the device after a failure
            print(f"step {name} ended with status {done.returncode}; stopping", file=sys.stderr)
            return done.returncode
        res.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
