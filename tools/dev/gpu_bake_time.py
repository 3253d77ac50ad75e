"""What the UV bake costs: harp_amd.bake.bake_texture for the bench scene — 256 frames, 512 x 512, the 3093-vertex hand,
chunks of 32 — device synchronised and warmed, beside one fitting epoch (8 steps of 32 frames, both stages) of the same sequence through
FitEngine.step, which this feature does not touch.

    python tools/dev/gpu_bake_time.py [--reps 3] [--out profiles/bake_time.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/dev/gpu_bake_time.py --profile      # one warm call + one call, bake only"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
T, S, B = 256, 512, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bake_time.json"))
    a = ap.parse_args()
    import tempfile
    from types import SimpleNamespace
    import torch
    from harp_amd import synth
    from harp_amd.bake import bake_texture
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.optimize_sequence import export_params
    from harp_amd.utils.config_utils import get_config
    from tests._scene import make_fit_case
    dev = "cuda"
    case = make_fit_case("hand", T=T, S=S, B=B, seed=0, device=dev)
    eng, tpl = case["eng"], case["tpl"]
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=synth.make_mano_model(tpl, seed=0), device=dev)
    uvs, fuvs = torch.from_numpy(tpl["verts_uvs"])[None], torch.from_numpy(tpl["faces_uvs"])[None]
    cfg = get_config(write_yaml=False, use_arm=False, img_size=S, focal_length=case["focal"], base_output_dir=tempfile.gettempdir() + "/")
    params = export_params(eng, {"joints": case["init_joints"]}, uvs, fuvs, case["uv_mask"], layer)
    targets = SimpleNamespace(fid=torch.arange(T, dtype=torch.int32), y_true=eng.y_true, y_sil_col=eng.y_sil_col)

    def bake():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = bake_texture(cfg, params, targets, layer, chunk=B, device=dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    _, out = bake()                                                  # warm: texel map, allocator
    if a.profile:
        bake()
        return
    bakes = [bake()[0] for _ in range(a.reps)]
    fids = torch.arange(T, dtype=torch.int32).reshape(T // B, B)
    eng.set_schedule(fids, tschedule=fids.long())

    def epoch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(T // B):
            eng.step(None, True, True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(3):                                               # warm: graph capture
        eng.set_schedule(fids, tschedule=fids.long())
        epoch()
    epochs = []
    for _ in range(a.reps):
        eng.set_schedule(fids, tschedule=fids.long())
        epochs.append(epoch())
    res = {"scene": {"frames": T, "size": S, "chunk": B, "vertices": 3093}, "device": torch.cuda.get_device_name(),
           "bake_texture_s": bakes, "bake_texture_median_s": statistics.median(bakes),
           "fit_epoch_s": epochs, "fit_epoch_median_s": statistics.median(epochs),
           "coverage": out["coverage"], "texels_seen": int(out["seen"].sum()), "texels_covered": int(out["covered"].sum())}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
