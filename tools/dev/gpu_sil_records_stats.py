"""Silhouette records per 16x16 tile of the camera view (harp_sil_records_bind) in the bench's scenes: tiles with records, the largest
count, the total per call — the numbers the engine's record capacity (FitEngine.sil_rec_cap) is chosen from.
usage: python tools/dev/gpu_sil_records_stats.py [hand:512:32 arm:1024:8 ...]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests._scene import make_fit_case  # noqa: E402


def main(specs):
    for spec in specs:
        kind, S, B = spec.split(":")
        S, B = int(S), int(B)
        case = make_fit_case(kind, T=min(B, 4), S=S, B=B, seed=2, device="cuda")
        eng = case["eng"]
        eng.keep_image = False
        eng.set_schedule((torch.arange(B) % min(B, 4)).reshape(1, B).int())
        for app in (False, True):
            eng.step(None, True, app, use_graph=False)
            torch.cuda.synchronize()
            s = eng.s
            rec = s["sil_rec"]
            nsx = (S + 63) // 64
            nt = B * nsx * nsx * 16
            rec.zero_()                               # (counts of tiles without faces are never written: zero them, then one more step)
            eng.step(None, True, app, use_graph=False)
            torch.cuda.synchronize()
            c = rec[:nt * 4].view(torch.int32).cpu()
            nz = c[c > 0].float()
            q = torch.quantile(nz, torch.tensor([0.5, 0.99, 0.999])).tolist() if nz.numel() else [0, 0, 0]
            print(f"{kind} S={S} B={B} stage={'both' if app else 'geometry'}: tiles with records {nz.numel()} of {nt}, records {int(nz.sum())}, "
                  f"max {int(c.max())}, median {q[0]:.0f}, p99 {q[1]:.0f}, p99.9 {q[2]:.0f}, over cap {eng.sil_rec_cap}: {(c > eng.sil_rec_cap).sum().item()}",
                  flush=True)
        del eng, case


if __name__ == "__main__":
    main(sys.argv[1:] or ["hand:512:32", "arm:1024:32"])
