"""-m gpu: ops.image_metrics (csrc/metrics.hip) against the float64 restatement of pytorch_msssim 0.2.1 (tests/_msssim_ref.py), the exact
cases, IoU / L1 against utils/eval_util.py, determinism, and the pytorch_msssim drop-in.

Bound: per-image MS-SSIM and every per-level, per-channel ssim and cs within 1e-5 absolute of float64 (the kernel computes each window's
moments about its own centre pixel, so flat regions do not cancel in float32).  Measured on the MI355X: worst per-image MS-SSIM 4.6e-6,
worst per-level ssim / cs 9.2e-6 (176² x 64 rendered-looking pairs; random and smooth pairs <= 1.2e-6); L1 sums 2.8e-8 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _msssim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _images(kind, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        X = torch.rand(N, 3, H, W, generator=g)
        Y = (X + 0.3 * torch.rand(N, 3, H, W, generator=g)).clamp(0, 1)
    elif kind == "wide":                                   # values outside [0, 1]
        X = torch.rand(N, 3, H, W, generator=g) * 2.0 - 0.5
        Y = X + 0.4 * torch.randn(N, 3, H, W, generator=g)
    elif kind == "smooth":
        X = F.interpolate(torch.rand(N, 3, 9, 11, generator=g), size=(H, W), mode="bicubic", align_corners=False)
        Y = X + 0.05 * F.interpolate(torch.randn(N, 3, 13, 7, generator=g), size=(H, W), mode="bilinear", align_corners=False)
    else:                                                  # "rendered": flat white background, a textured blob shifted between the two
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        tex = F.interpolate(torch.rand(N, 3, 24, 24, generator=g), size=(H, W), mode="bilinear", align_corners=False) * 0.6 + 0.2
        def blob(cy, cx):
            return (((yy - cy) / (0.3 * H)) ** 2 + ((xx - cx) / (0.25 * W)) ** 2 < 1).float()
        mx, my = blob(0.5 * H, 0.5 * W), blob(0.53 * H, 0.47 * W)
        X = torch.ones(N, 3, H, W) * (1 - mx) + tex * mx
        Y = torch.ones(N, 3, H, W) * (1 - my) + (tex * 0.9 + 0.02 * torch.rand(N, 3, H, W, generator=g)) * my
    return X.float().contiguous(), Y.float().contiguous()


def _run(X, Y, layout, **kw):
    """X, Y (N,C,H,W) CPU -> image_metrics on the device, read through NHWC or NCHW strides"""
    from harp_amd import ops
    if layout == "nhwc":
        return ops.image_metrics(X.permute(0, 2, 3, 1).contiguous().to(DEV), Y.permute(0, 2, 3, 1).contiguous().to(DEV), channels_last=True, **kw)
    return ops.image_metrics(X.to(DEV), Y.to(DEV), channels_last=False, **kw)


CASES = [((161, 161), 7, "random", "nhwc"), ((176, 333), 7, "smooth", "nchw"), ((333, 333), 1, "rendered", "nhwc"),
         ((448, 448), 7, "rendered", "nchw"), ((512, 512), 1, "smooth", "nhwc"), ((176, 176), 64, "rendered", "nhwc"),
         ((200, 240), 7, "wide", "nchw"), ((512, 512), 7, "rendered", "nhwc"), ((333, 176), 64, "smooth", "nchw"),
         ((448, 448), 1, "random", "nhwc")]
WORST = {}


@pytest.mark.parametrize("size,N,kind,layout", CASES)
def test_against_float64_restatement(size, N, kind, layout):
    H, W = size
    X, Y = _images(kind, N, H, W, seed=H * 7 + N)
    got = _run(X, Y, layout)
    ref = R.ms_ssim(X, Y)
    e = {k: (got[k].cpu().double() - ref[k]).abs().max().item() for k in ("ms_ssim", "ssim", "cs")}
    WORST[(size, N, kind, layout)] = e
    print(f"[image_metrics vs float64] {H}x{W} N={N} {kind} {layout}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) <= 1e-5, e
    assert got["ssim"].shape == (N, 5, 3) and got["cs"].shape == (N, 5, 3)


def test_exact_cases():
    X, _ = _images("rendered", 3, 200, 176, seed=5)
    got = _run(X, X.clone(), "nhwc")
    assert torch.equal(got["ms_ssim"].cpu(), torch.ones(3)) and torch.equal(got["ssim"].cpu(), torch.ones(3, 5, 3))
    assert torch.equal(got["cs"].cpu(), torch.ones(3, 5, 3))
    Xr = torch.rand(2, 3, 190, 170, generator=torch.Generator().manual_seed(6))
    assert torch.equal(_run(Xr, 1 - Xr, "nchw")["ms_ssim"].cpu(), torch.zeros(2))
    for S, (a, b) in [(512, (0.4, 0.6)), (448, (0.3, 0.45))]:
        got = _run(torch.full((1, 3, S, S), a), torch.full((1, 3, S, S), b), "nchw")
        want = ((2 * a * b + 1e-4) / (a * a + b * b + 1e-4)) ** 0.1333
        assert abs(got["ms_ssim"].item() - want) < 1e-5, (got["ms_ssim"].item(), want)


def test_iou_and_l1_against_eval_util():
    from harp_amd.utils import eval_util as E
    N, H, W = 7, 181, 203
    X, Y = _images("random", N, H, W, seed=9)
    g = torch.Generator().manual_seed(10)
    rm, pm = torch.rand(N, H, W, generator=g), torch.rand(N, H, W, generator=g)
    rm[0] = 0.5                                             # exactly at the threshold: counts as inside
    Xh, Yh = X.permute(0, 2, 3, 1).contiguous(), Y.permute(0, 2, 3, 1).contiguous()
    from harp_amd import ops
    got = ops.image_metrics(Xh.to(DEV), Yh.to(DEV), rm.to(DEV), pm[..., None].to(DEV))
    for i in range(N):
        want = torch.as_tensor(E.sil_iou(rm[i:i + 1], pm[i:i + 1]))
        assert torch.equal(got["iou"][i].cpu(), want), (i, got["iou"][i].item(), want.item())
    l1 = (Xh.double() - Yh.double()).abs().sum((1, 2, 3))
    rel = ((got["l1_sum"].cpu().double() - l1).abs() / l1).max().item()
    print(f"[image_metrics] L1 sum rel err vs float64: {rel:.2e}")
    assert rel <= 1e-6
    none = ops.image_metrics(Xh.to(DEV), Yh.to(DEV))
    assert none["iou"] is None and torch.equal(none["l1_sum"], got["l1_sum"]) and torch.equal(none["ms_ssim"], got["ms_ssim"])


def test_deterministic():
    X, Y = _images("rendered", 16, 512, 512, seed=11)
    a, b = _run(X, Y, "nhwc"), _run(X, Y, "nhwc")
    for k in ("inter", "l1_sum", "ms_ssim", "ssim", "cs"):
        assert torch.equal(a[k], b[k]), k


def test_levels_and_weights():
    """fewer levels (weights of length 1..4) and a data range other than 1, against the restatement"""
    X, Y = _images("smooth", 3, 176, 190, seed=12)
    for w in ([1.0], [0.5, 0.5], [0.2, 0.3, 0.5], [0.1, 0.2, 0.3, 0.4]):
        got = _run(X * 255, Y * 255, "nchw", data_range=255, weights=w)
        ref = R.ms_ssim(X * 255, Y * 255, data_range=255, weights=w)
        assert (got["ms_ssim"].cpu().double() - ref["ms_ssim"]).abs().max() <= 1e-5, w
        assert got["ssim"].shape == (3, len(w), 3)


def test_pytorch_msssim_shim_and_image_eval():
    from harp_amd import ops
    from harp_amd.pytorch_msssim import MS_SSIM, ms_ssim
    from harp_amd.utils import eval_util as E
    X, Y = _images("rendered", 5, 176, 176, seed=13)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    m = ops.image_metrics(Xd, Yd, channels_last=False)["ms_ssim"]
    v = MS_SSIM(data_range=1, size_average=True, channel=3)(Xd, Yd)
    assert v.dim() == 0 and torch.equal(v, m.mean())
    assert torch.equal(ms_ssim(Xd, Yd, data_range=1, size_average=False), m)
    with pytest.raises(RuntimeError, match="forward-only"):
        MS_SSIM(data_range=1, channel=3)(Xd.clone().requires_grad_(), Yd)
    with pytest.raises(AssertionError):
        ms_ssim(Xd[..., :160], Yd[..., :160], data_range=1)
    Xh, Yh = X.permute(0, 2, 3, 1).to(DEV), Y.permute(0, 2, 3, 1).to(DEV)
    mask = (torch.rand(5, 176, 176) > 0.5).float().to(DEV)
    st = E.image_eval({"ref_image": [Xh[:2], Xh[2:]], "pred_image": [Yh[:2], Yh[2:]], "ref_mask": [mask], "pred_mask": [mask]})
    assert isinstance(float(st["MS_SSIM"]), float) and st["LPIPS"] is None
    assert abs(float(st["MS_SSIM"]) - R.ms_ssim(X, Y)["ms_ssim"].mean().item()) <= 1e-5
    st_cpu = E.image_eval({"ref_image": [Xh.cpu()], "pred_image": [Yh.cpu()], "ref_mask": [mask.cpu()], "pred_mask": [mask.cpu()]}, device=DEV)
    assert abs(float(st_cpu["MS_SSIM"]) - float(st["MS_SSIM"])) <= 1e-7
    assert np.isclose(float(E.ms_ssim_diff(Xh, Yh)), float(st["MS_SSIM"]), rtol=0, atol=1e-7)
