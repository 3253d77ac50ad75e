"""-m gpu: LPIPS v0.1 / AlexNet (csrc/lpips.hip, ops.lpips_alex, harp_amd.lpips.LPIPS) against the float64 restatement
(tests/_lpips_ref.py) on seeded weights: per-image totals and per-tap values, NHWC and NCHW, normalize on and off, off-grid sizes down to the
31-px minimum; the exact cases (identical inputs, repeated calls, a batch against single calls); the raw ABI's argument checks; and the
real weights when HARP_LPIPS_WEIGHTS names them."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from tests import _lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL, RTOL = 1e-7, 1e-5                # measured worst on the MI355X: 9.9e-9 (31² case), the others <= 3.5e-9
WORST = {}


def _images(kind, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        X = torch.rand(N, 3, H, W, generator=g)
        Y = (X + 0.3 * torch.rand(N, 3, H, W, generator=g)).clamp(0, 1)
    else:                                                  # "rendered": flat white background, a textured blob shifted between the two
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        tex = F.interpolate(torch.rand(N, 3, 24, 24, generator=g), size=(H, W), mode="bilinear", align_corners=False) * 0.6 + 0.2

        def blob(cy, cx):
            return (((yy - cy) / (0.3 * H)) ** 2 + ((xx - cx) / (0.25 * W)) ** 2 < 1).float()
        mx, my = blob(0.5 * H, 0.5 * W), blob(0.53 * H, 0.47 * W)
        X = torch.ones(N, 3, H, W) * (1 - mx) + tex * mx
        Y = torch.ones(N, 3, H, W) * (1 - my) + (tex * 0.9 + 0.02 * torch.rand(N, 3, H, W, generator=g)) * my
    return X.float().contiguous(), Y.float().contiguous()


@pytest.fixture(scope="module")
def model():
    from harp_amd.lpips import LPIPS
    return LPIPS(weights="random", seed=3).to(DEV)


def _run(m, X, Y, layout, normalize):
    from harp_amd import ops
    net = m._packed(torch.device(DEV))
    if layout == "nhwc":
        return ops.lpips_alex(X.permute(0, 2, 3, 1).contiguous().to(DEV), Y.permute(0, 2, 3, 1).contiguous().to(DEV), net, True, normalize)
    return ops.lpips_alex(X.to(DEV), Y.to(DEV), net, False, normalize)


def _check(got, want, case):
    got = got.double().cpu()
    ref = torch.cat([want["total"][:, None], want["taps"]], 1)
    err = (got - ref).abs()
    bound = ATOL + RTOL * ref.abs()
    rel = (err / (ATOL + RTOL * ref.abs())).max().item()
    WORST[case] = (err.max().item(), rel)
    print(f"[lpips] {case}: worst |d| {err.max().item():.2e} ({rel:.2f} of the bound), totals {ref[:, 0].tolist()[:3]}")
    assert (err <= bound).all(), (case, err.max().item(), got, ref)


CASES = [((512, 512), 2, "random", "nhwc", False), ((512, 512), 2, "rendered", "nchw", True), ((300, 300), 3, "rendered", "nhwc", False),
         ((257, 193), 2, "random", "nchw", False), ((31, 31), 3, "random", "nhwc", True), ((193, 257), 2, "rendered", "nhwc", True),
         ((31, 47), 2, "rendered", "nchw", False)]


@pytest.mark.parametrize("size,N,kind,layout,normalize", CASES)
def test_against_float64_restatement(model, size, N, kind, layout, normalize):
    H, W = size
    X, Y = _images(kind, N, H, W, seed=H + 7 * W + N)
    got = _run(model, X, Y, layout, normalize)
    _check(got, R.lpips(X, Y, model.state_dict(), normalize=normalize), f"{H}x{W} {kind} {layout} normalize={normalize}")


def test_every_tap_is_alive(model):
    """the comparison is not vacuous: on the seeded weights every tap has non-zero features and a non-zero distance"""
    X, Y = _images("rendered", 2, 128, 128, seed=5)
    sd = model.state_dict()
    for k, f in enumerate(R.features(X.double(), sd)):
        assert (f > 0).double().mean() > 0.05, k
    got = _run(model, X, Y, "nchw", False).cpu()
    assert (got[:, 1:] > 1e-4).all(), got


def test_identical_inputs_give_exactly_zero(model):
    X, _ = _images("random", 3, 200, 160, seed=9)
    got = _run(model, X, X.clone(), "nhwc", False).cpu()
    assert torch.equal(got, torch.zeros_like(got)), got


def test_repeatable_and_batch_equals_singles(model):
    from harp_amd import ops
    X, Y = _images("rendered", 64, 64, 64, seed=11)
    Xd, Yd = X.permute(0, 2, 3, 1).contiguous().to(DEV), Y.permute(0, 2, 3, 1).contiguous().to(DEV)
    net = model._packed(torch.device(DEV))
    a, b = ops.lpips_alex(Xd, Yd, net), ops.lpips_alex(Xd, Yd, net)
    assert torch.equal(a, b)
    singles = torch.cat([ops.lpips_alex(Xd[i:i + 1], Yd[i:i + 1], net) for i in range(64)])
    assert torch.equal(a, singles)


def test_module_forward_and_retperlayer(model):
    X, Y = _images("random", 2, 96, 80, seed=12)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    with torch.no_grad():
        v = model(Xd, Yd)
        v2, per = model(Xd, Yd, retPerLayer=True)
    assert v.shape == (2, 1, 1, 1) and torch.equal(v, v2) and len(per) == 5 and all(p.shape == (2, 1, 1, 1) for p in per)
    want = R.lpips(X, Y, model.state_dict())
    assert (v.view(-1).double().cpu() - want["total"]).abs().max() <= ATOL + RTOL * want["total"].abs().max()
    # weights written in place are repacked
    with torch.no_grad():
        model.lin0.model[1].weight.mul_(2.0)
    try:
        v3, per3 = model(Xd, Yd, retPerLayer=True)
        assert torch.allclose(per3[0], 2 * per[0], rtol=1e-6, atol=0) and torch.equal(per3[1], per[1])
    finally:
        with torch.no_grad():
            model.lin0.model[1].weight.mul_(0.5)


def test_raw_abi_argument_checks(model):
    from harp_amd import _lib
    L = _lib.lib()
    net = model._packed(torch.device(DEV))
    img = torch.rand(1, 64, 64, 3, device=DEV)
    ws = torch.empty(max(L.harp_lpips_alex_ws_bytes(1, 64, 64), 256), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 6), -1.0, device=DEV)
    s = _lib.stream()
    args = lambda **kw: dict(dict(net=net.data_ptr(), ref=img.data_ptr(), pred=img.data_ptr(), N=1, H=64, W=64, ws=ws.data_ptr(),  # noqa: E731
                                  out=out.data_ptr()), **kw)

    def call(a):
        return L.harp_lpips_alex(a["net"], a["ref"], a["pred"], 64 * 64 * 3, 1, 64 * 3, 3, a["N"], a["H"], a["W"], 0, a["ws"], a["out"], s)
    assert call(args()) == 0
    for bad in (dict(net=None), dict(ref=None), dict(pred=None), dict(ws=None), dict(out=None), dict(H=30), dict(W=30), dict(N=0),
                dict(N=65536), dict(net=net.data_ptr() + 16), dict(ws=ws.data_ptr() + 16), dict(H=1 << 20, W=1 << 20)):
        assert call(args(**bad)) == 1, bad
    assert L.harp_lpips_alex_ws_bytes(1, 30, 64) == 0 and L.harp_lpips_alex_ws_bytes(0, 64, 64) == 0
    w = (ctypes.c_void_p * 5)()
    assert L.harp_lpips_alex_pack(w, w, w, net.data_ptr(), s) == 1
    torch.cuda.synchronize()


def test_real_weights_when_present():
    """HARP_LPIPS_WEIGHTS=<alexnet state dict>:<lpips v0.1 alex head> (or one lpips.LPIPS state dict) checks the real weights the same
    way; there is no network in the build image, so by default this skips"""
    spec = os.environ.get("HARP_LPIPS_WEIGHTS")
    paths = spec.split(os.pathsep) if spec else []
    if not (paths and all(os.path.exists(p) for p in paths)):
        pytest.skip("HARP_LPIPS_WEIGHTS does not name the weight files")
    from harp_amd.lpips import LPIPS
    m = LPIPS(weights=paths[0] if len(paths) == 1 else tuple(paths)).to(DEV)
    X, Y = _images("rendered", 2, 256, 256, seed=13)
    _check(_run(m, X, Y, "nhwc", False), R.lpips(X, Y, m.state_dict()), "real weights")
