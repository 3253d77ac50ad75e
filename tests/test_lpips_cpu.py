"""CPU checks of LPIPS v0.1 / AlexNet: the float64 restatement (tests/_lpips_ref.py) against an nn.Sequential in torchvision's AlexNet
layout, the two weight layouts of harp_amd.lpips, its errors, the workspace formula of harp_lpips_alex_ws_bytes, and that nothing runs on
CPU tensors (no device needed)."""
import pytest
import torch
import torch.nn.functional as F

from tests import _lpips_ref as R


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def _alexnet_features(sd):
    nn = torch.nn
    seq = nn.Sequential(nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(), nn.MaxPool2d(3, 2), nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(), nn.MaxPool2d(3, 2),
                        nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(), nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(), nn.Conv2d(256, 256, 3, padding=1),
                        nn.ReLU()).double()
    with torch.no_grad():
        for k, ix in zip(R.CONV_KEYS, (0, 3, 6, 8, 10)):
            seq[ix].weight.copy_(sd[k + ".weight"])
            seq[ix].bias.copy_(sd[k + ".bias"])
    return seq


@pytest.mark.parametrize("size", [(64, 64), (31, 45)])
def test_restatement_matches_torchvision_layout(size):
    from harp_amd.lpips import random_alex_weights
    sd = random_alex_weights(1)
    g = torch.Generator().manual_seed(0)
    X, Y = torch.rand(2, 3, *size, generator=g, dtype=torch.float64), torch.rand(2, 3, *size, generator=g, dtype=torch.float64)
    seq = _alexnet_features(sd)
    shift, scale = torch.tensor([-0.030, -0.088, -0.188]).double().view(1, 3, 1, 1), torch.tensor([0.458, 0.448, 0.450]).double().view(1, 3, 1, 1)

    def taps(x):
        out, h = [], (x - shift) / scale
        for ix, layer in enumerate(seq):
            h = layer(h)
            if ix in (1, 4, 7, 9, 11):
                out.append(h)
        return out
    total = 0
    for k, (a, b) in enumerate(zip(taps(X), taps(Y))):
        na = a / (torch.sqrt(torch.sum(a ** 2, 1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt(torch.sum(b ** 2, 1, keepdim=True)) + 1e-10)
        d = F.conv2d((na - nb) ** 2, sd[f"lin{k}.model.1.weight"].double()).mean((2, 3)).view(-1)
        total = total + d
        assert torch.allclose(R.lpips(X, Y, sd)["taps"][:, k], d, rtol=1e-12, atol=1e-15)
    assert torch.allclose(R.lpips(X, Y, sd)["total"], total, rtol=1e-12)
    for f in R.features(X, sd):
        assert (f > 0).any()
    assert torch.equal(R.lpips(X, X.clone(), sd)["total"], torch.zeros(2, dtype=torch.float64))


def test_two_weight_layouts_load_the_same(tmp_path):
    from harp_amd.lpips import LPIPS, random_alex_weights
    sd = random_alex_weights(2)
    tv = {f"features.{k.split('.')[2]}.{k.split('.')[3]}": v for k, v in sd.items() if k.startswith("net.")}
    tv["classifier.1.weight"] = torch.zeros(8, 8)                      # ignored
    head = {k: v for k, v in sd.items() if k.startswith("lin")}
    combined = dict(sd, **{"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "scaling_layer.scale": torch.ones(1, 3, 1, 1)})
    for name, obj in (("tv.pth", tv), ("head.pth", head), ("lpips.pth", combined)):
        torch.save(obj, tmp_path / name)
    a = LPIPS(pnet_path=str(tmp_path / "tv.pth"), model_path=str(tmp_path / "head.pth"))
    b = LPIPS(weights=str(tmp_path / "lpips.pth"))
    c = LPIPS(weights=(str(tmp_path / "tv.pth"), str(tmp_path / "head.pth")))
    d = LPIPS(weights=combined)
    for m in (a, b, c, d):
        got = m.state_dict()
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
        assert not any(p.requires_grad for p in m.parameters()) and not m.training


def test_wrong_shape_or_key_is_named(tmp_path):
    from harp_amd.lpips import LPIPS, random_alex_weights
    sd = random_alex_weights(3)
    bad = dict(sd)
    bad["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"net\.slice2\.3\.weight"):
        LPIPS(weights=bad)
    tv = {f"features.{k.split('.')[2]}.{k.split('.')[3]}": v for k, v in sd.items() if k.startswith("net.")}
    head = {k: v for k, v in sd.items() if k.startswith("lin")}
    tv["features.10.bias"] = torch.zeros(255)
    with pytest.raises(ValueError, match=r"features\.10\.bias"):
        LPIPS(weights=(tv, head))
    del head["lin3.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        LPIPS(pnet_path=tv, model_path=head)


def test_missing_weights_and_unsupported_options(tmp_path):
    from harp_amd.lpips import LPIPS
    with pytest.raises(RuntimeError, match="alexnet.*lin"):
        LPIPS()
    with pytest.raises(RuntimeError, match="not found"):
        LPIPS(weights=str(tmp_path / "nope.pth"))
    with pytest.raises(RuntimeError, match="not found"):
        LPIPS(pnet_path=str(tmp_path / "a.pth"), model_path=str(tmp_path / "b.pth"))
    for kw in (dict(net="vgg"), dict(net="squeeze"), dict(version="0.0"), dict(spatial=True)):
        with pytest.raises(NotImplementedError):
            LPIPS(weights="random", **kw)


def test_cpu_tensors_raise(lib):
    from harp_amd import ops
    from harp_amd.lpips import LPIPS
    m = LPIPS(weights="random")
    x = torch.rand(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lpips_alex(x, x, torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lpips_alex_pack([(c.weight, c.bias) for c in m.convs()], [m.lin0.model[1].weight] * 5, "cpu")


def test_image_eval_without_lpips_fn_stays_none():
    from harp_amd.utils.eval_util import image_eval, lpips_diff
    g = torch.Generator().manual_seed(4)
    ev = {"ref_image": [torch.rand(2, 40, 40, 3, generator=g)], "pred_image": [torch.rand(2, 40, 40, 3, generator=g)],
          "ref_mask": [(torch.rand(2, 40, 40, generator=g) > 0.5).float()], "pred_mask": [(torch.rand(2, 40, 40, generator=g) > 0.5).float()]}
    stat = image_eval(ev)
    assert list(stat) == ["Silhouette IoU", "L1", "LPIPS", "MS_SSIM"] and stat["LPIPS"] is None and stat["MS_SSIM"] is None
    with pytest.raises(ValueError, match="lpips_fn"):
        lpips_diff(ev["ref_image"][0], ev["pred_image"][0])


@pytest.mark.parametrize("N,H,W", [(1, 31, 31), (64, 512, 512), (3, 257, 193), (2, 300, 300), (1, 34, 1000)])
def test_ws_bytes_formula(lib, N, H, W):
    A = lambda b: (b + 255) // 256 * 256                  # noqa: E731
    h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    P = 2 * N
    t = [-(-h1 * w1 // 64), -(-h2 * w2 // 64)] + [-(-h3 * w3 // 64)] * 3
    want = (A(256 * P * h1 * w1) + A(256 * P * h2 * w2) + A(768 * P * h2 * w2) + A(768 * P * h3 * w3) + A(1536 * P * h3 * w3)
            + 2 * A(1024 * P * h3 * w3) + sum(A(4 * N * tk) for tk in t))
    assert lib.harp_lpips_alex_ws_bytes(N, H, W) == want
    assert lib.harp_lpips_alex_ws_bytes(N, 30, W) == 0 and lib.harp_lpips_alex_ws_bytes(0, H, W) == 0
    assert lib.harp_lpips_alex_ws_bytes(65536, H, W) == 0
    assert h3 >= 1 and w3 >= 1


def test_tap_sides_match_torch():
    """the tap sides at 512 px (127, 63, 31, 31, 31) and the 31-px minimum (7, 3, 1), from torch's own layers"""
    from harp_amd.lpips import random_alex_weights
    sd = random_alex_weights(0)
    assert [f.shape[-1] for f in R.features(torch.rand(1, 3, 512, 512, dtype=torch.float64), sd)] == [127, 63, 31, 31, 31]
    assert [f.shape[-1] for f in R.features(torch.rand(1, 3, 31, 31, dtype=torch.float64), sd)] == [7, 3, 1, 1, 1]
    with pytest.raises(RuntimeError):
        R.features(torch.rand(1, 3, 30, 30, dtype=torch.float64), sd)


def test_raw_abi_rejects_without_device(lib):
    assert lib.harp_lpips_alex(None, None, None, 0, 0, 0, 0, 1, 64, 64, 0, None, None, None) == 1       # HARP_ERR_ARG, no launch
    assert lib.harp_lpips_alex_net_bytes() % 256 == 0 and lib.harp_lpips_alex_net_bytes() > 0
