"""CPU checks of the post-fit evaluation metrics: the float64 restatement of pytorch_msssim's MS-SSIM (tests/_msssim_ref.py) on cases
with known answers, the workspace formula of harp_image_metrics_ws_bytes, and the argument checks of harp_image_metrics / ops.image_metrics
/ harp_amd.pytorch_msssim (all before any launch: no device needed)."""
import ctypes
import math

import pytest
import torch

from tests import _msssim_ref as R

C1, C2 = 0.01 ** 2, 0.03 ** 2


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def test_identical_pair_is_exactly_one():
    X = torch.rand(2, 3, 176, 201, generator=torch.Generator().manual_seed(0))
    r = R.ms_ssim(X, X.clone())
    assert torch.equal(r["ms_ssim"], torch.ones(2, dtype=torch.float64))
    assert torch.equal(r["ssim"], torch.ones_like(r["ssim"])) and torch.equal(r["cs"], torch.ones_like(r["cs"]))


@pytest.mark.parametrize("S", [512, 448])
@pytest.mark.parametrize("a,b", [(0.4, 0.6), (0.3, 0.45)])
def test_constant_images_closed_form(S, a, b):
    """every level of 512 / 448 is even, so the pooled images stay exactly constant: cs = 1 and ssim_4 = the luminance term.  (Up to
    the window's float32 taps summing to 1 - 3.1e-8, which leaves sigma^2 = c^2 (1 - S^4) != 0: cs_l = 1 - (a-b)^2 6.8e-5 here.)"""
    X = torch.full((1, 3, S, S), a, dtype=torch.float64)
    Y = torch.full((1, 3, S, S), b, dtype=torch.float64)
    r = R.ms_ssim(X, Y)
    want = ((2 * a * b + C1) / (a * a + b * b + C1)) ** 0.1333
    assert abs(r["ms_ssim"].item() - want) < 1e-5, (r["ms_ssim"].item(), want)
    assert (r["cs"] - 1).abs().max() < 1e-5


def test_anticorrelated_pair_is_zero():
    X = torch.rand(3, 3, 170, 190, generator=torch.Generator().manual_seed(1))
    r = R.ms_ssim(X, 1 - X)
    assert torch.equal(r["ms_ssim"], torch.zeros(3, dtype=torch.float64))
    assert (r["cs"][:, 0] < -0.9).all()                       # relu(cs_0) = 0 zeroes the product


@pytest.mark.parametrize("s", [161, 176, 333, 448, 512, 1001])
def test_pooled_sizes(s):
    x = torch.zeros(1, 1, s, s + 1)
    p = R.pool(x)
    assert p.shape[2] == (s // 2 + 1 if s % 2 else s // 2) == R.pooled_size(s)
    assert p.shape[3] == R.pooled_size(s + 1)
    # count_include_pad: an odd side averages a zero row into the first output row
    ones = R.pool(torch.ones(1, 1, 5, 4, dtype=torch.float64))
    assert torch.equal(ones[0, 0, :, 0], torch.tensor([0.5, 1.0, 1.0], dtype=torch.float64))


def _ws_formula(N, H, W):
    a256 = lambda b: (b + 255) // 256 * 256
    hs, ws = [H], [W]
    for _ in range(4):
        hs.append((hs[-1] + 1) // 2)
        ws.append((ws[-1] + 1) // 2)
    tiles = [math.ceil((h - 10) / 32) * math.ceil((w - 10) / 32) for h, w in zip(hs, ws)]
    return sum(2 * a256(12 * N * hs[l] * ws[l]) for l in range(1, 5)) + sum(a256(64 * N * tiles[l]) for l in range(5))


def test_ws_bytes_formula(lib):
    for N, H, W in [(1, 161, 161), (7, 176, 333), (64, 512, 512), (3, 1080, 1920), (256, 512, 512)]:
        assert lib.harp_image_metrics_ws_bytes(N, H, W) == _ws_formula(N, H, W), (N, H, W)
    for N, H, W in [(0, 512, 512), (1, 160, 512), (1, 512, 160), (2, 96, 96)]:
        assert lib.harp_image_metrics_ws_bytes(N, H, W) == 0


def test_bad_arguments_return_err_arg_without_launch(lib):
    w5 = (ctypes.c_float * 5)(*R.WEIGHTS)
    fake = 1 << 20                                             # never dereferenced: every call below must fail its argument check first
    def call(ref=fake, pred=fake, rm=None, pm=None, N=1, C=3, H=176, W=176, w=w5, nl=5, ws=fake, out=fake):
        return lib.harp_image_metrics(ref, pred, rm, pm, 0, 0, 0, 0, N, C, H, W, 1.0, w, nl, 0.01, 0.03, 1.5, ws, out, None)
    assert call(ref=None) == 1 and call(pred=None) == 1 and call(ws=None) == 1 and call(out=None) == 1
    assert call(H=160) == 1 and call(W=160) == 1 and call(H=96, W=96) == 1
    assert call(nl=0) == 1 and call(nl=6) == 1 and call(w=None) == 1
    assert call(C=0) == 1 and call(C=4) == 1 and call(N=0) == 1
    assert call(rm=fake) == 1                                  # one mask without the other


def test_entry_points_refuse_cpu_window_and_graph():
    from harp_amd import ops, pytorch_msssim
    X, Y = torch.rand(1, 3, 176, 176), torch.rand(1, 3, 176, 176)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.image_metrics(X, Y, channels_last=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pytorch_msssim.ms_ssim(X, Y, data_range=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pytorch_msssim.MS_SSIM(data_range=1, channel=3)(X, Y)
    with pytest.raises(ValueError, match="win_size"):
        pytorch_msssim.ms_ssim(X, Y, win_size=7)
    with pytest.raises(ValueError, match="win_size"):
        pytorch_msssim.MS_SSIM(data_range=1, win_size=9)
    g = X.clone().requires_grad_()
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.image_metrics(g, Y, channels_last=False)
    with pytest.raises(RuntimeError, match="forward-only"):
        pytorch_msssim.MS_SSIM(data_range=1, channel=3)(g, Y)


def test_image_eval_on_cpu_unchanged():
    """CPU tensors and no device: image_eval behaves as before (MS_SSIM None, no kernel involved)"""
    from harp_amd.utils import eval_util as E
    a, b = torch.rand(2, 176, 176, 3), torch.rand(2, 176, 176, 3)
    m = (torch.rand(2, 176, 176) > 0.5).float()
    st = E.image_eval({"ref_image": [a], "pred_image": [b], "ref_mask": [m], "pred_mask": [m]})
    assert st["MS_SSIM"] is None and st["LPIPS"] is None and abs(float(st["Silhouette IoU"]) - 1.0) < 1e-7


def test_load_gt_vert(tmp_path):
    from harp_amd.utils import eval_util as E
    v = torch.rand(778, 3).double().numpy() * 100
    import numpy as np
    np.savetxt(tmp_path / "503_manov.xyz", v)
    got = E.load_gt_vert(torch.tensor([2]), str(tmp_path), dataset="synthetic", start_from_one=True, idx_offset=500)
    assert np.allclose(got, v / 1000.0)
