"""Float64 restatement of pytorch_msssim 0.2.1's ms_ssim (the package the reference's utils/eval_util.py:4, 8, 56-60 imports; it is not
installed here), written from its algorithm: an 11-tap Gaussian window (float32 taps, as the package forms them), separable "valid"
filtering of X, Y, X*X, Y*Y, X*Y, per-level ssim / cs means over the valid map, avg_pool2d(2, padding=(H%2, W%2)) between levels, and
prod(relu(cs_0..L-2) ** w, relu(ssim_L-1) ** w_L-1) per (image, channel).  Everything after the taps runs in float64 on the CPU."""
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gauss_taps(win_size=11, sigma=1.5):
    """_fspecial_gauss_1d in float32 (the package builds its window in float32 and casts it to the input's dtype)"""
    coords = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _filter(x, taps):
    C = x.shape[1]
    w = taps.to(x.dtype).view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    x = F.conv2d(x, w, groups=C)                              # along W
    return F.conv2d(x, w.transpose(2, 3), groups=C)          # along H


def ssim_cs(X, Y, data_range=1.0, taps=None, K=(0.01, 0.03)):
    """-> (ssim, cs), each (N, C): the means of the two maps over the valid region"""
    taps = gauss_taps() if taps is None else taps
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = _filter(X, taps), _filter(Y, taps)
    s1 = _filter(X * X, taps) - mu1 * mu1
    s2 = _filter(Y * Y, taps) - mu2 * mu2
    s12 = _filter(X * Y, taps) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def pool(x):
    return F.avg_pool2d(x, kernel_size=2, padding=(x.shape[2] % 2, x.shape[3] % 2))


def pooled_size(s):
    return s // 2 if s % 2 == 0 else s // 2 + 1


def ms_ssim(X, Y, data_range=1.0, weights=WEIGHTS, sigma=1.5, K=(0.01, 0.03)):
    """X, Y (N,C,H,W) -> dict(ms_ssim (N,) = channel mean, ssim / cs (N, levels, C)), all float64"""
    X, Y = X.detach().cpu().double(), Y.detach().cpu().double()
    assert min(X.shape[-2:]) > 160
    taps = gauss_taps(11, sigma)
    ss, cs = [], []
    for lvl in range(len(weights)):
        s, c = ssim_cs(X, Y, data_range, taps, K)
        ss.append(s)
        cs.append(c)
        if lvl < len(weights) - 1:
            X, Y = pool(X), pool(Y)
    w = torch.tensor(weights, dtype=torch.float64).view(-1, 1, 1)
    stack = torch.stack([torch.relu(c) for c in cs[:-1]] + [torch.relu(ss[-1])], 0)
    val = torch.prod(stack ** w, 0)
    return {"ms_ssim": val.mean(1), "ssim": torch.stack(ss, 1), "cs": torch.stack(cs, 1)}
