"""Drop-in for the MS-SSIM half of pytorch_msssim 0.2.1 (requirements.txt:55), the package utils/eval_util.py:4 imports:
`ms_ssim` and `MS_SSIM` on NCHW float32 HIP tensors, computed by csrc/metrics.hip (ops.image_metrics).  A reference file only changes its
import to `from harp_amd.pytorch_msssim import ms_ssim, MS_SSIM`.

Supported: win_size 11 (the package default and the reference's setting), 1 to 5 level weights, 1 to 3 channels, forward only.  Anything
else raises — there is no fallback to another implementation."""
import torch

from . import ops

__all__ = ["ms_ssim", "MS_SSIM"]


def _check(X, Y, win_size, win):
    if win is not None:
        raise ValueError("a custom `win` is not supported: pass win_size=11 and win_sigma")
    if win_size != 11:
        raise ValueError(f"only win_size=11 is supported (the metrics kernel's window), got {win_size}")
    if not (torch.is_tensor(X) and torch.is_tensor(Y)):
        raise TypeError("ms_ssim takes tensors")
    ops.check_forward_only(X, Y)
    if not (X.is_cuda and Y.is_cuda):
        raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
    if X.dtype != torch.float32 or Y.dtype != torch.float32:
        raise TypeError(f"ms_ssim takes float32 tensors, got {X.dtype} / {Y.dtype}")
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d tensors, but got {tuple(X.shape)}")
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {tuple(X.shape)} and {tuple(Y.shape)}.")
    smaller_side = min(X.shape[-2:])
    assert smaller_side > (win_size - 1) * (2 ** 4), "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % (
        (win_size - 1) * (2 ** 4))


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None, K=(0.01, 0.03)):
    """pytorch_msssim.ms_ssim: X, Y (N,C,H,W) -> the mean over images and channels (size_average) or the (N,) channel means"""
    _check(X, Y, win_size, win)
    if weights is not None and torch.is_tensor(weights):
        weights = weights.detach().cpu().tolist()
    m = ops.image_metrics(X, Y, channels_last=False, data_range=data_range, weights=weights, win_sigma=win_sigma, K=K)["ms_ssim"]
    return m.mean() if size_average else m


class MS_SSIM(torch.nn.Module):
    """pytorch_msssim.MS_SSIM (as built at utils/eval_util.py:8: data_range=1, size_average=True, channel=3)"""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2, weights=None, K=(0.01, 0.03)):
        super().__init__()
        if win_size != 11:
            raise ValueError(f"only win_size=11 is supported (the metrics kernel's window), got {win_size}")
        if spatial_dims != 2:
            raise ValueError("only 2-D images are supported")
        self.win_size, self.win_sigma, self.channel = win_size, win_sigma, channel
        self.size_average, self.data_range, self.weights, self.K = size_average, data_range, weights, K

    def forward(self, X, Y):
        if X.dim() == 4 and X.shape[1] != self.channel:
            raise ValueError(f"MS_SSIM was built for {self.channel} channels, got {X.shape[1]}")
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win_size=self.win_size, win_sigma=self.win_sigma,
                       weights=self.weights, K=self.K)
