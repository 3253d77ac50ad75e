"""Drop-in for the `lpips` package's LPIPS v0.1 with net='alex', the metric utils/eval_util.py:7, 51-53 builds and calls
(`lpips.LPIPS(net='alex').to('cuda')`, then `loss_fn(ref, pred)` on [0, 1] images without `normalize`).  A reference file changes its import
to `from harp_amd import lpips`; the network runs on csrc/lpips.hip (ops.lpips_alex), forward only, float32.

Supported: net='alex', version='0.1', lpips=True, spatial=False, NCHW float32 HIP tensors with both sides >= 31 px.  Anything else raises
(`NotImplementedError` for the other backbones, versions and spatial maps); there is no fallback to another implementation.

Weights.  Nothing can be downloaded, so they are always given, in one of two forms (a path or an already loaded state dict each):
  (a) pnet_path = torchvision's alexnet state dict (keys features.{0,3,6,8,10}.{weight,bias}; everything else, e.g. the classifier, is
      ignored) and model_path = the lpips v0.1 head file (keys lin{0..4}.model.1.weight, shape (1, C, 1, 1));
  (b) weights = one state dict of an lpips.LPIPS module (net.slice1.0.*, net.slice2.3.*, net.slice3.6.*, net.slice4.8.*, net.slice5.10.*,
      lin{k}.model.1.weight; its scaling_layer buffers are ignored — the constants are fixed).
  weights=(pnet, head) is form (a) as a pair; weights="random" gives seeded filters of the same layout (tests only).
These key layouts are written from memory of the lpips and torchvision sources; neither package is installed where this was written, so they
have not been checked against the packages themselves.  This module's own state dict uses layout (b)."""
import os

import torch

from . import ops

__all__ = ["LPIPS", "load_alex_weights", "random_alex_weights"]

_CONV_IDX = (0, 3, 6, 8, 10)                       # torchvision alexnet.features indices of the five convolutions
_SLICE = {0: 1, 3: 2, 6: 3, 8: 4, 10: 5}           # lpips' alexnet: slice k holds features[...] up to relu k
_CHANNELS = tuple(co for co, _, _ in ops.LPIPS_ALEX_CONVS)
FILES_NEEDED = ("torchvision's AlexNet state dict (alexnet-owt-7be5be79.pth: features.{0,3,6,8,10}.{weight,bias}) and the lpips v0.1 "
                "head (lpips/weights/v0.1/alex.pth: lin{0..4}.model.1.weight), or one state dict of an lpips.LPIPS(net='alex') module")


def _shapes():
    """own (layout b) key -> shape"""
    s = {}
    for k, ix in enumerate(_CONV_IDX):
        co, ci, ks = ops.LPIPS_ALEX_CONVS[k]
        s[f"net.slice{_SLICE[ix]}.{ix}.weight"] = (co, ci, ks, ks)
        s[f"net.slice{_SLICE[ix]}.{ix}.bias"] = (co,)
        s[f"lin{k}.model.1.weight"] = (1, co, 1, 1)
    return s


def _read(src, what):
    if isinstance(src, dict):
        return src
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        if not os.path.isfile(src):
            raise RuntimeError(f"LPIPS weight file {os.fsdecode(src)!r} ({what}) not found; LPIPS(net='alex') needs {FILES_NEEDED} "
                               "(nothing can be downloaded)")
        sd = torch.load(src, map_location="cpu")
        if not isinstance(sd, dict):
            raise ValueError(f"{os.fsdecode(src)!r} holds a {type(sd).__name__}, not a state dict")
        return sd
    raise TypeError(f"LPIPS weights ({what}): a path or a state dict, got {type(src).__name__}")


def load_alex_weights(weights=None, pnet_path=None, model_path=None):
    """The five convolutions and five head weights as a state dict in this module's layout (b), from layout (a) (pnet_path + model_path, or
    weights=(pnet, head)) or layout (b) (weights).  Missing keys and shape mismatches raise, naming the key."""
    if isinstance(weights, (tuple, list)):
        if len(weights) != 2:
            raise ValueError("weights as a pair: (torchvision alexnet state dict, lpips v0.1 head)")
        pnet_path, model_path, weights = weights[0], weights[1], None
    if weights is None and (pnet_path is None or model_path is None):
        raise RuntimeError(f"LPIPS(net='alex') needs pretrained weights: {FILES_NEEDED} (nothing can be downloaded; pass pnet_path= and "
                           "model_path=, or weights=)")
    want = _shapes()
    picked = {}
    if weights is not None:                                                  # layout (b)
        sd = _read(weights, "lpips.LPIPS state dict")
        for k in want:
            if k in sd:
                picked[k] = (k, sd[k])
    else:                                                                    # layout (a)
        pnet, head = _read(pnet_path, "torchvision alexnet"), _read(model_path, "lpips v0.1 head")
        for ix in _CONV_IDX:
            for p in ("weight", "bias"):
                if f"features.{ix}.{p}" in pnet:
                    picked[f"net.slice{_SLICE[ix]}.{ix}.{p}"] = (f"features.{ix}.{p}", pnet[f"features.{ix}.{p}"])
        for k in range(5):
            if f"lin{k}.model.1.weight" in head:
                picked[f"lin{k}.model.1.weight"] = (f"lin{k}.model.1.weight", head[f"lin{k}.model.1.weight"])
    missing = [k for k in want if k not in picked]
    if missing:
        raise KeyError(f"LPIPS weights lack {missing}")
    out = {}
    for k, shape in want.items():
        src_key, v = picked[k]
        if not torch.is_tensor(v) or tuple(v.shape) != shape:
            got = tuple(v.shape) if torch.is_tensor(v) else type(v).__name__
            raise ValueError(f"LPIPS weight {src_key!r} has shape {got}, want {shape}")
        out[k] = v.detach().to(torch.float32)
    return out


def random_alex_weights(seed=0):
    """seeded stand-ins in layout (b) (tests only): filters N(0, 2 / fan_in) so that the deep taps stay alive, small biases, non-negative
    head weights"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shape in _shapes().items():
        if k.startswith("lin"):
            out[k] = torch.rand(shape, generator=g) * 0.2
        elif k.endswith("weight"):
            out[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        else:
            out[k] = torch.randn(shape, generator=g) * 0.01
    return out


class _NetLin(torch.nn.Module):
    """lpips' NetLinLayer: Dropout (a no-op in eval mode) and a bias-free 1x1 convolution to one channel"""

    def __init__(self, c):
        super().__init__()
        self.model = torch.nn.Sequential(torch.nn.Dropout(), torch.nn.Conv2d(c, 1, 1, bias=False))


def _alex_slices():
    """torchvision alexnet.features[0:12] cut after each ReLU, as lpips' `alexnet` module holds it"""
    nn = torch.nn
    layers = {0: nn.Conv2d(3, 64, 11, 4, 2), 1: nn.ReLU(), 2: nn.MaxPool2d(3, 2), 3: nn.Conv2d(64, 192, 5, padding=2), 4: nn.ReLU(),
              5: nn.MaxPool2d(3, 2), 6: nn.Conv2d(192, 384, 3, padding=1), 7: nn.ReLU(), 8: nn.Conv2d(384, 256, 3, padding=1), 9: nn.ReLU(),
              10: nn.Conv2d(256, 256, 3, padding=1), 11: nn.ReLU()}
    m = nn.Module()
    for s, (lo, hi) in enumerate(((0, 2), (2, 5), (5, 8), (8, 10), (10, 12)), start=1):
        seq = nn.Sequential()
        for ix in range(lo, hi):
            seq.add_module(str(ix), layers[ix])
        setattr(m, f"slice{s}", seq)
    return m


class LPIPS(torch.nn.Module):
    """lpips.LPIPS for net='alex', version='0.1' (the reference's metric).  forward(in0, in1, retPerLayer=False, normalize=False): NCHW
    float32 HIP tensors -> (N,1,1,1), or (value, [five (N,1,1,1) per-tap values]) with retPerLayer."""

    def __init__(self, pretrained=True, net="alex", version="0.1", lpips=True, spatial=False, pnet_rand=False, pnet_tune=False,
                 use_dropout=True, model_path=None, eval_mode=True, verbose=False, pnet_path=None, weights=None, seed=0):
        super().__init__()
        if net != "alex":
            raise NotImplementedError(f"only net='alex' is implemented (the reference's metric), got net={net!r}")
        if version != "0.1":
            raise NotImplementedError(f"only version='0.1' is implemented, got {version!r}")
        if spatial:
            raise NotImplementedError("spatial=True (per-pixel LPIPS maps) is not implemented")
        if not lpips or not pretrained or pnet_rand or pnet_tune:
            raise NotImplementedError("only the calibrated metric (lpips=True, pretrained, frozen backbone) is implemented")
        self.pnet_type, self.version, self.lpips, self.spatial = net, version, True, False
        self.net = _alex_slices()
        for k, c in enumerate(_CHANNELS):
            setattr(self, f"lin{k}", _NetLin(c))
        if isinstance(weights, str) and weights == "random":
            sd = random_alex_weights(seed)
        else:
            sd = load_alex_weights(weights, pnet_path=pnet_path, model_path=model_path)
        self.load_state_dict(sd)
        for p in self.parameters():
            p.requires_grad = False
        if eval_mode:
            self.eval()

    def convs(self):
        """the five Conv2d layers in features order"""
        return [getattr(getattr(self.net, f"slice{_SLICE[ix]}"), str(ix)) for ix in _CONV_IDX]

    def _packed(self, device):
        """the weights packed for csrc/lpips.hip on `device`, cached; repacked whenever a parameter was replaced or written in place
        (load_state_dict, .to(), an in-place edit: keyed on every parameter's storage and version counter)"""
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        cache = self.__dict__.get("_hip_cache")
        if cache is None or cache[0] != key:
            cache = self.__dict__["_hip_cache"] = (key, {})
        dev = str(device)
        if dev not in cache[1]:
            convs = [(m.weight, m.bias) for m in self.convs()]
            lins = [getattr(self, f"lin{k}").model[1].weight for k in range(5)]
            cache[1][dev] = ops.lpips_alex_pack(convs, lins, device)
        return cache[1][dev]

    def _apply(self, fn, *args, **kwargs):
        self.__dict__.pop("_hip_cache", None)             # new storage may reuse a freed pointer at version 0: repack regardless
        return super()._apply(fn, *args, **kwargs)

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        if not (torch.is_tensor(in0) and torch.is_tensor(in1)):
            raise TypeError("LPIPS takes tensors")
        if not (in0.is_cuda and in1.is_cuda):
            raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
        out = ops.lpips_alex(in0, in1, self._packed(in0.device), channels_last=False, normalize=normalize)
        N = out.shape[0]
        val = out[:, 0].reshape(N, 1, 1, 1)
        if retPerLayer:
            return val, [out[:, 1 + k].reshape(N, 1, 1, 1) for k in range(5)]
        return val
