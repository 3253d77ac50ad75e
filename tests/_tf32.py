"""The reference's own convolution arithmetic, emulated on the CPU: torch 1.11 + cuDNN with `torch.backends.cudnn.allow_tf32` on (its
default) runs the VGG16 convolutions, forward and data gradient, with both operands rounded to TF32 (float32 with a 10-bit stored
mantissa, round to nearest even) and float32 accumulation.  Here both operands are rounded to TF32 and the convolution runs in float64;
ReLU, max pool and the L1 run in float64.  With tf32=False the same stack is exact float64: the two together say what the reference's
hardware makes of an input, the yardstick of harp_conv3x3's single-pass f16 mode (precision 2)."""
import torch
import torch.nn.functional as F

from harp_amd.model.vgg import _CONVS, _SLICES


def tf32_round(x):
    """x (any float dtype) -> float64 holding float32(x) with its mantissa rounded to 10 bits, ties to even, on the bit pattern"""
    b = x.detach().float().contiguous().view(torch.int32).long() & 0xFFFFFFFF
    b = (b + 0xFFF + ((b >> 13) & 1)) & 0xFFFFE000
    b = torch.where(b >= 1 << 31, b - (1 << 32), b).to(torch.int32)
    return b.view(torch.float32).double()


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, tf32):
        ctx.save_for_backward(w)
        ctx.tf32 = tf32
        r = tf32_round if tf32 else (lambda t: t)
        return F.conv2d(r(x), r(w), b, padding=1)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        r = tf32_round if ctx.tf32 else (lambda t: t)
        return F.conv_transpose2d(r(g), r(w), padding=1), None, None, None


def conv(x, w, b=None, tf32=True):
    """3x3 / pad 1 convolution in float64, operands rounded to TF32 forward and in the data gradient (tf32=False: exact)"""
    return _Conv.apply(x, w, b, tf32)


def filters_of(vgg):
    """{features index: (weight, bias)} of a harp_amd.model.vgg.Vgg16Features, float64"""
    sd = vgg.state_dict()
    slice_of = {ix: n for n, (lo, hi) in enumerate(_SLICES, start=1) for ix in range(lo, hi)}
    return {ix: (sd[f"slice{slice_of[ix]}.{ix}.weight"].double(), sd[f"slice{slice_of[ix]}.{ix}.bias"].double()) for ix in _CONVS}


def taps(filters, x, tf32=True):
    """the four tap activations relu1_2 ... relu4_3 of x (N,3,H,W) float64"""
    out, h = [], x
    for lo, hi in _SLICES:
        for ix in range(lo, hi):
            if ix in _CONVS:
                h = conv(h, *filters[ix], tf32=tf32)
            elif ix in (4, 9, 16):
                h = F.max_pool2d(h, 2, 2)
            else:
                h = F.relu(h)
        out.append(h)
    return out


def rows(filters, layers_weights, x, tf32=True):
    """`Vgg16Features.forward`: the flattened input and the four flattened taps, scaled by layers_weights"""
    lw = layers_weights
    return torch.cat([lw[0] * x.flatten(1)] + [w * t.flatten(1) for w, t in zip(lw[1:], taps(filters, x, tf32))], 1)
