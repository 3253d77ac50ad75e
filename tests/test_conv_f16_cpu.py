"""CPU checks for the single-pass f16 mode of the perceptual term (harp_conv3x3 precision 2): the ctypes mirrors of harp_conv3x3_args and
harp_vgg16 against the C header, the mode constants, and the TF32-emulating float64 VGG stack the GPU tests measure against."""
import ctypes
import os
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_and_vgg16_structs_match_c(tmp_path):
    from harp_amd import _lib
    from harp_amd.model import conv_hip as C
    fields = [("harp_conv3x3_args", f) for f in ("in", "filters", "gate", "N", "precision", "epilogue", "in_channels", "tap_scale", "tile_list",
                                                 "max_tiles", "in_alt", "out_valid", "tile_origin", "out_valid_origin", "tile_pitch",
                                                 "tile_side", "out_valid_cell", "in_amax", "in_exp")]
    fields += [("harp_vgg16", f) for f in ("filters", "filters_t", "bias", "w0t", "layer_w", "precision")]
    body = ", ".join(["sizeof(harp_conv3x3_args)", "sizeof(harp_vgg16)", "HARP_CONV_F32", "HARP_CONV_BF16X3", "HARP_CONV_F16"] +
                     [f"offsetof({s}, {f})" for s, f in fields])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%s\\n", %s); return 0;}\n'
                   % (" ".join(["%zu"] * 2 + ["%d"] * 3 + ["%zu"] * len(fields)), body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    mirror = {"harp_conv3x3_args": _lib.Conv3x3Args, "harp_vgg16": _lib.Vgg16}
    want = [ctypes.sizeof(_lib.Conv3x3Args), ctypes.sizeof(_lib.Vgg16), C.F32, C.BF16X3, C.F16]
    want += [getattr(mirror[s], "in_" if f == "in" else f).offset for s, f in fields]
    assert got == want, (got, want)


def test_tf32_rounding_reproduces_known_bit_patterns():
    from tests._tf32 import tf32_round

    def bits(v):
        return int(torch.tensor([v], dtype=torch.float64).float().view(torch.int32).item()) & 0xFFFFFFFF

    cases = [
        (1.0, 0x3F800000),
        (1.0 + 2.0 ** -10, 0x3F802000),                  # representable: 10 stored bits
        (1.0 + 2.0 ** -11, 0x3F800000),                  # tie -> even (down)
        (1.0 + 3 * 2.0 ** -11, 0x3F804000),              # tie -> even (up)
        (1.0 + 2.0 ** -11 + 2.0 ** -20, 0x3F802000),     # above the tie -> up
        (-(1.0 + 2.0 ** -11 + 2.0 ** -20), 0xBF802000),  # sign kept
        (3.14159265, 0x40490000),                        # 0x40490FDB -> 0x40490000
        (2.0 ** -130 + 2.0 ** -143, 0x00080000),        # subnormal float32 (2^-149 units): the same bit rule
        (1.9999999, 0x40000000),                         # carries into the exponent
        (0.0, 0x00000000),
    ]
    for v, want in cases:
        got = bits(tf32_round(torch.tensor([v], dtype=torch.float64)).item())
        assert got == want, (v, hex(got), hex(want))
    x = torch.randn(10000, dtype=torch.float64)
    r = tf32_round(x)
    assert ((r.float().view(torch.int32) & 0x1FFF) == 0).all()
    assert ((r - x).abs() <= 2.0 ** -11 * x.abs() * (1 + 1e-6)).all()


def test_emulated_stack_is_the_module_in_float64():
    """with rounding off, the emulated stack is harp_amd.model.vgg.Vgg16Features in float64 (rows and input gradient)"""
    from harp_amd.model.vgg import Vgg16Features
    from tests import _tf32
    LW = [1, 1 / 16, 1 / 8, 1 / 4, 1]
    vgg = Vgg16Features(layers_weights=LW, weights="random", seed=4)
    vgg64 = Vgg16Features(layers_weights=LW, weights=vgg.state_dict()).double()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, 16, 16, generator=g, dtype=torch.float64).requires_grad_(True)
    R = torch.randn(1, vgg64(x.detach()).shape[1], generator=g, dtype=torch.float64)
    want = vgg64(x)
    (gw,) = torch.autograd.grad((want * R).sum(), x)
    got = _tf32.rows(_tf32.filters_of(vgg), LW, x, tf32=False)
    (gg,) = torch.autograd.grad((got * R).sum(), x)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-14) and torch.allclose(gg, gw, rtol=1e-10, atol=1e-14)
    # and rounding on moves it by the TF32 class (2^-11 per operand), not more
    t = _tf32.rows(_tf32.filters_of(vgg), LW, x.detach(), tf32=True)
    e = ((t - want).abs().max() / want.abs().max()).item()
    assert 1e-5 < e < 5e-3, e
