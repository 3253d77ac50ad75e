"""harp_conv3x3 (csrc/conv.hip) launch by launch through the raw C ABI against the float64 restatement of include/harp_hip.h
(tests/_conv_ref.py), on the cases of tests/_conv_cases.py: the full grid at 1 x 1 ... 23 x 37 (odd sizes, a one-pixel second tile), partly
populated input chunks, filters padded from 3 channels, per-frame tile lists of 16- and 8-pixel tiles on shifted grids that reach beyond the
image on all four sides, validity bitmaps of every cell size with and without `in_alt`, the un-pool routing with and without `out_valid`,
and every rule of the argument check — in all three precisions (the 8-pixel form has an LDS layout per precision).

Every output is prefilled with finite random sentinels.  Elements the header says a launch leaves alone must keep the prefill's BITS (`out`,
`pooled`, `g_tap`); the others are compared element by element, |got_i - ref_i| <= bound_i, with bound_i from the reference's A_i = sum |x||w|
+ |b| and K alone — derivations in tests/_conv_ref.py (U = 2^-24):
  mode 0  (K + 2) U A_i
  mode 1  2^-16 A_i + (3K + 2) U A_i     (the number of float32 roundings inside a 32x32x16 bf16 MFMA is not documented: the worst case, one
                                          per product term)
  mode 2  (2^-10 + 2^-22) A_i + (K + 2) U A_i + 2^-25 (2^-e sum|w| + sum|x|)
pooled: the largest of its window's four bounds (max is 1-Lipschitz); un-pool `+=`: + U |out_i|; g_tap: exactly +-tap_scale or 0 on the elements
the reference decides (|conv + b| and |out - target| above bound_i; at most 1 % are not, asserted on the CPU), one of the three values on
the rest; *loss: the owned pixels' share within `_conv_ref.loss_bound`.  Measured err / bound per case, group and precision, and the cases
each one-line mutation of conv.hip fails: docs/NOTEBOOK.md."""
import ctypes

import pytest
import torch

from tests import _conv_cases as C
from tests import _conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1
OUTPUTS = ("out", "pooled", "g_tap")


@pytest.fixture(scope="module")
def refs():
    """case and reference, once per case, shared by the three precisions, never modified"""
    built = {}
    yield built
    built.clear()


def get_ref(refs, name):
    if name not in refs:
        c = C.build(name)
        res = R.launch(c["a"])
        C.check(c, res)
        refs[name] = (c, res)
    return refs[name]


def fill_args(c, precision, keep):
    """c's arguments on the device as a _lib.Conv3x3Args; `keep` receives the device tensors by field name"""
    from harp_amd import _lib
    from harp_amd.model import conv_hip
    a = c["a"]
    s = _lib.Conv3x3Args()
    keep["filters"] = conv_hip.pack_filters(c["w_src"].to(DEV), precision, transpose=c["transpose"])
    for k in ("in_", "bias", "out", "pooled", "target", "target_row", "g_tap", "loss", "gate", "tile_list", "tile_count", "in_valid", "in_alt",
              "out_valid", "tile_origin", "in_valid_origin", "out_valid_origin"):
        if a[k] is not None:
            keep[k] = a[k].to(DEV).contiguous().clone()
    if precision == 2 and c["in_amax"] is not None:
        keep["in_amax"] = c["in_amax"].to(DEV)
    for k, t in keep.items():
        setattr(s, k, _lib.ptr(t))
    for k in ("N", "H", "W", "Cin", "Cout", "epilogue", "in_channels", "max_tiles", "in_valid_shift", "tile_pitch", "in_valid_pitch",
              "out_valid_pitch", "tile_side", "in_valid_cell", "out_valid_cell"):
        setattr(s, k, int(a[k]))
    s.precision, s.tap_scale, s.in_exp = precision, float(a["tap_scale"]), int(c["in_exp"]) if precision == 2 else 0
    return s


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_launch_against_the_float64_restatement(name, precision, refs):
    from harp_amd import _lib
    c, res = get_ref(refs, name)
    a = c["a"]
    keep = {}
    s = fill_args(c, precision, keep)
    rc = _lib.lib().harp_conv3x3(ctypes.byref(s), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)
    e = R.f16_exponent(c["in_amax"], c["in_exp"]) if precision == 2 else 0
    bd = R.bound(res, precision, e)
    bounds = {"out": R.unpool_bound(res, bd) if a["epilogue"] == R.UNPOOL else bd, "pooled": R.pooled_bound(bd) if a["pooled"] is not None else None}
    ratios = {}
    for k in OUTPUTS:
        if a[k] is None:
            continue
        got, written = keep[k].cpu(), res[k + "_written"]
        assert torch.isfinite(got).all(), (name, k)
        assert torch.equal(_bits(got)[~written], _bits(a[k])[~written]), (name, k, "an element the launch does not own changed")
        if k == "g_tap":
            und = R.tap_undecided(res, bd)
            dec = written & ~und
            assert torch.equal(got[dec], res[k][dec].float()), (name, "tap gradient on the decided elements")
            sc = float(a["tap_scale"])
            assert ((got == sc) | (got == -sc) | (got == 0))[written & und].all(), name
            ratios["g_tap undecided share"] = und.float().mean().item()
            continue
        err = (got.double() - res[k]).abs()
        assert (err[written & (bounds[k] == 0)] == 0).all(), (name, k, "an element whose operands are all zero")      # (no input, or padded filters)
        sel = written & (bounds[k] > 0)
        ratios[k] = (err / bounds[k])[sel].max().item() if sel.any() else 0.0
    if a["epilogue"] == R.RELU_TAP:
        lb = R.loss_bound(res, bd)
        ratios["loss"] = abs(float(keep["loss"].cpu()) - res["loss"]) / lb
        ratios["loss, relative error"] = abs(float(keep["loss"].cpu()) - res["loss"]) / res["loss_abs"]
    if c["spec"]["src"]:                                       # output channels padded from the source's: exactly relu(bias), or 0
        n_src = c["spec"]["src"][1]
        got = keep["out"].cpu()[..., n_src:]
        want = a["bias"][n_src:].clamp(min=0).expand_as(got) if a["bias"] is not None else torch.zeros_like(got)
        assert torch.equal(got, want), (name, "padded output channels")
    print(f"[{name} precision {precision}] err / bound: " + "  ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if k in ("out", "pooled", "loss") and not v <= 1.0}
    assert not bad, (name, precision, bad)


def test_every_rule_of_the_argument_check_refuses_and_leaves_the_outputs_alone():
    """each rule of harp_conv3x3's argument check as one change to a valid launch (real buffers; its tile lists are all empty, so nothing
    could be computed either way): HARP_ERR_ARG, and afterwards every output still holds its prefill"""
    from harp_amd import _lib
    g = torch.Generator().manual_seed(5)
    N, H, W, Cin, Cout, T = 2, 8, 8, 16, 64, 2
    t = dict(in_=torch.randn(N, H, W, Cin, generator=g), bias=torch.randn(Cout, generator=g), out=torch.randn(N, H, W, Cout, generator=g),
             pooled=torch.randn(N, H // 2, W // 2, Cout, generator=g), target=torch.randn(T, H, W, Cout, generator=g),
             g_tap=torch.randn(N, H, W, Cout, generator=g), loss=torch.tensor([0.75], dtype=torch.float64), gate=torch.randn(N, H, W, Cout, generator=g),
             tile_list=torch.zeros(T, 2, dtype=torch.int32), tile_count=torch.zeros(T, dtype=torch.int32), in_valid=torch.ones(T, 4, dtype=torch.int32),
             out_valid=torch.ones(T, 4, dtype=torch.int32))
    d = {k: v.to(DEV) for k, v in t.items()}
    d["filters"] = torch.zeros(_lib.lib().harp_conv3x3_filter_bytes(Cout, Cin), dtype=torch.uint8, device=DEV)
    ints = dict(N=N, H=H, W=W, Cin=Cin, Cout=Cout, precision=0, epilogue=R.RELU, in_channels=0, max_tiles=2, in_valid_shift=1, tile_pitch=2,
                in_valid_pitch=2, out_valid_pitch=2, tile_side=0, in_valid_cell=0, out_valid_cell=0)

    def call(change):
        s = _lib.Conv3x3Args()
        for k, v in d.items():
            setattr(s, k, None if (k in change and change[k] is None) else _lib.ptr(v))
        for k, v in ints.items():
            setattr(s, k, change.get(k, v))
        s.tap_scale = 0.5
        return _lib.lib().harp_conv3x3(ctypes.byref(s), _lib.stream())

    assert call({}) == 0                                       # the unchanged launch is accepted (and owns nothing)
    assert _lib.lib().harp_conv3x3(None, _lib.stream()) == ERR_ARG
    for what, change in C.REFUSALS:
        assert call(change) == ERR_ARG, what
    torch.cuda.synchronize()
    for k in ("out", "pooled", "g_tap", "loss"):
        assert torch.equal(d[k].cpu(), t[k]), k
