"""CPU: anchors of tests/_conv_ref.py, the float64 restatement of one harp_conv3x3 launch that tests/test_gpu_conv_paths.py compares the
kernel with — against torch's own conv2d / relu / max_pool2d and their float64 autograd (all four epilogues, odd H and W), and, chained over
the ten forward launches with the fields filled as harp_vgg16_term's bounded mode fills them from active_tiles(), against the float64
torch module (which pins the cell, origin and shift conventions to something that is not the kernel).  Then every case of
tests/_conv_cases.py: it reaches the path it is named for, and the reference alone decides all but 1 % of its tap gradient."""
import pytest
import torch
import torch.nn.functional as F

from tests import _conv_cases as C
from tests import _conv_ref as R


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (8, 6), (17, 9)])
def test_unbounded_launch_is_torchs_convolution_and_autograd(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    N, Cin, Cout, Tn = 2, 16, 64, 3
    x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(Cout, generator=g, dtype=torch.float64) * 0.1
    conv = F.conv2d(_nchw(x), w, b, padding=1).requires_grad_(True)
    act = F.relu(conv)
    even = H % 2 == 0 and W % 2 == 0
    # RELU (+ pool) and RELU_TAP
    target = torch.randn(Tn, H, W, Cout, generator=g, dtype=torch.float64).abs()
    rows = torch.tensor([2, 0], dtype=torch.int32)
    a = R.args(in_=x, w=w, bias=b, N=N, H=H, W=W, Cin=Cin, Cout=Cout, epilogue=R.RELU_TAP, out=torch.zeros(N, H, W, Cout),
               pooled=torch.zeros(N, H // 2, W // 2, Cout) if even else None, target=target, target_row=rows,
               g_tap=torch.zeros(N, H, W, Cout), loss=torch.tensor(0.5, dtype=torch.float64), tap_scale=0.37)
    res = R.launch(a)
    loss = 0.37 * (act - _nchw(target[rows.long()])).abs().sum()
    (g_conv,) = torch.autograd.grad(loss, conv)
    assert torch.allclose(_nchw(res["out"]), act.detach(), rtol=0, atol=1e-13)
    assert abs(res["loss"] - 0.5 - loss.item()) < 1e-10
    assert torch.equal(_nchw(res["g_tap"]), g_conv)                     # (+-0.37 or 0: exact)
    if even:
        assert torch.allclose(_nchw(res["pooled"]), F.max_pool2d(act.detach(), 2, 2), rtol=0, atol=1e-13)
    assert res["K"] == 9 * Cin and torch.allclose(_nchw(res["A"]), F.conv2d(_nchw(x).abs(), w.abs(), b.abs(), padding=1), rtol=1e-13)
    # GATE: d / d pre of conv_b(relu(pre)), the filters packed with transpose = 1
    pre = torch.randn(N, Cin, H, W, generator=g, dtype=torch.float64).requires_grad_(True)
    wb = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) * 0.1
    g_b = torch.randn(N, Cout, H, W, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(F.conv2d(F.relu(pre), wb, None, padding=1), pre, g_b)
    wt = R.effective_filters(wb, transpose=True)                        # (64 x 16 -> Cout 16 padded to 64, Cin 64)
    a = R.args(in_=_nhwc(g_b), w=wt, N=N, H=H, W=W, Cin=64, Cout=64, epilogue=R.GATE, out=torch.full((N, H, W, 64), 7.0),
               gate=F.pad(_nhwc(F.relu(pre.detach())), (0, 48)))
    got = R.launch(a)["out"]
    assert torch.allclose(_nchw(got[..., :Cin]), want, rtol=0, atol=1e-13) and (got[..., Cin:] == 0).all()
    # UNPOOL: tap layer -> pool -> conv_b, with exact ties and zeros in the tap activation
    pre = ((torch.randn(N, Cin, 2 * H, 2 * W, generator=g, dtype=torch.float64) * 2).round() / 2).requires_grad_(True)
    (want,) = torch.autograd.grad(F.conv2d(F.max_pool2d(F.relu(pre), 2, 2), wb, None, padding=1), pre, g_b)
    own = torch.randn(N, 2 * H, 2 * W, 64, generator=g, dtype=torch.float64)
    a = R.args(in_=_nhwc(g_b), w=wt, N=N, H=H, W=W, Cin=64, Cout=64, epilogue=R.UNPOOL, out=own,
               gate=F.pad(_nhwc(F.relu(pre.detach())), (0, 48)))
    res = R.launch(a)
    assert torch.allclose(_nchw((res["out"] - own)[..., :Cin]), want, rtol=0, atol=1e-13)
    assert torch.equal(res["out"][~res["out_written"]], own[~res["out_written"]])


_DIV = (1, 1, 2, 2, 4, 4, 4, 8, 8, 8)
_TAPS = (1, 3, 6, 9)
_BEHIND_POOL = (2, 4, 7)
SENT = -77.0


def _module_activations(vgg64, x):
    """relu(conv k), k = 0..9, and the three pooled maps of the float64 torch module, NHWC"""
    acts, pools, h = [], [], x
    for n in range(1, 5):
        for _, layer in getattr(vgg64, f"slice{n}").named_children():
            h = layer(h)
            if isinstance(layer, torch.nn.ReLU):
                acts.append(_nhwc(h))
            elif isinstance(layer, torch.nn.MaxPool2d):
                pools.append(_nhwc(h))
    return acts, pools


@pytest.mark.parametrize("sides", [(16, 8, 8, 8), (16, 16, 16, 8)])
@pytest.mark.parametrize("S", [24, 72])
def test_chained_bounded_launches_reproduce_the_torch_module_inside_the_tiles(S, sides):
    from harp_amd.model.vgg import Vgg16Features
    from harp_amd.model.vgg_hip import active_tiles
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(S)
    Tn, N = 3, 2
    vgg64 = Vgg16Features(weights="random", seed=5).double()
    convs = [m for n in range(1, 5) for m in getattr(vgg64, f"slice{n}").children() if isinstance(m, torch.nn.Conv2d)]
    for m in convs:
        m.bias.data = torch.randn(m.bias.shape, generator=g, dtype=torch.float64) * 0.05
    rgb = torch.rand(N, S, S, 3, generator=g, dtype=torch.float64)
    y_true = torch.rand(Tn, S, S, 3, generator=g, dtype=torch.float64)
    mask = torch.zeros(Tn, S, S, dtype=torch.float64)
    mask[0, S - 3:, S - 2:] = 1.0                                       # touches the bottom-right corner
    mask[2, S // 2 - 1:S // 2 + 1, S // 3:S // 3 + 3] = 0.5             # a few interior pixels; frame 1 is empty
    rows = torch.tensor([2, 0], dtype=torch.int32)
    m = mask[rows.long()][..., None]
    with torch.no_grad():
        want, want_pool = _module_activations(vgg64, _nchw(rgb * m))
        cache, cache_pool = _module_activations(vgg64, _nchw(y_true * mask[..., None]))     # the target frames' activations, all T rows
    bound = active_tiles(mask.float(), tile_sides=sides)
    x0 = torch.zeros(N, S, S, 4, dtype=torch.float64)
    x0[..., :3] = rgb * m
    inp, tap, unowned = x0, 0, 0
    for k in range(10):                                                 # the fields as vgg_forward fills them in bounded mode
        s, lv = S // _DIV[k], (0, 0, 1, 1, 2, 2, 2, 3, 3, 3)[k]
        cin = convs[k].in_channels
        Cin = (cin + 15) // 16 * 16
        w = torch.zeros(convs[k].out_channels, Cin, 3, 3, dtype=torch.float64)
        w[:, :cin] = convs[k].weight.data
        tiles, lst, cnt, mx, origin, pitch, side = bound[lv]
        a = R.args(in_=inp, w=w, bias=convs[k].bias.data, N=N, H=s, W=s, Cin=Cin, Cout=w.shape[0], epilogue=R.RELU,
                   in_channels=4 if k == 0 else 0, out=torch.full((N, s, s, w.shape[0]), SENT, dtype=torch.float64), target_row=rows,
                   tile_list=lst, tile_count=cnt, max_tiles=mx, tile_origin=origin, tile_pitch=pitch, tile_side=side)
        is_tap = k in _TAPS
        if is_tap and tap < 3:
            a["pooled"] = torch.full((N, s // 2, s // 2, w.shape[0]), SENT, dtype=torch.float64)
        if k > 0:
            behind = k in _BEHIND_POOL
            pt, _, _, _, po, pp, ps = bound[lv - 1 if behind else lv]
            a.update(in_valid=pt, in_valid_origin=po, in_valid_pitch=pp, in_valid_shift=0 if behind else 1,
                     in_valid_cell=ps // 2 if behind else ps, in_alt=cache_pool[_BEHIND_POOL.index(k)] if behind else cache[k - 1])
        res = R.launch(a, with_bounds=False)
        own = res["owned"]
        assert own.any()
        unowned += int(not own.all())
        assert (res["out"][~own] == SENT).all(), k
        err = (res["out"] - want[k])[own].abs().max().item()
        assert err < 1e-12, (k, err)                                    # inside the active tiles: the module's activation
        inp = res["out"]
        if is_tap and tap < 3:
            pown = res["pooled_written"][..., 0]
            assert (res["pooled"][~pown] == SENT).all() and (res["pooled"] - want_pool[tap])[pown].abs().max().item() < 1e-12, k
            inp = res["pooled"]
        tap += is_tap
    assert unowned >= (7 if S == 72 else 2), unowned                    # the tiles leave part of the maps out


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_case_reaches_its_path_and_the_reference_decides_its_tap_gradient(name):
    c = C.build(name)
    res = R.launch(c["a"])
    f = C.check(c, res)
    print(f"[{name}] K {res['K']}, reaches: " + " ".join(k for k, v in sorted(f.items()) if v))
    w = res.get("out_written")
    if c["a"]["epilogue"] == R.UNPOOL:
        assert w.any() and not w.all()
    if c["a"]["epilogue"] == R.RELU_TAP:
        e = R.f16_exponent(c["in_amax"], c["in_exp"])
        for precision in (0, 1, 2):
            und = R.tap_undecided(res, R.bound(res, precision, e))
            share = und.float().mean().item()
            print(f"[{name}] precision {precision}: undecided share of the tap gradient {share:.5f}")
            assert share <= 0.01, (name, precision, share)


def test_refusal_list_names_every_rule_once():
    names = [n for n, _ in C.REFUSALS]
    assert len(set(names)) == len(names) and all(set(ch) <= set(R.FIELDS) | {"filters"} for _, ch in C.REFUSALS)
