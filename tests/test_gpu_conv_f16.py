"""GPU: the single-pass f16 mode of the perceptual term's convolutions (harp_conv3x3 precision 2: one v_mfma_f32_32x32x16_f16 product per
MAC, float32 accumulation, a per-launch power-of-two shift of the staged input).  The yardstick is the reference's own arithmetic — TF32
convolutions (torch 1.11 + cuDNN, allow_tf32 on by default), emulated in float64 by tests/_tf32.py: every error of mode 2 against the exact
float64 stack must stay within twice what emulated TF32 makes of the same case."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _tf32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = 2
LW = [1, 1 / 16, 1 / 8, 1 / 4, 1]
SHAPES = [(16, 64, 32, 32), (64, 64, 40, 24), (64, 128, 32, 32), (128, 256, 16, 16), (256, 512, 16, 16), (512, 512, 8, 8)]


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _case(Cin, Cout, H, W, N=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g, dtype=torch.float64) * 0.1
    return x, w, b


def _err(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()


def _rel2(got, want):
    return ((got.double().cpu() - want).norm() / want.norm()).item()


# ---- (1) layer cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_relu_pool_f16(shape):
    from harp_amd.model import conv_hip as C
    Cin, Cout, H, W = shape
    x, w, b = _case(*shape)
    exact = F.relu(F.conv2d(x, w, b, padding=1))
    emu = F.relu(_tf32.conv(x, w, b))
    xd, bd = _nhwc(x).float().to(DEV), b.float().to(DEV)
    filt = C.pack_filters(w.float().to(DEV), F16)
    out = torch.full((x.shape[0], H, W, Cout), float("nan"), device=DEV)
    pooled = torch.full((x.shape[0], H // 2, W // 2, Cout), float("nan"), device=DEV)
    C.conv3x3(xd, filt, Cout, bias=bd, epilogue=C.RELU, precision=F16, out=out, pooled=pooled)
    torch.cuda.synchronize()
    e, et = _err(_nchw(out), exact), _err(emu, exact)
    ep, ept = _err(_nchw(pooled), F.max_pool2d(exact, 2, 2)), _err(F.max_pool2d(emu, 2, 2), F.max_pool2d(exact, 2, 2))
    print(f"[f16 RELU {shape}] out {e:.2e} (TF32 {et:.2e}), pooled {ep:.2e} (TF32 {ept:.2e})")
    assert e <= 2 * et and e <= 2e-3 and ep <= 2 * ept and ep <= 2e-3, (e, et, ep, ept)
    pooled2 = torch.empty_like(pooled)
    C.conv3x3(xd, filt, Cout, bias=bd, epilogue=C.RELU, precision=F16, out=None, pooled=pooled2)
    assert torch.equal(pooled2, pooled)


def test_tap_epilogue_f16():
    from harp_amd.model import conv_hip as C
    Cin, Cout, H, W = 64, 128, 32, 32
    x, w, b = _case(Cin, Cout, H, W, N=3)
    g = torch.Generator().manual_seed(9)
    target = torch.relu(torch.randn(5, Cout, H, W, generator=g, dtype=torch.float64))
    rows = torch.tensor([4, 0, 2])
    scale = 0.37
    pre = F.conv2d(x, w, b, padding=1)
    exact = F.relu(pre)
    emu = F.relu(_tf32.conv(x, w, b))
    loss_exact = scale * (exact - target[rows]).abs().sum().item()
    loss_emu = scale * (emu - target[rows]).abs().sum().item()
    filt = C.pack_filters(w.float().to(DEV), F16)
    out = torch.empty(3, H, W, Cout, device=DEV)
    g_tap = torch.empty_like(out)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    C.conv3x3(_nhwc(x).float().to(DEV), filt, Cout, bias=b.float().to(DEV), epilogue=C.RELU_TAP, precision=F16, out=out,
              target=_nhwc(target).float().to(DEV), target_row=rows.int().to(DEV), tap_scale=scale, g_tap=g_tap, loss=acc)
    torch.cuda.synchronize()
    e, et = _err(_nchw(out), exact), _err(emu, exact)
    dl = abs(acc.item() - loss_exact)
    dlt = abs(loss_emu - loss_exact)
    print(f"[f16 RELU_TAP] out {e:.2e} (TF32 {et:.2e}); loss error {dl / loss_exact:.2e} (TF32 {dlt / loss_exact:.2e})")
    assert e <= 2 * et and e <= 2e-3 and dl <= 2 * dlt + 1e-6 * loss_exact
    # g_tap = scale * sign(out - target) * [out > 0] wherever the sign is decided at the TF32 class
    d = _nchw(g_tap).double().cpu()
    want = (scale * torch.sign(exact - target[rows]) * (exact > 0)).float().double()
    clear = ((exact - target[rows]).abs() > 1e-2) & (pre.abs() > 1e-2)
    assert clear.float().mean() > 0.5 and torch.equal(d[clear], want[clear])


@pytest.mark.parametrize("shape", [(64, 64, 40, 24), (128, 64, 32, 32), (512, 256, 16, 16)])
def test_data_gradient_through_relu_f16(shape):
    from harp_amd.model import conv_hip as C
    Cout_b, Cin_b, H, W = shape
    g = torch.Generator().manual_seed(3)
    a = torch.randn(2, Cin_b, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout_b, Cin_b, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * Cin_b)) ** 0.5
    g_b = torch.randn(2, Cout_b, H, W, generator=g, dtype=torch.float64) * 1e-9      # (a gradient's magnitude: below f16's range unshifted)
    gate = (a > 0).double()
    exact = F.conv_transpose2d(g_b, w, padding=1) * gate
    emu = F.conv_transpose2d(_tf32.tf32_round(g_b), _tf32.tf32_round(w), padding=1) * gate
    filt = C.pack_filters(w.float().to(DEV), F16, transpose=True)
    out = torch.full((2, H, W, Cin_b), float("nan"), device=DEV)
    C.conv3x3(_nhwc(g_b).float().to(DEV), filt, Cin_b, epilogue=C.GATE, precision=F16, out=out, gate=_nhwc(F.relu(a)).float().to(DEV))
    torch.cuda.synchronize()
    e, et = _err(_nchw(out), exact), _err(emu, exact)
    print(f"[f16 GATE {shape}] {e:.2e} (TF32 {et:.2e})")
    assert e <= 2 * et and e <= 2e-3, (e, et)


def test_data_gradient_through_max_pool_f16():
    from harp_amd.model import conv_hip as C
    Cin_b, Cout_b, H, W = 64, 128, 16, 24
    g = torch.Generator().manual_seed(4)
    pre = (torch.randn(2, Cin_b, 2 * H, 2 * W, generator=g, dtype=torch.float64) * 2).round() / 2
    w = torch.randn(Cout_b, Cin_b, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * Cin_b)) ** 0.5
    g_b = torch.randn(2, Cout_b, H, W, generator=g, dtype=torch.float64)
    g_own = torch.randn(2, Cin_b, 2 * H, 2 * W, generator=g, dtype=torch.float64)
    act = F.relu(pre)

    def routed(conv_g):
        p = act.detach().clone().requires_grad_(True)
        (r,) = torch.autograd.grad(F.max_pool2d(p, 2, 2), p, conv_g)
        return r * (act > 0) + g_own
    exact = routed(F.conv_transpose2d(g_b, w, padding=1))
    emu = routed(F.conv_transpose2d(_tf32.tf32_round(g_b), _tf32.tf32_round(w), padding=1))
    filt = C.pack_filters(w.float().to(DEV), F16, transpose=True)
    out = _nhwc(g_own).float().to(DEV)
    C.conv3x3(_nhwc(g_b).float().to(DEV), filt, Cin_b, epilogue=C.UNPOOL, precision=F16, out=out, gate=_nhwc(act).float().to(DEV))
    torch.cuda.synchronize()
    e, et = _err(_nchw(out), exact), _err(emu, exact)
    print(f"[f16 UNPOOL] {e:.2e} (TF32 {et:.2e})")
    assert e <= 2 * et and e <= 2e-3, (e, et)


def test_precision_3_is_refused():
    from harp_amd import _lib
    from harp_amd.model import conv_hip as C
    w = torch.zeros(64, 16, 3, 3, device=DEV)
    with pytest.raises(RuntimeError, match="harp_conv3x3_pack_filters"):
        C.pack_filters(w, 3)
    f = C.pack_filters(w, F16)
    x = torch.zeros(1, 8, 8, 16, device=DEV)
    with pytest.raises(RuntimeError, match="harp_conv3x3"):
        C.conv3x3(x, f, 64, precision=3, out=torch.zeros(1, 8, 8, 64, device=DEV))
    net = _lib.Vgg16()
    net.precision = 3
    assert _lib.lib().harp_vgg16_term(ctypes.byref(net), None, None) == 1          # HARP_ERR_ARG, before any launch


# ---- (2) the whole term ------------------------------------------------------------------------------------------------------------------
def _term_reference(filters, lw, rgb, y_true, mask):
    """loss, d loss / d rgb and the four target taps of L1(vgg(rgb * mask), vgg(y_true * mask)), exact and TF32-emulated (float64)"""
    out = {}
    for tf32 in (False, True):
        r = rgb.detach().clone().requires_grad_(True)
        m = mask.unsqueeze(-1)
        loss = F.l1_loss(_tf32.rows(filters, lw, (r * m).permute(0, 3, 1, 2), tf32), _tf32.rows(filters, lw, (y_true * m).permute(0, 3, 1, 2), tf32))
        (gr,) = torch.autograd.grad(loss, r)
        out[tf32] = (loss.item(), gr)
    return out


def _check_term(tag, loss, grad, ref):
    (l0, g0), (lt, gt) = ref[False], ref[True]
    dl, dlt = abs(loss - l0), abs(lt - l0)
    r, rt = _rel2(grad, g0), _rel2(gt, g0)
    print(f"[f16 term {tag}] loss {loss:.8f} vs exact {l0:.8f}: {dl / l0:.1e} (TF32 {dlt / l0:.1e}); gradient rel-L2 {r:.2e} (TF32 {rt:.2e})")
    return dl, dlt, r, rt


def test_whole_term_f16_against_emulated_tf32():
    from harp_amd.model.vgg import Vgg16Features
    from harp_amd.model.vgg_hip import Vgg16Hip
    S, N, T = 64, 2, 3
    vgg = Vgg16Features(layers_weights=LW, weights="random", seed=1)
    filters = _tf32.filters_of(vgg)
    g = torch.Generator().manual_seed(11)
    rgb = torch.rand(N, S, S, 3, generator=g, dtype=torch.float64)
    y_true = torch.rand(T, S, S, 3, generator=g, dtype=torch.float64)
    mask = (torch.rand(T, S, S, generator=g, dtype=torch.float64) > 0.3).double()
    mask[:, ::7] *= 0.5
    rows = torch.tensor([2, 0])
    ref = _term_reference(filters, LW, rgb, y_true[rows], mask[rows])
    # tap features of the target frames
    hip = Vgg16Hip(vgg, DEV, F16)
    rgb_d, yt_d, mask_d = (t.float().to(DEV).contiguous() for t in (rgb, y_true, mask))
    rows_d = rows.int().to(DEV)
    feats = hip.features(yt_d, mask_d)
    xin = (y_true * mask.unsqueeze(-1)).permute(0, 3, 1, 2)
    for k, (f, ex, em) in enumerate(zip(feats, _tf32.taps(filters, xin, False), _tf32.taps(filters, xin, True))):
        e, et = _err(_nchw(f), ex), _err(em, ex)
        print(f"[f16 features tap {k}] {e:.2e} (TF32 {et:.2e})")
        assert e <= 2 * et, (k, e, et)
    for by_row in (1, 0):
        target = feats if by_row else hip.features(yt_d, mask_d, rows_d)
        g_rgb = torch.zeros(N, S, S, 3, device=DEV)
        loss = torch.zeros(1, device=DEV)
        hip.term(rgb_d, yt_d, mask_d, rows_d, target, by_row, g_rgb, loss, weight=1.0)
        torch.cuda.synchronize()
        dl, dlt, r, rt = _check_term(f"64x64 cached={by_row}", loss.item(), g_rgb, ref)
        assert dl <= 2 * dlt + 1e-6 * ref[False][0], (dl, dlt)
        assert r <= 2 * rt, (r, rt)


def _golden_pair(golden_dir):
    import sys
    from harp_amd.model.vgg import Vgg16Features
    sys.path.insert(0, golden_dir)
    from vgg_filters import state_dict_torchvision_layout
    ref = np.load(os.path.join(golden_dir, "vgg_ref.npz"))
    lw = [float(v) for v in ref["layers_weights_fit"]]
    return ref, lw, Vgg16Features(layers_weights=lw, weights=state_dict_torchvision_layout())


@pytest.mark.parametrize("shift", [True, False])
def test_reference_pair_full_and_bounded_f16(golden_dir, shift):
    from harp_amd.model.vgg_hip import Vgg16Hip, active_tiles
    ref, lw, vgg = _golden_pair(golden_dir)
    rgb, y_true, mask = (torch.from_numpy(ref[k]).double() for k in ("pair_pred", "pair_true", "pair_mask"))
    mask = mask[None]
    emu = _term_reference(_tf32.filters_of(vgg), lw, rgb, y_true, mask)
    hip = Vgg16Hip(vgg, DEV, F16)
    rgb_d, yt_d, mask_d = (t.float().to(DEV).contiguous() for t in (rgb, y_true, mask))
    rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    cache = hip.features(yt_d, mask_d, all_slots=True)
    res = {}
    for name, bd in (("full", None), ("bounded", active_tiles(mask_d, shift_grid=shift))):
        g_rgb, loss = torch.zeros_like(rgb_d), torch.zeros(1, device=DEV)
        hip.term(rgb_d, yt_d, mask_d, rows, cache, 1, g_rgb, loss, weight=1.0, bound=bd)
        torch.cuda.synchronize()
        res[name] = (loss.item(), g_rgb.double().cpu())
        dl, dlt, r, rt = _check_term(f"reference pair {name} shift={shift}", loss.item(), g_rgb, emu)
        print(f"   (the reference's own float32 run: loss {float(ref['pair_loss']):.8f}, gradient rel-L2 vs it {_rel2(g_rgb, torch.from_numpy(ref['pair_grad']).double()):.2e})")
        assert dl <= 2 * dlt + 1e-6 * emu[False][0] and r <= 2 * rt, (name, dl, dlt, r, rt)
    assert torch.equal(res["full"][1], res["bounded"][1]) and abs(res["full"][0] - res["bounded"][0]) <= 1e-6 * res["full"][0]


def test_module_call_f16_against_emulated_tf32(golden_dir):
    """`Vgg16Features.forward` / backward on HIP tensors with hip_precision = 2 (model/vgg_hip.py Vgg16Rows: one harp_conv3x3 per layer, the
    exponent shift reduced from each launch's input on the device)"""
    ref, lw, vgg = _golden_pair(golden_dir)
    vgg.hip_precision = F16
    filters = _tf32.filters_of(vgg)
    g = torch.Generator().manual_seed(9)
    x = torch.from_numpy(ref["x_64x48"]).double()
    R = torch.randn(2, _tf32.rows(filters, lw, x, False).shape[1], generator=g, dtype=torch.float64)
    want = {}
    for tf32 in (False, True):
        xr = x.clone().requires_grad_(True)
        row = _tf32.rows(filters, lw, xr, tf32)
        (gx,) = torch.autograd.grad((row * R).sum(), xr)
        want[tf32] = (row.detach(), gx)
    xd = x.float().to(DEV).requires_grad_(True)
    row = vgg(xd)
    (gx,) = torch.autograd.grad((row * R.float().to(DEV)).sum(), xd)
    torch.cuda.synchronize()
    e, et = _err(row.detach(), want[False][0]), _err(want[True][0], want[False][0])
    r, rt = _rel2(gx, want[False][1]), _rel2(want[True][1], want[False][1])
    print(f"[f16 module call 64x48] row {e:.2e} (TF32 {et:.2e}), input gradient rel-L2 {r:.2e} (TF32 {rt:.2e})")
    assert e <= 2 * et and r <= 2 * rt, (e, et, r, rt)


# ---- (3) range -----------------------------------------------------------------------------------------------------------------------------
def test_range_tiny_seeds_and_large_inputs():
    """the gradient seeds of the term at C3 (layer_w / n ~ 1e-9 ... 1e-10) and below lie under f16's smallest subnormal: without the
    exponent shift every backward convolution would stage zeros.  Layer weights x 2^-28 must scale loss and gradient by exactly 2^-28; a
    2^-28-scaled row gradient through the module call likewise; inputs and biases x 2^8 scale the features by 2^8, with nothing infinite."""
    from harp_amd.model.vgg import Vgg16Features
    from harp_amd.model.vgg_hip import Vgg16Hip
    S, N, T = 64, 2, 3
    g = torch.Generator().manual_seed(11)
    rgb = torch.rand(N, S, S, 3, generator=g).to(DEV)
    y_true = torch.rand(T, S, S, 3, generator=g).to(DEV)
    mask = (torch.rand(T, S, S, generator=g) > 0.3).float().to(DEV)
    rows = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    k = 2.0 ** -28
    res = {}
    for s in (1.0, k):
        vgg = Vgg16Features(layers_weights=[w * s for w in LW], weights="random", seed=1)
        hip = Vgg16Hip(vgg, DEV, F16)
        g_rgb, loss = torch.zeros(N, S, S, 3, device=DEV), torch.zeros(1, device=DEV)
        hip.term(rgb, y_true, mask, rows, hip.features(y_true, mask), 1, g_rgb, loss, weight=1.0)
        torch.cuda.synchronize()
        res[s] = (loss.item(), g_rgb.clone())
    (l1, g1), (lk, gk) = res[1.0], res[k]
    print(f"[f16 range] loss {l1:.6e} / x2^-28 {lk:.6e}; gradient max {g1.abs().max().item():.3e} / {gk.abs().max().item():.3e}")
    assert g1.abs().max() > 0 and abs(lk - k * l1) <= 1e-6 * k * l1
    assert torch.equal(gk, g1 * k)
    # the module call: a row gradient of magnitude 2^-28
    vgg = Vgg16Features(layers_weights=LW, weights="random", seed=1)
    vgg.hip_precision = F16
    x = torch.rand(2, 3, 64, 48, generator=g).to(DEV)
    R = torch.randn(2, vgg(x).shape[1], generator=g).to(DEV)
    grads = []
    for s in (1.0, k):
        xr = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(vgg(xr), xr, R * s)
        grads.append(gx)
    torch.cuda.synchronize()
    assert grads[0].abs().max() > 0 and torch.equal(grads[1], grads[0] * k)
    # forward: input and biases x 2^8
    big = Vgg16Features(layers_weights=LW, weights="random", seed=1)
    with torch.no_grad():
        for name, p in big.named_parameters():
            if name.endswith("bias"):
                p.mul_(256.0)
    hip1, hip8 = Vgg16Hip(Vgg16Features(layers_weights=LW, weights="random", seed=1), DEV, F16), Vgg16Hip(big, DEV, F16)
    f1 = hip1.features(y_true, mask, all_slots=True)
    f8 = hip8.features(y_true * 256.0, mask, all_slots=True)
    torch.cuda.synchronize()
    for a, b in zip(f1, f8):
        assert torch.isfinite(b).all() and torch.equal(b, a * 256.0)
    big.hip_precision = F16
    small = Vgg16Features(layers_weights=LW, weights="random", seed=1)
    small.hip_precision = F16
    with torch.no_grad():
        r1, r8 = small(x), big(x * 256.0)
    torch.cuda.synchronize()
    assert torch.isfinite(r8).all() and torch.equal(r8[:, 3 * 64 * 48:], r1[:, 3 * 64 * 48:] * 256.0)


# ---- (4) the engine ------------------------------------------------------------------------------------------------------------------------
def test_engine_perceptual_term_in_f16():
    from harp_amd.engine import FitEngine
    from harp_amd.model.vgg import Vgg16Features
    from tests._scene import make_scene
    sc = make_scene(T=3, S=128, seed=0)
    eng = FitEngine(sc["model_np"], sc["topo_np"], sc["tpl"]["verts_uvs"], sc["tpl"]["faces_uvs"], sc["uv_mask"].float(), sc["seq"], sc["S"],
                    sc["focal"], 2, device=DEV)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        eng.params["texture"].copy_(torch.rand(1, 512, 512, 3, generator=g) * 0.5 + 0.3)
    tg = sc["targets"]
    eng.set_targets(tg["y_true"], tg["y_sil"], tg["y_sil_col"])
    eng.compute_reference_mesh()
    vgg = Vgg16Features(layers_weights=LW, weights="random", seed=2)
    fid = torch.tensor([1, 2])
    res = {}
    for prec in (0, 2):
        eng.set_perceptual(vgg, weight=1.0, precision=prec)
        eng.fid.copy_(fid.int().to(DEV)); eng.tfid.copy_(fid.int().to(DEV))
        eng.set_stage(False, True)
        eng.w_vec.zero_()
        eng.forward_backward(False, True)
        torch.cuda.synchronize()
        res[prec] = (eng.losses()["vgg"], {k: eng.grads[k].clone() for k in ("texture", "normal_map")})
    (l0, g0), (l2, g2) = res[0], res[2]
    rels = {k: _rel2(g2[k], g0[k].double().cpu()) for k in g0}
    print(f"[f16 engine] vgg loss {l2:.8f} vs float32 mode {l0:.8f} ({abs(l2 - l0) / l0:.1e}); gradient rel-L2 vs float32 mode", rels)
    assert abs(l2 - l0) <= 1e-3 * abs(l0), (l2, l0)
    # (the whole-term tests put mode 2 and emulated TF32 at gradient rel-L2 of a few 1e-2 against float64: L1-of-features gradients are
    #  signs of differences, and the TF32 class flips the undecided ones)
    assert all(0 < r < 0.1 for r in rels.values()), rels
    # steps through the captured hipGraph
    eng.set_perceptual(vgg, weight=1.0, precision=2)
    eng.set_stage(False, True)
    before = eng.p_buf.clone()
    for _ in range(3):
        eng.step(fid, False, True)
    torch.cuda.synchronize()
    assert eng._graphs and torch.isfinite(eng.p_buf).all() and (eng.p_buf - before).abs().max() > 0
    assert abs(eng.losses()["vgg"]) > 0
    # any other mode is refused before anything changes
    keep = (eng.perceptual, eng._vgg_precision, eng._graphs)
    with pytest.raises(ValueError, match="precision"):
        eng.set_perceptual(vgg, weight=1.0, precision=3)
    assert (eng.perceptual, eng._vgg_precision, eng._graphs) == keep
