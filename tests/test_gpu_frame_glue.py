"""-m gpu: the per-frame glue of the fitting loop through the raw C ABI -- harp_frame_setup_fwd / _bwd (csrc/glue.hip) against their
definition in float64 (row gathers, camera convention, sigmoid of the ambient ratio, shared light; the backward against float64 autograd of
the same definition, with duplicate frame ids, untouched rows and every gradient slot NULL in turn), and harp_adam_apply2 against two
harp_adam_apply calls on the same arenas, bit for bit.  The fused fronts and backs are tested as "equal to harp_frame_setup_* + LBS + chain"
(test_gpu_parity.py), so this pins what they compute.  Conventions as in tests/test_gpu_building_blocks.py: U = 2^-24, every bound next
to its assertion, outputs pre-filled with NaN when overwritten and with random data when accumulated.

measured on the MI355X, worst error as a fraction of its bound: cam_T 0.33, colors 0.06; g_pose 0.32, g_rot 0.25, g_wrist_pose 0.13, g_trans 0.17,
g_cam 0.54, g_shape 0.33, g_light_positions 0.24, g_amb_ratio 0.20; harp_adam_apply2: 0 elements differ from harp_adam_apply."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_building_blocks import DEV, U, _L, _d, _f32, _gen, _keep_alive, _worst  # noqa: F401 (_keep_alive: autouse)

pytestmark = pytest.mark.gpu
T, S, FOCAL = 7, 100, _f32(446.4)
TABLES = dict(pose=(T, 45), rot=(T, 3), trans=(T, 3), cam=(T, 3), shape=(10,), light_positions=(T, 3), amb_ratio=(1,), wrist_pose=(T, 3))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _fid(B):
    """frame ids with duplicates that never name rows 3 and 5 of the T = 7 tables"""
    if B == 1:
        return torch.tensor([4], dtype=torch.int32)
    if B == 3:
        return torch.tensor([2, 2, 6], dtype=torch.int32)
    return torch.tensor([0, 1, 2, 4, 6], dtype=torch.int32)[torch.randint(0, 5, (B,), generator=_gen(B))]


def _tables(arm):
    g = _gen(17 + int(arm))
    tb = {k: torch.randn(s, generator=g) * 0.3 for k, s in TABLES.items()}
    tb["cam"] = torch.tensor([1.1, 0.02, -0.03]) + torch.randn(T, 3, generator=g) * 0.05          # S c0 ~ 110: away from 0
    tb["amb_ratio"] = torch.tensor([0.3])
    if not arm:
        del tb["wrist_pose"]
    return tb


def _definition(tb, fid, arm, share_light, self_shadow):
    """the forward in float64 (utils/visualize.py:26-27, 38-39, 268-271; optimize_sequence.py:453-456, 478-480): tb float64 leaves"""
    f = fid.long()
    B = f.shape[0]
    rows = [tb["rot"][f]] + ([tb["wrist_pose"][f]] if arm else []) + [tb["pose"][f]]
    betas = tb["shape"][None].repeat(B, 1)
    if arm:
        betas = torch.cat([betas, betas.new_zeros(B, 10)], 1)
    cam = tb["cam"][f]
    cam_T = torch.stack([-cam[:, 1], -cam[:, 2], 2 * FOCAL / (S * cam[:, 0] + 1e-9)], 1)
    light = tb["light_positions"][torch.zeros_like(f) if share_light else f]
    if self_shadow:
        amb = torch.sigmoid(tb["amb_ratio"])
        colors = torch.cat([amb.repeat(3), (1 - amb).repeat(3), amb.new_zeros(3)])
    else:
        colors = torch.tensor([0.5] * 3 + [0.4] * 3 + [0.1] * 3, dtype=torch.float64)
    return dict(pose48=torch.cat(rows, 1), betas=betas, trans_b=tb["trans"][f], cam_T=cam_T, light_pos=light, colors=colors)


def _struct(tbd, grads, arm, share_light):
    from harp_amd import _lib
    p = _lib.ptr
    ft = _lib.FrameTables(share_light=share_light, n_betas_out=20 if arm else 10)
    for k in TABLES:
        if k in tbd:
            setattr(ft, k, p(tbd[k]))
            setattr(ft, "g_" + k, p(grads.get(k)))
    return ft


@pytest.mark.parametrize("arm", [False, True], ids=["mano", "arm"])
@pytest.mark.parametrize("B", [1, 3, 65, 130])
def test_frame_setup_forward_is_the_definition(B, arm):
    L, p, st, ck = _L()
    tb, fid = _tables(arm), _fid(B)
    tbd = {k: _d(v) for k, v in tb.items()}
    ps, nbo = (51, 20) if arm else (48, 10)
    for share_light in (0, 1):
        for self_shadow in (0, 1):
            tag = f"frame_setup_fwd B={B} {'arm' if arm else 'mano'} share={share_light} shadow={self_shadow}"
            out = {k: torch.full(s, float("nan"), device=DEV) for k, s in (("pose48", (B, ps)), ("betas", (B, nbo)), ("trans_b", (B, 3)), ("cam_R", (B, 9)),
                                                                             ("cam_T", (B, 3)), ("light_pos", (B, 3)), ("colors", (9,)))}
            ft = _struct(tbd, {}, arm, share_light)
            ck(L.harp_frame_setup_fwd(ctypes.byref(ft), p(_d(fid)), B, S, FOCAL, self_shadow, *(p(out[k]) for k in ("pose48", "betas", "trans_b", "cam_R",
                                                                                                                      "cam_T", "light_pos", "colors")), st()), tag)
            torch.cuda.synchronize()
            ref = _definition({k: v.double() for k, v in tb.items()}, fid, arm, share_light, self_shadow)
            # gathered rows: copies, bit for bit (the zero padding of the betas included)
            for k in ("pose48", "betas", "trans_b", "light_pos"):
                assert torch.equal(_bits(out[k]), _bits(ref[k].float())), (tag, k)
            assert torch.equal(out["cam_R"].cpu(), torch.tensor([-1.0, 0, 0, 0, -1, 0, 0, 0, 1]).repeat(B, 1)), tag
            # cam_T: two negations (exact) and 2 focal / (S c0 + 1e-9): the product, the sum, the quotient: 3 U
            assert torch.equal(_bits(out["cam_T"][:, :2]), _bits(ref["cam_T"][:, :2].float())), tag
            _worst(tag + " cam_T", (out["cam_T"].cpu().double() - ref["cam_T"]).abs(), 3 * U * ref["cam_T"].abs() + 1e-300)
            if self_shadow:
                # sigmoid = 1 / (1 + exp(-x)) and 1 - sigmoid, values in (0, 1): 4 U
                _worst(tag + " colors", (out["colors"].cpu().double() - ref["colors"]).abs(), torch.tensor(4 * U))
                assert (out["colors"][6:] == 0).all()
            else:
                assert torch.equal(out["colors"].cpu(), torch.tensor([0.5] * 3 + [0.4] * 3 + [0.1] * 3)), tag


GRAD_SLOTS = ("pose", "rot", "trans", "cam", "shape", "light_positions", "amb_ratio", "wrist_pose")


@pytest.mark.parametrize("arm", [False, True], ids=["mano", "arm"])
@pytest.mark.parametrize("B", [1, 3, 65, 130])
def test_frame_setup_backward_against_float64_autograd(B, arm):
    L, p, st, ck = _L()
    tb, fid = _tables(arm), _fid(B)
    tbd = {k: _d(v) for k, v in tb.items()}
    ps, nbo = (51, 20) if arm else (48, 10)
    g = _gen(B * 2 + int(arm))
    cot = {k: torch.randn(s, generator=g) for k, s in (("pose48", (B, ps)), ("betas", (B, nbo)), ("trans_b", (B, 3)), ("cam_T", (B, 3)),
                                                      ("light_pos", (B, 3)), ("colors", (9,)))}
    cotd = {k: _d(v) for k, v in cot.items()}
    pre = {k: torch.randn(tb[k].shape, generator=g) for k in tb}                   # every gradient table accumulates (+=)
    slots = [k for k in GRAD_SLOTS if k in tb]
    absent = [r for r in range(T) if r not in set(fid.tolist())]
    assert len(set(fid.tolist())) < B or B == 1                                     # duplicates
    assert {3, 5} <= set(absent)
    for share_light, self_shadow in ((0, 1), (1, 1), (0, 0)):
        # ---- float64 autograd of the definition; absum: the same sums with every term replaced by its magnitude (the bound's scale)
        leaves = {k: v.double().requires_grad_() for k, v in tb.items()}
        out = _definition(leaves, fid, arm, share_light, self_shadow)
        keys = list(cot)
        gr = torch.autograd.grad(sum((out[k] * cot[k].double()).sum() for k in keys), list(leaves.values()), allow_unused=True)
        ref = {k: (torch.zeros_like(v) if r is None else r) for (k, v), r in zip(leaves.items(), gr)}
        f = fid.long()
        absum = {k: pre[k].double().abs() for k in tb}
        absum["rot"].index_add_(0, f, cot["pose48"][:, :3].double().abs())
        if arm:
            absum["wrist_pose"].index_add_(0, f, cot["pose48"][:, 3:6].double().abs())
        absum["pose"].index_add_(0, f, cot["pose48"][:, ps - 45:].double().abs())
        absum["shape"] += cot["betas"][:, :10].double().abs().sum(0)
        absum["trans"].index_add_(0, f, cot["trans_b"].double().abs())
        den = S * tb["cam"].double()[f, 0] + 1e-9
        absum["cam"].index_add_(0, f, torch.stack([cot["cam_T"][:, 2].double().abs() * 2 * FOCAL * S / den ** 2, cot["cam_T"][:, 0].double().abs(),
                                                   cot["cam_T"][:, 1].double().abs()], 1))
        absum["light_positions"].index_add_(0, torch.zeros_like(f) if share_light else f, cot["light_pos"].double().abs())
        amb = torch.sigmoid(tb["amb_ratio"].double())
        if self_shadow:
            absum["amb_ratio"] += cot["colors"][:6].double().abs().sum() * amb * (1 - amb)
        for null in [None] + (slots if B == 3 else []):
            tag = f"frame_setup_bwd B={B} {'arm' if arm else 'mano'} share={share_light} shadow={self_shadow} NULL={null}"
            grads = {k: _d(pre[k]) for k in slots if k != null}
            ft = _struct(tbd, grads, arm, share_light)
            ck(L.harp_frame_setup_bwd(ctypes.byref(ft), p(_d(fid)), B, S, FOCAL, self_shadow, *(p(cotd[k]) for k in keys), st()), tag)
            torch.cuda.synchronize()
            for k in grads:
                got = grads[k].cpu()
                # a float32 sum of at most B terms onto the pre-fill: (B + 2) U of the absolute sum
                _worst(f"{tag} g_{k}", (got.double() - pre[k].double() - ref[k]).abs(), (B + 2) * U * absum[k] + 1e-300)
                if k in ("pose", "rot", "trans", "cam", "wrist_pose") or (k == "light_positions" and not share_light):
                    assert torch.equal(_bits(got[absent]), _bits(pre[k][absent])), (tag, k)            # rows not in fid: untouched
                if k == "light_positions" and share_light:
                    assert torch.equal(_bits(got[1:]), _bits(pre[k][1:])) and ref[k][0].abs().max() > 0, (tag, k)   # everything sums into row 0
                if k == "amb_ratio" and not self_shadow:
                    assert torch.equal(_bits(got), _bits(pre[k])), (tag, k)
                elif null is None:
                    assert ref[k].abs().max() > 0, (tag, k)                            # non-vacuous
            if null is None and B > 1:
                d = int(torch.bincount(f).argmax())                                   # a duplicated row holds the SUM of its frames' gradients
                want = cot["trans_b"].double()[f == d].sum(0)
                assert (f == d).sum() > 1 and torch.allclose(ref["trans"][d], want, rtol=0, atol=1e-14), tag
        if self_shadow:
            # g_amb_ratio = (sum g_colors[0:3] - sum g_colors[3:6]) amb (1 - amb)
            want = (cot["colors"][:3].double().sum() - cot["colors"][3:6].double().sum()) * amb * (1 - amb)
            assert torch.allclose(ref["amb_ratio"], want, rtol=1e-13, atol=0)


def test_frame_and_light_setup_refuse_empty_batches_untouched():
    """B <= 0 returns HARP_ERR_ARG before any launch, with real buffers: nothing is written"""
    L, p, st, _ = _L()
    tb = _tables(True)
    tbd = {k: _d(v) for k, v in tb.items()}
    grads = {k: torch.full(tb[k].shape, 5.0, device=DEV) for k in tb}
    ft = _struct(tbd, grads, True, 0)
    fid = _d(torch.zeros(4, dtype=torch.int32))
    bufs = [torch.full((4, 51), 5.0, device=DEV) for _ in range(7)]
    for B in (0, -1):
        assert L.harp_frame_setup_fwd(ctypes.byref(ft), p(fid), B, S, FOCAL, 1, *(p(b) for b in bufs), st()) == 1
        assert L.harp_frame_setup_bwd(ctypes.byref(ft), p(fid), B, S, FOCAL, 1, *(p(b) for b in bufs[:6]), st()) == 1
        assert L.harp_light_setup_fwd(p(bufs[0]), p(bufs[1]), B, p(bufs[2]), p(bufs[3]), st()) == 1
        assert L.harp_light_setup_bwd(p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), B, 4, p(bufs[4]), p(bufs[5]), p(bufs[6]), st()) == 1
    torch.cuda.synchronize()
    assert all(bool((b == 5.0).all()) for b in bufs + list(grads.values()))


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_adam_apply2
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o0,n0,o1,n1", [(3, 0, 5, 1),                             # off a 16-byte boundary, an empty and a one-element segment
                                         (1, 300001, 300009, 400003),               # off the boundary, 700 004 elements: past the grid's 524 288 lanes
                                         (64, 1000000, 1000128, 1200000)])          # whole quads (the 16-byte path), 550 000 quads: past the grid again
def test_adam_apply2_equals_two_adam_apply_calls_bit_for_bit(o0, n0, o1, n1):
    L, p, st, ck = _L()
    n = o1 + n1 + 37
    g = _gen(o0 + n1)
    P0, G = torch.randn(n, generator=g), torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 4 - 3)
    M0, V0 = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
    raw = bytearray(64)                                                             # two harp_adam_hyper: lr b1 b2 eps grad_scale | step | derived
    np.frombuffer(raw, np.float32, 5, 0)[:] = [1e-2, 0.9, 0.999, 1e-8, 0.37]
    np.frombuffer(raw, np.float32, 5, 32)[:] = [3e-3, 0.8, 0.99, 1e-6, 1.0]
    hyper = _d(torch.frombuffer(raw, dtype=torch.uint8).clone())
    Gd = _d(G)
    A = [_d(t.clone()) for t in (P0, M0, V0)]                                       # harp_adam_apply2
    Bb = [_d(t.clone()) for t in (P0, M0, V0)]                                      # two harp_adam_apply calls
    for step in range(2):
        ck(L.harp_adam_tick(p(hyper), 2, st()), "adam_tick")
        ck(L.harp_adam_apply2(p(A[0]), p(Gd), p(A[1]), p(A[2]), o0, n0, o1, n1, p(hyper), st()), "adam_apply2")
        for o, m, h in ((o0, n0, 0), (o1, n1, 32)):
            if m:                                                                   # (an empty segment is no call: harp_adam_apply's grid would be empty)
                ck(L.harp_adam_apply(p(Bb[0]) + 4 * o, p(Gd) + 4 * o, p(Bb[1]) + 4 * o, p(Bb[2]) + 4 * o, m, p(hyper) + h, st()), "adam_apply")
    torch.cuda.synchronize()
    inside = torch.zeros(n, dtype=torch.bool)
    inside[o0:o0 + n0] = True
    inside[o1:o1 + n1] = True
    assert int(inside.sum()) == n0 + n1 and not inside[:o0].any()
    for a, b, init, name in zip(A, Bb, (P0, M0, V0), "pmv"):
        a, b = a.cpu(), b.cpu()
        assert torch.equal(_bits(a[~inside]), _bits(init[~inside])), name          # outside both segments: untouched
        differ = int((_bits(a) != _bits(b)).sum())
        print(f"[adam_apply2 o0={o0} n0={n0} o1={o1} n1={n1}] {name}: {differ} of {n0 + n1} elements differ from harp_adam_apply")
        assert differ == 0, (name, differ)
