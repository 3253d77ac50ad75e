"""-m gpu: the UV bake (csrc/bake.hip, harp_amd/bake.py) against the float64 restatement tests/_bake_ref.py: the texel map on dyadic
atlases (exact) and on the hand template, the accumulation on small quad scenes that hit every accept / reject branch, chunking and
repetition bit for bit, the dilation (exact: the reference runs in float32 with the kernel's summation order), the whole pipeline on the
synthetic hand, the initialisation inside a fit, and the evaluation / export switches."""
import os

import numpy as np
import pytest
import torch

from tests import _bake_cases as C
from tests import _bake_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ACC_KEYS = ("sum_w", "sum_wc", "sum_wc2", "count", "best_cos")


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


# ---- texel map
@pytest.mark.parametrize("Ht,Wt", C.UV_ATLASES)
def test_texel_map_dyadic_atlases_exact(Ht, Wt):
    """every coordinate and edge function of these cases is exact in float32 (tests/test_bake_cpu.py checks the premise), so the owner of
    EVERY texel — on shared edges and vertices, under a zero-area face, across the atlas border, in overlapping charts — must equal the
    reference's, and the barycentrics agree to float32 rounding"""
    from harp_amd import ops
    for name in C.UV_CASES:
        vu, fu = C.uv_case(name)
        want_f, want_b, _ = R.texel_map(vu, fu, Ht, Wt)
        face, bary = ops.uv_texel_map(_dev(vu), _dev(fu), Ht, Wt)
        assert np.array_equal(face.cpu().numpy(), want_f), name
        assert np.abs(bary.cpu().numpy().astype(np.float64) - want_b).max() <= 2.0 ** -22, name
        assert (want_f >= 0).any(), name
    # the lowest index owns the shared diagonal whichever triangle comes first
    a = R.texel_map(*C.uv_case("shared_edge"), Ht, Wt)[0]
    b = R.texel_map(*C.uv_case("shared_edge_swapped"), Ht, Wt)[0]
    diag = np.array([a[Ht - 1 - k * (Ht - 1) // 16, k * (Wt - 1) // 16] for k in range(17)])
    assert (diag == 0).all() and (a != -1).all() and not np.array_equal(a, 1 - b)


@pytest.mark.parametrize("Ht,Wt", C.HAND_ATLASES)
def test_texel_map_hand_template(Ht, Wt):
    from harp_amd import ops
    vu, fu = C.hand_uvs()
    want_f, _, und = C.hand_texel_map(Ht, Wt)
    face, bary = ops.uv_texel_map(_dev(vu), _dev(fu), Ht, Wt)
    face, bary = face.cpu().numpy(), bary.cpu().numpy().astype(np.float64)
    assert np.array_equal(face[~und], want_f[~und])
    cov = face >= 0
    assert cov.sum() > 0.2 * Ht * Wt
    # sum b_i P_i falls on the texel centre: 1e-4 texel is more than 4x the float32 rounding of a coordinate <= 128 through three operations
    P = R.texel_coords(vu, Ht, Wt)[fu[face[cov]]]                                # (n,3,2)
    b = np.concatenate([bary[cov], 1.0 - bary[cov].sum(1, keepdims=True)], 1)
    ys, xs = np.nonzero(cov)
    err = np.abs((b[:, :, None] * P).sum(1) - np.stack([xs, ys], 1)).max()
    print(f"[bake] hand template {Ht} x {Wt}: {cov.sum()} covered, {und.sum()} undecidable, max |sum b_i P_i - centre| = {err:.2e} texel")
    assert err <= 1e-4
    assert (b >= -1e-4).all()


# ---- accumulation
def _run_accum(case, frames=None, texel_idx=None, acc=None):
    from harp_amd import ops
    sl = slice(None) if frames is None else frames
    per_frame = ("ndc", "face_id", "zbuf", "rows", "verts", "vnormals", "cam_pos", "light_pos", "colors")
    kw = {k: _dev(case[k][sl] if (k in per_frame and case[k] is not None) else case[k]) for k in C.ACCUM_KEYS}
    acc = ops.bake_accumulators(C.HT, C.WT, DEV) if acc is None else acc
    return ops.texture_bake_accum(acc, texel_idx=texel_idx, **kw)


def _rel_to_sum_w(got, want, ok):
    """largest |got - want| / sum_w per accumulator over the decided texels the reference observed (sum_w > 0; the smallest weight of
    one observation is cos_min^2 = 0.04); where the reference's sum_w is 0 all three sums must be exactly 0"""
    pos = ok & (want["sum_w"] > 0)
    zero = ok & ~(want["sum_w"] > 0)
    for k in ("sum_w", "sum_wc", "sum_wc2"):
        assert (got[k][zero] == 0).all() and (want[k][zero] == 0).all(), k
    w = want["sum_w"][pos]
    return {k: (np.abs(got[k] - want[k])[pos] / (w if k == "sum_w" else w[:, None])).max() for k in ("sum_w", "sum_wc", "sum_wc2")}


@pytest.mark.parametrize("name", list(C.ACCUM_CASES))
def test_accumulate_against_float64(name):
    """Tolerances are the project's own: sums within 1e-5 relative to the texel's sum_w (the loss tolerance of DESIGN §7; exactly 0 where the
    reference's sum_w is 0), the mean within 1e-4 (the
    image tolerance of shade_common.h); count / seen exact.  Texels with an undecidable (texel, frame) pair are left out (<= 2 % of the
    observed ones, tests/test_bake_cpu.py).  The kernel evaluates a pair in float64 like the reference, so the measured differences are
    rounding-order noise."""
    from harp_amd import ops
    case = C.accum_case(name)
    want, info = C.accum_reference(name)
    for reason in case["expect"]:
        assert info["reasons"][reason] > 0 and info["observed"].any()
    acc = _run_accum(case)
    ok = ~info["undecided"].reshape(C.HT, C.WT)
    got = {k: acc[k].cpu().numpy() for k in ACC_KEYS}
    assert np.array_equal(got["count"][ok], want["count"][ok])
    errs = _rel_to_sum_w(got, want, ok)
    e_cos = np.abs(got["best_cos"] - want["best_cos"])[ok].max()
    mean, var, seen = (t.cpu().numpy() for t in ops.texture_bake_finish(acc))
    w_mean, w_var, w_seen = R.finish(want)
    e_mean, e_var = np.abs(mean - w_mean)[ok].max(), np.abs(var - w_var)[ok].max()
    print(f"[bake] {name}: {int(w_seen.sum())} seen, {int((~ok).sum())} left out; rel. errors {errs}, best_cos {e_cos:.1e}, mean {e_mean:.1e}, var {e_var:.1e}")
    assert np.array_equal(seen[ok], w_seen[ok]) and w_seen.sum() >= 50
    assert max(errs.values()) <= 1e-5 and e_cos <= 1e-6
    assert e_mean <= 1e-4 and e_var <= 1e-4
    assert (mean[seen == 0] == 0).all() and (var[seen == 0] == 0).all()
    # the compacted list of covered texels gives the same bits as all texels
    idx = torch.nonzero(_dev(case["texel_face"]).reshape(-1) >= 0)[:, 0].to(torch.int32)
    acc_idx = _run_accum(case, texel_idx=idx)
    for k in ACC_KEYS:
        assert torch.equal(acc_idx[k], acc[k]), k


def test_chunking_and_repetition_bit_for_bit():
    case = C.accum_case("raw")                                                   # six frames
    assert case["B"] == 6
    runs = []
    for cuts in ([slice(0, 6)], [slice(0, 3), slice(3, 6)], [slice(k, k + 1) for k in range(6)], [slice(0, 6)]):
        acc = None
        for sl in cuts:
            acc = _run_accum(case, frames=sl, acc=acc)
        runs.append(acc)
    for other in runs[1:]:
        for k in ACC_KEYS:
            assert torch.equal(runs[0][k], other[k]), k
    assert int(runs[0]["count"].max()) == 6


# ---- dilation
@pytest.mark.parametrize("Ht,Wt", C.UV_ATLASES)
@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_dilate_exact(Ht, Wt, Cn):
    """exact: the reference sums the valid neighbours in float32 in the kernel's order (row-major window) and divides once, correctly
    rounded on both sides.  Neither atlas is a multiple of the 256-thread workgroup."""
    from harp_amd import ops
    for kind in ("blob", "wall", "speckle"):
        tex, valid, allow = C.dilate_case(Ht, Wt, Cn, kind)
        for n_pass in (0, 1, 5):
            want, want_v = R.dilate(tex, valid, n_pass, allow)
            t = _dev(tex)
            out, v = ops.texture_dilate(t, _dev(valid), n_pass, allow=_dev(allow))
            assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(v.cpu().numpy(), want_v), (kind, n_pass)
            assert np.array_equal(t.cpu().numpy(), tex)                          # the input is left alone
            alias, _ = ops.texture_dilate(t, _dev(valid), n_pass, allow=_dev(allow), out=t)
            assert alias.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), want), (kind, n_pass, "out = tex")
            keep = want_v == 0
            assert np.array_equal(want[keep], tex[keep])                         # still invalid: the input value
            if kind == "blob" and n_pass == 5:                                   # a hole wider than 2 n_pass: far texels keep their value
                assert keep.sum() > 0 and want_v.sum() > valid.sum()
            if kind == "wall" and Ht >= 5:                                       # nothing crosses the wall
                assert (want_v[:, 8:] == 0).all() and (want_v[:, :8] == 1).all() == (n_pass >= 5)


def test_dilate_and_finish_refusals_on_real_buffers():
    """the refusals whose grid would not be empty, on real buffers: status 1 and nothing written"""
    from harp_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    tex = torch.rand(6, 7, 5, device=DEV)                                        # room for C = 5
    valid = torch.zeros(6, 7, dtype=torch.uint8, device=DEV)
    valid[2, 3] = 1
    out = torch.full_like(tex, -7.0)
    ws = torch.empty(L.harp_texture_dilate_ws_bytes(6, 7, 4) * 2, dtype=torch.uint8, device=DEV)
    for Cn, n_pass in [(0, 1), (5, 1), (-1, 1), (3, -1)]:
        assert L.harp_texture_dilate(p(tex), p(valid), None, 6, 7, Cn, n_pass, p(out), None, p(ws), _lib.stream()) == 1, (Cn, n_pass)
    acc = {k: torch.zeros(s, dtype=torch.float64, device=DEV) for k, s in (("w", (6, 7)), ("c", (6, 7, 3)), ("c2", (6, 7, 3)))}
    cnt = torch.zeros(6, 7, dtype=torch.int32, device=DEV)
    seen = torch.full((6, 7), 9, dtype=torch.uint8, device=DEV)
    for Ht, Wt in [(0, 7), (6, 0), (-1, 7)]:
        assert L.harp_texture_bake_finish(p(acc["w"]), p(acc["c"]), p(acc["c2"]), p(cnt), Ht, Wt, 1, p(out), None, p(seen), _lib.stream()) == 1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((seen == 9).all())


# ---- through the real pipeline
T_PIPE, S_PIPE = 3, 128
SKIN = (torch.tensor([232, 190, 172]) / 255.).numpy().astype(np.float64)       # optimize_sequence.py:234 as init_params forms it


def _smooth_texture():
    """a smooth texture far from the skin colour: two to three periods over the atlas"""
    v, u = np.meshgrid(np.arange(512) / 511.0, np.arange(512) / 511.0, indexing="ij")
    ch = [0.45 + 0.3 * np.sin(2 * np.pi * (fu * u + fv * v) + ph) for fu, fv, ph in ((2.0, 1.0, 0.3), (1.0, 2.5, 1.7), (3.0, 0.5, 4.0))]
    return torch.from_numpy(np.stack(ch, -1)[None]).float()


@pytest.fixture(scope="module")
def pipe(tmp_path_factory):
    """synthetic hand, targets rendered by the mirror from the smooth texture (self-shadow off); the fit's initial state otherwise"""
    from harp_amd.optimize_sequence import get_mesh_subdivider, mirror_render
    from tests._scene import erode
    from tests.test_gpu_evaluate import _setup
    tmp = tmp_path_factory.mktemp("bake")
    sc, cfg, layer, params, _ = _setup(T_PIPE, S_PIPE, 41, tmp, self_shadow=False, total_epoch=3, training_stage=[1, 2, 0])
    gt = _smooth_texture().to(DEV)
    with torch.no_grad():
        params["trans"].copy_(sc["seq"]["trans"])                                # the scene's own track: what a fit starts from
        params["light_positions"].copy_(torch.tensor((-0.5, -0.5, -0.5)).repeat(T_PIPE, 1))
        params["texture"].copy_(gt)
        P = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in params.items()}
        r = mirror_render(cfg, P, torch.arange(T_PIPE), layer, get_mesh_subdivider(layer, device=DEV), device=DEV)
        y_true, y_sil = r.y_pred.clone(), (r.y_sil_pred >= 0.5).float()
        y_col = erode(y_sil)
        params["texture"].copy_((torch.tensor([232, 190, 172]) / 255.).repeat(1, 512, 512, 1))
    ds = [(i, y_true[i].cpu(), y_sil[i][..., None].cpu(), y_col[i][..., None].cpu()) for i in range(T_PIPE)]
    return dict(sc=sc, cfg=cfg, layer=layer, params=params, ds=ds, gt=gt[0], tmp=tmp)


def test_bake_texture_through_the_pipeline(pipe):
    """bake_texture equals the reference fed with the same GPU face_id / zbuf / ndc (under the accumulate cap), and the baked albedo finds
    the texture the targets were rendered from: no worse than the reference's own round trip x 1.05 + 1e-4, which itself must beat the
    flat skin-colour initialisation threefold (a flipped u, v, x or y, shared by kernel and reference, would fail this)."""
    from harp_amd import bake as hbake, ops
    calls, real = [], ops.texture_bake_accum
    try:                                                                         # the one accumulate call's inputs, as the kernel receives them
        ops.texture_bake_accum = lambda acc, **kw: (calls.append(kw), real(acc, **kw))[1]
        out = hbake.bake_texture(pipe["cfg"], pipe["params"], pipe["ds"], pipe["layer"], device=DEV)
        acc, _ = hbake.bake_accumulate(pipe["cfg"], pipe["params"], pipe["ds"], pipe["layer"], device=DEV)
    finally:
        ops.texture_bake_accum = real
    assert len(calls) == 2 and out["texture"].shape == (1, 512, 512, 3)
    np_ = lambda t: None if t is None else t.detach().cpu().numpy()             # noqa: E731
    assert torch.equal(acc["count"], out["count"]) and torch.equal(acc["sum_w"], out["weight"])      # a repeated bake: the same bits
    call = {k: np_(v) if torch.is_tensor(v) else v for k, v in calls[0].items()}
    want = R.new_accumulators(512, 512)
    info = R.accumulate(want, **call)
    und = np.zeros(512 * 512, dtype=bool)
    und[info["texels"]] = info["undecided"]
    ok = ~und.reshape(512, 512)
    seen_any = np.zeros(512 * 512, dtype=bool)
    seen_any[info["texels"]] = info["observed"].any(0)
    share = (und & seen_any).sum() / seen_any.sum()
    w_mean, w_var, w_seen = R.finish(want)
    count, mean, var, seen = np_(out["count"]), np_(out["mean"]), np_(out["variance"]), np_(out["seen"])
    errs = _rel_to_sum_w({k: np_(acc[k]) for k in ACC_KEYS}, want, ok)
    e_w = max(errs.values())
    e_cos = np.abs(np_(acc["best_cos"]) - want["best_cos"])[ok].max()
    e_mean, e_var = np.abs(mean - w_mean)[ok].max(), np.abs(var - w_var)[ok].max()
    gt = np_(pipe["gt"]).astype(np.float64)
    rt_gpu = np.abs(mean - gt)[seen].mean()
    rt_ref = np.abs(w_mean - gt)[w_seen != 0].mean()
    rt_flat = np.abs(SKIN[None] - gt[w_seen != 0]).mean()
    print(f"[bake] pipeline: {int(w_seen.sum())} texels seen of {int(np_(out['covered']).sum())} covered (coverage {out['coverage']:.3f}), "
          f"{int(und.sum())} undecidable ({share:.2%}); sums rel. to sum_w {errs}, best_cos {e_cos:.1e}, mean {e_mean:.1e}, var {e_var:.1e}; round trip gpu {rt_gpu:.4f} ref {rt_ref:.4f} flat {rt_flat:.4f}")
    assert share <= 0.02 and w_seen.sum() > 5000
    assert np.array_equal(count[ok], want["count"][ok]) and np.array_equal(seen[ok], w_seen[ok] != 0)
    assert e_w <= 1e-5 and e_cos <= 1e-6 and e_mean <= 1e-4 and e_var <= 1e-4
    assert rt_ref < rt_flat / 3.0
    assert rt_gpu <= rt_ref * 1.05 + 1e-4
    # the returned texture: the mean where seen inside the mask, the input colour outside the charts
    tex, covered, uvm = np_(out["texture"])[0], np_(out["covered"]), np_(pipe["sc"]["uv_mask"]) > 0.5
    assert np.array_equal(tex[seen & uvm], mean[seen & uvm])
    assert np.abs(tex[~(covered & uvm)] - SKIN.astype(np.float32)).max() < 1e-6
    assert 0.0 < out["coverage"] <= 1.0


def test_texture_init_in_a_fit(pipe):
    """epoch 0 is coarse only, epoch 1 the first appearance epoch: with texture_init="bake" its mean loss is strictly lower, and the
    texture is still the initial colour, bit for bit, after epoch 0"""
    from harp_amd.optimize_sequence import optimize_hand_sequence
    sc, cfg, layer, ds = pipe["sc"], pipe["cfg"], pipe["layer"], pipe["ds"]
    uvs = (torch.from_numpy(sc["tpl"]["verts_uvs"])[None], torch.from_numpy(sc["tpl"]["faces_uvs"])[None])
    losses, flat_after_0 = {}, {}
    for mode in (None, "bake"):
        log = []

        def log_fn(epoch_id, loss, eng, log=log):
            t = eng.params["texture"]
            log.append((loss, bool(torch.equal(t, t[:, :1, :1].expand_as(t))), t[0, 0, 0].cpu().numpy()))
        base = str(pipe["tmp"]) + f"/fit_{mode}/"
        os.makedirs(base, exist_ok=True)
        out = optimize_hand_sequence(dict(cfg, base_output_dir=base), sc["seq"], ds, None, None, layer, *uvs, device=DEV,
                                     uv_mask=sc["uv_mask"], batch_size=T_PIPE, log_fn=log_fn, texture_init=mode)
        losses[mode], flat_after_0[mode] = [e[0] for e in log], log[0][1]
        assert np.array_equal(log[0][2], (torch.tensor([232, 190, 172]) / 255.).numpy())
        assert (log[1][1] is False) if mode else True                            # after epoch 1 the baked run's texture is no longer flat
        assert torch.isfinite(out["texture"]).all()
    print(f"[bake] fit: epoch losses without {losses[None]}, with bake {losses['bake']}")
    assert flat_after_0[None] and flat_after_0["bake"]
    assert losses["bake"][1] < losses[None][1]


@pytest.mark.filterwarnings("ignore:MS_SSIM left out")
def test_evaluate_coverage_and_padded_export(pipe):
    from PIL import Image
    from harp_amd.io import encode_png
    from harp_amd.optimize_sequence import evaluate_sequence
    cfg, layer, ds, sc = pipe["cfg"], pipe["layer"], pipe["ds"], pipe["sc"]
    uvm = (sc["uv_mask"] > 0.5).numpy()
    params = dict(pipe["params"])
    tex = pipe["gt"].clone()
    tex[torch.from_numpy(~uvm).to(DEV)] = 0.0                                    # black outside the charts, as a viewer would meet it
    params["texture"] = tex[None]
    runs = {}
    for tag, kw in (("plain", dict(export_mesh=True)), ("cov", dict(coverage=True, export_mesh=True, pad_texture=4))):
        base = str(pipe["tmp"]) + f"/eval_{tag}/"
        os.makedirs(base, exist_ok=True)
        stats = evaluate_sequence(dict(cfg, base_output_dir=base), params, ds, layer, device=DEV, **kw)
        runs[tag] = (base, stats, open(base + "eval_results.txt").read().splitlines())
    base, stats, lines = runs["plain"]
    assert list(stats) == ["Silhouette IoU", "L1"] and [ln.split(":")[0] for ln in lines] == [" Silhouette IoU", " L1"]
    assert not any(os.path.exists(base + "uv_out/" + f) for f in ("coverage.png", "baked_texture.png", "texture_std.png"))
    assert open(base + "mesh/0000.png", "rb").read() == encode_png(tex.cpu().clamp(0, 1))          # pad_texture = 0: the old bytes
    base, stats, lines = runs["cov"]
    assert list(stats) == ["Silhouette IoU", "L1", "Texel coverage"] and lines[-1] == " Texel coverage: %.5f" % stats["Texel coverage"]
    assert lines[:-1] == runs["plain"][2] and 0.0 < stats["Texel coverage"] <= 1.0
    for f, mode in (("coverage.png", "L"), ("baked_texture.png", "RGB"), ("texture_std.png", "RGB")):
        im = Image.open(base + "uv_out/" + f)
        assert im.size == (512, 512) and im.mode == mode, f
    cov = np.asarray(Image.open(base + "uv_out/coverage.png"))
    assert cov.max() == T_PIPE and (cov > 0).sum() > 5000
    # every texel within 4 of uv_mask is non-black in the exported PNG; the texels of the mask are unchanged
    png = np.asarray(Image.open(base + "mesh/0000.png").convert("RGB"))
    near = torch.nn.functional.max_pool2d(torch.from_numpy(uvm).float()[None, None], 9, stride=1, padding=4)[0, 0].numpy() > 0
    assert (png[near].max(-1) > 0).all() and (near & ~uvm).sum() > 1000
    plain = np.asarray(Image.open(runs["plain"][0] + "mesh/0000.png").convert("RGB"))
    assert np.array_equal(png[uvm], plain[uvm]) and (plain[near & ~uvm] == 0).all()
