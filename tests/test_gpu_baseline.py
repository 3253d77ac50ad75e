"""-m gpu parity at the BASELINE.json sizes and configurations, HIP path vs the CPU oracle evaluated in FLOAT64 on the
same inputs (so the comparison is against the mathematically exact result, not against another fp32 rounding of it):

  C2/C3  512x512, subdivided MANO hand, all terms, B = 2 — both image modes (keep_image / loss-only)
  C2     the reference's batch size B = 18 (optimize_sequence.py:396) at 128x128 (with a ragged tail) and at 512x512 (all gradients)
  C3     B = 32 at 512x512, all gradients (masked + unmasked companion)
  C5     1024x1024, SMPL-X arm mesh (4083 v / 8128 f), B = 1 — loss-only mode (what an 8-GPU job runs per rank); B = 8 through the
         striding kernels, all gradients; B = 32 against the plain grid
  C1     single 256x256 frame, RAW 778-vertex / 1538-face MANO mesh, silhouette loss only — through the engine and through the
         reference API (prepare_mesh(mesh_subdivider=None) -> silhouette renderer)
  off the tile grid: S = 300 / 301 / 448 / 200 (hand) and 520 (arm), where the last 16-px tile and 64-px super-tile are partial
  10 Adam steps vs torch.optim.Adam on the oracle; the appearance-only stage's geometry gradients (barycentric path of the shader backward)

Tolerances are SURVEY.md §8(d)'s: images |d| <= 1e-4 on >= 99.9 % of the pixels, nearest-face ids identical except <= 1e-4 of the pixels,
scalar losses rel 1e-5, gradients rel-L2 <= 1e-3, parameters after 10 Adam steps rel-L2 <= 1e-3.  Pixels whose colour is not decided
at float32 precision (pixel centre on a face edge in either view, shadow-tap index on its rounding boundary: 1-2 % of the covered
pixels, flagged by the float64 oracle alone) are taken out of the photometric mask first — see tests/_scene.mask_ambiguous_pixels."""
import numpy as np
import pytest
import torch

from tests._scene import ORACLE_KEYS, check_removed, engine_eval, make_fit_case, mask_ambiguous_pixels, oracle_inputs, oracle_step, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_TOL = 1e-3
LOSS_TOL = 1e-5


def _check_losses(lv, loss, tol=LOSS_TOL):
    for k, v in loss.items():
        assert abs(lv[k] - v.item()) <= tol * abs(v.item()) + 1e-9, (k, lv[k], v.item())


def _check_grads(eng, P, keys, tol=GRAD_TOL, tag=""):
    worst = {}
    for k in keys:
        ref = P[k].grad
        if ref is None or ref.abs().max() == 0:
            assert eng.grads[k].abs().max().item() == 0, (tag, k, "expected an exactly zero gradient")
            continue
        worst[k] = rel(eng.grads[k].cpu().double(), ref)
    bad = {k: v for k, v in worst.items() if not v < tol}
    print(f"[gradient rel-L2 vs fp64 oracle] {tag}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert not bad, (tag, bad, worst)
    return worst


def _check_images(eng, aux, n):
    a = eng.s["alpha"][:n].cpu().double()
    assert ((a - aux["y_sil_pred"]).abs() > 1e-4).float().mean() < 1e-3
    rgb = eng.s["rgb"][:n].cpu().double()
    assert ((rgb - aux["y_pred"]).abs().max(-1).values > 1e-4).float().mean() < 1e-3


@pytest.mark.parametrize("keep_image", [True, False])
def test_c2_c3_hand_512_b2_vs_fp64_oracle(keep_image):
    case = make_fit_case("hand", T=2, S=512, B=2, seed=0, device=DEV)
    eng = case["eng"]
    check_removed("c2c3_hand_512_b2", mask_ambiguous_pixels(case))
    eng.keep_image = keep_image
    eng.draw_texture_offsets()
    fid = torch.tensor([1, 0])
    lv = engine_eval(case, fid)
    P, loss, total, aux, _ = oracle_step(case, fid)
    _check_losses(lv, loss)
    if keep_image:
        _check_images(eng, aux, 2)
        cov = (eng.s["face_c"][:2] >= 0).float().mean().item()
        assert 0.05 < cov < 0.6
    keys = [k for k in ORACLE_KEYS if k != "wrist_pose"]
    _check_grads(eng, P, keys, tag=f"512 hand keep_image={keep_image}")


def test_c2_c3_hand_512_b2_unmasked_companion():
    """The same inputs as test_c2_c3_hand_512_b2_vs_fp64_oracle with NO pixel taken out of the photometric mask: what the mask removes is
    bounded, not ignored.  The image criterion is unchanged (|d| <= 1e-4 on >= 99.9 % of the pixels); losses
    rel 1e-4 (one pixel whose shadow tap rounds the other way moves the photometric mean by ~1e-5 relative) and gradients rel-L2
    <= 5e-3 (measured: <= 1.2e-3, texture; the masked run: <= 3e-4): a pixel float32 cannot decide moves a gradient by
    ~1/sqrt(#pixels) — the float32 ORACLE differs from the float64 one by 2e-3 on the same inputs — so an error CONFINED to edge /
    texel-boundary / tap-boundary pixels larger than that still fails here."""
    case = make_fit_case("hand", T=2, S=512, B=2, seed=0, device=DEV)
    eng = case["eng"]
    eng.draw_texture_offsets()
    fid = torch.tensor([1, 0])
    P, loss, total, aux, _ = oracle_step(case, fid)
    keys = [k for k in ORACLE_KEYS if k != "wrist_pose"]
    for keep in (True, False):
        eng.keep_image = keep
        lv = engine_eval(case, fid)
        _check_losses(lv, loss, tol=1e-4)
        if keep:
            _check_images(eng, aux, 2)
        _check_grads(eng, P, keys, tol=5e-3, tag=f"512 hand UNMASKED keep_image={keep}")


# Image sizes off the tile grid: the last 16-px tile and 64-px super-tile of every row / column are partial (the in-image guards, clamped
# shadow taps, window flushes near S - 1 and per-tile flag indexing of every kernel of the step).  (kind, S, B, seed, stages, variants):
# every stage (coarse, app) is one oracle evaluation that all engine variants (keep_image, light-view tile flags, HARP_RASTER_LOOP) meet.
_FULL, _GEOM, _APP = (True, True), (True, False), (False, True)
OFF_GRID = {
    "hand_300_b2": ("hand", 300, 2, 0, (_FULL,), [(k, f, l) for l in (0, 16) for f in (False, True) for k in (True, False) if not (f and l)]),
    "hand_301_b1": ("hand", 301, 1, 1, (_FULL,), [(True, False, 0), (False, False, 0)]),        # odd: a pixel centre on NDC 0
    "hand_448_b2": ("hand", 448, 2, 2, (_FULL,), [(True, False, 0), (False, False, 0)]),        # the reference's img_size (optimize_sequence.py:352)
    "hand_200_b3": ("hand", 200, 3, 3, (_GEOM, _APP), [(True, False, 0), (False, False, 0)]),
    "arm_520_b1": ("arm", 520, 1, 0, (_FULL,), [(True, False, 0), (False, False, 0)]),
}


@pytest.mark.parametrize("name", list(OFF_GRID))
def test_step_off_the_tile_grid_vs_fp64_oracle(name, monkeypatch):
    """The whole step at image sizes that are no multiple of 16 or 64 (S = 300, 301, 448, 200, 520) against the float64 oracle: every loss
    term (rel 1e-5), the image (SURVEY.md §8d criterion) and every gradient (rel-L2 <= 1e-3), float32-undecidable pixels out of the mask as
    everywhere.  Variants (keep_image, zl_tile_flags, raster loop): zl_tile_flags = True puts the light-view tile flags ((S + 15) >> 4 a
    side; on by default only at S >= 1024) on partial tiles; HARP_RASTER_LOOP=16 runs the striding raster / depth-backward kernels over
    ragged super-tiles."""
    kind, S, B, seed, stages, variants = OFF_GRID[name]
    case = make_fit_case(kind, T=B, S=S, B=B, seed=seed, device=DEV)
    eng = case["eng"]
    if S % 8:      # the engine's HIP perceptual term tiles the image by 8: refused at the call, before it changes anything
        from harp_amd.model.vgg import Vgg16Features
        with pytest.raises(ValueError, match=f"image size {S} "):
            eng.set_perceptual(Vgg16Features(weights="random"))
        assert eng.perceptual is None
    check_removed(f"offgrid_{name}", mask_ambiguous_pixels(case))
    eng.draw_texture_offsets()
    fid = torch.arange(B).flip(0)
    keys = [k for k in ORACLE_KEYS if kind == "arm" or k != "wrist_pose"]
    for coarse, app in stages:
        P, loss, total, aux, _ = oracle_step(case, fid, coarse=coarse, app=app)
        for keep, zl_flags, loop in variants:
            eng.keep_image, eng.zl_tile_flags = keep, zl_flags
            if loop:
                monkeypatch.setenv("HARP_RASTER_LOOP", str(loop))
            else:
                monkeypatch.delenv("HARP_RASTER_LOOP", raising=False)
            lv = engine_eval(case, fid, coarse=coarse, app=app)
            _check_losses(lv, loss)
            if keep and coarse and app:
                _check_images(eng, aux, B)
            elif keep and coarse:            # (the geometry-only stage shades nothing)
                a = eng.s["alpha"][:B].cpu().double()
                assert ((a - aux["y_sil_pred"]).abs() > 1e-4).float().mean() < 1e-3
            elif keep:
                rgb = eng.s["rgb"][:B].cpu().double()
                assert ((rgb - aux["y_pred"]).abs().max(-1).values > 1e-4).float().mean() < 1e-3
            _check_grads(eng, P, keys, tag=f"{name} coarse={coarse} app={app} keep_image={keep} zl_tile_flags={zl_flags} raster_loop={loop}")
    monkeypatch.delenv("HARP_RASTER_LOOP", raising=False)


def test_step_off_the_tile_grid_unmasked_companion():
    """test_step_off_the_tile_grid_vs_fp64_oracle[hand_300_b2] with NO pixel taken out of the photometric mask, at the tolerances of
    test_c2_c3_hand_512_b2_unmasked_companion (losses rel 1e-4, gradients rel-L2 <= 5e-3): the mask bounds the edge pixels of the partial
    tiles, it does not hide them."""
    case = make_fit_case("hand", T=2, S=300, B=2, seed=0, device=DEV)
    eng = case["eng"]
    eng.draw_texture_offsets()
    fid = torch.tensor([1, 0])
    P, loss, total, aux, _ = oracle_step(case, fid)
    keys = [k for k in ORACLE_KEYS if k != "wrist_pose"]
    for keep in (True, False):
        eng.keep_image = keep
        lv = engine_eval(case, fid)
        _check_losses(lv, loss, tol=1e-4)
        if keep:
            _check_images(eng, aux, 2)
        _check_grads(eng, P, keys, tol=5e-3, tag=f"300 hand UNMASKED keep_image={keep}")


def test_c2_reference_batch_18():
    """B = 18 (the reference's DataLoader batch, optimize_sequence.py:396) incl. a partial last batch of 36 % 18 ... = here 7 frames"""
    case = make_fit_case("hand", T=25, S=128, B=18, seed=1, device=DEV)
    eng = case["eng"]
    check_removed("c2_hand_128_b18", mask_ambiguous_pixels(case))
    eng.keep_image = False
    eng.draw_texture_offsets()
    for fid in (torch.arange(18), torch.arange(18, 25)):          # full batch, then the ragged tail (runs with B = 7)
        lv = engine_eval(case, fid)
        P, loss, total, aux, _ = oracle_step(case, fid)
        _check_losses(lv, loss)
        _check_grads(eng, P, [k for k in ORACLE_KEYS if k != "wrist_pose"], tag=f"B={len(fid)}")


def test_c5_arm_1024_b1_vs_fp64_oracle():
    case = make_fit_case("arm", T=1, S=1024, B=1, seed=0, device=DEV)
    eng = case["eng"]
    check_removed("c5_arm_1024_b1", mask_ambiguous_pixels(case))
    eng.draw_texture_offsets()
    fid = torch.tensor([0])
    P, loss, total, aux, _ = oracle_step(case, fid)
    for keep in (True, False):
        eng.keep_image = keep
        lv = engine_eval(case, fid)
        _check_losses(lv, loss)
        if keep:
            _check_images(eng, aux, 1)
            assert 0.02 < (eng.s["face_c"][:1] >= 0).float().mean().item() < 0.9
        _check_grads(eng, P, ORACLE_KEYS, tag=f"1024 arm keep_image={keep}")


def test_c5_arm_1024_b32_through_the_striding_kernels(monkeypatch):
    """C5 at its real per-GPU batch: 32 frames of the SMPL-X arm mesh at 1024x1024 = 131 072 tile workgroups per launch, above the 64 k
    limit where the rasteriser kernels switch to the capped, striding grid (csrc/raster.hip, raster_kernel<*, true>; depth backward).
    (i) Oracle parity on 2 of the 32 frames: every loss term that reaches a per-frame parameter row (pose, cam, rot, trans, wrist_pose)
    is a mean over the batch of per-frame terms, so row f of the batch gradient x 32 is the gradient of the ONE-frame step on frame f,
    which the float64 oracle evaluates (rel-L2 <= 1e-3, the two frames' float32-undecidable pixels out of the mask as everywhere).
    (ii) The whole batch against the same launch forced onto the plain 131 072-workgroup grid (HARP_RASTER_LOOP=0): losses and every
    gradient agree up to the order of the float atomics.  (iii) Size-independent properties of all 32 frames."""
    from tests._scene import ambiguous_pixels
    T = B = 32
    case = make_fit_case("arm", T=T, S=1024, B=B, seed=0, device=DEV)
    eng = case["eng"]
    assert B * (1024 // 64) ** 2 * 16 > 65536               # tile_grid(B, nsx): the striding kernels are what runs by default
    frames = (3, 17)
    P, model, targets = oracle_inputs(case, torch.float64)
    y_col = case["targets"]["y_sil_col"].clone()
    removed = []
    for f in frames:
        amb, aux = ambiguous_pixels(P, model, case["topo"], 1024, case["focal"], [f], targets["y_true"], use_arm=True)
        y_col[f][amb[0]] = 0.0
        removed.append(amb.sum().item() / max((aux["pix_to_face"][..., 0] >= 0).sum().item(), 1))
    check_removed("c5_arm_1024_b32", max(removed))
    case["targets"]["y_sil_col"] = y_col
    eng.set_targets(case["targets"]["y_true"], case["targets"]["y_sil"], y_col)
    eng.draw_texture_offsets()
    fid = torch.arange(T)
    res = {}
    for mode in (None, "0"):
        if mode is None:
            monkeypatch.delenv("HARP_RASTER_LOOP", raising=False)
        else:
            monkeypatch.setenv("HARP_RASTER_LOOP", mode)
        for keep in (True, False):
            eng.keep_image = keep
            lv = engine_eval(case, fid)
            res[(mode, keep)] = (lv, eng.g_buf.clone())
            if mode is None and keep:
                a, fc, rgb = eng.s["alpha"], eng.s["face_c"], eng.s["rgb"]
                assert (a >= 0).all() and (a <= 1).all() and (fc >= -1).all() and (fc < eng.topo.F).all()
                cov = fc >= 0
                assert 0.02 < cov.float().mean().item() < 0.9 and (a[cov] > 0.49).all() and (rgb[~cov] == 1.0).all()
                assert torch.isfinite(rgb).all() and torch.isfinite(eng.g_buf).all() and all(np.isfinite(v) for v in lv.values())
    monkeypatch.delenv("HARP_RASTER_LOOP", raising=False)
    ref_l, ref_g = res[("0", True)]
    for key, (lv, g) in res.items():
        for k, v in ref_l.items():       # (float32 atomics over 131 072 workgroup partial sums in another order: LOSS_TOL, not bit-for-bit)
            assert abs(v - lv[k]) <= LOSS_TOL * abs(v) + 1e-12, (key, k, v, lv[k])
        assert rel(g.cpu(), ref_g.cpu()) < 1e-4, key       # float atomics of 33 M pixels in another order (measured 2e-5)
    # (i) per-frame rows against the float64 oracle's one-frame steps
    eng.keep_image = False
    engine_eval(case, fid)
    rows = ("pose", "cam", "rot", "trans", "wrist_pose")
    got = {k: eng.grads[k].detach().cpu().double().clone() for k in rows}
    targets["y_sil_col"] = y_col.double()
    for f in frames:
        for k in ORACLE_KEYS:
            P[k].grad = None
        oracle_step(case, torch.tensor([f]), P=P, model=model, targets=targets)
        worst = {k: rel(got[k][f] * B, P[k].grad[f]) for k in rows}
        print(f"[gradient rel-L2 vs fp64 oracle] C5 B=32 frame {f}:", {k: f"{v:.1e}" for k, v in worst.items()})
        assert all(v < GRAD_TOL for v in worst.values()), (f, worst)


def _batch_all_gradients(kind, T, S, tag, mask_tag, seed, keeps=(True, False), unmasked_tol=None, sub_batch=None):
    """ONE step over T = B frames, EVERY gradient against the float64 oracle — the per-frame rows (pose, cam, rot, trans[, wrist_pose]) and
    the shared parameters on which all frames' atomics land (texture, normal_map, verts_disps, shape, light_positions, amb_ratio).  The
    oracle is linear in the frames: every image / mesh term is a mean over the batch of per-frame terms and the regularisers do not depend
    on the frames, so the batch objective is the average of the T one-frame objectives; it is evaluated frame by frame (K=50 fragments of
    ONE frame at a time) and the gradients accumulate.  Float32-undecidable pixels of all frames are out of the mask (both sides);
    unmasked_tol: afterwards the same comparison with NO pixel removed, at that looser gradient bound (losses rel 1e-4).
    sub_batch = (n, tag, mask_tag): the FIRST n frames as a step of their own (the engine runs a shorter batch of the same buffers), against the
    oracle's sums over those n frames — the frames are evaluated once and serve both batch sizes."""
    from oracle import harp_ref as H
    import torch.nn.functional as F
    B = T
    use_arm = kind == "arm"
    case = make_fit_case(kind, T=T, S=S, B=B, seed=seed, device=DEV)
    eng = case["eng"]
    P, model, targets = oracle_inputs(case, torch.float64)
    y_col_full = case["targets"]["y_sil_col"].clone()
    y_col = y_col_full.clone()
    fid = torch.arange(T)
    keys = [k for k in ORACLE_KEYS if use_arm or k != "wrist_pose"]
    rows_keys = ("pose", "cam", "rot", "trans") + (("wrist_pose",) if use_arm else ())
    passes = (True, False) if unmasked_tol is not None else (True,)
    eng.auto_draw = False
    eng.draw_texture_offsets()                           # ONE draw for the oracle and both engine passes
    # ---- the oracle, ONE render per frame: it flags the float32-undecidable pixels of the frame (tests/_scene.py: ambiguous_pixels — the same
    #      flags from the same float64 forward pass, which used to be a second render), they leave the photometric mask of this evaluation
    #      and of the engine's masked pass; the unmasked objective differs from the masked one only in that mask, so its gradient is the
    #      masked one plus the gradient of  w_photo * (photo(full mask) - photo(masked))  through the same render
    for k in ORACLE_KEYS:
        P[k].grad = None
    rv = case.get(("ref_verts", torch.float64))
    if rv is None:
        with torch.no_grad():
            _, rv = H.prepare_mesh(P, torch.tensor([0]), model, case["topo"], use_arm=use_arm)
        case[("ref_verts", torch.float64)] = rv
    loss_sum, delta_grad, photo_full_sum = {}, {k: None for k in keys}, 0.0
    full64 = y_col_full.double()
    n_cov, counts = 0, [0]
    for f in range(T):                                                # .grad accumulates over the T one-frame steps
        def mask_from_render(y_pred, raux, col, f=f):
            amb = raux["ambiguous"] | ((y_pred - targets["y_true"][f:f + 1]).abs() < 3e-4).any(-1)      # (+ the kink of the L1 term)
            amb = amb & (raux["pix_to_face"][..., 0] >= 0)
            counts[0] += amb.sum().item()
            y_col[f][amb[0]] = 0.0
            out = col.clone()
            out[amb] = 0.0
            return out
        loss, total, aux = H.step_losses(P, torch.tensor([f]), model, case["topo"], targets, S, case["focal"], rv, eng.dist_albedo.cpu().long(),
                                         eng.dist_normal.cpu().long(), coarse=True, app=True, self_shadow=eng.self_shadow, use_arm=use_arm,
                                         mask_from_render=mask_from_render)
        n_cov += (aux["render_aux"]["pix_to_face"][..., 0] >= 0).sum().item()
        total.backward(retain_graph=unmasked_tol is not None)
        for k, v in loss.items():
            loss_sum[k] = loss_sum.get(k, 0.0) + v.item()
        if unmasked_tol is not None:
            m = full64[f].unsqueeze(0).unsqueeze(-1)
            photo_full = F.l1_loss(targets["y_true"][f:f + 1] * m, aux["y_pred"] * m)
            photo_full_sum += photo_full.item()
            gs = torch.autograd.grad(H.LOSS_WEIGHTS["photo"] * (photo_full - loss["photo"]), [P[k] for k in keys], allow_unused=True)
            for k, g_ in zip(keys, gs):
                if g_ is not None:
                    delta_grad[k] = g_.detach().clone() if delta_grad[k] is None else delta_grad[k] + g_
        del loss, total, aux
        if sub_batch is not None and f == sub_batch[0] - 1:
            snap = dict(grad={k: (None if P[k].grad is None else P[k].grad.detach().clone()) for k in keys}, loss=dict(loss_sum), removed=counts[0] / max(n_cov, 1))
    check_removed(mask_tag, counts[0] / max(n_cov, 1))
    # ---- the engine: the masked step and (unmasked_tol) the same step with NO pixel removed
    got, lvs = {}, {}
    for masked in passes:
        col = y_col if masked else y_col_full
        case["targets"]["y_sil_col"] = col
        eng.set_targets(case["targets"]["y_true"], case["targets"]["y_sil"], col)
        for keep in keeps:
            eng.keep_image = keep
            lvs[masked, keep] = engine_eval(case, fid)
            got[masked, keep] = {k: eng.grads[k].detach().cpu().double().clone() for k in keys}
            if keep:
                a, fc, rgb = eng.s["alpha"], eng.s["face_c"], eng.s["rgb"]
                cov = fc >= 0
                assert (a >= 0).all() and (a <= 1).all() and (fc >= -1).all() and (fc < eng.topo.F).all()
                assert 0.02 < cov.float().mean().item() < 0.9 and (a[cov] > 0.49).all() and (rgb[~cov] == 1.0).all()
                assert torch.isfinite(rgb).all() and torch.isfinite(eng.g_buf).all()
        for k, v in lvs[masked, keeps[0]].items():
            assert abs(v - lvs[masked, keeps[-1]][k]) <= LOSS_TOL * abs(v) + 1e-12, (k, v, lvs[masked, keeps[-1]][k])
    for masked in passes:
        gtol, ltol = (GRAD_TOL, LOSS_TOL) if masked else (unmasked_tol, 1e-4)
        want_loss = dict(loss_sum) if masked else dict(loss_sum, photo=photo_full_sum)
        want_grad = {}
        for k in keys:
            gk = P[k].grad
            if not masked and delta_grad[k] is not None:
                gk = delta_grad[k] if gk is None else gk + delta_grad[k]
            want_grad[k] = gk
        for keep in keeps:
            for k, v in want_loss.items():
                assert abs(lvs[masked, keep][k] - v / T) <= ltol * abs(v / T) + 1e-9, (k, keep, masked, lvs[masked, keep][k], v / T)
            worst = {}
            for k in keys:
                if want_grad[k] is None or want_grad[k].abs().max() == 0:
                    assert got[masked, keep][k].abs().max().item() == 0, (k, "expected an exactly zero gradient")
                    continue
                worst[k] = rel(got[masked, keep][k], want_grad[k] / T)
            print(f"[gradient rel-L2 vs fp64 oracle] {tag}, all parameters, {'masked' if masked else 'UNMASKED'}, keep_image={keep}:",
                  {k: f"{v:.1e}" for k, v in worst.items()})
            assert all(v < gtol for v in worst.values()), (keep, masked, worst)
            assert all(k in worst for k in ("pose", "cam", "verts_disps", "shape", "light_positions", "amb_ratio", "texture", "normal_map", "rot", "trans"))
            # per-frame rows frame by frame (a wrong frame index would average out of the whole-table norm above)
            for k in rows_keys:
                rows = torch.stack([(got[masked, keep][k][f] - want_grad[k][f] / T).norm() / (want_grad[k][f] / T).norm().clamp_min(1e-30) for f in range(T)])
                assert rows.max().item() < 2 * gtol, (k, keep, masked, rows.max().item(), int(rows.argmax()))
    if sub_batch is not None:
        # ---- the first n frames as ONE step of their own (loss-only mode, what a fit runs), against the oracle's sums over those n frames
        n, stag, smask = sub_batch
        check_removed(smask, snap["removed"])
        case["targets"]["y_sil_col"] = y_col
        eng.set_targets(case["targets"]["y_true"], case["targets"]["y_sil"], y_col)
        eng.keep_image = False
        lv = engine_eval(case, torch.arange(n))
        for k, v in snap["loss"].items():
            assert abs(lv[k] - v / n) <= LOSS_TOL * abs(v / n) + 1e-9, (stag, k, lv[k], v / n)
        worst = {}
        for k in keys:
            gk = snap["grad"][k]
            g_e = eng.grads[k].detach().cpu().double()
            if gk is None or gk.abs().max() == 0:
                assert g_e.abs().max().item() == 0, (stag, k, "expected an exactly zero gradient")
                continue
            worst[k] = rel(g_e, gk / n)
        print(f"[gradient rel-L2 vs fp64 oracle] {stag}, all parameters, masked, keep_image=False:", {k: f"{v:.1e}" for k, v in worst.items()})
        assert all(v < GRAD_TOL for v in worst.values()), (stag, worst)
        for k in rows_keys:
            g_e = eng.grads[k].detach().cpu().double()
            rows = torch.stack([(g_e[f] - snap["grad"][k][f] / n).norm() / (snap["grad"][k][f] / n).norm().clamp_min(1e-30) for f in range(n)])
            assert rows.max().item() < 2 * GRAD_TOL, (stag, k, rows.max().item(), int(rows.argmax()))
            assert g_e[n:].abs().max().item() == 0, (stag, k, "rows of frames outside the batch")


def test_c3_hand_512_b32_and_c2_b18_all_gradients_vs_fp64_oracle():
    """C3 at the batch the headline number is quoted on: 32 frames of the subdivided hand at 512x512 in ONE step (the bench workload), in
    both image modes; then the UNMASKED companion of the same step (no pixel out of the photometric mask) at the 5e-3 gradient bound of
    the other unmasked companions.
    C2 at the reference's DataLoader batch (B = 18, optimize_sequence.py:396) at the full 512x512 — the configuration bench.py only times
    (`extras`): the first 18 of the same frames as ONE step, every gradient against the oracle's sums over those 18 frames (loss-only mode,
    what a fit runs).  The float64 oracle renders each frame once for both batch sizes (it was 74 s of the suite for a scene of its own)."""
    _batch_all_gradients("hand", 32, 512, "C3 B=32 512x512", "c3_hand_512_b32", seed=2, unmasked_tol=5e-3,
                         sub_batch=(18, "C2 B=18 512x512", "c2_hand_512_b18"))


def test_c5_arm_1024_b8_all_gradients_through_the_striding_kernels(monkeypatch):
    """C5's shared-parameter gradients at 1024x1024 on the arm mesh THROUGH THE STRIDING KERNELS: 8 frames = 32 768 tile workgroups, below
    the 64 k switch-over, so the capped grid is forced (HARP_RASTER_LOOP=4096: every workgroup of the rasterisers / depth backward strides
    over 8 tiles, as at B = 32 where 131 072 tiles run on the default cap) — texture, normal_map, verts_disps, shape, light_positions,
    amb_ratio and every per-frame row against the float64 oracle, frame by frame.  (test_c5_arm_1024_b32_... checks the real B = 32 launch
    against the plain grid and 2 of its frames against the oracle.)"""
    monkeypatch.setenv("HARP_RASTER_LOOP", "4096")
    _batch_all_gradients("arm", 8, 1024, "C5 B=8 1024x1024 arm (striding grid)", "c5_arm_1024_b8", seed=1, keeps=(False, True))


def test_unmasked_companions_c5_arm_1024_and_appearance_only_stage():
    """Companions of test_c5_arm_1024_b1_vs_fp64_oracle and test_appearance_only_stage_geometry_gradients with NO pixel taken out of the
    photometric mask (like test_c2_c3_hand_512_b2_unmasked_companion): image criterion unchanged, losses rel 1e-4, gradients rel-L2
    <= 5e-3 (the appearance-only stage's geometry gradients: against the float32 oracle's own distance from the float64 result, see
    below) — what the ambiguous-pixel mask removes in those two cases is bounded, not ignored."""
    for tag, kind, S, coarse, keys in (("C5 arm 1024 B=1", "arm", 1024, True, ORACLE_KEYS),
                                       ("app-only hand 256 B=2", "hand", 256, False, [k for k in ORACLE_KEYS if k != "wrist_pose"])):
        n = 1 if kind == "arm" else 2
        case = make_fit_case(kind, T=n, S=S, B=n, seed=0 if kind == "arm" else 3, device=DEV)
        eng = case["eng"]
        eng.draw_texture_offsets()
        fid = torch.arange(n)
        P, loss, total, aux, _ = oracle_step(case, fid, coarse=coarse, app=True)
        o32 = None
        for keep in (True, False):
            eng.keep_image = keep
            lv = engine_eval(case, fid, coarse=coarse, app=True)
            _check_losses(lv, loss, tol=1e-4)
            if keep and coarse:
                _check_images(eng, aux, n)
            elif keep:
                rgb = eng.s["rgb"][:n].cpu().double()
                assert ((rgb - aux["y_pred"]).abs().max(-1).values > 1e-4).float().mean() < 1e-3
            if coarse:
                _check_grads(eng, P, keys, tol=5e-3, tag=f"{tag} UNMASKED keep_image={keep}")
                continue
            # appearance-only stage: the geometry gradients exist ONLY through the photometric term's barycentric / shadow path, i.e. they
            # are made of exactly the pixels float32 cannot decide (sliver faces seen edge-on: d bary ~ 1/area amplifies the rounding of
            # the float32 NDC vertices; measured unmasked: pose 2.8e-2, shape 1.4e-2, cam / rot 1.1e-2 — appearance parameters <= 2e-4).
            # The yardstick is the ORACLE ITSELF evaluated in float32 on the same inputs: the HIP path may not be further from the
            # float64 result than 3 x the float32 oracle is (and never more than 5e-2); where float32 is decisive, 5e-3 holds.
            if o32 is None:
                P32, _, _, _, _ = oracle_step(case, fid, dtype=torch.float32, coarse=False, app=True)
                o32 = {k: rel(P32[k].grad.double(), P[k].grad) for k in keys if P[k].grad is not None and P[k].grad.abs().max() > 0}
                print(f"[gradient rel-L2 of the float32 ORACLE vs the float64 oracle] {tag} UNMASKED: " + ", ".join(f"{k} {v:.1e}" for k, v in o32.items()))
            got = {k: rel(eng.grads[k].cpu().double(), P[k].grad) for k in o32}
            print(f"[gradient rel-L2 vs fp64 oracle] {tag} UNMASKED keep_image={keep}: " + ", ".join(f"{k} {v:.1e}" for k, v in got.items()))
            for k, v in got.items():
                assert v < min(5e-2, max(5e-3, 3.0 * o32[k])), (tag, keep, k, v, o32[k])
        del case, eng
        torch.cuda.empty_cache()


def test_c1_raw_mano_mesh_silhouette_only():
    """config C1: one 256x256 frame, the un-subdivided MANO mesh, silhouette loss only"""
    from harp_amd.engine import LOSS_NAMES
    case = make_fit_case("hand", T=1, S=256, B=1, seed=2, device=DEV, raw=True)
    eng = case["eng"]
    assert eng.topo.V == 778 and eng.topo.F == 1538 and eng.topo.E0 == 0
    eng.set_disabled_terms([k for k in LOSS_NAMES if k != "silhouette"])
    fid = torch.tensor([0])
    lv = engine_eval(case, fid, coarse=True, app=False)
    P, loss, total, aux, _ = oracle_step(case, fid, coarse=True, app=False, terms=("silhouette",))
    assert abs(lv["silhouette"] - loss["silhouette"].item()) <= LOSS_TOL * loss["silhouette"].item()
    assert all(lv[k] == 0.0 for k in LOSS_NAMES if k != "silhouette")
    a = eng.s["alpha"][:1].cpu().double()
    assert ((a - aux["y_sil_pred"]).abs() > 1e-4).float().mean() < 1e-3
    assert 0.03 < (a > 0.5).float().mean() < 0.6
    _check_grads(eng, P, ("pose", "cam", "shape", "verts_disps", "rot", "trans"), tag="C1 engine")
    # ---- the same configuration through the reference API: prepare_mesh(mesh_subdivider=None) + silhouette renderer + L1
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.renderer import renderer_helper
    from harp_amd.structures import Meshes
    from harp_amd.utils.visualize import prepare_mesh, render_image
    S, focal = case["S"], case["focal"]
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model={k: v.numpy() for k, v in case["model"].items()}, device=DEV)
    params = {k: eng.params[k].detach().clone().requires_grad_() for k in ("pose", "rot", "trans", "shape", "cam", "verts_disps")}
    params.update(mesh_faces=layer.th_faces, texture=torch.ones(1, 4, 4, 3, device=DEV), faces_uvs=None, verts_uvs=None)
    _, verts, faces, tex = prepare_mesh(params, fid, layer, False, None, False, dict(model_type="harp"), device=DEV)
    assert verts.shape == (1, 778, 3)
    _, sil_renderer, _ = renderer_helper.get_renderers(image_size=S, silh_sigma=1e-7, silh_gamma=1e-1, silh_faces_per_pixel=50, device=DEV)
    y_sil_pred = render_image(Meshes(verts, faces, tex), params["cam"][fid.to(DEV)], 1, sil_renderer, S, focal, silhouette=True, device=DEV)
    l = torch.nn.L1Loss()(case["targets"]["y_sil"][fid].to(DEV), y_sil_pred)
    (7.0 * l).backward()
    assert abs(l.item() - loss["silhouette"].item()) <= LOSS_TOL * loss["silhouette"].item()
    for k in ("pose", "cam", "shape", "verts_disps", "rot", "trans"):
        assert rel(params[k].grad.cpu().double(), P[k].grad) < GRAD_TOL, ("C1 api", k, rel(params[k].grad.cpu().double(), P[k].grad))


def test_appearance_only_stage_geometry_gradients():
    """appearance-only stage (epochs >= 200, optimize_sequence.py:513-515): the photometric term reaches pose / cam / shape / verts_disps
    only through the barycentric path of the shader backward (uv, position, normal interpolation) and the shadow map — none of it is
    hidden under the 7x-weighted silhouette gradient here"""
    case = make_fit_case("hand", T=2, S=256, B=2, seed=3, device=DEV)
    eng = case["eng"]
    check_removed("app_only_hand_256_b2", mask_ambiguous_pixels(case))
    eng.draw_texture_offsets()
    fid = torch.tensor([0, 1])
    for keep in (True, False):
        eng.keep_image = keep
        lv = engine_eval(case, fid, coarse=False, app=True)
        P, loss, total, aux, _ = oracle_step(case, fid, coarse=False, app=True)
        _check_losses(lv, loss)
        w = _check_grads(eng, P, [k for k in ORACLE_KEYS if k != "wrist_pose"], tag=f"app-only keep_image={keep}")
        assert all(k in w for k in ("pose", "cam", "shape", "verts_disps", "rot", "trans", "texture", "normal_map", "light_positions", "amb_ratio")), w


def test_ten_adam_steps_kernel_vs_torch_adam():
    """10 optimiser steps (eager first, then the captured hipGraph).  (i) The fused Adam kernel == torch.optim.Adam: a replica driven by the
    HIP gradients of every step ends at the same parameters (float32 rounding).  (ii) Free-running against torch.optim.Adam driven by the
    fp64 ORACLE's gradients: rel-L2 <= 1e-3 over the first 3 steps.  Beyond that the comparison stops being meaningful for ANY two
    float32/float64 evaluations: with sigma = 1e-7 the silhouette gradient lives on a 0.2-pixel rim, a parameter difference of 8e-6 changes
    it by 1e-2, and the two trajectories separate geometrically (measured: gradient rel 3e-4, 1e-4, 3e-3, 4e-2, 1e-1, 2e-1, 8e-1 over
    steps 0..6, parameters 3e-3 apart after 10 steps; eager and graph-replayed runs are identical) — so SURVEY.md §8(d)'s "10 steps
    rel 1e-3" is enforced step by step under teacher forcing in the next test instead."""
    case = make_fit_case("hand", T=3, S=128, B=2, seed=4, device=DEV)
    eng = case["eng"]
    eng.keep_image = False
    keys_c, keys_a = ("pose", "cam", "verts_disps", "shape"), ("light_positions", "amb_ratio", "texture", "normal_map")
    R = {k: eng.params[k].detach().cpu().clone().requires_grad_() for k in keys_c + keys_a}
    rep_c = torch.optim.Adam([{"params": [R["pose"], R["cam"]], "lr": 1e-3}, {"params": [R["verts_disps"], R["shape"]], "lr": 1e-3}])
    rep_a = torch.optim.Adam([R[k] for k in keys_a], lr=1e-2)
    P, model, targets = oracle_inputs(case)
    p0 = {k: P[k].detach().clone() for k in ORACLE_KEYS}
    opt_c = torch.optim.Adam([{"params": [P["pose"], P["cam"]], "lr": 1e-3}, {"params": [P["verts_disps"], P["shape"]], "lr": 1e-3}])
    opt_a = torch.optim.Adam([P[k] for k in keys_a], lr=1e-2)
    eng.auto_draw = True
    for it in range(10):
        fid = torch.tensor([it % 3, (it + 1) % 3])
        eng.step(fid, True, True, use_graph=(it > 0))
        torch.cuda.synchronize()
        for k in R:
            R[k].grad = eng.grads[k].detach().cpu().clone()
        rep_c.step(); rep_a.step()
        if it < 3:
            opt_c.zero_grad(); opt_a.zero_grad()
            oracle_step(case, fid, P=P, model=model, targets=targets)          # same batches, same texture-regulariser offsets
            opt_c.step(); opt_a.step()
            for k in keys_c + keys_a:
                # (verts_disps: |values| ~ 6e-4 but every Adam step moves an element by ~lr = 1e-3, so its norm IS the updates)
                assert rel(eng.params[k].cpu().double(), P[k].detach()) < (1e-2 if k == "verts_disps" else 1e-3), (it, k)
    for k in R:
        got, ref = eng.params[k].cpu(), R[k].detach()
        assert rel(got, ref) < 2e-6 and (got - ref).abs().max() < 2e-6, (k, rel(got, ref), (got - ref).abs().max().item())
    for k in ("rot", "trans"):                            # no optimiser in the reference (optimize_sequence.py:254-289)
        assert torch.equal(eng.params[k].cpu().double(), p0[k])


def test_ten_steps_gradient_parity_along_the_oracle_trajectory():
    """SURVEY.md §8(d) "10 Adam steps" as a per-step statement: torch.optim.Adam on the fp64 oracle walks 10 steps; before every step the
    engine is set to the oracle's parameters, and its losses / gradients for that step must agree (rel 1e-5 / 1e-3)."""
    case = make_fit_case("hand", T=3, S=128, B=2, seed=4, device=DEV)
    eng = case["eng"]
    eng.keep_image = False
    keys_a = ("light_positions", "amb_ratio", "texture", "normal_map")
    P, model, targets = oracle_inputs(case)
    opt_c = torch.optim.Adam([{"params": [P["pose"], P["cam"]], "lr": 1e-3}, {"params": [P["verts_disps"], P["shape"]], "lr": 1e-3}])
    opt_a = torch.optim.Adam([P[k] for k in keys_a], lr=1e-2)
    y_col0 = case["targets"]["y_sil_col"].clone()
    keys = [k for k in ORACLE_KEYS if k != "wrist_pose"]
    for it in range(10):
        fid = torch.tensor([it % 3, (it + 1) % 3])
        with torch.no_grad():
            for k in keys:
                eng.params[k].copy_(P[k].detach().float().to(DEV))
        case["targets"]["y_sil_col"] = y_col0.clone()
        check_removed("ten_steps_hand_128", mask_ambiguous_pixels(case))     # the pixels float32 cannot decide, at THIS step's parameters
        targets["y_sil_col"] = case["targets"]["y_sil_col"].double()
        eng.draw_texture_offsets()
        lv = engine_eval(case, fid)
        for k in ORACLE_KEYS:
            P[k].grad = None                              # (rot / trans belong to no optimiser: zero_grad() would not reach them)
        _, loss, _, _, _ = oracle_step(case, fid, P=P, model=model, targets=targets)
        _check_losses(lv, loss)
        _check_grads(eng, P, keys, tag=f"step {it}")
        opt_c.step(); opt_a.step()


@pytest.mark.parametrize("sigma", [1e-5, 1e-7])
def test_ten_free_running_adam_steps_against_the_oracle(sigma, monkeypatch):
    """SURVEY.md §8(d) "parameters after 10 Adam steps rel 1e-3" (the loop optimize_sequence.py:567-573), FREE-RUNNING: the engine (eager
    step, then the replayed hipGraph) and torch.optim.Adam on the fp64 oracle each walk their own 10 steps from the same start, all terms on.
      sigma = 1e-5 — a silhouette rim ~1 px wide at this size instead of the production 0.1 px: the comparison is well-posed, and the
        parameters agree to rel-L2 1e-3 after EVERY one of the 10 steps (the 9 light-position values: 3e-3, see below), and a second
        engine run from the same start stays within the same 3e-3 of the first one's light positions;
      sigma = 1e-7 (optimize_sequence.py:426, production) — the silhouette gradient lives on a 0.2-px rim, the two trajectories separate
        geometrically in parameter space (test_ten_adam_steps_kernel_vs_torch_adam) — but they descend the same objective: the weighted total
        loss of the two runs stays within 1e-2 relative at every step (measured: <= 1e-4 for the first steps, 5e-3 at step 6 — the rim
        pixels whose coverage the two runs decide differently are 7 x 0.1 % of the silhouette term; 1e-3, the review's figure, holds for sigma = 1e-5)."""
    import math
    import oracle.harp_ref as H
    from harp_amd import ops
    monkeypatch.setattr(ops, "SIL_SIGMA", sigma)
    monkeypatch.setattr(ops, "SIL_BLUR", math.log(1.0 / 1e-4 - 1.0) * sigma)
    orig = H.render_silhouette
    monkeypatch.setattr(H, "render_silhouette", lambda *a, **k: orig(*a, **dict(k, sigma=sigma)))
    case = make_fit_case("hand", T=3, S=96, B=2, seed=4, device=DEV)
    eng = case["eng"]
    eng.keep_image = False
    eng.auto_draw = True
    keys_c, keys_a = ("pose", "cam", "verts_disps", "shape"), ("light_positions", "amb_ratio", "texture", "normal_map")
    P, model, targets = oracle_inputs(case)
    opt_c = torch.optim.Adam([{"params": [P["pose"], P["cam"]], "lr": 1e-3}, {"params": [P["verts_disps"], P["shape"]], "lr": 1e-3}])
    opt_a = torch.optim.Adam([P[k] for k in keys_a], lr=1e-2)
    worst_p, worst_l, trace = 0.0, 0.0, []
    start = [t.clone() for t in (eng.p_buf, eng.m_buf, eng.v_buf, eng.hyper, eng.draw_counter)]
    lp_run, lp_oracle = [], []
    for it in range(10):
        fid = torch.tensor([it % 3, (it + 1) % 3])
        eng.step(fid, True, True, use_graph=(it > 0))
        torch.cuda.synchronize()
        lp_run.append(eng.params["light_positions"].cpu().double().clone())
        lv = eng.losses()                                        # the terms at the parameters this step started from
        opt_c.zero_grad(); opt_a.zero_grad()
        _, loss, total, _, _ = oracle_step(case, fid, P=P, model=model, targets=targets)      # same batches, same texture-regulariser offsets
        opt_c.step(); opt_a.step()
        tot_e = sum(H.LOSS_WEIGHTS[k] * lv[k] for k in loss)
        dl = abs(tot_e - total.item()) / abs(total.item())
        worst_l = max(worst_l, dl)
        trace.append(float("%.1e" % dl))
        ltol = 1e-3 if sigma > 1e-6 else 1e-2
        assert dl < ltol, (sigma, it, tot_e, total.item(), trace)
        for k, v in loss.items():                                # every term that carries >= 1 % of the objective (production sigma: the
            if H.LOSS_WEIGHTS[k] * abs(v.item()) >= 1e-2 * abs(total.item()):      # silhouette term alone drifts by up to 2.4 %, the total by 5e-3)
                assert abs(lv[k] - v.item()) <= (2e-3 if sigma > 1e-6 else 5e-2) * abs(v.item()), (sigma, it, k, lv[k], v.item())
        if sigma > 1e-6:
            for k in keys_c + keys_a:
                r = rel(eng.params[k].cpu().double(), P[k].detach())
                worst_p = max(worst_p, r if k != "verts_disps" else 0.0)
                # (verts_disps: |values| ~ 6e-4 but every Adam step moves an element by ~lr = 1e-3, so its norm IS the updates.
                #  light_positions: 9 values that move by lr = 1e-2 per step on a gradient that reaches them through the shadow test of a few
                #  hundred pixels, and Adam turns a small component's difference into a full step.  The gap to the oracle has two parts
                #  (the second run below measures them): a reproducible 1.4e-4 ... 1.5e-4 after 10 steps — float32 against float64, two engine
                #  runs from the same start then stay within 1.1e-5 of each other (4 pairs of 5 on MI355X) — and, in some runs, a different
                #  order of the GPU's float atomics that Adam turns into a whole step from step 7 on: 4.0e-4 between two engine runs and
                #  4.0e-4 to the oracle in the 5th pair; 1.2e-3 to the oracle at step 7 in one run of four earlier.  3e-3 = 0.3 % of the
                #  value, 2 % of the distance it has moved by then)
                bound = {"verts_disps": 1e-2, "light_positions": 3e-3}.get(k, 1e-3)
                assert r < bound, (sigma, it, k, r)
                if k == "light_positions":
                    lp_oracle.append(r)
    print(f"[10 free-running steps, sigma {sigma:g}] worst parameter rel-L2 {worst_p:.1e}, total-loss rel per step {trace}")
    if sigma > 1e-6:
        # the same 10 engine steps again from the same start (no oracle): how far apart two runs' light positions are.  The order of the
        # float atomics is all that differs between them; the light_positions note above says what they measured
        for t, t0 in zip((eng.p_buf, eng.m_buf, eng.v_buf, eng.hyper, eng.draw_counter), start):
            t.copy_(t0)
        spread = []
        for it in range(10):
            eng.step(torch.tensor([it % 3, (it + 1) % 3]), True, True, use_graph=(it > 0))
            torch.cuda.synchronize()
            spread.append(rel(eng.params["light_positions"].cpu().double(), lp_run[it]))
        print("[10 free-running steps] light_positions rel-L2 per step: run vs run", [float("%.1e" % r) for r in spread],
              "engine vs oracle", [float("%.1e" % r) for r in lp_oracle])
        assert max(spread) < 3e-3, spread
