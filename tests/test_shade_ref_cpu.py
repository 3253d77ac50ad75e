"""CPU: tests/_shade_ref.py, the float64 restatement of the fused shader from separate leaves (the reference for element-wise tests of the
shader backward's gradient exits, docs/NOTEBOOK.md B.15), is itself checked against oracle.harp_ref.render_rgb on the hand scene: handed the
oracle's own face ids, light-view depth map and light camera it gives the same image and — chained through world_to_ndc and verts_normals by
autograd — the same gradients; and the per-pixel contributions it reports add up to the gradients."""
import pytest
import torch
import torch.nn.functional as F

from tests import _shade_ref as R
from tests._scene import make_scene

F64 = torch.float64


@pytest.fixture(scope="module")
def hand():
    from oracle import harp_ref as H
    S = 32
    sc = make_scene(T=1, S=S, seed=0)
    g = torch.Generator().manual_seed(5)
    seq = sc["seq"]
    P0 = dict(pose=seq["pose"].double(), rot=seq["rot"].double(), trans=seq["trans"].double(), shape=seq["shape"].mean(0).double(),
              verts_disps=torch.randn(3093, 1, generator=g, dtype=F64) * 5e-4)
    with torch.no_grad():
        _, verts = H.prepare_mesh(P0, torch.tensor([0]), {k: (v.double() if v.is_floating_point() else v) for k, v in sc["model"].items()}, sc["topo"])
    return dict(sc=sc, S=S, verts=verts, cam=seq["cam"][:1].double(), g=g)


@pytest.mark.parametrize("shadow", [True, False])
def test_restatement_equals_render_rgb_on_the_hand(hand, shadow):
    from oracle import harp_ref as H
    from oracle import p3d_like as P
    sc, S, focal = hand["sc"], hand["S"], hand["sc"]["focal"]
    g = torch.Generator().manual_seed(7 + shadow)
    faces = sc["topo"]["faces"]
    Fn = faces.shape[0]
    vuv, fuv = torch.from_numpy(sc["tpl"]["verts_uvs"]).double(), torch.from_numpy(sc["tpl"]["faces_uvs"]).long()
    Ht = Wt = 64
    base = dict(verts=hand["verts"], texture=torch.rand(1, Ht, Wt, 3, generator=g, dtype=F64) * 0.5 + 0.3,
                normal_map=torch.randn(1, Ht, Wt, 3, generator=g, dtype=F64) * 0.2 + torch.tensor([0.0, 0.0, 1.0], dtype=F64),
                light_positions=torch.tensor([[-0.4, -0.5, -0.6]], dtype=F64), amb_ratio=torch.tensor(0.3, dtype=F64))
    cot = torch.randn(1, S, S, 3, generator=g, dtype=F64)
    cam = hand["cam"]

    def leaves():
        return {k: v.clone().requires_grad_() for k, v in base.items()}
    # ---- the oracle
    a = leaves()
    params = dict(a, verts_uvs=vuv, faces_uvs=fuv)
    img, aux = H.render_rgb(a["verts"], sc["topo"], params, cam, S, focal, self_shadow=shadow, return_aux=True)
    (img * cot).sum().backward()
    # ---- the restatement, fed the oracle's face ids (and its light view), everything else recomputed from leaves of its own
    b = leaves()
    p2f = aux["pix_to_face"][..., 0]
    face_id = torch.where(p2f >= 0, p2f - torch.arange(1)[:, None, None] * Fn, p2f)
    if shadow:
        # the oracle's light view, re-derived from b's leaves: same operations, so its gradient paths (light camera, depth map) chain as well
        lR, lT, cam_R, cam_T = H.process_info_for_shadow(cam, b["light_positions"], b["verts"].mean(1), S, focal)
        ndc_l = P.world_to_ndc(b["verts"], lR, lT, focal, (S / 2.0, S / 2.0), S)[1]
        zl = P.rasterize_meshes(ndc_l, faces, S, 0.0, 1)[1][..., 0]
        assert torch.equal(zl.detach(), aux["zbuf_light"][..., 0].detach()) and torch.equal(lR.detach(), aux["light_R"].detach())
        assert torch.equal(lT.detach(), aux["light_T"].detach())
        amb = torch.sigmoid(b["amb_ratio"]) * torch.ones(3, dtype=F64)
        colors = torch.cat([amb, 1.0 - amb, torch.zeros(3, dtype=F64)])
    else:
        cam_R, cam_T = H.camera_RT(cam, S, focal)
        zl = lR = lT = None
        colors = torch.tensor([0.5] * 3 + [0.4] * 3 + [0.1] * 3, dtype=F64)
    lv = dict(ndc=P.world_to_ndc(b["verts"], cam_R, cam_T, focal, (S / 2.0, S / 2.0), S)[1], verts=b["verts"], vnormals=P.verts_normals(b["verts"], faces),
              tex=b["texture"][0], nmap=F.normalize(b["normal_map"][0], dim=-1), light_pos=b["light_positions"], colors=colors, zl=zl,
              light_R=lR, light_T=lT)
    out = R.shade(lv, face_id, faces, vuv, fuv, S, focal)
    (out["rgb"] * cot).sum().backward()
    n_cov = int(out["covered"].sum())
    assert n_cov > 100 and torch.equal(out["covered"], p2f >= 0)
    err = (out["rgb"] - img).abs().max().item()
    print(f"[shade_ref vs render_rgb, shadow={shadow}] covered {n_cov}, image {err:.2e}")
    assert err < 1e-12, err
    for k in ("texture", "normal_map", "light_positions", "verts") + (("amb_ratio",) if shadow else ()):
        want, got = a[k].grad, b[k].grad
        assert want.abs().max() > 0, k
        e = ((got - want).abs().max() / want.abs().max()).item()
        print(f"    d/d {k}: {e:.2e}")
        assert e < 1e-9, (k, e)


def test_per_pixel_contributions_add_up_to_the_gradients(hand):
    """what the bound is made of: scattering every pixel's own contribution (autograd on the gathered per-pixel inputs) reproduces the
    gradient of each leaf; N counts the contributing pixels; the ambiguous-pixel mask flags the classes it is meant to"""
    from oracle import harp_ref as H
    from oracle import p3d_like as P
    sc, S, focal = hand["sc"], hand["S"], hand["sc"]["focal"]
    g = torch.Generator().manual_seed(11)
    faces = sc["topo"]["faces"]
    vuv, fuv = torch.from_numpy(sc["tpl"]["verts_uvs"]).double(), torch.from_numpy(sc["tpl"]["faces_uvs"]).long()
    verts, cam = hand["verts"], hand["cam"]
    light = torch.tensor([[-0.4, -0.5, -0.6]], dtype=F64)
    with torch.no_grad():
        lR, lT, cR, cT = H.process_info_for_shadow(cam, light, verts.mean(1), S, focal)
        pp_ = (S / 2.0, S / 2.0)
        ndc = P.world_to_ndc(verts, cR, cT, focal, pp_, S)[1].float().double()
        face_id = P.rasterize_meshes(ndc, faces, S, 0.0, 1)[0][..., 0]
        zl = P.rasterize_meshes(P.world_to_ndc(verts, lR, lT, focal, pp_, S)[1], faces, S, 0.0, 1)[1][..., 0]
    Ht, Wt = 37, 29
    src = dict(ndc=ndc, verts=verts, vnormals=P.verts_normals(verts, faces), tex=torch.rand(Ht, Wt, 3, generator=g, dtype=F64),
               nmap=F.normalize(torch.randn(Ht, Wt, 3, generator=g, dtype=F64) * 0.2 + torch.tensor([0.0, 0.0, 1.0], dtype=F64), dim=-1),
               light_pos=light, colors=torch.tensor([0.3] * 3 + [0.7] * 3 + [0.05] * 3, dtype=F64), zl=zl, light_R=lR, light_T=lT)
    cot = torch.randn(1, S, S, 3, generator=g, dtype=F64)
    cot[0, :, : S // 2][face_id[0, :, : S // 2] >= 0] *= (torch.rand(S, S // 2, 1, generator=g, dtype=F64) > 0.3)[face_id[0, :, : S // 2] >= 0]
    res, out = R.gradients(src, cot, face_id, faces, vuv, fuv, S, focal)
    assert set(res) == set(R.LEAVES)
    n_act = int((out["covered"] & (cot != 0).any(-1)).sum())
    assert 100 < n_act < int(out["covered"].sum())
    # re-derive each gradient from the per-pixel pieces: autograd.grad again on the intermediates, scattered by the reported indices
    lv = R.leaves_like(src, F64)
    o2 = R.shade(lv, face_id, faces, vuv, fuv, S, focal)
    keys = list(o2["pp"])
    gp = dict(zip(keys, torch.autograd.grad((o2["rgb"] * cot).sum(), [o2["pp"][k] for k in keys])))
    V = verts.shape[1]
    vid = o2["ix"]["vid"].reshape(1, -1)
    for k in ("ndc", "verts", "vnormals"):
        tot = torch.stack([R._scatter(vid, gp[k].reshape(1, -1, 3)[..., j], V) for j in range(3)], -1)
        assert (tot - res[k]["ref"]).abs().max() <= 1e-12 * max(1.0, res[k]["ref"].abs().max().item()), k
        assert int(res[k]["N"][..., 0].sum()) == 3 * n_act and (res[k]["A"] + 1e-30 >= res[k]["ref"].abs() * (1 - 1e-9)).all()
        assert res[k]["M"] >= gp[k].abs().max().item() * (1 - 1e-12) and res[k]["M"] > 0
    w = o2["ix"]["tex_w"] * o2["ix"]["tex_valid"]
    for k, pk in (("tex", "texels"), ("nmap", "nm")):
        c = gp[pk][..., 0, None, :] * w[..., None]
        tot = torch.stack([R._scatter(o2["ix"]["tex_key"].clamp(0, Ht * Wt - 1).reshape(1, -1), c[..., j].reshape(1, -1), Ht * Wt) for j in range(3)], -1).view(Ht, Wt, 3)
        assert (tot - res[k]["ref"]).abs().max() <= 1e-10 * res[k]["ref"].abs().max(), (k, (tot - res[k]["ref"]).abs().max())
        assert (res[k]["A"] + 1e-30 >= res[k]["ref"].abs() * (1 - 1e-9)).all() and res[k]["N"].max() >= 2
    tot = R._scatter(o2["ix"]["tap"].reshape(1, -1), gp["taps"].reshape(1, -1), S * S).view(1, S, S)
    assert res["zl"]["ref"].abs().max() > 0 and (tot - res["zl"]["ref"]).abs().max() <= 1e-12 * res["zl"]["ref"].abs().max()
    for k in ("colors", "light_pos", "light_R", "light_T"):
        tot = gp[k].sum((0, 1, 2, 3)).reshape(res[k]["ref"].shape) if k in ("colors",) else gp[k].sum((1, 2)).reshape(res[k]["ref"].shape)
        assert (tot - res[k]["ref"]).abs().max() <= 1e-11 * max(res[k]["ref"].abs().max().item(), 1e-30), k
        assert int(res[k]["N"].max()) == n_act
    # only the third column of the light rotation (the depth in the light view) carries a gradient: the tap indices are rounded
    assert res["light_R"]["ref"][:, :, :2].abs().max() == 0 and res["light_R"]["ref"][:, :, 2].abs().max() > 0
    assert res["light_T"]["ref"][:, :2].abs().max() == 0 and res["light_T"]["ref"][:, 2].abs().max() > 0
    # the same function in float32: close to the float64 one on this scene (its difference is the bound's arithmetic term)
    r32, _ = R.gradients(src, cot * (~out["ambiguous"])[..., None], face_id, faces, vuv, fuv, S, focal, dtype=torch.float32, stats=False)
    r64, _ = R.gradients(src, cot * (~out["ambiguous"])[..., None], face_id, faces, vuv, fuv, S, focal, stats=False)
    for k in ("verts", "vnormals", "tex", "nmap", "colors"):
        e = ((r32[k].double() - r64[k]).abs().max() / r64[k].abs().max()).item()
        print(f"[float32 vs float64 restatement] {k}: {e:.2e}")
        assert e < 1e-3, (k, e)
