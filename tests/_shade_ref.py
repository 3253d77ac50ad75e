"""Float64 restatement of the fused K=1 shader (csrc/shade.hip, csrc/shade_bwd.hip) from SEPARATE leaves, composed from the oracle's own
pieces (oracle/p3d_like.py, oracle/harp_ref.py), with every pixel's gathered inputs kept as intermediates of the autograd graph — so that
torch.autograd.grad on them gives each pixel's OWN contribution to every vertex, texel, shadow-map tap and per-frame scalar.  That is what
an element-wise error bound for the shader backward's table exits (csrc/shade_bwd.hip) is made of: N_i contributions of at most M_g each,
sum of magnitudes A_i (docs/NOTEBOOK.md B.15).

It does not rasterise: it is handed a `face_id` image and recomputes the perspective-correct barycentrics of that face at the pixel centre
(p3d_like._pair_eval), O(pixels).  tests/test_shade_ref_cpu.py anchors it on oracle.harp_ref.render_rgb.  dtype-generic: the same function in
float32 measures how ill-conditioned a case's per-pixel arithmetic is."""
import torch
import torch.nn.functional as F

from oracle import harp_ref as H
from oracle import p3d_like as P

LEAVES = ("ndc", "verts", "vnormals", "tex", "nmap", "light_pos", "colors", "zl", "light_R", "light_T")


def shade(lv, face_id, faces, verts_uvs, faces_uvs, S, focal, bg=(1.0, 1.0, 1.0)):
    """lv: dict of the leaves — ndc, verts, vnormals (B,V,3); tex, nmap (Ht,Wt,3) (nmap: the NORMALISED map, or None); light_pos (B,3);
    colors (9,) = ambient, diffuse, specular; zl (B,S,S) light-view depth, light_R (B,3,3), light_T (B,3) (zl None: no shadow test).
    face_id (B,S,S) frame-local face index, -1 = empty; faces, faces_uvs (F,3) long; verts_uvs (VT,2).
    `ndc` is used AS GIVEN: the kernels read the rasteriser's float32 face records, so a caller that compares with them hands over
    float32-rounded values (gradients() rounds; the anchor test feeds the oracle's own unrounded ones to match it to 1e-12).
    Returns a dict: rgb (B,S,S,3), covered, ambiguous (B,S,S) bool, `pp` = the per-pixel intermediates, `ix` = per-pixel indices."""
    dt = lv["verts"].dtype
    B = lv["verts"].shape[0]
    cov = face_id >= 0
    fid = face_id.clamp(min=0).long()
    vid = faces[fid]                                              # (B,S,S,3) vertex ids of the pixel's face
    bi = torch.arange(B)[:, None, None, None]
    pp = {"ndc": lv["ndc"][bi, vid], "verts": lv["verts"][bi, vid], "vnormals": lv["vnormals"][bi, vid]}      # (B,S,S,3,3) each
    pc = P.pixel_centers(S, dt)
    px, py = pc[None, None, :].expand(B, S, S).reshape(-1), pc[None, :, None].expand(B, S, S).reshape(-1)
    # the rasteriser hands the shader the float32 NDC of the face; barycentrics at the pixel centre from those
    bary, pz, d2, inside = P._pair_eval(pp["ndc"].reshape(-1, 3, 3), px, py, True, False)
    n_pix = B * S * S
    p2f = torch.where(cov.reshape(-1), torch.arange(n_pix), torch.full((n_pix,), -1)).view(B, S, S, 1)        # every pixel is its own "face"
    bary4 = bary.view(B, S, S, 1, 3)
    pix_pos = P.interpolate_face_attributes(p2f, bary4, pp["verts"].reshape(n_pix, 3, 3))                     # (B,S,S,1,3)
    pix_n = P.interpolate_face_attributes(p2f, bary4, pp["vnormals"].reshape(n_pix, 3, 3))
    fidk = torch.where(cov, fid, torch.full_like(fid, -1))[..., None]
    Ht, Wt = lv["tex"].shape[:2]

    def sample(m):
        return torch.cat([P.sample_textures_uv(m[None], verts_uvs, faces_uvs, fidk[b:b + 1], bary4[b:b + 1], faces.shape[0]) for b in range(B)], 0)
    pp["texels"] = sample(lv["tex"])
    amb = torch.zeros(B, S, S, dtype=torch.bool)
    with torch.no_grad():
        # the bilinear footprint of every pixel (TexturesUV.sample_textures: align_corners, border padding, v flipped)
        puv = P.interpolate_face_attributes(p2f, bary4, verts_uvs[faces_uvs[fid]].reshape(n_pix, 3, 2))[..., 0, :]
        tx, ty = puv[..., 0] * (Wt - 1), (1 - puv[..., 1]) * (Ht - 1)
        amb |= ((tx - tx.round()).abs() < 1e-3) | ((ty - ty.round()).abs() < 1e-3)
        txc, tyc = tx.clamp(0, Wt - 1), ty.clamp(0, Ht - 1)
        x0, y0 = txc.floor(), tyc.floor()
        wx, wy = txc - x0, tyc - y0
        cx = torch.stack([x0, x0 + 1, x0, x0 + 1], -1).long()
        cy = torch.stack([y0, y0, y0 + 1, y0 + 1], -1).long()
        cw = torch.stack([(1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy], -1)
        cvalid = (cx < Wt) & (cy < Ht) & (cw != 0) & cov[..., None]
        amb |= bary.view(B, S, S, 3).min(-1).values < -1e-6          # pixel centre outside the face it was given
    if lv.get("nmap") is not None:
        pp["nm"] = sample(lv["nmap"])
        with torch.no_grad():
            amb |= pix_n[..., 0, 2].abs() < 1e-5 * pix_n[..., 0, :].norm(dim=-1).clamp(min=1e-12)
        pix_n = H.apply_normal_map(pix_n, pp["nm"])
    pp["light_pos"] = lv["light_pos"][:, None, None, None, :].expand(B, S, S, 1, 3) * 1.0
    pp["colors"] = lv["colors"].reshape(1, 1, 1, 1, 9).expand(B, S, S, 1, 9) * 1.0
    ambient, diffuse_c, specular = pp["colors"][..., 0:3], pp["colors"][..., 3:6], pp["colors"][..., 6:9]
    diff = P.point_light_diffuse(pix_pos, pix_n, pp["light_pos"], diffuse_c)
    with torch.no_grad():
        lh = F.normalize(pp["light_pos"] - pix_pos, dim=-1, eps=1e-6)
        amb |= (F.normalize(pix_n, dim=-1, eps=1e-6) * lh).sum(-1)[..., 0].abs() < 1e-5
    ix = {"vid": vid, "tex_key": cy * Wt + cx, "tex_x": cx, "tex_y": cy, "tex_w": cw, "tex_valid": cvalid}
    if lv.get("zl") is not None:
        pp["light_R"] = lv["light_R"][:, None, None].expand(B, S, S, 3, 3) * 1.0
        pp["light_T"] = lv["light_T"][:, None, None].expand(B, S, S, 3) * 1.0
        in_light = (pix_pos[..., 0, :, None] * pp["light_R"]).sum(-2) + pp["light_T"]                         # (B,S,S,3)
        xs, ys = P.view_to_screen_xy(in_light, focal, (S / 2.0, S / 2.0), S)
        xk, yk = xs.round().long(), ys.round().long()
        fx, fy = xs.detach() - torch.floor(xs.detach()), ys.detach() - torch.floor(ys.detach())
        amb |= ((fx - 0.5).abs() < 2e-3) | ((fy - 0.5).abs() < 2e-3)
        tyx = [((yk + ii).clamp(0, S - 1), (xk + jj).clamp(0, S - 1)) for ii in (-1, 0, 1) for jj in (-1, 0, 1)]
        ix["tap"] = torch.stack([a * S + b for a, b in tyx], -1)                                              # (B,S,S,9) row-major 3x3
        ix["tap_centre"] = torch.stack([yk, xk], -1)
        pp["taps"] = lv["zl"].reshape(B, S * S).gather(1, ix["tap"].reshape(B, -1)).view(B, S, S, 9)
        aa = in_light[..., 2] - 0.008
        vis = torch.sigmoid((pp["taps"] - aa[..., None]) * 1000.0).sum(-1) / 9.0
        colors = (ambient + diff * vis[..., None, None]) * pp["texels"] + specular
    else:
        colors = (ambient + diff) * pp["texels"] + specular
    sd = torch.where(inside, -d2, d2).view(B, S, S, 1)
    img = P.softmax_rgb_blend(colors, p2f, pz.view(B, S, S, 1), sd, background=bg)
    return {"rgb": img[..., :3], "covered": cov, "ambiguous": amb & cov, "pp": pp, "ix": ix}


def leaves_like(src, dtype):
    """fresh leaves (requires_grad) of `dtype` from a dict of tensors"""
    return {k: (None if src.get(k) is None else src[k].detach().to(dtype).clone().requires_grad_()) for k in LEAVES}


def _scatter(idx, val, n):
    """sum val (B,P) into (B,n) at idx (B,P)"""
    return torch.zeros(idx.shape[0], n, dtype=val.dtype).scatter_add(1, idx, val)


def gradients(src, cot, face_id, faces, verts_uvs, faces_uvs, S, focal, dtype=torch.float64, bg=(1.0, 1.0, 1.0), stats=True):
    """Gradients of (rgb * cot).sum() for every leaf of `src` (evaluated in `dtype`), and — stats=True — what the bound needs per output:
    {name: dict(ref=gradient, N=number of pixel contributions per element, A=sum of their magnitudes, M=largest single one of the group)}.
    Names: ndc, verts, vnormals, tex, nmap, light_pos, colors, zl, light_R, light_T.  Also returns the forward dict of shade().
    src["ndc"] is rounded to float32 first (the face records the shader kernels read).  A contribution = what one pixel adds to one output
    element: for the two texel maps the sampled texel's gradient TIMES the corner's bilinear weight (what the kernel's table receives), counted
    for corners inside the map with a non-zero weight (the kernel adds no others: `valid[k]` in shade_bwd.hip); their M is the largest
    sampled-texel gradient BEFORE weighting, which is what the kernel takes its table scale from."""
    lv = leaves_like(dict(src, ndc=src["ndc"].float()), dtype)
    out = shade(lv, face_id, faces, verts_uvs.to(dtype), faces_uvs, S, focal, bg)
    loss = (out["rgb"] * cot.to(dtype)).sum()
    names = [k for k in LEAVES if lv[k] is not None]
    pp, ix = out["pp"], out["ix"]
    pkeys = list(pp)
    g = torch.autograd.grad(loss, [lv[k] for k in names] + [pp[k] for k in pkeys], allow_unused=True)
    ref = {k: (torch.zeros_like(lv[k]) if x is None else x) for k, x in zip(names, g[:len(names)])}
    if not stats:
        return ref, out
    gp = {k: (torch.zeros_like(pp[k]) if x is None else x) for k, x in zip(pkeys, g[len(names):])}
    B, V = lv["verts"].shape[:2]
    active = (out["covered"] & (cot != 0).any(-1)).to(dtype)                                   # pixels the kernel shades
    res = {}
    vid = ix["vid"].reshape(B, -1)
    for k in ("ndc", "verts", "vnormals"):
        c = gp[k].reshape(B, -1, 3).abs()                                                     # (B, S*S*3 corners, 3)
        A = torch.stack([_scatter(vid, c[..., j], V) for j in range(3)], -1)
        N = _scatter(vid, active[..., None].expand(-1, -1, -1, 3).reshape(B, -1), V)[..., None].expand(B, V, 3)
        res[k] = dict(ref=ref[k], N=N, A=A, M=c.max().item())
    Ht, Wt = lv["tex"].shape[:2]
    key = ix["tex_key"].clamp(0, Ht * Wt - 1).reshape(1, -1)
    w = (ix["tex_w"] * ix["tex_valid"]).to(dtype)
    for k, pk in (("tex", "texels"), ("nmap", "nm")):
        if pk not in gp:
            continue
        c = (gp[pk][..., 0, None, :] * w[..., None]).abs()                                    # (B,S,S,4 corners,3)
        A = torch.stack([_scatter(key, c[..., j].reshape(1, -1), Ht * Wt) for j in range(3)], -1).view(Ht, Wt, 3)
        N = _scatter(key, (ix["tex_valid"] * active[..., None]).to(dtype).reshape(1, -1), Ht * Wt).view(Ht, Wt, 1).expand(Ht, Wt, 3)
        # M: the UNWEIGHTED gradient of the sampled texel — the kernel scales its texel table by the wave maximum of that (shade_bwd.hip:
        # fixed_scale(ma) / fixed_scale(mm)), so the quantum of an add is set by it, not by the (smaller) weighted contribution
        res[k] = dict(ref=ref[k], N=N, A=A, M=gp[pk].abs().max().item())
    n_act = active.sum((1, 2))                                                                 # (B,)
    c = gp["colors"][..., 0, :].abs()
    res["colors"] = dict(ref=ref["colors"], N=n_act.sum().expand(9), A=c.sum((0, 1, 2)), M=c.max().item())
    c = gp["light_pos"][..., 0, :].abs()
    res["light_pos"] = dict(ref=ref["light_pos"], N=n_act[:, None].expand(B, 3), A=c.sum((1, 2)), M=c.max().item())
    if "taps" in gp:
        c = gp["taps"].abs().reshape(B, -1)
        tap = ix["tap"].reshape(B, -1)
        res["zl"] = dict(ref=ref["zl"], N=_scatter(tap, active[..., None].expand(-1, -1, -1, 9).reshape(B, -1), S * S).view(B, S, S),
                         A=_scatter(tap, c, S * S).view(B, S, S), M=c.max().item())
        c = gp["light_R"].abs()
        res["light_R"] = dict(ref=ref["light_R"], N=n_act[:, None, None].expand(B, 3, 3), A=c.sum((1, 2)), M=c.max().item())
        c = gp["light_T"].abs()
        res["light_T"] = dict(ref=ref["light_T"], N=n_act[:, None].expand(B, 3), A=c.sum((1, 2)), M=c.max().item())
    return res, out
