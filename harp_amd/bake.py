"""The frames baked into UV space (csrc/bake.hip): every texel of the atlas finds the pixel it is seen at in every frame —
under the current mesh, camera and hard rasterisation — reads the target colour there, divides out the current Lambert shading and
accumulates a weighted mean.  `bake_texture` returns the projective albedo, its per-texel observation count, weight and colour variance,
and the texture to start (or to look at) with: the mean where seen, dilated into the unseen texels of the charts, the input elsewhere.
The reference has no such pass: it starts from one flat colour (optimize_sequence.py:234) and learns the rest with Adam."""
import torch

from . import ops
from .utils.visualize import _cam_RT, get_mesh_subdivider, params_on, prepare_mesh

_MAP_CACHE = {}


def texel_map(verts_uvs, faces_uvs, Ht, Wt):
    """(texel_face (Ht,Wt) int32, texel_bary (Ht,Wt,2), texel_idx int32 list of covered texels) of ops.uv_texel_map, cached per
    (verts_uvs, faces_uvs, Ht, Wt) — keyed on the CONTENT of the two small tables (an address can be reused after a tensor is freed).  Hashing them is one
    device-to-host copy of ~70 KB per bake, i.e. one synchronisation; a bake runs between two epochs or after the fit, never inside a step"""
    import hashlib
    digest = lambda t: hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()      # noqa: E731
    key = (digest(verts_uvs), digest(faces_uvs), int(Ht), int(Wt), str(verts_uvs.device))
    if key not in _MAP_CACHE:
        face, bary = ops.uv_texel_map(verts_uvs, faces_uvs, Ht, Wt)
        idx = torch.nonzero(face.reshape(-1) >= 0)[:, 0].to(torch.int32).contiguous()
        if len(_MAP_CACHE) >= 8:                          # a handful of templates and atlas sizes at most: bounded
            _MAP_CACHE.pop(next(iter(_MAP_CACHE)))
        _MAP_CACHE[key] = (face, bary, idx)
    return _MAP_CACHE[key]


def camera_centres(R, T):
    """world positions of the camera centres of x_view = x_world R + T (the row-vector convention of ops.project): -T R^T"""
    return -torch.einsum("bj,bij->bi", T, R)


def frame_lights(configs, P, fd):
    """(light_pos (B,3), colors (B,9) = ambient | diffuse | specular) of frames `fd` exactly as mirror_render hands them to its renderer:
    share_light_position, and sigmoid(amb_ratio) with self_shadow (MeshRendererShadow), the constants of the phong renderer without"""
    B, dev = fd.shape[0], fd.device
    light = P["light_positions"][0].repeat(B, 1) if configs["share_light_position"] else P["light_positions"][fd]
    if configs["self_shadow"]:
        amb = torch.sigmoid(P["amb_ratio"].detach().float()).reshape(()) * torch.ones(3, device=dev)
        colors = torch.cat([amb, 1.0 - amb, torch.zeros(3, device=dev)])
    else:
        colors = torch.tensor([0.5] * 3 + [0.4] * 3 + [0.1] * 3, device=dev)
    return light.detach().float().contiguous(), colors[None].repeat(B, 1).contiguous()


def _resident(targets, device, device_ingest):
    if all(hasattr(targets, k) for k in ("fid", "y_true", "y_sil_col")):
        return targets
    from .utils.data_util import ResidentTargets
    if device_ingest:
        return ResidentTargets(targets, device=device, ingest="device")
    return ResidentTargets(targets, device=device)


def bake_accumulate(configs, params, targets, hand_layer, *, delight=True, chunk=32, device="cuda", device_ingest=False, **kernel_params):
    """The accumulation half of bake_texture: -> (accumulators of ops.bake_accumulators, (texel_face, texel_bary, texel_idx)).  Per chunk of
    `chunk` frames: prepare_mesh (the displaced, subdivided mesh as the fit sees it), ops.project, ops.vertex_normals, one hard
    ops.rasterize_fwd(want_zbuf=True), one ops.texture_bake_accum."""
    unknown = set(kernel_params) - set(ops.BAKE_DEFAULTS)
    if unknown:
        raise TypeError(f"bake_texture: unknown kernel parameters {sorted(unknown)} (known: {sorted(ops.BAKE_DEFAULTS)})")
    dev = torch.device(device)
    S, focal, use_arm = int(configs["img_size"]), configs["focal_length"], bool(configs["use_arm"])
    rt = _resident(targets, dev, device_ingest)
    P = params_on(params, dev)
    y_true, y_mask = rt.y_true.to(dev), rt.y_sil_col.to(dev).reshape(rt.y_true.shape[:3])
    if tuple(y_true.shape[1:]) != (S, S, 3):
        raise ValueError(f"targets {tuple(y_true.shape)} do not fit configs['img_size'] = {S}")
    Ht, Wt = P["texture"].shape[1:3]
    sub = get_mesh_subdivider(hand_layer, use_arm=use_arm, device=dev)
    topo = sub.topo
    verts_uvs = torch.as_tensor(P["verts_uvs"]).to(dev).float().reshape(-1, 2).contiguous()
    faces_uvs = torch.as_tensor(P["faces_uvs"]).to(dev).to(torch.int32).reshape(-1, 3).contiguous()
    if faces_uvs.shape[0] != topo.faces.shape[0]:
        raise ValueError(f"faces_uvs has {faces_uvs.shape[0]} rows for the mesh's {topo.faces.shape[0]} faces")
    tface, tbary, tidx = texel_map(verts_uvs, faces_uvs, Ht, Wt)
    acc = ops.bake_accumulators(Ht, Wt, dev)
    fids = torch.as_tensor(rt.fid).long()
    n = fids.shape[0]
    with torch.no_grad(), torch.cuda.device(dev):
        for lo in range(0, n, max(1, int(chunk))):
            fid = fids[lo:lo + max(1, int(chunk))]
            B, fd = fid.shape[0], fid.to(dev)
            _, verts, _, _ = prepare_mesh(P, fid, hand_layer, False, sub, False, configs, device=dev, use_arm=use_arm)
            verts = verts.float().contiguous()
            R, T = _cam_RT(P["cam"][fd], B, S, focal, dev)
            ndc = ops.project(verts, R, T, focal, S)
            vn = ops.vertex_normals(verts, topo)
            face_id, zbuf, _, _ = ops.rasterize_fwd(ndc, topo.faces, S, want_zbuf=True)
            light, colors = frame_lights(configs, P, fd) if delight else (None, None)
            rows = torch.arange(lo, lo + B, dtype=torch.int32, device=dev)
            call = dict(texel_face=tface, texel_bary=tbary, faces=topo.faces, ndc=ndc, face_id=face_id, zbuf=zbuf, y_true=y_true, y_mask=y_mask,
                        rows=rows, texel_idx=tidx, verts=verts, vnormals=vn, cam_pos=camera_centres(R, T.float()).contiguous(), light_pos=light,
                        colors=colors, **kernel_params)
            ops.texture_bake_accum(acc, **call)
    return acc, (tface, tbary, tidx)


def bake_finish(acc, maps, params, *, min_count=1, fill_passes=64, device="cuda"):
    """The second half of bake_texture: accumulators (summed over ranks, if any) -> the result dict."""
    dev = torch.device(device)
    tface = maps[0]
    Ht, Wt = tface.shape
    with torch.no_grad(), torch.cuda.device(dev):
        mean, var, seen = ops.texture_bake_finish(acc, min_count=min_count)
        covered = tface >= 0
        uvm = params.get("uv_mask")
        inside = covered if uvm is None else covered & (torch.as_tensor(uvm).to(dev).reshape(Ht, Wt) > 0.5)
        seen_in = (seen != 0) & inside
        base = params["texture"].detach().to(dev).float().reshape(Ht, Wt, 3)
        start = torch.where(seen_in[..., None], mean, base).contiguous()
        tex, filled = ops.texture_dilate(start, seen_in, int(fill_passes), allow=inside)
        n_in = int(inside.sum())
        coverage = float(seen_in.sum()) / n_in if n_in else 0.0
    return {"texture": tex[None], "mean": mean, "variance": var, "count": acc["count"], "weight": acc["sum_w"], "best_cos": acc["best_cos"],
            "seen": seen != 0, "covered": covered, "filled": filled != 0, "coverage": coverage}


def bake_texture(configs, params, targets, hand_layer, *, delight=True, chunk=32, min_count=1, fill_passes=64, device="cuda",
                 device_ingest=False, **kernel_params):
    """Bake the frames of `targets` into the atlas under the parameters `params` (the reference's dict: pose, rot, trans, shape,
    verts_disps, cam, light_positions, amb_ratio, texture, uv_mask, verts_uvs, faces_uvs).

    targets: a utils.data_util.ResidentTargets (or anything with fid, y_true (T,S,S,3) and y_sil_col (T,S,S)), or a dataset, which goes
    through ResidentTargets (device_ingest: its device path).  delight: divide the Lambert shading of the current lights out (off: the raw
    colours).  chunk: frames per call.  min_count: frames a texel must be observed in to count as seen.  fill_passes: 3 x 3 dilation passes
    from the seen texels into the unseen ones of the charts.  kernel_params: depth_tol (4e-3: ~2 mm at 0.5 m, between the ~1 mm per pixel
    depth slope of a surface slanted 75 degrees at focal 2000 and the >= 10 mm gaps between fingers), cos_min (0.2), cos_power (2),
    shade_floor (0.1) — parameters of the bake, not tolerances.
    Returns a dict: texture (1,Ht,Wt,3) = the mean where seen inside uv_mask and the charts, dilated from there into the rest of
    uv_mask & covered, params["texture"] elsewhere; mean, variance (Ht,Wt,3); count (int32), weight (float64), seen, covered (bool)
    (Ht,Wt); coverage = the share of uv_mask & covered texels that are seen."""
    acc, maps = bake_accumulate(configs, params, targets, hand_layer, delight=delight, chunk=chunk, device=device, device_ingest=device_ingest,
                                **kernel_params)
    return bake_finish(acc, maps, params, min_count=min_count, fill_passes=fill_passes, device=device)


def allreduce_accumulators(acc):
    """sum (count, weights, sums) / maximum (best_cos) of the accumulators over the ranks of the torch.distributed process group: every
    rank then finishes to the same texture"""
    import torch.distributed as tdist
    for k in ("sum_w", "sum_wc", "sum_wc2", "count"):
        tdist.all_reduce(acc[k], op=tdist.ReduceOp.SUM)
    tdist.all_reduce(acc["best_cos"], op=tdist.ReduceOp.MAX)
    return acc


def pad_texture(tex, uv_mask, passes):
    """tex (Ht,Wt,3) float32 HIP tensor dilated by `passes` 3 x 3 passes from uv_mask > 0.5 into the rest (the band a viewer's bilinear
    lookup reaches across the chart borders); passes = 0 returns tex as it is"""
    if int(passes) <= 0:
        return tex
    valid = torch.as_tensor(uv_mask).to(tex.device).reshape(tex.shape[:2]) > 0.5
    return ops.texture_dilate(tex.detach().float().contiguous(), valid, int(passes))[0]
