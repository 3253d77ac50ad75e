"""torch.autograd bindings of the HIP kernels (C-ABI in include/harp_hip.h).

These are the building blocks the reference-API mirror modules (renderer/, utils/, loss/, manopth/) and the
fused engine call.  Every op takes/returns plain contiguous float32/int32 HIP tensors."""
import collections
import math

import ctypes

import numpy as np
import torch

from . import _lib

SIL_SIGMA = 1e-7                                        # optimize_sequence.py:426
SIL_BLUR = math.log(1.0 / 1e-4 - 1.0) * SIL_SIGMA       # renderer_helper.py:46


def rasterize_workspace(B, F, S, device):
    n = _lib.lib().harp_rasterize_ws_bytes(B, F, S)
    return torch.empty(n, dtype=torch.uint8, device=device)


def rasterize_ws_nact(ws, B, F, S):
    """number of (frame, 64x64 super-tile) pairs that hold faces, read back from a rasteriser workspace (csrc/harp_common.h:
    raster_ws_split — ... | nact (256 B) | hit bitmaps at the tail); debugging / tests: one D2H copy"""
    nst = ((S + 63) // 64) ** 2
    bits = B * nst * ((F + 63) // 64) * 8
    return int(ws[-(256 + bits):][:4].view(torch.int32)[0])


def rasterize_fwd(ndc, faces, S, soft=False, blur_radius=0.0, sigma=1.0, want_zbuf=True, ws=None):
    """ndc (B,V,3) f32, faces (F,3) i32 -> face_id (B,S,S) i32, zbuf (B,S,S)|None, alpha (B,S,S)|None, ws."""
    B, V, _ = ndc.shape
    F = faces.shape[0]
    dev = ndc.device
    if ws is None:
        ws = rasterize_workspace(B, F, S, dev)
    face_id = torch.empty(B, S, S, dtype=torch.int32, device=dev)
    zbuf = torch.empty(B, S, S, dtype=torch.float32, device=dev) if want_zbuf else None
    alpha = torch.empty(B, S, S, dtype=torch.float32, device=dev) if soft else None
    rc = _lib.lib().harp_rasterize_fwd(_lib.ptr(ndc), _lib.ptr(faces), B, V, F, S, int(soft), blur_radius, sigma,
                                       _lib.ptr(ws), _lib.ptr(face_id), _lib.ptr(zbuf), _lib.ptr(alpha), _lib.stream())
    _lib.check(rc, "harp_rasterize_fwd")
    return face_id, zbuf, alpha, ws


def silhouette_bwd(faces, V, S, blur_radius, sigma, ws, alpha, g_alpha, g_ndc):
    B = alpha.shape[0]
    rc = _lib.lib().harp_silhouette_bwd(_lib.ptr(faces), B, V, faces.shape[0], S, blur_radius, sigma, _lib.ptr(ws),
                                        _lib.ptr(alpha), _lib.ptr(g_alpha.contiguous()), _lib.ptr(g_ndc), _lib.stream())
    _lib.check(rc, "harp_silhouette_bwd")


class _SoftSilhouette(torch.autograd.Function):
    """alpha = SoftSilhouetteShader(MeshRasterizer(K=50, blur))(mesh)[..., 3] (renderer_helper.py:44-58)."""

    @staticmethod
    def forward(ctx, ndc, faces, S, blur_radius, sigma):
        ndc = ndc.contiguous()
        face_id, _, alpha, ws = rasterize_fwd(ndc, faces, S, soft=True, blur_radius=blur_radius, sigma=sigma, want_zbuf=False)
        ctx.save_for_backward(faces, alpha, ws)
        ctx.meta = (ndc.shape, S, blur_radius, sigma)
        ctx.mark_non_differentiable(face_id)
        return alpha, face_id

    @staticmethod
    def backward(ctx, g_alpha, _g_face):
        faces, alpha, ws = ctx.saved_tensors
        shape, S, blur_radius, sigma = ctx.meta
        g_ndc = torch.zeros(shape, dtype=torch.float32, device=alpha.device)
        silhouette_bwd(faces, shape[1], S, blur_radius, sigma, ws, alpha, g_alpha, g_ndc)
        return g_ndc, None, None, None, None


def soft_silhouette(ndc, faces, S, blur_radius=SIL_BLUR, sigma=SIL_SIGMA):
    return _SoftSilhouette.apply(ndc, faces, S, blur_radius, sigma)


# ------------------------------------------------------------------------------------------------------
# static topology on the device
# ------------------------------------------------------------------------------------------------------
class DeviceTopology:
    """int32 HBM copies of the host tables of harp_amd.synth.build_topology / topology.py."""

    def __init__(self, topo, verts_uvs, faces_uvs, device):
        def i32(a):
            t = torch.as_tensor(np.asarray(a), dtype=torch.int32).contiguous()
            if t.numel() == 0:                             # un-subdivided template: empty tables still need a valid device pointer
                t = torch.zeros((1,) + tuple(t.shape[1:]), dtype=torch.int32)
            return t.to(device)
        self.V0, self.V = int(topo["n_verts0"]), int(topo["n_verts"])
        for k in ("faces0", "edges0", "faces", "edges", "nbr_off", "nbr_idx", "vf_off", "vf_idx", "nc_pairs", "vp_off", "vp_idx", "sub_off", "sub_idx"):
            setattr(self, k, i32(topo[k]))
        self.E0, self.F, self.E = int(np.asarray(topo["edges0"]).shape[0]), self.faces.shape[0], self.edges.shape[0]
        # expanded vertex -> incident-face table for the fused mesh chain: (i0, i1, i2, corner) per CSR entry, one 16-B load
        fc = torch.as_tensor(np.asarray(topo["vf_idx"]), dtype=torch.int64)
        fa = torch.as_tensor(np.asarray(topo["faces"]), dtype=torch.int64)
        self.vf_tri = torch.cat([fa[fc // 3], (fc % 3)[:, None]], 1).to(torch.int32).contiguous().to(device)
        self.verts_uvs = torch.as_tensor(verts_uvs, dtype=torch.float32).reshape(-1, 2).contiguous().to(device)
        self.faces_uvs = i32(faces_uvs).reshape(-1, 3)
        self.device = device
        self._check_uvs()

    def _check_uvs(self):
        # the shader kernels read verts_uvs[faces_uvs] without a bounds check
        lo, hi = int(self.faces_uvs.min()), int(self.faces_uvs.max())
        if lo < 0 or hi >= self.verts_uvs.shape[0]:
            raise ValueError(f"faces_uvs must index verts_uvs ({self.verts_uvs.shape[0]} rows): found indices in [{lo}, {hi}]")

    def set_uvs(self, verts_uvs, faces_uvs):
        """(re)bind the UV tables (TexturesUV(faces_uvs=, verts_uvs=), utils/visualize.py:84-87); accepts the reference's (1,VT,2)/(1,F,3)"""
        key = (verts_uvs.data_ptr() if torch.is_tensor(verts_uvs) else id(verts_uvs), faces_uvs.data_ptr() if torch.is_tensor(faces_uvs) else id(faces_uvs))
        if getattr(self, "_uv_key", None) != key:
            self.verts_uvs = torch.as_tensor(verts_uvs, dtype=torch.float32).reshape(-1, 2).contiguous().to(self.device)
            self.faces_uvs = torch.as_tensor(faces_uvs).to(torch.int32).reshape(-1, 3).contiguous().to(self.device)
            self._check_uvs()
            self._uv_key = key


def _f32(t):
    return t.contiguous().float()


class _Subdivide(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v0, topo, scale):
        v0 = _f32(v0)
        B = v0.shape[0]
        vs = torch.empty(B, topo.V, 3, dtype=torch.float32, device=v0.device)
        _lib.check(_lib.lib().harp_subdivide_fwd(_lib.ptr(v0), _lib.ptr(topo.edges0), B, topo.V0, topo.E0, scale, _lib.ptr(vs),
                                                 _lib.stream()), "harp_subdivide_fwd")
        ctx.topo, ctx.scale = topo, scale
        return vs

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        topo, B = ctx.topo, g.shape[0]
        g0 = torch.empty(B, topo.V0, 3, dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().harp_subdivide_bwd(_lib.ptr(g), _lib.ptr(topo.sub_off), _lib.ptr(topo.sub_idx), B, topo.V0, topo.V,
                                                 ctx.scale, _lib.ptr(g0), _lib.stream()), "harp_subdivide_bwd")
        return g0, None, None


def subdivide(v0, topo, scale=1.0):
    """[scale*v0 ; edge midpoints] (SubdivideMeshes, utils/visualize.py:45-52)."""
    return _Subdivide.apply(v0, topo, scale)


class _NormalsDisplace(torch.autograd.Function):
    """n = unit vertex normals of v; optionally vd = v + n * disp (utils/visualize.py:58-64)."""

    @staticmethod
    def forward(ctx, v, disp, topo):
        v = _f32(v)
        B = v.shape[0]
        n = torch.empty_like(v)
        inv_len = torch.empty(B, topo.V, dtype=torch.float32, device=v.device)
        d = _f32(disp.reshape(-1)) if disp is not None else None
        vd = torch.empty_like(v) if disp is not None else None
        _lib.check(_lib.lib().harp_vertex_normals_fwd(_lib.ptr(v), _lib.ptr(topo.faces), _lib.ptr(topo.vf_off), _lib.ptr(topo.vf_idx),
                                                      B, topo.V, _lib.ptr(n), _lib.ptr(inv_len), _lib.ptr(d), _lib.ptr(vd),
                                                      _lib.stream()), "harp_vertex_normals_fwd")
        ctx.topo, ctx.has_disp = topo, disp is not None
        ctx.disp_shape = disp.shape if disp is not None else None
        ctx.save_for_backward(v, n, inv_len, d)
        return (n, vd) if disp is not None else (n, None)

    @staticmethod
    def backward(ctx, g_n, g_vd):
        v, n, inv_len, d = ctx.saved_tensors
        topo, B = ctx.topo, v.shape[0]
        L = _lib.lib()
        g_v = torch.zeros_like(v)
        g_disp = None
        g_n_tot = _f32(g_n) if g_n is not None else torch.zeros_like(v)
        if ctx.has_disp and g_vd is not None:
            g_vd = _f32(g_vd)
            g_v = g_vd.clone()
            g_nd = torch.empty_like(v)
            g_disp = torch.zeros(topo.V, dtype=torch.float32, device=v.device)
            _lib.check(L.harp_displace_bwd(_lib.ptr(g_vd), _lib.ptr(n), _lib.ptr(d), B, topo.V, _lib.ptr(g_nd), _lib.ptr(g_disp),
                                           _lib.stream()), "harp_displace_bwd")
            g_n_tot = g_n_tot + g_nd
            g_disp = g_disp.reshape(ctx.disp_shape)
        tmp = torch.empty_like(v)
        _lib.check(L.harp_vertex_normals_bwd(_lib.ptr(v), _lib.ptr(topo.faces), _lib.ptr(topo.vf_off), _lib.ptr(topo.vf_idx), B, topo.V,
                                             _lib.ptr(n), _lib.ptr(inv_len), _lib.ptr(g_n_tot.contiguous()), _lib.ptr(tmp), _lib.ptr(g_v),
                                             _lib.stream()), "harp_vertex_normals_bwd")
        return g_v, g_disp, None


def vertex_normals(v, topo):
    return _NormalsDisplace.apply(v, None, topo)[0]


def normals_displace(v, disp, topo):
    return _NormalsDisplace.apply(v, disp, topo)


class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, R, T, focal, ppx, ppy, S):
        v, R, T = _f32(v), _f32(R).reshape(-1, 9), _f32(T)
        B, V, _ = v.shape
        ndc = torch.empty_like(v)
        _lib.check(_lib.lib().harp_project_fwd(_lib.ptr(v), _lib.ptr(R), _lib.ptr(T), B, V, focal, ppx, ppy, S, _lib.ptr(ndc),
                                               _lib.stream()), "harp_project_fwd")
        ctx.save_for_backward(v, R, T)
        ctx.meta = (focal, S)
        return ndc

    @staticmethod
    def backward(ctx, g):
        v, R, T = ctx.saved_tensors
        focal, S = ctx.meta
        B, V, _ = v.shape
        g_v = torch.zeros_like(v)
        g_R = torch.zeros(B, 9, dtype=torch.float32, device=v.device)
        g_T = torch.zeros(B, 3, dtype=torch.float32, device=v.device)
        _lib.check(_lib.lib().harp_project_bwd(_lib.ptr(v), _lib.ptr(R), _lib.ptr(T), _lib.ptr(_f32(g)), B, V, focal, S, _lib.ptr(g_v),
                                               _lib.ptr(g_R), _lib.ptr(g_T), _lib.stream()), "harp_project_bwd")
        return g_v, g_R.view(B, 3, 3), g_T, None, None, None, None


def project(v, R, T, focal, S, pp=None):
    """world -> (x_ndc, y_ndc, z_view), MeshRasterizer.transform for PerspectiveCameras(in_ndc=False)."""
    ppx, ppy = (S / 2.0, S / 2.0) if pp is None else pp
    return _Project.apply(v, R, T, float(focal), float(ppx), float(ppy), int(S))


class _DepthRaster(torch.autograd.Function):
    """K=1 hard rasterisation returning (zbuf, face_id, ws); differentiable through zbuf."""

    @staticmethod
    def forward(ctx, ndc, faces, S):
        ndc = _f32(ndc)
        face_id, zbuf, _, ws = rasterize_fwd(ndc, faces, S, soft=False, want_zbuf=True)
        ctx.save_for_backward(face_id, ws, faces)
        ctx.meta = (ndc.shape, S)
        ctx.mark_non_differentiable(face_id, ws)
        return zbuf, face_id, ws

    @staticmethod
    def backward(ctx, g_z, _a, _b):
        face_id, ws, faces = ctx.saved_tensors
        shape, S = ctx.meta
        g_ndc = torch.zeros(shape, dtype=torch.float32, device=face_id.device)
        _lib.check(_lib.lib().harp_depth_bwd(_lib.ptr(face_id), _lib.ptr(ws), _lib.ptr(faces), _lib.ptr(_f32(g_z)), shape[0], shape[1],
                                             faces.shape[0], S, _lib.ptr(g_ndc), _lib.stream()), "harp_depth_bwd")
        return g_ndc, None, None


def depth_raster(ndc, faces, S):
    return _DepthRaster.apply(ndc, faces, S)


def _shade_args(face_id, ws, topo, verts, vnormals, tex, nmap, light_pos, colors, zl, light_R, light_T, S, focal, pp, bg):
    a = _lib.ShadeArgs()
    B, V, _ = verts.shape
    for k, t in (("face_id", face_id), ("recs", ws), ("faces", topo.faces), ("faces_uvs", topo.faces_uvs), ("verts_uvs", topo.verts_uvs),
                 ("verts", verts), ("vnormals", vnormals), ("tex", tex), ("nmap", nmap), ("light_pos", light_pos), ("colors", colors),
                 ("zl", zl), ("light_R", light_R), ("light_T", light_T)):
        setattr(a, k, _lib.ptr(t))
    a.B, a.V, a.F, a.S, a.Ht, a.Wt = B, V, topo.F, S, tex.shape[-3], tex.shape[-2]
    a.focal, a.ppx, a.ppy = focal, pp[0], pp[1]
    a.bg[0], a.bg[1], a.bg[2] = bg
    return a


# the shader backward's texel gradients as records + harp_texel_reduce (include/harp_hip.h: harp_shade_args.trec) instead of the in-kernel
# scatter; False: the table form.  Same gradients either way (tests/test_gpu_parity.py::test_texel_records_match_the_table_form).
TEXEL_RECORDS = True
_trec_cache = {}


def texel_record_capacity(n_pixels, div, floor):
    """capacity of one texel tile's record list (harp_shade_args.trec_cap): max(floor, n_pixels // div), rounded UP to a multiple of 4 —
    harp_shade_bwd and harp_texel_reduce refuse any other value"""
    cap = max(int(floor), int(n_pixels) // max(1, int(div)))
    return (cap + 3) & ~3


def texel_record_buffers(device, Ht, Wt, cap):
    """(records, counters, cap, double accumulators of both maps) for harp_shade_args.trec / trec_cnt / trec_cap and harp_texel_reduce /
    harp_texel_finish; None when the map has more tiles than the reduce handles"""
    nb = _lib.lib().harp_texel_bins(int(Ht), int(Wt))
    if nb > 1024:
        return None
    key = (str(device), int(Ht), int(Wt), int(cap))
    if key not in _trec_cache:
        _trec_cache.clear()
        _trec_cache[key] = (torch.empty(nb * 9 * int(cap), dtype=torch.float32, device=device),
                            torch.zeros(nb * 16 + 16, dtype=torch.int32, device=device), int(cap),
                            torch.zeros(2, int(Ht) * int(Wt) * 3, dtype=torch.float64, device=device))
    return _trec_cache[key]


class _Shade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ndc, verts, vnormals, tex, nmap, light_pos, colors, zl, light_R, light_T, face_id, ws, topo, S, focal, pp, bg):
        verts, vnormals, tex = _f32(verts), _f32(vnormals), _f32(tex)
        nmap = _f32(nmap) if nmap is not None else None
        light_pos, colors = _f32(light_pos), _f32(colors).reshape(9)
        if zl is not None:
            zl, light_R, light_T = _f32(zl), _f32(light_R).reshape(-1, 9), _f32(light_T)
        B = verts.shape[0]
        rgb = torch.empty(B, S, S, 3, dtype=torch.float32, device=verts.device)
        a = _shade_args(face_id, ws, topo, verts, vnormals, tex, nmap, light_pos, colors, zl, light_R, light_T, S, focal, pp, bg)
        a.rgb = _lib.ptr(rgb)
        _lib.check(_lib.lib().harp_shade_fwd(a, _lib.stream()), "harp_shade_fwd")
        ctx.save_for_backward(verts, vnormals, tex, nmap, light_pos, colors, zl, light_R, light_T, face_id, ws)
        ctx.meta = (topo, S, focal, pp, bg)
        return rgb

    @staticmethod
    def backward(ctx, g_rgb):
        verts, vnormals, tex, nmap, light_pos, colors, zl, light_R, light_T, face_id, ws = ctx.saved_tensors
        topo, S, focal, pp, bg = ctx.meta
        a = _shade_args(face_id, ws, topo, verts, vnormals, tex, nmap, light_pos, colors, zl, light_R, light_T, S, focal, pp, bg)
        g_rgb = _f32(g_rgb)
        z = torch.zeros_like
        g_ndc, g_verts, g_vn, g_tex = z(verts), z(verts), z(verts), z(tex)
        g_nmap = z(nmap) if nmap is not None else None
        g_lp, g_col = z(light_pos), z(colors)
        g_zl = z(zl) if zl is not None else None
        g_lR = z(light_R) if zl is not None else None
        g_lT = z(light_T) if zl is not None else None
        for k, t in (("g_rgb", g_rgb), ("g_tex", g_tex), ("g_nmap", g_nmap), ("g_verts", g_verts), ("g_vnormals", g_vn), ("g_ndc", g_ndc),
                     ("g_zl", g_zl), ("g_light_pos", g_lp), ("g_colors", g_col), ("g_light_R", g_lR), ("g_light_T", g_lT)):
            setattr(a, k, _lib.ptr(t))
        B = verts.shape[0]
        bufs = texel_record_buffers(verts.device, a.Ht, a.Wt, texel_record_capacity(B * S * S, 8, 4096)) if TEXEL_RECORDS else None
        if bufs is not None:
            a.trec, a.trec_cnt, a.trec_cap = _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), bufs[2]
            a.trec_acc_tex, a.trec_acc_nmap = _lib.ptr(bufs[3][0]), _lib.ptr(bufs[3][1])
        _lib.check(_lib.lib().harp_shade_bwd(a, _lib.stream()), "harp_shade_bwd")
        if bufs is not None:
            at, an = _lib.ptr(bufs[3][0]), (_lib.ptr(bufs[3][1]) if g_nmap is not None else None)
            _lib.check(_lib.lib().harp_texel_reduce(_lib.ptr(bufs[0]), _lib.ptr(bufs[1]), bufs[2], a.Ht, a.Wt, at, an, B * S * S // 6, _lib.stream()), "harp_texel_reduce")
            _lib.check(_lib.lib().harp_texel_finish(at, _lib.ptr(g_tex), an, _lib.ptr(g_nmap), None, a.Ht * a.Wt, _lib.stream()), "harp_texel_finish")
        return (g_ndc, g_verts, g_vn, g_tex, g_nmap, g_lp, g_col, g_zl, g_lR.view(B, 3, 3) if g_lR is not None else None, g_lT,
                None, None, None, None, None, None, None)


def shade(ndc, verts, vnormals, tex, nmap, light_pos, colors, face_id, ws, topo, S, focal, zl=None, light_R=None, light_T=None,
          pp=None, bg=(1.0, 1.0, 1.0)):
    """Fused K=1 shader (see csrc/shade.hip). `ndc` is only used to route the barycentric gradient."""
    pp = (S / 2.0, S / 2.0) if pp is None else pp
    return _Shade.apply(ndc, verts, vnormals, tex, nmap, light_pos, colors, zl, light_R, light_T, face_id, ws, topo, int(S), float(focal),
                        (float(pp[0]), float(pp[1])), tuple(float(x) for x in bg))


# ------------------------------------------------------------------------------------------------------
# fragment-level rasterisation (PyTorch3D's op pair; off the fitting loop's path)
# ------------------------------------------------------------------------------------------------------
class _RasterizeFragments(torch.autograd.Function):
    """_C.rasterize_meshes / _C.rasterize_meshes_backward for a batch sharing one face table."""

    @staticmethod
    def forward(ctx, ndc, faces, S, blur_radius, K):
        ndc = _f32(ndc)
        B, V, _ = ndc.shape
        F = faces.shape[0]
        dev = ndc.device
        ws = rasterize_workspace(B, F, S, dev)
        p2f = torch.empty(B, S, S, K, dtype=torch.int32, device=dev)
        zbuf = torch.empty(B, S, S, K, dtype=torch.float32, device=dev)
        bary = torch.empty(B, S, S, K, 3, dtype=torch.float32, device=dev)
        dists = torch.empty(B, S, S, K, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().harp_rasterize_fragments_fwd(_lib.ptr(ndc), _lib.ptr(faces), B, V, F, S, float(blur_radius), int(K), _lib.ptr(ws),
                                                           _lib.ptr(p2f), _lib.ptr(zbuf), _lib.ptr(bary), _lib.ptr(dists), _lib.stream()),
                   "harp_rasterize_fragments_fwd")
        ctx.save_for_backward(ndc, faces, p2f)
        ctx.meta = (S, float(blur_radius), int(K))
        ctx.mark_non_differentiable(p2f)
        return p2f, zbuf, bary, dists

    @staticmethod
    def backward(ctx, _g_p2f, g_zbuf, g_bary, g_dists):
        ndc, faces, p2f = ctx.saved_tensors
        S, blur_radius, K = ctx.meta
        B, V, _ = ndc.shape
        g_ndc = torch.zeros_like(ndc)
        c = lambda g: None if g is None else _f32(g)
        gz, gb, gd = c(g_zbuf), c(g_bary), c(g_dists)
        _lib.check(_lib.lib().harp_rasterize_fragments_bwd(_lib.ptr(ndc), _lib.ptr(faces), _lib.ptr(p2f), _lib.ptr(gz), _lib.ptr(gb), _lib.ptr(gd),
                                                           B, V, faces.shape[0], S, blur_radius, K, _lib.ptr(g_ndc), _lib.stream()),
                   "harp_rasterize_fragments_bwd")
        return g_ndc, None, None, None, None


def rasterize_fragments(ndc, faces, S, blur_radius=0.0, faces_per_pixel=1, packed=True):
    """ndc (B,V,3) = (x_ndc, y_ndc, z_view), faces (F,3) int32 -> pix_to_face (B,S,S,K) int64 [PyTorch3D's packed index b*F + f when
    `packed`, -1 empty], zbuf, bary (B,S,S,K,3), dists — the outputs of pytorch3d.renderer.mesh.rasterize_meshes, differentiable
    w.r.t. ndc through zbuf / bary / dists.  faces_per_pixel caps the number of fragments kept per pixel (1..64)."""
    p2f, zbuf, bary, dists = _RasterizeFragments.apply(ndc, faces, int(S), float(blur_radius), int(faces_per_pixel))
    p2f = p2f.long()
    if packed:
        off = (torch.arange(ndc.shape[0], device=ndc.device) * faces.shape[0]).view(-1, 1, 1, 1)
        p2f = torch.where(p2f >= 0, p2f + off, p2f)
    return p2f, zbuf, bary, dists


# ------------------------------------------------------------------------------------------------------
# post-fit evaluation metrics (csrc/metrics.hip): MS-SSIM, silhouette IoU, L1
# ------------------------------------------------------------------------------------------------------
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # pytorch_msssim 0.2.1 ms_ssim default
MS_SSIM_MIN_SIDE = (11 - 1) * 2 ** 4                          # its assertion: min(H, W) > 160


def check_forward_only(*ts):
    """the metrics have no backward: refuse to be part of an autograd graph rather than silently detach (nobody should take MS-SSIM
    for a loss here)"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        raise RuntimeError("image_metrics is forward-only (no MS-SSIM gradient): evaluate under torch.no_grad() or detach the inputs")


def image_metrics(ref, pred, ref_mask=None, pred_mask=None, channels_last=True, data_range=1.0, weights=None, win_sigma=1.5, K=(0.01, 0.03)):
    """Per-image evaluation metrics of utils/eval_util.py (image_eval :10-26) in one launch chain, forward only.

    ref / pred: float32 HIP tensors (N,H,W,C) (channels_last, the reference's render layout) or (N,C,H,W), C <= 3, read in place.
    ref_mask / pred_mask: optional (N,H,W[,1]) silhouettes (IoU of the >= 0.5 masks, :41-49).  MS-SSIM: pytorch_msssim 0.2.1
    ms_ssim(..., size_average=False) with an 11-tap window of `win_sigma` and len(weights) levels.  Returns a dict of per-image tensors:
    iou, l1 (mean |ref - pred|), l1_sum, inter, union, ms_ssim (N,), ssim and cs (N, levels, C) (means over each level's valid map)."""
    if not (torch.is_tensor(ref) and torch.is_tensor(pred)):
        raise TypeError("image_metrics takes tensors")
    check_forward_only(ref, pred)
    if not (ref.is_cuda and pred.is_cuda):
        raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
    if ref.dtype != torch.float32 or pred.dtype != torch.float32:
        raise TypeError(f"image_metrics takes float32 images, got {ref.dtype} / {pred.dtype}")
    if ref.dim() != 4 or ref.shape != pred.shape:
        raise ValueError(f"image_metrics takes two images of the same 4-D shape, got {tuple(ref.shape)} and {tuple(pred.shape)}")
    if ref.device != pred.device:
        raise ValueError("ref and pred live on different devices")
    if channels_last:
        N, H, W, C = ref.shape
    else:
        N, C, H, W = ref.shape
    weights = list(MS_SSIM_WEIGHTS if weights is None else [float(w) for w in weights])
    if not 1 <= len(weights) <= 5:
        raise ValueError(f"1 to 5 level weights, got {len(weights)}")
    if not 1 <= C <= 3:
        raise ValueError(f"1 to 3 channels, got {C}")
    if min(H, W) <= MS_SSIM_MIN_SIDE:
        raise ValueError(f"MS-SSIM needs both image sides > {MS_SSIM_MIN_SIDE} (pytorch_msssim's assertion), got {H} x {W}")
    if N > 65535:
        raise ValueError("at most 65535 images per call")
    if ref.stride() != pred.stride() or min(ref.stride()) < 0:
        ref, pred = ref.contiguous(), pred.contiguous()
    s = ref.stride()
    sn, sy, sx, sc = (s[0], s[1], s[2], s[3]) if channels_last else (s[0], s[2], s[3], s[1])
    masks = (ref_mask, pred_mask)
    if (ref_mask is None) != (pred_mask is None):
        raise ValueError("pass both masks or neither")
    if ref_mask is not None:
        masks = tuple(m.detach().reshape(N, H, W).to(device=ref.device, dtype=torch.float32).contiguous() for m in masks)
    dev = ref.device
    L = _lib.lib()
    ws = torch.empty(L.harp_image_metrics_ws_bytes(N, H, W), dtype=torch.uint8, device=dev)
    nl = len(weights)
    out = torch.empty(N, 4 + 2 * nl * C, dtype=torch.float32, device=dev)
    w = (ctypes.c_float * nl)(*weights)
    with torch.cuda.device(dev):
        rc = L.harp_image_metrics(ref.data_ptr(), pred.data_ptr(), _lib.ptr(masks[0]), _lib.ptr(masks[1]), sn, sc, sy, sx, N, C, H, W,
                                  float(data_range), w, nl, float(K[0]), float(K[1]), float(win_sigma), _lib.ptr(ws), _lib.ptr(out),
                                  _lib.stream())
    _lib.check(rc, "harp_image_metrics")
    inter, union = out[:, 0], out[:, 1]
    return {"iou": inter / union if ref_mask is not None else None, "l1": out[:, 2] / float(H * W * C), "l1_sum": out[:, 2],
            "inter": inter, "union": union, "ms_ssim": out[:, 3],
            "ssim": out[:, 4:4 + nl * C].reshape(N, nl, C), "cs": out[:, 4 + nl * C:].reshape(N, nl, C)}


# ------------------------------------------------------------------------------------------------------
# LPIPS v0.1 / AlexNet of the post-fit evaluation (csrc/lpips.hip)
# ------------------------------------------------------------------------------------------------------
LPIPS_MIN_SIDE = 31                       # below it the second 3x3 / stride-2 pool has no window (torch's layers fail there too)
LPIPS_ALEX_CONVS = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))    # (Cout, Cin, kernel) of features 0, 3, 6, 8, 10


def lpips_alex_pack(convs, lins, device):
    """Pack the LPIPS / AlexNet weights for csrc/lpips.hip: convs = five (weight (Cout,Cin,k,k), bias (Cout,)) pairs in torch's layout,
    lins = the five head weights ((1,C,1,1) or (C,)).  Returns the opaque net buffer (uint8 tensor on `device`)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
    ws, bs, ls = [], [], []
    for k, ((w, b), lin) in enumerate(zip(convs, lins)):
        co, ci, ks = LPIPS_ALEX_CONVS[k]
        if tuple(w.shape) != (co, ci, ks, ks) or tuple(b.shape) != (co,) or lin.numel() != co:
            raise ValueError(f"LPIPS layer {k}: weight {tuple(w.shape)}, bias {tuple(b.shape)}, lin {tuple(lin.shape)}; "
                             f"want ({co}, {ci}, {ks}, {ks}), ({co},), (1, {co}, 1, 1)")
        ws.append(w.detach().to(device, torch.float32).contiguous())
        bs.append(b.detach().to(device, torch.float32).contiguous())
        ls.append(lin.detach().reshape(-1).to(device, torch.float32).contiguous())
    L = _lib.lib()
    net = torch.empty(L.harp_lpips_alex_net_bytes(), dtype=torch.uint8, device=device)
    arr = lambda ts: (ctypes.c_void_p * 5)(*[t.data_ptr() for t in ts])      # noqa: E731
    with torch.cuda.device(device):
        rc = L.harp_lpips_alex_pack(arr(ws), arr(bs), arr(ls), net.data_ptr(), _lib.stream())
        _lib.check(rc, "harp_lpips_alex_pack")
        torch.cuda.current_stream().synchronize()      # (the float32 copies above are freed on return)
    return net


def lpips_alex(ref, pred, net, channels_last=True, normalize=False):
    """Per-image LPIPS v0.1 (net='alex', spatial=False) of utils/eval_util.py:51-53, forward only, in one launch chain.

    ref / pred: float32 HIP tensors (N,H,W,3) (channels_last, the reference's render layout) or (N,3,H,W), read in place; both sides
    >= 31 px.  net: lpips_alex_pack(...).  normalize=False (the reference's call) feeds the values as they are, i.e. as if in [-1, 1];
    normalize=True maps [0, 1] -> [-1, 1] first.  Returns (N, 6) float32: LPIPS, then the five taps' spatial means (relu1 .. relu5)."""
    if not (torch.is_tensor(ref) and torch.is_tensor(pred)):
        raise TypeError("lpips_alex takes tensors")
    check_forward_only(ref, pred)
    if not (ref.is_cuda and pred.is_cuda):
        raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
    if ref.dtype != torch.float32 or pred.dtype != torch.float32:
        raise TypeError(f"lpips_alex takes float32 images, got {ref.dtype} / {pred.dtype}")
    if ref.dim() != 4 or ref.shape != pred.shape:
        raise ValueError(f"lpips_alex takes two images of the same 4-D shape, got {tuple(ref.shape)} and {tuple(pred.shape)}")
    if ref.device != pred.device or not (torch.is_tensor(net) and net.device == ref.device):
        raise ValueError("ref, pred and the packed net must live on the same device")
    if channels_last:
        N, H, W, C = ref.shape
    else:
        N, C, H, W = ref.shape
    if C != 3:
        raise ValueError(f"LPIPS takes 3-channel images, got {C}")
    if min(H, W) < LPIPS_MIN_SIDE:
        raise ValueError(f"LPIPS / AlexNet needs both image sides >= {LPIPS_MIN_SIDE}, got {H} x {W}")
    if N > 65535:
        raise ValueError("at most 65535 images per call")
    if ref.stride() != pred.stride() or min(ref.stride()) < 0:
        ref, pred = ref.contiguous(), pred.contiguous()
    s = ref.stride()
    sn, sy, sx, sc = (s[0], s[1], s[2], s[3]) if channels_last else (s[0], s[2], s[3], s[1])
    dev = ref.device
    L = _lib.lib()
    ws = torch.empty(L.harp_lpips_alex_ws_bytes(N, H, W), dtype=torch.uint8, device=dev)
    out = torch.empty(N, 6, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = L.harp_lpips_alex(net.data_ptr(), ref.data_ptr(), pred.data_ptr(), sn, sc, sy, sx, N, H, W, int(bool(normalize)), _lib.ptr(ws),
                               _lib.ptr(out), _lib.stream())
    _lib.check(rc, "harp_lpips_alex")
    return out


# ------------------------------------------------------------------------------------------------------
# what a fit is looked at with (csrc/present.hip): the K-fragment normal image and the uint8 panel strips
# ------------------------------------------------------------------------------------------------------
NORMAL_IMAGE_MAX_K = 16


def normal_image(ndc, vnormals, faces, S, K=10, nmap=None, verts_uvs=None, faces_uvs=None, sigma=1e-4, gamma=1e-4, znear=1.0, zfar=100.0,
                 background=(1.0, 1.0, 1.0), check_uvs=True):
    """MeshRenderer(MeshRasterizer(K, blur 0), SoftPhongNormalShader) (renderer_helper.py:83-101, 216-301) in one kernel, forward only:
    ndc (B,V,3) from ops.project, vnormals (B,V,3), faces (F,3) int32 -> (B,S,S,4) float32 as softmax_rgb_blend returns it.  nmap: the
    NORMALISED normal map, (Ht,Wt,3) shared by the batch or (B,Ht,Wt,3), with verts_uvs (VT,2) / faces_uvs (F,3).  K = 1..16.  No tensor
    with a fragment dimension is allocated: output + the rasteriser workspace is all."""
    check_forward_only(ndc, vnormals, *([nmap] if nmap is not None else []))
    if not (ndc.is_cuda and vnormals.is_cuda and faces.is_cuda):
        raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
    B, V, _ = ndc.shape
    if vnormals.shape != ndc.shape:
        raise ValueError(f"vnormals {tuple(vnormals.shape)} must match ndc {tuple(ndc.shape)}")
    if not 1 <= int(K) <= NORMAL_IMAGE_MAX_K:
        raise ValueError(f"normal_image keeps 1 to {NORMAL_IMAGE_MAX_K} fragments per pixel, got K = {K}")
    ndc, vnormals = _f32(ndc.detach()), _f32(vnormals.detach())
    dev = ndc.device
    Fn = faces.shape[0]
    stride, Ht, Wt = 0, 0, 0
    if nmap is not None:
        if verts_uvs is None or faces_uvs is None:
            raise ValueError("a normal map needs verts_uvs and faces_uvs")
        nmap = _f32(nmap.detach())
        if nmap.dim() == 4 and nmap.shape[0] == 1:
            nmap = nmap[0]
        if nmap.dim() == 4:
            if nmap.shape[0] != B:
                raise ValueError(f"{nmap.shape[0]} normal maps for a batch of {B}")
            stride = nmap.shape[1] * nmap.shape[2] * 3
        if nmap.shape[-1] != 3:
            raise ValueError(f"normal map {tuple(nmap.shape)}: 3 channels last")
        Ht, Wt = nmap.shape[-3], nmap.shape[-2]
        verts_uvs = _f32(verts_uvs).reshape(-1, 2)
        faces_uvs = faces_uvs.to(torch.int32).reshape(-1, 3).contiguous()
        if faces_uvs.shape[0] != Fn:
            raise ValueError(f"faces_uvs has {faces_uvs.shape[0]} rows for {Fn} faces")
        if check_uvs:                                      # the kernel reads verts_uvs[faces_uvs] without a bounds check
            lo, hi = int(faces_uvs.min()), int(faces_uvs.max())
            if lo < 0 or hi >= verts_uvs.shape[0]:
                raise ValueError(f"faces_uvs must index verts_uvs ({verts_uvs.shape[0]} rows): found indices in [{lo}, {hi}]")
    ws = rasterize_workspace(B, Fn, int(S), dev)
    out = torch.empty(B, S, S, 4, dtype=torch.float32, device=dev)
    bg = (ctypes.c_float * 3)(*[float(x) for x in background])
    with torch.cuda.device(dev):
        rc = _lib.lib().harp_normal_image(_lib.ptr(ndc), _lib.ptr(vnormals), _lib.ptr(faces), B, V, Fn, int(S), int(K), float(sigma), float(gamma),
                                          float(znear), float(zfar), bg, _lib.ptr(nmap), stride, Ht, Wt, _lib.ptr(verts_uvs), _lib.ptr(faces_uvs),
                                          _lib.ptr(ws), _lib.ptr(out), _lib.stream())
    _lib.check(rc, "harp_normal_image")
    return out


def panels_u8(images, mask_true=None, mask_pred=None, channels_last=True):
    """The uint8 strip of optimize_sequence.py:744-755 on the device: `images` = up to three float32 HIP images (N,H,W,C >= 3) (or
    (N,C,H,W) with channels_last=False), read in place through their strides, each a panel uint8(trunc(clip(x, 0, 1) * 255)) of its first
    three channels; with both masks (N,H,W[,1]) one more panel (uint8(trunc(m_true * 225)), 0, uint8(trunc(m_pred * 225))).  Returns
    (N, H, P * W, 3) uint8 on the device — bit for bit what numpy gives.  One image and no masks: the clip * 255 -> uint8 of a render."""
    if torch.is_tensor(images):
        images = [images]
    images = list(images)
    if len(images) > 3:
        raise ValueError(f"at most three colour panels, got {len(images)}")
    if (mask_true is None) != (mask_pred is None):
        raise ValueError("pass both masks or neither")
    if not images and mask_true is None:
        raise ValueError("no panel to write")
    first = images[0] if images else mask_true
    if not first.is_cuda:
        raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
    dev = first.device
    shape = None
    ptrs, strides = [], []
    for im in images:
        if not im.is_cuda:
            raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
        if im.dtype != torch.float32 or im.dim() != 4:
            raise TypeError(f"panels_u8 takes 4-D float32 images, got {im.dtype} {tuple(im.shape)}")
        im = im.detach()
        if min(im.stride()) < 0:
            im = im.contiguous()
        N, H, W, C = im.shape if channels_last else (im.shape[0], im.shape[2], im.shape[3], im.shape[1])
        if C < 3:
            raise ValueError(f"a colour panel needs 3 channels, got {C}")
        if shape is not None and shape != (N, H, W):
            raise ValueError(f"panels of different sizes: {shape} and {(N, H, W)}")
        shape = (N, H, W)
        s = im.stride()
        strides += [s[0], s[1], s[2], s[3]] if channels_last else [s[0], s[2], s[3], s[1]]
        ptrs.append(im)
    masks = (None, None)
    if mask_true is not None:
        n = mask_true.shape[0]
        masks = tuple(m.detach().reshape(n, m.shape[1], m.shape[2]).to(device=dev, dtype=torch.float32).contiguous() for m in (mask_true, mask_pred))
        if shape is not None and tuple(masks[0].shape) != shape or masks[0].shape != masks[1].shape:
            raise ValueError(f"masks {tuple(masks[0].shape)} / {tuple(masks[1].shape)} do not match the images {shape}")
        shape = tuple(masks[0].shape)
    N, H, W = shape
    P = len(ptrs) + (masks[0] is not None)
    out = torch.empty(N, H, P * W, 3, dtype=torch.uint8, device=dev)
    pa = (ctypes.c_void_p * max(1, len(ptrs)))(*[t.data_ptr() for t in ptrs])
    sa = (ctypes.c_longlong * max(1, len(strides)))(*strides)
    with torch.cuda.device(dev):
        rc = _lib.lib().harp_panels_u8(pa, sa, len(ptrs), _lib.ptr(masks[0]), _lib.ptr(masks[1]), N, H, W, _lib.ptr(out), _lib.stream())
    _lib.check(rc, "harp_panels_u8")
    return out


SHEET_MODES = {"image": 0, "overlay": 1, "absdiff": 2, "normal": 3}
SHEET_MAX_D, SHEET_MAX_CELLS = 8, 64


def sheet_u8(a, b=None, mask=None, mode="image", grid=(3, 3), d=1, channels_last=True):
    """One uint8 contact sheet (csrc/sheet.hip; show_img_pair, optimize_sequence.py:37-64) in one launch: the frames of `a` (N,H,W,C >= 3)
    (or (N,C,H,W) with channels_last=False; (N,H,W[,1]) masks in "overlay" mode), float32 HIP tensors read in place through their
    strides, laid out edge to edge on a grid = (rows, cols) of cells of ceil(H / d) x ceil(W / d) pixels, each output pixel the float32
    box average of its d x d source pixels; cells past N are white.  mode "image": clip(a); "overlay": (clip(a), 0, clip(b)) with
    a = true and b = predicted mask; "absdiff": clip(|a * mask - b * mask|); "normal": clip(normalize(a) * 0.5 + 0.5).
    Returns (rows * ceil(H / d), cols * ceil(W / d), 3) uint8 on the device."""
    if mode not in SHEET_MODES:
        raise ValueError(f"mode is one of {sorted(SHEET_MODES)}, got {mode!r}")
    m = SHEET_MODES[mode]
    rows, cols, d = int(grid[0]), int(grid[1]), int(d)
    if (m in (1, 2)) != (b is not None) or (m == 2) != (mask is not None):
        raise ValueError(f"mode {mode!r} takes " + {0: "a", 1: "a and b", 2: "a, b and mask", 3: "a"}[m])

    def view(t, single):
        """tensor, (frame, row, column, channel) strides and (N,H,W) of an operand read in place"""
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"sheet_u8 takes float32 tensors, got {t.dtype}")
        t = t.detach()
        if t.dim() == 3 and single:
            t = t.unsqueeze(-1 if channels_last else 1)
        if t.dim() != 4:
            raise TypeError(f"sheet_u8 takes (N,H,W,C) frames{' or (N,H,W) masks' if single else ''}, got {tuple(t.shape)}")
        if min(t.stride()) < 0:
            t = t.contiguous()
        if not channels_last:
            t = t.permute(0, 2, 3, 1)
        if t.shape[3] < (1 if single else 3):
            raise ValueError(f"a colour frame needs 3 channels, got {t.shape[3]}")
        if single and t.shape[3] != 1:
            raise ValueError(f"a mask has one channel, got {t.shape[3]}")
        return t, list(t.stride()), tuple(t.shape[:3])

    ta, sa, shape = view(a, m == 1)
    tb = sb = tm = sm = None
    if b is not None:
        tb, sb, shape_b = view(b, m == 1)
        if shape_b != shape:
            raise ValueError(f"a {shape} and b {shape_b} differ in size")
    if mask is not None:
        tm, sm, shape_m = view(mask, True)
        if shape_m != shape:
            raise ValueError(f"a {shape} and mask {shape_m} differ in size")
    N, H, W = shape
    if rows < 1 or cols < 1 or rows * cols > SHEET_MAX_CELLS or not 1 <= d <= SHEET_MAX_D:
        raise ValueError(f"grid of 1..{SHEET_MAX_CELLS} cells and d in 1..{SHEET_MAX_D}, got {rows} x {cols}, d = {d}")
    if not 1 <= N <= rows * cols or H < 1 or W < 1:
        raise ValueError(f"{N} frames of {H} x {W} do not fit a {rows} x {cols} sheet")
    out = torch.empty(rows * -(-H // d), cols * -(-W // d), 3, dtype=torch.uint8, device=ta.device)
    ll = lambda s, n: None if s is None else (ctypes.c_longlong * n)(*s[:n])
    with torch.cuda.device(ta.device):
        rc = _lib.lib().harp_sheet_u8(m, ta.data_ptr(), ll(sa, 4), None if tb is None else tb.data_ptr(), ll(sb, 4),
                                      None if tm is None else tm.data_ptr(), ll(sm, 3), N, H, W, rows, cols, d, _lib.ptr(out), _lib.stream())
    _lib.check(rc, "harp_sheet_u8")
    return out


INGEST_MAX_D = 8


def targets_from_u8(rgb, mask, d=1, eroded=True, out=None):
    """The three resident targets of a fit from decoded uint8 frames (csrc/ingest.hip; everything behind the image decoder in
    utils/data_util.py:11-51) in one launch, forward only: rgb (N,H0,W0,3) and mask (N,H0,W0) uint8 HIP tensors ->
    (y_true (N,H,W,3), y_sil (N,H,W), y_sil_col (N,H,W)) float32 with H = ceil(H0 / d), W = ceil(W0 / d) — `img[::d, ::d] / 255` and, for
    y_sil_col, the mask eroded twice with a 3 x 3 square (out-of-image neighbours ignored), bit for bit what ImagesDataset yields.
    eroded=False skips the erosion and returns None in its place.  out = (y_true, y_sil, y_sil_col): contiguous float32 tensors of those
    shapes to write into, e.g. slices [n0 : n0 + N] of larger buffers (out[2] is neither read nor written with eroded=False)."""
    for name, t in (("rgb", rgb), ("mask", mask)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
        if t.dtype != torch.uint8:
            raise TypeError(f"targets_from_u8 takes uint8 tensors, got {name} {t.dtype}")
    if rgb.dim() != 4 or rgb.shape[3] != 3:
        raise TypeError(f"targets_from_u8 takes (N,H0,W0,3) frames, got {tuple(rgb.shape)}")
    N, H0, W0 = rgb.shape[:3]
    if tuple(mask.shape) != (N, H0, W0) or mask.device != rgb.device:
        raise ValueError(f"rgb {tuple(rgb.shape)} on {rgb.device} and mask {tuple(mask.shape)} on {mask.device} do not match")
    d = int(d)
    if not 1 <= d <= INGEST_MAX_D or N < 1 or H0 < 1 or W0 < 1:
        raise ValueError(f"at least one frame of at least one pixel and d in 1..{INGEST_MAX_D}, got {tuple(rgb.shape)}, d = {d}")
    H, W = -(-H0 // d), -(-W0 // d)
    shapes = ((N, H, W, 3), (N, H, W), (N, H, W))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=rgb.device) if (k < 2 or eroded) else None for k, s in enumerate(shapes))
    else:
        out = tuple(out)
        if len(out) != 3:
            raise ValueError("out = (y_true, y_sil, y_sil_col)")
        for k, (t, s) in enumerate(zip(out, shapes)):
            if k == 2 and not eroded:
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != s or t.device != rgb.device or not t.is_contiguous():
                raise ValueError(f"out[{k}] must be a contiguous float32 tensor {s} on {rgb.device}")
    with torch.cuda.device(rgb.device):
        rc = _lib.lib().harp_targets_from_u8(_lib.ptr(rgb), _lib.ptr(mask), N, H0, W0, d, _lib.ptr(out[0]), _lib.ptr(out[1]),
                                             _lib.ptr(out[2]) if eroded else None, _lib.stream())
    _lib.check(rc, "harp_targets_from_u8")
    return out[0], out[1], (out[2] if eroded else None)


# ------------------------------------------------------------------------------------------------------
# export of the fitted avatar (csrc/smooth.hip): Taubin smoothing of the meshes that save_obj writes
# ------------------------------------------------------------------------------------------------------
TAUBIN_LDS_MAX_V = 4096                                  # vertices one workgroup keeps resident in LDS (mode 1)


def taubin_smooth(verts, topo, lambd=0.53, mu=-0.53, num_iter=10, mode=0):
    """The passes of pytorch3d.ops.taubin_smoothing (optimize_sequence.py:780) on plain tensors, forward only: verts (B,V,3) or (V,3)
    float32 HIP tensor (any strides), topo = anything with the vertex -> neighbour CSR `nbr_off` (V+1) / `nbr_idx` int32 on the same device
    (a DeviceTopology) -> a new tensor of the same shape.  mode 0 picks the kernel, 1 = LDS-resident (V <= TAUBIN_LDS_MAX_V), 2 = one
    launch per pass through a workspace.  A vertex without neighbours keeps its position (PyTorch3D: NaN)."""
    if torch.is_grad_enabled() and verts.requires_grad:
        raise NotImplementedError("taubin_smooth is forward-only (the reference calls it under torch.no_grad()): detach the vertices")
    if not verts.is_cuda:
        raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
    if verts.dim() not in (2, 3) or verts.shape[-1] != 3:
        raise ValueError(f"taubin_smooth takes (B,V,3) or (V,3) vertices, got {tuple(verts.shape)}")
    v = _f32(verts.detach())
    v3 = v.reshape(-1, v.shape[-2], 3)
    B, V = v3.shape[0], v3.shape[1]
    if topo.nbr_off.numel() != V + 1:
        raise ValueError(f"the neighbour table is for {topo.nbr_off.numel() - 1} vertices, the mesh has {V}")
    if int(num_iter) < 0 or int(mode) not in (0, 1, 2):
        raise ValueError(f"num_iter >= 0 and mode in (0, 1, 2), got {num_iter}, {mode}")
    if int(mode) == 1 and V > TAUBIN_LDS_MAX_V:
        raise ValueError(f"mode 1 keeps at most {TAUBIN_LDS_MAX_V} vertices in LDS, the mesh has {V}")
    out = torch.empty_like(v3)
    if B == 0 or V == 0:
        return out.reshape(v.shape)
    L = _lib.lib()
    ws = None
    if int(num_iter) > 0 and (int(mode) == 2 or V > TAUBIN_LDS_MAX_V):
        ws = torch.empty(L.harp_taubin_ws_bytes(B, V), dtype=torch.uint8, device=v.device)
    with torch.cuda.device(v.device):
        rc = L.harp_taubin_smooth(_lib.ptr(v3), _lib.ptr(topo.nbr_off), _lib.ptr(topo.nbr_idx), B, V, float(lambd), float(mu), int(num_iter),
                                  int(mode), _lib.ptr(out), _lib.ptr(ws), _lib.stream())
    _lib.check(rc, "harp_taubin_smooth")
    return out.reshape(v.shape)


def taubin_smoothing(meshes, lambd=0.53, mu=-0.53, num_iter=10):
    """pytorch3d.ops.taubin_smoothing(meshes, lambd, mu, num_iter) as optimize_sequence.py:780 calls it: a new harp_amd.structures.Meshes
    with smoothed vertices and the same faces, textures and topology."""
    from .structures import Meshes
    return Meshes(taubin_smooth(meshes.verts_padded(), meshes.topo, lambd, mu, num_iter), meshes.faces_padded(), meshes.textures, meshes.topo)


# ------------------------------------------------------------------------------------------------------
# geometric accuracy of the post-fit evaluation (csrc/pose_eval.hip): Procrustes, PCK counts, F-score
# ------------------------------------------------------------------------------------------------------
FSCORE_MAX_THRESHOLDS = 512                              # harp_point_set_fscore keeps 16 counters per threshold in LDS


def _pose_eval_input(name, what, *ts):
    for t in ts:
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise TypeError(f"{name} takes tensors")
        if torch.is_grad_enabled() and t.requires_grad:
            raise NotImplementedError(f"{name} is forward-only ({what}): detach the inputs or evaluate under torch.no_grad()")
        if not t.is_cuda:
            raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
        if t.device != ts[0].device:
            raise ValueError(f"{name}: the tensors live on different devices")


def procrustes_align(gt, pred, valid=None, pred_idx=None, return_trafo=False):
    """align_w_scale (utils/eval_util.py:212-235) for N frames in one launch, forward only, float64 inside (include/harp_hip.h).

    gt (N,K,3) or (K,3), pred (N,Kp,3) or (Kp,3) HIP tensors; pred_idx: K indices into the Kp points (the gather without a copy), else
    Kp = K; valid (N,K) or (K,), non-zero = the point is used.  Returns (aligned, err, n_valid): float32 (N,K,3) and (N,K), NaN at points
    not used and in frames with fewer than 3 used points, and int32 (N,) — without the leading axis for (K,3) inputs.  With return_trafo a
    fourth tensor: (N,14) float64 = R row-major, s, s1, t1 - t2 (the reference's tuple).  No determinant correction: a mirrored
    prediction is aligned by a reflection, as scipy's orthogonal_procrustes does."""
    _pose_eval_input("procrustes_align", "no gradient through the alignment", gt, pred, valid, pred_idx)
    if gt.dim() not in (2, 3) or gt.shape[-1] != 3 or pred.dim() != gt.dim() or pred.shape[-1] != 3:
        raise ValueError(f"procrustes_align takes (N,K,3) or (K,3) point sets, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    single = gt.dim() == 2
    g = _f32(gt.detach()).reshape(-1, gt.shape[-2], 3)
    p = _f32(pred.detach()).reshape(-1, pred.shape[-2], 3)
    N, K, Kp = g.shape[0], g.shape[1], p.shape[1]
    if p.shape[0] != N:
        raise ValueError(f"{N} frames of ground truth, {p.shape[0]} of prediction")
    if pred_idx is not None:
        pred_idx = pred_idx.detach().to(torch.int32).contiguous().reshape(-1)
        if pred_idx.numel() != K:
            raise ValueError(f"pred_idx holds {pred_idx.numel()} indices, the ground truth {K} points")
    elif Kp != K:
        raise ValueError(f"{K} points of ground truth, {Kp} of prediction and no pred_idx")
    if valid is not None:
        valid = valid.detach().to(torch.float32).contiguous()
        if valid.numel() != N * K:
            raise ValueError(f"valid has {valid.numel()} entries for {N} x {K} points")
    if N == 0 or K == 0 or Kp == 0:
        raise ValueError("procrustes_align needs at least one frame and one point")
    dev = g.device
    aligned = torch.empty(N, K, 3, dtype=torch.float32, device=dev)
    err = torch.empty(N, K, dtype=torch.float32, device=dev)
    n_valid = torch.empty(N, dtype=torch.int32, device=dev)
    trafo = torch.empty(N, 14, dtype=torch.float64, device=dev) if return_trafo else None
    with torch.cuda.device(dev):
        rc = _lib.lib().harp_procrustes_align(_lib.ptr(g), _lib.ptr(p), _lib.ptr(pred_idx), _lib.ptr(valid), N, K, Kp, _lib.ptr(aligned),
                                              _lib.ptr(err), _lib.ptr(trafo), _lib.ptr(n_valid), _lib.stream())
    _lib.check(rc, "harp_procrustes_align")
    out = (aligned[0], err[0], n_valid[0]) if single else (aligned, err, n_valid)
    return out + ((trafo[0] if single else trafo),) if return_trafo else out


def pck_counts(err, valid, thresholds):
    """The counting of EvalUtil.get_measures (utils/eval_util.py:103-163) per keypoint: err (N,K) float32 HIP tensor, valid (N,K) or None
    (non-zero = visible), thresholds (n_thr,).  A measurement is seen when it is visible and not NaN.  Returns (counts (K,n_thr) int32 =
    seen n with err <= threshold in float32, n_vis (K,) int32, err_sum (K,) float64)."""
    _pose_eval_input("pck_counts", "counts have no gradient", err, valid, thresholds)
    if err.dim() != 2:
        raise ValueError(f"pck_counts takes (N,K) errors, got {tuple(err.shape)}")
    e = _f32(err.detach())
    N, K = e.shape
    thr = thresholds.detach().to(torch.float32).contiguous().reshape(-1)
    if valid is not None:
        valid = valid.detach().to(torch.float32).contiguous()
        if valid.numel() != N * K:
            raise ValueError(f"valid has {valid.numel()} entries for {N} x {K} errors")
    if N == 0 or K == 0 or thr.numel() < 1:
        raise ValueError("pck_counts needs at least one frame, one keypoint and one threshold")
    dev = e.device
    counts = torch.empty(K, thr.numel(), dtype=torch.int32, device=dev)
    n_vis = torch.empty(K, dtype=torch.int32, device=dev)
    err_sum = torch.empty(K, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().harp_pck_counts(_lib.ptr(e), _lib.ptr(valid), _lib.ptr(thr), N, K, thr.numel(), _lib.ptr(counts), _lib.ptr(n_vis),
                                        _lib.ptr(err_sum), _lib.stream())
    _lib.check(rc, "harp_pck_counts")
    return counts, n_vis, err_sum


def point_set_fscore(gt, pred, thresholds):
    """Precision, recall and F between two point sets per frame (the mesh measure of the FreiHAND benchmark; include/harp_hip.h): gt
    (N,Kg,3) or (Kg,3), pred (N,Kp,3) or (Kp,3) float32 HIP tensors, thresholds (n_thr,) distances in the points' unit.  All pairs in
    float64; a point counts when its nearest neighbour in the other set is strictly nearer than the threshold.  Returns (out (N,n_thr,3) =
    precision, recall, F; nn_gt (N,Kg), nn_pred (N,Kp) nearest distances) — without the leading axis for 2-D inputs."""
    _pose_eval_input("point_set_fscore", "counts have no gradient", gt, pred, thresholds)
    if gt.dim() not in (2, 3) or gt.shape[-1] != 3 or pred.dim() != gt.dim() or pred.shape[-1] != 3:
        raise ValueError(f"point_set_fscore takes (N,K,3) or (K,3) point sets, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    single = gt.dim() == 2
    g = _f32(gt.detach()).reshape(-1, gt.shape[-2], 3)
    p = _f32(pred.detach()).reshape(-1, pred.shape[-2], 3)
    N, Kg, Kp = g.shape[0], g.shape[1], p.shape[1]
    thr = thresholds.detach().to(torch.float32).contiguous().reshape(-1)
    if p.shape[0] != N:
        raise ValueError(f"{N} frames of ground truth, {p.shape[0]} of prediction")
    if N == 0 or Kg == 0 or Kp == 0 or not 1 <= thr.numel() <= FSCORE_MAX_THRESHOLDS:
        raise ValueError(f"point_set_fscore needs at least one frame, one point per set and 1 to {FSCORE_MAX_THRESHOLDS} thresholds")
    dev = g.device
    out = torch.empty(N, thr.numel(), 3, dtype=torch.float32, device=dev)
    nn_gt = torch.empty(N, Kg, dtype=torch.float32, device=dev)
    nn_pred = torch.empty(N, Kp, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().harp_point_set_fscore(_lib.ptr(g), _lib.ptr(p), _lib.ptr(thr), N, Kg, Kp, thr.numel(), _lib.ptr(out), _lib.ptr(nn_gt),
                                              _lib.ptr(nn_pred), _lib.stream())
    _lib.check(rc, "harp_point_set_fscore")
    return (out[0], nn_gt[0], nn_pred[0]) if single else (out, nn_gt, nn_pred)


# ------------------------------------------------------------------------------------------------------
# the frames baked into UV space (csrc/bake.hip): texel map, per-texel accumulation, finish, seam dilation
# ------------------------------------------------------------------------------------------------------
BAKE_DEFAULTS = dict(depth_tol=4e-3, cos_min=0.2, cos_power=2.0, shade_floor=0.1)      # parameters of the bake, not tolerances


def _bake_input(name, *ts):
    check_forward_only(*[t for t in ts if t is not None])
    for t in ts:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"{name}: harp_amd ops need HIP device tensors (no CPU path)")


def uv_texel_map(verts_uvs, faces_uvs, Ht, Wt):
    """The UV triangles rasterised at the texel centres of an (Ht, Wt) atlas, forward only: verts_uvs (VT,2) float32, faces_uvs (F,3)
    int32 HIP tensors -> (texel_face (Ht,Wt) int32: the owning face, the lowest index where several contain the centre, or -1;
    texel_bary (Ht,Wt,2) float32: b0, b1 with b2 = 1 - b0 - b1).  Texel (x, y) <-> u = x / (Wt - 1), v = 1 - y / (Ht - 1)."""
    _bake_input("uv_texel_map", verts_uvs, faces_uvs)
    vu = _f32(verts_uvs.detach()).reshape(-1, 2)
    fu = faces_uvs.detach().to(torch.int32).reshape(-1, 3).contiguous()
    Ht, Wt = int(Ht), int(Wt)
    if vu.shape[0] < 1 or fu.shape[0] < 1 or Ht < 2 or Wt < 2:
        raise ValueError(f"uv_texel_map needs at least one UV vertex, one face and a 2 x 2 atlas, got {tuple(vu.shape)}, {tuple(fu.shape)}, {Ht} x {Wt}")
    face = torch.empty(Ht, Wt, dtype=torch.int32, device=vu.device)
    bary = torch.empty(Ht, Wt, 2, dtype=torch.float32, device=vu.device)
    with torch.cuda.device(vu.device):
        rc = _lib.lib().harp_uv_texel_map(_lib.ptr(vu), _lib.ptr(fu), fu.shape[0], vu.shape[0], Ht, Wt, _lib.ptr(face), _lib.ptr(bary), _lib.stream())
    _lib.check(rc, "harp_uv_texel_map")
    return face, bary


def bake_accumulators(Ht, Wt, device):
    """zeroed accumulators of texture_bake_accum: dict of sum_w (Ht,Wt), sum_wc, sum_wc2 (Ht,Wt,3) float64, count (Ht,Wt) int32 and
    best_cos (Ht,Wt) float32 (-1: never seen)"""
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=device)      # noqa: E731
    return {"sum_w": z(Ht, Wt), "sum_wc": z(Ht, Wt, 3), "sum_wc2": z(Ht, Wt, 3), "count": z(Ht, Wt, dt=torch.int32),
            "best_cos": torch.full((Ht, Wt), -1.0, dtype=torch.float32, device=device)}


def texture_bake_accum(acc, texel_face, texel_bary, faces, ndc, face_id, zbuf, y_true, y_mask, rows, texel_idx=None, verts=None, vnormals=None,
                       cam_pos=None, light_pos=None, colors=None, depth_tol=BAKE_DEFAULTS["depth_tol"], cos_min=BAKE_DEFAULTS["cos_min"],
                       cos_power=BAKE_DEFAULTS["cos_power"], shade_floor=BAKE_DEFAULTS["shade_floor"]):
    """Add the B frames of one call to the per-texel accumulators `acc` (bake_accumulators), in place and in frame order (include/harp_hip.h:
    harp_texture_bake_accum).  texel_face / texel_bary from uv_texel_map; faces (F,3) int32; ndc (B,V,3) from ops.project; face_id / zbuf
    (B,S,S) from the hard rasterize_fwd; y_true (N,S,S,3), y_mask (N,S,S) and rows (B,) int32 into them; texel_idx: int32 list of covered
    texels (None: all).  verts / vnormals (B,V,3) and cam_pos (B,3) switch the viewing-angle test and weight on, light_pos (B,3) and
    colors (B,9) the division by the Lambert shading.  Cutting a sequence into calls differently gives the same bits.  Returns acc."""
    ts = (texel_face, texel_bary, faces, ndc, face_id, zbuf, y_true, y_mask, rows, texel_idx, verts, vnormals, cam_pos, light_pos, colors)
    _bake_input("texture_bake_accum", *ts, *acc.values())
    Ht, Wt = texel_face.shape
    B, V, _ = ndc.shape
    S, N = face_id.shape[-1], y_true.shape[0]
    if tuple(face_id.shape) != (B, S, S) or tuple(zbuf.shape) != (B, S, S) or tuple(y_true.shape) != (N, S, S, 3) or y_mask.numel() != N * S * S:
        raise ValueError(f"face_id {tuple(face_id.shape)}, zbuf {tuple(zbuf.shape)}, y_true {tuple(y_true.shape)}, y_mask {tuple(y_mask.shape)} "
                         f"do not fit {B} frames of {S} x {S}")
    if rows.numel() != B or tuple(texel_bary.shape) != (Ht, Wt, 2) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"rows {tuple(rows.shape)} for {B} frames, texel_bary {tuple(texel_bary.shape)} for a {Ht} x {Wt} atlas, faces {tuple(faces.shape)}")
    for name, t, shape in (("verts", verts, (B, V, 3)), ("vnormals", vnormals, (B, V, 3)), ("cam_pos", cam_pos, (B, 3)),
                           ("light_pos", light_pos, (B, 3)), ("colors", colors, (B, 9))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} {tuple(t.shape)}: expected {shape}")
    for k, (dt, shape) in {"sum_w": (torch.float64, (Ht, Wt)), "sum_wc": (torch.float64, (Ht, Wt, 3)), "sum_wc2": (torch.float64, (Ht, Wt, 3)),
                           "count": (torch.int32, (Ht, Wt)), "best_cos": (torch.float32, (Ht, Wt))}.items():
        if acc[k].dtype != dt or tuple(acc[k].shape) != shape or not acc[k].is_contiguous():
            raise ValueError(f"acc[{k!r}] must be a contiguous {dt} tensor {shape}")
    i32 = lambda t: None if t is None else t.detach().to(torch.int32).contiguous()      # noqa: E731
    f32 = lambda t: None if t is None else _f32(t.detach())                              # noqa: E731
    keep = dict(texel_idx=i32(texel_idx), texel_face=i32(texel_face), texel_bary=f32(texel_bary), faces=i32(faces), ndc=f32(ndc),
                face_id=i32(face_id), zbuf=f32(zbuf), y_true=f32(y_true), y_mask=f32(y_mask), rows=i32(rows), verts=f32(verts),
                vnormals=f32(vnormals), cam_pos=f32(cam_pos), light_pos=f32(light_pos), colors=f32(colors))
    a = _lib.BakeArgs()
    for k, t in keep.items():
        setattr(a, k, _lib.ptr(t))
    for k, t in acc.items():
        setattr(a, k, _lib.ptr(t))
    a.n = keep["texel_idx"].numel() if texel_idx is not None else Ht * Wt
    a.Ht, a.Wt, a.F, a.V, a.B, a.S, a.N = Ht, Wt, faces.shape[0], V, B, S, N
    a.depth_tol, a.cos_min, a.cos_power, a.shade_floor = float(depth_tol), float(cos_min), float(cos_power), float(shade_floor)
    if a.n == 0:
        return acc
    with torch.cuda.device(ndc.device):
        rc = _lib.lib().harp_texture_bake_accum(ctypes.byref(a), _lib.stream())
    _lib.check(rc, "harp_texture_bake_accum")
    return acc


def texture_bake_finish(acc, min_count=1):
    """accumulators -> (mean (Ht,Wt,3) float32 = clamp(sum_wc / sum_w, 0, 1), var (Ht,Wt,3) = max(sum_wc2 / sum_w - mean^2, 0) of the
    unclamped mean, seen (Ht,Wt) uint8 = count >= min_count and sum_w > 0); mean and var are 0 where not seen."""
    _bake_input("texture_bake_finish", *acc.values())
    Ht, Wt = acc["sum_w"].shape
    dev = acc["sum_w"].device
    mean = torch.empty(Ht, Wt, 3, dtype=torch.float32, device=dev)
    var = torch.empty_like(mean)
    seen = torch.empty(Ht, Wt, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().harp_texture_bake_finish(_lib.ptr(acc["sum_w"]), _lib.ptr(acc["sum_wc"]), _lib.ptr(acc["sum_wc2"]), _lib.ptr(acc["count"]),
                                                 Ht, Wt, int(min_count), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(seen), _lib.stream())
    _lib.check(rc, "harp_texture_bake_finish")
    return mean, var, seen


def texture_dilate(tex, valid, n_pass, allow=None, out=None):
    """n_pass 3 x 3 Jacobi passes over tex (Ht,Wt,C <= 4) float32 and valid (Ht,Wt) (non-zero = valid): an invalid texel with a valid
    8-neighbour becomes the float32 mean of its valid neighbours and is valid from the next pass on; allow (Ht,Wt): texels with 0 are
    never filled and never sources.  out: None (a new tensor) or a contiguous tensor like tex, which may be tex itself.  Returns
    (out, valid_out uint8)."""
    _bake_input("texture_dilate", tex, valid, allow, out)
    if tex.dim() != 3 or not 1 <= tex.shape[2] <= 4 or tex.dtype != torch.float32:
        raise ValueError(f"texture_dilate takes a float32 (Ht,Wt,C <= 4) map, got {tex.dtype} {tuple(tex.shape)}")
    Ht, Wt, C = tex.shape
    if tuple(valid.shape) != (Ht, Wt) or (allow is not None and tuple(allow.shape) != (Ht, Wt)) or int(n_pass) < 0 or Ht < 1 or Wt < 1:
        raise ValueError(f"valid / allow must be ({Ht}, {Wt}) and n_pass >= 0")
    u8 = lambda t: None if t is None else (t != 0).to(torch.uint8).contiguous()      # noqa: E731
    src = tex.detach() if tex.is_contiguous() else tex.detach().contiguous()
    if out is None:
        out = torch.empty_like(src)
    elif out.dtype != torch.float32 or tuple(out.shape) != (Ht, Wt, C) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor ({Ht}, {Wt}, {C})")
    v, al = u8(valid), u8(allow)
    v_out = torch.empty(Ht, Wt, dtype=torch.uint8, device=src.device)
    L = _lib.lib()
    ws = torch.empty(L.harp_texture_dilate_ws_bytes(Ht, Wt, C), dtype=torch.uint8, device=src.device) if int(n_pass) > 0 else None
    with torch.cuda.device(src.device):
        rc = L.harp_texture_dilate(_lib.ptr(src), _lib.ptr(v), _lib.ptr(al), Ht, Wt, C, int(n_pass), _lib.ptr(out), _lib.ptr(v_out), _lib.ptr(ws),
                                   _lib.stream())
    _lib.check(rc, "harp_texture_dilate")
    return out, v_out


# ------------------------------------------------------------------------------------------------------
# playback of a fitted avatar (csrc/playback.hip): motion resampling, supersampled float render -> uint8 frames
# ------------------------------------------------------------------------------------------------------
RESOLVE_MAX_SS = 4


def _playback_input(name, *ts):
    first = None
    for t in ts:
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError("harp_amd ops need HIP device tensors (no CPU path)")
        if first is not None and t.device != first.device:
            raise ValueError(f"{name}: tensors on {first.device} and {t.device}")
        first = t if first is None else first
    check_forward_only(*[t for t in ts if t is not None and t.is_floating_point()])


def _background_input(background, bg_rows, bg_color, B, S, device):
    """resolve_u8's checks of (background, bg_rows, bg_color) -> (background, n_bg, bg_rows, the colour as a (3,) float32 device tensor)"""
    n_bg = 0
    if background is not None:
        if background.dtype != torch.uint8 or background.dim() != 4 or tuple(background.shape[1:]) != (S, S, 3) or background.shape[0] < 1:
            raise TypeError(f"background must be uint8 (n_bg, {S}, {S}, 3), got {background.dtype} {tuple(background.shape)}")
        n_bg = background.shape[0]
        if bg_rows is None and n_bg not in (1, B):
            raise ValueError(f"{n_bg} backgrounds for {B} frames: pass bg_rows")
        background = background.contiguous()
    if bg_rows is not None:
        if bg_rows.dtype != torch.int32 or tuple(bg_rows.shape) != (B,):
            raise TypeError(f"bg_rows must be int32 ({B},), got {bg_rows.dtype} {tuple(bg_rows.shape)}")
        bg_rows = bg_rows.contiguous()
    if torch.is_tensor(bg_color):
        if bg_color.dtype != torch.float32 or tuple(bg_color.shape) != (3,):
            raise TypeError(f"bg_color must be three numbers or a float32 (3,) tensor, got {bg_color.dtype} {tuple(bg_color.shape)}")
        return background, n_bg, bg_rows, bg_color.detach().contiguous()
    return background, n_bg, bg_rows, torch.tensor([float(c) for c in bg_color], dtype=torch.float32).reshape(3).to(device)


def _frames_out(out, B, S, C, device):
    """the (B,S,S,C) uint8 frames to write into: the caller's `out` checked, or new ones"""
    if out is None:
        return torch.empty(B, S, S, C, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (B, S, S, C) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor {(B, S, S, C)}")
    return out


def _scene_depth_input(name, scene_depth, scene_rows, B, S):
    """the checks of (scene_depth, scene_rows) of composite_layers_u8 and the label ops -> (scene_depth, scene_rows, n_scene), contiguous"""
    n_scene = 0
    if scene_depth is not None:
        if scene_depth.dtype != torch.float32 or scene_depth.dim() != 3 or tuple(scene_depth.shape[1:]) != (S, S) or scene_depth.shape[0] < 1:
            raise TypeError(f"scene_depth must be float32 (n_scene, {S}, {S}), got {scene_depth.dtype} {tuple(scene_depth.shape)}")
        n_scene = scene_depth.shape[0]
        if scene_rows is None and n_scene not in (1, B):
            raise ValueError(f"{n_scene} scene depths for {B} frames: pass scene_rows")
        scene_depth = scene_depth.detach().contiguous()
    if scene_rows is not None:
        if scene_depth is None:
            raise ValueError("scene_rows without a scene_depth")
        if scene_rows.dtype != torch.int32 or tuple(scene_rows.shape) != (B,):
            raise TypeError(f"scene_rows must be int32 ({B},), got {scene_rows.dtype} {tuple(scene_rows.shape)}")
        scene_rows = scene_rows.contiguous()
    return scene_depth, scene_rows, n_scene


def motion_resample(keys, times, n_rot, rot_offset=None):
    """Key-frame rows at fractional times (csrc/playback.hip: harp_motion_resample), forward only: keys (Tk, 3 n_rot + n_lin) float32 =
    n_rot axis-angle triples then n_lin linear channels, times (Tn,) float32 in key-frame units (clamped to [0, Tk - 1]) ->
    (Tn, 3 n_rot + n_lin).  The triples are interpolated as rotations (shortest-arc slerp) after rot_offset (3 n_rot,) — the model's pose
    mean — has been added; a time on a key returns that row bit for bit."""
    _playback_input("motion_resample", keys, times, rot_offset)
    n_rot = int(n_rot)
    if keys.dtype != torch.float32 or times.dtype != torch.float32 or (rot_offset is not None and rot_offset.dtype != torch.float32):
        raise TypeError("motion_resample takes float32 tensors")
    if keys.dim() != 2 or times.dim() != 1 or n_rot < 0 or keys.shape[1] < 3 * n_rot or keys.shape[1] == 0:
        raise ValueError(f"motion_resample takes keys (Tk, 3 n_rot + n_lin) and times (Tn,), got {tuple(keys.shape)}, {tuple(times.shape)}, n_rot = {n_rot}")
    Tk, W = keys.shape
    Tn, n_lin = times.shape[0], W - 3 * n_rot
    if Tk < 1 or Tn < 1:
        raise ValueError(f"at least one key and one time, got {Tk} and {Tn}")
    if rot_offset is not None and tuple(rot_offset.shape) != (3 * n_rot,):
        raise ValueError(f"rot_offset must be ({3 * n_rot},), got {tuple(rot_offset.shape)}")
    keys, times = keys.detach().contiguous(), times.detach().contiguous()
    off = None if rot_offset is None or n_rot == 0 else rot_offset.detach().contiguous()
    out = torch.empty(Tn, W, dtype=torch.float32, device=keys.device)
    with torch.cuda.device(keys.device):
        rc = _lib.lib().harp_motion_resample(_lib.ptr(keys), Tk, n_rot, n_lin, _lib.ptr(off), _lib.ptr(times), Tn, _lib.ptr(out), _lib.stream())
    _lib.check(rc, "harp_motion_resample")
    return out


FILTER_MAX_RADIUS = _lib.FILTER_MAX_RADIUS
FILTER_MAX_ITERS = 8


def gaussian_taps(sigma, radius=None):
    """The taps of a Gaussian window by distance, exp(-d^2 / (2 sigma^2)) for d = 0 .. radius, as a host list (motion_filter normalises by
    the weights it actually uses).  radius defaults to ceil(3 sigma) and is capped at FILTER_MAX_RADIUS (64)."""
    import math
    sigma = float(sigma)
    if not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"sigma must be positive and finite, got {sigma}")
    if radius is None:
        radius = min(int(math.ceil(3.0 * sigma)), FILTER_MAX_RADIUS)
    radius = int(radius)
    if not 0 <= radius <= FILTER_MAX_RADIUS:
        raise ValueError(f"radius in 0..{FILTER_MAX_RADIUS}, got {radius}")
    return [math.exp(-0.5 * (d / sigma) ** 2) for d in range(radius + 1)]


def _filter_taps(taps):
    """a host sequence of R + 1 finite, non-negative taps with taps[0] > 0 -> list of floats"""
    import math
    if torch.is_tensor(taps) or isinstance(taps, (str, bytes)):
        raise TypeError("motion_filter takes its taps as a host sequence of numbers (gaussian_taps), not a tensor")
    taps = [float(v) for v in taps]
    if not 1 <= len(taps) <= FILTER_MAX_RADIUS + 1:
        raise ValueError(f"1..{FILTER_MAX_RADIUS + 1} taps (radius 0..{FILTER_MAX_RADIUS}), got {len(taps)}")
    if not all(math.isfinite(v) and v >= 0 for v in taps) or not taps[0] > 0:
        raise ValueError("taps must be finite and non-negative, and taps[0] positive")
    return taps


def motion_filter(rows, n_rot, n_vec, taps, weights=None, segment=None, trim=None, rot_offset=None, iters=2):
    """A confidence-weighted, rotation-aware window filter over the rows of a motion (csrc/filter.hip: harp_motion_filter, whose contract
    include/harp_hip.h states), forward only: rows (T, 3 n_rot + 3 n_vec + n_lin) float32 = n_rot axis-angle triples, n_vec 3-vectors, then
    n_lin scalars -> (out of the same shape, used (T, nch) int32: the samples in each channel's final mean, -1 for antipodal rotations).
    taps: R + 1 window taps by distance, a HOST sequence (gaussian_taps); the window shrinks symmetrically at the ends of the clip and
    where `segment` (T,) int32 changes.  weights: None, (T,) or (T, nch) float32 confidences (<= 0 or not finite: the sample is not used).
    trim: None or (nch,) float32, > 0 switches on the trimmed second pass of that channel (radians for a rotation).  Rotations are averaged
    on the manifold after rot_offset (3 n_rot,) — the model's pose mean — has been added, with `iters` (0..8) geodesic-mean iterations."""
    _playback_input("motion_filter", rows, weights, segment, trim, rot_offset)
    n_rot, n_vec, iters = int(n_rot), int(n_vec), int(iters)
    taps = _filter_taps(taps)
    if rows.dtype != torch.float32 or any(t is not None and t.dtype != torch.float32 for t in (weights, trim, rot_offset)):
        raise TypeError("motion_filter takes float32 tensors")
    if segment is not None and segment.dtype != torch.int32:
        raise TypeError(f"segment must be int32, got {segment.dtype}")
    if rows.dim() != 2 or n_rot < 0 or n_vec < 0 or rows.shape[1] < 3 * (n_rot + n_vec) or rows.shape[1] == 0 or rows.shape[0] < 1:
        raise ValueError(f"motion_filter takes rows (T, 3 n_rot + 3 n_vec + n_lin), got {tuple(rows.shape)} with n_rot = {n_rot}, n_vec = {n_vec}")
    if not 0 <= iters <= FILTER_MAX_ITERS:
        raise ValueError(f"iters in 0..{FILTER_MAX_ITERS}, got {iters}")
    T, W = rows.shape
    n_lin = W - 3 * (n_rot + n_vec)
    nch = n_rot + n_vec + n_lin
    if weights is not None and tuple(weights.shape) not in ((T,), (T, nch)):
        raise ValueError(f"weights must be ({T},) or ({T}, {nch}), got {tuple(weights.shape)}")
    if segment is not None and tuple(segment.shape) != (T,):
        raise ValueError(f"segment must be ({T},), got {tuple(segment.shape)}")
    if trim is not None and tuple(trim.shape) != (nch,):
        raise ValueError(f"trim must be ({nch},), got {tuple(trim.shape)}")
    if rot_offset is not None and tuple(rot_offset.shape) != (3 * n_rot,):
        raise ValueError(f"rot_offset must be ({3 * n_rot},), got {tuple(rot_offset.shape)}")
    c = lambda t: None if t is None else t.detach().contiguous()      # noqa: E731
    rows, weights, segment, trim = c(rows), c(weights), c(segment), c(trim)
    off = None if n_rot == 0 else c(rot_offset)
    w_cols = 0 if weights is None else (1 if weights.dim() == 1 else nch)
    taps_dev = torch.tensor(taps, dtype=torch.float32).to(rows.device)
    out = torch.empty(T, W, dtype=torch.float32, device=rows.device)
    used = torch.empty(T, nch, dtype=torch.int32, device=rows.device)
    with torch.cuda.device(rows.device):
        rc = _lib.lib().harp_motion_filter(_lib.ptr(rows), T, n_rot, n_vec, n_lin, _lib.ptr(off), _lib.ptr(taps_dev), len(taps) - 1,
                                           _lib.ptr(weights), w_cols, _lib.ptr(segment), _lib.ptr(trim), iters, _lib.ptr(out), _lib.ptr(used),
                                           _lib.stream())
    _lib.check(rc, "harp_motion_filter")
    return out, used


def resolve_u8(rgb, face_id, ss=1, background=None, bg_rows=None, bg_color=(1, 1, 1), alpha=False, out=None):
    """A supersampled render over a background as finished 8-bit frames (csrc/playback.hip: harp_resolve_u8), forward only: rgb
    (B, S ss, S ss, 3) float32 and face_id (B, S ss, S ss) int32 (>= 0: covered) -> (B,S,S,3) uint8, or (B,S,S,4) with alpha=True (alpha =
    the covered share of the pixel).  background: None or (n_bg,S,S,3) uint8; bg_rows: None (n_bg must be 1 or B) or (B,) int32 rows of it,
    a row outside [0, n_bg) taking bg_color; bg_color: three numbers in [0,1] or a (3,) float32 device tensor.  out: a contiguous uint8
    tensor of the result's shape to write into."""
    _playback_input("resolve_u8", rgb, face_id, background, bg_rows, bg_color if torch.is_tensor(bg_color) else None, out)
    ss = int(ss)
    if not 1 <= ss <= RESOLVE_MAX_SS:
        raise ValueError(f"ss in 1..{RESOLVE_MAX_SS}, got {ss}")
    if rgb.dtype != torch.float32 or rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.shape[1] != rgb.shape[2] or rgb.shape[1] % ss or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise TypeError(f"resolve_u8 takes a float32 (B, S ss, S ss, 3) render, got {rgb.dtype} {tuple(rgb.shape)} with ss = {ss}")
    B, S = rgb.shape[0], rgb.shape[1] // ss
    if face_id.dtype != torch.int32 or tuple(face_id.shape) != tuple(rgb.shape[:3]):
        raise TypeError(f"face_id must be int32 {tuple(rgb.shape[:3])}, got {face_id.dtype} {tuple(face_id.shape)}")
    background, n_bg, bg_rows, color = _background_input(background, bg_rows, bg_color, B, S, rgb.device)
    C = 4 if alpha else 3
    out = _frames_out(out, B, S, C, rgb.device)
    with torch.cuda.device(rgb.device):
        rc = _lib.lib().harp_resolve_u8(_lib.ptr(rgb.detach().contiguous()), _lib.ptr(face_id.contiguous()), B, S, ss, _lib.ptr(background), n_bg,
                                        _lib.ptr(bg_rows), _lib.ptr(color), C, _lib.ptr(out), _lib.stream())
    _lib.check(rc, "harp_resolve_u8")
    return out


COMPOSITE_MAX_LAYERS = 4


def composite_layers_u8(layers, ss=1, scene_depth=None, scene_rows=None, background=None, bg_rows=None, bg_color=(1, 1, 1), alpha=False,
                        owner=False, out=None):
    """Several supersampled renders with their view depth as ONE finished 8-bit frame with depth-correct occlusion (csrc/composite.hip:
    harp_composite_layers_u8, whose contract include/harp_hip.h states), forward only.  layers: 1..4 of (rgb (B, S ss, S ss, 3) float32,
    zbuf (B, S ss, S ss) float32 view depth with > 0 = covered, flip) — a flipped layer is read mirrored in x.  Per sub-sample the nearest
    layer in front of scene_depth wins, ties going to the lower index.  scene_depth: None or (n_scene,S,S) float32 at output resolution
    (a value > 0 is a measurement); scene_rows: None (n_scene must be 1 or B) or (B,) int32 rows of it, a row outside [0, n_scene) meaning
    no scene depth.  background, bg_rows, bg_color, alpha, out: as resolve_u8.  Returns the (B,S,S,3|4) uint8 frames, or with owner=True
    (frames, owner (B,S,S) uint8: 0 = background, 1 + the layer that won most of the pixel's sub-samples)."""
    layers = [tuple(l) for l in layers]
    if not 1 <= len(layers) <= COMPOSITE_MAX_LAYERS or any(len(l) != 3 for l in layers):
        raise ValueError(f"composite_layers_u8 takes 1..{COMPOSITE_MAX_LAYERS} layers of (rgb, zbuf, flip), got {len(layers)}")
    _playback_input("composite_layers_u8", *[t for l in layers for t in l[:2]], scene_depth, scene_rows, background, bg_rows,
                    bg_color if torch.is_tensor(bg_color) else None, out)
    ss = int(ss)
    if not 1 <= ss <= RESOLVE_MAX_SS:
        raise ValueError(f"ss in 1..{RESOLVE_MAX_SS}, got {ss}")
    rgb = layers[0][0]
    if rgb.dtype != torch.float32 or rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.shape[1] != rgb.shape[2] or rgb.shape[1] % ss or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise TypeError(f"composite_layers_u8 takes float32 (B, S ss, S ss, 3) renders, got {rgb.dtype} {tuple(rgb.shape)} with ss = {ss}")
    B, S = rgb.shape[0], rgb.shape[1] // ss
    for i, (c, z, _) in enumerate(layers):
        if c.dtype != torch.float32 or z.dtype != torch.float32:
            raise TypeError(f"layer {i}: rgb and zbuf must be float32, got {c.dtype} and {z.dtype}")
        if tuple(c.shape) != tuple(rgb.shape) or tuple(z.shape) != tuple(rgb.shape[:3]):
            raise ValueError(f"layer {i}: rgb {tuple(c.shape)} and zbuf {tuple(z.shape)} must be {tuple(rgb.shape)} and {tuple(rgb.shape[:3])}")
    scene_depth, scene_rows, n_scene = _scene_depth_input("composite_layers_u8", scene_depth, scene_rows, B, S)
    background, n_bg, bg_rows, color = _background_input(background, bg_rows, bg_color, B, S, rgb.device)
    C = 4 if alpha else 3
    out = _frames_out(out, B, S, C, rgb.device)
    own = torch.empty(B, S, S, dtype=torch.uint8, device=rgb.device) if owner else None
    keep = [(c.detach().contiguous(), z.detach().contiguous()) for c, z, _ in layers]      # (alive until the launch is enqueued)
    arr = (_lib.Layer * len(layers))(*[_lib.Layer(_lib.ptr(c), _lib.ptr(z), int(bool(l[2])), 0) for (c, z), l in zip(keep, layers)])
    with torch.cuda.device(rgb.device):
        rc = _lib.lib().harp_composite_layers_u8(arr, len(layers), B, S, ss, _lib.ptr(scene_depth), n_scene, _lib.ptr(scene_rows),
                                                 _lib.ptr(background), n_bg, _lib.ptr(bg_rows), _lib.ptr(color), C, _lib.ptr(out), _lib.ptr(own),
                                                 _lib.stream())
    _lib.check(rc, "harp_composite_layers_u8")
    return (out, own) if owner else out


# ---- what the frames show (csrc/annotate.hip) ------------------------------------------------------------------------
LayerLabels = collections.namedtuple("LayerLabels", "owner part depth face uv bbox")
KeypointVisibility = collections.namedtuple("KeypointVisibility", "uvz vis")
LABEL_OCCLUDER_SCENE = 255                             # vis[..., 1] of a joint hidden by the scene depth
_LABEL_LAYER_KEYS = ("face_id", "zbuf", "face_label", "flip", "ndc", "faces", "verts_uvs", "faces_uvs")


def _label_layers(name, layers, ss, with_uv, depth_only=False):
    """layers: 1..4 dicts (face_id, zbuf, face_label, flip [, ndc, faces, verts_uvs, faces_uvs]) checked -> (the C array, the tensors
    it points at, B, S)"""
    layers = list(layers)
    if not 1 <= len(layers) <= COMPOSITE_MAX_LAYERS or any(not isinstance(l, dict) or set(l) - set(_LABEL_LAYER_KEYS) for l in layers):
        raise ValueError(f"{name} takes 1..{COMPOSITE_MAX_LAYERS} layers, dicts with keys of {_LABEL_LAYER_KEYS}, got {len(layers)}")
    _playback_input(name, *[l.get(k) for l in layers for k in _LABEL_LAYER_KEYS if k != "flip"])
    if not 1 <= ss <= RESOLVE_MAX_SS:
        raise ValueError(f"ss in 1..{RESOLVE_MAX_SS}, got {ss}")
    z0 = layers[0].get("zbuf")
    if z0 is None or z0.dtype != torch.float32 or z0.dim() != 3 or z0.shape[1] != z0.shape[2] or z0.shape[1] % ss or z0.shape[0] < 1 or z0.shape[1] < 1:
        raise TypeError(f"{name} takes float32 (B, S ss, S ss) depths, got {None if z0 is None else (z0.dtype, tuple(z0.shape))} with ss = {ss}")
    B, S = z0.shape[0], z0.shape[1] // ss
    keep, arr = [], (_lib.LabelLayer * len(layers))()
    c = lambda t: t.detach().contiguous()               # noqa: E731
    for i, l in enumerate(layers):
        z = l.get("zbuf")
        if z is None or z.dtype != torch.float32:
            raise TypeError(f"layer {i}: zbuf must be float32, got {None if z is None else z.dtype}")
        if tuple(z.shape) != tuple(z0.shape):
            raise ValueError(f"layer {i}: zbuf {tuple(z.shape)} must be {tuple(z0.shape)}")
        a = arr[i]
        ts = [c(z)]
        a.zbuf, a.flip_x, a.reserved = _lib.ptr(ts[0]), int(bool(l.get("flip", False))), 0
        if not depth_only:
            fid, lab = l.get("face_id"), l.get("face_label")
            if fid is None or fid.dtype != torch.int32 or lab is None or lab.dtype != torch.uint8:
                raise TypeError(f"layer {i}: face_id must be int32 and face_label uint8")
            if tuple(fid.shape) != tuple(z0.shape) or lab.dim() != 1 or lab.shape[0] < 1:
                raise ValueError(f"layer {i}: face_id {tuple(fid.shape)} must be {tuple(z0.shape)} and face_label (F,), got {tuple(lab.shape)}")
            ts += [c(fid), c(lab)]
            a.face_id, a.face_label, a.F = _lib.ptr(ts[1]), _lib.ptr(ts[2]), lab.shape[0]
            if with_uv:
                ndc, faces, vuv, fuv = (l.get(k) for k in ("ndc", "faces", "verts_uvs", "faces_uvs"))
                if any(t is None for t in (ndc, faces, vuv, fuv)):
                    raise ValueError(f"layer {i}: the uv output needs ndc, faces, verts_uvs and faces_uvs")
                if ndc.dtype != torch.float32 or vuv.dtype != torch.float32 or faces.dtype != torch.int32 or fuv.dtype != torch.int32:
                    raise TypeError(f"layer {i}: ndc and verts_uvs must be float32, faces and faces_uvs int32")
                F = lab.shape[0]
                if (ndc.dim() != 3 or ndc.shape[0] != B or ndc.shape[1] < 1 or ndc.shape[2] != 3 or tuple(faces.shape) != (F, 3)
                        or tuple(fuv.shape) != (F, 3) or vuv.dim() != 2 or vuv.shape[0] < 1 or vuv.shape[1] != 2):
                    raise ValueError(f"layer {i}: ndc ({B}, V, 3), faces ({F}, 3), verts_uvs (Vt, 2), faces_uvs ({F}, 3), got {tuple(ndc.shape)}, "
                                     f"{tuple(faces.shape)}, {tuple(vuv.shape)}, {tuple(fuv.shape)}")
                ts += [c(ndc), c(faces), c(vuv), c(fuv)]
                a.ndc, a.faces, a.verts_uvs, a.faces_uvs = (_lib.ptr(t) for t in ts[3:])
                a.V, a.Vt = ndc.shape[1], vuv.shape[0]
        keep.append(ts)
    return arr, keep, B, S


def annotate_layers(layers, ss=1, scene_depth=None, scene_rows=None, owner=True, part=True, depth=True, face=True, uv=False, bbox=True):
    """What the frame of composite_layers_u8 on the same layers SHOWS (csrc/annotate.hip: harp_annotate_layers, whose contract
    include/harp_hip.h states), forward only.  layers: 1..4 dicts of face_id (B, S ss, S ss) int32 and zbuf (B, S ss, S ss) float32 as the
    camera-view rasteriser leaves them, face_label (F,) uint8 (playback.labels.face_part_labels), flip, and for uv=True ndc (B,V,3)
    float32, faces (F,3) int32, verts_uvs (Vt,2) float32, faces_uvs (F,3) int32.  scene_depth, scene_rows: as composite_layers_u8.
    Returns LayerLabels(owner (B,S,S) uint8 — bit for bit the composite's —, part (B,S,S) uint8, depth (B,S,S) float32 view depth, face
    (B,S,S) int32, uv (B,S,S,2) float32, bbox (B, len(layers), 4) int32 as (xmin, ymin, xmax, ymax), -1 for a layer that owns no pixel),
    None for an output that was not asked for."""
    ss, want_uv = int(ss), bool(uv)
    arr, keep, B, S = _label_layers("annotate_layers", layers, ss, want_uv)
    _playback_input("annotate_layers", keep[0][0], scene_depth, scene_rows)
    scene_depth, scene_rows, n_scene = _scene_depth_input("annotate_layers", scene_depth, scene_rows, B, S)
    if not any((owner, part, depth, face, uv, bbox)):
        raise ValueError("annotate_layers: no output asked for")
    dev = keep[0][0].device
    new = lambda on, shape, dt: torch.empty(*shape, dtype=dt, device=dev) if on else None      # noqa: E731
    o = LayerLabels(new(owner, (B, S, S), torch.uint8), new(part, (B, S, S), torch.uint8), new(depth, (B, S, S), torch.float32),
                    new(face, (B, S, S), torch.int32), new(uv, (B, S, S, 2), torch.float32),
                    torch.zeros(B, len(keep), 4, dtype=torch.int32, device=dev) if bbox else None)
    with torch.cuda.device(dev):
        rc = _lib.lib().harp_annotate_layers(arr, len(keep), B, S, ss, _lib.ptr(scene_depth), n_scene, _lib.ptr(scene_rows), *[_lib.ptr(t) for t in o],
                                             _lib.stream())
    _lib.check(rc, "harp_annotate_layers")
    return o._replace(bbox=bbox_from_extents(o.bbox, S)) if bbox else o


def bbox_from_extents(ext, S):
    """harp_annotate_layers' accumulated (S - xmin, S - ymin, xmax + 1, ymax + 1), all zeros for nothing -> (xmin, ymin, xmax, ymax), -1
    for nothing (device arithmetic, no synchronisation)"""
    box = torch.stack([S - ext[..., 0], S - ext[..., 1], ext[..., 2] - 1, ext[..., 3] - 1], -1)
    return torch.where((ext[..., 2:3] > 0).expand_as(box), box, torch.full_like(box, -1))


def keypoint_visibility(joints, cam_R, cam_T, focal, S, layers, self_layer=0, ss=1, scene_depth=None, scene_rows=None, tol=0.02):
    """The joints of layer `self_layer` in the image, and whether each is seen (csrc/annotate.hip: harp_keypoint_visibility, whose contract
    include/harp_hip.h states), forward only.  joints (B,NJ,3) float32 metres, cam_R (B,9), cam_T (B,3) float32 as the fused front leaves
    them; focal and S of the output image; layers: 1..4 dicts of zbuf (B, S ss, S ss) float32 and flip (other keys are ignored);
    scene_depth, scene_rows: as composite_layers_u8; tol metres: a joint lies under its own skin, so it counts as visible when the nearest
    surface is no nearer than Z - tol.  Returns KeypointVisibility(uvz (B,NJ,3) float32 = (u, v, view depth), vis (B,NJ,2) uint8 =
    (0 not in the image | 1 hidden | 2 visible, what hides it: 0 nothing, 1 + the layer, 255 the scene depth))."""
    import math
    ss, S, self_layer, focal, tol = int(ss), int(S), int(self_layer), float(focal), float(tol)
    _playback_input("keypoint_visibility", joints, cam_R, cam_T, scene_depth, scene_rows)
    arr, keep, B, S_l = _label_layers("keypoint_visibility", layers, ss, False, depth_only=True)
    _playback_input("keypoint_visibility", joints, keep[0][0])
    if any(t.dtype != torch.float32 for t in (joints, cam_R, cam_T)):
        raise TypeError("keypoint_visibility takes float32 joints, cam_R and cam_T")
    if joints.dim() != 3 or joints.shape[0] != B or joints.shape[1] < 1 or joints.shape[2] != 3 or tuple(cam_R.shape) != (B, 9) or tuple(cam_T.shape) != (B, 3):
        raise ValueError(f"keypoint_visibility takes joints ({B}, NJ, 3), cam_R ({B}, 9) and cam_T ({B}, 3), got {tuple(joints.shape)}, "
                         f"{tuple(cam_R.shape)}, {tuple(cam_T.shape)}")
    if S != S_l:
        raise ValueError(f"the layers are {S_l * ss} wide: S = {S_l} at ss = {ss}, got S = {S}")
    if not 0 <= self_layer < len(keep):
        raise ValueError(f"self_layer in 0..{len(keep) - 1}, got {self_layer}")
    if not (focal > 0 and math.isfinite(focal)) or not (tol >= 0 and math.isfinite(tol)):
        raise ValueError(f"focal must be positive and tol non-negative, both finite; got {focal}, {tol}")
    scene_depth, scene_rows, n_scene = _scene_depth_input("keypoint_visibility", scene_depth, scene_rows, B, S)
    NJ = joints.shape[1]
    j, R, T = joints.detach().contiguous(), cam_R.detach().contiguous(), cam_T.detach().contiguous()
    o = KeypointVisibility(torch.empty(B, NJ, 3, dtype=torch.float32, device=j.device), torch.empty(B, NJ, 2, dtype=torch.uint8, device=j.device))
    with torch.cuda.device(j.device):
        rc = _lib.lib().harp_keypoint_visibility(_lib.ptr(j), _lib.ptr(R), _lib.ptr(T), B, NJ, focal, S, ss, self_layer, arr, len(keep),
                                                 _lib.ptr(scene_depth), n_scene, _lib.ptr(scene_rows), tol, _lib.ptr(o.uvz), _lib.ptr(o.vis),
                                                 _lib.stream())
    _lib.check(rc, "harp_keypoint_visibility")
    return o


# ---- where the surface points of a frame are in another frame (csrc/flow.hip) ----------------------------------------
LayerFlow = collections.namedtuple("LayerFlow", "flow dz status")
# metres: a convention, not a tuned value.  The tracked point lies ON the surface (a joint lies under it: LABEL_TOL is 0.02), so the
# tolerance only absorbs the depth difference between the point where it lands and the centre of the sub-pixel it is tested at
FLOW_TOL = 0.005
FLOW_STATUS = ("none", "untrackable", "outside", "hidden", "visible")      # status[..., 0]
_FLOW_LAYER_KEYS = ("face_id", "zbuf", "face_label", "flip", "ndc", "faces")


def flow_layers(layers, to, ss=1, scene_depth=None, scene_rows=None, scene_depth_to=None, scene_rows_to=None, tol=FLOW_TOL):
    """Where the surface point that each output pixel of composite_layers_u8 on `layers` shows lies in the TARGET frames (csrc/flow.hip:
    harp_flow_layers, whose contract include/harp_hip.h states), forward only.  layers: annotate_layers' 1..4 dicts of the SOURCE frames
    with face_id, zbuf, face_label, flip, ndc (B,V,3) float32 and faces (F,3) int32 (verts_uvs and faces_uvs are ignored); to: per layer a
    dict of the same mesh in the target frames, ndc (B,V,3) float32 and zbuf (B, S ss, S ss) float32.  scene_depth, scene_rows: the scene
    depth of the source frames, scene_depth_to, scene_rows_to: of the target frames, each as composite_layers_u8.  tol metres: the point is
    visible when the nearest target surface where it lands is no nearer than its own depth minus tol (FLOW_TOL).  Returns LayerFlow(flow
    (B,S,S,2) float32 in output pixels, dz (B,S,S) float32 metres, status (B,S,S,2) uint8 = (0 no owner | 1 not trackable | 2 lands
    outside the image | 3 hidden | 4 visible, what hides it: 0 nothing, 1 + the layer, 255 the scene depth)); flow and dz are zero
    where status is 0 or 1."""
    import math
    ss, tol = int(ss), float(tol)
    layers, to = list(layers), list(to)
    src = [{k: v for k, v in l.items() if k not in ("verts_uvs", "faces_uvs")} if isinstance(l, dict) else l for l in layers]
    arr_l, keep, B, S = _label_layers("flow_layers", src, ss, False)
    if len(to) != len(src) or any(not isinstance(t, dict) or set(t) != {"ndc", "zbuf"} for t in to):
        raise ValueError(f"flow_layers takes one dict (ndc, zbuf) of the target frames per layer, got {len(to)} for {len(src)} layers")
    _playback_input("flow_layers", keep[0][0], *[l.get(k) for l in src for k in ("ndc", "faces")], *[t[k] for t in to for k in ("ndc", "zbuf")],
                    scene_depth, scene_rows, scene_depth_to, scene_rows_to)
    if not (tol >= 0 and math.isfinite(tol)):
        raise ValueError(f"tol must be non-negative and finite, got {tol}")
    z0 = keep[0][0]
    c = lambda t: t.detach().contiguous()               # noqa: E731
    arr = (_lib.FlowLayer * len(src))()
    for i, (l, t) in enumerate(zip(src, to)):
        ndc, faces, ndc_to, z_to = l.get("ndc"), l.get("faces"), t["ndc"], t["zbuf"]
        if ndc is None or faces is None:
            raise ValueError(f"layer {i}: the flow needs ndc and faces")
        if ndc.dtype != torch.float32 or ndc_to.dtype != torch.float32 or z_to.dtype != torch.float32 or faces.dtype != torch.int32:
            raise TypeError(f"layer {i}: ndc and the target's ndc and zbuf must be float32, faces int32")
        F = arr_l[i].F
        if (ndc.dim() != 3 or ndc.shape[0] != B or ndc.shape[1] < 1 or ndc.shape[2] != 3 or tuple(faces.shape) != (F, 3)
                or tuple(ndc_to.shape) != tuple(ndc.shape) or tuple(z_to.shape) != tuple(z0.shape)):
            raise ValueError(f"layer {i}: ndc ({B}, V, 3), faces ({F}, 3), the target's ndc as the source's and its zbuf {tuple(z0.shape)}, got "
                             f"{tuple(ndc.shape)}, {tuple(faces.shape)}, {tuple(ndc_to.shape)}, {tuple(z_to.shape)}")
        ts = [c(ndc), c(faces), c(ndc_to), c(z_to)]
        keep.append(ts)
        a = arr[i]
        a.face_id, a.zbuf, a.face_label, a.F, a.flip_x, a.reserved = arr_l[i].face_id, arr_l[i].zbuf, arr_l[i].face_label, F, arr_l[i].flip_x, 0
        a.ndc, a.faces, a.ndc_to, a.zbuf_to = (_lib.ptr(x) for x in ts)
        a.V = ndc.shape[1]
    scene_depth, scene_rows, n_scene = _scene_depth_input("flow_layers", scene_depth, scene_rows, B, S)
    scene_depth_to, scene_rows_to, n_scene_to = _scene_depth_input("flow_layers", scene_depth_to, scene_rows_to, B, S)
    dev = z0.device
    o = LayerFlow(torch.empty(B, S, S, 2, dtype=torch.float32, device=dev), torch.empty(B, S, S, dtype=torch.float32, device=dev),
                  torch.empty(B, S, S, 2, dtype=torch.uint8, device=dev))
    with torch.cuda.device(dev):
        rc = _lib.lib().harp_flow_layers(arr, len(src), B, S, ss, _lib.ptr(scene_depth), n_scene, _lib.ptr(scene_rows), _lib.ptr(scene_depth_to),
                                         n_scene_to, _lib.ptr(scene_rows_to), tol, *[_lib.ptr(t) for t in o], _lib.stream())
    _lib.check(rc, "harp_flow_layers")
    return o


# ---- contact labels: distance, nearest face and winding number between two meshes (csrc/contact.hip) ---------------------
# one side of mesh_contact: verts (B,V,3), cam_R (B,9), cam_T (B,3) float32 as the fused front leaves vd, cam_R and cam_T; faces (F,3)
# int32 (the target's; the query's is not read); flip: the mesh is shown mirrored in x
ContactMesh = collections.namedtuple("ContactMesh", "verts cam_R cam_T faces flip", defaults=(None, False))
MeshContact = collections.namedtuple("MeshContact", "dist face wind")
_CONTACT_OUTPUTS = ("dist", "face", "wind")
CONTACT_EXCL_FACES = 128                               # HARP_CONTACT_EXCL_FACES: the faces one 16-byte word of an exclusion table covers


def _contact_side(name, side, B, target):
    """one ContactMesh (or a dict of its fields) checked -> (the C struct, the tensors it points at)"""
    if isinstance(side, dict):
        if set(side) - set(ContactMesh._fields):
            raise ValueError(f"mesh_contact: {name} takes the keys {ContactMesh._fields}, got {sorted(side)}")
        side = ContactMesh(**side)
    if not isinstance(side, ContactMesh):
        raise TypeError(f"mesh_contact: {name} is an ops.ContactMesh or a dict of its fields")
    v, R, T, faces = side.verts, side.cam_R, side.cam_T, side.faces
    _playback_input("mesh_contact", v, R, T, faces)
    if any(t is None or t.dtype != torch.float32 for t in (v, R, T)):
        raise TypeError(f"mesh_contact: {name} takes float32 verts, cam_R and cam_T")
    if v.dim() != 3 or v.shape[0] < 1 or v.shape[1] < 1 or v.shape[2] != 3:
        raise ValueError(f"mesh_contact: {name}.verts is (B, V, 3), got {tuple(v.shape)}")
    B = v.shape[0] if B is None else B
    if v.shape[0] != B or tuple(R.shape) != (B, 9) or tuple(T.shape) != (B, 3):
        raise ValueError(f"mesh_contact: {name} takes verts ({B}, V, 3), cam_R ({B}, 9) and cam_T ({B}, 3), got {tuple(v.shape)}, "
                         f"{tuple(R.shape)}, {tuple(T.shape)}")
    keep = [v.detach().contiguous(), R.detach().contiguous(), T.detach().contiguous()]
    m = _lib.ContactMesh(verts=_lib.ptr(keep[0]), cam_R=_lib.ptr(keep[1]), cam_T=_lib.ptr(keep[2]), V=v.shape[1], F=0,
                         flip_x=int(bool(side.flip)), reserved=0)
    if target:
        if faces is None or faces.dtype != torch.int32:
            raise TypeError(f"mesh_contact: {name}.faces must be int32, got {None if faces is None else faces.dtype}")
        if faces.dim() != 2 or faces.shape[0] < 1 or faces.shape[1] != 3:
            raise ValueError(f"mesh_contact: {name}.faces is (F, 3), got {tuple(faces.shape)}")
        keep.append(faces.detach().contiguous())
        m.faces, m.F = _lib.ptr(keep[3]), faces.shape[0]
    return m, keep


def mesh_contact(query, target, max_dist=math.inf, want=_CONTACT_OUTPUTS, exclude=None):
    """For every vertex of `query` its relation to the surface of `target`, frame by frame (csrc/contact.hip: harp_mesh_contact, whose
    contract include/harp_hip.h states), forward only: a label, no gradient.  query, target: ops.ContactMesh (or dicts of its fields) of
    device tensors over the same B frames; the target needs faces.  max_dist metres, >= 0, inf for no limit.  want: which of "dist",
    "face", "wind" to compute.  Returns MeshContact(dist (B,Vq) float32: the unsigned distance to the target's nearest triangle, +inf
    beyond max_dist; face (B,Vq) int32: a face that attains it, -1 for none; wind (B,Vq) float32: the generalised winding number of the
    target about the vertex (about 1 inside, 0 outside; > 0.5 is the playback's "inside"), 0 where dist is +inf), None for an output that
    was not asked for.  exclude: None, or the faces that do not count for a vertex's distance minimum (harp_mesh_contact_excl, DESIGN.md
    §37): an int32 or uint32 contiguous device tensor (ceil(F / 128), Vq, 4), bit k & 31 of exclude[c, i, k >> 5] for face 128 c + k and
    query vertex i, the same for every frame (playback.selfcontact.pack_exclusion makes it from a (Vq, F) bool); wind is not masked."""
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or set(want) - set(_CONTACT_OUTPUTS):
        raise ValueError(f"mesh_contact: want is a non-empty selection of {_CONTACT_OUTPUTS}, got {want}")
    max_dist = float(max_dist)
    if not max_dist >= 0:
        raise ValueError(f"mesh_contact: max_dist must not be negative or NaN, got {max_dist}")
    q, keep_q = _contact_side("query", query, None, False)
    B = keep_q[0].shape[0]
    t, keep_t = _contact_side("target", target, B, True)
    _playback_input("mesh_contact", keep_q[0], keep_t[0])
    dev, Vq = keep_q[0].device, keep_q[0].shape[1]
    if exclude is not None:
        shape = (-(-t.F // CONTACT_EXCL_FACES), Vq, 4)
        if not torch.is_tensor(exclude) or exclude.dtype not in (torch.int32, torch.uint32):
            raise TypeError(f"mesh_contact: exclude must be an int32 or uint32 tensor, got {exclude.dtype if torch.is_tensor(exclude) else type(exclude)}")
        if exclude.device != dev:
            raise ValueError(f"mesh_contact: exclude is on {exclude.device}, the meshes on {dev}")
        if tuple(exclude.shape) != shape:
            raise ValueError(f"mesh_contact: exclude must be {shape} = (chunks of {CONTACT_EXCL_FACES} faces, Vq, 4), got {tuple(exclude.shape)}")
        if not exclude.is_contiguous():
            raise ValueError("mesh_contact: exclude must be contiguous")
    L = _lib.lib()
    ws = torch.empty(L.harp_mesh_contact_ws_floats(B, t.F), dtype=torch.float32, device=dev)
    new = lambda k, dt: torch.empty(B, Vq, dtype=dt, device=dev) if k in want else None      # noqa: E731
    o = MeshContact(new("dist", torch.float32), new("face", torch.int32), new("wind", torch.float32))
    with torch.cuda.device(dev):
        if exclude is None:
            rc = L.harp_mesh_contact(ctypes.byref(q), ctypes.byref(t), B, max_dist, _lib.ptr(ws), *[_lib.ptr(x) for x in o], _lib.stream())
        else:
            rc = L.harp_mesh_contact_excl(ctypes.byref(q), ctypes.byref(t), _lib.ptr(exclude), B, max_dist, _lib.ptr(ws),
                                          *[_lib.ptr(x) for x in o], _lib.stream())
    _lib.check(rc, "harp_mesh_contact" if exclude is None else "harp_mesh_contact_excl")
    return o


# ---- the front that the six batched Levenberg-Marquardt solvers below share ---------------------------------------------
# A wrapper runs, in this order: _playback_input (device tensors, forward only), _lm_float32, its own check of `targets`, _lm_shapes,
# _lm_scalars, its own checks, _lm_model_device, _lm_result, _lm_start, _lm_input, then its options struct and its one call.
def _lm_float32(fn, **named):
    """every tensor of `named` that is not None is float32, else a TypeError that names the field"""
    for name, t in named.items():
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"{fn} takes float32 tensors, {name} is {t.dtype}")


def _lm_shapes(*named):
    """named: (name, tensor or None, shape) or, for a field with a choice such as betas and cam, (name, tensor, [shape, ...]); a tensor of
    another shape raises a ValueError that names the field and both shapes"""
    for name, t, want in named:
        if t is not None and tuple(t.shape) != want and not (isinstance(want, list) and tuple(t.shape) in want):
            want = " or ".join(map(str, want)) if isinstance(want, list) else want
            raise ValueError(f"{name} must be {want}, got {tuple(t.shape)}")


def _lm_scalars(iters, **weights):
    """iters >= 0 and every weight (already a float) finite and >= 0, else a ValueError that lists the names and the values"""
    if iters < 0 or any(not (0.0 <= v < float("inf")) for v in weights.values()):
        raise ValueError(f"iters >= 0 and finite {', '.join(weights)} >= 0, got {iters}, {', '.join(map(str, weights.values()))}")


def _lm_model_device(dm, targets):
    if dm.v_template.device != targets.device:
        raise ValueError(f"the model is on {dm.v_template.device}, the targets on {targets.device}")


def _lm_result(kind, want, out, dev):
    """The result namedtuple `kind` on `dev`.  want: one shape per field, None for an output that was not asked for; status is the one
    int32 field, the rest are float32.  out=None: new tensors.  Else `out` itself, once every field fits: None exactly where want is, and
    otherwise of that shape, on dev, contiguous and of the field's dtype — nothing is allocated then."""
    if out is None:
        return kind(*[None if shape is None else torch.empty(shape, dtype=torch.int32 if name == "status" else torch.float32, device=dev)
                      for name, shape in zip(kind._fields, want)])
    for name, t, shape in zip(kind._fields, out, want):
        if (t is None) != (shape is None) or (t is not None and (tuple(t.shape) != shape or t.device != dev or not t.is_contiguous()
                                                                  or t.dtype != (torch.int32 if name == "status" else torch.float32))):
            raise ValueError(f"out.{name} does not fit this call")
    return out


def _lm_start(out, **start):
    """the start rows into the result's fields of the same names: the kernel iterates in place, the caller's tensors stay untouched"""
    for name, t in start.items():
        getattr(out, name).copy_(t.detach())


def _lm_input(t):
    """an input as the kernel reads it, which is by its pointer alone: contiguous — the tensor itself when it already is, without a new
    tensor object — else a detached contiguous copy; None as None"""
    return t if t is None or t.is_contiguous() else t.detach().contiguous()


# ---- batched MANO inverse kinematics (csrc/ik.hip) -----------------------------------------------------------------
IkResult = collections.namedtuple("IkResult", "pose48 trans cost status joints jac")


def mano_ik_frames_per_block():
    """the frames one workgroup of harp_mano_ik solves"""
    return int(_lib.lib().harp_mano_ik_frames_per_block())


def mano_ik(dm, betas, targets, pose48, trans, weights=None, prior=None, iters=15, lambda0=1e-3, prior_weight=0.0, joints=False, jac=False,
            out=None):
    """3-D keypoints -> MANO pose rows: T Levenberg-Marquardt solves in one launch (csrc/ik.hip: harp_mano_ik, whose contract
    include/harp_hip.h states), forward only.  dm: a ManoDeviceModel; betas (10,) for all frames or (T,10); targets (T,21,3) metres in the
    order of the model's joints; pose48 (T,48) = [rot | pose] and trans (T,3): the start, left untouched; weights (T,21) or None (ones; a
    joint with weight <= 0 or a non-finite target is unused); prior (T,45) or None (the mean pose) with prior_weight on
    sum (pose - prior)^2.  Returns IkResult(pose48, trans, cost (T,2) = at the start and at the result, status (T,) int32 = accepted steps
    or -1 for a frame with fewer than 3 used joints (returned as it came), joints (T,21,3) mm or None, jac (T,63,51) or None).
    iters = 0 evaluates at the start.  out: an earlier IkResult of the same shapes whose tensors are written instead of new ones — the
    call then allocates nothing and can be captured into a graph."""
    _playback_input("mano_ik", betas, targets, pose48, trans, weights, prior)
    _lm_float32("mano_ik", betas=betas, targets=targets, pose48=pose48, trans=trans, weights=weights, prior=prior)
    if targets.dim() != 3 or tuple(targets.shape[1:]) != (21, 3) or targets.shape[0] < 1:
        raise ValueError(f"targets must be (T, 21, 3), got {tuple(targets.shape)}")
    T = targets.shape[0]
    _lm_shapes(("betas", betas, [(10,), (T, 10)]), ("pose48", pose48, (T, 48)), ("trans", trans, (T, 3)), ("weights", weights, (T, 21)),
               ("prior", prior, (T, 45)))
    iters, lambda0, prior_weight = int(iters), float(lambda0), float(prior_weight)
    _lm_scalars(iters, lambda0=lambda0, prior_weight=prior_weight)
    _lm_model_device(dm, targets)
    out = _lm_result(IkResult, ((T, 48), (T, 3), (T, 2), (T,), (T, 21, 3) if joints else None, (T, 63, 51) if jac else None), out, targets.device)
    _lm_start(out, pose48=pose48, trans=trans)
    betas, targets, weights, prior = map(_lm_input, (betas, targets, weights, prior))
    opt = _lib.IkOptions(iters, lambda0, prior_weight, int(betas.dim() == 2))
    with torch.cuda.device(targets.device):
        rc = _lib.lib().harp_mano_ik(ctypes.byref(dm.struct), _lib.ptr(betas), _lib.ptr(targets), _lib.ptr(weights), _lib.ptr(prior), T,
                                     ctypes.byref(opt), _lib.ptr(out.pose48), _lib.ptr(out.trans), _lib.ptr(out.cost), _lib.ptr(out.status),
                                     _lib.ptr(out.joints), _lib.ptr(out.jac), _lib.stream())
    _lib.check(rc, "harp_mano_ik")
    return out


# ---- batched MANO vertex fit (csrc/vertex_fit.hip) ------------------------------------------------------------------
VertexFitResult = collections.namedtuple("VertexFitResult", "pose48 betas trans cost status verts jac A g")


def mano_vertex_fit_frames_per_block():
    """the frames one workgroup of harp_mano_vertex_fit solves"""
    return int(_lib.lib().harp_mano_vertex_fit_frames_per_block())


def mano_vertex_fit(dm, targets, pose48, betas, trans, weights=None, prior=None, solve_shape=True, iters=10, lambda0=1e-3, pose_prior_weight=0.0,
                    shape_prior_weight=0.0, verts=False, jac=False, normal=False, out=None):
    """Mesh vertices -> MANO rows: T Levenberg-Marquardt solves in one launch (csrc/vertex_fit.hip: harp_mano_vertex_fit, whose contract
    include/harp_hip.h states), forward only.  dm: a ManoDeviceModel; targets (T,778,3) metres; pose48 (T,48) = [rot | pose], betas and
    trans (T,3): the start, left untouched; betas (T,10) with solve_shape=True, (10,) for all frames or (T,10) with solve_shape=False (an
    avatar's shape: given, not solved, returned as it came); weights (T,778) or None (ones; a vertex with weight <= 0 or a non-finite
    target is unused); prior (T,45) or None (the mean pose) with pose_prior_weight on sum (pose - prior)^2; shape_prior_weight on
    sum betas^2.  Returns VertexFitResult(pose48, betas, trans, cost (T,2) = at the start and at the result, status (T,) int32 = accepted
    steps or -1 for a frame with fewer than 21 used vertices (returned as it came), verts (T,778,3) mm or None, jac (T,2334,61) or None,
    A (T,61,61) and g (T,61) with normal=True, else None), the optional ones at the result.  iters = 0 evaluates at the start.  out: an
    earlier VertexFitResult of the same shapes whose tensors are written instead of new ones — the call then allocates nothing and can be
    captured into a graph."""
    _playback_input("mano_vertex_fit", targets, pose48, betas, trans, weights, prior)
    _lm_float32("mano_vertex_fit", targets=targets, pose48=pose48, betas=betas, trans=trans, weights=weights, prior=prior)
    if targets.dim() != 3 or tuple(targets.shape[1:]) != (778, 3) or targets.shape[0] < 1:
        raise ValueError(f"targets must be (T, 778, 3), got {tuple(targets.shape)}")
    T = targets.shape[0]
    solve_shape = bool(solve_shape)
    _lm_shapes(("betas", betas, [(T, 10)] if solve_shape else [(T, 10), (10,)]), ("pose48", pose48, (T, 48)), ("trans", trans, (T, 3)),
               ("weights", weights, (T, 778)), ("prior", prior, (T, 45)))
    iters, lambda0, pose_prior_weight, shape_prior_weight = int(iters), float(lambda0), float(pose_prior_weight), float(shape_prior_weight)
    _lm_scalars(iters, lambda0=lambda0, pose_prior_weight=pose_prior_weight, shape_prior_weight=shape_prior_weight)
    _lm_model_device(dm, targets)
    want = ((T, 48), tuple(betas.shape), (T, 3), (T, 2), (T,), (T, 778, 3) if verts else None, (T, 2334, 61) if jac else None,
            (T, 61, 61) if normal else None, (T, 61) if normal else None)
    out = _lm_result(VertexFitResult, want, out, targets.device)
    _lm_start(out, pose48=pose48, betas=betas, trans=trans)
    targets, weights, prior = map(_lm_input, (targets, weights, prior))
    opt = _lib.VertexFitOptions(iters, lambda0, pose_prior_weight, shape_prior_weight, int(solve_shape), int(betas.dim() == 2))
    with torch.cuda.device(targets.device):
        rc = _lib.lib().harp_mano_vertex_fit(ctypes.byref(dm.struct), _lib.ptr(targets), _lib.ptr(weights), _lib.ptr(prior), T, ctypes.byref(opt),
                                             _lib.ptr(out.pose48), _lib.ptr(out.betas), _lib.ptr(out.trans), _lib.ptr(out.cost),
                                             _lib.ptr(out.status), _lib.ptr(out.verts), _lib.ptr(out.jac), _lib.ptr(out.A), _lib.ptr(out.g),
                                             _lib.stream())
    _lib.check(rc, "harp_mano_vertex_fit")
    return out


# ---- batched SMPL-X arm vertex fit (csrc/arm_vertex_fit.hip) --------------------------------------------------------
ArmVertexFitResult = collections.namedtuple("ArmVertexFitResult", "in_pose betas trans cost status verts jac A g")


def arm_vertex_fit_frames_per_block():
    """the frames one workgroup of harp_arm_vertex_fit solves"""
    return int(_lib.lib().harp_arm_vertex_fit_frames_per_block())


def arm_vertex_fit(dm, targets, in_pose, betas, trans, vert_idx=None, weights=None, prior=None, solve_shape=True, solve_wrist=True, iters=10,
                   lambda0=1e-3, pose_prior_weight=0.0, wrist_prior_weight=0.0, shape_prior_weight=0.0, verts=False, jac=False, normal=False,
                   out=None):
    """Mesh vertices -> SMPL-X arm rows: T Levenberg-Marquardt solves in one launch (csrc/arm_vertex_fit.hip: harp_arm_vertex_fit, whose
    contract include/harp_hip.h states), forward only.  dm: a TreeDeviceModel (hand_models_harp.body_models); targets (T,n_t,3) metres, row
    i belonging to model vertex vert_idx[i] ((n_t,) int32 or int64 on the device, every entry in [0, NV) — checked here; None: n_t = NV,
    the identity); in_pose (T,17,3) = [rot | wrist | pose(15)], betas and trans (T,3): the start, left untouched; betas (T,10) with
    solve_shape=True, (10,) for all frames or (T,10) with solve_shape=False (an avatar's shape: given, not solved, returned as it came);
    solve_wrist=False holds the wrist row at what in_pose gives; weights (T,n_t) or None (ones; a target with weight <= 0 or a non-finite
    coordinate is unused); prior (T,45) or None (the mean pose) with pose_prior_weight on sum (pose - prior)^2; wrist_prior_weight on
    sum wrist^2; shape_prior_weight on sum betas^2.  Returns ArmVertexFitResult(in_pose, betas, trans, cost (T,2) = at the start and at the
    result, status (T,) int32 = accepted steps or -1 for a frame with fewer than 22 used targets (returned as it came), verts (T,NV,3) mm
    (all model vertices) or None, jac (T,3 n_t,64) or None, A (T,64,64) and g (T,64) with normal=True, else None), the optional ones at the
    result.  iters = 0 evaluates at the start.  out: an earlier ArmVertexFitResult of the same shapes whose tensors are written instead of
    new ones — the call then allocates nothing (pass an int32 vert_idx) and can be captured into a graph."""
    _playback_input("arm_vertex_fit", targets, in_pose, betas, trans, weights, prior, vert_idx)
    _lm_float32("arm_vertex_fit", targets=targets, in_pose=in_pose, betas=betas, trans=trans, weights=weights, prior=prior)
    NV = int(dm.NV)
    if targets.dim() != 3 or targets.shape[2] != 3 or targets.shape[0] < 1 or not 1 <= targets.shape[1] <= NV:
        raise ValueError(f"targets must be (T, n_t <= {NV}, 3), got {tuple(targets.shape)}")
    T, n_t = int(targets.shape[0]), int(targets.shape[1])
    if vert_idx is None:
        if n_t != NV:
            raise ValueError(f"targets must be (T, {NV}, 3) without vert_idx, got {tuple(targets.shape)}")
    else:
        if vert_idx.dtype not in (torch.int32, torch.int64) or tuple(vert_idx.shape) != (n_t,):
            raise ValueError(f"vert_idx must be ({n_t},) int32 or int64, got {tuple(vert_idx.shape)} {vert_idx.dtype}")
        if not torch.cuda.is_current_stream_capturing() and (int(vert_idx.min()) < 0 or int(vert_idx.max()) >= NV):
            raise ValueError(f"vert_idx must lie in [0, {NV})")
        vert_idx = vert_idx.to(torch.int32).contiguous()
    solve_shape, solve_wrist = bool(solve_shape), bool(solve_wrist)
    _lm_shapes(("betas", betas, [(T, 10)] if solve_shape else [(T, 10), (10,)]), ("in_pose", in_pose, (T, 17, 3)), ("trans", trans, (T, 3)),
               ("weights", weights, (T, n_t)), ("prior", prior, (T, 45)))
    iters, lambda0 = int(iters), float(lambda0)
    pose_prior_weight, wrist_prior_weight, shape_prior_weight = float(pose_prior_weight), float(wrist_prior_weight), float(shape_prior_weight)
    _lm_scalars(iters, lambda0=lambda0, pose_prior_weight=pose_prior_weight, wrist_prior_weight=wrist_prior_weight,
                shape_prior_weight=shape_prior_weight)
    _lm_model_device(dm, targets)
    want = ((T, 17, 3), tuple(betas.shape), (T, 3), (T, 2), (T,), (T, NV, 3) if verts else None, (T, 3 * n_t, 64) if jac else None,
            (T, 64, 64) if normal else None, (T, 64) if normal else None)
    out = _lm_result(ArmVertexFitResult, want, out, targets.device)
    _lm_start(out, in_pose=in_pose, betas=betas, trans=trans)
    targets, weights, prior = map(_lm_input, (targets, weights, prior))
    opt = _lib.ArmVertexFitOptions(iters, lambda0, pose_prior_weight, wrist_prior_weight, shape_prior_weight, int(solve_shape), int(solve_wrist),
                                   int(betas.dim() == 2))
    with torch.cuda.device(targets.device):
        rc = _lib.lib().harp_arm_vertex_fit(ctypes.byref(dm.struct), _lib.ptr(vert_idx), n_t, _lib.ptr(targets), _lib.ptr(weights), _lib.ptr(prior),
                                            T, ctypes.byref(opt), _lib.ptr(out.in_pose), _lib.ptr(out.betas), _lib.ptr(out.trans),
                                            _lib.ptr(out.cost), _lib.ptr(out.status), _lib.ptr(out.verts), _lib.ptr(out.jac), _lib.ptr(out.A),
                                            _lib.ptr(out.g), _lib.stream())
    _lib.check(rc, "harp_arm_vertex_fit")
    return out


# ---- batched SMPL-X arm inverse kinematics (csrc/arm_ik.hip) --------------------------------------------------------
ArmIkResult = collections.namedtuple("ArmIkResult", "in_pose trans cost status joints jac")


def arm_ik_frames_per_block():
    """the frames one workgroup of harp_arm_ik solves"""
    return int(_lib.lib().harp_arm_ik_frames_per_block())


def arm_ik(dm, betas, targets, in_pose, trans, weights=None, prior=None, wrist_prior=None, solve_wrist=True, iters=15, lambda0=1e-3,
           pose_prior_weight=0.0, wrist_prior_weight=0.0, joints=False, jac=False, out=None):
    """3-D keypoints -> SMPL-X arm rows: T Levenberg-Marquardt solves in one launch (csrc/arm_ik.hip: harp_arm_ik, whose contract
    include/harp_hip.h states), forward only.  dm: a TreeDeviceModel (hand_models_harp.body_models) with n = n_joints_out output joints
    (the arm: 22 = the wrist, the five fingers root to tip, the elbow); betas (10,) for all frames or (T,10); targets (T,n,3) metres in the
    order of the model's joints; in_pose (T,17,3) = [rot | wrist | pose(15)] and trans (T,3): the start, left untouched; solve_wrist=False
    holds the wrist row at what in_pose gives; weights (T,n) or None (ones; a joint with weight <= 0 or a non-finite target is unused);
    prior (T,45) or None (the mean pose) with pose_prior_weight on sum (pose - prior)^2; wrist_prior (T,3) or None (zeros) with
    wrist_prior_weight on sum (wrist - wrist_prior)^2.  Returns ArmIkResult(in_pose, trans, cost (T,2) = at the start and at the result,
    status (T,) int32 = accepted steps or -1 for a frame with fewer than 3 used joints (returned as it came), joints (T,n,3) mm or None,
    jac (T,3 n,54) or None), the optional ones at the result.  iters = 0 evaluates at the start.  out: an earlier ArmIkResult of the same
    shapes whose tensors are written instead of new ones — the call then allocates nothing and can be captured into a graph."""
    _playback_input("arm_ik", betas, targets, in_pose, trans, weights, prior, wrist_prior)
    _lm_float32("arm_ik", betas=betas, targets=targets, in_pose=in_pose, trans=trans, weights=weights, prior=prior, wrist_prior=wrist_prior)
    n = int(dm.struct.n_joints_out)
    if targets.dim() != 3 or tuple(targets.shape[1:]) != (n, 3) or targets.shape[0] < 1:
        raise ValueError(f"targets must be (T, {n}, 3), got {tuple(targets.shape)}")
    T = int(targets.shape[0])
    _lm_shapes(("betas", betas, [(10,), (T, 10)]), ("in_pose", in_pose, (T, 17, 3)), ("trans", trans, (T, 3)), ("weights", weights, (T, n)),
               ("prior", prior, (T, 45)), ("wrist_prior", wrist_prior, (T, 3)))
    iters, lambda0, pose_prior_weight, wrist_prior_weight = int(iters), float(lambda0), float(pose_prior_weight), float(wrist_prior_weight)
    _lm_scalars(iters, lambda0=lambda0, pose_prior_weight=pose_prior_weight, wrist_prior_weight=wrist_prior_weight)
    _lm_model_device(dm, targets)
    out = _lm_result(ArmIkResult, ((T, 17, 3), (T, 3), (T, 2), (T,), (T, n, 3) if joints else None, (T, 3 * n, 54) if jac else None), out,
                     targets.device)
    _lm_start(out, in_pose=in_pose, trans=trans)
    betas, targets, weights, prior, wrist_prior = map(_lm_input, (betas, targets, weights, prior, wrist_prior))
    opt = _lib.ArmIkOptions(iters, lambda0, pose_prior_weight, wrist_prior_weight, int(bool(solve_wrist)), int(betas.dim() == 2))
    with torch.cuda.device(targets.device):
        rc = _lib.lib().harp_arm_ik(ctypes.byref(dm.struct), _lib.ptr(betas), _lib.ptr(targets), _lib.ptr(weights), _lib.ptr(prior),
                                    _lib.ptr(wrist_prior), T, ctypes.byref(opt), _lib.ptr(out.in_pose), _lib.ptr(out.trans), _lib.ptr(out.cost),
                                    _lib.ptr(out.status), _lib.ptr(out.joints), _lib.ptr(out.jac), _lib.stream())
    _lib.check(rc, "harp_arm_ik")
    return out


# ---- batched 2.5-D reprojection inverse kinematics of the MANO hand (csrc/reproj_ik.hip) ------------------------------
ReprojIkResult = collections.namedtuple("ReprojIkResult", "pose48 trans cost status proj jac")


def mano_reproj_ik_frames_per_block():
    """the problems one workgroup of harp_mano_reproj_ik solves"""
    return int(_lib.lib().harp_mano_reproj_ik_frames_per_block())


def mano_reproj_ik(dm, betas, targets, pose48, trans, cam, focal, S, weights=None, depth_weights=None, prior=None, z_prior=None, iters=20,
                   lambda0=1e-3, pose_prior_weight=0.0, z_prior_weight=0.0, proj=False, jac=False, out=None):
    """Image keypoints -> MANO pose rows: N Levenberg-Marquardt solves in one launch (csrc/reproj_ik.hip: harp_mano_reproj_ik, whose
    contract include/harp_hip.h states), forward only.  dm: a ManoDeviceModel; betas (10,) for all problems or (N,10); targets (N,21,3) =
    (u, v, d): continuous pixels (the centre of column i at i + 0.5) and the depth relative to the wrist in metres, in the order of the
    model's joints; pose48 (N,48) = [rot | pose] and trans (N,3): the start, left untouched; cam (3,) or (N,3), focal (pixels) and S (the
    image size): the player's camera; weights (N,21) or None (ones) on the pixel rows and depth_weights (N,21) or None (no depth rows),
    both in px^2 per squared unit of the residual — an entry with weight <= 0 or a non-finite target is unused; prior (N,45) or None (the
    mean pose) with pose_prior_weight on sum (pose - prior)^2; z_prior (N,) with z_prior_weight on (trans_z - z_prior)^2 (None: the weight
    must be 0).  Returns ReprojIkResult(pose48, trans, cost (N,2) = at the start and at the result, status (N,) int32 = accepted steps, -1
    for a problem with fewer than 4 used pixel joints or -2 for one with a used joint behind the camera at the start (both returned as
    they came), proj (N,21,3) = (u, v, d) or None, jac (N,63,51) or None).  iters = 0 evaluates at the start.  out: an earlier
    ReprojIkResult of the same shapes whose tensors are written instead of new ones — the call then allocates nothing and can be
    captured into a graph."""
    _playback_input("mano_reproj_ik", betas, targets, pose48, trans, cam, weights, depth_weights, prior, z_prior)
    _lm_float32("mano_reproj_ik", betas=betas, targets=targets, pose48=pose48, trans=trans, cam=cam, weights=weights,
                depth_weights=depth_weights, prior=prior, z_prior=z_prior)
    if targets.dim() != 3 or tuple(targets.shape[1:]) != (21, 3) or targets.shape[0] < 1:
        raise ValueError(f"targets must be (N, 21, 3), got {tuple(targets.shape)}")
    N = targets.shape[0]
    _lm_shapes(("betas", betas, [(10,), (N, 10)]), ("cam", cam, [(3,), (N, 3)]), ("pose48", pose48, (N, 48)), ("trans", trans, (N, 3)),
               ("weights", weights, (N, 21)), ("depth_weights", depth_weights, (N, 21)), ("prior", prior, (N, 45)), ("z_prior", z_prior, (N,)))
    iters, lambda0, pose_prior_weight, z_prior_weight, focal = int(iters), float(lambda0), float(pose_prior_weight), float(z_prior_weight), float(focal)
    _lm_scalars(iters, lambda0=lambda0, pose_prior_weight=pose_prior_weight, z_prior_weight=z_prior_weight)
    if not (0.0 < focal < float("inf")) or int(S) != S or int(S) <= 0:
        raise ValueError(f"focal > 0 and an image size S >= 1, got {focal}, {S}")
    if z_prior is None and z_prior_weight != 0.0:
        raise ValueError("z_prior_weight needs z_prior")
    _lm_model_device(dm, targets)
    out = _lm_result(ReprojIkResult, ((N, 48), (N, 3), (N, 2), (N,), (N, 21, 3) if proj else None, (N, 63, 51) if jac else None), out,
                     targets.device)
    _lm_start(out, pose48=pose48, trans=trans)
    betas, targets, cam, weights, depth_weights, prior, z_prior = map(_lm_input, (betas, targets, cam, weights, depth_weights, prior, z_prior))
    opt = _lib.ReprojIkOptions(iters, lambda0, pose_prior_weight, z_prior_weight, int(betas.dim() == 2), int(cam.dim() == 2), focal, int(S))
    with torch.cuda.device(targets.device):
        rc = _lib.lib().harp_mano_reproj_ik(ctypes.byref(dm.struct), _lib.ptr(betas), _lib.ptr(cam), _lib.ptr(targets), _lib.ptr(weights),
                                            _lib.ptr(depth_weights), _lib.ptr(prior), _lib.ptr(z_prior), N, ctypes.byref(opt),
                                            _lib.ptr(out.pose48), _lib.ptr(out.trans), _lib.ptr(out.cost), _lib.ptr(out.status),
                                            _lib.ptr(out.proj), _lib.ptr(out.jac), _lib.stream())
    _lib.check(rc, "harp_mano_reproj_ik")
    return out


# ---- batched 2.5-D reprojection inverse kinematics of the SMPL-X arm (csrc/arm_reproj_ik.hip) -------------------------
ArmReprojIkResult = collections.namedtuple("ArmReprojIkResult", "in_pose trans cost status proj jac")


def arm_reproj_ik_frames_per_block():
    """the problems one workgroup of harp_arm_reproj_ik solves"""
    return int(_lib.lib().harp_arm_reproj_ik_frames_per_block())


def arm_reproj_ik(dm, betas, targets, in_pose, trans, cam, focal, S, weights=None, depth_weights=None, prior=None, wrist_prior=None, z_prior=None,
                  solve_wrist=True, iters=20, lambda0=1e-3, pose_prior_weight=0.0, wrist_prior_weight=0.0, z_prior_weight=0.0, proj=False,
                  jac=False, out=None):
    """Image keypoints -> SMPL-X arm rows: N Levenberg-Marquardt solves in one launch (csrc/arm_reproj_ik.hip: harp_arm_reproj_ik, whose
    contract include/harp_hip.h states), forward only.  dm: a TreeDeviceModel (hand_models_harp.body_models) with n = n_joints_out output
    joints (the arm: 22 = the wrist, the five fingers root to tip, the elbow); betas (10,) for all problems or (N,10); targets (N,n,3) =
    (u, v, d): continuous pixels (the centre of column i at i + 0.5) and the depth relative to the wrist in metres, in the order of the
    model's joints; in_pose (N,17,3) = [rot | wrist | pose(15)] and trans (N,3): the start, left untouched; solve_wrist=False holds the
    wrist row at what in_pose gives; cam (3,) or (N,3), focal (pixels) and S (the image size): the player's camera; weights (N,n) or None
    (ones) on the pixel rows and depth_weights (N,n) or None (no depth rows), both in px^2 per squared unit of the residual — an entry with
    weight <= 0 or a non-finite target is unused; prior (N,45) or None (the mean pose) with pose_prior_weight on sum (pose - prior)^2;
    wrist_prior (N,3) or None (zeros) with wrist_prior_weight on sum (wrist - wrist_prior)^2; z_prior (N,) with z_prior_weight on
    (trans_z - z_prior)^2 (None: the weight must be 0).  Returns ArmReprojIkResult(in_pose, trans, cost (N,2) = at the start and at the
    result, status (N,) int32 = accepted steps, -1 for a problem with fewer than 4 used pixel joints, -2 for a tree the kernel's tables do
    not hold or -3 for one with a used joint behind the camera at the start (all returned as they came), proj (N,n,3) = (u, v, d) or None,
    jac (N,3 n,54) or None), the optional ones at the result.  iters = 0 evaluates at the start.  out: an earlier ArmReprojIkResult of the
    same shapes whose tensors are written instead of new ones — the call then allocates nothing and can be captured into a graph."""
    _playback_input("arm_reproj_ik", betas, targets, in_pose, trans, cam, weights, depth_weights, prior, wrist_prior, z_prior)
    _lm_float32("arm_reproj_ik", betas=betas, targets=targets, in_pose=in_pose, trans=trans, cam=cam, weights=weights, depth_weights=depth_weights,
                prior=prior, wrist_prior=wrist_prior, z_prior=z_prior)
    n = int(dm.struct.n_joints_out)
    if targets.dim() != 3 or tuple(targets.shape[1:]) != (n, 3) or targets.shape[0] < 1:
        raise ValueError(f"targets must be (N, {n}, 3), got {tuple(targets.shape)}")
    N = int(targets.shape[0])
    _lm_shapes(("betas", betas, [(10,), (N, 10)]), ("cam", cam, [(3,), (N, 3)]), ("in_pose", in_pose, (N, 17, 3)), ("trans", trans, (N, 3)),
               ("weights", weights, (N, n)), ("depth_weights", depth_weights, (N, n)), ("prior", prior, (N, 45)),
               ("wrist_prior", wrist_prior, (N, 3)), ("z_prior", z_prior, (N,)))
    iters, lambda0, focal = int(iters), float(lambda0), float(focal)
    pose_prior_weight, wrist_prior_weight, z_prior_weight = float(pose_prior_weight), float(wrist_prior_weight), float(z_prior_weight)
    _lm_scalars(iters, lambda0=lambda0, pose_prior_weight=pose_prior_weight, wrist_prior_weight=wrist_prior_weight, z_prior_weight=z_prior_weight)
    if not (0.0 < focal < float("inf")) or int(S) != S or int(S) <= 0:
        raise ValueError(f"focal > 0 and an image size S >= 1, got {focal}, {S}")
    if z_prior is None and z_prior_weight != 0.0:
        raise ValueError("z_prior_weight needs z_prior")
    _lm_model_device(dm, targets)
    out = _lm_result(ArmReprojIkResult, ((N, 17, 3), (N, 3), (N, 2), (N,), (N, n, 3) if proj else None, (N, 3 * n, 54) if jac else None), out,
                     targets.device)
    _lm_start(out, in_pose=in_pose, trans=trans)
    betas, targets, cam, weights, depth_weights, prior, wrist_prior, z_prior = map(
        _lm_input, (betas, targets, cam, weights, depth_weights, prior, wrist_prior, z_prior))
    opt = _lib.ArmReprojIkOptions(iters, lambda0, pose_prior_weight, wrist_prior_weight, z_prior_weight, int(bool(solve_wrist)),
                                  int(betas.dim() == 2), int(cam.dim() == 2), focal, int(S))
    with torch.cuda.device(targets.device):
        rc = _lib.lib().harp_arm_reproj_ik(ctypes.byref(dm.struct), _lib.ptr(betas), _lib.ptr(cam), _lib.ptr(targets), _lib.ptr(weights),
                                           _lib.ptr(depth_weights), _lib.ptr(prior), _lib.ptr(wrist_prior), _lib.ptr(z_prior), N,
                                           ctypes.byref(opt), _lib.ptr(out.in_pose), _lib.ptr(out.trans), _lib.ptr(out.cost),
                                           _lib.ptr(out.status), _lib.ptr(out.proj), _lib.ptr(out.jac), _lib.stream())
    _lib.check(rc, "harp_arm_reproj_ik")
    return out
