"""More known-answer tests for the CPU oracle: the parts of the hot path whose arithmetic lives in
PyTorch3D (absent from /root/reference -> "parity unpinned") are pinned here against INDEPENDENT constructions — analytic ray casting
in numpy float64 for the shadow / lighting chain, hand-derived closed forms for the tangent frame, the mesh regularisers and
look_at_rotation — plus fp64 `torch.autograd.gradcheck` of every differentiable oracle op."""
import math

import numpy as np
import pytest
import torch

from harp_amd import topology
from oracle import harp_ref as H
from oracle import p3d_like as P

F64 = torch.float64


# ----------------------------------------------------------------------------------------------------------------------
# Scene of two axis-aligned rectangles: a receiver in the plane z = 0 and a smaller occluder in the plane z = zo < 0
# (camera and light both sit on the -z side), rendered by the oracle and, independently, by ray casting.
# ----------------------------------------------------------------------------------------------------------------------
RECV = (-0.12, 0.11, -0.10, 0.13, 0.0)          # x0, x1, y0, y1, z
OCCL = (-0.035, 0.025, -0.02, 0.03, -0.04)


def _quad(r):
    x0, x1, y0, y1, z = r
    return [[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]]


def _two_quads():
    v = torch.tensor(_quad(RECV) + _quad(OCCL), dtype=F64)
    # winding such that the area-weighted vertex normal (v2-v1)x(v0-v1) (Appendix A.7) points to -z, towards camera and light
    f = torch.tensor([[0, 2, 1], [0, 3, 2], [4, 6, 5], [4, 7, 6]])
    return v, f


def _ray_hit(o, d):
    """nearest intersection of rays o + t d (t > 0) with the two rectangles: (t, which) with which = 0 receiver, 1 occluder, -1 none"""
    best_t = np.full(d.shape[:-1], np.inf)
    which = np.full(d.shape[:-1], -1)
    for k, (x0, x1, y0, y1, z) in enumerate((RECV, OCCL)):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (z - o[..., 2]) / d[..., 2]
        p = o + t[..., None] * d
        ok = (t > 0) & (p[..., 0] > x0) & (p[..., 0] < x1) & (p[..., 1] > y0) & (p[..., 1] < y1) & (t < best_t)
        best_t = np.where(ok, t, best_t)
        which = np.where(ok, k, which)
    return best_t, which


def _look_at(pos, at, up=np.array([0.0, 1.0, 0.0])):
    z = (at - pos) / np.linalg.norm(at - pos)
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x); y /= np.linalg.norm(y)
    return np.stack([x, y, z], 1)                       # columns x, y, z (row-vector convention X_view = X_world R + T)


def _independent_render(S, focal, cam, light_pos, amb, tex_rgb):
    """numpy float64 restatement by ray casting of: K=1 camera rasterisation, hit points, the light camera of
    process_info_for_shadow (renderer_helper.py:454-468), its depth map, the 3x3 shadow test (:385-408) and
    colour = (ambient + diffuse * vis) * texel (:513-518) for a constant texture and a flat (+z) normal map."""
    pc = -1.0 + (2.0 * (S - 1 - np.arange(S)) + 1.0) / S                      # NDC of pixel centres (Appendix A.2)
    PX, PY = np.meshgrid(pc, pc, indexing="xy")                               # [row, col]
    k = S / (2.0 * focal)
    # camera: X_view = (-x - c1, -y - c2, z + tz)  (utils/visualize.py:268-271)
    tz = 2.0 * focal / (S * cam[0] + 1e-9)
    o_cam = np.array([-cam[1], -cam[2], -tz])                                 # world position of the camera centre
    d_cam = np.stack([-PX * k, -PY * k, np.ones_like(PX)], -1)               # world direction of the pixel ray (view z = 1)
    t, which = _ray_hit(np.broadcast_to(o_cam, d_cam.shape), d_cam)
    covered = which >= 0
    p = o_cam + np.where(covered, t, 0.0)[..., None] * d_cam                  # hit points (world)
    # light camera
    verts = np.array(_quad(RECV) + _quad(OCCL))
    c = verts.mean(0)
    dl = light_pos - c
    pos = c + dl * (1.5 / np.linalg.norm(dl))
    R = _look_at(pos, c)
    T = -R.T @ pos
    # light-view depth map by ray casting: view direction (px k, py k, 1) -> world direction R (view) (X_world = (X_view - T) R^T)
    d_view = np.stack([PX * k, PY * k, np.ones_like(PX)], -1)
    d_l = d_view @ R.T
    tl, wl = _ray_hit(np.broadcast_to(pos, d_l.shape), d_l)
    zl = np.where(wl >= 0, tl, -1.0)                                          # view depth == t because the view-space direction has z = 1
    # hit points in the light view, their screen pixel (transform_points_screen: x right, y down), 3x3 taps
    q = p @ R + T
    xs = S / 2.0 - focal * q[..., 0] / q[..., 2]
    ys = S / 2.0 - focal * q[..., 1] / q[..., 2]
    ix, iy = np.rint(xs).astype(np.int64), np.rint(ys).astype(np.int64)       # torch.round(): half to even
    vis = np.zeros_like(xs)
    for ii in (-1, 0, 1):
        for jj in (-1, 0, 1):
            d_at = zl[np.clip(iy + ii, 0, S - 1), np.clip(ix + jj, 0, S - 1)]
            vis += 1.0 / (1.0 + np.exp(np.clip(-(d_at - (q[..., 2] - 0.008)) * 1000.0, -700.0, 700.0)))
    vis /= 9.0
    # Lambert: both rectangles face -z; l^ = normalize(light_pos - p)
    n = np.array([0.0, 0.0, -1.0])
    l = light_pos - p
    l /= np.linalg.norm(l, axis=-1, keepdims=True)
    cosang = np.maximum((l * n).sum(-1), 0.0)
    a = 1.0 / (1.0 + math.exp(-amb))
    shade = a + (1.0 - a) * cosang * vis
    img = np.where(covered[..., None], shade[..., None] * np.asarray(tex_rgb), 1.0)
    return dict(covered=covered, which=which, p=p, zl=zl, vis=vis, img=img, R=R, T=T, depth=np.where(covered, t, -1.0))


@pytest.mark.parametrize("light", [(-0.3, -0.2, -1.0), (0.25, 0.1, -0.6), (0.003, -0.002, -1.0)])
def test_quad_shadows_quad_against_ray_casting(light):
    S = 64
    focal = 1000.0 * S / 224.0
    cam = np.array([2.0 * focal / (S * 1.1), 0.003, -0.007])               # tz = 1.1 m; small offsets keep pixel centres off the quads' diagonals
    v, f = _two_quads()
    tex_rgb = (0.8, 0.55, 0.3)
    amb = 0.4
    params = dict(texture=torch.tensor(tex_rgb, dtype=F64).repeat(1, 16, 16, 1), normal_map=torch.tensor([0.0, 0.0, 1.0], dtype=F64).repeat(1, 16, 16, 1),
                  amb_ratio=torch.tensor(amb, dtype=F64), light_positions=torch.tensor([light], dtype=F64),
                  verts_uvs=torch.tensor([[0.1, 0.1], [0.9, 0.1], [0.9, 0.9], [0.1, 0.9]] * 2, dtype=F64), faces_uvs=f.clone())
    img, aux = H.render_rgb(v[None], {"faces": f}, params, torch.from_numpy(cam)[None], S, focal, self_shadow=True, return_aux=True)
    ref = _independent_render(S, focal, cam, np.asarray(light, dtype=np.float64), amb, tex_rgb)
    cov = torch.from_numpy(ref["covered"])
    # K=1 coverage, nearest face (faces 0,1 = receiver, 2,3 = occluder) and perspective-correct depth
    p2f = aux["pix_to_face"][0, :, :, 0]
    assert torch.equal(p2f >= 0, cov)
    assert torch.equal((p2f >= 2)[cov], torch.from_numpy(ref["which"] == 1)[cov])
    assert (aux["zbuf"][0, :, :, 0] - torch.from_numpy(ref["depth"])).abs().max() < 1e-10
    # look_at_rotation + light_T (Appendix A.9; renderer_helper.py:466-467)
    assert (aux["light_R"][0] - torch.from_numpy(ref["R"])).abs().max() < 1e-12
    assert (aux["light_T"][0] - torch.from_numpy(ref["T"])).abs().max() < 1e-12
    # light-view depth map (-1 where the light camera sees nothing)
    assert (aux["zbuf_light"][0, :, :, 0] - torch.from_numpy(ref["zl"])).abs().max() < 1e-10
    # shadow term: rounding, clamping and the 9 sigmoid taps
    vis = aux["vis"][0, :, :, 0]
    assert (vis - torch.from_numpy(ref["vis"]))[cov].abs().max() < 1e-9
    recv = cov & torch.from_numpy(ref["which"] == 0)
    if abs(light[0]) > 0.1:                                                  # (an on-axis light hides its shadow behind the occluder)
        assert (vis[recv] < 0.02).any() and (vis[recv] > 0.98).any()       # the receiver is partly shadowed, partly lit
    assert (vis[cov & ~recv] > 0.98).all()                                   # nothing shadows the occluder
    # ambient + diffuse * visibility composition and the K=1 blend (background exactly white)
    assert (img[0] - torch.from_numpy(ref["img"])).abs().max() < 1e-9


def test_shadow_taps_clamp_at_light_image_border():
    """a receiver larger than the light camera's frustum: hit points projecting outside the light image use the clamped border
    texel (renderer_helper.py:399-401) -> fully lit for a plane facing the light; and empty light pixels (zbuf = -1) count as shadow"""
    S = 32
    focal = 1000.0 * S / 224.0
    big = torch.tensor([[-3.0, -2.5, 0.0], [3.1, -2.5, 0.0], [3.1, 2.7, 0.0], [-3.0, 2.7, 0.0]], dtype=F64)     # (not a square: its diagonal misses the pixel centres)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]])
    params = dict(texture=torch.full((1, 4, 4, 3), 0.5, dtype=F64), normal_map=torch.tensor([0.0, 0.0, 1.0], dtype=F64).repeat(1, 4, 4, 1),
                  amb_ratio=torch.tensor(0.0, dtype=F64), light_positions=torch.tensor([[0.05, 0.1, -1.0]], dtype=F64),      # straight above the centroid: the plane is fronto-parallel in the light view
                  verts_uvs=torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=F64), faces_uvs=f.clone())
    cam = torch.tensor([[2.0 * focal / (S * 3.0), 0.011, 0.017]], dtype=F64)       # camera 3 m away sees more of the plane than the light camera (1.5 m)
    _, aux = H.render_rgb(big[None], {"faces": f}, params, cam, S, focal, self_shadow=True, return_aux=True)
    assert (aux["zbuf_light"] > 0).all()                                               # the plane fills the light view
    cov = aux["pix_to_face"][0, :, :, 0] >= 0
    assert cov.float().mean() > 0.95
    # some camera pixels do land outside the light image: reproduce their screen coordinates
    q = torch.einsum("hwc,cd->hwd", P.interpolate_face_attributes(aux["pix_to_face"], aux["bary"], big[f])[0, :, :, 0], aux["light_R"][0]) + aux["light_T"][0]
    xs = S / 2.0 - focal * q[..., 0] / q[..., 2]
    assert ((xs < -2) | (xs > S + 1))[cov].any()
    assert (aux["vis"][0, :, :, 0][cov] - 1.0 / (1.0 + math.exp(-8.0))).abs().max() < 1e-9
    # a small receiver: taps that fall off its silhouette in the light view read -1 -> sigmoid(-1000 * ~2.5) = 0, so vis = k/9 * sigmoid(8)
    small = big * 0.01
    params["light_positions"] = params["light_positions"] * torch.tensor([0.01, 0.01, 1.0], dtype=F64)
    _, aux = H.render_rgb(small[None], {"faces": f}, params, torch.tensor([[2.0 * focal / (S * 1.0), 0.0003, 0.0007]], dtype=F64), S, focal,
                          self_shadow=True, return_aux=True)
    cov = aux["pix_to_face"][0, :, :, 0] >= 0
    lit = 1.0 / (1.0 + math.exp(-8.0))
    ninth = (aux["vis"][0, :, :, 0][cov] / (lit / 9.0))
    assert (ninth - ninth.round()).abs().max() < 1e-6 and ninth.min() < 8.5 and ninth.max() > 8.5     # every value is an integer count of lit taps


# ----------------------------------------------------------------------------------------------------------------------
# tangent frame + normal map (renderer/pbr_materials.py:58-124)
# ----------------------------------------------------------------------------------------------------------------------
def test_tangent_frame_closed_forms():
    th = 0.7
    s_, c_ = math.sin(th), math.cos(th)
    n = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [s_, 0.0, c_], [0.0, 0.0, 0.0]], dtype=F64)
    uv = H.compute_tangent(n)
    want = torch.tensor([[[1, 0, 0], [0, 1, 0]],                       # z = 1: s = 1, a = -1/2, b = 0
                         [[1, 0, 0], [0, -1, 0]],                      # z = -1: s = -1, a = 1/2
                         [[c_, 0, -s_], [0, 1, 0]],                    # 1 - sin^2/(1+cos) = cos
                         [[1, 0, 0], [0, 1, 0]]], dtype=F64)           # zero normal (empty pixel): s = 1 (z >= 0), a = -1
    assert (uv - want).abs().max() < 1e-12
    # unit normals: {u, v, n} is an orthonormal basis (Pixar "Building an orthonormal basis, revisited")
    g = torch.Generator().manual_seed(0)
    nn = torch.nn.functional.normalize(torch.randn(200, 3, generator=g, dtype=F64), dim=-1)
    uv = H.compute_tangent(nn)
    M = torch.cat([uv, nn[:, None]], 1)
    assert (M @ M.transpose(1, 2) - torch.eye(3, dtype=F64)).abs().max() < 1e-12
    # the reference feeds UN-normalised normals (Appendix C.4): n = 2 (sin, 0, cos) by hand
    x, z = 2 * s_, 2 * c_
    a = -1.0 / (1.0 + z)
    uv2 = H.compute_tangent(torch.tensor([[x, 0.0, z]], dtype=F64))
    assert (uv2[0] - torch.tensor([[1 + x * x * a, 0.0, -x], [0.0, 1.0, 0.0]], dtype=F64)).abs().max() < 1e-12


def test_apply_normal_map_tilted_plane():
    th = 0.5
    s_, c_ = math.sin(th), math.cos(th)
    pn = torch.tensor([s_, 0.0, c_], dtype=F64).expand(1, 2, 2, 1, 3).contiguous()
    flat = torch.tensor([0.0, 0.0, 1.0], dtype=F64).expand(1, 2, 2, 1, 3)
    assert (H.apply_normal_map(pn, flat) - pn).abs().max() < 1e-12          # m = +z leaves the (normalised) normal alone
    m = torch.nn.functional.normalize(torch.tensor([0.3, -0.2, 0.9], dtype=F64), dim=0)
    got = H.apply_normal_map(pn, m.expand(1, 2, 2, 1, 3))[0, 0, 0, 0]
    # TBN rows = (-u, -v, n) with u = (cos, 0, -sin), v = (0, 1, 0): n' = normalize(-m_x u - m_y v + m_z n)
    want = -m[0] * torch.tensor([c_, 0.0, -s_], dtype=F64) - m[1] * torch.tensor([0.0, 1.0, 0.0], dtype=F64) + m[2] * torch.tensor([s_, 0.0, c_], dtype=F64)
    assert (got - want / want.norm()).abs().max() < 1e-12
    assert abs(got.norm().item() - 1.0) < 1e-12
    # -z facing normal: s = -1 flips the sign of v's y component: n' = (-m_x, +m_y, -m_z)
    got = H.apply_normal_map(torch.tensor([0.0, 0.0, -1.0], dtype=F64).expand(1, 1, 1, 1, 3), m.expand(1, 1, 1, 1, 3))[0, 0, 0, 0]
    assert (got - torch.stack([-m[0], m[1], -m[2]])).abs().max() < 1e-12


def test_no_shadow_renderer_lighting_constants():
    """phong renderer without shadows (renderer_helper.py:60-81, 106-190): ambient .5, diffuse .4, shininess-0 specular = constant .1"""
    S = 16
    focal = 1000.0 * S / 224.0
    v = torch.tensor(_quad((-0.3, 0.3, -0.3, 0.3, 0.0)), dtype=F64)
    f = torch.tensor([[0, 2, 1], [0, 3, 2]])                                   # vertex normals towards -z (camera / light side)
    params = dict(texture=torch.full((1, 4, 4, 3), 0.5, dtype=F64), normal_map=torch.tensor([0.0, 0.0, 1.0], dtype=F64).repeat(1, 4, 4, 1),
                  amb_ratio=torch.tensor(0.4, dtype=F64), light_positions=torch.tensor([[0.0, 0.0, -2.0]], dtype=F64),
                  verts_uvs=torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]], dtype=F64), faces_uvs=f.clone())
    cam = torch.tensor([[2.0 * focal / (S * 1.0), 0.001, 0.002]], dtype=F64)
    img, aux = H.render_rgb(v[None], {"faces": f}, params, cam, S, focal, self_shadow=False, return_aux=True)
    cov = aux["pix_to_face"][0, :, :, 0] >= 0
    assert cov.all()
    p = P.interpolate_face_attributes(aux["pix_to_face"], aux["bary"], v[f])[0, :, :, 0]
    l = torch.tensor([0.0, 0.0, -2.0], dtype=F64) - p
    cosang = (-l[..., 2] / l.norm(dim=-1)).clamp(min=0)                        # normal = -z
    want = (0.5 + 0.4 * cosang)[..., None] * 0.5 + 0.1
    assert (img[0] - want).abs().max() < 1e-9


# ----------------------------------------------------------------------------------------------------------------------
# mesh regularisers (optimize_sequence.py:536-537; Appendix A.11 / A.12), on tables built by harp_amd.topology
# ----------------------------------------------------------------------------------------------------------------------
def _tables(faces, V):
    edges, _ = topology.unique_edges(faces, V)
    rows = np.concatenate([edges[:, 0], edges[:, 1]])
    cols = np.concatenate([edges[:, 1], edges[:, 0]])
    off, idx = topology.csr_from_pairs(rows, cols, V)
    return torch.from_numpy(off).long(), torch.from_numpy(idx).long(), torch.from_numpy(topology.normal_consistency_pairs(faces, V)).long()


def test_laplacian_uniform_closed_form():
    # two triangles sharing edge (0,1): neighbours 0:{1,2,3} 1:{0,2,3} 2:{0,1} 3:{0,1}
    faces = np.array([[0, 1, 2], [1, 0, 3]])
    off, idx, _ = _tables(faces, 4)
    v = torch.tensor([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 3.0, 0.0], [1.0, -1.0, 2.0]]], dtype=F64)
    nb = {0: [1, 2, 3], 1: [0, 2, 3], 2: [0, 1], 3: [0, 1]}
    want = sum((v[0, nb[i]].mean(0) - v[0, i]).norm() for i in range(4)) / 4.0
    got = P.mesh_laplacian_smoothing_uniform(v, off, idx)
    assert abs(got.item() - want.item()) < 1e-12
    # batch of 2 = mean over meshes; a regular hexagon fan with the centre lifted by h: centre term is exactly h
    v2 = torch.cat([v, v * 2.0])
    assert abs(P.mesh_laplacian_smoothing_uniform(v2, off, idx).item() - 1.5 * want.item()) < 1e-12
    ang = torch.arange(6, dtype=F64) * (math.pi / 3)
    ring = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros(6, dtype=F64)], 1)
    hexv = torch.cat([torch.tensor([[0.0, 0.0, 0.25]], dtype=F64), ring])[None]
    hexf = np.array([[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)])
    off, idx, pairs = _tables(hexf, 7)
    lv = P.mesh_laplacian_smoothing_uniform(hexv, off, idx) * 7.0
    # rim vertex i: neighbours = centre and its two ring neighbours; by symmetry all six rim terms are equal
    r0 = (torch.stack([hexv[0, 0], hexv[0, 2], hexv[0, 6]]).mean(0) - hexv[0, 1]).norm()
    assert abs(lv.item() - (0.25 + 6 * r0.item())) < 1e-12
    assert pairs.shape[0] == 6                                                # six interior edges, boundary edges have no pair


def test_laplacian_isolated_vertex_adds_its_norm():
    # PyTorch3D's laplacian_packed takes 1/deg = 0 at a vertex of degree 0: its row is -v, which adds |v| / V (and not 0 * inf = NaN)
    faces = np.array([[0, 1, 2], [1, 0, 3]])
    off, idx, _ = _tables(faces, 5)                                           # vertex 4 is in no face
    assert off[5] - off[4] == 0
    v = torch.tensor([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 3.0, 0.0], [1.0, -1.0, 2.0], [3.0, -4.0, 12.0]]], dtype=F64)
    nb = {0: [1, 2, 3], 1: [0, 2, 3], 2: [0, 1], 3: [0, 1]}
    rest = sum((v[0, nb[i]].mean(0) - v[0, i]).norm() for i in range(4))
    vv = v.clone().requires_grad_()
    got = P.mesh_laplacian_smoothing_uniform(vv, off, idx)
    assert abs(got.item() - (rest.item() + 13.0) / 5.0) < 1e-12             # |(3, -4, 12)| = 13
    got.backward()
    assert torch.allclose(vv.grad[0, 4], v[0, 4] / 13.0 / 5.0, rtol=0, atol=1e-15)   # d|v|/dv / V: the row's own gradient only
    assert torch.isfinite(vv.grad).all()


def test_normal_consistency_closed_form_and_torch111_clamp():
    faces = np.array([[0, 1, 2], [1, 0, 3]])
    _, _, pairs = _tables(faces, 4)
    assert pairs.shape == (1, 4) and sorted(pairs[0, :2].tolist()) == [0, 1] and sorted(pairs[0, 2:].tolist()) == [2, 3]
    for phi in (0.0, 0.4, 1.2, math.pi / 2, 2.5):
        # hinge along the x axis; first wing in the xy plane, second wing rotated by phi out of it: dihedral = pi - phi
        v = torch.tensor([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 1.5, 0.0], [1.0, -1.5 * math.cos(phi), 1.5 * math.sin(phi)]]], dtype=F64)
        got = P.mesh_normal_consistency(v, pairs)
        assert abs(got.item() - (1.0 - math.cos(phi))) < 1e-12, phi         # flat (phi = 0) -> 0, folded back -> 2
    # millimetre-sized triangles in metre units: |n0|^2 |n1|^2 < eps^2 = 1e-16 -> torch 1.11's cosine_similarity clamps the PRODUCT:
    # loss = 1 - (n0 . n1) / 1e-8
    sc = 1e-3
    v = torch.tensor([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 1.5, 0.0], [1.0, -1.5 * math.cos(0.4), 1.5 * math.sin(0.4)]]], dtype=F64) * sc
    n0n1 = (3.0 * sc * sc) ** 2 * math.cos(0.4)                             # |n| = |e| h = 2 * 1.5 * sc^2 for both wings
    assert (3.0 * sc * sc) ** 4 < 1e-16
    assert abs(P.mesh_normal_consistency(v, pairs).item() - (1.0 - n0n1 / 1e-8)) < 1e-12
    # just above the clamp the plain cosine comes back
    v = v * 20.0
    assert (3.0 * (20 * sc) ** 2) ** 4 > 1e-16
    assert abs(P.mesh_normal_consistency(v, pairs).item() - (1.0 - math.cos(0.4))) < 1e-10


def test_look_at_rotation_branches():
    up = torch.tensor([[0.0, 1.0, 0.0]], dtype=F64)
    at = torch.zeros(1, 3, dtype=F64)
    # generic: orthonormal, right-handed, third column = viewing direction
    pos = torch.tensor([[0.4, -0.3, -1.2]], dtype=F64)
    R = P.look_at_rotation(pos, at, up)[0]
    assert (R.T @ R - torch.eye(3, dtype=F64)).abs().max() < 1e-12 and abs(torch.det(R).item() - 1.0) < 1e-12
    assert (R[:, 2] - (-pos[0] / pos[0].norm())).abs().max() < 1e-12
    assert abs(R[1, 0].item()) < 1e-12                                        # x axis = up x z has no y component
    # camera exactly above the target: up x z = 0 -> x, y and the replacement x are all zero vectors (PyTorch3D's documented
    # degenerate output: normalize() of a zero vector with eps); z is still the viewing direction
    R = P.look_at_rotation(torch.tensor([[0.0, 1.5, 0.0]], dtype=F64), at, up)[0]
    assert (R[:, 0].abs().max() == 0) and (R[:, 1].abs().max() == 0) and (R[:, 2] - torch.tensor([0.0, -1.0, 0.0], dtype=F64)).abs().max() < 1e-12
    # nearly degenerate, |up x z| = 2e-8 < 5e-3 * eps: x = (up x z)/eps is "close to 0" -> replaced by normalize(y x z), a unit vector
    R = P.look_at_rotation(torch.tensor([[2e-8 * 1.5, 1.5, 0.0]], dtype=F64), at, up)[0]
    assert abs(R[:, 0].norm().item() - 1.0) < 1e-9 and abs((R[:, 0] * R[:, 2]).sum().item()) < 1e-9


def test_k_cap_keeps_the_nearest_faces():
    """faces_per_pixel is a CAP: with 3 stacked triangles and K = 2 the farthest is dropped (silhouette product over the K nearest
    only, renderer_helper.py:44-55 uses K = 50 which never binds for a hand: Appendix C.7)"""
    S = 12
    tri = [[0.9, 0.9], [-0.7, 0.9], [0.9, -0.7]]
    v = torch.tensor([[[x, y, z] for z in (3.0, 1.0, 2.0) for x, y in tri]], dtype=F64)
    f = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    p2f, zbuf, _, d = P.rasterize_meshes(v, f, S, 1e-3, 2)
    cov = p2f[0, :, :, 0] >= 0
    assert cov.any() and (p2f[0, :, :, 0][cov] == 1).all() and (p2f[0, :, :, 1][cov] == 2).all()      # z = 1 then z = 2; z = 3 dropped
    p3, z3, _, d3 = P.rasterize_meshes(v, f, S, 1e-3, 3)
    assert (p3[0, :, :, 2][cov] == 0).all()
    a2, a3 = P.sigmoid_alpha_blend(p2f, d, 1e-2), P.sigmoid_alpha_blend(p3, d3, 1e-2)
    rim = cov & (a3[0] < 1 - 1e-9)
    assert rim.any() and (a2[0][rim] < a3[0][rim]).all()                     # the capped product misses the third factor
    # equal depths: ties keep the lower face index first
    v_eq = torch.tensor([[[x, y, 2.0] for _ in range(2) for x, y in tri]], dtype=F64)
    p, _, _, _ = P.rasterize_meshes(v_eq, torch.tensor([[0, 1, 2], [3, 4, 5]]), S, 0.0, 1)
    assert (p[p >= 0] == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# fp64 gradcheck of every differentiable oracle op
# ----------------------------------------------------------------------------------------------------------------------
def _small_mesh(seed=0):
    g = torch.Generator().manual_seed(seed)
    faces0 = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [5, 2, 1], [5, 3, 2], [5, 4, 3], [5, 1, 4]])   # octahedron
    v = torch.tensor([[0, 0, 0.3], [0.3, 0, 0], [0, 0.3, 0], [-0.3, 0, 0], [0, -0.3, 0], [0, 0, -0.3]], dtype=F64)
    v = v + torch.randn(6, 3, generator=g, dtype=F64) * 0.02
    return v, torch.from_numpy(faces0).long(), faces0


def test_gradcheck_rasterizer_and_blends():
    S = 10
    v, f, _ = _small_mesh()
    ndc0 = (v * torch.tensor([2.2, 2.2, 1.0], dtype=F64) + torch.tensor([0.013, -0.021, 2.0], dtype=F64))[None]

    def hard(ndc):
        _, zbuf, bary, _ = P.rasterize_meshes(ndc, f, S, 0.0, 1)
        m = zbuf > 0
        return zbuf[m].sum() + (bary[m.unsqueeze(-1).expand_as(bary)] ** 2).sum()

    def soft(ndc):
        p2f, zbuf, bary, d = P.rasterize_meshes(ndc, f, S, 4e-3, 4)
        return P.sigmoid_alpha_blend(p2f, d, 1e-3).sum() + (bary * (p2f >= 0)[..., None]).sum() * 0.1 + (zbuf * (p2f >= 0)).sum() * 0.1

    def rgb(ndc, col):
        p2f, zbuf, bary, d = P.rasterize_meshes(ndc, f, S, 2e-3, 3)
        return P.softmax_rgb_blend(col, p2f, zbuf, d, sigma=1e-2, gamma=1e-1).pow(2).sum()

    x = ndc0.clone().requires_grad_()
    assert torch.autograd.gradcheck(hard, (x,), eps=1e-7, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(soft, (x,), eps=1e-7, atol=1e-6, rtol=1e-5)
    col = torch.rand(1, S, S, 3, 3, dtype=F64, generator=torch.Generator().manual_seed(1)).requires_grad_()
    assert torch.autograd.gradcheck(rgb, (x, col), eps=1e-7, atol=1e-6, rtol=1e-5)


def test_gradcheck_fragment_consumers_and_mesh_ops():
    S = 8
    v, f, faces0 = _small_mesh(1)
    g = torch.Generator().manual_seed(2)
    ndc = (v * torch.tensor([2.2, 2.2, 1.0], dtype=F64) + torch.tensor([0.013, -0.021, 2.0], dtype=F64))[None]
    p2f, zbuf, bary, d = P.rasterize_meshes(ndc, f, S, 0.0, 1)
    attrs = torch.randn(f.shape[0], 3, 4, generator=g, dtype=F64).requires_grad_()
    b = bary.clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda b_, a_: P.interpolate_face_attributes(p2f, b_, a_), (b, attrs), eps=1e-7, atol=1e-7)
    maps = torch.rand(1, 5, 6, 3, generator=g, dtype=F64).requires_grad_()
    vuv = (torch.rand(6, 2, generator=g, dtype=F64) * 0.8 + 0.1).requires_grad_()
    assert torch.autograd.gradcheck(lambda m_, u_, b_: P.sample_textures_uv(m_, u_, f, p2f, b_, f.shape[0]), (maps, vuv, b), eps=1e-7, atol=1e-6)
    vv = v[None].clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda x: P.verts_normals(x, f), (vv,), eps=1e-7, atol=1e-6)
    off, idx, pairs = _tables(faces0, 6)
    assert torch.autograd.gradcheck(lambda x: P.mesh_laplacian_smoothing_uniform(x, off, idx), (vv,), eps=1e-7, atol=1e-7)
    assert torch.autograd.gradcheck(lambda x: P.mesh_normal_consistency(x, pairs), (vv,), eps=1e-7, atol=1e-7)          # unclamped branch
    small = (v[None] * 0.02).clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda x: P.mesh_normal_consistency(x, pairs) * 1e3, (small,), eps=1e-9, atol=1e-5)  # clamped (torch 1.11) branch
    edges = torch.from_numpy(topology.unique_edges(faces0, 6)[0]).long()
    ref = v[None] + 0.01
    assert torch.autograd.gradcheck(lambda x: H.arap_loss(x, ref, edges), (vv,), eps=1e-7, atol=1e-5)
    R = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))[0][None].requires_grad_()
    T = torch.tensor([[0.01, -0.02, 1.3]], dtype=F64).requires_grad_()
    assert torch.autograd.gradcheck(lambda x, r, t: P.world_to_ndc(x, r, t, 285.7, (32.0, 32.0), 64)[1], (vv, R, T), eps=1e-7, atol=1e-6)
    pos = torch.tensor([[0.4, -0.3, -1.2]], dtype=F64).requires_grad_()
    at = torch.tensor([[0.01, 0.02, 0.03]], dtype=F64).requires_grad_()
    up = torch.tensor([[0.0, 1.0, 0.0]], dtype=F64)
    assert torch.autograd.gradcheck(lambda p_, a_: P.look_at_rotation(p_, a_, up), (pos, at), eps=1e-7, atol=1e-7)
    pts = torch.randn(5, 3, generator=g, dtype=F64).requires_grad_()
    nrm = torch.randn(5, 3, generator=g, dtype=F64).requires_grad_()
    lp = torch.tensor([[0.3, 0.5, -2.0]], dtype=F64).requires_grad_()
    dc = torch.tensor([[0.4, 0.5, 0.6]], dtype=F64)
    assert torch.autograd.gradcheck(lambda p_, n_, l_: P.point_light_diffuse(p_, n_, l_, dc), (pts, nrm, lp), eps=1e-7, atol=1e-7)


def test_gradcheck_harp_ref_ops():
    g = torch.Generator().manual_seed(3)
    pn = torch.randn(1, 2, 2, 1, 3, generator=g, dtype=F64).requires_grad_()
    nm = torch.nn.functional.normalize(torch.randn(1, 2, 2, 1, 3, generator=g, dtype=F64) * 0.3 + torch.tensor([0.0, 0.0, 1.0], dtype=F64), dim=-1).requires_grad_()
    assert torch.autograd.gradcheck(H.apply_normal_map, (pn, nm), eps=1e-7, atol=1e-6)
    cam = torch.tensor([[0.9, 0.02, -0.03]], dtype=F64).requires_grad_()
    lp = torch.tensor([[-0.5, -0.4, -0.6]], dtype=F64).requires_grad_()
    ce = torch.tensor([[0.01, 0.0, 0.02]], dtype=F64).requires_grad_()
    assert torch.autograd.gradcheck(lambda c, l, x: H.process_info_for_shadow(c, l, x, 64, 285.7)[:2] + (H.process_info_for_shadow(c, l, x, 64, 285.7)[3],),
                                    (cam, lp, ce), eps=1e-7, atol=1e-6)
    gt = torch.randn(2, 21, 3, generator=g, dtype=F64) * 40
    pr = (gt / 1000 + torch.randn(2, 21, 3, generator=g, dtype=F64) * 0.004).requires_grad_()
    assert torch.autograd.gradcheck(lambda p_: H.kps_loss(gt, p_), (pr,), eps=1e-8, atol=1e-5)
    tex = torch.rand(1, 6, 5, 3, generator=g, dtype=F64).requires_grad_()
    dist = torch.normal(0, 1.0, (6, 5, 2), generator=g).to(torch.int).long()
    mask = (torch.rand(6, 5, generator=g) > 0.3).double()
    assert torch.autograd.gradcheck(lambda t_: H.albedo_reg(t_, dist, mask), (tex,), eps=1e-7, atol=1e-7)
    nmap = (torch.randn(1, 6, 5, 3, generator=g, dtype=F64) * 0.2 + torch.tensor([0.0, 0.0, 1.0], dtype=F64)).requires_grad_()
    assert torch.autograd.gradcheck(lambda t_: H.normal_reg(t_, dist, mask), (nmap,), eps=1e-7, atol=1e-7)
    # hand layers (fp64 copies of the synthetic models)
    from harp_amd import synth
    model = {k: torch.from_numpy(v).to(F64) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in synth.make_mano_model(seed=0).items()}
    pose = (torch.randn(1, 48, generator=g, dtype=F64) * 0.3).requires_grad_()
    betas = (torch.randn(1, 10, generator=g, dtype=F64) * 0.5).requires_grad_()
    trans = (torch.randn(1, 3, generator=g, dtype=F64) * 0.05).requires_grad_()
    wv = torch.randn(1, 778, 3, generator=g, dtype=F64)
    wj = torch.randn(1, 21, 3, generator=g, dtype=F64)

    def mano(p_, b_, t_):
        vv, jj = H.mano_forward(model, p_, b_, t_)
        return (vv * wv).sum() + (jj * wj).sum()
    assert torch.autograd.gradcheck(mano, (pose, betas, trans), eps=1e-6, atol=1e-4, rtol=1e-5)
    arm = {k: torch.from_numpy(v).to(F64) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in synth.make_smplx_arm_model(seed=0).items()}
    a_betas = (torch.randn(1, 10, generator=g, dtype=F64) * 0.5).requires_grad_()
    go = (torch.randn(1, 3, generator=g, dtype=F64) * 0.3).requires_grad_()
    tr = (torch.randn(1, 3, generator=g, dtype=F64) * 0.02).requires_grad_()
    hp = (torch.randn(1, 45, generator=g, dtype=F64) * 0.3).requires_grad_()
    wp = (torch.randn(1, 3, generator=g, dtype=F64) * 0.3).requires_grad_()
    wv = torch.randn(1, 1026, 3, generator=g, dtype=F64)
    wj = torch.randn(1, 22, 3, generator=g, dtype=F64)

    def armf(*a):
        vv, jj = H.smplxarm_forward(arm, *a)
        return (vv * wv).sum() + (jj * wj).sum()
    assert torch.autograd.gradcheck(armf, (a_betas, go, tr, hp, wp), eps=1e-6, atol=1e-4, rtol=1e-5)
