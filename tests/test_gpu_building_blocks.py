"""-m gpu: the stand-alone building blocks of the fitting step through the raw C ABI against float64 torch on the CPU (values and autograd
gradients), at the tails and edges the whole-step tests never reach: n = 1, n % 256 != 0, sizes past every grid cap (the grid-stride loops
wrap at least twice), non-square maps, clamped normalisations, accumulate / overwrite semantics of every output, and the size checks that
only real buffers can show (a refused call leaves its outputs untouched).  The fused kernels are tested by equality with these blocks
(test_gpu_parity.py), so these pin what the fused kernels compute.

Every bound is stated next to its assertion in float32 units (U = 2^-24, one rounding) with the reason; each case prints its worst error
as a fraction of its bound (<= 1 passes)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                  # unit roundoff of float32


def _L():
    from harp_amd import _lib
    return _lib.lib(), _lib.ptr, _lib.stream, _lib.check


_KEEP = []                      # device copies made inside a call's argument list: alive until the test ends (a freed temporary's block
                                # would be handed to the next copy in the same argument list before the kernel has read it)


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _d(t):
    t = t.contiguous().to(DEV)
    _KEEP.append(t)
    return t


def _f32(x):
    return float(np.float32(x))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _worst(name, err, bound):
    """err, bound: float64 tensors of one shape (bound > 0); prints and asserts max(err / bound) <= 1"""
    err, bound = err.double(), bound.double().expand_as(err)
    assert torch.isfinite(err).all(), name
    r = (err / bound).max().item() if err.numel() else 0.0
    i = int((err / bound).argmax()) if err.numel() else 0
    print(f"[{name}] worst err {err.flatten()[i].item():.3e} at bound {bound.flatten()[i].item():.3e} ({r:.3f} of it)")
    assert r <= 1.0, (name, r, err.flatten()[i].item(), bound.flatten()[i].item())


def _mano_topology():
    from harp_amd import synth
    tpl = synth.load_template("hand")
    return synth.build_topology(tpl["faces0"], tpl["base_verts"].shape[0]), tpl


FIVE = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [1, 5, 2]], np.int32)      # a fan + one face off its rim: 6 vertices


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_subdivide_fwd / bwd
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["mano", "five"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("scale", [1.0, 1e-3])
def test_subdivide_against_float64(mesh, B, scale):
    from harp_amd import ops, synth
    L, p, st, ck = _L()
    if mesh == "mano":
        topo, tpl = _mano_topology()
        dt = ops.DeviceTopology(topo, tpl["verts_uvs"], tpl["faces_uvs"], DEV)
        edges0, sub_off, sub_idx, V0, V, E0 = dt.edges0, dt.sub_off, dt.sub_idx, dt.V0, dt.V, dt.E0
    else:
        topo = synth.build_topology(FIVE, 6)
        edges0, sub_off, sub_idx = (_d(torch.from_numpy(topo[k])) for k in ("edges0", "sub_off", "sub_idx"))
        V0, V, E0 = 6, topo["n_verts"], topo["edges0"].shape[0]
    assert V == V0 + E0
    g = _gen(V0 + B)
    v0 = torch.randn(B, V0, 3, generator=g) * (80.0 if scale != 1.0 else 0.08)          # millimetres when the call scales to metres
    s = _f32(scale)
    e = torch.from_numpy(topo["edges0"]).long()
    v64 = v0.double().requires_grad_()
    ref = torch.cat([s * v64, s * v64[:, e].mean(2)], 1)                                  # SubdivideMeshes of the scaled vertices
    gvs = torch.randn(B, V, 3, generator=g)
    ref.backward(gvs.double())
    vs = torch.full((B, V, 3), float("nan"), device=DEV)
    ck(L.harp_subdivide_fwd(p(_d(v0)), p(edges0), B, V0, E0, s, p(vs), st()), "subdivide_fwd")
    gv0 = torch.full((B, V0, 3), float("nan"), device=DEV)                                # overwritten
    ck(L.harp_subdivide_bwd(p(_d(gvs)), p(sub_off), p(sub_idx), B, V0, V, s, p(gv0), st()), "subdivide_bwd")
    torch.cuda.synchronize()
    # forward: s*v is one rounding; a midpoint (s*a + s*c) * 0.5 is three, each within U of |s a| + |s c|
    a64 = v0.double().abs()
    mag = torch.cat([s * a64, s * (a64[:, e[:, 0]] + a64[:, e[:, 1]])], 1)
    _worst(f"subdivide_fwd {mesh} B={B} s={scale}", (vs.cpu().double() - ref.detach()).abs(), 2 * U * mag + 1e-300)
    # backward: s * (g_i + 0.5 * sum of up to deg children) summed in float32: (deg + 2) roundings of the sum of magnitudes
    deg = int(np.diff(topo["sub_off"]).max())
    absref = torch.autograd.grad(torch.cat([s * v64, s * v64[:, e].mean(2)], 1), v64, gvs.double().abs())[0]
    _worst(f"subdivide_bwd {mesh} B={B} s={scale}", (gv0.cpu().double() - v64.grad).abs(), (deg + 3) * U * absref + 1e-300)


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_vertex_normals_fwd / bwd (+- disp), harp_displace_bwd
# ----------------------------------------------------------------------------------------------------------------------------------
def _edge_mesh():
    """(verts (2,V,3) float32, faces (F,3) int32, components [vertex lists]) of a small mesh with every clamp case of the normal kernels:
    a regular fan; (a) an isolated vertex; (b) a face with two coincident corners (its face normal is exactly 0); (c) one face and its
    opposite-wound copy on integer coordinates (the two face normals cancel exactly: N = 0 at its corners); (d) a face 1e-4 on a side
    (|N| = 1e-8, clearly below the 1e-6 clamp but not zero).  Frame 1 = 2 * frame 0 + 1 (exact on the integer corners)."""
    P = [(0, 0, 1), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0),            # fan 0..4
         (2, 2, 2),                                                          # (a) 5
         (3, 0, 0), (3, 0, 0), (4, 1, 0),                                    # (b) 6, 7 coincident, 8
         (5, 0, 0), (6, 0, 0), (5, 1, 0),                                    # (c) 9, 10, 11
         (0.5, 0.5, 0.5), (0.5 + 1e-4, 0.5, 0.5), (0.5, 0.5 + 1e-4, 0.5)]    # (d) 12, 13, 14
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [6, 7, 8], [9, 10, 11], [9, 11, 10], [12, 13, 14]], np.int32)
    v = torch.tensor(P, dtype=torch.float32)[None]
    v = torch.cat([v, v * 2 + 1], 0)
    comps = [[0, 1, 2, 3, 4], [5], [6, 7, 8], [9, 10, 11], [12, 13, 14]]
    return v, faces, comps


def _vf_tables(faces, V):
    from harp_amd.topology import csr_from_pairs
    off, idx = csr_from_pairs(faces.reshape(-1), np.arange(faces.size), V)
    return _d(torch.from_numpy(off)), _d(torch.from_numpy(idx))


def _normals_case(mesh):
    if mesh == "edge":
        v, faces, comps = _edge_mesh()
        return v, faces, comps
    topo, tpl = _mano_topology()
    e = torch.from_numpy(topo["edges0"]).long()
    base = torch.from_numpy(tpl["base_verts"]).float()
    vs = torch.cat([base, base[e].mean(1)], 0)
    g = _gen(5)
    v = vs[None] + 1e-3 * torch.randn(3, vs.shape[0], 3, generator=g)            # B = 3 frames of the subdivided MANO template
    return v.float().contiguous(), topo["faces"], [list(range(vs.shape[0]))]


def _cond(v64, faces):
    """per vertex sum_f |face normal| / max(|N|, 1e-6): how much cancellation the float32 sum N of the face normals went through"""
    f = torch.from_numpy(faces).long()
    fv = v64[:, f]
    fn = torch.cross(fv[:, :, 2] - fv[:, :, 1], fv[:, :, 0] - fv[:, :, 1], dim=-1)
    s = torch.zeros(v64.shape[:2], dtype=torch.float64)
    N = torch.zeros_like(v64)
    for k in range(3):
        s = s.index_add(1, f[:, k], fn.norm(dim=-1))
        N = N.index_add(1, f[:, k], fn)
    return s / N.norm(dim=-1).clamp_min(1e-6), N.norm(dim=-1)


@pytest.mark.parametrize("mesh", ["edge", "mano"])
@pytest.mark.parametrize("with_disp", [False, True])
def test_vertex_normals_against_float64(mesh, with_disp):
    from oracle import p3d_like as P
    L, p, st, ck = _L()
    v, faces_np, comps = _normals_case(mesh)
    B, V = v.shape[:2]
    faces = torch.from_numpy(faces_np).long()
    vf_off, vf_idx = _vf_tables(faces_np, V)
    faces_d = _d(torch.from_numpy(faces_np))
    g = _gen(V + int(with_disp))
    disp = (torch.randn(V, generator=g) * 1e-3).float()
    gn = torch.randn(B, V, 3, generator=g)
    G0 = torch.randn(B, V, 3, generator=g)                                     # g_v ACCUMULATES into what the buffer holds
    # ---- float64 reference
    v64 = v.double().requires_grad_()
    n_ref = P.verts_normals(v64, faces)
    out = v64 + n_ref * disp.double()[None, :, None] if with_disp else n_ref
    g_out = gn.double()
    out.backward(g_out)
    # ---- device
    n = torch.full((B, V, 3), float("nan"), device=DEV)
    il = torch.full((B, V), float("nan"), device=DEV)
    vd = torch.full((B, V, 3), float("nan"), device=DEV) if with_disp else None
    disp_d = _d(disp) if with_disp else None
    vv = _d(v)
    ck(L.harp_vertex_normals_fwd(p(vv), p(faces_d), p(vf_off), p(vf_idx), B, V, p(n), p(il), p(disp_d), p(vd), st()), "normals_fwd")
    tmp = torch.empty(B, V, 3, device=DEV)
    gv = _d(G0)
    if with_disp:                         # vd = v + n * disp: g_v gets g_vd directly, g_n = g_vd * disp through harp_displace_bwd
        gvd = _d(gn)
        g_n = torch.full((B, V, 3), float("nan"), device=DEV)
        g_disp = torch.zeros(V, device=DEV)
        ck(L.harp_displace_bwd(p(gvd), p(n), p(disp_d), B, V, p(g_n), p(g_disp), st()), "displace_bwd")
        gv += gvd
    else:
        g_n = _d(gn)
    ck(L.harp_vertex_normals_bwd(p(vv), p(faces_d), p(vf_off), p(vf_idx), B, V, p(n), p(il), p(g_n), p(tmp), p(gv), st()), "normals_bwd")
    torch.cuda.synchronize()
    cond, Nlen = _cond(v.double(), faces_np)
    clamped = Nlen <= 1e-6
    tag = f"normals {mesh} disp={with_disp}"
    # the kernel's clamp flag: inv_len = 0 exactly where |N| <= 1e-6 (cases a-d), 1/|N| elsewhere
    assert torch.equal(il.cpu() == 0, clamped), tag
    if mesh == "edge":
        assert clamped[:, 5:].all() and not clamped[:, :5].any()
        assert (Nlen[:, 12:] > 1e-9).all() and (Nlen[:, 6:12] == 0).all()   # (d) non-zero below the clamp; (b), (c) exactly zero
    # normals: the float32 sum N of the face normals carries ~ (3 deg + 4) U of sum_f |fn|, relative to |N| that is cond * (3 deg + 4) U
    # (clamped: n = N 1e6, the same error times 1e6 = cond); + 4 U for the normalisation itself
    deg = int(np.bincount(faces_np.reshape(-1), minlength=V).max())
    nb = (((3 * deg + 8) * cond + 4) * U)[..., None]
    if mesh == "edge":
        assert (n[:, 6:12] == 0).all()          # N exactly 0 at (b) and (c): n = 0 exactly (the bound there is meaningless: cond = 2e6 at (c))
    _worst(tag + " n", (n.cpu().double() - n_ref.detach()).abs(), nb + 1e-300)
    if with_disp:
        want = (v64 + n_ref * disp.double()[None, :, None]).detach()
        # v + n d: two roundings of |v| + |n d| on top of n's own error times |d|
        _worst(tag + " vd", (vd.cpu().double() - want).abs(), 2 * U * (v.double().abs() + (n_ref.detach() * disp.double()[None, :, None]).abs())
               + nb * disp.double().abs()[None, :, None] + 1e-300)
        # g_n = g_vd * d: one rounding; g_disp = sum over frames and channels of g_vd . n (atomics into a zeroed buffer)
        _worst(tag + " g_n", (g_n.cpu().double() - gn.double() * disp.double()[None, :, None]).abs(),
               U * (gn.double() * disp.double()[None, :, None]).abs() + 1e-300)
        want_gd = (gn.double() * n_ref.detach()).sum((0, 2))
        _worst(tag + " g_disp", (g_disp.cpu().double() - want_gd).abs(),
               (3 * B + 2) * U * (gn.double().abs() * n_ref.detach().abs()).sum((0, 2)) + (gn.double().abs() * nb).sum((0, 2)) + 1e-300)
    # g_v: every face adds cross products of its edges with the sum of its corners' g_N, where |g_N| <= |g_n| / max(|N|, 1e-6) (exactly
    # 1e6 |g_n| under the clamp).  Per vertex, mag = sum over its faces of that sum times |A| + |B|; the float32 chain rule carries ~16
    # roundings of mag, plus what the error of n itself (cond x (3 deg + 8) U, unclamped vertices only) does to g_N.  At (c) the two
    # windings' terms, ~1e6 each, cancel exactly in float64 and to within those roundings in float32.
    f = torch.from_numpy(faces_np).long()
    v64d = v.double()
    fv = v64d[:, f]
    A, Bv = fv[:, :, 2] - fv[:, :, 1], fv[:, :, 0] - fv[:, :, 1]
    g_n_in = gn.double() * (disp.double()[None, :, None] if with_disp else 1.0)
    gmag = g_n_in.norm(dim=-1) / Nlen.clamp_min(1e-6)
    mag_f = gmag[:, f].sum(-1) * (A.norm(dim=-1) + Bv.norm(dim=-1))
    mag = torch.zeros(B, V, dtype=torch.float64)
    for k in range(3):
        mag = mag.index_add(1, f[:, k], mag_f)
    cond_nc = torch.where(clamped, torch.zeros_like(cond), cond)
    got = gv.cpu().double() - G0.double()
    want = v64.grad
    for c in comps:
        kc = 16 + (3 * deg + 8) * cond_nc[:, c].max().item()
        _worst(tag + f" g_v piece {c[0]}..{c[-1]}", (got[:, c] - want[:, c]).abs(),
               kc * U * mag[:, c, None] + 2 * U * (G0.double()[:, c].abs() + want[:, c].abs()) + 1e-300)
    if mesh == "edge" and not with_disp:
        # the isolated vertex has no gradient; the clamped branch gives exactly 1e6 g_N to the corners of (b) -- a non-zero gradient
        assert (got[:, 5] == 0).all() and want[:, 6:9].abs().max() > 1e4


def test_normals_and_displace_refuse_bad_arguments_untouched():
    """NULL vertex -> face tables in the backward and B = 0 in harp_displace_bwd (whose grid depends on V alone) refuse before launching"""
    L, p, st, _ = _L()
    v, faces_np, _ = _edge_mesh()
    B, V = v.shape[:2]
    vf_off, vf_idx = _vf_tables(faces_np, V)
    bufs = [torch.full((B, V, 3), 3.0, device=DEV) for _ in range(4)]
    il = torch.ones(B, V, device=DEV)
    fd, vv = _d(torch.from_numpy(faces_np)), _d(v)
    assert L.harp_vertex_normals_bwd(p(vv), p(fd), None, p(vf_idx), B, V, p(bufs[0]), p(il), p(bufs[1]), p(bufs[2]), p(bufs[3]), st()) == 1
    assert L.harp_vertex_normals_bwd(p(vv), p(fd), p(vf_off), None, B, V, p(bufs[0]), p(il), p(bufs[1]), p(bufs[2]), p(bufs[3]), st()) == 1
    disp, g_disp = torch.ones(V, device=DEV), torch.full((V,), 5.0, device=DEV)
    assert L.harp_displace_bwd(p(bufs[0]), p(bufs[1]), p(disp), 0, V, p(bufs[2]), p(g_disp), st()) == 1
    so, si = torch.zeros(V + 1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert L.harp_subdivide_bwd(p(bufs[0]), p(so), p(si), 1, V, V - 1, 1.0, p(bufs[3]), st()) == 1      # V < V0
    torch.cuda.synchronize()
    assert all(bool((b == 3.0).all()) for b in bufs) and bool((g_disp == 5.0).all())


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_project_fwd / bwd
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outs", ["none", "both", "R_only"])
def test_project_against_float64(outs):
    from oracle import p3d_like as P
    L, p, st, ck = _L()
    B, V, S, focal = 2, 4083, 333, _f32(611.3)
    pp = (_f32(150.25), _f32(190.75))                                   # off the centre (166.5) in both axes
    g = _gen(7)
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, dtype=torch.float64))[0].float()
    T = torch.tensor([[0.05, -0.03, 0.6], [-0.02, 0.04, 0.55]])
    v = (torch.rand(B, V, 3, generator=g) - 0.5) * 0.4                  # |v R| < 0.35: view z in [0.2, 0.95]
    v64, R64, T64 = v.double().requires_grad_(), R.double().requires_grad_(), T.double().requires_grad_()
    view, ndc_ref = P.world_to_ndc(v64, R64, T64, focal, pp, S)
    view.retain_grad()
    assert view[..., 2].min() > 0.15
    gndc = torch.randn(B, V, 3, generator=g)
    (ndc_ref * gndc.double()).sum().backward()
    ndc = torch.full((B, V, 3), float("nan"), device=DEV)
    vd, Rd, Td = _d(v), _d(R), _d(T)
    ck(L.harp_project_fwd(p(vd), p(Rd), p(Td), B, V, focal, pp[0], pp[1], S, p(ndc), st()), "project_fwd")
    G0v, G0R, G0T = (torch.randn(*s, generator=g) for s in ((B, V, 3), (B, 3, 3), (B, 3)))
    gv, gR, gT = _d(G0v), _d(G0R), _d(G0T)
    ck(L.harp_project_bwd(p(vd), p(Rd), p(Td), p(_d(gndc)), B, V, focal, S, p(gv), p(gR) if outs != "none" else None,
                          p(gT) if outs == "both" else None, st()), "project_bwd")
    torch.cuda.synchronize()
    # forward: X = v . R[:, 0] + T (3 roundings of the sum of |terms|), focal X / Z + px - 2 px + S/2 (4 more), / (S/2)
    absX = torch.bmm(v.double().abs(), R.double().abs()) + T.double().abs()[:, None]
    Z = view[..., 2].detach()
    half = S / 2.0
    bxy = 8 * U * (focal * absX[..., :2] / Z[..., None] * (1 + absX[..., 2:] / Z[..., None]) + 2 * torch.tensor(pp, dtype=torch.float64) + half) / half
    bz = 4 * U * absX[..., 2:]
    _worst(f"project_fwd S={S}", (ndc.cpu().double() - ndc_ref.detach()).abs(), torch.cat([bxy, bz], -1))
    # g_v = R (gX, gY, gZ): a few roundings of each view-space gradient, which carry the cancellation of gZ = g_z - (gX X + gY Y) / Z
    gview = view.grad
    absgv = gview.abs() + torch.cat([torch.zeros_like(gview[..., :2]), (gview[..., :2].abs() * absX[..., :2]).sum(-1, keepdim=True) / Z[..., None]], -1)
    bgv = 8 * U * torch.bmm(absgv, R.double().abs().transpose(1, 2)) + U * G0v.double().abs()
    _worst(f"project_bwd g_v ({outs})", (gv.cpu().double() - G0v.double() - v64.grad).abs(), bgv + 1e-300)
    # g_R / g_T: float32 sums over V vertices (8-level tree in a workgroup, V / 256 atomics per frame) of terms that carry 8 U each
    k = 8 + 8 + math.ceil(V / 256)
    bR = k * U * torch.bmm(v.double().abs().transpose(1, 2), absgv) + U * G0R.double().abs()
    bT = k * U * absgv.sum(1) + U * G0T.double().abs()
    if outs != "none":
        _worst(f"project_bwd g_R ({outs})", (gR.cpu().double() - G0R.double() - R64.grad).abs(), bR)
    else:
        assert torch.equal(gR.cpu(), G0R)
    if outs == "both":
        _worst(f"project_bwd g_T ({outs})", (gT.cpu().double() - G0T.double() - T64.grad).abs(), bT)
    else:
        assert torch.equal(gT.cpu(), G0T)


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_centroid, harp_scale
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 255, 257, 4083])
def test_centroid_against_float64(V):
    L, p, st, ck = _L()
    B = 3
    v = torch.randn(B, V, 3, generator=_gen(V)) * 0.1 + 0.3
    c = torch.full((B, 3), float("nan"), device=DEV)
    ck(L.harp_centroid(p(_d(v)), B, V, p(c), st()), "centroid")
    torch.cuda.synchronize()
    # ceil(V / 256) sequential adds per lane, an 8-level tree, the division: that many roundings of sum |v| / V
    _worst(f"centroid V={V}", (c.cpu().double() - v.double().mean(1)).abs(), (math.ceil(V / 256) + 10) * U * v.double().abs().mean(1))
    if V == 1:
        for bad in (0, -1):                                               # V <= 0 refused before the launch (B workgroups would run)
            c2 = torch.full((B, 3), 7.0, device=DEV)
            assert L.harp_centroid(p(_d(v)), B, bad, p(c2), st()) == 1
            torch.cuda.synchronize()
            assert (c2 == 7.0).all()


@pytest.mark.parametrize("n", [1, 255, 257, 12249, 1000003])
def test_scale_is_the_rounded_product(n):
    L, p, st, ck = _L()
    x = torch.randn(n, generator=_gen(n)) * 100
    y = torch.full((n,), float("nan"), device=DEV)
    s = _f32(1e-3)
    ck(L.harp_scale(p(_d(x)), s, n, p(y), st()), "scale")
    torch.cuda.synchronize()
    # exact: one correctly rounded float32 product per element, the same bits as torch's float32 product
    assert torch.equal(y.cpu(), x * torch.tensor(s, dtype=torch.float32)), n
    _worst(f"scale n={n}", (y.cpu().double() - x.double() * s).abs(), U * (x.double() * s).abs() + 1e-300)


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_sum_squares, harp_mse
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 16385, 64 * 256 * 3 + 5])
@pytest.mark.parametrize("weighted", [True, False])
def test_sum_squares_against_float64(n, weighted):
    L, p, st, ck = _L()
    g = _gen(n)
    x = torch.randn(n, generator=g)
    G0 = torch.randn(n, generator=g)
    w = _f32(0.7)
    xd = _d(x)
    x64 = x.double().requires_grad_()
    ref = (x64 ** 2).sum()
    ref.backward()
    loss = torch.full((1,), 1.25, device=DEV)                             # accumulates
    gd = _d(G0)                                                           # accumulates w * d/dx
    wd = _d(torch.tensor([w]))
    ck(L.harp_sum_squares(p(xd), n, p(wd) if weighted else None, p(loss), p(gd), st()), "sum_squares")
    torch.cuda.synchronize()
    blocks = min((n + 255) // 256, 64)
    # positive terms: ceil(n / 16384) per lane, 8 tree levels, `blocks` atomics, the prefill: that many roundings of the total
    k = math.ceil(n / (64 * 256)) + 8 + blocks + 2
    tot = 1.25 + ref.item()
    _worst(f"sum_squares n={n} loss", torch.tensor([abs(loss.item() - tot)]), torch.tensor([k * U * tot]))
    if weighted:
        # (2 w) x: one rounding, then the atomic add onto the prefill: one more
        _worst(f"sum_squares n={n} grad", (gd.cpu().double() - G0.double() - w * x64.grad).abs(),
               U * (2 * (w * x64.grad).abs() + (G0.double() + w * x64.grad).abs()) + 1e-300)
    else:
        assert torch.equal(gd.cpu(), G0)                                  # no weight: the gradient is not touched


@pytest.mark.parametrize("n", [1, 262145, 1000003])
def test_mse_against_float64(n):
    L, p, st, ck = _L()
    g = _gen(n + 1)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    x64 = x.double().requires_grad_()
    ref = torch.nn.MSELoss()(x64, y.double())
    ref.backward()
    loss = torch.full((1,), 0.5, device=DEV)                              # accumulates
    gx = torch.full((n,), float("nan"), device=DEV)                       # overwritten: every element must be written once
    ck(L.harp_mse(p(_d(x)), p(_d(y)), n, p(loss), p(gx), st()), "mse")
    torch.cuda.synchronize()
    blocks = min((n + 255) // 256, 1024)
    k = math.ceil(n / (1024 * 256)) + 8 + blocks + 3
    tot = 0.5 + ref.item()
    _worst(f"mse n={n} loss", torch.tensor([abs(loss.item() - tot)]), torch.tensor([k * U * tot]))
    # x - y (one rounding of the difference), * 2 exact, * fl(1/n): three roundings of the element's own gradient
    _worst(f"mse n={n} grad", (gx.cpu().double() - x64.grad).abs(), 3 * U * x64.grad.abs() + 1e-300)


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_texture_smooth_reg, harp_close_to_z_reg
# ----------------------------------------------------------------------------------------------------------------------------------
HW = [(72, 100), (100, 72), (33, 129), (129, 33), (257, 1031)]          # the last: H W = 264 967 > 2 x 512 x 256 texels (wraps twice)


def _offsets(H, W, g):
    """int(N(0, 2)) per texel and axis like loss/texture_reg.py, plus 3 % far draws that clamp at all four borders"""
    d = (torch.randn(H, W, 2, generator=g) * 2.0).to(torch.int32)
    far = torch.rand(H, W, generator=g) < 0.03
    big = torch.randint(-2 * max(H, W), 2 * max(H, W) + 1, (H, W, 2), generator=g, dtype=torch.int32)
    d[far] = big[far]
    gx, gy = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    tx, ty = gx + d[..., 0], gy + d[..., 1]
    assert (tx < 0).any() and (tx > H - 1).any() and (ty < 0).any() and (ty > W - 1).any()
    return d


@pytest.mark.parametrize("hw", HW)
@pytest.mark.parametrize("masked", [False, True])
def test_texture_smooth_reg_against_float64(hw, masked):
    from oracle import harp_ref as R
    L, p, st, ck = _L()
    H, W = hw
    g = _gen(H * 7 + W + int(masked))
    tex = torch.rand(H, W, 3, generator=g)
    dist = _offsets(H, W, g)
    mask = None
    if masked:                                                            # fractional, 30 % exactly zero
        mask = torch.rand(H, W, generator=g)
        mask[torch.rand(H, W, generator=g) < 0.3] = 0.0
    w = _f32(0.9)
    t64 = tex.double()[None].requires_grad_()
    ref = R._smooth_reg(t64, dist.long(), None if mask is None else mask.double())
    (w * ref).backward()
    k = w / (3.0 * H * W)
    # The inputs are float32 numbers, and the float32 difference of two of them has the exact sign (zero only when they are equal): the
    # sign of every |t[p] - t[j(p)]| is decided, so no texel has to be left out.  Ties (j(p) == p after the clamp, or equal values)
    # give 0 on both sides.
    G0 = torch.randn(H, W, 3, generator=g) * k                            # g_tex accumulates (atomics)
    loss = torch.full((1,), 0.3, device=DEV)
    gt = _d(G0)
    ck(L.harp_texture_smooth_reg(p(_d(tex)), p(_d(dist)), p(_d(mask)) if masked else None, H, W, p(_d(torch.tensor([w]))),
                                 p(loss), p(gt), st()), "texture_smooth_reg")
    torch.cuda.synchronize()
    tag = f"texture_smooth_reg {H}x{W} mask={masked}"
    blocks = min((H * W + 255) // 256, 512)
    nk = math.ceil(H * W / (512 * 256)) + 8 + blocks + 4
    tot = 0.3 + ref.item()
    _worst(tag + " loss", torch.tensor([abs(loss.item() - tot)]), torch.tensor([nk * U * tot]))
    # each texel's gradient is its own term and one from every source that targets it (n_t terms of k m, each k m rounded thrice):
    # (n_t + 4) roundings of n_t k, plus the prefill's
    gx_, gy_ = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    j = (gx_ + dist[..., 0]).clamp(0, H - 1) * W + (gy_ + dist[..., 1]).clamp(0, W - 1)
    n_t = torch.bincount(j.flatten(), minlength=H * W).view(H, W).double() + 1
    bound = ((n_t + 4) * n_t * U * k)[..., None] + 2 * U * (G0.double().abs() + t64.grad[0].abs())
    _worst(tag + " grad", (gt.cpu().double() - G0.double() - t64.grad[0]).abs(), bound + 1e-300)


@pytest.mark.parametrize("hw", HW)
def test_close_to_z_reg_against_float64(hw):
    from oracle import harp_ref as R
    L, p, st, ck = _L()
    H, W = hw
    g = _gen(H * 5 + W)
    nm = F.normalize(torch.randn(H, W, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    nm[3] = torch.tensor([0.0, 0.0, 1.0])                                 # a row whose three norms are exactly 0: no gradient there
    nm[5, :, 0] = 0.0                                                     # one (row, channel) norm exactly 0
    scale, w = _f32(0.2), _f32(0.1)
    n64 = nm.double()[None].requires_grad_()
    ref = scale * R.close_to_z_reg(n64)
    (w * ref).backward()
    G0 = torch.randn(H, W, 3, generator=g) * 1e-4                         # g accumulates
    loss = torch.full((1,), 0.3, device=DEV)
    gd = _d(G0)
    ck(L.harp_close_to_z_reg(p(_d(nm)), H, W, scale, p(_d(torch.tensor([w]))), p(loss), p(gd), st()), "close_to_z")
    torch.cuda.synchronize()
    tag = f"close_to_z_reg {H}x{W}"
    # per (row, channel): a sum of W squares (ceil(W/256) per lane + 8 levels), the root, then H atomics of positive terms
    kl = math.ceil(W / 256) + 8 + H + 6
    tot = 0.3 + ref.item()
    _worst(tag + " loss", torch.tensor([abs(loss.item() - tot)]), torch.tensor([kl * U * tot]))
    # g = w s / (9 H) * (nm - z) / norm: the norm's (ceil(W/256) + 10) roundings and 4 more
    kg = math.ceil(W / 256) + 14
    _worst(tag + " grad", (gd.cpu().double() - G0.double() - n64.grad[0]).abs(), kg * U * n64.grad[0].abs() + 2 * U * G0.double().abs() + 1e-300)
    assert torch.equal(gd[3].cpu(), G0[3]) and torch.equal(gd[5, :, 0].cpu(), G0[5, :, 0])
    for Hb, Wb in [(H, 0), (H, -1), (-1, W)]:                              # refused with real buffers (H workgroups would run for W <= 0)
        l2 = torch.full((1,), 0.3, device=DEV)
        assert L.harp_close_to_z_reg(p(_d(nm)), Hb, Wb, scale, None, p(l2), None, st()) == 1
        torch.cuda.synchronize()
        assert l2.item() == _f32(0.3)


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_normalize3_fwd / bwd
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_normalize3_against_float64(n):
    L, p, st, ck = _L()
    g = _gen(n + 3)
    x = torch.randn(n, 3, generator=g)
    unit = F.normalize(torch.randn(8, 3, generator=g), dim=-1)
    special = torch.cat([torch.zeros(1, 3), unit[:2] * 1e-13, unit[2:4] * 4e-13, unit[4:6] * 3e-12, unit[6:8] * 1e-11])   # 0, below, above the clamp
    m = min(n, special.shape[0])
    x[:m] = special[:m] if n > 1 else unit[:1] * 1e-13
    gy = torch.randn(n, 3, generator=g)
    G0 = torch.randn(n, 3, generator=g)
    x64 = x.double().requires_grad_()
    y_ref = F.normalize(x64, dim=-1)
    y_ref.backward(gy.double())
    y = torch.full((n, 3), float("nan"), device=DEV)
    xd = _d(x)
    ck(L.harp_normalize3_fwd(p(xd), n, p(y), st()), "normalize3_fwd")
    gx = _d(G0)                                                           # accumulates
    ck(L.harp_normalize3_bwd(p(xd), p(_d(gy)), n, p(gx), st()), "normalize3_bwd")
    torch.cuda.synchronize()
    nx = x.double().norm(dim=-1, keepdim=True)
    # y = x / max(|x|, 1e-12f): a fused sum of squares, the root, the reciprocal, the product: 4 roundings of |y| (<= 1), and the clamp
    # constant 1e-12f is 1e-12 (1 - 2e-8)
    _worst(f"normalize3_fwd n={n}", (y.cpu().double() - y_ref.detach()).abs(), 4 * U * (nx / nx.clamp_min(1e-12)) + 1e-300)
    # gx = (g - n (n . g)) / |x| (or g 1e12 under the clamp): 8 roundings of |g| / max(|x|, 1e-12), one of the prefill
    _worst(f"normalize3_bwd n={n}", (gx.cpu().double() - G0.double() - x64.grad).abs(),
           8 * U * gy.double().abs().sum(-1, keepdim=True) / nx.clamp_min(1e-12) + 2 * U * G0.double().abs())


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_kps_loss, harp_image_l1
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NJp", [21, 22])
@pytest.mark.parametrize("B,fid", [(1, None), (5, [2, 2, 0, 3, 2])])
def test_kps_loss_against_float64(NJp, B, fid):
    from oracle import harp_ref as R
    L, p, st, ck = _L()
    g = _gen(NJp * 10 + B)
    T = 4
    gt = torch.randn(T, 21, 3, generator=g) * 60.0                        # millimetres
    f = torch.tensor(fid if fid is not None else list(range(B)))
    pred = torch.randn(B, NJp, 3, generator=g) * 0.06
    pred[:, :21] = gt[f] / 1000.0 + torch.randn(B, 21, 3, generator=g) * 5e-3          # metres, 5 mm off the targets
    w = _f32(0.6)
    p64 = pred.double().requires_grad_()
    ref = R.kps_loss(gt[f].double(), p64, use_arm=NJp > 21)
    (w * ref).backward()
    G0 = torch.randn(B, NJp, 3, generator=g) * 1e-2                       # g_pred accumulates
    loss = torch.full((1,), 0.2, device=DEV)
    gp = _d(G0)
    fd = _d(f.int()) if fid is not None else None
    ck(L.harp_kps_loss(p(_d(gt)), p(fd), p(_d(pred)), B, NJp, p(_d(torch.tensor([w]))), p(loss), p(gp), st()), "kps")
    torch.cuda.synchronize()
    tag = f"kps_loss NJp={NJp} B={B}"
    # d = (gt_j - gt_0) - 1000 (pred_j - pred_0) carries 5 U of the magnitudes it cancels (~20x |d| here)
    gg, pp = gt[f].double(), pred[:, :21].double()
    mag = gg.abs() + gg[:, :1].abs() + 1000 * (pp.abs() + pp[:, :1].abs())
    d = (gg - gg[:, :1]) - 1000 * (pp - pp[:, :1])
    dd = 5 * U * mag
    bl = ((2 * d.abs() * dd).sum() / 1e4 + (ref.item() * 21 * B) * 12 * U) / (21 * B) + (12 + B) * U * (0.2 + ref.item())
    _worst(tag + " loss", torch.tensor([abs(loss.item() - 0.2 - ref.item())]), torch.tensor([bl.item()]))
    kk = w * 0.2 / (21 * B)
    bg = kk * (dd.sum((1, 2), keepdim=True) + 30 * U * d.abs().sum((1, 2), keepdim=True)) + 2 * U * (G0[:, :21].double().abs() + p64.grad[:, :21].abs())
    _worst(tag + " grad", (gp[:, :21].cpu().double() - G0[:, :21].double() - p64.grad[:, :21]).abs(), bg + 1e-300)
    if NJp > 21:
        assert torch.equal(gp[:, 21:].cpu(), G0[:, 21:])                   # the arm's extra joints take no part


@pytest.mark.parametrize("B,T,fid,S,C,masked", [(3, 4, [1, 1, 3], 37, 3, False), (2, 3, [2, 2], 129, 1, True), (3, 4, [0, 3, 3], 129, 3, True),
                                                 (2, 2, None, 257, 1, False), (1, 1, None, 1, 1, True)])
def test_image_l1_against_float64(B, T, fid, S, C, masked):
    L, p, st, ck = _L()
    g = _gen(S * 3 + C + B)
    npf = S * S * C                                                       # 4107 | 16641 | 49923 | 66049 | 1: off the 256 grid, past 64 x 256
    pred, tgt = torch.rand(B, npf, generator=g), torch.rand(T, npf, generator=g)
    f = torch.tensor(fid if fid is not None else list(range(B)))
    mask = None
    if masked:
        mask = torch.rand(T, S * S, generator=g)
        mask[torch.rand(T, S * S, generator=g) < 0.3] = 0.0
    w = _f32(0.8)
    p64 = pred.double().requires_grad_()
    m64 = mask.double()[f].repeat_interleave(C, 1) if masked else torch.ones(B, npf, dtype=torch.float64)
    ref = torch.nn.L1Loss()(p64 * m64, tgt.double()[f] * m64)
    (w * ref).backward()
    loss = torch.full((1,), 0.1, device=DEV)
    gp = torch.full((B, npf), float("nan"), device=DEV)                  # overwritten
    pd, td = _d(pred), _d(tgt)
    ck(L.harp_image_l1(p(pd), p(td), p(_d(mask)) if masked else None, p(_d(f.int())) if fid is not None else None, B, npf, C,
                       p(_d(torch.tensor([w]))), p(loss), p(gp), st()), "image_l1")
    torch.cuda.synchronize()
    tag = f"image_l1 B={B} S={S} C={C} mask={masked}"
    pm, tm = pred.double() * m64, tgt.double()[f] * m64
    undecided = (pm - tm).abs() <= 2 * U * (pm.abs() + tm.abs())          # fl(p m) - fl(t m) may take either sign (or 0) here
    undecided &= (pm != tm)
    print(f"[{tag}] undecided signs: {int(undecided.sum())} of {undecided.numel()}")
    assert undecided.float().mean() < 1e-4
    cnt = B * npf
    k = math.ceil(npf / (64 * 256)) + 8 + 64 * B + 3
    bl = k * U * (0.1 + ref.item()) + 3 * U * (pm.abs() + tm.abs()).sum().item() / cnt
    _worst(tag + " loss", torch.tensor([abs(loss.item() - 0.1 - ref.item())]), torch.tensor([bl]))
    # w / count * sign * m: fl(1/count), fl(w * that), * m: 3 roundings
    err = (gp.cpu().double() - p64.grad).abs()
    err[undecided] = 0.0
    _worst(tag + " grad", err, 3 * U * p64.grad.abs() + 1e-300)
    l2 = torch.full((1,), 0.1, device=DEV)                               # C <= 0 and n_per_frame % C != 0: refused before the launch
    assert L.harp_image_l1(p(pd), p(td), None, None, 1, npf, 0, None, p(l2), None, st()) == 1
    assert L.harp_image_l1(p(pd), p(td), None, None, 1, min(npf, 4), 3, None, p(l2), None, st()) == 1
    torch.cuda.synchronize()
    assert l2.item() == _f32(0.1)


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_adam_step (and harp_adam_tick + harp_adam_apply)
# ----------------------------------------------------------------------------------------------------------------------------------
def test_adam_step_against_torch_adam_float64():
    """10 steps on n = 1 100 003 elements (past the 2048 x 256 grid cap: the grid-stride loop wraps twice), grad_scale 0.37, beta2 0.999
    from step 1 (where bias correction 2 is 1e-3 .. 1e-2 and matters).  The reference is torch.optim.Adam in float64 with the float32
    values the kernel receives (lr, betas and eps rounded to float32), on grad * grad_scale.  harp_adam_tick + harp_adam_apply derive the
    same bias corrections (host double pow vs the device's: the float32 results agree exactly, checked every step) but do NOT give the same
    bits: the compiler contracts the two kernels' identical source differently (adam_kernel fuses grad * grad_scale into the exp_avg
    lerp, fma(g, gs, -m); adam_dev_kernel is compiled without contraction, to round like harp_adam_apply2), so both are held to the float64 bounds."""
    L, p, st, ck = _L()
    n, steps = 1100003, 10
    lr, b1, b2, eps, gs = _f32(1e-2), _f32(0.9), _f32(0.999), _f32(1e-8), _f32(0.37)
    g = _gen(11)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 4 - 3) for _ in range(steps)]
    # ---- reference
    ref = p0.double().clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=lr, betas=(b1, b2), eps=eps)
    for t in range(steps):
        ref.grad = grads[t].double() * gs
        opt.step()
    st_ = opt.state[ref]
    # ---- harp_adam_step (host bias corrections)
    P1, M1, V1 = _d(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    # ---- harp_adam_tick + harp_adam_apply (device-resident hyper-parameters)
    P2, M2, V2 = _d(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    raw = bytearray(32)                                                   # harp_adam_hyper: lr b1 b2 eps grad_scale | step | step_size inv_sqrt_bc2
    np.frombuffer(raw, np.float32, 5, 0)[:] = [lr, b1, b2, eps, gs]
    hyper = torch.frombuffer(raw, dtype=torch.uint8).clone().to(DEV)
    for t in range(1, steps + 1):
        gd = _d(grads[t - 1])
        ck(L.harp_adam_step(p(P1), p(gd), p(M1), p(V1), n, lr, b1, b2, eps, t, gs, st()), "adam_step")
        ck(L.harp_adam_tick(p(hyper), 1, st()), "adam_tick")
        ck(L.harp_adam_apply(p(P2), p(gd), p(M2), p(V2), n, p(hyper), st()), "adam_apply")
        torch.cuda.synchronize()
        h = hyper.cpu().numpy()
        assert int(h[20:24].view(np.int32)[0]) == t
        ss, isb = h[24:32].view(np.float32)
        assert ss == np.float32(np.float64(lr) / (1.0 - np.float64(b1) ** t)) and isb == np.float32(1.0 / math.sqrt(1.0 - np.float64(b2) ** t)), (t, ss, isb)
    gabs = torch.stack([gg.double().abs() * gs for gg in grads]).max(0).values
    for (Pk, Mk, Vk), how in (((P1, M1, V1), "adam_step"), ((P2, M2, V2), "tick+apply")):
        # p: each step rounds p (U |p|) and an update of lr |m^ / (sqrt(v^) + eps)| (<= ~3 lr) computed with ~30 roundings
        _worst(f"{how} p", (Pk.cpu().double() - ref.detach()).abs(), U * (steps * 2 * ref.detach().abs() + steps * 30 * 3 * lr))
        # m: a lerp per step (3 roundings of |g| + |m|); v: positive terms (4 roundings per step)
        _worst(f"{how} m", (Mk.cpu().double() - st_["exp_avg"]).abs(), U * steps * 8 * gabs + 1e-300)
        _worst(f"{how} v", (Vk.cpu().double() - st_["exp_avg_sq"]).abs(), U * steps * 6 * st_["exp_avg_sq"] + 1e-300)
    print(f"[adam_step vs tick+apply] elements that differ: p {int((P1 != P2).sum())}, m {int((M1 != M2).sum())}, v {int((V1 != V2).sum())} of {n}")
    # n == 0 is refused (the grid would be empty)
    assert L.harp_adam_step(p(P1), p(gd), p(M1), p(V1), 0, lr, b1, b2, eps, 1, gs, st()) == 1


# ----------------------------------------------------------------------------------------------------------------------------------
# harp_depth_bwd
# ----------------------------------------------------------------------------------------------------------------------------------
def test_depth_bwd_against_zbuf_autograd():
    """harp_depth_bwd (the backward of ops.depth_raster) against autograd through oracle/p3d_like.rasterize_meshes' zbuf, K = 1, on a
    scene of 14 well-shaped triangles per frame that overlap in depth layers 0.4 apart (no depth ties: each triangle's depth varies by
    < 0.1 over it).  Pixels whose coverage is not decided at float32 precision (return_ambiguous) get no gradient."""
    from harp_amd import ops
    from oracle import p3d_like as P
    L, p, st, ck = _L()
    B, S, nf = 2, 67, 14
    g = _gen(23)
    ctr = (torch.rand(B, nf, 1, 2, generator=g) - 0.5) * 1.4
    ang = torch.rand(B, nf, 1, generator=g) * 6.283 + torch.tensor([0.0, 2.1, 4.2])
    rad = 0.25 + 0.2 * torch.rand(B, nf, 3, generator=g)
    xy = ctr + torch.stack([rad * torch.cos(ang), rad * torch.sin(ang)], -1)
    z = (1.0 + 0.4 * torch.arange(nf, dtype=torch.float32))[None, :, None] + 0.1 * torch.rand(B, nf, 3, generator=g)
    ndc = torch.cat([xy, z[..., None]], -1).reshape(B, nf * 3, 3).float().contiguous()
    faces = torch.arange(nf * 3, dtype=torch.int32).view(nf, 3)
    V, Fn = nf * 3, nf
    n64 = ndc.double().requires_grad_()
    p2f, zb, _, _, amb = P.rasterize_meshes(n64, faces.long(), S, 0.0, 1, return_ambiguous=True)
    fid_ref = torch.where(p2f[..., 0] >= 0, p2f[..., 0] % Fn, p2f[..., 0])
    gz = torch.randn(B, S, S, generator=g)
    gz[amb] = 0.0
    (zb[..., 0] * gz.double() * (p2f[..., 0] >= 0)).sum().backward()
    face_id, zbuf, _, ws = ops.rasterize_fwd(_d(ndc), _d(faces), S, soft=False)
    G0 = torch.randn(B, V, 3, generator=g)
    gn = _d(G0)                                                           # accumulates
    ck(L.harp_depth_bwd(p(face_id), p(ws), p(_d(faces)), p(_d(gz)), B, V, Fn, S, p(gn), st()), "depth_bwd")
    torch.cuda.synchronize()
    keep = ~amb
    assert int((fid_ref >= 0).sum()) > S * S // 4
    assert torch.equal(face_id.cpu().long()[keep], fid_ref[keep]), "K = 1 face ids differ away from the undecided pixels"
    # per pixel: perspective-correct barycentrics of a well-shaped triangle (~30 roundings, x 1 / (its area in pixels) in the x, y
    # gradient); summed over up to S^2 / nf pixels per vertex with atomics.  Relative to the largest entry: 2e-5
    want = n64.grad
    _worst("depth_bwd", (gn.cpu().double() - G0.double() - want).abs(), 2e-5 * want.abs().max() + 2 * U * G0.double().abs())
