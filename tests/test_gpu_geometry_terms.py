"""-m gpu: the geometry kernels that feed the loss, through the raw C ABI, against float64 torch on the CPU (values and autograd gradients):
harp_mesh_regularizers (uniform Laplacian, normal consistency, ARAP) on meshes that reach every branch of mesh_reg_kernel (both sides of the
staged / unstaged switch at V = 5120, both sides of the |n0||n1| = 1e-8 clamp, isolated vertices, zero-area faces, coincident vertices,
non-manifold edges, P = 0, a mesh 1 m from the origin), and the two skinning layers (harp_lbs_mano_* and harp_lbs_tree_*) at batch sizes
across their frame blocks with rotations of angle 0, 1e-7 ... 1e-3, pi +- 1e-3, 2 pi, 3 pi and 10 rad mixed over the frames of one batch.

Every bound is stated next to its assertion in float32 units (U = 2^-24, one rounding), derived from the magnitudes the rounding acts on,
with the reason; each case prints its worst error as a fraction of its bound (<= 1 passes)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24                  # unit roundoff of float32
ARM_CORR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "harp_amd", "assets", "arm_corr.npz")


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


def _dpad(a):
    """int32 device copy of a table; an empty table gets one (never read) element so that its pointer is not NULL"""
    t = torch.from_numpy(np.ascontiguousarray(a, np.int32)).reshape(-1)
    return _d(t if t.numel() else torch.zeros(1, dtype=torch.int32))


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


# ----------------------------------------------------------------------------------------------------------------------------------
# meshes
# ----------------------------------------------------------------------------------------------------------------------------------
def _grid(nx, ny, h, g):
    """nx x ny vertices, spacing h, two triangles per cell, z bumps of 0.3 h (no two neighbouring faces coplanar)"""
    x, y = torch.meshgrid(torch.arange(nx, dtype=torch.float64) * h, torch.arange(ny, dtype=torch.float64) * h, indexing="ij")
    z = 0.3 * h * torch.randn(nx, ny, generator=g, dtype=torch.float64)
    v = torch.stack([x, y, z], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing="ij")
    a = (i * ny + j).reshape(-1)
    faces = np.concatenate([np.stack([a, a + ny, a + 1], 1), np.stack([a + 1, a + ny, a + ny + 1], 1)], 0)
    return v, faces


def _hand(levels):
    """the MANO template subdivided `levels` times (1: the fitting step's 3093-vertex mesh), metres"""
    from harp_amd import synth, topology
    tpl = synth.load_template("hand")
    v = torch.from_numpy(tpl["base_verts"]).double()
    faces = tpl["faces0"].astype(np.int64)
    for _ in range(levels):
        e, faces = topology.subdivide_topology(faces, v.shape[0])
        v = torch.cat([v, v[torch.from_numpy(e)].mean(1)], 0)
    return v, faces


def _edge_mesh():
    """(verts (15,3), faces) with every branch of the kernel on dyadic coordinates (exact in float32, also after the per-frame scale and
    shift of _frames): a fan 0..4 whose centre is the exact mean of its rim (Laplacian row exactly 0: n = 0) with boundary edges on the rim;
    5, 6 coincident (ARAP l = 0 on edge 5-6) in the face [5, 6, 7] of area exactly 0 (n0 = 0 in the pair on edge 6-7); the edge 9-10
    shared by three faces (three pairs); 14 in no face (degree 0)."""
    P = [(0, 0, 0), (1, 0, 0.5), (0, 1, -0.5), (-1, 0, 0.5), (0, -1, -0.5),
         (3, 0, 0), (3, 0, 0), (4, 1, 0), (3.5, -1, 0.5),
         (6, 0, 0), (7, 0, 0), (6.5, 1, 0), (6.5, -1, 0.25), (6.5, 0.25, 1),
         (2, -3, 1.5)]
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [5, 6, 7], [6, 8, 7], [9, 10, 11], [10, 9, 12], [9, 10, 13]])
    return torch.tensor(P, dtype=torch.float64), faces


def _mesh(name):
    """(verts (V,3) float64, faces, frame noise) of a named case"""
    g = _gen(sum(map(ord, name)))
    if name == "hand_m":                            # millimetre faces in metres: every normal-consistency pair clamped
        v, f = _hand(1)
        return v, f, 2e-4
    if name == "hand_unit":                         # the same mesh x 20 (3.3 across): every pair unclamped (at x 6, unit size, the
        v, f = _hand(1)                             # smallest faces' |n0||n1| is still below 1e-8)
        return v * 20.0, f, 2e-3
    if name == "hand_far":                          # ~1 m from the origin: cancellation in mean(nbrs) - p, 1000 l - 1000 r
        v, f = _hand(1)
        return v + torch.tensor([0.6, -0.5, 0.6], dtype=torch.float64), f, 1e-3
    if name == "hand12k":                           # subdivided once more: 12k vertices, the unstaged kernel
        v, f = _hand(2)
        return v, f, 1e-3
    if name == "grid5120":                          # V * 12 B = 60 KB exactly: the last staged size
        v, f = _grid(64, 80, 1.0 / 8, g)
        return v, f, 1e-3
    if name == "grid5121":                          # one vertex more: the first unstaged size
        v, f = _grid(3, 1707, 1.0 / 8, g)
        return v, f, 1e-3
    if name == "mixed":                             # cells 3e-3 .. 3e-2 on a side: |n0||n1| from ~1e-10 to ~1e-6, both sides of 1e-8
        h = 3e-3 * 10.0 ** (torch.arange(24, dtype=torch.float64) / 23)
        c = torch.cat([torch.zeros(1, dtype=torch.float64), h.cumsum(0)])
        x, y = torch.meshgrid(c, c, indexing="ij")
        hh = torch.minimum(torch.cat([h, h[-1:]])[:, None], torch.cat([h, h[-1:]])[None, :])
        v = torch.stack([x, y, 0.3 * hh * torch.randn(25, 25, generator=g, dtype=torch.float64)], -1).reshape(-1, 3)
        _, f = _grid(25, 25, 1.0, g)
        return v, f, 0.0
    if name == "edge":
        v, f = _edge_mesh()
        return v, f, 0.0
    if name == "tri":                               # P = 0
        return torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, -0.5]], dtype=torch.float64), np.array([[0, 1, 2]]), 0.0
    raise KeyError(name)


def _frames(v, B, noise, g, name):
    """(B,V,3) float32 frames: frame b = v * (1 + b / 8) + (b / 4, -b / 8, b / 16) (exact on dyadic coordinates), + noise * N(0, 1)
    (not for the edge mesh, whose special vertices must stay exact)"""
    b = torch.arange(B, dtype=torch.float64)
    s = (1 + b / 8)[:, None, None] if name in ("edge", "tri") else torch.ones(B, 1, 1, dtype=torch.float64)
    t = torch.stack([b / 4, -b / 8, b / 16], -1)[:, None] if name in ("edge", "tri") else torch.zeros(B, 1, 3, dtype=torch.float64)
    out = v[None] * s + t
    if noise:
        out = out + noise * torch.randn(out.shape, generator=g, dtype=torch.float64)
    if name == "edge":                              # the non-manifold piece and the isolated vertex: generic positions per frame
        out[:, 9:] += 0.1 * torch.randn(B, 6, 3, generator=g, dtype=torch.float64)
    return out.float()


def _tables(faces, V, verts32=None):
    """every table of harp_mesh_regularizers, built with harp_amd.topology exactly as synth.build_topology does; pairs whose |n0||n1| (on
    any frame of verts32, float64) lies within 5 % of the 1e-8 clamp are LEFT OUT: there float32 cannot decide the branch (the kernel's
    l0 l1 and torch's sqrt(w1 w2) differ by a few U).  Returns the tables and the number of pairs left out."""
    from harp_amd import topology
    edges, _ = topology.unique_edges(faces, V)
    rows = np.concatenate([edges[:, 0], edges[:, 1]])
    cols = np.concatenate([edges[:, 1], edges[:, 0]])
    nbr_off, nbr_idx = topology.csr_from_pairs(rows, cols, V)
    pairs = topology.normal_consistency_pairs(faces, V)
    dropped = 0
    if verts32 is not None and len(pairs):
        n0, n1 = _pair_normals(verts32.double(), torch.from_numpy(pairs).long())
        ratio = n0.norm(dim=-1) * n1.norm(dim=-1) / 1e-8
        keep = ((ratio - 1).abs() >= 0.05).all(0).numpy()
        dropped = int((~keep).sum())
        pairs = pairs[keep]
    vp_off, vp_idx = topology.csr_from_pairs(pairs.reshape(-1), np.arange(pairs.size), V)   # vertex -> pair*4+role
    return dict(edges=edges, nbr_off=nbr_off, nbr_idx=nbr_idx, pairs=pairs.reshape(-1, 4), vp_off=vp_off, vp_idx=vp_idx), dropped


def _pair_normals(v, p):
    v0, v1, a, b = v[:, p[:, 0]], v[:, p[:, 1]], v[:, p[:, 2]], v[:, p[:, 3]]
    return torch.cross(v1 - v0, a - v0, dim=-1), -torch.cross(v1 - v0, b - v0, dim=-1)


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 reference and bounds of harp_mesh_regularizers
# ----------------------------------------------------------------------------------------------------------------------------------
def _reference(v32, ref32, T, w):
    """per-term losses and weighted gradients, float64 autograd on the float32 inputs"""
    from oracle import harp_ref as H
    from oracle import p3d_like as P
    v64 = v32.double().requires_grad_()
    off, idx = torch.from_numpy(T["nbr_off"]).long(), torch.from_numpy(T["nbr_idx"]).long()
    terms = [P.mesh_laplacian_smoothing_uniform(v64, off, idx), P.mesh_normal_consistency(v64, torch.from_numpy(T["pairs"]).long()),
             H.arap_loss(v64, ref32.double()[None], torch.from_numpy(T["edges"]).long())]
    grads = []
    for k, t in enumerate(terms):
        gk = torch.autograd.grad(w[k] * t, v64, allow_unused=True)[0] if t.requires_grad else None
        grads.append(torch.zeros_like(v64) if gk is None else gk.detach())
    return [t.item() for t in terms], grads


def _lap_bounds(v, T, B, V, w0):
    """Laplacian.  lv = a / deg - p with a a float32 sum of deg neighbours: per component (deg + 3) U (|a| / deg + |p|) (the |p| part is the
    cancellation of a mesh far from the origin); n = |lv| adds 3 U n.  Loss: sc (e_lv + 6 U n) per vertex.  Gradient: the unit vector lv / n
    carries min(2, 2 e_lv / n) (a unit vector cannot be off by more than 2, which also covers n = 0 exactly: both sides then take the zero
    subgradient) and ~6 roundings; a vertex gets its own row's and 1 / deg of each neighbour's row, summed in float32 ((deg + 1) U more)."""
    off, idx = torch.from_numpy(T["nbr_off"]).long(), torch.from_numpy(T["nbr_idx"]).long()
    deg = (off[1:] - off[:-1]).double()
    row = torch.repeat_interleave(torch.arange(V), (off[1:] - off[:-1]))
    a = torch.zeros_like(v).index_add(1, row, v[:, idx])
    aabs = torch.zeros_like(v).index_add(1, row, v[:, idx].abs())
    inv = torch.where(deg > 0, 1.0 / deg.clamp_min(1), torch.zeros_like(deg))[None, :, None]
    lv = a * inv - v
    n = lv.norm(dim=-1)
    e_lv = ((deg[None, :, None] + 3) * U * (aabs * inv + v.abs())).norm(dim=-1)
    sc = 1.0 / (V * B)
    loss_b = (sc * (e_lv + 6 * U * n)).sum().item()
    W = abs(w0) * sc
    dirv = torch.clamp(2 * e_lv / n.clamp_min(1e-300), max=2.0)
    own = W * (dirv + 6 * U)
    nbr = torch.zeros(B, V, dtype=torch.float64).index_add(1, row, (W * inv[..., 0] * (dirv + 7 * U))[:, idx])
    mag = W * (1 + torch.zeros(B, V, dtype=torch.float64).index_add(1, row, inv[..., 0].expand(B, V)[:, idx]))
    return loss_b, own + nbr + (deg[None] + 1) * U * mag


def _arap_bounds(v, ref, T, B, V, w2):
    """ARAP.  d = p_u - p_nb is one rounding of an exact difference (U |d|), l = |d| carries 3 U l, r likewise: diff = 1000 l - 1000 r carries
    1000 (4 l + 4 r) U + U |diff| whatever diff is.  Per directed edge (each edge is visited from both ends): loss 0.5 sc diff^2 carries
    sc (|diff| e + e^2 / 2) + 4 U of it; gradient 2000 W diff d / l carries 2000 W (e + 10 U |diff|) (|d| / l = 1; l = 0: both sides give 0).
    A vertex sums deg such terms (deg U of their sum)."""
    off, idx = torch.from_numpy(T["nbr_off"]).long(), torch.from_numpy(T["nbr_idx"]).long()
    E = T["edges"].shape[0]
    row = torch.repeat_interleave(torch.arange(V), (off[1:] - off[:-1]))
    l = (v[:, row] - v[:, idx]).norm(dim=-1)
    r = (ref[row] - ref[idx]).norm(dim=-1)[None]
    diff = 1000 * (l - r)
    e = 1000 * U * (4 * l + 4 * r) + U * diff.abs()
    sc = 1.0 / (E * B)
    loss_b = (sc * (diff.abs() * e + 0.5 * e * e + 4 * U * 0.5 * diff * diff)).sum().item()
    W = abs(w2) * sc
    deg = (off[1:] - off[:-1]).double()[None]
    gb = torch.zeros(B, V, dtype=torch.float64).index_add(1, row, 2000 * W * (e + 10 * U * diff.abs()))
    gm = torch.zeros(B, V, dtype=torch.float64).index_add(1, row, 2000 * W * diff.abs())
    return loss_b, gb + deg * U * gm


def _nc_bounds(v, T, B, V, w1):
    """Normal consistency, per pair.  e = v1 - v0, da = a - v0, db = b - v0: one rounding each (inputs exact).  n0 = e x da: per component two
    products and a difference on top of the inputs' errors: 4 U of the |e| x |da| magnitudes (the cancellation of a thin face); l0 adds 2 U l0;
    dp = n0 . n1 carries |dn0| l1 + l0 |dn1| + 3 U sum |n0 n1|.  den = max(l0 l1, 1e-8f): its error (unclamped) or the constant's rounding
    (clamped: 1e-8f = 1e-8 (1 - 6e-9)).  cs = dp / den: e_cs = e_dp / den + |dp| e_den / den^2 + U |cs|.  Gradient: g0 = kk (n1 / den - cs n0
    / l0^2) (unclamped) or kk n1 / den (clamped), g1 likewise; each vertex of the pair gets cross products of (e, da, db) with (g0, g1), the
    v0 role the sum of three: 3 x ((|e| + |da| + |db|) (e_g0 + e_g1) + (U (|e| + |da| + |db|) + 6 U (...)) (|g0| + |g1|)), and the float32 sum
    over the vertex's pairs adds (pairs + 2) U of the sum of magnitudes."""
    p = torch.from_numpy(T["pairs"]).long()
    Pn = p.shape[0]
    if Pn == 0:
        return 0.0, torch.zeros(B, V, dtype=torch.float64), torch.zeros(B, 0, dtype=torch.bool)
    v0, v1, a, b = v[:, p[:, 0]], v[:, p[:, 1]], v[:, p[:, 2]], v[:, p[:, 3]]
    ev, da, db = v1 - v0, a - v0, b - v0

    def xabs(x, y):
        x, y = x.abs(), y.abs()
        return torch.stack([x[..., 1] * y[..., 2] + x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] + x[..., 0] * y[..., 2],
                            x[..., 0] * y[..., 1] + x[..., 1] * y[..., 0]], -1)
    n0, n1 = torch.cross(ev, da, dim=-1), -torch.cross(ev, db, dim=-1)
    en0, en1 = 4 * U * xabs(ev, da).norm(dim=-1), 4 * U * xabs(ev, db).norm(dim=-1)
    l0, l1 = n0.norm(dim=-1), n1.norm(dim=-1)
    el0, el1 = en0 + 2 * U * l0, en1 + 2 * U * l1
    dp = (n0 * n1).sum(-1)
    edp = en0 * l1 + l0 * en1 + 3 * U * (n0 * n1).abs().sum(-1)
    clamped = l0 * l1 <= 1e-8
    den = torch.where(clamped, torch.full_like(l0, 1e-8), l0 * l1)
    eden = torch.where(clamped, U * den, el0 * l1 + l0 * el1 + U * l0 * l1)
    cs = dp / den
    ecs = edp / den + dp.abs() * eden / den ** 2 + U * cs.abs()
    sc = 1.0 / (Pn * B)
    loss_b = (sc * (ecs + 3 * U * (1 - cs).abs())).sum().item()
    kk = abs(w1) * sc
    l0s, l1s = l0.clamp_min(1e-300), l1.clamp_min(1e-300)
    g0 = torch.where(clamped, kk * l1 / den, kk * (l1 / den + cs.abs() / l0s))
    g1 = torch.where(clamped, kk * l0 / den, kk * (l0 / den + cs.abs() / l1s))
    eg0 = torch.where(clamped, kk * (en1 + 3 * U * l1) / den,
                      kk * (en1 / den + l1 * eden / den ** 2 + ecs / l0s + cs.abs() * 3 * el0 / l0s ** 2 + 6 * U * (l1 / den + cs.abs() / l0s)))
    eg1 = torch.where(clamped, kk * (en0 + 3 * U * l0) / den,
                      kk * (en0 / den + l0 * eden / den ** 2 + ecs / l1s + cs.abs() * 3 * el1 / l1s ** 2 + 6 * U * (l0 / den + cs.abs() / l1s)))
    # (at a zero-area face, l0 = 0 exactly on both sides: it is clamped, and its g0 term is kk n1 / den with no 1 / l0)
    arm = ev.norm(dim=-1) + da.norm(dim=-1) + db.norm(dim=-1)
    per = 3 * (arm * (eg0 + eg1) + 7 * U * arm * (g0 + g1))
    mag = 3 * arm * (g0 + g1)
    cnt = torch.zeros(V, dtype=torch.float64).index_add(0, p.reshape(-1), torch.ones(4 * Pn, dtype=torch.float64))
    gb = torch.zeros(B, V, dtype=torch.float64)
    gm = torch.zeros(B, V, dtype=torch.float64)
    for k in range(4):
        gb = gb.index_add(1, p[:, k], per)
        gm = gm.index_add(1, p[:, k], mag)
    return loss_b, gb + (cnt[None] + 2) * U * gm, clamped


def _run_meshreg(L, p, st, v32, ref32, T, w, loss0, G0, *, with_ref=True, with_w=True, with_g=True, P=None, E=None, B=None):
    B_, V = v32.shape[:2]
    loss = _d(torch.tensor(loss0, dtype=torch.float32))
    g = _d(G0.float())
    st_ = L.harp_mesh_regularizers(p(_d(v32)), p(_d(ref32)) if with_ref else None, p(_dpad(T["nbr_off"])), p(_dpad(T["nbr_idx"])),
                                   p(_dpad(T["pairs"])), p(_dpad(T["vp_off"])), p(_dpad(T["vp_idx"])), B_ if B is None else B, V,
                                   T["pairs"].shape[0] if P is None else P, T["edges"].shape[0] if E is None else E,
                                   p(_d(torch.tensor(w, dtype=torch.float32))) if with_w else None, p(loss), p(g) if with_g else None, st())
    torch.cuda.synchronize()
    return st_, loss.cpu().double(), g.cpu().double()


MESHES = [("edge", 1), ("edge", 33), ("tri", 3), ("hand_m", 3), ("hand_m", 33), ("hand_unit", 3), ("hand_far", 3), ("mixed", 3),
          ("grid5120", 1), ("grid5121", 1), ("hand12k", 3)]


def _case(name, B):
    v, faces, noise = _mesh(name)
    V = v.shape[0]
    g = _gen(V * 7 + B)
    v32 = _frames(v, B, noise, g, name)
    T, dropped = _tables(faces, V, v32)
    e = torch.from_numpy(T["edges"]).long()
    h = (v[e[:, 0]] - v[e[:, 1]]).norm(dim=-1).mean()
    ref32 = (v + 0.1 * h * torch.randn(V, 3, generator=g, dtype=torch.float64)).float()          # reference mesh: edges ~10 % off
    if name == "edge":
        ref32[6] = ref32[5] + torch.tensor([0.25, 0.0, 0.0])                # 5, 6 apart in the reference: diff = -1000 r at l = 0
    return v32, ref32, T, dropped, faces


@pytest.mark.parametrize("name,B", MESHES)
def test_mesh_regularizers_against_float64(name, B, monkeypatch):
    L, p, st, ck = _L()
    v32, ref32, T, dropped, faces = _case(name, B)
    V = v32.shape[1]
    w = [0.7, 1.3, 0.9]
    w32 = [float(np.float32(x)) for x in w]
    g = _gen(V + B)
    loss0 = [0.25, -0.5, 0.125]                                             # loss[0..2] and g_verts accumulate
    G0 = torch.randn(B, V, 3, generator=g, dtype=torch.float64).float() * 1e-3
    ref_l, ref_g = _reference(v32, ref32, T, w32)
    v = v32.double()
    lb_lap, gb_lap = _lap_bounds(v, T, B, V, w32[0])
    lb_ar, gb_ar = _arap_bounds(v, ref32.double(), T, B, V, w32[2])
    out = _nc_bounds(v, T, B, V, w32[1])
    lb_nc, gb_nc = out[0], out[1]
    tag = f"meshreg {name} B={B} V={V}"
    P = T["pairs"].shape[0]
    ncl = int(out[2].sum())
    print(f"[{tag}] P={P} (left out at the clamp: {dropped}), clamped pair-frames {ncl} of {P * B}, "
          f"{'staged' if V * 12 <= 60 * 1024 else 'unstaged'}")
    if name == "hand_m":
        assert ncl == P * B and dropped == 0
    if name == "hand_unit":
        assert ncl == 0 and dropped == 0
    if name == "mixed":                                                    # both sides of the clamp, each well populated
        assert 0.2 * P * B < ncl < 0.8 * P * B, ncl
    if name == "edge":
        deg = np.diff(T["nbr_off"])
        assert deg[14] == 0 and (T["pairs"][:, :2] == [9, 10]).all(1).sum() == 3
    if name == "tri":
        assert P == 0
    # loss: each term's bound above + the float32 sum of positive partials (6 wave levels, up to 8 waves, one atomic per workgroup and
    # frame, the prefill): (16 + B ceil(V / 256)) U of the total
    k_sum = 16 + B * math.ceil(V / 256)
    for how in ("default", "lds80000") if V * 12 <= 60 * 1024 else ("default",):
        if how == "lds80000":                                              # the > 64 KB hipFuncSetAttribute path: same bounds (float atomics)
            monkeypatch.setenv("HARP_MESHREG_LDS", "80000")
        stt, loss, gv = _run_meshreg(L, p, st, v32, ref32, T, w32, loss0, G0)
        assert stt == 0, stt
        monkeypatch.delenv("HARP_MESHREG_LDS", raising=False)
        for k, (lb, nm) in enumerate(((lb_lap, "laplacian"), (lb_nc, "normal"), (lb_ar, "arap"))):
            want = loss0[k] + ref_l[k]
            _worst(f"{tag} {how} loss {nm}", torch.tensor([abs(loss[k].item() - want)]),
                   torch.tensor([lb + k_sum * U * (abs(loss0[k]) + abs(ref_l[k])) + 1e-300]))
        if name == "tri":
            assert loss[1].item() == np.float32(loss0[1])                  # P = 0: nothing added, no NaN
        # gradient: the three terms' bounds + three float atomics onto the prefill (U each of |G0| + the partial sums)
        want = G0.double() + ref_g[0] + ref_g[1] + ref_g[2]
        atom = 3 * U * (G0.double().abs() + ref_g[0].abs() + ref_g[1].abs() + ref_g[2].abs()).amax(-1)
        err = (gv - want).abs().amax(-1)
        _worst(f"{tag} {how} g_verts", err, gb_lap + gb_nc + gb_ar + atom + 1e-300)
        if name == "edge":
            assert (gv[:, 14] - G0[:, 14].double()).abs().max() > 0        # the isolated vertex's row -v has a gradient (and no NaN)


def test_mesh_regularizers_call_semantics():
    """w or g_verts NULL: losses only, g_verts untouched; ref_verts NULL: loss[2] untouched; P < 0, E < 0 refused with real buffers (the
    harp_mesh_kps_terms form too) and nothing written."""
    L, p, st, ck = _L()
    v32, ref32, T, _, _ = _case("edge", 3)
    B, V = v32.shape[:2]
    w = [0.7, 1.3, 0.9]
    G0 = torch.randn(B, V, 3, generator=_gen(3)).float()
    loss0 = [0.25, -0.5, 0.125]
    _, full_loss, _ = _run_meshreg(L, p, st, v32, ref32, T, w, loss0, G0)
    for kw in ({"with_w": False}, {"with_g": False}):
        stt, loss, gv = _run_meshreg(L, p, st, v32, ref32, T, w, loss0, G0, **kw)
        assert stt == 0 and torch.equal(gv, G0.double()), kw
        # the same loss as with the gradient (atomics may order the partials differently: a few U of the totals)
        assert (loss - full_loss).abs().max() <= 64 * U * (full_loss.abs().max() + 1), (kw, loss, full_loss)
    stt, loss, gv = _run_meshreg(L, p, st, v32, ref32, T, w, loss0, G0, with_ref=False)
    assert stt == 0 and loss[2].item() == np.float32(loss0[2])
    assert (loss[:2] - full_loss[:2]).abs().max() <= 64 * U * (full_loss.abs().max() + 1)
    for kw in ({"P": -1}, {"E": -1}):
        stt, loss, gv = _run_meshreg(L, p, st, v32, ref32, T, w, loss0, G0, **kw)
        assert stt == 1 and torch.equal(gv, G0.double()) and torch.equal(loss, torch.tensor(loss0, dtype=torch.float32).double()), kw
        Pn, En = kw.get("P", T["pairs"].shape[0]), kw.get("E", T["edges"].shape[0])
        lk = torch.full((1,), 0.5, device=DEV)
        gp = torch.full((B, 21, 3), 2.0, device=DEV)
        lm = torch.full((3,), 0.5, device=DEV)
        gm = torch.full((B, V, 3), 2.0, device=DEV)
        stt = L.harp_mesh_kps_terms(p(_d(v32)), p(_d(ref32)), p(_dpad(T["nbr_off"])), p(_dpad(T["nbr_idx"])), p(_dpad(T["pairs"])),
                                    p(_dpad(T["vp_off"])), p(_dpad(T["vp_idx"])), B, V, Pn, En, p(_d(torch.tensor(w))), p(lm), p(gm),
                                    p(_d(torch.zeros(B, 21, 3))), None, p(_d(torch.zeros(B, 21, 3))), 21, p(_d(torch.ones(1))), p(lk), p(gp), st())
        torch.cuda.synchronize()
        assert stt == 1 and (lk == 0.5).all() and (gp == 2.0).all() and (lm == 0.5).all() and (gm == 2.0).all(), kw


# ----------------------------------------------------------------------------------------------------------------------------------
# skinning layers
# ----------------------------------------------------------------------------------------------------------------------------------
ANGLES = [0.0, 1e-7, 1e-5, 1e-3, math.pi - 1e-3, math.pi + 1e-3, 2 * math.pi, 3 * math.pi, 10.0]


def _rotations(B, NJ, g):
    """(B,NJ,3) float64 axis-angles: every (frame, joint) takes one of ANGLES along an axis or a generic direction, the assignment shifted
    per frame (so that an indexing error between frames shows), and every third one a generic N(0, 0.4) rotation"""
    axes = torch.eye(3, dtype=torch.float64)
    out = torch.empty(B, NJ, 3, dtype=torch.float64)
    for b in range(B):
        for j in range(NJ):
            k = (b * 5 + j * 7) % (len(ANGLES) * 2 + 4)
            if k >= 2 * len(ANGLES):
                out[b, j] = torch.randn(3, generator=g, dtype=torch.float64) * 0.4
                continue
            d = axes[(b + j) % 3] if k % 2 == 0 else torch.nn.functional.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0)
            out[b, j] = ANGLES[k // 2] * d
    return out


def _angle(aa32_sum):
    return aa32_sum.norm(dim=-1)


def _skin_vertex_bound(theta_chain, R, mag_vp, depth):
    """verts / joints in mm.  A rotation built in float32 carries (24 + 2 theta) U (the quaternion or sin / cos form's ~20 operations, and the
    float32 angle argument, which carries 2 U theta); a chain of `depth` rotations moves a point at distance <= R (metres) by the sum of that
    along the chain, plus 3 U per 3 x 3 product and level, 16 U for the skinning sum over joints and 4 U for T v + t.  The blend shapes
    v_t + S beta + P pose_map are float32 sums of 146 terms in 4 slices: 48 U of the sum of their magnitudes.  x 1000 (mm)."""
    return 1000.0 * ((theta_chain * U + (3 * depth + 20) * U) * R + 48 * U * mag_vp)


def _mano_vertex_bound(m64, hm, pose, betas, v_ref):
    """_skin_vertex_bound of the MANO layer (B,1,1) [mm] for pose (B,48) / betas (B,10) float32 and the float64 vertices v_ref (B,778,3) mm;
    m64: the model in float64 (shapedirs (778,3,10), posedirs (778,3,135)), hm (15,3) the float32 hands_mean.  Shared with
    tests/test_gpu_step_front_back.py (the same layer inside the fused front)."""
    B = pose.shape[0]
    th = _angle(pose.view(B, 16, 3).double() + torch.cat([torch.zeros(1, 3), hm]).double())
    chain = th[:, :1] + th[:, 1:].view(B, 5, 3).sum(-1).amax(-1, keepdim=True)       # root + the worst finger
    # |v_t| + sum |S| |beta| + 2 sum |P| (|R - I| <= 2 per entry), the largest over the vertices
    vp = (m64["v_template"].abs()[None] + torch.einsum("vck,bk->bvc", m64["shapedirs"].abs(), betas.double().abs())
          + 2 * m64["posedirs"].abs().sum(-1)[None]).amax((1, 2))[:, None]
    R = (v_ref / 1000).norm(dim=-1).amax(-1, keepdim=True) + 0.2                     # metres: |posed vertex| + the hand's extent
    # capped at the golden tolerance (3e-3 mm): never looser than it
    return _skin_vertex_bound(2 * chain + 4 * 24, R, vp, 4).clamp(max=3e-3)[:, :, None]


def test_mano_lbs_against_float64_at_rotation_edges():
    from harp_amd import synth
    from harp_amd.manopth.manolayer import ManoDeviceModel
    from oracle import harp_ref as H
    from tests._scene import rel
    L, p, st, ck = _L()
    model = synth.make_mano_model(seed=0)
    dm = ManoDeviceModel(model, DEV)
    m64 = {k: torch.from_numpy(np.asarray(model[k], np.float32)).double() for k in ("v_template", "J_regressor", "weights", "hands_mean")}
    m64["shapedirs"] = torch.from_numpy(np.asarray(model["shapedirs"], np.float32)).double().reshape(778, 3, 10)
    m64["posedirs"] = torch.from_numpy(np.asarray(model["posedirs"], np.float32)).double().reshape(778, 3, 135)
    hm = torch.from_numpy(np.asarray(model["hands_mean"], np.float32)).reshape(15, 3)
    for B in (1, 7, 9, 17, 33):                                           # 9, 17, 33: a partial last block of FRAMES_PER_BLOCK = 8
        g = _gen(100 + B)
        aa = _rotations(B, 16, g)
        pose = aa.clone()
        pose[:, 1:] -= hm.double()                                        # finger rotation = pose + hands_mean; angle 0: pose = -hands_mean
        pose = pose.float().reshape(B, 48)
        zero = (aa == 0).all(-1)
        pose.view(B, 16, 3)[:, 1:][zero[:, 1:]] = -hm.expand(B, 15, 3)[zero[:, 1:]]
        betas = (torch.randn(B, 10, generator=g) * 1.0).float()
        betas[::3, 0], betas[1::3, 3] = 3.0, -3.0                        # large betas
        trans = (torch.randn(B, 3, generator=g) * 0.05).float()
        cpu = [t.double().requires_grad_() for t in (pose, betas, trans)]
        v_ref, j_ref = H.mano_forward(m64, *cpu)
        gv, gj = torch.randn(B, 778, 3, generator=g), torch.randn(B, 21, 3, generator=g)
        ((v_ref * gv.double()).sum() + (j_ref * gj.double()).sum()).backward()
        ws = torch.empty(L.harp_lbs_mano_ws_floats(B), device=DEV)
        verts, joints = torch.full((B, 778, 3), float("nan"), device=DEV), torch.full((B, 21, 3), float("nan"), device=DEV)
        pd, bd, td = _d(pose), _d(betas), _d(trans)
        ck(L.harp_lbs_mano_fwd(ctypes.byref(dm.struct), p(pd), p(bd), p(td), B, p(ws), p(verts), p(joints), st()), "mano_fwd")
        outs = []
        for rep in range(2):                                              # twice on one forward workspace: the same gradients
            gvd = _d(gv)
            og = [torch.full(s, float("nan"), device=DEV) for s in ((B, 48), (B, 10), (B, 3))]      # overwritten
            ck(L.harp_lbs_mano_bwd(ctypes.byref(dm.struct), p(pd), p(bd), p(td), B, p(ws), p(gvd), p(_d(gj)), *[p(o) for o in og], st()),
               "mano_bwd")
            torch.cuda.synchronize()
            outs.append([o.cpu() for o in og] + [gvd.cpu()])
        for a, b_ in zip(outs[0][:3], outs[1][:3]):                       # (atomics in the reductions: equal to a few U, not bit-equal)
            assert rel(a.double(), b_.double()) < 1e-6, B
        # g_verts in place: the tip vertices get the tip joints' gradient added, every other entry is left as it was
        tips = list(H.MANO_TIPS_RIGHT)
        want_gv = gv.clone()
        for k, src in enumerate(H.MANO_JOINT_REORDER):
            if src >= 16:
                want_gv[:, tips[src - 16]] += gj[:, k]
        assert torch.equal(outs[0][3], want_gv), B
        tag = f"mano B={B}"
        bv = _mano_vertex_bound(m64, hm, pose, betas, v_ref.detach())
        _worst(tag + " verts", (verts.cpu().double() - v_ref.detach()).abs(), bv)
        _worst(tag + " joints", (joints.cpu().double() - j_ref.detach()).abs(), bv)
        # gradients: the golden tolerance (rel-L2 1e-4) per frame and block, tighter than over the batch (a derived element bound would have
        # to follow the cancellation of 778 x 3 signed terms per reduction; the per-frame rel-L2 keeps a frame-indexing error visible)
        for o, ref_, nm in zip(outs[0][:3], cpu, ("g_pose", "g_betas", "g_trans")):
            _worst(f"{tag} {nm} per frame", (o.double() - ref_.grad).norm(dim=-1), 1e-4 * ref_.grad.norm(dim=-1) + 1e-300)
            assert rel(o.double(), ref_.grad) < 1e-4


def _tree_setup():
    from harp_amd import synth
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    m = synth.make_smplx_arm_model(seed=0)
    corr = np.load(ARM_CORR)
    dm = SMPLXARM(m, m["faces"], corr["mano_vert_from_arm"], device=DEV).device_model
    return m, dm


def test_tree_lbs_against_float64_at_rotation_edges():
    from oracle import harp_ref as H
    from tests._scene import rel
    L, p, st, ck = _L()
    m, dm = _tree_setup()
    mt = {k: torch.from_numpy(v).double() if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in m.items()}
    pm = torch.from_numpy(m["pose_mean"]).view(55, 3)
    rows = [0, 21] + list(range(40, 55))                                  # the joint each in_pose row drives
    NB, no = dm.struct.NB, dm.struct.n_joints_out
    for B in (1, 5, 17, 33):                                              # past kSkinF = 4 and the 16-row MFMA tiles
        g = _gen(200 + B)
        aa = _rotations(B, 17, g)
        zero = (aa == 0).all(-1)
        in_pose = (aa - pm[rows].double()).float()
        in_pose[zero] = -pm[rows].expand(B, 17, 3)[zero]                 # angle exactly 0: in_pose = -pose_mean
        betas = torch.randn(B, NB, generator=g).float()                   # 10 betas | 10 expression coefficients
        betas[::3, 0], betas[1::3, 12] = 3.0, -3.0
        transl = (torch.randn(B, 3, generator=g) * 0.05).float()
        cpu = [betas[:, :10].double().requires_grad_(), in_pose[:, 0].double().requires_grad_(), transl.double().requires_grad_(),
               in_pose[:, 2:].reshape(B, 45).double().requires_grad_(), in_pose[:, 1].double().requires_grad_(),
               betas[:, 10:].double().requires_grad_()]
        v_ref, j_ref = H.smplxarm_forward(mt, *cpu[:5], expression=cpu[5])
        gv, gj = torch.randn(v_ref.shape, generator=g), torch.randn(j_ref.shape, generator=g)
        ((v_ref * gv.double()).sum() + (j_ref * gj.double()).sum()).backward()
        ws = torch.empty(L.harp_lbs_tree_ws_floats(ctypes.byref(dm.struct), B), device=DEV)
        verts, joints = torch.full(v_ref.shape, float("nan"), device=DEV), torch.full(j_ref.shape, float("nan"), device=DEV)
        ipd, bd, td = _d(in_pose), _d(betas), _d(transl)
        ck(L.harp_lbs_tree_fwd(ctypes.byref(dm.struct), p(ipd), p(bd), p(td), B, p(ws), p(verts), p(joints), st()), "tree_fwd")
        outs = []
        for rep in range(2):
            gvd = _d(gv)
            og = [torch.full(s, float("nan"), device=DEV) for s in ((B, 17, 3), (B, NB), (B, 3))]   # overwritten
            ck(L.harp_lbs_tree_bwd(ctypes.byref(dm.struct), p(ipd), p(bd), p(td), B, p(ws), p(gvd), p(_d(gj)), *[p(o) for o in og], st()),
               "tree_bwd")
            torch.cuda.synchronize()
            outs.append([o.cpu() for o in og] + [gvd.cpu()])
        for a, b_ in zip(outs[0][:3], outs[1][:3]):                       # (atomics in the reductions: equal to a few U, not bit-equal)
            assert rel(a.double(), b_.double()) < 1e-6, B
        # g_verts in place: the tip vertices get their joints' gradient added (atomics: exact for one addend), every other entry unchanged
        want_gv = gv.clone()
        for k, j in enumerate(H.ARM_JOINT_IDX):
            if j >= 71:
                want_gv[:, int(m["tip_verts"][j - 71])] += gj[:, k]
        assert torch.equal(outs[0][3], want_gv), B
        tag = f"tree B={B}"
        th = _angle(in_pose.double() + pm[rows].double())
        chain = th[:, :2].sum(-1, keepdim=True) + th[:, 2:].view(B, 5, 3).sum(-1).amax(-1, keepdim=True)
        vp = (mt["v_template"].abs()[None] + torch.einsum("vck,bk->bvc", mt["shapedirs"].abs(), betas.double().abs())
              + 2 * mt["posedirs"].abs().sum(0).view(-1, 3)[None]).amax((1, 2))[:, None]
        # metres: the posed vertex (before the recentring on the wrist) is within |J| + |v| of every joint of its chain
        R = mt["J_template"].norm(dim=-1).max() + (v_ref.detach() / 1000 - transl.double()[:, None]).norm(dim=-1).amax(-1, keepdim=True)
        # 11 levels (root, 3 spine, collar, shoulder, elbow, wrist, 3 finger); only the 5 driven joints rotate (the others: exactly I);
        # capped at the golden tolerance (3e-3 mm)
        bv = _skin_vertex_bound(2 * chain + 5 * 24, R, vp, 11).clamp(max=3e-3)[:, :, None]
        _worst(tag + " verts", (verts.cpu().double() - v_ref.detach()).abs(), bv)
        _worst(tag + " joints", (joints.cpu().double() - j_ref.detach()).abs(), bv)
        ref_g = [cpu[1].grad, cpu[4].grad] + list(cpu[3].grad.view(B, 15, 3).unbind(1))
        g_in_ref = torch.stack(ref_g, 1)
        for got, want, nm in ((outs[0][0], g_in_ref, "g_in_pose"), (outs[0][1], torch.cat([cpu[0].grad, cpu[5].grad], 1), "g_betas"),
                              (outs[0][2], cpu[2].grad, "g_transl")):
            _worst(f"{tag} {nm} per frame", (got.double() - want).reshape(B, -1).norm(dim=-1), 1e-4 * want.reshape(B, -1).norm(dim=-1) + 1e-300)
            assert rel(got.double(), want) < 1e-4


def test_tree_lbs_bwd_refuses_oversized_models_untouched():
    """NJ > 64 or NB > 32 (which the forward call refuses) and B = 0 make the backward call return HARP_ERR_ARG before any launch (B < 0 is
    not tried: without the check its grid would not be empty).  Real buffers, sized for the larger model, and a real forward workspace;
    nothing is written."""
    L, p, st, ck = _L()
    _, dm = _tree_setup()
    B = 2
    s = dm.struct
    ws = torch.zeros(L.harp_lbs_tree_ws_floats(ctypes.byref(s), B) * 2, device=DEV)
    ip, bt, tr = _d(torch.zeros(B, 17, 3)), _d(torch.zeros(B, 64)), _d(torch.zeros(B, 3))
    verts, joints = torch.empty(B, dm.NV, 3, device=DEV), torch.empty(B, s.n_joints_out, 3, device=DEV)
    ck(L.harp_lbs_tree_fwd(ctypes.byref(s), p(ip), p(bt), p(tr), B, p(ws), p(verts), p(joints), st()), "tree_fwd")
    torch.cuda.synchronize()
    ws0 = ws.clone()
    for kw in ({"NJ": 65}, {"NB": 33}, {"B": 0}):
        t = type(s).from_buffer_copy(s)
        for k, val in kw.items():
            if k != "B":
                setattr(t, k, val)
        gv = torch.full((B, dm.NV, 3), 2.0, device=DEV)
        og = [torch.full(sz, 3.0, device=DEV) for sz in ((B, 17, 3), (B, 64), (B, 3))]
        if "B" not in kw:                                                 # (the forward call refuses the same model)
            assert L.harp_lbs_tree_fwd(ctypes.byref(t), p(ip), p(bt), p(tr), B, p(ws), p(verts), p(joints), st()) == 1
        stt = L.harp_lbs_tree_bwd(ctypes.byref(t), p(ip), p(bt), p(tr), kw.get("B", B), p(ws), p(gv), p(_d(torch.ones(B, s.n_joints_out, 3))),
                                  *[p(o) for o in og], st())
        torch.cuda.synchronize()
        assert stt == 1, kw
        assert (gv == 2.0).all() and all(bool((o == 3.0).all()) for o in og) and torch.equal(ws, ws0), kw
    from harp_amd.manopth.manolayer import ManoDeviceModel
    from harp_amd import synth
    mdm = ManoDeviceModel(synth.make_mano_model(seed=0), DEV)
    mws = torch.zeros(L.harp_lbs_mano_ws_floats(B), device=DEV)
    og = [torch.full(sz, 3.0, device=DEV) for sz in ((B, 48), (B, 10), (B, 3))]
    gv = torch.full((B, 778, 3), 2.0, device=DEV)
    for bad in (0,):
        assert L.harp_lbs_mano_bwd(ctypes.byref(mdm.struct), p(_d(torch.zeros(B, 48))), p(_d(torch.zeros(B, 10))), p(_d(torch.zeros(B, 3))),
                                   bad, p(mws), p(gv), p(_d(torch.ones(B, 21, 3))), *[p(o) for o in og], st()) == 1
    torch.cuda.synchronize()
    assert (gv == 2.0).all() and all(bool((o == 3.0).all()) for o in og) and (mws == 0).all()
