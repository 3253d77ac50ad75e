"""-m gpu: both compiled forms of the per-frame mesh chain through the raw C ABI -- harp_mesh_chain_fwd / _bwd (one 1024-thread workgroup
per frame, csrc/chain.hip + chain_body.h) and harp_mesh_chain_fwd_wide / _bwd_wide (four workgroups per frame, csrc/chain_wide.hip) --
against the float64 reference tests/_chain_ref.py, on synthetic meshes that are each the smallest to reach one path the two production
templates never reach: a wide part that owns no vertex, V % 4 != 0, E0 = 0, E0 > 3 * 1024, valence above kPre = 8, both il == 0 clamp
branches, V = harp_mesh_chain_max_vertices() exactly; with a general camera rotation and a light exactly on the vertical through the
centroid (look_at_rotation's degenerate branch).  The two production templates are cases as well: `mano` (3093 vertices) and `arm` (the
SMPL-X arm: 1026 + 3057 = 4083 vertices, 1021 per wide part, 0.8 m in front of the camera because it reaches 0.34 m from its centroid).

Forward: stage by stage, each stage against the reference evaluated on the kernel's OWN float32 output of the stage before, so that every
stage carries the bound derived for its stand-alone building block in tests/test_gpu_building_blocks.py (U = 2^-24).
Backward: the yardstick is the float64 VJP through the reference.  A bound composed through two chained normal passes cannot be derived
in advance, so the already pinned stand-alone sequence (harp_project_bwd x 2, harp_light_setup_bwd, harp_vertex_normals_bwd,
harp_displace_bwd, harp_vertex_normals_bwd, harp_subdivide_bwd) is run in float32 on the same inputs and the fused kernel passes if, per
output and connected component, e_chain <= 4 e_blocks + 8 U |reference|_max: the factor 4 covers the different summation order (a
1024-thread block sum / four partial sums instead of atomics), the floor the components where both are exact.  That rule holds g_v0 and
g_disp (thousands of numbers per case, where the fused error stays at a quarter of the bound).  g_cam_T and g_light_pos are three numbers
per frame, and the blocks sum them with atomics across workgroups, in an order that changes from run to run: their e_blocks moves by a
factor of ten between runs of the same inputs, and a run in which it happened to be small failed the `full` mesh's one-workgroup case.  These
two are therefore held to a derived float32 summation bound (_scalar_sum_bounds), deterministic like the fused kernels themselves; both
errors against the float64 VJP are still printed.

The `five` mesh (FIVE of the building-block tests) subdivides to 16 vertices; V % 4 = 3 is reached by `clamp` (15), = 2 by `tri`, = 1 by
`hub`, `hub_raw` and `mano`.  With B = 3, frame 0 has cam_R = diag(-1, -1, 1), frames 1 and 2 a seeded rotation, and frame 1 its light on
the vertical through the centroid; a B = 1 case is one frame with a seeded rotation and a generic light.  In the frame with the vertical light
the light view's cotangent g_ndc_l has only its depth component (see _cotangents): what the degenerate branch of the light camera does to
x / y camera sums over the vertices (a gain estimated at 1e15, not measured) is NOT tested; its x / y backward is reached only through the
shader's share g_light_R / g_light_T.  Frames 0 and 2 carry the full cotangent.

measured on the MI355X (three runs): forward, worst error as a fraction of its bound: vs 0.49, n1 0.08, il1 0.10, vd 0.50, n2 0.08, il2 0.10,
ndc_c 0.48, centroid 0.14, light_R 0.06, light_T 0.04, ndc_l 0.23.  Backward: g_v0 at most 0.45 and g_disp 0.25 of 4 e_blocks + 8 U |reference|_max,
in each run (only a few B = 3 g_disp lines, summed over frames by atomics on both sides, move at all); g_cam_T 0.038 and g_light_pos 0.037 of their derived bounds.  Worst e_chain / |reference|_max against the float64 VJP:
g_v0 2.8e-4 (the cancelling windings of `clamp` (c); 6.4e-5 on `dense`, <= 1.3e-5 elsewhere), g_disp 3.6e-5, g_cam_T 2.2e-7, g_light_pos 8.2e-6
(generic frames).  e_blocks of g_light_pos on `full`, one workgroup, same inputs: 4.1e-8, 9.5e-8, 9.7e-8, 1.9e-7 in four runs (e_chain 7.6e-8 in all)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import _chain_ref as C
from tests.test_gpu_building_blocks import DEV, FIVE, U, _L, _cond, _d, _f32, _gen, _keep_alive, _worst  # noqa: F401 (_keep_alive: autouse)

pytestmark = pytest.mark.gpu
MM = _f32(1e-3)                  # the kernels' millimetre -> metre factor
S, FOCAL = 100, _f32(446.4)      # S not a power of two
SHADOW_ONLY = ("centroid", "light_R", "light_T", "ndc_l")
FWD_SHAPES = dict(joints_m="J3", vs="V3", n1="V3", il1="V", vd="V3", n2="V3", il2="V", ndc_c="V3", centroid="3", light_R="9", light_T="3", ndc_l="V3")
COT_SCALE = dict(g_ndc_c=1e-3, g_ndc_l=1e-3, g_n2=1e-3, g_vd=1e-2, g_joints_m=1e-2, g_light_R=1e-3, g_light_T=1e-3)
DISP_SCALE = 1e-3


# ----------------------------------------------------------------------------------------------------------------------------------
# meshes
# ----------------------------------------------------------------------------------------------------------------------------------
def _numpy_topology(faces0, V0, subdivide):
    """the chain's tables without normal_consistency_pairs (not needed here, and not meant for non-manifold meshes)"""
    from harp_amd.topology import csr_from_pairs, subdivide_topology
    faces0 = np.asarray(faces0, np.int64)
    if subdivide:
        edges0, faces = subdivide_topology(faces0, V0)
    else:
        edges0, faces = np.zeros((0, 2), np.int64), faces0
    E0 = len(edges0)
    V = V0 + E0
    vf_off, vf_idx = csr_from_pairs(faces.reshape(-1), np.arange(faces.size), V)
    srow = np.concatenate([edges0[:, 0], edges0[:, 1]])
    scol = np.concatenate([np.arange(E0), np.arange(E0)]) + V0
    sub_off, sub_idx = csr_from_pairs(srow, scol, V0)
    return dict(edges0=edges0.astype(np.int32), faces=faces.astype(np.int32), vf_off=vf_off, vf_idx=vf_idx, sub_off=sub_off, sub_idx=sub_idx,
                n_verts0=V0, n_verts=V)


def _components(faces, V):
    lab = np.arange(V)
    while True:
        new = lab.copy()
        np.minimum.at(new, faces.reshape(-1), np.repeat(lab[faces].min(1), 3))
        if (new == lab).all():
            return [np.nonzero(lab == k)[0] for k in np.unique(lab)]
        lab = new


def _fan(n):
    """closed fan of n faces round vertex 0 (the apex of a shallow cone), positions in units of the rim radius"""
    a = 2 * math.pi * np.arange(n) / n
    P = np.concatenate([[[0.0, 0.0, 0.4]], np.stack([np.cos(a), np.sin(a), 0 * a], 1)])
    return np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)]), P


def _mesh_tables(name):
    """(faces0, base positions (V0,3) in millimetres about the origin, subdivide, through synth.build_*)"""
    if name == "tri":
        return np.array([[0, 1, 2]]), np.array([[-30.0, -20.0, 5.0], [40.0, -10.0, -5.0], [0.0, 35.0, 10.0]]), True, True
    if name == "five":
        P = np.array([(0, 0, 1), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (1, 1, -0.5)], np.float64) * 40.0
        return FIVE, P, True, True
    if name in ("hub", "hub_raw"):
        f, P = _fan(12)
        return f, P * 50.0, name == "hub", True
    if name == "clamp":
        # the `five` fan + the clamp cases (b), (c), (d) of the building-block tests' _edge_mesh() without its isolated vertex (a), hand-sized:
        # (b) a face with two coincident corners (its normal is exactly 0 in float64), (c) a face and its opposite-wound copy (the two
        # normals cancel), (d) a face 0.1 mm on a side (|N| = 1e-8 m^2: below the 1e-6 clamp, not zero)
        P5 = np.array([(0, 0, 1), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (1, 1, -0.5)], np.float64) * 40.0
        Pb = np.array([(30, -70, 0), (30, -70, 0), (-30, -10, 20)], np.float64)
        Pc = np.array([(-80, 0, 0), (-60, 0, 10), (-80, 25, 0)], np.float64)
        Pd = np.array([(60, 60, 10), (60.1, 60, 10), (60, 60.1, 10)], np.float64)
        f = np.concatenate([FIVE, [[6, 7, 8], [9, 10, 11], [9, 11, 10], [12, 13, 14]]])
        return f, np.concatenate([P5, Pb, Pc, Pd]), False, False
    if name == "full":
        # 30 x 33 cells: 31 x 34 = 1054 vertices, 30*34 + 31*33 + 30*33 = 3033 edges; + one quad (4 vertices, 5 edges): V0 + E0 = 4096
        nx, ny = 31, 34
        ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        x, y = 3.0 * (ix - 15), 3.0 * (iy - 16.5)
        P = np.stack([x, y, 8.0 * np.sin(x / 15.0) * np.cos(y / 12.0)], -1).reshape(-1, 3)
        vid = lambda i, j: i * ny + j
        f = []
        for i in range(nx - 1):
            for j in range(ny - 1):
                f += [[vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)]]
        q = nx * ny
        Pq = np.array([(60, -60, 20), (75, -60, 22), (75, -45, 20), (60, -45, 25)], np.float64)
        f += [[q, q + 1, q + 2], [q, q + 2, q + 3]]
        return np.array(f), np.concatenate([P, Pq]), True, True
    if name == "dense":
        # 80 points on a sphere (Fibonacci spiral); one face per pair (i, j) with a third vertex: every pair of vertices is an edge
        n = 80
        k = np.arange(n) + 0.5
        ph, th = np.arccos(1 - 2 * k / n), math.pi * (1 + 5 ** 0.5) * k
        P = 50.0 * np.stack([np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph)], 1)
        f = []
        for i in range(n):
            for j in range(i + 1, n):
                t = (j + 1 + i % 7) % n
                while t in (i, j):
                    t = (t + 1) % n
                f.append([i, j, t])
        return np.array(f), P, True, False
    assert name in ("mano", "arm")
    from harp_amd import synth
    tpl = synth.load_template("hand" if name == "mano" else "arm")
    P = tpl["base_verts"].astype(np.float64) * 1000.0
    return tpl["faces0"], P - P.mean(0), True, True


NJ_OF = dict(tri=1, hub=341)      # every other mesh: 21
CAM_DIST = dict(arm=0.8)          # every other mesh: 0.5 m in front of the camera


@functools.lru_cache(maxsize=None)
def _case(name, B):
    """host side of one case: tables, float32 inputs, connected components.  Cached, never modified."""
    from harp_amd import synth
    faces0, P0, subdivide, through_synth = _mesh_tables(name)
    V0 = P0.shape[0]
    if through_synth:
        topo = (synth.build_topology if subdivide else synth.build_raw_topology)(faces0, V0)
    else:
        topo = _numpy_topology(faces0, V0, subdivide)
    V, E0 = int(topo["n_verts"]), topo["edges0"].shape[0]
    assert V == V0 + E0 and int(np.diff(topo["vf_off"]).min()) >= 1          # the documented precondition: every vertex lies in a face
    faces = np.asarray(topo["faces"], np.int64)
    fc = np.asarray(topo["vf_idx"], np.int64)
    vf_tri = np.concatenate([faces[fc // 3], (fc % 3)[:, None]], 1).astype(np.int32)            # as ops.DeviceTopology
    NJ = NJ_OF.get(name, 21)
    g = _gen(V * 7 + B)
    base = torch.from_numpy(P0)
    frames = [base * (1.0 + 0.1 * b) + torch.tensor([10.0 - 8.0 * b, -20.0 + 5.0 * b, 450.0 + 20.0 * b], dtype=torch.float64) for b in range(B)]
    verts_mm = torch.stack(frames).float()
    joints_mm = (torch.randn(B, NJ, 3, generator=g) * 50.0).float()
    cam_R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, dtype=torch.float64))[0].float()
    if B > 1:
        cam_R[0] = torch.diag(torch.tensor([-1.0, -1.0, 1.0]))
    centre = verts_mm.double().mean(1) * 1e-3
    # the mesh 0.5 m in front of the camera whatever the rotation: view z within 0.5 +- 0.15
    # (the arm reaches 0.34 m from its centroid: 0.8 m)
    cam_T = (torch.tensor([0.01, -0.02, CAM_DIST.get(name, 0.5)], dtype=torch.float64) - torch.bmm(centre[:, None], cam_R.double())[:, 0]).float()
    light = (centre + torch.tensor([[0.4, -0.8, -0.3], [-0.5, 0.6, 0.4], [0.3, 0.7, -0.6]], dtype=torch.float64)[:B]).float()
    disp = (torch.randn(V, generator=g) * DISP_SCALE).float()
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32)))
    pad = lambda t: t if t.numel() else torch.zeros((1,) + tuple(t.shape[1:]), dtype=torch.int32)    # empty tables still need a pointer
    tables = dict(edges0=pad(i32(topo["edges0"])), vf_off=i32(topo["vf_off"]), vf_tri=i32(vf_tri), vf_idx=i32(topo["vf_idx"]),
                  sub_off=i32(topo["sub_off"]), sub_idx=pad(i32(topo["sub_idx"])), faces=i32(faces))
    return dict(name=name, B=B, V0=V0, E0=E0, V=V, NJ=NJ, faces_np=faces.astype(np.int32), edges0_np=np.asarray(topo["edges0"], np.int64).reshape(-1, 2),
                vf_off_np=np.asarray(topo["vf_off"]), tables=tables, verts_mm=verts_mm, joints_mm=joints_mm, cam_R=cam_R, cam_T=cam_T, light=light,
                disp=disp, comps=_components(faces, V), vertical=1 if B > 1 else None, P0=P0)


def _assert_property(cs):
    """the path each mesh is there for, asserted from its tables"""
    name, V, V0, E0 = cs["name"], cs["V"], cs["V0"], cs["E0"]
    per = (V + 3) // 4
    if name == "tri":
        assert (V0, E0, V) == (3, 3, 6) and 3 * per >= V and V % 4 == 2            # wide part 3 owns no vertex
    elif name == "five":
        assert (V0, E0, V) == (6, 10, 16)
    elif name == "hub":
        assert int(np.diff(cs["vf_off_np"]).max()) == 12 and V % 4 == 1            # valence 12 > kPre = 8 (the pre-fetch's tail loop)
    elif name == "hub_raw":
        assert E0 == 0 and V == V0 == 13 and int(np.diff(cs["vf_off_np"]).max()) == 12
    elif name == "clamp":
        assert E0 == 0 and V == 15 and V % 4 == 3
    elif name == "full":
        assert (V0, E0) == (1054 + 4, 3033 + 5) and V == 4096 == _L()[0].harp_mesh_chain_max_vertices() and len(cs["comps"]) == 2
    elif name == "dense":
        assert V0 == 80 and E0 == 80 * 79 // 2 == 3160 and E0 > 3 * 1024 and V == 3240
    elif name == "arm":
        assert (V0, E0, V) == (1026, 3057, 4083) and per == 1021 and V % 4 == 3   # the SMPL-X arm template: the largest production mesh
    else:
        assert (V0, V) == (778, 3093)


CASES = [(m, B) for m in ("tri", "five", "hub", "hub_raw", "clamp") for B in (1, 3)] + [("full", 1), ("dense", 1), ("mano", 1), ("arm", 1)]


# ----------------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _shape(cs, code):
    return {"J3": (cs["B"], cs["NJ"], 3), "V3": (cs["B"], cs["V"], 3), "V": (cs["B"], cs["V"]), "3": (cs["B"], 3), "9": (cs["B"], 9)}[code]


class _Dev:
    """device copies of a case's inputs and tables + NaN-filled forward outputs; struct() mirrors them into a harp_mesh_chain"""

    def __init__(self, cs, light=None):
        self.cs = cs
        self.t = {k: _d(v) for k, v in cs["tables"].items()}
        self.t.update(disp=_d(cs["disp"]), verts_mm=_d(cs["verts_mm"]), joints_mm=_d(cs["joints_mm"]), cam_R=_d(cs["cam_R"].reshape(-1, 9)),
                      cam_T=_d(cs["cam_T"]), light_pos=_d(cs["light"] if light is None else light))
        for k, code in FWD_SHAPES.items():
            self.t[k] = torch.full(_shape(cs, code), float("nan"), device=DEV)

    def struct(self, shadow, ng=0, light_only=0, **over):
        from harp_amd import _lib
        cs = self.cs
        ch = _lib.MeshChain(B=cs["B"], V0=cs["V0"], E0=cs["E0"], NJ=cs["NJ"], S=S, focal=FOCAL, shadow=shadow, has_normal_grad=ng, light_only=light_only)
        for n, ty in _lib.MeshChain._fields_:
            if ty is ctypes.c_void_p and n in self.t:
                setattr(ch, n, _lib.ptr(self.t[n]))
        for k, v in over.items():
            setattr(ch, k, v)
        return ch


def _ws(cs):
    L = _L()[0]
    return torch.empty(L.harp_mesh_chain_wide_ws_floats(cs["B"], cs["V"]), dtype=torch.float32, device=DEV)


def _forward(cs, wide, shadow=1, clear=0):
    """runs the forward of one form; with a `vertical` frame, twice: the light of that frame is put exactly above the centroid the first
    run wrote (the centroid does not depend on the light), so light - centroid = (0, 0.7, 0) in float32 whatever the summation order"""
    L, p, st, ck = _L()
    light = cs["light"]
    for _ in range(2 if (cs["vertical"] is not None and shadow) else 1):
        d = _Dev(cs, light)
        d.ws = _ws(cs)
        g = _gen(31)
        d.t["g_vd"] = _d(torch.randn(cs["B"], cs["V"], 3, generator=g))
        d.t["g_joints_m"] = _d(torch.randn(cs["B"], cs["NJ"], 3, generator=g))
        d.pre = {k: d.t[k].clone() for k in ("g_vd", "g_joints_m")}
        ch = d.struct(shadow)
        if wide:
            ck(L.harp_mesh_chain_fwd_wide(ctypes.byref(ch), clear, p(d.ws), st()), "mesh_chain_fwd_wide")
        else:
            ck(L.harp_mesh_chain_fwd(ctypes.byref(ch), st()), "mesh_chain_fwd")
        torch.cuda.synchronize()
        if cs["vertical"] is not None and shadow:
            light = light.clone()
            light[cs["vertical"]] = d.t["centroid"][cs["vertical"]].cpu() + torch.tensor([0.0, 0.7, 0.0])
    d.light = light
    return d


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _project_bound(v64, R64, T64, ndc_ref):
    """the bound of harp_project_fwd (test_project_against_float64) with the principal point at the centre"""
    absX = torch.bmm(v64.abs(), R64.abs()) + T64.abs()[:, None]
    Z = ndc_ref[..., 2:]
    half = S / 2.0
    bxy = 8 * U * (FOCAL * absX[..., :2] / Z * (1 + absX[..., 2:] / Z) + 2 * half + half) / half
    return torch.cat([bxy, 4 * U * absX[..., 2:]], -1)


# ----------------------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------------------
def _check_forward_stages(tag, cs, out32, light, general_rotation=True):
    """every forward output of a chain (out32: FWD_SHAPES -> float32 CPU tensors) against the float64 reference, stage by stage, each stage
    from the kernel's own output of the stage before.  cs: verts_mm, joints_mm, cam_R (B,3,3), cam_T, disp (float32, what the chain read),
    faces_np, edges0_np, vf_off_np, name, comps, vertical, B, V; light (B,3): the light positions the chain read.  Shared with
    tests/test_gpu_step_front_back.py, whose chain runs inside the fused front behind the camera convention's fixed rotation
    (general_rotation = False: the assertion that the last frame's rotation is a general one does not apply)."""
    mesh, B = cs["name"], cs["B"]
    faces = torch.from_numpy(cs["faces_np"]).long()
    edges0 = torch.from_numpy(cs["edges0_np"]).long()
    deg = int(np.diff(cs["vf_off_np"]).max())
    o = {k: out32[k].double() for k in FWD_SHAPES}
    assert all(torch.isfinite(v).all() for v in o.values()), tag                  # every element of every output written (NaN pre-fill)
    # ---- metres + SubdivideMeshes: s v is one rounding, a midpoint (s a + s c) * 0.5 three, each within U of |s a| + |s c|
    assert torch.equal(out32["joints_m"], cs["joints_mm"] * torch.tensor(MM, dtype=torch.float32)), tag
    a64 = cs["verts_mm"].double().abs()
    mag = torch.cat([MM * a64, MM * (a64[:, edges0[:, 0]] + a64[:, edges0[:, 1]])], 1)
    _worst(tag + " vs", (o["vs"] - C.subdivide(cs["verts_mm"].double(), edges0, MM)).abs(), 2 * U * mag + 1e-300)
    # ---- the two normal passes, each from the kernel's own positions: ((3 deg + 8) cond + 4) U; il = 0 exactly under the clamp
    for pos, n, il in (("vs", "n1", "il1"), ("vd", "n2", "il2")):
        n_ref, il_ref = C.normals(o[pos], faces)
        cond, Nlen = _cond(o[pos], cs["faces_np"])
        clamped = Nlen <= 1e-6
        assert torch.equal(o[il] == 0, clamped), (tag, il)
        nb = ((3 * deg + 8) * cond + 4) * U
        _worst(f"{tag} {n}", (o[n] - n_ref).abs(), nb[..., None] + 1e-300)
        _worst(f"{tag} {il}", (o[il] - il_ref).abs(), nb * il_ref + 1e-300)           # 1 / |N|: the same relative error as N
        if mesh == "clamp":
            c_idx = np.concatenate(cs["comps"][1:])
            assert len(cs["comps"]) == 4 and clamped[:, c_idx].all() and not clamped[:, cs["comps"][0]].any(), tag
            assert (Nlen[:, 12:] > 1e-10).all() and (Nlen[:, 6:9] == 0).all()         # (d) non-zero below the clamp, (b) exactly zero
        else:
            assert not clamped.any() or mesh == "mano", tag
        if pos == "vs":
            # ---- displacement from the kernel's vs and n1: v + n d, two roundings of |v| + |n d|
            nd = o["n1"] * cs["disp"].double()[None, :, None]
            _worst(tag + " vd", (o["vd"] - (o["vs"] + nd)).abs(), 2 * U * (o["vs"].abs() + nd.abs()) + 1e-300)
    # ---- camera view from the kernel's vd, with a general rotation
    R64, T64 = cs["cam_R"].double(), cs["cam_T"].double()
    ndc_ref = C.project(o["vd"], R64, T64, S, FOCAL)
    assert ndc_ref[..., 2].min() > 0.3
    if B > 1 or not general_rotation:
        assert torch.equal(cs["cam_R"][0], torch.diag(torch.tensor([-1.0, -1.0, 1.0])))
    if general_rotation:
        assert (cs["cam_R"][-1] - cs["cam_R"][-1].T).abs().max() > 0.1                # a general rotation: a transposed index would show
    _worst(tag + " ndc_c", (o["ndc_c"] - ndc_ref).abs(), _project_bound(o["vd"], R64, T64, ndc_ref))
    # ---- centroid from the kernel's vd.  harp_centroid's bound: (ceil(V / 256) + 10) roundings of sum |v| / V (here the tree is <= 3 adds
    # per lane, 6 wave levels, 16 wave sums or four part sums, the division: at most 26 roundings, usually far fewer non-zero terms)
    V = cs["V"]
    _worst(tag + " centroid", (o["centroid"] - o["vd"].mean(1)).abs(), (math.ceil(V / 256) + 10) * U * o["vd"].abs().mean(1))
    # ---- light camera from the kernel's centroid.  No building-block bound in U exists for it: 2e-6 (R) / 5e-6 (T, |pos| <= 2.4 m) are the
    # empirical constants at which the shared device function light_cam is already pinned by
    # test_gpu_parity.py::test_light_camera_incl_look_at_replacement_branch (34 U of a unit axis, 84 U of T), not derived ones
    lR_ref, lT_ref = C.light_camera(o["centroid"], light.double(), S, FOCAL)
    lR = o["light_R"].view(B, 3, 3)
    _worst(tag + " light_R", (lR - lR_ref).abs(), torch.tensor(2e-6))
    _worst(tag + " light_T", (o["light_T"] - lT_ref).abs(), torch.tensor(5e-6))
    if cs["vertical"] is not None:
        b = cs["vertical"]
        assert (lR[b, :, 0] == 0).all() and (lR[b, :, 1] == 0).all() and (lR_ref[b, :, :2] == 0).all(), tag      # x = y = 0, like the reference
        assert (light[b] - out32["centroid"][b])[[0, 2]].abs().max() == 0
    # ---- light view from the kernel's vd, light_R, light_T
    ndl_ref = C.project(o["vd"], lR, o["light_T"], S, FOCAL)
    assert ndl_ref[..., 2].min() > 1.0
    _worst(tag + " ndc_l", (o["ndc_l"] - ndl_ref).abs(), _project_bound(o["vd"], lR, o["light_T"], ndl_ref))


@pytest.mark.parametrize("wide", [False, True], ids=["one_wg", "wide"])
@pytest.mark.parametrize("mesh,B", CASES)
def test_mesh_chain_forward_stage_by_stage_against_float64(mesh, B, wide):
    cs = _case(mesh, B)
    _assert_property(cs)
    tag = f"chain_fwd {mesh} B={B} {'wide' if wide else 'one_wg'}"
    d = _forward(cs, wide, shadow=1)
    _check_forward_stages(tag, cs, {k: d.t[k].cpu() for k in FWD_SHAPES}, d.light)
    # ---- g_vd / g_joints_m are inputs of this call (clear_grads = 0): untouched
    for k in ("g_vd", "g_joints_m"):
        assert torch.equal(_bits(d.t[k]), _bits(d.pre[k])), (tag, k)
    # ---- shadow = 0: the same camera-view outputs, the four shadow-only outputs keep their NaN pre-fill bit for bit
    d0 = _forward(cs, wide, shadow=0, clear=1 if wide else 0)
    nan_bits = _bits(torch.full((1,), float("nan")))[0]
    for k in FWD_SHAPES:
        if k in SHADOW_ONLY:
            assert (_bits(d0.t[k]) == nan_bits).all(), (tag, k)
        else:
            assert torch.equal(_bits(d0.t[k]), _bits(d.t[k])), (tag, k)
    if wide:                                                                          # clear_grads = 1 zeroes the two gradient segments
        assert (d0.t["g_vd"] == 0).all() and (d0.t["g_joints_m"] == 0).all() and d0.pre["g_vd"].abs().min() > 0, tag


# ----------------------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------------------
def _cotangents(cs):
    g = _gen(9)
    shapes = dict(g_ndc_c="V3", g_ndc_l="V3", g_n2="V3", g_vd="V3", g_joints_m="J3", g_light_R="9", g_light_T="3")
    cot = {k: (torch.randn(_shape(cs, shapes[k]), generator=g) * COT_SCALE[k]).float() for k in shapes}
    if cs["vertical"] is not None:
        # In the frame whose light stands on the vertical, the x and y columns of light_R are exactly 0 and their gradient passes three
        # times through the g / eps = 1e5 g branch of the clamped normalisations: a gain of 1e15 onto g_light_pos and, through the centroid,
        # onto every vertex.  A float32 sum over the vertices feeding those columns would turn the comparison into that of two single
        # rounding errors times 1e15, for which no fixed factor holds; so the light view's cotangent has only its depth component there
        # (the sums into the x / y columns and T.x / T.y are then exact zeros, the shader's share g_light_R / g_light_T still takes the
        # degenerate branch), and the other frames carry the full cotangent.
        cot["g_ndc_l"][cs["vertical"], :, :2] = 0.0
    return cot


def _reference_grads(cs, cot, light, centroid, shadow, ng):
    """float64 VJP through the reference at the float32 inputs, the light camera evaluated at the centroid the float32 backward reads"""
    leaves = [t.double().requires_grad_() for t in (cs["verts_mm"], cs["joints_mm"], cs["cam_T"], light, cs["disp"])]
    out = C.chain(leaves[0], leaves[1], cs["cam_R"].double(), leaves[2], leaves[3], leaves[4], torch.from_numpy(cs["edges0_np"]).long(),
                  torch.from_numpy(cs["faces_np"]).long(), S, FOCAL, mm=MM, centroid_value=centroid)
    pairs = [("ndc_c", "g_ndc_c"), ("vd", "g_vd"), ("joints_m", "g_joints_m")]
    if shadow:
        pairs += [("ndc_l", "g_ndc_l"), ("light_R", "g_light_R"), ("light_T", "g_light_T")]
    if ng:
        pairs += [("n2", "g_n2")]
    total = sum((out[a].reshape(cot[b].shape) * cot[b].double()).sum() for a, b in pairs)
    gr = torch.autograd.grad(total, leaves, allow_unused=True)
    return dict(zip(("g_v0", "g_joints_mm", "g_cam_T", "g_light_pos", "g_disp"), gr))


def _blocks_backward(cs, d, cotd, pre, shadow, ng):
    """the stand-alone float32 sequence on the same inputs (the forward outputs of the form under test), accumulating like the chain"""
    L, p, st, ck = _L()
    B, V, V0 = cs["B"], cs["V"], cs["V0"]
    t = d.t
    G = cotd["g_vd"].clone()
    out = {k: _d(pre[k]) for k in ("g_light_pos", "g_cam_T", "g_disp")}
    if shadow:
        gR, gT = cotd["g_light_R"].clone(), cotd["g_light_T"].clone()
        ck(L.harp_project_bwd(p(t["vd"]), p(t["light_R"]), p(t["light_T"]), p(cotd["g_ndc_l"]), B, V, FOCAL, S, p(G), p(gR), p(gT), st()), "project_bwd")
    ck(L.harp_project_bwd(p(t["vd"]), p(t["cam_R"]), p(t["cam_T"]), p(cotd["g_ndc_c"]), B, V, FOCAL, S, p(G), None, p(out["g_cam_T"]), st()), "project_bwd")
    if shadow:
        gc = torch.empty(B, 3, device=DEV)
        ck(L.harp_light_setup_bwd(p(t["centroid"]), p(t["light_pos"]), p(gR), p(gT), B, V, p(out["g_light_pos"]), p(gc), p(G), st()), "light_setup_bwd")
    tmp = torch.empty(B, V, 3, device=DEV)
    if ng:
        ck(L.harp_vertex_normals_bwd(p(t["vd"]), p(t["faces"]), p(t["vf_off"]), p(t["vf_idx"]), B, V, p(t["n2"]), p(t["il2"]), p(cotd["g_n2"]), p(tmp), p(G),
                                     st()), "normals_bwd")
    g_n1 = torch.empty(B, V, 3, device=DEV)
    ck(L.harp_displace_bwd(p(G), p(t["n1"]), p(t["disp"]), B, V, p(g_n1), p(out["g_disp"]), st()), "displace_bwd")
    ck(L.harp_vertex_normals_bwd(p(t["vs"]), p(t["faces"]), p(t["vf_off"]), p(t["vf_idx"]), B, V, p(t["n1"]), p(t["il1"]), p(g_n1), p(tmp), p(G), st()),
       "normals_bwd")
    out["g_v0"] = torch.full((B, V0, 3), float("nan"), device=DEV)
    ck(L.harp_subdivide_bwd(p(G), p(t["sub_off"]), p(t["sub_idx"]), B, V0, V, MM, p(out["g_v0"]), st()), "subdivide_bwd")
    torch.cuda.synchronize()
    return out


KSUM = 8 + 27      # roundings of one camera sum: 8 in a term (harp_project_bwd's count), then <= 4 adds per lane, 6 wave levels, 16 wave sums
                   # (one workgroup) or 1 + 6 + 16 and four part sums (wide): <= 27


def _camera_sums(vd, R, T, g_ndc):
    """float64 projection backward of every vertex summed per frame: the 9 + 3 camera sums (B,12) [p_i g_j row-major | g] and the same sums
    of magnitudes, where gZ = g_z - (gX X + gY Y) / Z counts |g_z| + (|gX X| + |gY Y|) / Z"""
    view = torch.bmm(vd, R) + T[:, None]
    X, Y, Z = view.unbind(-1)
    k = FOCAL / (Z * (S / 2.0))
    gX, gY = g_ndc[..., 0] * k, g_ndc[..., 1] * k
    gv = torch.stack([gX, gY, g_ndc[..., 2] - (gX * X + gY * Y) / Z], -1)
    av = torch.stack([gX.abs(), gY.abs(), g_ndc[..., 2].abs() + ((gX * X).abs() + (gY * Y).abs()) / Z.abs()], -1)
    B = vd.shape[0]
    sums = torch.cat([torch.einsum("bvi,bvj->bij", vd, gv).reshape(B, 9), gv.sum(1)], 1)
    mags = torch.cat([torch.einsum("bvi,bvj->bij", vd.abs(), av).reshape(B, 9), av.sum(1)], 1)
    return sums, mags


def _scalar_sum_bounds(cs, d, cot, pre, shadow):
    """g_cam_T and g_light_pos are sums over all vertices of a frame, three numbers each.  The building blocks form them with atomics
    across workgroups, in an order that changes from run to run, so their error is no yardstick for three numbers (measured on the `full`
    mesh: e_blocks of g_cam_T between 1.1e-8 and 1.2e-7, of g_light_pos between 8.7e-8 and 1.9e-7 over four runs of the same inputs, the
    fused kernel's own error constant).  They get a derived float32 bound instead, like the centroid: the float64 value of the same sums
    from the kernel's own vd / light_R / light_T / centroid, KSUM roundings of the sum of magnitudes, and for g_light_pos that error
    carried through |Jacobian| of the light camera plus 48 roundings for light_cam_bwd itself (its longest dependency chain: four
    normalisation backwards of ~9 roundings each, the totals before and the 1.5 / |d| scaling after; taken of the frame's largest
    component, since its cross products and projections mix the three)."""
    o = {k: d.t[k].cpu().double() for k in ("vd", "light_R", "light_T", "centroid")}
    B = cs["B"]
    out = {}
    sc, mc = _camera_sums(o["vd"], cs["cam_R"].double(), cs["cam_T"].double(), cot["g_ndc_c"].double())
    p0 = pre["g_cam_T"].double()
    out["g_cam_T"] = (sc[:, 9:], KSUM * U * mc[:, 9:] + 2 * U * (p0.abs() + sc[:, 9:].abs()) + 1e-300)
    if shadow:
        sl, ml = _camera_sums(o["vd"], o["light_R"].view(B, 3, 3), o["light_T"], cot["g_ndc_l"].double())
        share = torch.cat([cot["g_light_R"], cot["g_light_T"]], 1).double()
        w = share + sl                                                               # totals of dL/d(light_R, light_T)
        dw = KSUM * U * ml + U * (share.abs() + sl.abs())
        light = d.light.double()

        def cam(lp):
            lR, lT = C.light_camera(o["centroid"], lp, S, FOCAL)
            return torch.cat([lR.reshape(B, 9), lT], 1)
        J = torch.autograd.functional.jacobian(cam, light)                           # (B,12,B,3): frames do not mix
        J = torch.stack([J[b, :, b] for b in range(B)])                              # (B,12,3)
        want = torch.einsum("bk,bkc->bc", w, J)
        p0 = pre["g_light_pos"].double()
        own = 48 * U * torch.einsum("bk,bkc->bc", w.abs(), J.abs()).max(1, keepdim=True).values   # cross products mix the three components
        bound = torch.einsum("bk,bkc->bc", dw, J.abs()) + own + 2 * U * (p0.abs() + want.abs()) + 1e-300
        out["g_light_pos"] = (want, bound)
    return out


def _compare(tag, cs, got, blk, ref, pre, keys, worst, sums=None):
    """per output and connected component: e_chain <= 4 e_blocks + 8 U |reference|_max, every reference gradient non-zero; the outputs in
    `sums` (_scalar_sum_bounds) are held to their derived bound instead, both errors against the float64 VJP still printed"""
    for k in keys:
        if k == "g_v0":
            pieces = [(f" piece {c[0]}..", (slice(None), c[c < cs["V0"]])) for c in cs["comps"]]
        elif k == "g_disp":
            pieces = [(f" piece {c[0]}..", (c,)) for c in cs["comps"]]
        else:
            pieces = [("", (slice(None),))]
        p0 = pre[k].double() if k in pre else 0.0
        for name, ix in pieces:
            want = ref[k][ix]
            rmax = want.abs().max().item()
            # non-vacuous; the one exception: N = 0 exactly on the clamped components (b) and (c), so n1 = 0 and g_disp = g . n1 = 0
            assert rmax > 0 or (cs["name"] == "clamp" and k == "g_disp" and name in (" piece 6..", " piece 9..")), (tag, k, name)
            e_chain = ((got[k].cpu().double() - p0)[ix] - want).abs().max().item()
            e_blocks = ((blk[k].cpu().double() - p0)[ix] - want).abs().max().item()
            bound = 4 * e_blocks + 8 * U * rmax
            print(f"[{tag} {k}{name}] e_chain {e_chain:.3e} e_blocks {e_blocks:.3e} |ref|max {rmax:.3e}: e_chain / |ref| {e_chain / max(rmax, 1e-300):.2e}, "
                  f"{e_chain / (bound + 1e-300):.3f} of 4 e_blocks + 8 U |ref|")
            if rmax > 0:
                worst[k] = max(worst.get(k, 0.0), e_chain / rmax)
            if sums and k in sums:
                _worst(f"{tag} {k} (derived)", (got[k].cpu().double() - p0 - sums[k][0]).abs(), sums[k][1])
            else:
                assert math.isfinite(e_chain) and e_chain <= bound, (tag, k, name, e_chain, e_blocks, rmax)


@pytest.mark.parametrize("wide", [False, True], ids=["one_wg", "wide"])
@pytest.mark.parametrize("mesh,B", CASES)
def test_mesh_chain_backward_against_float64_and_the_building_blocks(mesh, B, wide):
    L, p, st, ck = _L()
    cs = _case(mesh, B)
    _assert_property(cs)
    V0, NJ = cs["V0"], cs["NJ"]
    d = _forward(cs, wide, shadow=1)
    centroid = d.t["centroid"].cpu().double()
    cot = _cotangents(cs)
    cotd = {k: _d(v) for k, v in cot.items()}
    d.t.update(cotd)
    g = _gen(13)
    pre = {k: torch.randn(s, generator=g) * 1e-3 for k, s in (("g_light_pos", (B, 3)), ("g_cam_T", (B, 3)), ("g_disp", (cs["V"],)))}
    worst = {}
    for shadow, ng in ((1, 1), (0, 0), (1, 0)):
        tag = f"chain_bwd {mesh} B={B} {'wide' if wide else 'one_wg'} shadow={shadow} ng={ng}"
        got = {k: _d(v) for k, v in pre.items()}                                      # (+=): accumulate into random data
        got["g_v0"] = torch.full((B, V0, 3), float("nan"), device=DEV)                # overwritten
        got["g_joints_mm"] = torch.full((B, NJ, 3), float("nan"), device=DEV)
        d.t.update(got)
        ch = d.struct(shadow, ng)
        if wide:
            ck(L.harp_mesh_chain_bwd_wide(ctypes.byref(ch), p(d.ws), st()), "mesh_chain_bwd_wide")
        else:
            ck(L.harp_mesh_chain_bwd(ctypes.byref(ch), st()), "mesh_chain_bwd")
        torch.cuda.synchronize()
        blk = _blocks_backward(cs, d, cotd, pre, shadow, ng)
        ref = _reference_grads(cs, cot, d.light, centroid, shadow, ng)
        assert torch.isfinite(got["g_v0"]).all() and torch.isfinite(got["g_joints_mm"]).all(), tag
        # g_joints_mm = fl(g_joints_m * 1e-3f), bit for bit, and one rounding from the reference
        assert torch.equal(got["g_joints_mm"].cpu(), cot["g_joints_m"] * torch.tensor(MM, dtype=torch.float32)), tag
        _worst(tag + " g_joints_mm", (got["g_joints_mm"].cpu().double() - ref["g_joints_mm"]).abs(), U * ref["g_joints_mm"].abs() + 1e-300)
        assert ref["g_joints_mm"].abs().max() > 0
        keys = ["g_v0", "g_cam_T", "g_disp"] + (["g_light_pos"] if shadow else [])
        sums = _scalar_sum_bounds(cs, d, cot, pre, shadow)
        _compare(tag, cs, got, blk, ref, pre, keys, worst, sums)
        if not shadow:                                                                # shadow only: left alone
            assert torch.equal(_bits(got["g_light_pos"]), _bits(pre["g_light_pos"])), tag
        if mesh == "clamp":
            # the il == 0 branches hand g * 1e6 to the un-normalised normal.  Component (b) (vertices 6..8, edges of 0.085 m) turns that
            # into a position gradient (per metre: 1e3 g_v0) of ~1e6 x 0.085 x the cotangent of the normal: above 1e4 times its scale, which
            # no other path reaches (they give ~20 x the cotangent scales).  With g_n2 that is il2's branch; without, il1's, whose cotangent
            # is g_vd d.  (c)'s two windings cancel exactly and (d)'s edges are 1e-4 m: their gradients are only asserted non-zero above.
            per_metre = 1e3 * ref["g_v0"][0, 6:9].abs().max().item()
            scale = COT_SCALE["g_n2"] if ng else COT_SCALE["g_vd"] * DISP_SCALE
            print(f"[{tag}] clamped component (b): |d/d metres| {per_metre:.3e} = {per_metre / scale:.3e} x the normal's cotangent scale")
            assert per_metre > 1e4 * scale, (tag, per_metre, scale)
        if shadow and ng and not wide:
            # ---- light_only: nothing but g_light_pos (+=) is written, and it is the full backward's light share
            lo = {k: _d(v) for k, v in pre.items()}
            lo["g_v0"] = torch.full((B, V0, 3), float("nan"), device=DEV)
            lo["g_joints_mm"] = torch.full((B, NJ, 3), float("nan"), device=DEV)
            d.t.update(lo)
            ch = d.struct(1, 1, light_only=1)
            ck(L.harp_mesh_chain_bwd(ctypes.byref(ch), st()), "mesh_chain_bwd light_only")
            torch.cuda.synchronize()
            _compare(tag + " light_only", cs, lo, blk, ref, pre, ["g_light_pos"], {}, sums)
            nan_bits = _bits(torch.full((1,), float("nan")))[0]
            assert (_bits(lo["g_v0"]) == nan_bits).all() and (_bits(lo["g_joints_mm"]) == nan_bits).all(), tag
            assert torch.equal(_bits(lo["g_cam_T"]), _bits(pre["g_cam_T"])) and torch.equal(_bits(lo["g_disp"]), _bits(pre["g_disp"])), tag
    print(f"[chain_bwd {mesh} B={B} {'wide' if wide else 'one_wg'}] worst e_chain / |reference|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ----------------------------------------------------------------------------------------------------------------------------------
# argument checks: refused on the host, nothing written
# ----------------------------------------------------------------------------------------------------------------------------------
FWD_REQUIRED = ("edges0", "vf_off", "vf_tri", "disp", "verts_mm", "joints_mm", "cam_R", "cam_T", "joints_m", "vs", "n1", "il1", "vd", "n2", "il2", "ndc_c",
                "light_pos", "centroid", "light_R", "light_T", "ndc_l")
BWD_REQUIRED = ("vf_off", "vf_tri", "disp", "sub_off", "sub_idx", "vd", "vs", "n1", "il1", "cam_R", "cam_T", "g_vd", "g_ndc_c", "g_joints_m", "g_joints_mm",
                "g_v0", "g_cam_T", "g_disp", "n2", "il2", "g_n2", "light_pos", "centroid", "light_R", "light_T", "g_ndc_l", "g_light_R", "g_light_T",
                "g_light_pos")


@pytest.mark.parametrize("wide", [False, True], ids=["one_wg", "wide"])
def test_mesh_chain_refuses_bad_arguments_untouched(wide):
    L, p, st, _ = _L()
    cs = _case("tri", 1)
    d = _Dev(cs)
    ws = _ws(cs)
    outs = list(FWD_SHAPES) + ["g_v0", "g_joints_mm", "g_light_pos", "g_cam_T", "g_disp", "g_vd", "g_joints_m"]
    for k, v in _cotangents(cs).items():
        d.t[k] = _d(v)
    for k, s in (("g_v0", (1, 3, 3)), ("g_joints_mm", (1, cs["NJ"], 3)), ("g_light_pos", (1, 3)), ("g_cam_T", (1, 3)), ("g_disp", (cs["V"],))):
        d.t[k] = torch.full(s, 5.0, device=DEV)
    for k in FWD_SHAPES:
        d.t[k].fill_(5.0)
    before = {k: d.t[k].clone() for k in outs}

    def fwd(ch, w=ws, clear=0):
        return L.harp_mesh_chain_fwd_wide(ctypes.byref(ch), clear, p(w), st()) if wide else L.harp_mesh_chain_fwd(ctypes.byref(ch), st())

    def bwd(ch, w=ws):
        return L.harp_mesh_chain_bwd_wide(ctypes.byref(ch), p(w), st()) if wide else L.harp_mesh_chain_bwd(ctypes.byref(ch), st())
    for k in FWD_REQUIRED:
        assert fwd(d.struct(1, **{k: None})) == 1, k
    for k in BWD_REQUIRED + (() if wide else ("edges0",)):
        assert bwd(d.struct(1, 1, **{k: None})) == 1, k
    # sizes: one vertex past harp_mesh_chain_max_vertices() (the `full` mesh + one base vertex), NJ * 3 > 1024 (341, which the `hub` cases run,
    # is the largest accepted), empty sizes
    full = _case("full", 1)
    assert full["V0"] + 1 + full["E0"] == 4097
    for over in (dict(V0=full["V0"] + 1, E0=full["E0"]), dict(NJ=342), dict(B=0), dict(V0=0), dict(E0=-1)):
        assert fwd(d.struct(1, **over)) == 1 and bwd(d.struct(1, 1, **over)) == 1, over
    assert fwd(d.struct(1, NJ=341, joints_mm=None)) == 1                               # NJ = 341 itself passes the size check (NULL refuses it)
    if wide:                                                                          # the wide forms' own rules
        assert fwd(d.struct(1), w=None) == 1 and bwd(d.struct(1, 1), w=None) == 1     # no scratch
        assert fwd(d.struct(1, g_vd=None), clear=1) == 1 and fwd(d.struct(1, g_joints_m=None), clear=1) == 1
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(_bits(d.t[k]), _bits(before[k])), k

