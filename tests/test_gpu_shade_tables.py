"""The shader backward's gradient exits (csrc/shade_bwd.hip: harp_shade_bwd, wave-autonomous form) against float64, at the edges of their
wave-private tables.  Every exit of that kernel has a fast path and a fallback — vertex table / probe exhaustion, direct-mapped texel table /
second-chance slot / memory atomics, texel records / full list, shadow-tap window / out-of-window atomics — and the hand scene the rest of the
suite runs was what the tables were sized for.  Here synthetic one-layer meshes FORCE each path (every case asserts, from the face-id image
and the reference's per-pixel texel and tap indices, that its path is taken), through `ops.shade` and the raw `harp_shade_args` struct, and
EVERY returned gradient is compared element by element with tests/_shade_ref.py (anchored on the oracle by tests/test_shade_ref_cpu.py):

    |got_i - ref64_i| <= N_i * M_g * 2^-24 + 4 * E32_g + 2^-22 * A_i

N_i pixel contributions to element i, M_g the largest single per-pixel contribution of the group (every wave's fixed-point quantum is at most
2^-23 of its own maximum: half of it per add), A_i the sum of the contributions' magnitudes (float32 accumulation), E32_g = |ref32 - ref64|_inf
of the same restatement evaluated in float32 on the CPU (how ill-conditioned the case's per-pixel arithmetic is — measured on the reference,
never on the kernel; 4 x for the kernel's approximate reciprocals and square roots).  Record form: the texel maps are reduced in double, no
first term.  The cotangent is zeroed on the pixels the reference flags as undecided at float32 precision (at most 2 % of the covered ones);
nothing is masked out of the outputs.  Measured err / bound per case and group, and the mutations these cases catch: docs/NOTEBOOK.md."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _shade_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64

# the table sizes of harp_amd/csrc/shade_bwd.hip
K_VSLOTS = 32            # :73  kVSlots = 1 << SHADE_VSLOTS_LOG2 (:65), vertex table slots per wave
K_VPROBES = 4            # :530 linear probes before a vertex falls through to memory atomics
K_TW, K_TH = 32, 7       # :63  kTW, kTH (SHADE_BWD_TH :61): texel table, slot = (x & 31) + 32 * (y mod 7)
K_TSLOTS = K_TW * K_TH   # :63  224
K_ZW = K_ZH = 16         # :74  kZW, kZH (:68, :71): shadow-tap window
TILE, STRIP = 16, 4      # a workgroup's tile; one wave = 64 consecutive entries of the tile's compacted pixel list = 4 rows of a full tile
FOCAL_PER_S = 1.0


# ----------------------------------------------------------------------------------------------------------------------
# meshes: one layer facing the camera (no depth ties), UVs = the grid's own parametrisation
# ----------------------------------------------------------------------------------------------------------------------
def _bump(x, y, amp):
    return amp * np.sin(3.0 * x + 0.3) * np.cos(2.0 * y + 0.7)


def grid_mesh(nx, ny, x0, x1, y0, y1, amp=0.04, uv=(0.06, 0.94, 0.07, 0.93)):
    xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
    X, Y = np.meshgrid(xs, ys)
    verts = np.stack([X, Y, _bump(X, Y, amp)], -1).reshape(-1, 3)
    I, J = np.meshgrid(np.arange(nx + 1) / nx, np.arange(ny + 1) / ny)
    uvs = np.stack([uv[0] + (uv[1] - uv[0]) * I, uv[2] + (uv[3] - uv[2]) * J], -1).reshape(-1, 2)
    a = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).reshape(-1)
    b, c, d = a + 1, a + nx + 2, a + nx + 1
    faces = np.concatenate([np.stack([a, c, b], 1), np.stack([a, d, c], 1)], 0)          # normals towards -z (the camera's side)
    return verts, faces.astype(np.int64), uvs


def fan_mesh(n=64, centre=(-0.4631, -0.4417), radius=2.3, amp=0.04):
    ang = 2 * np.pi * (np.arange(n) + 0.37) / n
    rim = np.stack([centre[0] + radius * np.cos(ang), centre[1] + radius * np.sin(ang)], -1)
    xy = np.concatenate([np.array([centre]), rim], 0)
    verts = np.concatenate([xy, _bump(xy[:, 0], xy[:, 1], amp)[:, None]], 1)
    k = np.arange(n)
    faces = np.stack([np.zeros(n, np.int64), 1 + (k + 1) % n, 1 + k], 1)
    return verts, faces, 0.5 + xy / 5.2


def join(*meshes):
    vs, fs, us, off = [], [], [], 0
    for v, f, u in meshes:
        vs.append(v)
        fs.append(f + off)
        us.append(u)
        off += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs), np.concatenate(us)


def look_at(pos, at, up=(0.0, 1.0, 0.0)):
    from oracle import p3d_like as P
    Rm = P.look_at_rotation(pos, at, torch.tensor([up], dtype=F64))
    return Rm, -torch.bmm(Rm.transpose(1, 2), pos[:, :, None])[:, :, 0]


HW = 1.06            # half width of the meshes: the image of both cameras is covered


def build_case(name):
    """CPU description of a case: float32 leaves (B = 2, two cameras and lights), topology, the light view's NDC vertices and the cotangent"""
    from oracle import p3d_like as P
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    # S = 32, with two exceptions.  off_grid: 40, for a ragged last tile.  light_zoom: 64 — a 16-px tile seen 3.2 x larger needs a light
    # image wider than 51 px for its 2 304 taps to land on distinct pixels; a 32 x 32 light image has 1 024 pixels in all.
    S, B = {"off_grid": 40, "light_zoom": 64}.get(name, 32), 2
    focal = FOCAL_PER_S * S
    tex_hw, nm_amp = (48, 64), 0.2
    faces_uvs = None
    if name in ("dense", "range", "light_zoom", "light_far"):
        mesh = grid_mesh(48, 48, -HW, HW, -HW, HW, amp=0.0003 if name == "light_far" else 0.04)
    elif name == "one_face":
        mesh = grid_mesh(1, 1, -HW, HW, -HW, HW)
    elif name == "fan":
        mesh = fan_mesh()
    elif name == "tex_minified":
        mesh = grid_mesh(12, 12, -HW, HW, -HW, HW, uv=(0.013, 0.9871, 0.0171, 0.9853))
        tex_hw = (256, 512)
    elif name == "tex_magnified":
        mesh = grid_mesh(12, 12, -HW, HW, -HW, HW, uv=(0.5912, 1.0431, -0.0617, 1.0533))
        tex_hw = (3, 5)
    elif name == "two_charts":
        # the left and the right half of the mesh on charts in opposite corners of the map: the seam column of vertices has two UV rows
        v, f, _ = grid_mesh(12, 12, -HW, HW, -HW, HW)
        seam_x = 0.2713                                     # through the middle of a tile column in both views
        xs = np.linspace(-HW, HW, 13)
        xs[np.argmin(np.abs(xs - seam_x))] = seam_x
        v[:, 0] = np.tile(xs, 13)
        v[:, 2] = _bump(v[:, 0], v[:, 1], 0.04)
        t = (v[:, :2] + HW) / (2 * HW)
        uv_a = np.stack([0.004 + 0.105 * t[:, 0], 0.79 + 0.2 * t[:, 1]], 1)          # chart A: texels x 1..28, y 0..47
        uv_b = np.stack([0.871 + 0.105 * t[:, 0], 0.006 + 0.2 * t[:, 1]], 1)         # chart B: texels x 222..249, y 177..222
        cx_face = v[f][:, :, 0].mean(1)
        Vn = v.shape[0]
        faces_uvs = np.where((cx_face < seam_x)[:, None], f, f + Vn)
        mesh = (v, f, np.concatenate([uv_a, uv_b], 0))
        tex_hw = (224, 256)
    elif name == "off_grid":
        s = 0.0371
        mesh = join(grid_mesh(1, 1, -HW, HW, -HW, s, uv=(0.06, 0.94, 0.07, 0.5)), grid_mesh(48, 24, -HW, HW, s, HW, uv=(0.06, 0.94, 0.5, 0.93)))
    else:
        raise KeyError(name)
    v_np, f_np, uv_np = mesh
    verts = torch.from_numpy(v_np).float()[None].repeat(B, 1, 1).contiguous()
    faces = torch.from_numpy(f_np).long()
    fuv = faces if faces_uvs is None else torch.from_numpy(faces_uvs).long()
    assert P.verts_normals(verts[:1].double(), faces)[..., 2].max() < 0                    # facing the camera
    cam_R = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=F64))[None].repeat(B, 1, 1)
    cam_T = torch.tensor([[0.0131, -0.0213, 2.0], [-0.0271, 0.0173, 2.09]], dtype=F64)
    pp = (S / 2.0, S / 2.0)
    ndc = P.world_to_ndc(verts.double(), cam_R, cam_T, focal, pp, S)[1].float()
    light_pos = torch.tensor([[0.5, -0.4, -1.5], [-0.6, 0.3, -1.7]], dtype=F64)
    centre = torch.zeros(B, 3, dtype=F64)
    if name == "light_zoom":            # the mesh 3.2 x larger than in the camera view, part of it outside the light image
        d = torch.nn.functional.normalize(torch.tensor([[0.2, -0.15, -1.0], [-0.12, 0.1, -1.0]], dtype=F64), dim=-1)
        at = torch.tensor([[-0.26, -0.24, 0.0], [0.27, -0.25, 0.0]], dtype=F64)            # a camera tile wholly inside the light image
        light_R, light_T = look_at(at + d * torch.tensor([[2.0 / 3.2], [2.09 / 3.2]], dtype=F64), at)
    elif name == "light_far":           # the whole mesh about 3 light pixels wide, in the corner of the light image (clamped taps)
        dist = 2.0 * HW * S / 3.0
        # (nearly) planar mesh seen head-on, the light image rolled against the camera's pixel grid: every covered tap has the same shadow-test argument, so the adds on one cell are of one size and sign
        # and their sum really uses the window scale's head room
        d = torch.tensor([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]], dtype=F64)
        light_R, light_T = look_at(centre + d * dist, centre, up=(0.31, 1.0, 0.0))
        light_T = light_T + torch.tensor([[0.5 * dist * (1 - 3.071 / S), 0.5 * dist * (1 - 2.953 / S), 0.0], [-0.5 * dist * (1 - 3.237 / S), 0.5 * dist * (1 - 2.771 / S), 0.0]], dtype=F64)
    else:
        d = torch.nn.functional.normalize(light_pos - centre, dim=-1)
        light_R, light_T = look_at(centre + d * 1.5, centre)
    light_R, light_T = light_R.float(), light_T.float()
    ndc_l = P.world_to_ndc(verts.double(), light_R.double(), light_T.double(), focal, pp, S)[1].float()
    Ht, Wt = tex_hw
    tex = torch.rand(Ht, Wt, 3, generator=g) * 0.6 + 0.2
    nmap = torch.nn.functional.normalize(torch.randn(Ht, Wt, 3, generator=g) * nm_amp + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    cot = torch.rand(B, S, S, 3, generator=g) * 0.8 + 0.2
    if name == "light_far":
        cot = torch.rand(B, S, S, 3, generator=g) * 0.2 + 0.8
    if name == "range":                 # magnitudes 2^-20 .. 1 mixed inside every tile
        cot = torch.exp2(-20.0 * torch.rand(B, S, S, 1, generator=g)) * torch.where(torch.rand(B, S, S, 3, generator=g) < 0.5, -1.0, 1.0)
    return dict(name=name, S=S, B=B, focal=focal, verts=verts, faces=faces, verts_uvs=torch.from_numpy(uv_np).float(), faces_uvs=fuv, ndc=ndc, ndc_l=ndc_l,
                tex=tex, nmap=nmap, light_pos=light_pos.float(), colors=torch.tensor([0.31, 0.33, 0.29, 0.66, 0.7, 0.63, 0.04, 0.03, 0.05]),
                light_R=light_R, light_T=light_T, cot=cot)


# ----------------------------------------------------------------------------------------------------------------------
# the reference side: float64 gradients + per-element bound terms, float32 companion, preconditions
# ----------------------------------------------------------------------------------------------------------------------
def reference(c, face_id, zl, vnormals):
    """everything the comparison needs, from CPU tensors: c["ref"] (computed once per case, shared by its tests, never modified)"""
    src = dict(ndc=c["ndc"], verts=c["verts"], vnormals=vnormals, tex=c["tex"], nmap=c["nmap"], light_pos=c["light_pos"], colors=c["colors"],
               zl=zl, light_R=c["light_R"], light_T=c["light_T"])
    args = (face_id.long(), c["faces"], c["verts_uvs"], c["faces_uvs"], c["S"], c["focal"])
    with torch.no_grad():
        fwd = R.shade({k: v.double() for k, v in src.items()}, args[0], args[1], args[2].double(), *args[3:])
    amb, cov = fwd["ambiguous"], fwd["covered"]
    n_cov, n_amb = int(cov.sum()), int(amb.sum())
    print(f"[{c['name']}] covered {n_cov}, ambiguous {n_amb} ({n_amb / max(n_cov, 1):.4f})")
    assert n_amb <= 0.02 * n_cov, (n_amb, n_cov)
    assert n_cov - n_amb >= 200
    cot = c["cot"] * (~amb)[..., None]
    res, out = R.gradients(src, cot, *args)
    r32, out32 = R.gradients(src, cot, *args, dtype=torch.float32, stats=False)
    e32 = {k: (r32[k].double() - res[k]["ref"]).abs().max().item() for k in res}
    ok = cov & ~amb
    e32["rgb"] = (out32["rgb"].detach().double() - out["rgb"].detach())[ok].abs().max().item()
    return dict(src=src, cot=cot, res=res, e32=e32, rgb=out["rgb"].detach(), ok=ok, cov=cov, amb=amb, ix=out["ix"], active=ok & (cot != 0).any(-1))


def full_tiles(cov):
    """(b, ty, tx) of the fully covered 16x16 tiles"""
    B, S, _ = cov.shape
    n = S // TILE
    t = cov[:, :n * TILE, :n * TILE].reshape(B, n, TILE, n, TILE).all(4).all(2)
    return [tuple(x) for x in torch.nonzero(t).tolist()]


def tile_of(x, b, ty, tx):
    return x[b, ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]


def strips_of(x, b, ty, tx):
    """the four waves' shares of a fully covered tile: rows 4 w .. 4 w + 3.  Exact, not an approximation: with a gradient image the kernel
    compacts the tile's pixels by COVERAGE alone (shade_bwd.hip: act0 = f0 >= 0, ballot, s_list), wave w takes entries [64 w, 64 w + 64) of
    that list, and only afterwards drops the lanes whose cotangent is zero (act && gc != 0) — a zeroed ambiguous pixel keeps its place in the
    list, so the strips of a fully covered tile do not shift.  What such a pixel changes is which lanes of the strip are active (`act`)."""
    t = tile_of(x, b, ty, tx)
    return [t[STRIP * w:STRIP * (w + 1)] for w in range(TILE // STRIP)]


def distinct(x, mask=None):
    x = x.reshape(-1) if mask is None else x[mask]
    return int(torch.unique(x).numel())


def precondition(c, ref):
    """each case's path, asserted from the face-id image and the reference's per-pixel indices"""
    name, ix, cov, act = c["name"], ref["ix"], ref["cov"], ref["active"]
    tiles = full_tiles(cov)
    assert tiles, "no fully covered tile"
    info = {}
    if name in ("dense", "range", "off_grid"):
        per_tile = [distinct(tile_of(ix["vid"], *t)) for t in tiles]
        per_strip = [distinct(s) for t in tiles for s in strips_of(ix["vid"], *t)]
        info = dict(tiles=len(tiles), min_vertices_per_tile=min(per_tile), max_vertices_per_strip=max(per_strip))
        if name != "off_grid":
            assert min(per_tile) > K_VPROBES * K_VSLOTS                       # pigeonhole: some wave of every such tile exhausts its probes
        assert max(per_strip) > K_VSLOTS                                      # ... and at least one wave cannot even hold its vertices
    if name == "range":
        mag = ref["cot"].abs().amax(-1)
        ratio = min((tile_of(mag, *t)[tile_of(act, *t)].max() / tile_of(mag, *t)[tile_of(act, *t)].min()).item() for t in tiles)
        info["min_cot_ratio_per_tile"] = ratio
        assert ratio >= 2.0 ** 15
    if name == "off_grid":
        S = c["S"]
        assert S % TILE != 0 and cov[:, (S // TILE) * TILE:, :].any() and cov[:, :, (S // TILE) * TILE:].any()            # ragged last tile row / column
        fid = ref["face_id"]
        one = [1 for t in tiles for f in strips_of(fid, *t) if distinct(f) == 1]
        info.update(one_face_strips=len(one), ragged=S % TILE)
        assert one
    if name == "one_face":
        fid = ref["face_id"]
        one = [int(tile_of(act, *t).sum()) for t in tiles if distinct(tile_of(fid, *t)) == 1]
        info = dict(tiles=len(tiles), active_pixels_of_the_one_face_tiles=one)
        assert one and max(one) >= 240                                        # full merge, 3 slots, (nearly) 256 pixels into each vertex
    if name == "fan":
        fid = ref["face_id"]
        shared = [distinct(s) for t in tiles for s in strips_of(fid, *t)]     # every face of the fan holds the centre vertex 0
        assert bool((c["faces"] == 0).any(1).all())
        info = dict(max_faces_per_strip_on_vertex_0=max(shared))
        assert max(shared) >= 24
    if name in ("tex_minified", "tex_magnified", "two_charts"):
        key, valid = ix["tex_key"], ix["tex_valid"] & act[..., None]
        slot = (ix["tex_x"] & (K_TW - 1)) + K_TW * (ix["tex_y"] % K_TH)
        per_tile = [distinct(tile_of(key, *t), tile_of(valid, *t)) for t in tiles]
        per_strip = [distinct(k, m) for t in tiles for k, m in zip(strips_of(key, *t), strips_of(valid, *t))]
        info = dict(tiles=len(tiles), min_texels_per_tile=min(per_tile), max_texels_per_tile=max(per_tile), min_texels_per_strip=min(per_strip),
                    max_texels_per_strip=max(per_strip))
        if name == "tex_minified":
            assert min(per_tile) > 4 * K_TSLOTS and max(per_strip) > K_TSLOTS          # conflicts, second chance, memory atomics
        if name == "tex_magnified":
            full = [int(m[..., 0].sum()) for t in tiles for k, m in zip(strips_of(key, *t), strips_of(valid, *t)) if distinct(k, m) <= 4]
            Ht, Wt = c["tex"].shape[:2]
            edge = ((ix["tex_x"] >= Wt) | (ix["tex_y"] >= Ht)).any(-1) & act
            zero_w = ((ix["tex_w"] == 0) & (ix["tex_x"] < Wt) & (ix["tex_y"] < Ht)).any(-1) & act
            info.update(max_lanes_on_four_slots=max(full, default=0), pixels_with_a_corner_beyond_the_map=int(edge.sum()), pixels_with_a_zero_weight=int(zero_w.sum()))
            assert max(full, default=0) >= 60 and int(edge.sum()) > 0 and int(zero_w.sum()) > 0
        if name == "two_charts":
            clash = 0
            for t in tiles:
                for k, s, m in zip(strips_of(key, *t), strips_of(slot, *t), strips_of(valid, *t)):
                    pairs = torch.unique(torch.stack([s[m], k[m]], 1), dim=0)
                    clash += int(pairs.shape[0] - torch.unique(pairs[:, 0]).numel())
            info["texels_sharing_a_primary_slot_in_one_strip"] = clash
            assert clash > 0                                                  # a second texel on a taken slot: the second-chance probe
    if name in ("light_zoom", "light_far"):
        S = c["S"]
        tap, ctr = ix["tap"], ix["tap_centre"]
        per_tile = [distinct(tile_of(tap, *t), tile_of(act, *t)[..., None].expand(-1, -1, 9)) for t in tiles]
        outside, worst_cell = 0, 0
        for t in tiles:
            for tp, a in zip(strips_of(tap, *t), strips_of(act, *t)):
                if not a.any():
                    continue
                tp = tp[a]                                                     # (n, 9)
                ty, tx = tp // S, tp % S
                y0, x0 = ty[:, 0].min(), tx[:, 0].min()                        # the window's anchor: smallest clamped (iy - 1, ix - 1)
                outside += int(((tx - x0 >= K_ZW) | (ty - y0 >= K_ZH)).sum())
                worst_cell = max(worst_cell, int(torch.bincount(tp.reshape(-1)).max()))
        clamped = ((ctr - 1 < 0) | (ctr + 1 > S - 1)).any(-1) & act
        info = dict(min_taps_per_tile=min(per_tile), max_taps_per_tile=max(per_tile), taps_outside_their_window=outside, max_adds_on_one_cell_per_strip=worst_cell, pixels_with_clamped_taps=int(clamped.sum()))
        print(f"[{name}] {info}")
        if name == "light_zoom":
            # (some tile: the tiles that look past the border of the light image clamp most of their taps onto it)
            assert max(per_tile) > 4 * K_ZW * K_ZH and outside > 0 and int(clamped.sum()) > 0
        else:
            assert worst_cell > 64                                             # more adds on one cell than the wave has lanes: clamped taps pile up
    print(f"[{name}] precondition: {info}")
    return info


def bound_ratio(got, r, e32, fixed=True):
    """max over the elements of err / (N M 2^-24 + 4 E32 + 2^-22 A)"""
    err = (got.double().cpu() - r["ref"]).abs()
    bound = (r["N"].double() * r["M"] * 2.0 ** -24 if fixed else 0.0) + 4.0 * e32 + 2.0 ** -22 * r["A"]
    bound = torch.as_tensor(bound, dtype=F64).expand_as(err)
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    return ratio.max().item(), err.max().item()


# ----------------------------------------------------------------------------------------------------------------------
# the device side
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    """the cases built so far in this module (device tensors and references), released at its end"""
    built = {}
    yield built
    built.clear()


def device_case(_cases, name):
    """case + device topology + both rasterisations + the shared reference (built, and its precondition asserted, once per case)"""
    if name in _cases:
        return _cases[name]
    from harp_amd import ops, synth
    c = build_case(name)
    V = c["verts"].shape[1]
    topo = ops.DeviceTopology(synth.build_raw_topology(c["faces"].numpy(), V), c["verts_uvs"].numpy(), c["faces_uvs"].numpy(), DEV)
    S = c["S"]
    face_id, _, _, ws = ops.rasterize_fwd(c["ndc"].to(DEV), topo.faces, S)
    face_id_l, zl, _, ws_l = ops.rasterize_fwd(c["ndc_l"].to(DEV), topo.faces, S)
    vn = ops.vertex_normals(c["verts"].to(DEV), topo).detach()
    torch.cuda.synchronize()
    ref = reference(c, face_id.cpu(), zl.cpu(), vn.cpu())
    ref["face_id"] = face_id.cpu().long()
    precondition(c, ref)
    c.update(topo=topo, d_face_id=face_id, d_ws=ws, d_face_id_l=face_id_l, d_ws_l=ws_l, ref=ref)
    _cases[name] = c
    return c


def device_leaves(c):
    return {k: v.to(DEV).clone().requires_grad_() for k, v in c["ref"]["src"].items()}


GROUPS = ("ndc", "verts", "vnormals", "tex", "nmap", "light_pos", "colors", "zl", "light_R", "light_T")


def check_gradients(c, got, tag, records=False, groups=GROUPS):
    ref = c["ref"]
    worst = {}
    for k in groups:
        r = ref["res"][k]
        assert r["ref"].abs().max() > 0, k
        worst[k], err = bound_ratio(got[k], r, ref["e32"][k], fixed=not (records and k in ("tex", "nmap")))
    print(f"[{c['name']} {tag}] err / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (c["name"], tag, bad)
    return worst


def run_ops_shade(c, monkeypatch, records, cap=None):
    from harp_amd import ops
    monkeypatch.setattr(ops, "TEXEL_RECORDS", records)
    if cap is not None:
        real = ops.texel_record_buffers
        monkeypatch.setattr(ops, "texel_record_buffers", lambda dev, h, w, n: real(dev, h, w, cap))
    t = device_leaves(c)
    rgb = ops.shade(t["ndc"], t["verts"], t["vnormals"], t["tex"], t["nmap"], t["light_pos"], t["colors"], c["d_face_id"], c["d_ws"], c["topo"], c["S"],
                    c["focal"], zl=t["zl"], light_R=t["light_R"], light_T=t["light_T"])
    (rgb * c["ref"]["cot"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return rgb.detach().cpu(), {k: v.grad for k, v in t.items()}


CASES = ("dense", "one_face", "fan", "tex_minified", "tex_magnified", "two_charts", "light_zoom", "light_far", "range", "off_grid")
RECORD_CASES = (("tex_minified", None), ("tex_magnified", None), ("tex_magnified", 4))


@pytest.mark.parametrize("name", CASES)
def test_table_form_gradient_exits_against_float64(name, cases, monkeypatch):
    """the table form (in-kernel texel scatter) through ops.shade: every returned gradient within the derived bound of the float64
    restatement, the forward image too; the case's own path asserted from the face ids and the reference's texel / tap indices"""
    c = device_case(cases, name)
    ref = c["ref"]
    rgb, got = run_ops_shade(c, monkeypatch, records=False)
    ok, cov = ref["ok"], ref["cov"]
    assert torch.equal(rgb[~cov], torch.ones_like(rgb[~cov]))                                           # the exact background elsewhere
    err = (rgb.double() - ref["rgb"]).abs()
    lim = 4.0 * ref["e32"]["rgb"] + 2.0 ** -22 * ref["rgb"].abs().clamp(min=1.0)
    print(f"[{name}] forward image err / bound {(err / lim)[ok].max().item():.3f} (E32 {ref['e32']['rgb']:.2e})")
    assert (err <= lim)[ok].all()
    check_gradients(c, got, "table")
    lr = got["light_R"].cpu()
    assert lr[:, :, :2].abs().max() == 0 and got["light_T"].cpu()[:, :2].abs().max() == 0


@pytest.mark.parametrize("name,cap", RECORD_CASES)
def test_record_form_gradient_exits_against_float64(name, cap, cases, monkeypatch):
    """the record form (harp_shade_args.trec + harp_texel_reduce + harp_texel_finish) on the texture cases, with a list capacity of 4 on top
    (every record but four per UV tile takes the full-list path into the double maps): no fixed-point term for the two maps"""
    c = device_case(cases, name)
    _, got = run_ops_shade(c, monkeypatch, records=True, cap=cap)
    check_gradients(c, got, f"records cap={cap}", records=True)


# ---- the raw struct -----------------------------------------------------------------------------------------------------------------
def raw_args(c, geometry=True):
    """harp_shade_args as ops._shade_args fills it + zeroed outputs for every gradient (table form); returns (args, outputs, keep-alive)"""
    from harp_amd import _lib, ops
    t = {k: v.to(DEV).contiguous() for k, v in c["ref"]["src"].items()}
    t["light_R"] = t["light_R"].reshape(-1, 9)
    a = ops._shade_args(c["d_face_id"], c["d_ws"], c["topo"], t["verts"], t["vnormals"], t["tex"], t["nmap"], t["light_pos"], t["colors"], t["zl"],
                        t["light_R"], t["light_T"], c["S"], c["focal"], (c["S"] / 2.0, c["S"] / 2.0), (1.0, 1.0, 1.0))
    g_rgb = c["ref"]["cot"].to(DEV).contiguous()
    out = {k: torch.zeros_like(t[k]) for k in GROUPS}
    names = dict(tex="g_tex", nmap="g_nmap", verts="g_verts", vnormals="g_vnormals", ndc="g_ndc", zl="g_zl", light_pos="g_light_pos", colors="g_colors",
                 light_R="g_light_R", light_T="g_light_T")
    a.g_rgb = _lib.ptr(g_rgb)
    for k, field in names.items():
        if geometry or k not in ("verts", "vnormals", "ndc"):
            setattr(a, field, _lib.ptr(out[k]))
    return a, out, (t, g_rgb)


def shade_bwd(a):
    from harp_amd import _lib
    rc = _lib.lib().harp_shade_bwd(ctypes.byref(a), _lib.stream())
    torch.cuda.synchronize()
    return rc


def _views(c, out):
    return dict(out, light_R=out["light_R"].view(c["B"], 3, 3))


@pytest.mark.parametrize("name", ["dense", "light_zoom"])
def test_raw_struct_interleaved_vertex_gradients(name, cases):
    """g_vert9 set: the vertex gradients of table flush AND probe-exhaustion atomics land in the interleaved buffer; harp_vert9_unpack moves
    them into the three arrays (same bound) and hands the buffer back all-zero"""
    from harp_amd import _lib
    c = device_case(cases, name)
    a, out, keep = raw_args(c)
    V = c["verts"].shape[1]
    g9 = torch.zeros(c["B"], V, 9, device=DEV)
    a.g_vert9 = _lib.ptr(g9)
    assert shade_bwd(a) == 0
    assert g9.abs().max().item() > 0 and all(out[k].abs().max().item() == 0 for k in ("verts", "vnormals", "ndc"))
    _lib.check(_lib.lib().harp_vert9_unpack(_lib.ptr(g9), c["B"] * V, _lib.ptr(out["verts"]), _lib.ptr(out["vnormals"]), _lib.ptr(out["ndc"]), _lib.stream()), "unpack")
    torch.cuda.synchronize()
    assert int((g9 != 0).sum()) == 0
    check_gradients(c, _views(c, out), "g_vert9")


@pytest.mark.parametrize("name", ["dense", "light_zoom"])
def test_raw_struct_light_view_tile_flags(name, cases):
    """g_zl_tiles set: every 16x16 light-view tile whose reference tap gradient is non-zero is flagged (window flush and out-of-window atomics
    alike), no tile is flagged that no tap touches; harp_depth_bwd_tiles on the matching light-view rasterisation leaves image and flags zero"""
    from harp_amd import _lib
    c = device_case(cases, name)
    ref, S, B = c["ref"], c["S"], c["B"]
    a, out, keep = raw_args(c)
    nt = (S + 15) // 16
    flags = torch.zeros(B, nt, nt, dtype=torch.uint8, device=DEV)
    a.g_zl_tiles = _lib.ptr(flags)
    assert shade_bwd(a) == 0
    check_gradients(c, _views(c, out), "g_zl_tiles")
    fl = flags.cpu() != 0

    def tiles(img):
        p = torch.zeros(B, nt * 16, nt * 16, dtype=torch.bool)
        p[:, :S, :S] = img
        return p.view(B, nt, 16, nt, 16).any(4).any(2)
    # "non-zero" at float32: an entry above its own error bound, which the kernel therefore cannot have left at zero (the float64 reference
    # also holds entries like 1e-130, from sigmoid tails that are exact zeros in float32)
    rz = ref["res"]["zl"]
    need = tiles(rz["ref"].abs() > rz["N"] * rz["M"] * 2.0 ** -24 + 4.0 * ref["e32"]["zl"] + 2.0 ** -22 * rz["A"])
    touched = torch.zeros(B, S * S, dtype=torch.bool)
    tap = ref["ix"]["tap"][ref["cov"]]
    bsel = torch.nonzero(ref["cov"])[:, 0]
    touched[bsel[:, None].expand(-1, 9).reshape(-1), tap.reshape(-1)] = True
    may = tiles(touched.view(B, S, S))
    print(f"[{name}] light-view tiles: {int(need.sum())} hold a gradient, {int(fl.sum())} flagged, {int(may.sum())} touched by a tap")
    assert int(need.sum()) > 0 and bool((fl | ~need).all()) and bool((may | ~fl).all())
    g_ndc_l = torch.zeros_like(out["ndc"])
    V, F = c["verts"].shape[1], c["faces"].shape[0]
    _lib.check(_lib.lib().harp_depth_bwd_tiles(_lib.ptr(c["d_face_id_l"]), _lib.ptr(c["d_ws_l"]), _lib.ptr(c["topo"].faces), _lib.ptr(out["zl"]), B, V, F, S,
                                               _lib.ptr(g_ndc_l), _lib.ptr(flags), _lib.stream()), "harp_depth_bwd_tiles")
    torch.cuda.synchronize()
    assert out["zl"].abs().max().item() == 0 and int(flags.max()) == 0 and g_ndc_l.abs().max().item() > 0


@pytest.mark.parametrize("name", ["dense", "light_zoom"])
def test_raw_struct_without_geometry_gradients(name, cases):
    """g_verts = g_vnormals = g_ndc = NULL (the appearance-only stage): texture, normal map, tap and scalar gradients within the same bound;
    a MIX of NULL and non-NULL geometry pointers is refused with every output untouched"""
    c = device_case(cases, name)
    a, out, keep = raw_args(c, geometry=False)
    assert shade_bwd(a) == 0
    assert all(out[k].abs().max().item() == 0 for k in ("verts", "vnormals", "ndc"))
    check_gradients(c, _views(c, out), "no geometry", groups=tuple(k for k in GROUPS if k not in ("verts", "vnormals", "ndc")))
    for missing in ("g_verts", "g_vnormals", "g_ndc"):
        a, out, keep = raw_args(c)
        setattr(a, missing, None)
        assert shade_bwd(a) == 1                                               # HARP_ERR_ARG
        assert all(v.abs().max().item() == 0 for v in out.values()), missing
