"""TEST INFRASTRUCTURE ONLY — the synthetic meshes of tests/test_gpu_depth_bwd_paths.py (given directly as light-view NDC vertices), the
float64 reference of the depth map's backward and, per case, the condition that makes it reach its edge of depth_bwd_kernel
(csrc/shade.hip).

Reference: zbuf = the perspective-correct depth of the nearest face per pixel of a K = 1 hard rasterisation (tests/_raster_ref.py: the
nearest face and the `undecided` flags of the bbox-pair path; the depth expression is `_raster_ref._pair`'s), and autograd of
sum(cot * zbuf) to the float32 `ndc` the kernel receives.  tests/test_depth_cases_cpu.py shows that gradient equal to autograd through
oracle/p3d_like.rasterize_meshes' zbuf to 1e-12 on every case, and asserts every case's conditions on the reference alone — no GPU."""
import numpy as np
import torch

from tests import _raster_cases as C
from tests import _raster_ref as R

F64 = torch.float64
TILE, SUPER, STRIP = R.TILE, R.SUPER, 4           # a workgroup's 16x16 tile; one wave = a 16x4 strip of it (shade.hip:681-682)
K_SLOTS = 256                                     # shade.hip:654  VertexAccum<256, 3> (harp_common.h:164: 32 probes)
GRID_CAP = 4096                                   # shade.hip:803  min(tile_grid(B, nsx), 4096u)
RIDER_CAP = 1024 * 256                            # shade.hip:835, 852  min(..., 1024) workgroups of 256 lanes per rider
CASES = ("dense", "one_face", "fan", "off_grid", "range", "empty_frame", "wrap")

# extents a little beyond the image and asymmetric: no vertex, edge or diagonal runs through pixel centres
X0, X1, Y0, Y1 = -1.0613, 1.0571, -1.0537, 1.0631


def _px(i, S):
    """NDC coordinate of the (fractional) pixel index i"""
    return 1.0 - (2.0 * i + 1.0) / S


def build(name):
    """dict(name, S, B, ndc (B,V,3) float32, faces (F,3) int64, cot0 (B,S,S) float32: the cotangent before it is restricted to the covered,
    decided pixels)"""
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 11)
    S = {"off_grid": 40, "wrap": 80}.get(name, 32)
    if name in ("dense", "range"):
        v0, f = C.grid(48, 48, X0, X1, Y0, Y1, z=1.5, amp=0.05)
        v = np.stack([v0, v0 + np.array([0.0071, -0.0053, 0.07])])
    elif name == "one_face":
        v0, f = C.grid(1, 1, X0, X1, Y0, Y1)
        v0[:, 2] = [1.3, 2.1, 1.9, 1.6]
        v1 = v0 + np.array([0.0113, -0.0091, 0.0])
        v1[:, 2] = [2.2, 1.4, 1.7, 1.2]
        v = np.stack([v0, v1])
    elif name == "fan":
        # the hub inside a wave's strip (rows 4..7 of tile (0, 0) / rows 16..19 of tile (1, 1)), placed so that the strip's 64 pixel centres fall
        # into 35 of the 64 sectors, none closer than 0.03 sector widths to a spoke
        v0, f = C.fan(64, (_px(6.21, S), _px(5.13, S)), 3.0)
        v1, _ = C.fan(64, (_px(22.21, S), _px(17.13, S)), 3.0)
        v = np.stack([v0, v1])
    elif name == "off_grid":
        v0, f = C.grid(12, 12, X0, X1, Y0, Y1, z=1.4, amp=0.08)
        v = np.stack([v0, v0 + np.array([-0.0171, 0.0233, 0.1])])
    elif name == "empty_frame":
        v0, f = C.grid(6, 6, X0, X1, Y0, Y1, z=1.4, amp=0.08)
        v = np.stack([v0, v0 + np.array([3.2, 0.0, 0.0]), v0 * np.array([0.83, 0.79, 1.0]) + np.array([0.0371, -0.0293, 0.2])])
    elif name == "wrap":
        # S = 80: two super-tile columns / rows, the second 16 px wide (NDC < -0.6); every frame reaches into it
        B = 72
        v0, f = C.grid(20, 20, -1.0, 1.0, -1.0, 1.0, z=1.5, amp=0.06)
        b = np.arange(B)
        sc = 0.8131 + 0.2873 * ((b * 37) % B) / B
        dx, dy = 0.0771 * np.sin(1.3 * b + 0.2), 0.0693 * np.cos(0.9 * b + 0.5)
        v = v0[None] * np.stack([sc, sc * (1.0 + 0.03 * np.sin(b)), np.ones(B)], -1)[:, None] + np.stack([dx, dy, 0.011 * (b % 9)], -1)[:, None]
    else:
        raise KeyError(name)
    B = v.shape[0]
    mag = torch.rand(B, S, S, generator=g) * 0.8 + 0.2
    if name == "range":                                    # magnitudes 2^-20 .. 1 mixed inside every tile
        mag = torch.exp2(-20.0 * torch.rand(B, S, S, generator=g))
    cot0 = mag * torch.where(torch.rand(B, S, S, generator=g) < 0.5, -1.0, 1.0)
    return dict(name=name, S=S, B=B, ndc=torch.from_numpy(np.asarray(v)).float().contiguous(), faces=torch.from_numpy(f).long(), cot0=cot0)


def frame(c, b=0):
    """the one-frame version of a case (the anchor on the oracle)"""
    return dict(c, B=1, ndc=c["ndc"][b:b + 1].contiguous(), cot0=c["cot0"][b:b + 1].contiguous())


# ----------------------------------------------------------------------------------------------------------------------
# reference
# ----------------------------------------------------------------------------------------------------------------------
def raster(c, dtype=F64):
    """K = 1 hard rasterisation on the bbox-pair path -> face_id (B,S,S) (-1: none), undecided (B,S,S): covered pixels whose nearest face is
    not decided at float32 precision and uncovered ones that may become covered"""
    h = R.rasterize(c["ndc"], c["faces"], c["S"], dtype=dtype)
    return dict(face_id=R.dense(h, "face_id", -1), z=R.dense(h, "z", -1.0), undecided=R.undecided_image(h))


def cotangent(c, ras):
    """non-zero only on covered pixels, as in a step; zero on the undecided ones"""
    return torch.where((ras["face_id"] >= 0) & ~ras["undecided"], c["cot0"], torch.zeros_like(c["cot0"]))


def zbuf_gradient(c, face_id, cot, dtype=F64, stats=True):
    """d sum(cot * zbuf) / d ndc for the given nearest-face image, evaluated in `dtype`: (B,V,3); stats: dict(ref, A) with A_i the sum of
    the magnitudes of the per-pixel contributions to element i"""
    B, S, V = c["B"], c["S"], c["ndc"].shape[1]
    pix = torch.nonzero(face_id.reshape(-1) >= 0)[:, 0]
    fid = face_id.reshape(-1)[pix]
    b, rem = pix // (S * S), pix % (S * S)
    leaf = c["ndc"].to(dtype).requires_grad_()
    fvs = leaf[b[:, None], c["faces"][fid]]                                # (P,3,3): every pixel's own copy of its face
    pc = R.pixel_centers(S, dtype)
    z = R._pair(fvs, pc[rem % S], pc[rem // S], 0.0)["pz"]
    g_leaf, g_fvs = torch.autograd.grad((z * cot.reshape(-1)[pix].to(dtype)).sum(), [leaf, fvs])
    if not stats:
        return g_leaf
    vid = (b[:, None] * V + c["faces"][fid]).reshape(-1)
    A = torch.zeros(B * V, 3, dtype=dtype).index_add_(0, vid, g_fvs.abs().reshape(-1, 3)).view(B, V, 3)
    return dict(ref=g_leaf, A=A)


def reference(c, face_id, cot):
    """float64 gradient and A, and E32 = |ref32 - ref64|_inf of the same code evaluated in float32"""
    r = zbuf_gradient(c, face_id, cot)
    r32 = zbuf_gradient(c, face_id, cot, dtype=torch.float32, stats=False)
    r["E32"] = (r32.double() - r["ref"]).abs().max().item()
    return r


# ----------------------------------------------------------------------------------------------------------------------
# conditions: asserted from a face-id image (the reference's without a GPU, the rasteriser's in the GPU test)
# ----------------------------------------------------------------------------------------------------------------------
def tiles_of(img, side=TILE):
    """(B,S,S,...) -> (B,nt,nt,side*side,...); the pixels of a ragged tile beyond the image read 0 / False"""
    B, S = img.shape[:2]
    n = (S + side - 1) // side
    pad = torch.zeros((B, n * side, n * side) + img.shape[3:], dtype=img.dtype)
    pad[:, :S, :S] = img
    pad = pad.view(B, n, side, n, side, *img.shape[3:])
    return pad.permute(0, 1, 3, 2, 4, *range(5, pad.dim())).reshape(B, n, n, side * side, *img.shape[3:])


def tile_grid(B, S):
    nsx = (S + SUPER - 1) // SUPER
    return ((B * nsx * nsx + 7) // 8) * 8 * (SUPER // TILE) ** 2


def _distinct(x, m):
    return int(torch.unique(x[m]).numel())


def conditions(c, face_id, cot, undecided, nact=None, order=None):
    """the share of undecided pixels, the number of active ones and the case's own edge; returns what it found (printed, docs/NOTEBOOK.md)"""
    name, B, S, V, faces = c["name"], c["B"], c["S"], c["ndc"].shape[1], c["faces"]
    cov = face_id >= 0
    act = cov & (cot != 0)
    n_cov, n_und = int(cov.sum()), int((undecided & cov).sum()) + int((undecided & ~cov).sum())
    info = dict(covered=n_cov, undecided=n_und, share=round(n_und / max(n_cov, 1), 4), active=int(act.sum()))
    assert n_und <= 0.02 * n_cov, info                                    # move the vertices, not the cap
    assert info["active"] >= 200, info
    assert not (cot != 0)[~cov].any()
    t_act, t_fid = tiles_of(act), tiles_of(face_id.long())
    if name in ("dense", "range"):
        vid = tiles_of(faces[face_id.long().clamp(min=0)])                # (B,n,n,256,3)
        full = torch.nonzero(tiles_of(cov).all(-1)).tolist()
        per = [_distinct(vid[b, y, x], t_act[b, y, x]) for b, y, x in full]
        info.update(full_tiles=len(full), min_active_vertices_per_full_tile=min(per), max_active_vertices_per_full_tile=max(per))
        assert full and min(per) > K_SLOTS, info                          # pigeonhole: the table cannot hold them
    if name == "range":
        m = tiles_of(cot.abs())
        ratios = [(m[b, y, x][t_act[b, y, x]].max() / m[b, y, x][t_act[b, y, x]].min()).item() for b, y, x in torch.nonzero(t_act.any(-1)).tolist()]
        info["min_cot_ratio_per_tile"] = min(ratios)
        assert min(ratios) >= 1e5, info
    if name == "one_face":
        one = [int(t_act[b, y, x].sum()) for b, y, x in torch.nonzero(t_act.any(-1)).tolist() if _distinct(t_fid[b, y, x], t_act[b, y, x]) == 1]
        info["active_pixels_of_the_one_face_tiles"] = sorted(one)
        assert one and max(one) >= 250, info
    if name == "fan":
        assert bool((faces == 0).any(1).all())                            # every face holds the hub, vertex 0
        s_act, s_fid = t_act.view(B, -1, TILE // STRIP, STRIP * TILE), t_fid.view(B, -1, TILE // STRIP, STRIP * TILE)      # (B, tile, wave, 64)
        per = [_distinct(s_fid[b, t, w], s_act[b, t, w]) for b, t, w in torch.nonzero(s_act.any(-1)).tolist()]
        info["max_faces_per_strip_on_vertex_0"] = max(per)
        assert max(per) >= 32, info
    if name == "off_grid":
        edge = (S // TILE) * TILE
        info.update(ragged=S % TILE, active_in_ragged_rows=int(act[:, edge:, :].sum()), active_in_ragged_columns=int(act[:, :, edge:].sum()))
        assert S % TILE == 8 and info["active_in_ragged_rows"] > 0 and info["active_in_ragged_columns"] > 0, info
    nsx = (S + SUPER - 1) // SUPER
    pairs = int(tiles_of(act, SUPER).any(-1).sum())                      # (frame, super-tile) pairs that hold active pixels
    if name == "empty_frame":
        info.update(slots=B * nsx * nsx, pairs_with_active_pixels=pairs, nact=nact)
        assert B == 3 and not cov[1].any() and cov[0].any() and cov[2].any() and pairs < B * nsx * nsx, info
        assert nact is None or (pairs <= nact < B * nsx * nsx), info
    if name == "wrap":
        info.update(tile_grid=tile_grid(B, S), pairs_with_active_pixels=pairs, nact=nact, v9_floats=B * V * 9)
        assert tile_grid(B, S) > GRID_CAP and pairs > GRID_CAP // 16, info                # work at virtual workgroup ids >= 4096
        assert bool(tiles_of(act, SUPER).any(-1).all()) and nsx == 2 and S % SUPER == TILE          # all four super-tiles of every frame; tiles decoded past S
        assert B * V * 9 > RIDER_CAP, info
        if order is not None:
            n = B * nsx * nsx
            info["launch_order_moved"] = int((order[:n] != torch.arange(n)).sum())
            assert torch.equal(torch.sort(order[:nact]).values, torch.arange(nact)) and info["launch_order_moved"] > 0, info
    print(f"[{name}] conditions: {info}")
    return info
