"""TEST INFRASTRUCTURE ONLY — the inputs of the bake tests (tests/test_bake_cpu.py checks the references and the undecidable caps on
them, tests/test_gpu_bake.py runs csrc/bake.hip on them): UV layouts on dyadic atlases, and small quad scenes whose face_id / zbuf come
from tests/_raster_ref.py, built without the product's rasteriser."""
import functools

import numpy as np
import torch

from tests import _bake_ref as R
from tests import _raster_ref as RR

# ---- texel map: UVs in multiples of 1/16 on atlases with Wt - 1, Ht - 1 powers of two: every texel-space coordinate and every edge
# function is exact in float32, so ties are exactly decidable
_Q = lambda *p: np.array(p, dtype=np.float32) / 16.0       # noqa: E731
UV_CASES = {
    # the shared diagonal runs through texel centres: the lower face index owns them
    "shared_edge": (_Q((0, 0), (16, 0), (16, 16), (0, 16)), [[0, 1, 2], [0, 2, 3]]),
    "shared_edge_swapped": (_Q((0, 0), (16, 0), (16, 16), (0, 16)), [[0, 2, 3], [0, 1, 2]]),
    # a fan of four faces around a vertex that sits on a texel centre
    "shared_vertex": (_Q((8, 8), (2, 2), (14, 2), (14, 14), (2, 14)), [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]]),
    # face 0 has no area and lies inside face 1: it owns nothing although its index is the lowest
    "zero_area": (_Q((4, 4), (8, 8), (12, 12), (0, 0), (16, 0), (16, 16)), [[0, 1, 2], [3, 4, 5], [2, 2, 2]]),
    "partly_outside": (_Q((-8, 4), (8, 4), (8, 24), (20, -4), (12, 12), (20, 12)), [[0, 1, 2], [3, 4, 5]]),
    "overlapping_charts": (_Q((0, 0), (12, 0), (0, 12), (4, 4), (16, 4), (16, 16), (2, 2), (10, 2), (10, 10)), [[3, 4, 5], [0, 1, 2], [6, 7, 8]]),
    "one_face": (_Q((1, 1), (15, 3), (5, 13)), [[0, 1, 2]]),
    "clockwise": (_Q((1, 1), (5, 13), (15, 3)), [[0, 1, 2]]),
}
UV_ATLASES = [(17, 17), (33, 17)]                          # (Ht, Wt)


def uv_case(name):
    vu, fu = UV_CASES[name]
    return vu, np.asarray(fu, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def hand_uvs():
    from harp_amd import synth
    tpl = synth.load_template("hand")
    return np.asarray(tpl["verts_uvs"], dtype=np.float32).reshape(-1, 2), np.asarray(tpl["faces_uvs"], dtype=np.int32).reshape(-1, 3)


HAND_ATLASES = [(64, 64), (65, 33)]


@functools.lru_cache(maxsize=None)
def hand_texel_map(Ht, Wt):
    return R.texel_map(*hand_uvs(), Ht, Wt)


# ---- accumulation: up to four quads (8 triangles), each with a chart of its own
FL = 2.0                                                   # x_ndc = FL X / Z for a camera at the origin looking along +z
HT, WT = 24, 40                                            # neither a power of two nor a multiple of the 256-thread workgroup

#         centre              half-edge a       half-edge b
QUADS = {
    "front": ((0.0, 0.0, 2.0), (0.45, 0.0, 0.1), (0.0, 0.45, 0.0)),
    "back": ((0.3, 0.2, 2.6), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0)),                # partly hidden behind "front"
    "side": ((-1.0, -0.6, 2.2), (0.5, 0.0, 0.0), (0.0, 0.3, 0.05)),             # partly left of the image
    "steep": ((0.1, -0.75, 2.0), (0.4, 0.0, 0.0), (0.0, 0.03, 0.4)),            # seen at a grazing angle
    "through": ((0.6, -0.1, 0.3), (0.0, 0.0, 0.6), (0.0, 0.2, 0.0)),            # straddles the camera plane z = 0
}
# name -> (S, B, quads, switches, reasons that must reject at least one (texel, frame) pair)
ACCUM_CASES = {
    "delit": (32, 3, ("front", "back", "side", "steep"), dict(normals=True, light=True), ("occluded", "outside", "angle")),
    "raw": (48, 6, ("front", "back", "side", "steep"), dict(normals=True), ("occluded", "outside", "angle")),
    "no_normals": (32, 1, ("front", "back", "side", "steep"), dict(), ("occluded", "outside")),
    "mask_rows": (48, 3, ("front", "back"), dict(normals=True, light=True, mask=True, rows=(3, 0, 2), N=4), ("mask", "occluded")),
    "hole_badrow": (32, 3, ("front", "side"), dict(normals=True, hole=True, rows=(1, -1, 0), N=2), ("no_face", "row")),
    "behind": (32, 1, ("front", "through"), dict(normals=True, light=True), ("behind",)),
    "two_triangles": (48, 6, ("front",), dict(normals=True, light=True), ()),
}


def _targets(N, S, seed):
    """smooth sinusoids in [0.1, 0.9]"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    img = np.empty((N, S, S, 3), dtype=np.float32)
    for n in range(N):
        for c in range(3):
            fx, fy, ph = rng.uniform(0.05, 0.25), rng.uniform(0.05, 0.25), rng.uniform(0, 6.28)
            img[n, :, :, c] = 0.5 + 0.4 * np.sin(fx * x + fy * y + ph)
    return img


@functools.lru_cache(maxsize=None)
def accum_case(name, seed=0):
    """-> dict of float32 / int32 numpy arrays: everything harp_texture_bake_accum takes, and `expect`"""
    S, B, quads, sw, expect = ACCUM_CASES[name]
    rng = np.random.default_rng(seed)
    nq = len(quads)
    verts_uvs, faces, corners, normals = [], [], [], []
    for q, key in enumerate(quads):
        c, a, b = (np.array(v, dtype=np.float64) for v in QUADS[key])
        u0, u1 = q * 0.25 + 0.02, q * 0.25 + 0.23
        verts_uvs += [(u0, 0.1), (u1, 0.1), (u1, 0.9), (u0, 0.9)]
        faces += [(4 * q, 4 * q + 1, 4 * q + 2), (4 * q, 4 * q + 2, 4 * q + 3)]
        corners.append(np.stack([c - a - b, c + a - b, c + a + b, c - a + b]))
        n = np.cross(a, b)
        n = n / np.linalg.norm(n)
        n = -n if n @ c > 0 else n                                              # towards the camera at the origin
        vn = np.repeat(n[None], 4, 0)
        if key == "steep":                                                      # two corners turned away: cosv crosses cos_min inside the quad
            vn[2] = vn[3] = np.array([1.0, 0.0, 0.0])
        normals.append(vn + 0.05 * rng.normal(size=(4, 3)))
    verts0, vn0 = np.concatenate(corners), np.concatenate(normals)
    V = 4 * nq
    verts = np.stack([verts0 + np.array([0.02, -0.015, 0.01]) * k + 0.004 * rng.normal(size=(V, 3)) for k in range(B)]).astype(np.float32)
    vnormals = np.stack([vn0 + 0.02 * rng.normal(size=(V, 3)) for _ in range(B)]).astype(np.float32)
    v64 = verts.astype(np.float64)
    ndc = np.stack([FL * v64[..., 0] / v64[..., 2], FL * v64[..., 1] / v64[..., 2], v64[..., 2]], -1).astype(np.float32)
    faces = np.asarray(faces, dtype=np.int32)
    ref = RR.rasterize(torch.from_numpy(ndc), torch.from_numpy(faces), S)
    face_id = RR.dense(ref, "face_id", -1).numpy().astype(np.int32)
    zbuf = RR.dense(ref, "z", -1.0).numpy().astype(np.float32)
    if sw.get("hole"):                                                          # the hard pass saw nothing in this block of pixels
        face_id[:, S // 2 - 4:S // 2 + 3, S // 2 - 5:S // 2 + 2] = -1
        zbuf[:, S // 2 - 4:S // 2 + 3, S // 2 - 5:S // 2 + 2] = -1.0
    N = sw.get("N", B)
    rows = np.asarray(sw.get("rows", range(B)), dtype=np.int32)
    y_true = _targets(N, S, seed + 1)
    y_mask = np.ones((N, S, S), dtype=np.float32)
    if sw.get("mask"):
        y_mask[:, :, S // 2:] = 0.0
        y_mask[:, : S // 4] = 0.25
    verts_uvs = np.asarray(verts_uvs, dtype=np.float32)
    tf, tbary, _ = R.texel_map(verts_uvs, faces, HT, WT)
    case = dict(name=name, S=S, B=B, N=N, verts_uvs=verts_uvs, faces=faces, texel_face=tf, texel_bary=tbary.astype(np.float32), ndc=ndc,
                face_id=face_id, zbuf=zbuf, y_true=y_true, y_mask=y_mask, rows=rows, expect=expect, verts=None, vnormals=None, cam_pos=None,
                light_pos=None, colors=None)
    if sw.get("normals"):
        case.update(verts=verts, vnormals=vnormals, cam_pos=np.zeros((B, 3), dtype=np.float32) + 0.01 * rng.normal(size=(B, 3)).astype(np.float32))
    if sw.get("light"):
        case["light_pos"] = (np.array([-0.5, -0.5, -0.5]) + 0.2 * rng.normal(size=(B, 3))).astype(np.float32)
        amb = rng.uniform(0.3, 0.5, size=(B, 1))
        case["colors"] = np.concatenate([np.repeat(amb, 3, 1), np.repeat(1.0 - amb, 3, 1), np.full((B, 3), 0.05)], 1).astype(np.float32)
    return case


ACCUM_KEYS = ("texel_face", "texel_bary", "faces", "ndc", "face_id", "zbuf", "y_true", "y_mask", "rows", "verts", "vnormals", "cam_pos",
              "light_pos", "colors")


@functools.lru_cache(maxsize=None)
def accum_reference(name, seed=0):
    """(accumulators, info) of tests/_bake_ref.accumulate on the whole case in one call; computed once, never modified"""
    case = accum_case(name, seed)
    acc = R.new_accumulators(HT, WT)
    info = R.accumulate(acc, **{k: case[k] for k in ACCUM_KEYS})
    return acc, info


def dilate_case(Ht, Wt, C, kind, seed=0):
    """tex (Ht,Wt,C) float32, valid, allow (or None) uint8"""
    rng = np.random.default_rng(seed + 31 * Ht + 7 * Wt + C)
    tex = rng.uniform(0.0, 1.0, size=(Ht, Wt, C)).astype(np.float32)
    y, x = np.meshgrid(np.arange(Ht), np.arange(Wt), indexing="ij")
    allow = None
    if kind == "blob":                                     # a valid disc: everything else is a hole far wider than 2 n_pass
        valid = (y - Ht // 3) ** 2 + (x - Wt // 2) ** 2 <= 9
    elif kind == "wall":                                   # valid left strip; a wall of allow = 0 keeps the fill from the right part
        valid = x < 3
        allow = (x != 8).astype(np.uint8)
    elif kind == "speckle":
        valid = rng.uniform(size=(Ht, Wt)) < 0.15
    else:
        raise KeyError(kind)
    return tex, valid.astype(np.uint8), allow
