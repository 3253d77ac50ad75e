"""float64 numpy restatement of what harp_mesh_contact_excl adds to harp_mesh_contact's contract (include/harp_hip.h), on
top of tests/_contact_ref.py and independent of the package: the masked minimum, the bit table, the geodesic exclusion by Floyd-Warshall,
the two-sphere mesh of the wind > 1 rule, and the masks that tests/test_contact_excl_cpu.py (caps, counted on the reference alone) and
tests/test_gpu_contact_excl.py (the kernel against the reference) share."""
import numpy as np

from tests import _contact_ref as CR

EXCL_FACES = 128
MASK_TAGS = ("zero", "bernoulli", "nearest", "odd", "chunks", "last")


# ---- the contract's addition ---------------------------------------------------------------------------------------------------------------
def masked(ref, mask):
    """ref: CR.mesh_contact's dict; mask (Vq,F) bool, the same for every frame -> the dict with D, d_min and face taken over the faces that
    count: the minimum over np.where(mask, inf, D), the lowest index among equal values; wind_all and M as they are"""
    D = np.where(np.asarray(mask, bool)[None], np.inf, ref["D"])
    d_min = D.min(-1)
    face = np.where(np.isfinite(d_min), D.argmin(-1), -1)                   # (argmin: the first of equal values)
    return dict(ref, D=D, d_min=d_min, face=face)


def pack(mask):
    """(V,F) bool -> (ceil(F / 128), V, 4) uint32: bit k & 31 of [c, i, k >> 5] is face 128 c + k for vertex i.  Face by face over the
    128 places of a chunk (tests/test_contact_excl_cpu.py checks single hand-set bits against the formula of the header)"""
    mask = np.asarray(mask, bool)
    V, F = mask.shape
    C = -(-F // EXCL_FACES)
    out = np.zeros((C, V, 4), np.uint32)
    for k in range(EXCL_FACES):
        f = np.arange(C) * EXCL_FACES + k                                   # place k of every chunk
        have = f < F
        out[have, :, k >> 5] |= mask[:, f[have]].T.astype(np.uint32) << np.uint32(k & 31)
    return out


# ---- the geodesic exclusion ----------------------------------------------------------------------------------------------------------------
def edge_paths(verts, faces):
    """(V,V) float64 shortest path lengths along the mesh's edges, Floyd-Warshall; inf between components"""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    V = v.shape[0]
    P = np.full((V, V), np.inf)
    P[np.arange(V), np.arange(V)] = 0.0
    for a, b in ((0, 1), (1, 2), (2, 0)):
        w = np.linalg.norm(v[f[:, a]] - v[f[:, b]], axis=1)
        np.minimum.at(P, (f[:, a], f[:, b]), w)
        np.minimum.at(P, (f[:, b], f[:, a]), w)
    for k in range(V):
        P = np.minimum(P, P[:, k, None] + P[None, k, :])
    return P


def exclusion(P, faces, radius):
    """face f is excluded for vertex i iff some corner of f is within radius of i (an unreachable corner is not, whatever the radius)"""
    near = np.isfinite(P) & (P <= radius)
    return near[:, np.asarray(faces, np.int64)].any(-1)


# ---- the two spheres of the wind > 1 rule --------------------------------------------------------------------------------------------------
def two_spheres(gap):
    """two unit 320-face icospheres, centres `gap` apart along x, as ONE mesh -> (verts (324,3), faces (640,3), sphere of every vertex
    (324,), sphere of every face (640,))"""
    v, f = CR.icosphere(2)
    n = len(v)
    verts = np.concatenate([v, v + np.array([gap, 0.0, 0.0])])
    faces = np.concatenate([f, f + n]).astype(np.int32)
    return verts, faces, np.repeat([0, 1], n), np.repeat([0, 1], len(f))


def self_case(gap, B=1, scale=CR.SCALE):
    """the two-sphere mesh at the workload's scale as query AND target under one camera per frame, and the mask that excludes each
    sphere's own faces for its vertices -> (side dict, mask (324,640))"""
    verts, faces, vs, fs = two_spheres(gap)
    cam_R, cam_T = CR.cameras(np.random.default_rng(5), B)
    side = dict(verts=np.repeat((scale * verts)[None], B, 0).astype(np.float32), cam_R=cam_R, cam_T=cam_T, faces=faces, flip=False)
    return side, vs[:, None] == fs[None, :]


# ---- the masks of the grid ----------------------------------------------------------------------------------------------------------------
def masks(ref, seed):
    """the six masks of one case, from its unmasked reference: (tag, mask (Vq,F) bool) in the order of MASK_TAGS.
    zero: nothing excluded.  bernoulli: each (vertex, face) with probability 0.3.  nearest: for every vertex its nearest face of EVERY
    frame (the table is the same for all frames), which forces the runner-up.  odd: every face for the odd vertices.  chunks: the even
    chunks of 128 faces for every vertex (all faces of a target of up to 128).  last: everything but the last face."""
    B, Vq, F = ref["D"].shape
    rng = np.random.default_rng(seed)
    zero = np.zeros((Vq, F), bool)
    yield "zero", zero
    yield "bernoulli", rng.random((Vq, F)) < 0.3
    near = zero.copy()
    for b in range(B):
        ok = np.isfinite(ref["d_min"][b])
        near[np.nonzero(ok)[0], ref["D"][b].argmin(-1)[ok]] = True
    yield "nearest", near
    odd = zero.copy()
    odd[1::2] = True
    yield "odd", odd
    chunks = zero.copy()
    chunks[:, (np.arange(F) // EXCL_FACES) % 2 == 0] = True
    yield "chunks", chunks
    last = ~zero
    last[:, F - 1] = False
    yield "last", last


def with_duplicate(target, f0):
    """the target with face f0 once more at the end of its face list: the pair ties exactly"""
    return dict(target, faces=np.concatenate([target["faces"], target["faces"][f0:f0 + 1]]).astype(np.int32))


def caps(ref_m, max_dist):
    """(undecided vertices, near vertices with |wind_all - 0.5| < CR.INSIDE_BAND, vertices) of a masked reference at max_dist: the two
    counts that tests/test_gpu_contact_excl.py allows up to 2 % of a case each"""
    maybe = CR.undecided(ref_m, max_dist)
    near = np.isfinite(ref_m["d_min"]) & (ref_m["d_min"] <= max_dist)
    band = near & (np.abs(ref_m["wind_all"] - 0.5) < CR.INSIDE_BAND)
    return int(maybe.sum()), int(band.sum()), int(near.size)


# ---- the players' composition ---------------------------------------------------------------------------------------------------------------
def compose_self(d, f, w, part_table, own, P):
    """SelfContact's documented rule (harp_amd/playback/player.py) from harp_mesh_contact_excl's outputs of a mesh against itself, in numpy,
    vertex by vertex the plain way: d, f, w (n,V); part_table (F,) the part of every face; own (V,) the part of every vertex; P parts ->
    [dist, face, part, own_part, wind, touch, min_dist, max_penetration]"""
    n, V = d.shape
    part = np.zeros((n, V), np.uint8)
    touch = np.zeros((n, P, P), bool)
    for t in range(n):
        for i in np.nonzero(f[t] >= 0)[0]:
            part[t, i] = part_table[f[t, i]]
            touch[t, own[i], part[t, i]] = True
    signed = np.where(w > 1.0, -d, d)
    return [signed, f, part, own, w, touch, signed.min(1), np.where(w > 1.0, d, 0).max(1).clip(min=0)]
