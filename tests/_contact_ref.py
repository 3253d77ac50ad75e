"""float64 numpy restatement of harp_mesh_contact's contract (include/harp_hip.h; csrc/contact.hip), brute force: every query vertex
against every target face of its frame, no culling, no chunks.  Plus the small meshes and the case table that tests/test_contact_cpu.py
(the reference against known geometry) and tests/test_gpu_contact.py (the kernel against the reference) share."""
import itertools

import numpy as np

EPS32 = 2.0 ** -24
DIST_FACTOR = 32.0                 # |dist - dist64| <= 32 * 2^-24 * M, M the largest absolute view coordinate of the case
WIND_TOL = 1e-4
INSIDE_BAND = 0.05                 # the inside flag is compared where |wind64 - 0.5| >= 0.05
MAX_DISTS = (0.0, 0.004, 0.02, np.inf)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def icosphere(sub):
    """unit icosphere, outward-oriented faces: 20 * 4^sub faces, sub in 0..2 -> (verts (V,3) float64, faces (F,3) int32)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(int(sub)):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                mid[key] = len(v)
                v.append(m / np.linalg.norm(m))
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int32)


def open_icosphere(sub, z_cut=-0.7):
    """the icosphere without the faces whose centroid lies below z_cut: a polar cap removed, the analogue of the wrist (276 faces at
    sub = 2) -> (verts, kept faces, removed faces)"""
    v, f = icosphere(sub)
    keep = v[f].mean(1)[:, 2] > z_cut
    return v, f[keep], f[~keep]


def quad():
    """two triangles over the unit square in the plane z = 0, normal +z"""
    return np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], float), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def spherical_area(a, b, c):
    """area of the spherical triangle of three unit vectors by Girard's theorem: the sum of its angles minus pi"""
    def angle(p, q, r):                                # at p, between the great circles to q and r
        u, w = np.cross(p, q), np.cross(p, r)
        return np.arccos(np.clip(np.dot(u, w) / (np.linalg.norm(u) * np.linalg.norm(w)), -1.0, 1.0))
    return angle(a, b, c) + angle(b, c, a) + angle(c, a, b) - np.pi


# ---- the contract -------------------------------------------------------------------------------------------------------------------------
def view_space(verts, cam_R, cam_T, flip):
    """harp_project_fwd's transform: X = p . r[0,3,6] + T[0], Y = p . r[1,4,7] + T[1], Z = p . r[2,5,8] + T[2]; then the mirror"""
    v = np.asarray(verts, np.float64)
    R = np.asarray(cam_R, np.float64).reshape(v.shape[0], 3, 3)
    with np.errstate(all="ignore"):
        out = np.einsum("bvk,bkj->bvj", v, R) + np.asarray(cam_T, np.float64)[:, None, :]
    if flip:
        out[..., 0] = -out[..., 0]
    return out


def _dot(x, y):
    return (x * y).sum(-1)


def _segment(p, o, d):
    """distance from p to the segment o + t d, t in [0, 1]; a zero-length segment is its point"""
    dd, w = _dot(d, d), p - o
    with np.errstate(all="ignore"):
        t = np.where(dd > 0, np.clip(_dot(w, d) / np.where(dd > 0, dd, 1.0), 0.0, 1.0), 0.0)
    e = w - t[..., None] * d
    return np.sqrt(_dot(e, e))


def point_triangle(p, a, b, c):
    """distance from p to the triangle (a, b, c), broadcasting over leading axes: the closest point by the Voronoi regions of the
    triangle (Ericson, Real-Time Collision Detection 5.1.5); a zero-area triangle (zero normal) as the nearest of its three segments"""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        den = 1.0 / (va + vb + vc)
        q = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]

        def sel(cond, val, q):
            return np.where(cond[..., None], val, q)
        q = sel((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None], q)
        q = sel((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * (d2 / (d2 - d6))[..., None], q)
        q = sel((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * (d1 / (d1 - d3))[..., None], q)
        q = sel((d6 >= 0) & (d5 <= d6), c, q)
        q = sel((d3 >= 0) & (d4 <= d3), b, q)
        q = sel((d1 <= 0) & (d2 <= 0), a, q)
        d = np.sqrt(_dot(p - q, p - q))
    n = np.cross(ab, ac)
    flat = _dot(n, n) == 0
    if flat.any():
        seg = np.minimum(np.minimum(_segment(p, a, ab), _segment(p, a, ac)), _segment(p, b, c - b))
        d = np.where(flat, seg, d)
    return d


def half_solid_angle(p, a, b, c):
    """atan2(det[a,b,c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) with a, b, c the corners minus p (van Oosterom and Strackee): half
    the signed solid angle; exactly 0 for a zero-area face"""
    n = np.cross(b - a, c - a)
    flat = _dot(n, n) == 0
    A, B, C = a - p, b - p, c - p
    la, lb, lc = (np.sqrt(_dot(x, x)) for x in (A, B, C))
    det = _dot(A, np.cross(B, C))
    den = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
    return np.where(flat, 0.0, np.arctan2(det, den))


def mesh_contact(query, target, max_dist=np.inf):
    """query, target: dicts of verts (B,V,3), cam_R (B,9), cam_T (B,3), flip and, for the target, faces (F,3) -> dict of
      dist (B,Vq) float64, +inf beyond max_dist; face (B,Vq) the lowest face that attains the float64 minimum, -1 for none; wind (B,Vq), 0
        where dist is +inf — the three outputs of the contract;
      D (B,Vq,F) the distance to every face, +inf for a skipped one; d_min, wind_all: dist and wind without max_dist;
      M: the largest finite absolute view coordinate of the case."""
    q = view_space(query["verts"], query["cam_R"], query["cam_T"], query.get("flip", False))
    t = view_space(target["verts"], target["cam_R"], target["cam_T"], target.get("flip", False))
    faces = np.asarray(target["faces"]).astype(np.int64)
    Vt = t.shape[1]
    in_range = ((faces >= 0) & (faces < Vt)).all(1)
    fc = np.where(in_range[:, None], faces, 0)
    corners = t[:, fc]                                                       # (B,F,3,3)
    valid = in_range[None, :] & np.isfinite(corners).all((2, 3))             # (B,F)
    corners = np.where(valid[..., None, None], corners, 0.0)
    q_ok = np.isfinite(q).all(-1)                                            # (B,Vq)
    p = np.where(q_ok[..., None], q, 0.0)[:, :, None, :]                     # (B,Vq,1,3)
    a, b, c = (corners[:, None, :, k, :] for k in range(3))                  # (B,1,F,3)
    use = valid[:, None, :] & q_ok[:, :, None]
    D = np.where(use, point_triangle(p, a, b, c), np.inf)
    d_min = D.min(-1)
    face = np.where(np.isfinite(d_min), D.argmin(-1), -1)                    # (argmin: the first of equal values)
    sign = -1.0 if target.get("flip", False) else 1.0
    wind_all = sign * (2.0 * np.where(use, half_solid_angle(p, a, b, c), 0.0)).sum(-1) / (4.0 * np.pi)
    near = q_ok & (d_min <= max_dist)
    finite = np.concatenate([q[np.isfinite(q)], t[np.isfinite(t)]])
    return dict(dist=np.where(near, d_min, np.inf), face=np.where(near, face, -1), wind=np.where(near, wind_all, 0.0), D=D, d_min=d_min,
                wind_all=wind_all, M=float(np.abs(finite).max()) if finite.size else 0.0)


def dist_bound(M):
    return DIST_FACTOR * EPS32 * M


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------------------------
SCALE = 0.05                                            # the workload's mesh scale, metres
QUERY_V = (1, 63, 64, 65, 130)
# F = 1, 2, 20, 80, 276 (open), 320 and, around the kernel's chunk of 128 faces, 127, 128, 129; then 960 faces spread over 0.9 m, 8 chunks:
# each of the kernel's four waves walks two chunks, so the second is culled, or not, by the distances the first left (the cull by the
# tile's worst best-distance, which max_dist = inf leaves alone to decide), and the query sits in the middle of the row of pieces, so the
# nearest face is in an early chunk for some vertices and in a late one for others
TARGETS = ("tri", "quad", "ico0", "ico1", "open2", "ico2", "multi127", "multi128", "multi129", "spread960")
SPREAD_STEP = 1.6                                       # unit lengths between the pieces of "spread960" (0.08 m at SCALE)
QUERY_OFFSET = {"spread960": (SCALE * SPREAD_STEP * 5.4, 0.01, 0.02)}      # where the query ball sits; the others: make_pair's default


def spread_mesh(n=12):
    """n 80-face icospheres of radius 0.5 in a row along x, SPREAD_STEP apart, wobbling in y and z: closed pieces, 80 n faces"""
    v, f = icosphere(1)
    centres = [np.array([SPREAD_STEP * k, 0.5 * np.sin(1.3 * k), 0.5 * np.cos(1.7 * k)]) for k in range(n)]
    return np.concatenate([c + 0.5 * v for c in centres]), np.concatenate([f + k * len(v) for k in range(n)]).astype(np.int32)


def multi_mesh(n_tets, n_tris):
    """80 + 4 n_tets + n_tris faces: the 80-face icosphere, then small closed tetrahedra on a ring of radius 1.5 about it, then tiny lone
    triangles on the same ring (closed pieces keep the winding number 0 or 1 almost everywhere, unlike a sphere cut at a face count)"""
    v, f = icosphere(1)
    verts, faces = [v], [f]
    tet = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float)
    tf = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    nrm = np.cross(tet[tf[:, 1]] - tet[tf[:, 0]], tet[tf[:, 2]] - tet[tf[:, 0]])
    tf = np.where(((nrm * tet[tf[:, 0]]).sum(1) > 0)[:, None], tf, tf[:, ::-1])      # outward
    n = len(v)
    for k in range(n_tets + n_tris):
        ang = 2.0 * np.pi * k / (n_tets + n_tris)
        centre = 1.5 * np.array([np.cos(ang), np.sin(ang), 0.3 * np.sin(3.0 * ang)])
        if k < n_tets:
            verts.append(centre + 0.12 * tet); faces.append(tf + n); n += 4
        else:
            verts.append(centre + 0.03 * tet[:3]); faces.append(np.array([[n, n + 1, n + 2]], np.int32)); n += 3
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32)


def target_mesh(name):
    """unit-size target mesh `name` of TARGETS -> (verts (V,3) float64, faces (F,3) int32)"""
    if name == "tri":
        return 0.4 * np.array([[-0.8, -0.6, 0.1], [0.9, -0.5, -0.1], [0.0, 0.9, 0.2]]), np.array([[0, 1, 2]], np.int32)
    if name == "quad":
        v, f = quad()
        return v - np.array([0.5, 0.5, 0.0]), f
    if name.startswith("ico"):
        return icosphere(int(name[3:]))
    if name == "open2":
        return open_icosphere(2)[:2]
    if name == "spread960":
        return spread_mesh()
    return multi_mesh(*{"multi127": (11, 3), "multi128": (12, 0), "multi129": (12, 1)}[name])


def cameras(rng, B):
    """per frame a random rigid cam_R (B,9) and cam_T (B,3) with z in 0.3..1.0, float32"""
    R = np.linalg.qr(rng.normal(size=(B, 3, 3)))[0]
    R *= np.sign(np.linalg.det(R))[:, None, None]
    T = np.stack([rng.uniform(-0.02, 0.02, B), rng.uniform(-0.2, 0.2, B), rng.uniform(0.3, 1.0, B)], 1)
    return R.reshape(B, 9).astype(np.float32), T.astype(np.float32)


def make_pair(seed, B, Vq, target, q_flip=False, t_flip=False, offset=(0.02, 0.01, 0.045)):
    """A query of Vq points scattered in a ball of radius 0.08 m about `offset` and the target mesh at scale 0.05 m about the origin, each
    frame moved a little, under one camera per frame (a scene's players share the camera) -> (query, target) dicts of float32 / int32"""
    rng = np.random.default_rng(seed)
    v, f = target_mesh(target)
    cam_R, cam_T = cameras(rng, B)
    tv = SCALE * v[None] + rng.normal(scale=0.002, size=(B, 1, 3))
    d = rng.normal(size=(B, Vq, 3))
    qv = np.asarray(offset) + d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.0, 0.08, size=(B, Vq, 1))
    return (dict(verts=qv.astype(np.float32), cam_R=cam_R, cam_T=cam_T, flip=bool(q_flip)),
            dict(verts=tv.astype(np.float32), cam_R=cam_R, cam_T=cam_T, faces=f.copy(), flip=bool(t_flip)))


def grid_cases(B, Vq):
    """every target and both flip patterns of each side for one (B, Vq): (name, query, target)"""
    for ti, (name, (qf, tf)) in enumerate(itertools.product(TARGETS, itertools.product((False, True), repeat=2))):
        kw = dict(offset=QUERY_OFFSET[name]) if name in QUERY_OFFSET else {}
        yield f"B{B}-V{Vq}-{name}-q{int(qf)}t{int(tf)}", *make_pair(1000 * B + 10 * Vq + ti, B, Vq, name, qf, tf, **kw)


def apart_case(B=3, Vq=65):
    """the pair 0.5 m apart: at max_dist = 0.02 every chunk is culled and every output is (+inf, -1, 0)"""
    return make_pair(7, B, Vq, "ico2", offset=(0.5, 0.0, 0.0))


def coincident_case(B=3):
    """the query IS the target's vertices under the same camera and flip: dist is 0"""
    q, t = make_pair(8, B, 1, "ico2")
    return dict(q, verts=t["verts"].copy()), t


def degenerate_case(B, q_flip, t_flip):
    """an 80-face icosphere with a face of two equal indices (a segment), one of three (a point), a NaN vertex (every face on it is
    skipped), an index past V and a negative one; and a query with a NaN and an infinite vertex"""
    q, t = make_pair(9 + B, B, 65, "ico1", q_flip, t_flip)
    f = t["faces"]
    f[3] = (f[3, 0], f[3, 0], f[3, 2])
    f[7] = (f[7, 1], f[7, 1], f[7, 1])
    f[11, 2] = t["verts"].shape[1]
    f[12, 0] = -1
    t["verts"][:, 5, 1] = np.nan
    q["verts"][:, 2, 0] = np.nan
    q["verts"][0, 9, 2] = np.inf
    return q, t


def undecided(ref, max_dist):
    """the vertices whose float64 distance lies within the distance bound of max_dist: they may be finite or +inf"""
    return np.abs(ref["d_min"] - max_dist) <= dist_bound(ref["M"]) if np.isfinite(max_dist) else np.zeros(ref["d_min"].shape, bool)
