"""float64 numpy restatement of harp_flow_layers (csrc/flow.hip), literally as include/harp_hip.h states it: the yardstick of
tests/test_flow_cpu.py and tests/test_gpu_flow.py.  The source point is tests/_annotate_ref.py's (winners, vote, bary: the same owner, face
and barycentric point as the labels).  float32 inputs convert to float64 exactly, so the owner, the face and every comparison of depths
are decided bit for bit; the landing point (cx, cy) and Z' carry rounding, and a pixel whose status hangs on it is flagged UNDECIDABLE.
Also a small float64 rasteriser and the seeded cases, built on the host so that the CPU and the GPU tests see identical inputs."""
import functools

import numpy as np

from tests import _annotate_ref as AR

FLOW_TOL = 0.005
OCCLUDER_SCENE = 255                                   # status[1] of a point hidden by the scene depth
SEED_FLOW = 3301


def flow_layers(layers, to, ss, scene_z=None, scene_rows=None, scene_z_to=None, scene_rows_to=None, tol=FLOW_TOL):
    """layers: [dict(face_id (B, S ss, S ss) int32, zbuf float32, face_label (F,) uint8, flip, ndc (B,V,3) float32, faces (F,3) int32)], to:
    [dict(ndc (B,V,3), zbuf (B, S ss, S ss))] -> dict(flow (B,S,S,2) float64, dz (B,S,S) float64, status (B,S,S,2) uint8, decidable (B,S,S)
    bool).  A pixel is UNDECIDABLE in float32 when cx or cy lies within 1e-3 of an integer (the image's edges included) or
    |z_near - (Z' - tol)| < 1e-5 m."""
    tol = float(np.float32(tol))
    flips = [bool(l["flip"]) for l in layers]
    win, zw, _ = AR.winners([l["zbuf"] for l in layers], flips, ss, scene_z, scene_rows)
    win_to, zw_to, d_to = AR.winners([t["zbuf"] for t in to], flips, ss, scene_z_to, scene_rows_to)
    B, Sh = win.shape[:2]
    S = Sh // ss
    fids = [np.asarray(l["face_id"])[:, :, ::-1] if f else np.asarray(l["face_id"]) for l, f in zip(layers, flips)]
    f64 = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    ndc, ndc_to = [f64(l["ndc"]) for l in layers], [f64(t["ndc"]) for t in to]
    out = dict(flow=np.zeros((B, S, S, 2)), dz=np.zeros((B, S, S)), status=np.zeros((B, S, S, 2), np.uint8), decidable=np.ones((B, S, S), bool))
    for b in range(B):
        for y in range(S):
            for x in range(S):
                samples, where = [], []
                for sy in range(ss):
                    for sx in range(ss):
                        Y, X = y * ss + sy, x * ss + sx
                        l = int(win[b, Y, X])
                        if l < 0:
                            samples.append((-1, 0, 0.0, -1))
                        else:
                            f = int(fids[l][b, Y, X])
                            tab = np.asarray(layers[l]["face_label"])
                            samples.append((l, int(tab[f]) if 0 <= f < tab.shape[0] else 0, float(zw[b, Y, X]), f))
                        where.append((Y, X))
                owner, _, rep = AR.vote(samples)
                if owner == 0:
                    continue
                l, _, z, f = samples[rep]
                out["status"][b, y, x] = (1, 0)
                faces = np.asarray(layers[l]["faces"])
                V = ndc[l].shape[1]
                if not 0 <= f < faces.shape[0] or faces[f].min() < 0 or faces[f].max() >= V:
                    continue
                Y, X = where[rep]
                Xs = Sh - 1 - X if flips[l] else X        # the SOURCE sub-pixel the layer was read at
                bc = AR.bary(ndc[l][b][faces[f]], 1.0 - 2.0 * (Xs + 0.5) / Sh, 1.0 - 2.0 * (Y + 0.5) / Sh)
                tri = ndc_to[l][b][faces[f]]
                Zp = float(bc @ tri[:, 2])
                if not Zp > 1e-3:
                    continue
                with np.errstate(all="ignore"):
                    xp, yp = float(bc @ (tri[:, 0] * tri[:, 2])) / Zp, float(bc @ (tri[:, 1] * tri[:, 2])) / Zp
                    cx, cy = (1.0 - xp) * Sh / 2.0, (1.0 - yp) * Sh / 2.0
                if flips[l]:
                    cx = Sh - cx
                if not (np.isfinite(Zp) and np.isfinite(cx) and np.isfinite(cy)):
                    continue
                out["flow"][b, y, x] = ((cx - (X + 0.5)) / ss, (cy - (Y + 0.5)) / ss)
                out["dz"][b, y, x] = Zp - z
                if min(abs(cx - round(cx)), abs(cy - round(cy))) < 1e-3:
                    out["decidable"][b, y, x] = False
                if not (0 <= cx < Sh and 0 <= cy < Sh):
                    out["status"][b, y, x] = (2, 0)
                    continue
                Xt, Yt = min(int(cx), Sh - 1), min(int(cy), Sh - 1)
                lt = int(win_to[b, Yt, Xt])
                dd = d_to[b, Yt // ss, Xt // ss]
                near, by = (zw_to[b, Yt, Xt], 1 + lt) if lt >= 0 else ((dd, OCCLUDER_SCENE) if dd > 0 else (None, 0))
                if near is not None and abs(near - (Zp - tol)) < 1e-5:
                    out["decidable"][b, y, x] = False
                visible = near is None or near >= Zp - tol
                out["status"][b, y, x] = (4, 0) if visible else (3, by)
    return out


def rasterize(ndc, faces, Sh):
    """A float64 rasteriser for the seeded cases: ndc (B,V,3) (x_ndc, y_ndc, z_view > 0), faces (F,3) -> (face_id (B,Sh,Sh) int32, -1 =
    empty; zbuf (B,Sh,Sh) float32, -1 = empty).  A sub-pixel belongs to a face when its centre, 1 - 2 (i + 0.5) / Sh, lies inside it (the
    three edge functions of one sign, zero included); its depth is interpolated in 1/z; the nearest face is kept, the lower index among
    equals."""
    ndc = np.asarray(ndc, np.float32).astype(np.float64)
    B = ndc.shape[0]
    c = 1.0 - 2.0 * (np.arange(Sh) + 0.5) / Sh
    px, py = np.meshgrid(c, c, indexing="xy")            # [Y, X]
    fid, zb = np.full((B, Sh, Sh), -1, np.int32), np.full((B, Sh, Sh), np.inf)
    for b in range(B):
        for f, (i0, i1, i2) in enumerate(np.asarray(faces)):
            (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = ndc[b, i0], ndc[b, i1], ndc[b, i2]
            area = AR.edge_fn(x2, y2, x0, y0, x1, y1)
            if abs(area) < 1e-12:
                continue
            w0, w1, w2 = AR.edge_fn(px, py, x1, y1, x2, y2) / area, AR.edge_fn(px, py, x2, y2, x0, y0) / area, AR.edge_fn(px, py, x0, y0, x1, y1) / area
            z = 1.0 / (w0 / z0 + w1 / z1 + w2 / z2)
            take = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (z < zb[b])
            fid[b], zb[b] = np.where(take, f, fid[b]), np.where(take, z, zb[b])
    return fid, np.where(fid >= 0, zb, -1.0).astype(np.float32)


def grid_mesh(rng, B, scale=1.0):
    """tests/test_gpu_annotate.py's mesh: a 3 x 3 grid of vertices as 8 triangles, every vertex at its own depth in [0.4, 0.9], tilted
    differently per frame -> (ndc (B,9,3) float32, faces (8,3) int32)"""
    g = np.linspace(-0.75, 0.75, 3)
    xy = np.stack(np.meshgrid(g, g, indexing="xy"), -1).reshape(9, 2)
    ndc = np.zeros((B, 9, 3), np.float32)
    for b in range(B):
        ndc[b, :, :2] = (xy + rng.uniform(-0.08, 0.08, size=(9, 2))) * scale
        ndc[b, :, 2] = rng.uniform(0.4, 0.9, size=9)
    faces = []
    for r in range(2):
        for c in range(2):
            a = 3 * r + c
            faces += [[a, a + 1, a + 4], [a, a + 4, a + 3]]
    return ndc, np.array(faces, np.int32)


SCALES = (1.0, 0.8, 0.65, 0.5)                          # later layers are smaller: all show, and they interleave in depth
FLIPS = (False, True, True, False)
KINDS = ("none", "one", "per_row", "rows")
TO_KIND = {"none": "per_row", "one": "none", "per_row": "rows", "rows": "one"}      # the target frames' scene depth: every kind occurs on both sides


def target_scene(rng, kind, B, S):
    """the scene depth of the TARGET frames: a block at 0.3, in front of every mesh, over one quadrant of every other map, nothing elsewhere;
    kind as tests/_annotate_ref.py scene_case -> (scene_z or None, scene_rows or None)"""
    n = {"none": 0, "one": 1, "per_row": B, "rows": 4}[kind]
    if not n:
        return None, None
    sz = np.zeros((n, S, S), np.float32)
    qy, qx = int(rng.integers(0, 2)), int(rng.integers(0, 2))
    sz[::2, qy * (S // 2):qy * (S // 2) + (S + 1) // 2, qx * (S // 2):qx * (S // 2) + (S + 1) // 2] = 0.3
    rows = None
    if kind == "rows":
        rows = rng.integers(0, 4, size=B).astype(np.int32)
        rows[rng.integers(0, B)] = [-1, 4][int(rng.integers(0, 2))]
    return sz, rows


def flow_case(rng, L, B, S, ss, kind, corrupt=True):
    """One seeded case -> dict(layers, to, scene (scene_z, scene_rows), scene_to).  Per layer the grid mesh rasterised by `rasterize`;
    the target is the same mesh shifted by up to +-0.35 ndc per frame, re-tilted by +-0.04 per vertex, depths moved by +-0.05; zbuf_to is
    the moved mesh's own raster, pushed 0.02 nearer on a quarter of the covered samples (self-occlusion), with holes on a tenth and a few
    NaN.  corrupt: face ids of -1 and past the table on covered samples, one face with a vertex index of V, one target vertex with z <= 0
    (all made AFTER the rasters, which stay those of the clean mesh)."""
    Sh = S * ss
    layers, to = [], []
    for l in range(L):
        ndc, faces = grid_mesh(rng, B, SCALES[l])
        fid, zbuf = rasterize(ndc, faces, Sh)
        ndc_to = ndc.copy()
        ndc_to[..., :2] += rng.uniform(-0.35, 0.35, size=(B, 1, 2)) + rng.uniform(-0.04, 0.04, size=(B, 9, 2))
        ndc_to[..., 2] += rng.uniform(-0.05, 0.05, size=(B, 9))
        ndc_to = ndc_to.astype(np.float32)
        _, z_to = rasterize(ndc_to, faces, Sh)
        covered = z_to > 0
        z_to = np.where(covered & (rng.uniform(size=z_to.shape) < 0.25), z_to - np.float32(0.02), z_to)
        z_to = np.where(covered & (rng.uniform(size=z_to.shape) < 0.1), -1.0, z_to).astype(np.float32)
        z_to.reshape(-1)[rng.integers(0, z_to.size, size=max(1, z_to.size // 100))] = np.nan
        faces_k = faces.copy()
        if corrupt:
            cov = np.flatnonzero(fid.reshape(-1) >= 0)
            fid.reshape(-1)[rng.choice(cov, size=max(1, cov.size // 50))] = -1
            fid.reshape(-1)[rng.choice(cov, size=max(1, cov.size // 50))] = faces.shape[0] + 5
            faces_k[rng.integers(0, 8), rng.integers(0, 3)] = 9
            ndc_to[rng.integers(0, B), rng.integers(0, 9), 2] = [0.0, -0.2][int(rng.integers(0, 2))]
        layers.append(dict(face_id=fid, zbuf=zbuf, face_label=rng.integers(1, 4, size=8).astype(np.uint8), flip=FLIPS[l], ndc=ndc, faces=faces_k))
        to.append(dict(ndc=ndc_to, zbuf=z_to))
    return dict(layers=layers, to=to, scene=AR.scene_case(rng, kind, B, S), scene_to=target_scene(rng, TO_KIND[kind], B, S))


CASE_S, CASE_B = 9, 3                                   # 243 pixels: four waves, the last one partial, waves that straddle two frames


@functools.lru_cache(maxsize=None)
def seeded_cases(ss):
    """the cases of one ss, shared by the CPU and the GPU tests and computed once: [(L, kind, case, its float64 result)]"""
    rng = np.random.default_rng(SEED_FLOW + ss)
    out = []
    for L in (1, 2, 4):
        for kind in KINDS:
            c = flow_case(rng, L, CASE_B, CASE_S, ss, kind)
            out.append((L, kind, c, flow_layers(c["layers"], c["to"], ss, *c["scene"], *c["scene_to"], tol=FLOW_TOL)))
    return out
