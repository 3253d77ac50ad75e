"""float64 numpy restatement of harp_annotate_layers and harp_keypoint_visibility (csrc/annotate.hip), literally as include/harp_hip.h
states them: the yardstick of tests/test_annotate_cpu.py and tests/test_gpu_annotate.py.  float32 depths convert to float64 exactly, so
winners, owner, part, face, depth and the boxes are decided bit for bit; only uv and (u, v, Z) carry rounding.  The winner rule is
tests/_layers_ref.py's (test_annotate_cpu.py holds the two owners against each other)."""
import numpy as np

K_EPS = 1e-8                                           # csrc/harp_common.h kEps
SEED_KEYPOINTS = 3207                                  # the keypoint inputs of test_gpu_annotate.py, which test_annotate_cpu.py proves decidable


def scene_per_frame(scene_z, scene_rows, B, S):
    """(n_scene,S,S) and rows -> (B,S,S) float64, 0 where there is none (tests/_layers_ref.py's rule)"""
    d = np.zeros((B, S, S))
    if scene_z is not None:
        scene_z = np.asarray(scene_z, np.float32).astype(np.float64)
        rows = np.asarray(scene_rows) if scene_rows is not None else (np.arange(B) if scene_z.shape[0] == B else np.zeros(B, np.int64))
        for b in range(B):
            if 0 <= rows[b] < scene_z.shape[0]:
                d[b] = scene_z[rows[b]]
    return d


def winners(zs, flips, ss, scene_z=None, scene_rows=None):
    """zs: per layer (B, S ss, S ss) float32 -> (win (B, S ss, S ss) int64: the winning layer per output sub-sample or -1, z (.., float64)
    its depth, d (B,S,S) the scene depth per frame).  Candidate: z > 0 and in front of a valid scene depth; the smallest z, the lowest
    index among equals; a flipped layer is read at sub-column S ss - 1 - X."""
    z0 = np.asarray(zs[0])
    B, Sh = z0.shape[:2]
    S = Sh // ss
    d = scene_per_frame(scene_z, scene_rows, B, S)
    with np.errstate(invalid="ignore"):
        d_valid = np.repeat(np.repeat(d > 0, ss, 1), ss, 2)
        d_sub = np.repeat(np.repeat(np.where(d > 0, d, np.inf), ss, 1), ss, 2)
        win, zw = np.full((B, Sh, Sh), -1, np.int64), np.zeros((B, Sh, Sh))
        for l, (z, flip) in enumerate(zip(zs, flips)):
            z = np.asarray(z, np.float32).astype(np.float64)
            z = z[:, :, ::-1] if flip else z
            take = (z > 0) & (~d_valid | (z < d_sub)) & ((win < 0) | (z < zw))      # (strictly nearer than an earlier layer)
            win, zw = np.where(take, l, win), np.where(take, z, zw)
    return win, zw, d


def vote(samples):
    """The three rules on ONE output pixel: samples = [(layer or -1, label, z, face)] in row-major order of the sub-samples ->
    (owner, part, index of the representative sample or -1)."""
    L = 1 + max([s[0] for s in samples] + [0])
    counts = [sum(1 for s in samples if s[0] == l) for l in range(L)]
    if max(counts) == 0:
        return 0, 0, -1
    ol = int(np.argmax(counts))                          # (the first of equal counts: the lower index)
    mine = [i for i, s in enumerate(samples) if s[0] == ol]
    labels = sorted({samples[i][1] for i in mine})
    part = max(labels, key=lambda lab: (sum(1 for i in mine if samples[i][1] == lab), -lab))
    rep = -1
    for i in mine:
        if samples[i][1] == part and (rep < 0 or samples[i][2] < samples[rep][2]):
            rep = i
    return ol + 1, int(part), rep


def edge_fn(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def bary(tri, px, py):
    """csrc/shade_common.h bary_fwd in float64: tri (3,3) = three (x_ndc, y_ndc, z_view) rows -> the perspective-corrected (b0, b1, b2)"""
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = tri
    area = edge_fn(x2, y2, x0, y0, x1, y1) + K_EPS
    w0, w1, w2 = edge_fn(px, py, x1, y1, x2, y2) / area, edge_fn(px, py, x2, y2, x0, y0) / area, edge_fn(px, py, x0, y0, x1, y1) / area
    t = np.array([w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2])
    return t / max(t.sum(), K_EPS)


def annotate_layers(layers, ss, scene_z=None, scene_rows=None, uv=False):
    """layers: [dict(face_id (B, S ss, S ss) int32, zbuf float32, face_label (F,) uint8, flip [, ndc (B,V,3), faces (F,3), verts_uvs (Vt,2),
    faces_uvs (F,3)])] -> dict(owner, part uint8 (B,S,S), depth float64, face int64, uv float64 (B,S,S,2), bbox (B,L,4) int64 = (xmin, ymin,
    xmax, ymax) or -1)"""
    L = len(layers)
    flips = [bool(l["flip"]) for l in layers]
    win, zw, _ = winners([l["zbuf"] for l in layers], flips, ss, scene_z, scene_rows)
    B, Sh = win.shape[:2]
    S = Sh // ss
    fids = [np.asarray(l["face_id"])[:, :, ::-1] if f else np.asarray(l["face_id"]) for l, f in zip(layers, flips)]
    out = dict(owner=np.zeros((B, S, S), np.uint8), part=np.zeros((B, S, S), np.uint8), depth=np.zeros((B, S, S)),
               face=np.full((B, S, S), -1, np.int64), uv=np.zeros((B, S, S, 2)), bbox=np.full((B, L, 4), -1, np.int64))
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
                owner, part, rep = vote(samples)
                if owner == 0:
                    continue
                l, _, z, f = samples[rep]
                out["owner"][b, y, x], out["part"][b, y, x], out["depth"][b, y, x], out["face"][b, y, x] = owner, part, z, f
                if uv and 0 <= f < np.asarray(layers[l]["face_label"]).shape[0]:
                    lay = layers[l]
                    Y, X = where[rep]
                    Xs = Sh - 1 - X if flips[l] else X    # the SOURCE sub-pixel the layer was read at
                    px, py = 1.0 - 2.0 * (Xs + 0.5) / Sh, 1.0 - 2.0 * (Y + 0.5) / Sh
                    tri = np.asarray(lay["ndc"], np.float32).astype(np.float64)[b][np.asarray(lay["faces"])[f]]
                    bc = bary(tri, px, py)
                    out["uv"][b, y, x] = bc @ np.asarray(lay["verts_uvs"], np.float32).astype(np.float64)[np.asarray(lay["faces_uvs"])[f]]
        for l in range(L):
            ys, xs = np.nonzero(out["owner"][b] == l + 1)
            if ys.size:
                out["bbox"][b, l] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def project(joints, R, T, focal, S):
    """harp_project_fwd's view transform (view = j @ R (3,3) + T) and the pixel, float64: joints (B,NJ,3), R (B,9), T (B,3) ->
    (u, v, Z) (B,NJ,3), no case handled"""
    j = np.asarray(joints, np.float32).astype(np.float64)
    R = np.asarray(R, np.float32).astype(np.float64).reshape(-1, 3, 3)
    view = np.einsum("bji,bik->bjk", j, R) + np.asarray(T, np.float32).astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = S / 2.0 - focal * view[..., 0] / view[..., 2]
        v = S / 2.0 - focal * view[..., 1] / view[..., 2]
    return np.stack([u, v, view[..., 2]], -1)


def keypoint_visibility(joints, R, T, focal, S, ss, self_layer, zs, flips, scene_z=None, scene_rows=None, tol=0.02):
    """-> dict(uvz (B,NJ,3) float64, vis (B,NJ,2) uint8, decidable (B,NJ) bool).  A joint is UNDECIDABLE in float32 when
    |z_near - (Z - tol)| < 1e-5 m, or u ss or v ss lies within 1e-3 of an integer (the image's edges included)."""
    focal, tol = float(np.float32(focal)), float(np.float32(tol))
    uvz = project(joints, R, T, focal, S)
    B, NJ = uvz.shape[:2]
    win, zw, d = winners(zs, flips, ss, scene_z, scene_rows)
    Sh = S * ss
    vis, ok = np.zeros((B, NJ, 2), np.uint8), np.ones((B, NJ), bool)
    for b in range(B):
        for k in range(NJ):
            u, v, Z = uvz[b, k]
            if not Z > 1e-3:
                uvz[b, k] = 0.0
                continue
            if flips[self_layer]:
                u = uvz[b, k, 0] = S - u
            if np.isfinite(u) and np.isfinite(v) and min(abs(u * ss - round(u * ss)), abs(v * ss - round(v * ss))) < 1e-3:
                ok[b, k] = False
            if not (np.isfinite(Z) and 0 <= u < S and 0 <= v < S):
                continue
            X, Y = min(int(u * ss), Sh - 1), min(int(v * ss), Sh - 1)
            l = int(win[b, Y, X])
            dd = d[b, Y // ss, X // ss]
            near, by = (zw[b, Y, X], 1 + l) if l >= 0 else ((dd, 255) if dd > 0 else (None, 0))
            if near is not None and abs(near - (Z - tol)) < 1e-5:
                ok[b, k] = False
            visible = near is None or near >= Z - tol
            vis[b, k] = (2, 0) if visible else (1, by)
    return dict(uvz=uvz, vis=vis, decidable=ok)


# ---- seeded inputs shared by the CPU and the GPU tests ------------------------------------------------------------------------------
def label_case(rng, L, B, S, ss, F=40, n_labels=3):
    """Synthetic layers for the exact maps: depths as tests/test_gpu_scene_player.py's (uniform in [0.2, 1.0], half of them snapped to
    eighths so that equal depths occur WITHIN a pixel, ~40 % holes of -1, a sprinkle of 0, NaN and +inf, and on 10 % of the sub-samples a
    copy of an earlier layer's depth at the same or the mirrored place: exact ties between layers); face ids in [0, F) where the depth is
    positive, -1 in the holes, and a sprinkle of -1 and of ids past the table (F + 5) ON covered samples; tables of n_labels distinct
    labels so that label ties occur."""
    Sh = S * ss
    out = []
    for _ in range(L):
        z = rng.uniform(0.2, 1.0, size=(B, Sh, Sh)).astype(np.float32)
        z = np.where(rng.uniform(size=z.shape) < 0.5, np.round(z * 8) / 8, z).astype(np.float32)
        z[rng.uniform(size=z.shape) < 0.4] = -1.0
        for v in (0.0, np.nan, np.inf):
            z.reshape(-1)[rng.integers(0, z.size, size=max(1, z.size // 100))] = v
        out.append(dict(zbuf=z))
    for l in range(1, L):
        src = out[rng.integers(0, l)]["zbuf"]
        same, mirrored = rng.uniform(size=src.shape) < 0.05, rng.uniform(size=src.shape) < 0.05
        out[l]["zbuf"] = np.where(same, src, np.where(mirrored, src[:, :, ::-1], out[l]["zbuf"])).astype(np.float32)
    for lay in out:
        z = lay["zbuf"]
        with np.errstate(invalid="ignore"):
            fid = np.where(z > 0, rng.integers(0, F, size=z.shape), -1).astype(np.int32)
        fid.reshape(-1)[rng.integers(0, fid.size, size=max(1, fid.size // 50))] = -1
        fid.reshape(-1)[rng.integers(0, fid.size, size=max(1, fid.size // 50))] = F + 5
        lay["face_id"] = fid
        lay["face_label"] = rng.integers(1, n_labels + 1, size=F).astype(np.uint8)
    return out


def scene_case(rng, kind, B, S):
    """the scene depth of a case: kind "none" | "one" | "per_row" | "rows" -> (scene_z or None, scene_rows or None); zeros on 20 %, a few
    NaN; "rows" has one entry out of range (no scene depth for that frame)"""
    n = {"none": 0, "one": 1, "per_row": B, "rows": 4}[kind]
    if not n:
        return None, None
    sz = rng.uniform(0.2, 1.0, size=(n, S, S)).astype(np.float32)
    sz[rng.uniform(size=sz.shape) < 0.2] = 0.0
    sz.reshape(-1)[rng.integers(0, sz.size, size=max(1, sz.size // 50))] = np.nan
    rows = None
    if kind == "rows":
        rows = rng.integers(0, 4, size=B).astype(np.int32)
        rows[rng.integers(0, B)] = [-1, 4][int(rng.integers(0, 2))]
    return sz, rows


KP_S, KP_B, KP_NJ, KP_FOCAL, KP_FLIPS = 64, 4, 21, 120.0, (False, True, False)      # (the players' tests run at 64 pixels too: one bound)


def keypoint_case(ss, seed=SEED_KEYPOINTS):
    """Seeded joints and crafted depth layers at S = 64, B = 4, three layers (the middle one flipped) -> dict(joints (B,21,3), R (B,9), T
    (B,3) float32 — the player's camera, R = diag(-1,-1,1), T = (-cam1, -cam2, t_z) with t_z around 0.5 m —, zs: three (B, S ss, S ss)
    float32, scene_z (B,S,S)).  The joints' view depth is t_z +- 0.05.  Layer 0 is a skin around t_z +- 0.06 with holes (a joint is in
    front of it, just under it, or deep behind it: self-occluded for self_layer 0), layer 1 a nearer sheet over the left half (hides),
    layer 2 a far sheet, the scene depth a near block in one corner with zeros and NaN elsewhere.  Joint 3 of every frame lies far
    outside the image, joint 7 behind the camera (Z < 0)."""
    rng = np.random.default_rng(seed + ss)
    S, B, NJ, Sh = KP_S, KP_B, KP_NJ, KP_S * ss
    cam12, tz = rng.uniform(-0.02, 0.02, size=(B, 2)), rng.uniform(0.45, 0.55, size=B)
    R = np.tile(np.array([-1, 0, 0, 0, -1, 0, 0, 0, 1], np.float32), (B, 1))
    T = np.concatenate([-cam12, tz[:, None]], 1).astype(np.float32)
    j = np.concatenate([rng.uniform(-0.12, 0.12, size=(B, NJ, 2)), rng.uniform(-0.05, 0.05, size=(B, NJ, 1))], -1)
    j[:, 3, 0] = 0.5                                     # u far outside [0, S)
    j[:, 7, 2] = -tz - 0.1                               # Z = -0.1
    hole = lambda p: rng.uniform(size=(B, Sh, Sh)) < p      # noqa: E731
    z0 = np.where(hole(0.3), -1.0, tz[:, None, None] + rng.uniform(-0.06, 0.06, size=(B, Sh, Sh)))
    z1 = np.where(hole(0.3), -1.0, tz[:, None, None] - 0.1 + rng.uniform(-0.02, 0.02, size=(B, Sh, Sh)))
    z1[:, :, Sh // 2:] = -1.0
    z2 = np.where(hole(0.5), -1.0, tz[:, None, None] + 0.2 + rng.uniform(-0.02, 0.02, size=(B, Sh, Sh)))
    sc = np.zeros((B, S, S))
    sc[:, S // 2:, S // 2:] = tz[:, None, None] - 0.2
    sc.reshape(-1)[rng.integers(0, sc.size, size=sc.size // 50)] = np.nan
    f32 = lambda a: np.ascontiguousarray(a, np.float32)      # noqa: E731
    return dict(joints=f32(j), R=R, T=T, zs=[f32(z0), f32(z1), f32(z2)], scene_z=f32(sc))
