"""TEST INFRASTRUCTURE ONLY — the four kernels of csrc/bake.hip restated in float64 NumPy exactly as include/harp_hip.h defines them
(texel map, per-texel accumulation over frames, finish, 3 x 3 dilation), plus, per case, the items whose accept / reject test flips
within a small margin ("undecidable": a float32 input rounded differently could decide them the other way), which the comparisons
against the device leave out.  Anchored on closed forms by tests/test_bake_cpu.py."""
import numpy as np

EDGE_MARGIN = 1e-4        # texel: distance of a texel centre to a UV edge of a candidate face
PIXEL_MARGIN = 1e-4       # px: distance of a projected texel to a pixel boundary
DEPTH_MARGIN = 1e-5       # relative to z: distance of z to the depth threshold
COS_MARGIN = 1e-5         # distance of cosv to cos_min
DEFAULTS = dict(depth_tol=4e-3, cos_min=0.2, cos_power=2.0, shade_floor=0.1)
REASONS = ("row", "behind", "outside", "no_face", "occluded", "mask", "angle")


def texel_coords(verts_uvs, Ht, Wt):
    """texel-space coordinates of the UV vertices: tx = u (Wt - 1), ty = (1 - v) (Ht - 1)"""
    uv = np.asarray(verts_uvs, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    return np.stack([uv[:, 0] * (Wt - 1), (1.0 - uv[:, 1]) * (Ht - 1)], 1)


def _seg_dist(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    t = np.clip(((px - ax) * dx + (py - ay) * dy) / l2, 0.0, 1.0) if l2 > 0 else 0.0
    return np.hypot(px - (ax + t * dx), py - (ay + t * dy))


def texel_map(verts_uvs, faces_uvs, Ht, Wt):
    """-> texel_face (Ht,Wt) int32 (-1: none), texel_bary (Ht,Wt,2) float64, undecided (Ht,Wt) bool"""
    P = texel_coords(verts_uvs, Ht, Wt)
    faces_uvs = np.asarray(faces_uvs).reshape(-1, 3)
    big = np.iinfo(np.int32).max
    face = np.full((Ht, Wt), big, dtype=np.int64)
    und = np.zeros((Ht, Wt), dtype=bool)
    for f, (i0, i1, i2) in enumerate(faces_uvs):
        (x0, y0), (x1, y1), (x2, y2) = P[i0], P[i1], P[i2]
        if not np.all(np.isfinite([x0, y0, x1, y1, x2, y2])):
            continue
        xs, ys = (x0, x1, x2), (y0, y1, y2)
        if max(xs) < -1 or max(ys) < -1 or min(xs) > Wt or min(ys) > Ht:
            continue
        xa, xb = int(max(np.floor(min(xs)) - 1, 0)), int(min(np.ceil(max(xs)) + 1, Wt - 1))
        ya, yb = int(max(np.floor(min(ys)) - 1, 0)), int(min(np.ceil(max(ys)) + 1, Ht - 1))
        if xa > xb or ya > yb:
            continue
        py, px = np.meshgrid(np.arange(ya, yb + 1, dtype=np.float64), np.arange(xa, xb + 1, dtype=np.float64), indexing="ij")
        d = np.minimum(np.minimum(_seg_dist(px, py, x0, y0, x1, y1), _seg_dist(px, py, x1, y1, x2, y2)), _seg_dist(px, py, x2, y2, x0, y0))
        und[ya:yb + 1, xa:xb + 1] |= d < EDGE_MARGIN
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        e0 = (x1 - px) * (y2 - py) - (y1 - py) * (x2 - px)
        e1 = (x2 - px) * (y0 - py) - (y2 - py) * (x0 - px)
        e2 = (x0 - px) * (y1 - py) - (y0 - py) * (x1 - px)
        inside = (e0 / area >= 0) & (e1 / area >= 0) & (e2 / area >= 0)
        sl = face[ya:yb + 1, xa:xb + 1]
        sl[inside] = np.minimum(sl[inside], f)
    bary = np.zeros((Ht, Wt, 2))
    ys, xs = np.nonzero(face != big)
    for y, x in zip(ys, xs):
        i0, i1, i2 = faces_uvs[face[y, x]]
        (x0, y0), (x1, y1), (x2, y2) = P[i0], P[i1], P[i2]
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        bary[y, x, 0] = ((x1 - x) * (y2 - y) - (y1 - y) * (x2 - x)) / area
        bary[y, x, 1] = ((x2 - x) * (y0 - y) - (y2 - y) * (x0 - x)) / area
    face[face == big] = -1
    return face.astype(np.int32), bary, und


def new_accumulators(Ht, Wt):
    return {"sum_w": np.zeros((Ht, Wt)), "sum_wc": np.zeros((Ht, Wt, 3)), "sum_wc2": np.zeros((Ht, Wt, 3)),
            "count": np.zeros((Ht, Wt), dtype=np.int32), "best_cos": np.full((Ht, Wt), -1.0, dtype=np.float32)}


def _unit(a):
    return a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-6)


def accumulate(acc, texel_face, texel_bary, faces, ndc, face_id, zbuf, y_true, y_mask, rows, texel_idx=None, verts=None, vnormals=None,
               cam_pos=None, light_pos=None, colors=None, depth_tol=DEFAULTS["depth_tol"], cos_min=DEFAULTS["cos_min"],
               cos_power=DEFAULTS["cos_power"], shade_floor=DEFAULTS["shade_floor"]):
    """Adds the frames to `acc` in place (frame order).  Every array is what the device call receives (float32 data), evaluated in float64.
    -> dict: observed (B,n) bool, undecided (n,) bool (any undecidable pair of the texel), reasons {name: number of (texel, frame) pairs
    rejected FIRST by that test}, texels (n,) flat texel indices, covered (n,) bool (the texel has a usable face)."""
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)      # noqa: E731
    texel_face = np.asarray(texel_face)
    Ht, Wt = texel_face.shape
    tb = f64(texel_bary).reshape(-1, 2)
    faces = np.asarray(faces).reshape(-1, 3)
    ndc, zbuf, y_true, y_mask = f64(ndc), f64(zbuf), f64(y_true), f64(y_mask)
    face_id, rows = np.asarray(face_id), np.asarray(rows).reshape(-1)
    verts, vnormals, cam_pos, light_pos, colors = f64(verts), f64(vnormals), f64(cam_pos), f64(light_pos), f64(colors)
    B, V, _ = ndc.shape
    S, N = face_id.shape[-1], y_true.shape[0]
    y_mask = y_mask.reshape(N, S, S)
    depth_tol, cos_min, cos_power, shade_floor = (float(np.float32(v)) for v in (depth_tol, cos_min, cos_power, shade_floor))
    t = np.arange(Ht * Wt) if texel_idx is None else np.asarray(texel_idx).reshape(-1).astype(np.int64)
    n = t.shape[0]
    f = texel_face.reshape(-1)[t]
    cov = (f >= 0) & (f < faces.shape[0])
    tri = faces[np.where(cov, f, 0)]                                             # (n,3)
    cov &= ((tri >= 0) & (tri < V)).all(1)
    tri = np.where(cov[:, None], tri, 0)
    b = np.concatenate([tb[t], 1.0 - tb[t].sum(1, keepdims=True)], 1)            # (n,3)
    observed = np.zeros((B, n), dtype=bool)
    undecided = np.zeros(n, dtype=bool)
    reasons = dict.fromkeys(REASONS, 0)
    half = 0.5 * S
    sw, sc, sc2 = acc["sum_w"].reshape(-1), acc["sum_wc"].reshape(-1, 3), acc["sum_wc2"].reshape(-1, 3)
    cnt, best = acc["count"].reshape(-1), acc["best_cos"].reshape(-1)
    for k in range(B):
        alive = cov.copy()

        def reject(name, ok):
            nonlocal alive
            reasons[name] += int((alive & ~ok).sum())
            alive = alive & ok

        row = int(rows[k])
        reject("row", np.full(n, 0 <= row < N))
        if not alive.any():
            continue
        p = ndc[k][tri]                                                          # (n,3,3)
        z = (b * p[:, :, 2]).sum(1)
        undecided |= alive & (np.abs(z) < 1e-6)
        reject("behind", z > 0)
        zs = np.where(z > 0, z, 1.0)
        x = (b * p[:, :, 0] * p[:, :, 2]).sum(1) / zs
        y = (b * p[:, :, 1] * p[:, :, 2]).sum(1) / zs
        fx, fy = (1.0 - x) * half, (1.0 - y) * half
        near = (np.abs(fx - np.round(fx)) < PIXEL_MARGIN) | (np.abs(fy - np.round(fy)) < PIXEL_MARGIN)
        # the same coordinate in float32 arithmetic landing in another pixel (a changed floor) is undecidable as well
        x32 = (np.float32(1.0) - x.astype(np.float32)) * np.float32(half)
        y32 = (np.float32(1.0) - y.astype(np.float32)) * np.float32(half)
        with np.errstate(invalid="ignore"):
            near |= (np.floor(x32) != np.floor(fx)) | (np.floor(y32) != np.floor(fy))
        undecided |= alive & near
        inside = (fx >= 0) & (fx < S) & (fy >= 0) & (fy < S)
        reject("outside", inside)
        ix = np.where(inside, np.floor(fx), 0).astype(np.int64)
        iy = np.where(inside, np.floor(fy), 0).astype(np.int64)
        reject("no_face", face_id[k, iy, ix] >= 0)
        thr = zbuf[k, iy, ix] * (1.0 + depth_tol)
        undecided |= alive & (np.abs(z - thr) < DEPTH_MARGIN * np.abs(z))
        reject("occluded", z <= thr)
        reject("mask", y_mask[row, iy, ix] >= 0.5)
        cosv, shade, spec = np.ones(n), np.ones((n, 3)), np.zeros((1, 3))
        if vnormals is not None:
            nh = _unit((b[:, :, None] * vnormals[k][tri]).sum(1))
            pw = (b[:, :, None] * verts[k][tri]).sum(1)
            cosv = (nh * _unit(cam_pos[k][None] - pw)).sum(1)
            undecided |= alive & (np.abs(cosv - cos_min) < COS_MARGIN)
            reject("angle", cosv >= cos_min)
            if light_pos is not None:
                cosl = np.maximum((nh * _unit(light_pos[k][None] - pw)).sum(1), 0.0)
                shade = np.maximum(colors[k][None, 0:3] + colors[k][None, 3:6] * cosl[:, None], shade_floor)
                spec = colors[k][None, 6:9]
        w = np.ones(n) if vnormals is None else np.maximum(cosv, 0.0) ** cos_power
        cx, cy = np.clip(fx - 0.5, 0.0, S - 1.0), np.clip(fy - 0.5, 0.0, S - 1.0)
        cx, cy = np.where(alive, cx, 0.0), np.where(alive, cy, 0.0)
        x0, y0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, S - 1), np.minimum(y0 + 1, S - 1)
        wx, wy = (cx - x0)[:, None], (cy - y0)[:, None]
        img = y_true[row]
        top = (1.0 - wx) * img[y0, x0] + wx * img[y0, x1]
        bot = (1.0 - wx) * img[y1, x0] + wx * img[y1, x1]
        v = ((1.0 - wy) * top + wy * bot - spec) / shade
        a = alive
        ta = t[a]
        sw[ta] += w[a]
        sc[ta] += w[a, None] * v[a]
        sc2[ta] += w[a, None] * v[a] * v[a]
        cnt[ta] += 1
        best[ta] = np.maximum(best[ta], cosv[a].astype(np.float32))
        observed[k] = a
    return {"observed": observed, "undecided": undecided, "reasons": reasons, "texels": t, "covered": cov}


def finish(acc, min_count=1):
    """-> mean (Ht,Wt,3) float32, var (Ht,Wt,3) float32, seen (Ht,Wt) uint8"""
    w = acc["sum_w"]
    ok = (acc["count"] >= min_count) & (w > 0)
    ws = np.where(ok, w, 1.0)[..., None]
    mu = acc["sum_wc"] / ws
    mean = np.where(ok[..., None], np.clip(mu, 0.0, 1.0), 0.0)
    var = np.where(ok[..., None], np.maximum(acc["sum_wc2"] / ws - mu * mu, 0.0), 0.0)
    return mean.astype(np.float32), var.astype(np.float32), ok.astype(np.uint8)


def dilate(tex, valid, n_pass, allow=None, dtype=np.float32):
    """n_pass Jacobi passes in `dtype` with the kernel's summation order (row-major window, one division) -> (tex, valid uint8)"""
    tex = np.array(tex, dtype=dtype)
    valid = np.asarray(valid) != 0
    Ht, Wt, C = tex.shape
    al = np.ones((Ht, Wt), dtype=bool) if allow is None else np.asarray(allow) != 0
    for _ in range(int(n_pass)):
        src = valid & al
        acc = np.zeros((Ht, Wt, C), dtype=dtype)
        cnt = np.zeros((Ht, Wt), dtype=np.int32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy == 0 and dx == 0:
                    continue
                ys, yd = slice(max(dy, 0), Ht + min(dy, 0)), slice(max(-dy, 0), Ht + min(-dy, 0))
                xs, xd = slice(max(dx, 0), Wt + min(dx, 0)), slice(max(-dx, 0), Wt + min(-dx, 0))
                m = src[ys, xs]
                acc[yd, xd] = np.where(m[..., None], (acc[yd, xd] + tex[ys, xs]).astype(dtype), acc[yd, xd])
                cnt[yd, xd] += m
        fill = ~valid & al & (cnt > 0)
        filled = (acc / np.maximum(cnt, 1)[..., None].astype(dtype)).astype(dtype)
        tex = np.where(fill[..., None], filled, tex)
        valid = valid | fill
    return tex, valid.astype(np.uint8)


def textured_quad_scene(S=32, Ht=17, Wt=17, z=2.0, extent=0.5, flip=False):
    """A fronto-parallel quad (two triangles) that maps the whole atlas onto the NDC square [-extent, extent]^2 at depth z: inputs of
    `accumulate` without a rasteriser, with face_id / zbuf filled analytically.  -> dict"""
    verts_uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    sx = -1.0 if flip else 1.0
    ndc = np.array([[[-extent * sx, -extent, z], [extent * sx, -extent, z], [extent * sx, extent, z], [-extent * sx, extent, z]]], dtype=np.float32)
    i = np.arange(S)
    c = -1.0 + (2.0 * (S - 1 - i) + 1.0) / S                                     # pix_to_ndc
    inside = (np.abs(c)[None, :] <= extent) & (np.abs(c)[:, None] <= extent)
    face_id = np.where(inside, 0, -1).astype(np.int32)[None]
    zbuf = np.where(inside, z, -1.0).astype(np.float32)[None]
    return dict(verts_uvs=verts_uvs, faces_uvs=faces, faces=faces, ndc=ndc, face_id=face_id, zbuf=zbuf, S=S, Ht=Ht, Wt=Wt)
