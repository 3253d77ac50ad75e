"""float64 numpy restatement of harp_composite_layers_u8 (csrc/composite.hip), literally as include/harp_hip.h states it: the yardstick of
tests/test_layers_cpu.py and tests/test_gpu_scene_player.py.  float32 depths convert to float64 exactly, so coverage, winners, n, alpha and
owner are decided bit for bit; only the colour rounding is not.  (tests/_scene.py is something else: the synthetic fitting scene.)"""
import numpy as np


def quantise(v):
    return np.clip(np.floor(255.0 * v + 0.5), 0, 255).astype(np.int64)


def composite_layers(layers, ss, scene_z=None, scene_rows=None, bg=None, bg_rows=None, bg_color=(1.0, 1.0, 1.0), channels=3):
    """layers: [(rgb (B, S ss, S ss, 3) float32, zbuf (B, S ss, S ss) float32, flip)] -> dict(out (B,S,S,channels) uint8, v255 (B,S,S,3)
    float64 = 255 v before rounding, n (B,S,S) covered sub-samples, owner (B,S,S) uint8)"""
    L = len(layers)
    z0 = np.asarray(layers[0][1])
    B, Sh = z0.shape[:2]
    S, N = Sh // ss, ss * ss
    # the background bytes, as harp_resolve_u8
    color_b = quantise(np.fmin(np.fmax(np.asarray(bg_color, np.float32).astype(np.float64), 0.0), 1.0))
    back = np.broadcast_to(color_b, (B, S, S, 3)).copy()
    if bg is not None:
        bg = np.asarray(bg)
        rows = np.asarray(bg_rows) if bg_rows is not None else (np.arange(B) if bg.shape[0] == B else np.zeros(B, np.int64))
        for b in range(B):
            if 0 <= rows[b] < bg.shape[0]:
                back[b] = bg[rows[b]]
    # the scene depth per output pixel: 0 where there is none
    d = np.zeros((B, S, S))
    if scene_z is not None:
        scene_z = np.asarray(scene_z, np.float32).astype(np.float64)
        rows = np.asarray(scene_rows) if scene_rows is not None else (np.arange(B) if scene_z.shape[0] == B else np.zeros(B, np.int64))
        for b in range(B):
            if 0 <= rows[b] < scene_z.shape[0]:
                d[b] = scene_z[rows[b]]
    with np.errstate(invalid="ignore"):
        d_valid = d > 0                                    # (a NaN is not)
        d_sub = np.repeat(np.repeat(np.where(d_valid, d, np.inf), ss, 1), ss, 2)
        dv_sub = np.repeat(np.repeat(d_valid, ss, 1), ss, 2)
        zs, cs = [], []
        for rgb, z, flip in layers:
            rgb, z = np.asarray(rgb, np.float32).astype(np.float64), np.asarray(z, np.float32).astype(np.float64)
            if flip:                                       # read at sub-column S ss - 1 - X
                rgb, z = rgb[:, :, ::-1], z[:, :, ::-1]
            cand = (z > 0) & (~dv_sub | (z < d_sub))
            zs.append(np.where(cand, z, np.nan))
            cs.append(np.fmin(np.fmax(rgb, 0.0), 1.0))     # (fmax / fmin ignore a NaN: it becomes 0)
    zs, cs = np.stack(zs), np.stack(cs)
    cand = ~np.isnan(zs)
    covered = cand.any(0)
    key = np.where(cand, zs, np.inf)
    # the smallest depth, the lowest index among equals; a candidate at +inf still beats a non-candidate
    best = key.min(0)
    win = np.full(covered.shape, -1, np.int64)
    for l in range(L - 1, -1, -1):
        win = np.where(cand[l] & (key[l] == best), l, win)
    col = np.zeros(covered.shape + (3,))
    for l in range(L):
        col = np.where((win == l)[..., None], cs[l], col)
    cov5 = covered.reshape(B, S, ss, S, ss)
    n = cov5.sum((2, 4))
    tot = (col * covered[..., None]).reshape(B, S, ss, S, ss, 3).sum((2, 4))
    v255 = 255.0 * (tot + (N - n)[..., None] * (back / 255.0)) / N
    out = np.where((n == 0)[..., None], back, np.clip(np.floor(v255 + 0.5), 0, 255).astype(np.int64))
    if channels == 4:
        out = np.concatenate([out, ((255 * n + N // 2) // N)[..., None]], -1)
    counts = np.stack([(win == l).reshape(B, S, ss, S, ss).sum((2, 4)) for l in range(L)])
    owner = np.where(n == 0, 0, counts.argmax(0) + 1)        # (argmax: the first of equal counts, the lower index)
    return dict(out=out.astype(np.uint8), v255=v255, n=n, owner=owner.astype(np.uint8))
