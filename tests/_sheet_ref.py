"""numpy float32 restatement of harp_sheet_u8 (include/harp_hip.h): the same IEEE operations in the same order — per source pixel the
colour of its mode, per output pixel np.float32 adds over the d x d box offsets in row-major order from 0, a float32 division by the
number of pixels summed, `* np.float32(255)` and truncation — so modes 0, 1 and 2 compare bit for bit."""
import numpy as np

F = np.float32


def clip01(x):
    return np.fmin(np.fmax(x, F(0)), F(1))                       # fminf(fmaxf(x, 0), 1): a NaN counts as 0


def colours(mode, a, b=None, mask=None):
    """(N,H,W,3) float32 colours of the source pixels; a, b (N,H,W,C) (masks (N,H,W) in mode 1), mask (N,H,W)"""
    a = np.asarray(a, F)
    if mode == 0:
        return clip01(a[..., :3])
    if mode == 1:
        return np.stack([clip01(a), np.zeros_like(a), clip01(np.asarray(b, F))], -1)
    if mode == 2:
        m = np.asarray(mask, F)[..., None]
        return clip01(np.abs(a[..., :3] * m - np.asarray(b, F)[..., :3] * m))       # two float32 products, one float32 difference
    raise ValueError(mode)


def box_sheet(p, grid=(3, 3), d=1):
    """(N,H,W,3) float32 colours -> (rows * ch, cols * cw, 3) uint8 sheet"""
    N, H, W, _ = p.shape
    rows, cols = grid
    ch, cw = -(-H // d), -(-W // d)
    pad = np.zeros((N, ch * d, cw * d, 3), F)
    pad[:, :H, :W] = p
    s, cnt = np.zeros((N, ch, cw, 3), F), np.zeros((ch, cw), F)
    for dy in range(d):                                          # row-major over the box; an offset past the edge adds an exact 0
        for dx in range(d):
            ys, xs = np.arange(ch) * d + dy, np.arange(cw) * d + dx
            valid = ((ys < H)[:, None] & (xs < W)[None, :])
            s = s + np.where(valid[None, :, :, None], pad[:, ys][:, :, xs], F(0))
            cnt = cnt + valid.astype(F)
    u8 = ((s / cnt[None, :, :, None]) * F(255)).astype(np.uint8)
    assert s.dtype == F and cnt.dtype == F
    out = np.full((rows * ch, cols * cw, 3), 255, np.uint8)
    for k in range(N):
        r, c = divmod(k, cols)
        out[r * ch:(r + 1) * ch, c * cw:(c + 1) * cw] = u8[k]
    return out


def numpy_sheet(mode, a, b=None, mask=None, grid=(3, 3), d=1):
    return box_sheet(colours(mode, a, b, mask), grid, d)


def normal_levels_f64(a):
    """float64 value * 255 of mode 3 for (N,H,W,3) maps: clip(a / max(|a|, 1e-12) * 0.5 + 0.5) * 255"""
    a = np.asarray(a, np.float64)
    n = np.maximum(np.sqrt((a * a).sum(-1, keepdims=True)), 1e-12)
    return np.clip(a / n * 0.5 + 0.5, 0, 1) * 255
