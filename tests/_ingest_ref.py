"""numpy restatement of harp_targets_from_u8 (include/harp_hip.h, csrc/ingest.hip) and the cases its tests share: subsample first, the
5 x 5 minimum over the window clipped to the image on the uint8 codes, then (u.astype(float64) / 255).astype(float32) — the conversion
the host path performs (numpy's float64 division, then torch.Tensor).  tests/test_ingest_cpu.py pins it to load_img on the CPU."""
import numpy as np
from PIL import Image

# (H0, W0): a tile of 16 x 64 output pixels and its halo of 2 at every offset from an image border, and images smaller than the window
SIZES = [(1, 1), (2, 3), (5, 5), (15, 62), (16, 64), (17, 65), (18, 66), (19, 67), (33, 130)]
FACTORS = [1, 2, 3]


def unit(u):
    return (np.asarray(u).astype(np.float64) / 255).astype(np.float32)


def min5x5(m):
    """(..., H, W) uint8 -> the minimum over the 5 x 5 window clipped to the image"""
    H, W = m.shape[-2:]
    p = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(2, 2), (2, 2)], mode="constant", constant_values=255)
    return np.minimum.reduce([p[..., dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)])


def targets(rgb, mask, d=1):
    """rgb (N,H0,W0,3), mask (N,H0,W0) uint8 -> y_true (N,H,W,3), y_sil (N,H,W), y_sil_col (N,H,W) float32"""
    rgb, mask = np.asarray(rgb)[:, ::d, ::d], np.asarray(mask)[:, ::d, ::d]
    return unit(rgb), unit(mask), unit(min5x5(mask))


def make_frames(n, H0, W0, seed):
    """seeded uint8 frames: random colours; masks = random codes (every window minimum is decided by one pixel) with a block of 255 so that
    some windows keep a high value"""
    g = np.random.default_rng(seed)
    rgb = g.integers(0, 256, (n, H0, W0, 3), dtype=np.uint8)
    mask = g.integers(0, 256, (n, H0, W0), dtype=np.uint8)
    mask[:, H0 // 4:H0 // 4 + max(1, H0 // 2), W0 // 4:W0 // 4 + max(1, W0 // 2)] = 255
    return rgb, mask


def write_files(folder, rgb, mask):
    """lossless files (the tests' truth is whatever PIL decodes from them) -> (image_paths, mask_paths)"""
    ips, mps = [], []
    for i in range(rgb.shape[0]):
        ips.append(str(folder / ("%04d.png" % i)))
        mps.append(str(folder / ("%04d_mask.png" % i)))
        Image.fromarray(rgb[i], "RGB").save(ips[-1])
        Image.fromarray(mask[i], "L").save(mps[-1])
    return ips, mps


def bad_argument_calls(fn, rgb, mask, y_true, y_sil, y_col):
    """every call of harp_targets_from_u8 that must return HARP_ERR_ARG without a launch: [(what, status)]"""
    ok = dict(rgb=rgb, mask=mask, N=1, H0=4, W0=4, d=1, y_true=y_true, y_sil=y_sil, y_col=y_col)
    cases = [(k, None) for k in ("rgb", "mask", "y_true", "y_sil")]
    cases += [(k, v) for k in ("N", "H0", "W0") for v in (0, -1)]
    cases += [("d", v) for v in (0, -1, 9)]
    out = []
    for k, v in cases:
        a = dict(ok, **{k: v})
        out.append(((k, v), fn(a["rgb"], a["mask"], a["N"], a["H0"], a["W0"], a["d"], a["y_true"], a["y_sil"], a["y_col"], None)))
    big = 2 ** 31 - 1
    # more than 2^31 - 1 tiles of 16 x 64 output pixels: in one frame, over the frames only, and with the fewest tiles per source pixel (d = 8)
    for N, H0, W0, d in [(1, big, big, 1), (big, 16, 128, 1), (big, big, big, 8), (1 << 20, 1 << 20, 1 << 20, 8)]:
        out.append((("size", N, H0, W0, d), fn(rgb, mask, N, H0, W0, d, y_true, y_sil, y_col, None)))
    return out
