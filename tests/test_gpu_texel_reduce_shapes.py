"""harp_texel_reduce through the raw C ABI on small maps: both launch shapes (the small job's and the large job's) on hand-made record lists
that cover the 2 048-record chunk boundaries and every path of the in-register combining of a thread's four consecutive records
(csrc/texel_reduce.hip: add_records), against an exact scatter-add of the same footprints.

Maps: 64x64 (four UV tiles) and 70x45 (W x H: partial last tiles, not square), list capacity 4 096.  A list of that capacity holds two
chunks at most, so the tile with THREE chunks sits in a third case with capacity 6 144 on the 70x45 map.

Lists: 0, 1, 2 047, 2 048, 2 049 records, a count above the capacity (clamped), three chunks.  Every list cycles through blocks of 32 records
of each pattern, so that each thread's four records (4 t .. 4 t + 3 of a chunk) are: all on one texel; alternating x0 / x0 + 1 (dx = +1, -1);
x0 in steps of 2 (nothing combines); x0 ascending and descending by 1; a row change after the second record; fractions that are exactly zero
(corners with weight 0); on the tile's last column and row (x0 = Wt - 1, y0 = Ht - 1 in the map's last tiles: corners outside the map); random.
Gradient components have mixed signs and magnitudes from 2^-16 to 1 of the list's largest.

Bounds.  The reference takes each footprint as the kernel does — the float32 weights (1 - wx) * (1 - wy), ..., the float32 product
weight * gradient — and adds the products exactly (math.fsum).  The kernel rounds every product to a multiple of 2^(e - 40), 2^(e - 1) <= m < 2^e for
the chunk's largest component m: at most m * 2^-40 per contribution, and a texel takes at most one corner of a record, so a list of N records with
largest component M is within N * 2^-40 * M; a texel on the seam of two tiles gets the sum of its lists' bounds.
The double maps of the two launch shapes are BIT-identical: every chunk's table is an exact integer sum, and the doubles the chunks add into the
map are multiples of one 2^(e - 40) whose partial sums stay below 2^53 such units (the lists below put the same largest component into every
chunk, so a map has one scale, and no texel takes 2^11 contributions of < 2^40 units each: asserted where the lists are built), so those
additions are exact in any order as well."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (name, Ht, Wt, capacity, record count per tile as the shader backward would have left it — it counts past the capacity)
CASES = [
    ("64x64", 64, 64, 4096, [2047, 2048, 2049, 5000]),
    ("70x45", 45, 70, 4096, [0, 1, 2049, 2047, 5000, 2048]),
    ("70x45_three_chunks", 45, 70, 6144, [4100, 0, 1, 3, 7000, 2050]),
]
PATTERNS = 9
BLOCK = 32


def _positions(pat, k, xlo, xhi, ylo, yhi, rng):
    """texel (x0, y0) and fractions of record k (its index in the list) under pattern `pat`"""
    tw, th = xhi - xlo + 1, yhi - ylo + 1
    g, j = k // 4, k % 4                          # the thread's group of four, the record in it
    wx, wy = float(rng.random()), float(rng.random())
    if pat == 0:                                  # four on one texel
        x, y = xlo + (5 * g) % tw, ylo + (3 * g) % th
    elif pat == 1:                                # alternating x0 / x0 + 1
        x, y = xlo + (7 * g) % max(tw - 1, 1) + (j & 1), ylo + g % th
    elif pat == 2:                                # steps of 2
        x, y = xlo + (2 * j + 9 * g) % tw, ylo + (g * 5) % th
    elif pat == 3:                                # ascending by 1
        x, y = xlo + (g + j) % tw, ylo + (g * 7) % th
    elif pat == 4:                                # descending by 1
        x, y = xlo + (g + 3 - j) % tw, ylo + (g * 11) % th
    elif pat == 5:                                # row change after the second record
        x, y = xlo + (3 * g) % max(tw - 1, 1) + (j & 1), ylo + (g + (j >> 1)) % th
    elif pat == 6:                                # zero fractions
        x, y = xlo + (g * 3 + (j >> 1)) % tw, ylo + g % th
        wx, wy = (0.0 if j & 1 else wx), (0.0 if (j >> 1) ^ (g & 1) else wy)
    elif pat == 7:                                # last column / last row of the tile (of the map, in its last tiles)
        x, y = (xhi, ylo + (g + j) % th) if g & 1 else (xlo + (g + (j >> 1)) % tw, yhi)
        if g % 3 == 0:
            x, y = xhi, yhi
    else:                                         # random
        x, y = xlo + int(rng.integers(tw)), ylo + int(rng.integers(th))
    return x, y, wx, wy


def _build(name, H, W, cap, counts):
    rng = np.random.default_rng(abs(hash((H, W, cap))) % (2 ** 31))
    nbx, nby = (W + 31) // 32, (H + 31) // 32
    nb = nbx * nby
    assert len(counts) == nb
    rec = np.zeros((nb, 9, cap), np.float32)
    cnt = np.zeros(nb * 16 + 16, np.int32)
    big = (np.float32(3.1e-3), np.float32(0.37))                 # largest component of every list, per map
    ref = np.zeros((2, H, W, 3))
    bound = np.zeros((2, H, W, 3))
    per_cell = {}
    n_texel = np.zeros((H, W), np.int64)
    for b in range(nb):
        n = min(counts[b], cap)
        cnt[16 * b] = counts[b]
        if n == 0:
            continue
        bx, by = b % nbx, b // nbx
        xlo, xhi, ylo, yhi = bx * 32, min(bx * 32 + 31, W - 1), by * 32, min(by * 32 + 31, H - 1)
        pos = [_positions((k // BLOCK) % PATTERNS, k, xlo, xhi, ylo, yhi, rng) for k in range(n)]
        x0 = np.array([p[0] for p in pos]); y0 = np.array([p[1] for p in pos])
        wx = np.array([p[2] for p in pos], np.float32); wy = np.array([p[3] for p in pos], np.float32)
        assert x0.min() >= xlo and x0.max() <= xhi and y0.min() >= ylo and y0.max() <= yhi
        grads = np.zeros((n, 6), np.float32)
        for m in range(2):
            mag = np.exp2(-16.0 * rng.random((n, 3))) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
            grads[:, 3 * m:3 * m + 3] = (mag * float(big[m])).astype(np.float32)
            for c0 in range(0, n, 2048):                         # every chunk holds the list's largest component: one scale per list
                grads[c0, 3 * m + (c0 // 2048) % 3] = big[m] * (-1.0 if (c0 // 2048) & 1 else 1.0)
        key = (x0 | (y0 << 16)).astype(np.int32).view(np.float32)
        rec[b, 0, :n], rec[b, 1, :n], rec[b, 2, :n] = key, wx, wy
        rec[b, 3:, :n] = grads.T
        rec[b, :, n:] = np.float32(1e30)                          # stale slots past the count are never read as records
        rec[b, 0, n:] = 0.0
        # ---- the same footprints in float32, added exactly
        one = np.float32(1.0)
        ax, ay = one - wx, one - wy
        cw = [ax * ay, wx * ay, ax * wy, wx * wy]
        for k in range(4):
            cx, cy = x0 + (k & 1), y0 + (k >> 1)
            on = (cx < W) & (cy < H) & (cw[k] != 0)
            np.add.at(n_texel, (cy[on], cx[on]), 1)
            for ch in range(6):
                prod = (grads[:, ch] * cw[k]).astype(np.float32)
                assert prod.dtype == np.float32
                for i in np.nonzero(on)[0]:
                    per_cell.setdefault((ch // 3, int(cy[i]), int(cx[i]), ch % 3), []).append(float(prod[i]))
        for m in range(2):
            M = float(np.abs(grads[:, 3 * m:3 * m + 3]).max())
            assert M == float(big[m])
            bound[m, ylo:min(yhi + 2, H), xlo:min(xhi + 2, W), :] += n * 2.0 ** -40 * M
    for (m, y, x, ch), vals in per_cell.items():
        ref[m, y, x, ch] = math.fsum(vals)
    assert n_texel.max() < 2 ** 11                                 # (exact double additions into the maps: see the module docstring)
    return {"name": name, "H": H, "W": W, "cap": cap, "nb": nb, "rec": torch.from_numpy(rec), "cnt": torch.from_numpy(cnt),
            "ref": torch.from_numpy(ref), "bound": torch.from_numpy(bound)}


_cache = {}


def _case(i):
    if i not in _cache:
        _cache[i] = _build(*CASES[i])
    return _cache[i]


def _reduce(c, hint, tex=True, nmap=True):
    from harp_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream
    assert L.harp_texel_bins(c["H"], c["W"]) == c["nb"]
    rec_d, cnt_d = c["rec"].to(DEV).contiguous(), c["cnt"].to(DEV)
    acc = torch.zeros(2, c["H"], c["W"], 3, dtype=torch.float64, device=DEV)
    _lib.check(L.harp_texel_reduce(p(rec_d), p(cnt_d), c["cap"], c["H"], c["W"], p(acc[0]) if tex else None, p(acc[1]) if nmap else None, hint, st()),
               "harp_texel_reduce")
    torch.cuda.synchronize()
    assert int(cnt_d.abs().max()) == 0, "the list counters come back zeroed"
    return acc.cpu()


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_both_launch_shapes_bit_identical_and_within_the_fixed_point_bound(i):
    c = _case(i)
    small, large = _reduce(c, 1), _reduce(c, 3_000_000)
    assert torch.equal(small, large), (c["name"], (small - large).abs().max().item())
    for tag, got in (("small", small), ("large", large)):
        err = (got - c["ref"]).abs()
        worst = (err / c["bound"].clamp_min(1e-300)).max().item()
        print(c["name"], tag, "largest error / bound %.3f, largest error %.3e" % (worst, err.max().item()))
        assert bool((err <= c["bound"]).all()), (c["name"], tag, worst)
        assert int((got != 0).sum()) > 0 and bool((got[c["bound"] == 0] == 0).all())


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
@pytest.mark.parametrize("hint", [1, 3_000_000], ids=["small", "large"])
def test_frozen_maps(i, hint):
    """acc_nmap = NULL / acc_tex = NULL: the other map's sums are those of the call with both, the frozen one is not touched"""
    c = _case(i)
    both = _reduce(c, hint)
    only_tex, only_nmap = _reduce(c, hint, nmap=False), _reduce(c, hint, tex=False)
    assert torch.equal(only_tex[0], both[0]) and int((only_tex[1] != 0).sum()) == 0
    assert torch.equal(only_nmap[1], both[1]) and int((only_nmap[0] != 0).sum()) == 0
