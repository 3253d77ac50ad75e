"""-m gpu: ops.sheet_u8 / harp_sheet_u8 (csrc/sheet.hip), the contact sheets of the in-fit monitor.  Modes 0, 1 and 2 are bit-equal to the
numpy float32 restatement of tests/_sheet_ref.py (same IEEE operations, same order: no tolerance); mode 3 (normalise) is compared with
its float64 evaluation, where a level may differ only next to an integer boundary."""
import ctypes

import numpy as np
import pytest
import torch

from tests._sheet_ref import F, normal_levels_f64, numpy_sheet

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = {0: "image", 1: "overlay", 2: "absdiff", 3: "normal"}
SIZES = [(4, 4), (7, 5), (33, 17), (64, 64)]
LAYOUTS = [(1, (3, 3)), (5, (3, 3)), (9, (3, 3)), (2, (1, 2))]


def operands(mode, N, H, W, rng, nan=True):
    """uniform in [-0.2, 1.2] with one NaN in `a`"""
    u = lambda *s: rng.uniform(-0.2, 1.2, size=s).astype(F)
    if mode == 1:
        a, b, m = u(N, H, W), u(N, H, W), None
    else:
        a, b, m = u(N, H, W, 3), (u(N, H, W, 3) if mode == 2 else None), (u(N, H, W) if mode == 2 else None)
    if nan:
        a.reshape(-1)[rng.integers(a.size)] = np.nan
    return a, b, m


def run(mode, a, b, m, grid, d, **kw):
    from harp_amd import ops
    t = lambda x: None if x is None else torch.from_numpy(x).to(DEV)
    return ops.sheet_u8(t(a), t(b), t(m), mode=MODES[mode], grid=grid, d=d, **kw)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_sheet_bit_equal_to_numpy(mode, H, W):
    rng = np.random.default_rng(100 * mode + H)
    for N, grid in LAYOUTS:
        for d in (1, 2, 3, 8):
            a, b, m = operands(mode, N, H, W, rng)
            want = numpy_sheet(mode, a, b, m, grid, d)
            ch, cw = -(-H // d), -(-W // d)
            assert want.shape == (grid[0] * ch, grid[1] * cw, 3)
            got = run(mode, a, b, m, grid, d)
            assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
            g = got.cpu().numpy()
            assert np.array_equal(g, want), (N, grid, d, int((g != want).sum()), np.argwhere(g != want)[:5])
            for k in range(N, grid[0] * grid[1]):                                     # empty cells: white
                r, c = divmod(k, grid[1])
                assert (g[r * ch:(r + 1) * ch, c * cw:(c + 1) * cw] == 255).all(), (N, grid, d, k)
            if d == 1:                                                                 # the NaN's pixel writes 0
                n, y, x = np.argwhere(np.isnan(a))[0][:3]
                r, c = divmod(int(n), grid[1])
                px = g[r * ch + y, c * cw + x]
                assert px[0 if mode == 1 else int(np.argwhere(np.isnan(a))[0][3])] == 0, px


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_level_boundaries(mode):
    """k / 255 and its two float32 neighbours for every k at d = 1: 768 values = one 16 x 16 x 3 frame (three 16 x 16 masks in mode 1)"""
    k = (np.arange(256, dtype=np.float64) / 255).astype(F)
    vals = np.concatenate([k, np.nextafter(k, F(2)), np.nextafter(k, F(-1))]).astype(F)
    rng = np.random.default_rng(5)
    if mode == 1:
        a, b, m = vals.reshape(3, 16, 16), rng.permutation(vals).reshape(3, 16, 16), None
    else:
        a = rng.permutation(vals).reshape(1, 16, 16, 3)
        b, m = (np.zeros_like(a), np.ones((1, 16, 16), F)) if mode == 2 else (None, None)
    want = numpy_sheet(mode, a, b, m, (2, 2), 1)
    assert len(np.unique(want[:16, :16])) >= 250                                 # the levels are all there
    assert np.array_equal(run(mode, a, b, m, (2, 2), 1).cpu().numpy(), want)


def test_inputs_are_read_in_place():
    """a channels-first tensor and view, a batch slice with a step, a 4-channel image of which three channels are read, (N,H,W,1) masks"""
    from harp_amd import ops
    rng = np.random.default_rng(9)
    N, H, W = 5, 33, 17
    a, b, m = operands(2, N, H, W, rng)
    for d in (1, 3):
        want0, want2 = numpy_sheet(0, a, grid=(3, 3), d=d), numpy_sheet(2, a, b, m, (3, 3), d)
        nchw = torch.from_numpy(a).permute(0, 3, 1, 2).contiguous().to(DEV)
        assert np.array_equal(ops.sheet_u8(nchw, d=d, channels_last=False).cpu().numpy(), want0)
        assert np.array_equal(ops.sheet_u8(nchw.permute(0, 2, 3, 1), d=d).cpu().numpy(), want0)
        big = torch.full((2 * N, H, W, 3), 7.0, device=DEV)
        big[::2] = torch.from_numpy(a).to(DEV)
        assert not big[::2].is_contiguous()
        assert np.array_equal(ops.sheet_u8(big[::2], d=d).cpu().numpy(), want0)
        rgba = torch.cat([torch.from_numpy(a), torch.full((N, H, W, 1), 7.0)], -1).to(DEV)
        assert np.array_equal(ops.sheet_u8(rgba, d=d).cpu().numpy(), want0)
        bb = torch.cat([torch.from_numpy(b), torch.full((N, H, W, 1), 7.0)], -1).to(DEV)
        got2 = ops.sheet_u8(rgba, bb[..., :3], torch.from_numpy(m).to(DEV)[..., None], mode="absdiff", d=d)
        assert np.array_equal(got2.cpu().numpy(), want2)
    ma, mb, _ = operands(1, N, H, W, rng)
    got1 = ops.sheet_u8(torch.from_numpy(ma).to(DEV)[..., None], torch.from_numpy(mb).to(DEV), mode="overlay", d=2)
    assert np.array_equal(got1.cpu().numpy(), numpy_sheet(1, ma, mb, grid=(3, 3), d=2))


def normal_map_case():
    rng = np.random.default_rng(11)
    a = rng.normal(size=(1, 37, 29, 3)).astype(F)
    a[0, 5, 7] = 0.0                                                                   # a zero texel: 0 / 1e-12 * 0.5 + 0.5 = level 127
    v = normal_levels_f64(a)
    frac = v - np.floor(v)
    return a, v, (frac >= 0.01) & (frac <= 0.99)


def test_normal_mode_against_float64():
    """float32 error is ~1e-4 level: never more than one level off, equal wherever the float64 value is not within 0.01 of an integer —
    and that set holds at least 90 % of the values, so the filter cannot hide a failure"""
    a, v, decided = normal_map_case()
    assert decided.mean() >= 0.9, decided.mean()
    got = run(3, a, None, None, (1, 1), 1).cpu().numpy().astype(np.int64)
    assert got.shape == (37, 29, 3)
    want = np.floor(v[0]).astype(np.int64)
    assert np.abs(got - want).max() <= 1, np.abs(got - want).max()
    assert np.array_equal(got[decided[0]], want[decided[0]]), int((got != want)[decided[0]].sum())
    assert tuple(got[5, 7]) == (127, 127, 127)


def test_sheet_refuses_bad_arguments():
    from harp_amd import _lib, ops
    L = _lib.lib()
    f = 1 << 20                                                                        # a fake device pointer, never dereferenced
    st4, st3 = (ctypes.c_longlong * 4)(48, 12, 3, 1), (ctypes.c_longlong * 3)(16, 4, 1)
    neg = (ctypes.c_longlong * 4)(48, -12, 3, 1)
    ok = dict(mode=0, a=f, sa=st4, b=None, sb=None, m=None, sm=None, N=1, H=4, W=4, rows=3, cols=3, d=1, out=f)
    two = dict(mode=1, b=f, sb=st4)
    three = dict(mode=2, b=f, sb=st4, m=f, sm=st3)
    bad = [dict(mode=-1), dict(mode=4), dict(a=None), dict(sa=None), dict(out=None), dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(H=-3),
           dict(rows=0), dict(cols=0), dict(cols=-1), dict(d=0), dict(d=9), dict(rows=5, cols=13), dict(N=10), dict(N=3, rows=1, cols=2),
           dict(sa=neg), dict(b=f, sb=st4), dict(mode=3, b=f, sb=st4), dict(m=f, sm=st3), dict(mode=1), dict(two, sb=None), dict(two, sb=neg),
           dict(two, m=f, sm=st3), dict(mode=2), dict(three, b=None, sb=None), dict(three, m=None, sm=None), dict(three, sm=None),
           dict(three, sm=(ctypes.c_longlong * 3)(16, -4, 1))]
    for case in bad:
        c = dict(ok, **case)
        rc = L.harp_sheet_u8(c["mode"], c["a"], c["sa"], c["b"], c["sb"], c["m"], c["sm"], c["N"], c["H"], c["W"], c["rows"], c["cols"], c["d"],
                             c["out"], None)
        assert rc == 1, case
    x = torch.zeros(1, 4, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sheet_u8(x)
    xd = x.to(DEV)
    for kw in (dict(mode="nope"), dict(mode="overlay"), dict(b=xd), dict(mode="absdiff", b=xd), dict(d=9), dict(grid=(9, 9)), dict(grid=(1, 1), d=0)):
        with pytest.raises(ValueError):
            ops.sheet_u8(xd, **kw)
    with pytest.raises(ValueError):
        ops.sheet_u8(torch.zeros(2, 4, 4, 3, device=DEV), grid=(1, 1))


def test_two_calls_give_identical_bytes():
    rng = np.random.default_rng(3)
    for mode in (0, 1, 2, 3):
        a, b, m = operands(mode, 9, 33, 17, rng, nan=False)
        first, second = run(mode, a, b, m, (3, 3), 2), run(mode, a, b, m, (3, 3), 2)
        assert torch.equal(first, second), mode
