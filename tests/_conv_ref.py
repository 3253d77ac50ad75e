"""float64 restatement of ONE launch of harp_conv3x3, written from the text of include/harp_hip.h (the comment above
`harp_conv3x3_args` and the field comments), not from csrc/conv.hip: the reference of tests/test_gpu_conv_paths.py, anchored on torch's
own convolution / ReLU / max pool / autograd and on the float64 torch module by tests/test_conv_ref_cpu.py.

`launch(a)` takes the struct's fields as a dict of CPU tensors / ints (key `in_` for `in`; `w` = the convolution's filters
(Cout, Cin, 3, 3) as `effective_filters` returns them, in place of the packed `filters`; outputs hold their PREFILL) and returns the
expected outputs with everything the header says is left alone still holding the prefill, the masks of the elements the launch writes,
and the ingredients of the error bounds: A_i = sum |x_eff| |w| + |b| per output element and K = 9 x (input channels that can be non-zero).

Where the header was silent and the kernel had to be read, the place is marked "(conv.hip)" below; the header now carries those
sentences.

Bounds (`bound`), per element of conv + bias, U = 2^-24; none is measured on the kernel:
  mode 0  (K + 2) U A                                   float32 fma chain of K terms (MI355X: the f32 MFMA is bitwise an fmaf chain), the
                                                        bias add and one spare rounding.
  mode 1  2^-16 A + (3K + 2) U A                        x = hi + lo + r with |r| <= 2^-18 |x| for both operands, the dropped lo.lo is another
                                                        2^-18 of the product: 3 x 2^-18 < 2^-16.  How many float32 roundings a 32x32x16 bf16
                                                        MFMA performs over its 16 products is not documented: the worst case is taken, one
                                                        rounding per product term, of which there are 3 per MAC.
  mode 2  (2^-10 + 2^-22) A + (K + 2) U A + floor       both operands rounded to 11 bits: (1 + 2^-11)^2 - 1; one product term per MAC (same
                                                        worst case); floor = 2^-25 (2^-e sum |w| + sum |x|): below f16's normal range the
                                                        staged input x 2^e and the filters keep an absolute error of half a subnormal step
                                                        2^-24 (sums over the taps that meet a non-zero partner).
ReLU and max are 1-Lipschitz: relu(conv + b) keeps the bound, a pooled value takes the largest of its window's four.  GATE multiplies by
0 / 1.  UNPOOL adds into `out`: one more rounding of the result's magnitude, U |out|."""
import math

import torch

RELU, RELU_TAP, GATE, UNPOOL = 0, 1, 2, 3
U = 2.0 ** -24

FIELDS = ("in_", "w", "bias", "out", "pooled", "target", "target_row", "g_tap", "loss", "gate", "N", "H", "W", "Cin", "Cout", "precision",
          "epilogue", "in_channels", "tap_scale", "tile_list", "tile_count", "max_tiles", "in_valid_shift", "in_valid", "in_alt", "out_valid",
          "tile_origin", "in_valid_origin", "out_valid_origin", "tile_pitch", "in_valid_pitch", "out_valid_pitch", "tile_side",
          "in_valid_cell", "out_valid_cell", "in_amax", "in_exp")


def args(**kw):
    """a zero-initialised harp_conv3x3_args as a dict"""
    a = {k: None for k in FIELDS}
    for k in ("N", "H", "W", "Cin", "Cout", "precision", "epilogue", "in_channels", "max_tiles", "in_valid_shift", "tile_pitch", "in_valid_pitch",
              "out_valid_pitch", "tile_side", "in_valid_cell", "out_valid_cell", "in_exp"):
        a[k] = 0
    a["tap_scale"] = 0.0
    bad = set(kw) - set(FIELDS)
    assert not bad, bad
    a.update(kw)
    return a


def effective_filters(w, transpose=False):
    """harp_conv3x3_pack_filters in words: a forward weight (Cout, Cin, 3, 3); transpose: the data-gradient filters — channels swap roles,
    taps are mirrored; channels zero-padded to the multiples of 64 (out) and 16 (in)"""
    w = w.double()
    if transpose:
        w = w.permute(1, 0, 2, 3).flip(2, 3)
    co, ci = w.shape[:2]
    out = torch.zeros((co + 63) // 64 * 64, (ci + 15) // 16 * 16, 3, 3, dtype=torch.float64)
    out[:co, :ci] = w
    return out


def f16_exponent(in_amax, in_exp):
    """e of HARP_CONV_F16: in_exp - floor(log2(*in_amax)) when in_amax is given, else in_exp; clamped to [-126, 126]"""
    e = int(in_exp)
    if in_amax is not None:
        v = abs(float(in_amax.reshape(-1)[0]))
        if v > 0 and math.isfinite(v):
            e -= math.frexp(v)[1] - 1
    return max(-126, min(126, e))


def conv_nhwc(x, w):
    """3x3 / pad 1 / stride 1 over NHWC in float64: nine shifted products (no library convolution: that is what it is anchored on)"""
    N, H, W, _ = x.shape
    xp = torch.zeros(N, H + 2, W + 2, x.shape[3], dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = torch.zeros(N, H, W, w.shape[0], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("nhwc,oc->nhwo", xp[:, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return out


def _rows(a):
    return [int(r) for r in a["target_row"]] if a["target_row"] is not None else list(range(a["N"]))


def effective_input(a):
    """x_eff (N,H,W,Cin) float64, src (N,H,W): 0 = `in`, 1 = `in_alt`, 2 = zero (no in_alt), and the per-pixel cell tables
    cell_y (N,H) / cell_x (N,W) (-1 without in_valid) with `beyond` (N,H,W): the pixel's cell lies at or beyond in_valid_pitch"""
    N, H, W, Cin = a["N"], a["H"], a["W"], a["Cin"]
    ic = a["in_channels"] or Cin
    rows = _rows(a)
    x = torch.zeros(N, H, W, Cin, dtype=torch.float64)
    src = torch.zeros(N, H, W, dtype=torch.long)
    cell_y, cell_x = torch.full((N, H), -1, dtype=torch.long), torch.full((N, W), -1, dtype=torch.long)
    beyond = torch.zeros(N, H, W, dtype=torch.bool)
    yy, xx = torch.arange(H), torch.arange(W)
    for n, r in enumerate(rows):
        valid = torch.ones(H, W, dtype=torch.bool)
        if a["in_valid"] is not None:
            shift = a["in_valid_shift"]
            cell = a["in_valid_cell"] or (8 << shift)
            # (conv.hip) the producer's origin is given in the PRODUCER's pixels; behind a pool (shift 0) those are twice as fine as this
            # convolution's input pixels, so the (even) origin halves
            poy, pox = ((int(v) >> (1 - shift)) for v in a["in_valid_origin"][r]) if a["in_valid_origin"] is not None else (0, 0)
            P = a["in_valid_pitch"]
            cy, cx = (yy + poy) // cell, (xx + pox) // cell
            cell_y[n], cell_x[n] = cy, cx
            # (conv.hip) cells at or beyond the bitmap's pitch are invalid
            inside = (cy < P)[:, None] & (cx < P)[None, :]
            bm = a["in_valid"][r].reshape(P, P) != 0
            valid = inside & bm[cy.clamp(max=P - 1)][:, cx.clamp(max=P - 1)]
            beyond[n] = ~inside
        alt = a["in_alt"][r].double() if a["in_alt"] is not None else torch.zeros(H, W, ic, dtype=torch.float64)
        x[n, :, :, :ic] = torch.where(valid[..., None], a["in_"][n].double(), alt)
        src[n] = torch.where(valid, 0, 1 if a["in_alt"] is not None else 2)
    return dict(x=x, src=src, cell_y=cell_y, cell_x=cell_x, beyond=beyond)


def owned_pixels(a):
    """owned (N,H,W) and the listed tiles [(n, y0, x0, side)] (unclipped)"""
    N, H, W = a["N"], a["H"], a["W"]
    owned = torch.zeros(N, H, W, dtype=torch.bool)
    tiles = []
    if a["tile_list"] is None:
        owned[:] = True
        return owned, tiles
    side = a["tile_side"] or 16
    for n, r in enumerate(_rows(a)):
        oy, ox = (int(v) for v in a["tile_origin"][r]) if a["tile_origin"] is not None else (0, 0)
        for i in range(int(a["tile_count"][r])):
            ty, tx = divmod(int(a["tile_list"][r, i]), a["tile_pitch"])
            y0, x0 = side * ty - oy, side * tx - ox
            tiles.append((n, y0, x0, side))
            owned[n, max(y0, 0):max(min(y0 + side, H), 0), max(x0, 0):max(min(x0 + side, W), 0)] = True
    return owned, tiles


def _windows(t, H, W):
    """(N,2H,2W,C) -> (N,H,W,4,C), the 2x2 windows in row-major order"""
    N, C = t.shape[0], t.shape[3]
    return t.reshape(N, H, 2, W, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, 4, C)


def _unwindows(t):
    N, H, W, _, C = t.shape
    return t.reshape(N, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, C)


def launch(a, with_bounds=True):
    N, H, W, Cin, Cout, epi = a["N"], a["H"], a["W"], a["Cin"], a["Cout"], a["epilogue"]
    rows = _rows(a)
    w = a["w"].double()
    assert tuple(w.shape) == (Cout, Cin, 3, 3)
    eff = effective_input(a)
    x = eff["x"]
    owned, tiles = owned_pixels(a)
    conv = conv_nhwc(x, w)
    has_bias = epi in (RELU, RELU_TAP) and a["bias"] is not None
    b = a["bias"].double() if has_bias else torch.zeros(Cout, dtype=torch.float64)
    res = dict(eff, owned=owned, tiles=tiles, conv=conv, pre=conv + b, rows=rows)
    if with_bounds:
        ic = a["in_channels"] or Cin
        live = (torch.arange(Cin) < ic) & (w.abs().amax((0, 2, 3)) > 0)
        res["K"] = 9 * int(live.sum())
        res["A"] = conv_nhwc(x.abs(), w.abs()) + b.abs()
        res["Sw"] = conv_nhwc((x != 0).double(), w.abs())           # sum |w| over the taps that meet a non-zero input
        res["Sx"] = conv_nhwc(x.abs(), (w != 0).double())           # sum |x| over the taps that meet a non-zero filter
    own4 = owned[..., None].expand(N, H, W, Cout)
    if epi in (RELU, RELU_TAP):
        v = res["pre"].clamp(min=0)
        res["act"] = v
        if a["out"] is not None:
            res["out"], res["out_written"] = torch.where(own4, v, a["out"].double()), own4
        if a["pooled"] is not None:
            assert H % 2 == 0 and W % 2 == 0
            # (conv.hip) a 2x2 pool window belongs to the tile of its pixels: origins are even, so the four agree
            o4 = _windows(owned[..., None], H // 2, W // 2)[..., 0]
            assert (o4.all(-1) == o4.any(-1)).all()
            pown = o4[..., 0][..., None].expand(N, H // 2, W // 2, Cout)
            res["pooled"], res["pooled_written"] = torch.where(pown, _windows(v, H // 2, W // 2).amax(3), a["pooled"].double()), pown
        if epi == RELU_TAP:
            d = v - a["target"][rows].double()
            s = float(a["tap_scale"])
            g = torch.where(v > 0, s * torch.sign(d), torch.zeros((), dtype=torch.float64))
            res["d"], res["tap_scale"] = d, s
            res["g_tap"], res["g_tap_written"] = torch.where(own4, g, a["g_tap"].double()), own4
            # only the owned pixels' share
            res["loss"] = float(a["loss"].double()) + s * float((d.abs() * own4).sum())
            res["loss_abs"] = s * float((d.abs() * own4).sum())
    elif epi == GATE:
        g = conv * (a["gate"].double() > 0)
        res["out"], res["out_written"] = torch.where(own4, g, a["out"].double()), own4
    else:
        gate = _windows(a["gate"].double(), H, W)                   # (N,H,W,4,C)
        best, idx = gate[:, :, :, 0], torch.zeros(N, H, W, Cout, dtype=torch.long)
        for k in range(1, 4):                                       # the FIRST maximum in row-major order: a later one must be larger
            better = gate[:, :, :, k] > best
            best, idx = torch.where(better, gate[:, :, :, k], best), torch.where(better, k, idx)
        keep = owned.clone()
        skipped = torch.zeros(N, H, W, dtype=torch.bool)
        if a["out_valid"] is not None:
            cell = a["out_valid_cell"] or 16
            P = a["out_valid_pitch"]
            for n, r in enumerate(rows):
                oy, ox = (int(v) for v in a["out_valid_origin"][r]) if a["out_valid_origin"] is not None else (0, 0)
                cy, cx = (2 * torch.arange(H) + oy) // cell, (2 * torch.arange(W) + ox) // cell
                # (conv.hip) the bitmap must cover `out`: the kernel does not look at out_valid_pitch before it indexes
                assert int(cy.max()) < P and int(cx.max()) < P, "out_valid does not cover `out`"
                ok = a["out_valid"][r].reshape(P, P)[cy][:, cx] != 0
                skipped[n] = owned[n] & ~ok
                keep[n] &= ok
        route = keep[..., None] & (best > 0)
        onehot = torch.zeros(N, H, W, 4, Cout, dtype=torch.bool).scatter_(3, idx[:, :, :, None], route[:, :, :, None])
        written = _unwindows(onehot)
        add = _unwindows(onehot * conv[:, :, :, None])
        res.update(out=a["out"].double() + add, out_written=written, skipped=skipped, best=best, idx=idx, gate_w=gate)
    return res


def bound(res, precision, e=0):
    """bound_i of conv + bias (N,H,W,Cout), see the module docstring"""
    A, K = res["A"], res["K"]
    if precision == 0:
        return (K + 2) * U * A
    if precision == 1:
        return 2.0 ** -16 * A + (3 * K + 2) * U * A
    return (2.0 ** -10 + 2.0 ** -22) * A + (K + 2) * U * A + 2.0 ** -25 * (2.0 ** -e * res["Sw"] + res["Sx"])


def pooled_bound(bd):
    N, H, W, _ = bd.shape
    return _windows(bd, H // 2, W // 2).amax(3)


def unpool_bound(res, bd):
    """per element of `out` (N,2H,2W,Cout): the routed convolution value's bound plus one rounding of the sum"""
    N, H, W, C = bd.shape
    return _unwindows(bd[:, :, :, None].expand(N, H, W, 4, C)) + U * res["out"].abs()


def tap_undecided(res, bd):
    """elements whose tap gradient the reference does not decide: |conv + b| <= bound or |out - target| <= bound"""
    return (res["pre"].abs() <= bd) | (res["d"].abs() <= bd)


def loss_bound(res, bd, n_sum=16 * 16 * 64):
    """*loss: every |out - target| carries bound_i and the subtraction's rounding; the terms of one workgroup (at most a 16 x 16 x 64 tile)
    are summed in float32 in an order the header does not fix: worst case (n - 1) U of the sum; the double accumulator adds 2^-53"""
    own = res["g_tap_written"]
    s = res["loss_abs"]
    return float(abs(res["tap_scale"]) * (bd * own).sum()) + (n_sum + 1) * U * s + 2.0 ** -50 * abs(res["loss"])
