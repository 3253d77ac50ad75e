"""One small harp_conv3x3 launch per path of csrc/conv.hip (include/harp_hip.h, `harp_conv3x3_args`): the smallest synthetic arguments that reach
it, each with the conditions (`expect`) that `reach()` derives from the ARGUMENTS and the float64 restatement alone (tests/_conv_ref.py) —
tests/test_conv_ref_cpu.py asserts them for every case, tests/test_gpu_conv_paths.py runs the cases on the kernel.

Every case: H, W <= 40, Cin 16 or 32 (32: two staged chunks, the second one's prefetch), Cout 64 or 128 (128: two channel blocks in the block
id), N = 2 - 3 images over T = 4 frame rows with a target_row that is neither the identity nor free of duplicates.  Tile origins are even and
non-negative, every listed tile index lies inside its grid, every bitmap has pitch^2 entries and out_valid covers `out`: `build` asserts it
(the kernel does not check them)."""
import math
import zlib

import torch

from tests import _conv_ref as R

T = 4
ROWS_A, ROWS_B = [2, 0, 2], [1, 2, 1]
TAP_SCALE, LOSS0 = 0.375, 0.75            # (exact in float32)

# ---- tile grids ------------------------------------------------------------------------------------------------------------------------------
# 16-pixel tiles over 40 x 24 (pitch ceil(40 / 16) + 1 = 4): frame 0 empty, frame 1 below max_tiles, frame 2 full, in an order that is not
# the raster's; frame 2's origin (14, 6): tile (0, 0) starts at (-14, -6), (3, .) ends at 50 > H, (., 1) at 26 > W
TL16 = dict(side=16, pitch=4, origins=[(4, 12), (2, 10), (14, 6), (0, 0)], pad=(2, 0),
            lists=[[], [(1, 0), (3, 1)], [(0, 0), (1, 1), (3, 0), (2, 1), (3, 1)], [(2, 0)]])
# 16-pixel tiles over 40 x 40: frame 2's tile (1, 1) = pixels [2, 18) x [10, 26), its patch [1, 18] x [9, 26] wholly inside the image
TL16V = dict(side=16, pitch=4, origins=[(4, 12), (2, 10), (14, 6), (0, 0)], pad=(2, 2),
             lists=[[(1, 2), (2, 1)], [(0, 0)], [(1, 1), (0, 0), (2, 2), (3, 1)], []])
# 8-pixel tiles over 24 x 20 (pitch ceil(24 / 8) + 1 = 4), 1, 2, 3 and 5 tiles: max_tiles 5 = two groups of four; origin (6, 2): tile (0, 0)
# starts at (-6, -2), (3, .) ends at 26 > H, (., 2) at 22 > W
TL8 = dict(side=8, pitch=4, origins=[(2, 6), (6, 2), (6, 2), (4, 2)], pad=(1, 1),
           lists=[[(2, 1)], [(0, 0), (3, 2)], [(0, 0), (1, 1), (3, 2)], [(1, 1), (0, 0), (3, 2), (2, 0), (1, 2)], ])
# ... and 4, 0, 2 tiles with max_tiles 4: one full group
TL8C = dict(side=8, pitch=4, origins=[(6, 2), (0, 0), (2, 4), (0, 0)], pad=(1, 1),
            lists=[[(1, 1), (0, 0), (3, 2), (2, 1)], [], [(1, 0), (2, 2)], []])
# 8-pixel tiles over a 12 x 20 map (the un-pool convolution's own resolution)
TL8U = dict(side=8, pitch=4, origins=[(2, 6), (0, 0), (6, 2), (0, 0)], pad=(1, 1),
            lists=[[(1, 1), (0, 1)], [], [(0, 0), (1, 1), (2, 2), (1, 3), (2, 0)], []])


def V(shift, cell, pitch, alt, origins=((6, 4), (2, 10), (12, 12), (0, 0)), p=0.65):
    return dict(shift=shift, cell=cell, pitch=pitch, alt=alt, origins=list(origins), p=p)


def case(H, W, Cin=16, Cout=64, N=2, rows=None, epi=R.RELU, ic=0, bias=True, out=True, pooled=False, src=None, tiles=None, valid=None,
         out_valid=None, f16=(True, 14), expect=()):
    return dict(H=H, W=W, Cin=Cin, Cout=Cout, N=N, rows=rows, epi=epi, ic=ic, bias=bias, out=out, pooled=pooled, src=src, tiles=tiles,
                valid=valid, out_valid=out_valid, f16=f16, expect=tuple(expect))


TILE_EDGES = ("y0_neg", "x0_neg", "past_H", "past_W", "rows_mixed")
CASES = {
    # ---- full grid
    "full_1x1": case(1, 1, expect=("odd",)),
    "full_2x2": case(2, 2, pooled=True),
    "full_5x5": case(5, 5, f16=(False, 3), expect=("odd",)),
    "full_9x9_tap": case(9, 9, 32, 128, N=3, rows=ROWS_A, epi=R.RELU_TAP, expect=("odd", "two_blocks", "rows_mixed")),
    "full_16x16_pooled_only": case(16, 16, 32, out=False, pooled=True),
    "full_17x17": case(17, 17, 32, 128, expect=("odd", "second_tile_1px", "two_blocks")),
    "full_23x37_nobias": case(23, 37, 32, bias=False, expect=("odd",)),
    "full_40x24_tap": case(40, 24, 32, 128, N=3, rows=ROWS_A, epi=R.RELU_TAP, pooled=True, expect=("two_blocks", "rows_mixed")),
    "full_ic4": case(8, 12, 16, ic=4, pooled=True, expect=("partial_chunk",)),
    "full_ic20": case(17, 9, 32, ic=20, expect=("partial_chunk", "odd")),
    "full_t3_relu": case(12, 20, 32, 64, src=(32, 3, True), expect=("padded_out",)),
    "full_t3_gate": case(7, 18, 32, 64, epi=R.GATE, src=(32, 3, True), expect=("padded_out", "odd")),
    "gate_12x20": case(12, 20, 32, 128, epi=R.GATE, expect=("two_blocks", "gate_zeros")),
    # ---- un-pool, every tile
    "unpool_full": case(8, 12, 32, 64, epi=R.UNPOOL, expect=("ties", "zero_windows")),
    "unpool_odd": case(5, 7, 16, 128, epi=R.UNPOOL, expect=("ties", "zero_windows", "odd", "two_blocks")),
    # ---- 16-pixel tile lists
    "tl16_tap": case(40, 24, 32, 128, N=3, rows=ROWS_A, epi=R.RELU_TAP, pooled=True, tiles=TL16,
                     expect=TILE_EDGES + ("count_zero", "count_full", "unowned", "two_blocks")),
    "tl16_relu": case(40, 24, 32, 64, N=3, rows=ROWS_B, tiles=TL16, expect=TILE_EDGES + ("count_partial", "count_full", "unowned")),
    # ---- validity bitmaps under 16-pixel tiles: the same-resolution producer (shift 1) on 16- and 8-pixel tiles, the producer behind a
    #      pool (shift 0) on 16-pixel tiles (cells of 8); 18-pixel patches span two cells of 16 (three only
    #      when the two origins agree), four of 8
    "v16_same16": case(40, 40, 32, 64, N=3, rows=ROWS_A, tiles=TL16V, valid=V(1, 0, 2, True),
                       expect=("mix", "beyond_pitch", "two_cells", "origins_differ", "alt")),
    "v16_same8": case(40, 40, 32, 64, N=3, rows=ROWS_A, tiles=TL16V, valid=V(1, 8, 5, True, origins=((6, 4), (2, 10), (6, 6), (0, 0))),
                      expect=("mix", "beyond_pitch", "four_cells", "origins_differ", "alt")),
    "v16_pool8": case(40, 40, 32, 128, N=3, rows=ROWS_A, tiles=TL16V, valid=V(0, 0, 5, False),
                      expect=("mix", "beyond_pitch", "four_cells", "origins_differ", "no_alt", "two_blocks")),
    # ---- 8-pixel tiles, 1 / 2 / 3 / 4 / 5 per frame; validity cells of 4 (behind a pool) and 8
    "t8_relu_pool4": case(24, 20, 32, 128, N=3, rows=ROWS_A, pooled=True, tiles=TL8, valid=V(0, 4, 6, True, origins=((4, 4), (2, 10), (4, 12), (0, 0))),
                          expect=TILE_EDGES + ("partial_group", "wg_returns", "mix", "beyond_pitch", "four_cells", "alt", "unowned")),
    "t8_tap_same8": case(24, 20, 32, 128, N=3, rows=[1, 3, 1], epi=R.RELU_TAP, tiles=TL8, valid=V(1, 8, 3, True, origins=((4, 4), (2, 2), (4, 12), (6, 0))),
                         expect=TILE_EDGES + ("partial_group", "wg_returns", "second_group", "mix", "beyond_pitch", "alt", "unowned")),
    "t8_gate_same8": case(24, 20, 32, 64, N=3, rows=[0, 0, 2], epi=R.GATE, tiles=TL8C, valid=V(1, 8, 4, False, origins=((2, 6), (0, 0), (2, 4), (0, 0))),
                          expect=("rows_mixed", "full_group", "partial_group", "mix", "no_alt", "unowned")),
    # ---- un-pool in bounded mode: windows outside `out`'s valid tiles are skipped
    "unpool_ov16": case(12, 20, 32, 64, N=3, rows=ROWS_A, epi=R.UNPOOL, tiles=TL8U, valid=V(1, 8, 4, False, origins=((2, 6), (0, 0), (6, 2), (0, 0))),
                        out_valid=dict(cell=16, pitch=4, origins=[(6, 10), (0, 0), (10, 4), (0, 0)], p=0.5),
                        expect=("window_skipped", "window_kept", "ties", "zero_windows", "unowned", "rows_mixed")),
    "unpool_ov8": case(9, 7, 16, 64, N=3, rows=ROWS_A, epi=R.UNPOOL, out_valid=dict(cell=8, pitch=3, origins=[(2, 6), (0, 0), (6, 2), (0, 0)], p=0.5),
                       expect=("window_skipped", "window_kept", "ties", "zero_windows", "odd", "rows_mixed")),
}


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


def build(name):
    """the arguments of case `name`: c["a"] = the struct's fields for tests/_conv_ref.py (outputs = their prefill), c["w_src"] /
    c["transpose"] = what harp_conv3x3_pack_filters is given"""
    s = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    H, W, Cin, Cout, N, epi = s["H"], s["W"], s["Cin"], s["Cout"], s["N"], s["epi"]
    ic = s["ic"] or Cin
    rn = lambda *shape: torch.randn(*shape, generator=g)
    tap = epi == R.RELU_TAP
    # tap cases: non-negative inputs (activations behind a ReLU) and filters with a per-channel offset, so that conv + b is rarely within the
    # arithmetic's error of zero — what the tap's gradient [out > 0] needs to be decided by the reference alone
    x = rn(N, H, W, ic).abs() if tap else rn(N, H, W, ic)
    if s["src"]:
        co_s, ci_s, transpose = s["src"]
        w_src = rn(co_s, ci_s, 3, 3) * (2.0 / (9 * ci_s)) ** 0.5
    else:
        transpose = False
        w_src = rn(Cout, Cin, 3, 3) * (2.0 / (9 * Cin)) ** 0.5
        if tap:
            w_src = w_src + (2.0 / (9 * Cin)) ** 0.5 * torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0)[:, None, None, None]
    w = R.effective_filters(w_src, transpose)
    assert tuple(w.shape) == (Cout, Cin, 3, 3), (name, w.shape)
    a = R.args(in_=x, w=w, N=N, H=H, W=W, Cin=Cin, Cout=Cout, epilogue=epi, in_channels=s["ic"])
    if s["bias"] and epi in (R.RELU, R.RELU_TAP):
        a["bias"] = rn(Cout) * 0.1
    if s["rows"] is not None:
        a["target_row"] = _i32(s["rows"])
    sent = lambda *shape: rn(*shape) * 3.0 + 0.125                                           # finite random sentinels
    if epi == R.UNPOOL:
        a["out"] = sent(N, 2 * H, 2 * W, Cout)                                              # (the tap's own gradient on entry)
        a["gate"] = ((rn(N, 2 * H, 2 * W, Cout) * 2).round() / 2).clamp(min=0)              # exact ties, exact zeros
    else:
        if s["out"] or epi == R.GATE:
            a["out"] = sent(N, H, W, Cout)
        if s["pooled"]:
            a["pooled"] = sent(N, H // 2, W // 2, Cout)
        if epi == R.GATE:
            a["gate"] = rn(N, H, W, Cout).clamp(min=0)
    if tap:
        a["target"] = rn(T, H, W, Cout).abs() + 0.05                                        # independent of the output, never 0
        a["g_tap"], a["loss"], a["tap_scale"] = sent(N, H, W, Cout), torch.tensor(LOSS0, dtype=torch.float64), TAP_SCALE
    tl = s["tiles"]
    if tl:
        side, P = tl["side"], tl["pitch"]
        assert P == max(math.ceil(H / side), math.ceil(W / side)) + 1
        mx = max(len(l) for l in tl["lists"])
        lst = torch.full((T, mx), tl["pad"][0] * P + tl["pad"][1], dtype=torch.int32)       # slots past tile_count hold a real tile's index
        for r, l in enumerate(tl["lists"]):
            assert len(set(l)) == len(l) and all(0 <= ty < P and 0 <= tx < P for ty, tx in l)
            for i, (ty, tx) in enumerate(l):
                lst[r, i] = ty * P + tx
        assert all(oy % 2 == 0 and ox % 2 == 0 and 0 <= oy < side and 0 <= ox < side for oy, ox in tl["origins"])
        a.update(tile_list=lst, tile_count=_i32([len(l) for l in tl["lists"]]), max_tiles=mx, tile_origin=_i32(tl["origins"]), tile_pitch=P,
                 tile_side=side)
    v = s["valid"]
    if v:
        P = v["pitch"]
        assert all(oy % 2 == 0 and ox % 2 == 0 and oy >= 0 and ox >= 0 for oy, ox in v["origins"])
        a.update(in_valid=(torch.rand(T, P * P, generator=g) < v["p"]).int(), in_valid_shift=v["shift"], in_valid_cell=v["cell"],
                 in_valid_pitch=P, in_valid_origin=_i32(v["origins"]))
        if v["alt"]:
            a["in_alt"] = rn(T, H, W, ic).abs() if tap else rn(T, H, W, ic)
    ov = s["out_valid"]
    if ov:
        P, cell = ov["pitch"], ov["cell"]
        for oy, ox in ov["origins"]:
            assert oy % 2 == 0 and ox % 2 == 0 and oy >= 0 and ox >= 0 and (2 * H - 1 + oy) // cell < P and (2 * W - 1 + ox) // cell < P
        a.update(out_valid=(torch.rand(T, P * P, generator=g) < ov["p"]).int(), out_valid_cell=cell, out_valid_pitch=P,
                 out_valid_origin=_i32(ov["origins"]))
    amax = None
    if s["f16"][0]:
        amax = x.abs().max()
        if a["in_alt"] is not None:
            amax = torch.maximum(amax, a["in_alt"].abs().max())
        amax = amax.reshape(1)
    return dict(name=name, spec=s, a=a, w_src=w_src, transpose=transpose, in_amax=amax, in_exp=s["f16"][1])


def reach(c, res):
    """what the case reaches, from its arguments and the restatement's tables (no kernel involved)"""
    a, s = c["a"], c["spec"]
    H, W, N = a["H"], a["W"], a["N"]
    rows = res["rows"]
    f = {}
    f["odd"] = bool(H % 2 or W % 2)
    f["two_blocks"] = a["Cout"] == 128
    f["second_tile_1px"] = H % 16 == 1 and W % 16 == 1
    f["partial_chunk"] = (a["in_channels"] or a["Cin"]) % 16 != 0
    f["rows_mixed"] = a["target_row"] is not None and rows != list(range(N)) and len(set(rows)) < N
    f["padded_out"] = bool(s["src"]) and s["src"][1] < a["Cout"]
    f["gate_zeros"] = a["gate"] is not None and bool((a["gate"] == 0).any()) and bool((a["gate"] > 0).any())
    tiles = res["tiles"]
    f["y0_neg"] = any(y0 < 0 for _, y0, _, _ in tiles)
    f["x0_neg"] = any(x0 < 0 for _, _, x0, _ in tiles)
    f["past_H"] = any(y0 + sd > H for _, y0, _, sd in tiles)
    f["past_W"] = any(x0 + sd > W for _, _, x0, sd in tiles)
    f["unowned"] = not bool(res["owned"].all())
    if a["tile_list"] is not None:
        cnt, mx = [int(a["tile_count"][r]) for r in rows], a["max_tiles"]
        f["count_zero"], f["count_full"] = 0 in cnt, mx in cnt
        f["count_partial"] = any(0 < n < mx for n in cnt)
        if a["tile_side"] == 8:                       # four tiles of the list per workgroup, one per wave
            groups = (mx + 3) // 4
            f["partial_group"] = any(n % 4 for n in cnt)                                   # a wave without a tile
            f["full_group"] = any(n and n % 4 == 0 for n in cnt)
            f["wg_returns"] = any(4 * (groups - 1) >= n for n in cnt) and groups > 1       # a whole workgroup with nothing to do
            f["second_group"] = any(n > 4 for n in cnt)
    if a["in_valid"] is not None:
        f["alt"], f["no_alt"] = a["in_alt"] is not None, a["in_alt"] is None
        f["origins_differ"] = a["tile_origin"] is not None and any(a["tile_origin"][r].tolist() != a["in_valid_origin"][r].tolist() for r in rows)
        mix = beyond = False
        most = 0
        for n, y0, x0, sd in tiles:                   # the tile's patch: one pixel of halo, clipped to the image
            ys, xs = slice(max(y0 - 1, 0), max(min(y0 + sd + 1, H), 0)), slice(max(x0 - 1, 0), max(min(x0 + sd + 1, W), 0))
            src = res["src"][n, ys, xs]
            if src.numel() == 0:
                continue
            mix |= bool((src == 0).any() and (src != 0).any())
            beyond |= bool(res["beyond"][n, ys, xs].any())
            most = max(most, min(len(set(res["cell_y"][n, ys].tolist())), len(set(res["cell_x"][n, xs].tolist()))))
        f["mix"], f["beyond_pitch"], f["two_cells"], f["four_cells"] = mix, beyond, most >= 2, most >= 4
    if a["epilogue"] == R.UNPOOL:
        own = res["owned"]
        f["window_skipped"] = bool(res["skipped"].any())
        f["window_kept"] = bool((own & ~res["skipped"]).any())
        g, best = res["gate_w"], res["best"]
        sel = (own & ~res["skipped"])[..., None]
        f["ties"] = bool((((g == best[:, :, :, None]).sum(3) > 1) & (best > 0) & sel).any())
        f["zero_windows"] = bool(((best == 0) & sel).any())
    return f


def check(c, res):
    f = reach(c, res)
    missing = [k for k in c["spec"]["expect"] if not f.get(k)]
    assert not missing, (c["name"], "does not reach", missing)
    # f16 mode: the staged input stays below the saturation threshold (the bound has no term for it)
    e = R.f16_exponent(c["in_amax"], c["in_exp"])
    assert float(res["x"].abs().max()) * 2.0 ** e <= 65504.0, c["name"]
    return f


# ---- refusals: every rule of harp_conv3x3's argument check, as changes to a valid launch whose tile lists are all empty ------------------
REFUSALS = [
    ("in NULL", dict(in_=None)), ("filters NULL", dict(filters=None)), ("N 0", dict(N=0)), ("H 0", dict(H=0)), ("W -1", dict(W=-1)),
    ("Cin 0", dict(Cin=0)), ("Cout 0", dict(Cout=0)), ("Cin 24", dict(Cin=24)), ("Cout 96", dict(Cout=96)),
    ("H W Cin past 2^31", dict(H=16384, W=16384)), ("in_channels -4", dict(in_channels=-4)), ("in_channels 20 > Cin", dict(in_channels=20)),
    ("in_channels 6", dict(in_channels=6)), ("RELU without out and pooled", dict(out=None, pooled=None)),
    ("TAP without target", dict(epilogue=R.RELU_TAP, target=None)), ("TAP without g_tap", dict(epilogue=R.RELU_TAP, g_tap=None)),
    ("TAP without loss", dict(epilogue=R.RELU_TAP, loss=None)), ("GATE without out", dict(epilogue=R.GATE, out=None)),
    ("GATE without gate", dict(epilogue=R.GATE, gate=None)), ("UNPOOL without gate", dict(epilogue=R.UNPOOL, gate=None)),
    ("UNPOOL without out", dict(epilogue=R.UNPOOL, out=None)), ("epilogue 4", dict(epilogue=4)), ("epilogue -1", dict(epilogue=-1)),
    ("pooled with odd H", dict(H=7)), ("pooled with odd W", dict(W=7)), ("tile_list without tile_count", dict(tile_count=None)),
    ("max_tiles 0", dict(max_tiles=0)), ("tile_pitch 0", dict(tile_pitch=0)), ("in_valid_pitch 0", dict(in_valid_pitch=0)),
    ("out_valid_pitch 0", dict(out_valid_pitch=0)), ("in_valid_shift 2", dict(in_valid_shift=2)), ("in_valid_shift -1", dict(in_valid_shift=-1)),
    ("tile_side 4", dict(tile_side=4)), ("tile_side 8 without tile_list", dict(tile_side=8, tile_list=None)),
    ("in_valid_cell 2", dict(in_valid_cell=2)), ("in_valid_cell 4 with 16-pixel tiles", dict(in_valid_cell=4)),
    ("out_valid_cell 4", dict(out_valid_cell=4)), ("precision 3", dict(precision=3)), ("precision -1", dict(precision=-1)),
]
