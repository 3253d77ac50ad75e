"""The light-view depth map's backward (csrc/shade.hip: depth_bwd_kernel) through each of its five entry points — harp_depth_bwd,
harp_depth_bwd_consume, harp_depth_bwd_tiles, harp_depth_nmap_bwd, harp_depth_bwd_riders: the forms a fitting step launches — against float64,
at the edges of the kernel: a full LDS vertex table (probe exhaustion -> memory atomics beside the table flush), a whole tile on one face (the
lane merge over every xor distance), a fan (one key from every lane), a ragged tile row / column, cotangents spanning 1e5 inside a tile,
an empty frame (slots past `nact`), and a grid beyond the 4096-workgroup cap (the tile loop wraps, as does the vertex-gradient rider's).
Synthetic one-layer NDC meshes (tests/_depth_cases.py, anchored on the oracle by tests/test_depth_cases_cpu.py); every case asserts from the
rasteriser's face ids that it reaches its edge.  Per element of g_ndc

    |got_i - ref64_i| <= 2^-22 * A_i + 4 * E32 + 2 * 2^-24 * |G0_i|

A_i the sum of the magnitudes of the per-pixel contributions (float32 lane merge, flush and memory atomics; the table itself sums in double, so
there is no per-add quantum), E32 = |ref32 - ref64|_inf of the reference evaluated in float32 on the CPU (never measured on the kernel; 4 x for
the kernel's approximate reciprocals, the convention of tests/test_gpu_shade_tables.py), G0 the random pre-fill every output accumulates onto.
The cotangent is zero on pixels the reference flags as undecided at float32 precision; the face ids agree on every other pixel; nothing is
masked out of the outputs.  Measured err / bound per case and form, and the mutations these cases catch: docs/NOTEBOOK.md B.19."""
import pytest
import torch
import torch.nn.functional as F

from tests import _depth_cases as D
from tests import _raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
N_TEXELS = D.RIDER_CAP + 257          # one past what the normal-map rider's 1024 workgroups cover in one pass, and off the 256 grid


def _L():
    from harp_amd import _lib
    return _lib.lib(), _lib.ptr


def _st():
    from harp_amd import _lib
    return _lib.stream()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _launch_order(ws, B, Fn, S):
    """(nact, order) of a rasteriser workspace: csrc/harp_common.h raster_ws_split — records | boxes | bins | counts | order | nact | ..."""
    from harp_amd import ops
    nst = ((S + 63) // 64) ** 2
    r256 = (B * nst * 4 + 255) // 256 * 256
    off = B * Fn * 64 + B * Fn * 16 + B * nst * Fn * 4 + r256
    order = ws[off:off + B * nst * 4].view(torch.int32).cpu().long()
    nact = int(ws[off + r256:off + r256 + 4].view(torch.int32)[0])
    assert nact == ops.rasterize_ws_nact(ws, B, Fn, S)
    return nact, order


# ----------------------------------------------------------------------------------------------------------------------
# cases: built once per module, shared by the forms, never modified
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    built = {}
    yield built
    built.clear()


def device_case(_cases, name):
    if name in _cases:
        return _cases[name]
    from harp_amd import ops
    c = D.build(name)
    B, S, V, Fn = c["B"], c["S"], c["ndc"].shape[1], c["faces"].shape[0]
    ras = D.raster(c)
    cot = D.cotangent(c, ras)
    faces = c["faces"].int().contiguous().to(DEV)
    face_id, _, _, ws = ops.rasterize_fwd(c["ndc"].to(DEV), faces, S, soft=False)
    torch.cuda.synchronize()
    fid = face_id.cpu().long()
    und = ras["undecided"]
    assert torch.equal(fid[~und], ras["face_id"][~und]), "K = 1 face ids differ away from the undecided pixels"
    nact, order = _launch_order(ws, B, Fn, S)
    info = D.conditions(c, fid, cot, und, nact, order)
    g = torch.Generator().manual_seed(B * 1000 + V)
    nt = (S + 15) // 16
    holds = D.tiles_of(cot != 0).any(-1)                                 # (B,nt,nt): tiles that hold a cotangent
    bb, ty, tx = torch.meshgrid(torch.arange(B), torch.arange(nt), torch.arange(nt), indexing="ij")
    half = holds & ((bb + ty + tx) % 2 == 0)
    assert half.any() and (holds & ~half).any()
    in_half = R.per_pixel(half, 16, S)
    cot_half = torch.where(in_half, cot, torch.zeros_like(cot))
    # (the reference's own face ids: the rasteriser's are the same wherever the cotangent is non-zero)
    c.update(V=V, Fn=Fn, d_faces=faces, d_face_id=face_id, d_ws=ws, fid=fid, cot=cot, ref=D.reference(c, ras["face_id"], cot),
             ref_half=D.reference(c, ras["face_id"], cot_half), cot_half=cot_half, in_half=in_half, holds=holds, half=half, info=info,
             G0=torch.randn(B, V, 3, generator=g),
             cot_everywhere=torch.where((fid < 0) & (ras["face_id"] < 0) & ~und, c["cot0"], cot))
    _cases[name] = c
    return c


def head(c, gz, g_ndc):
    L, p = _L()
    return (p(c["d_face_id"]), p(c["d_ws"]), p(c["d_faces"]), p(gz), c["B"], c["V"], c["Fn"], c["S"], p(g_ndc))


def check(c, g_ndc, tag, ref=None):
    """max over the elements of err / (2^-22 A + 4 E32 + 2 * 2^-24 |G0|), printed and asserted <= 1"""
    r = ref or c["ref"]
    G0 = c["G0"].double()
    err = (g_ndc.cpu().double() - G0 - r["ref"]).abs()
    bound = 2.0 ** -22 * r["A"] + 4.0 * r["E32"] + 2.0 * U * G0.abs()
    assert r["ref"].abs().max() > 0 and torch.isfinite(err).all()
    worst = (err / bound).max().item()
    print(f"[{c['name']} {tag}] err / bound {worst:.3f} (worst err {err.max().item():.2e}, E32 {r['E32']:.2e})")
    assert worst <= 1.0, (c["name"], tag, worst)
    return worst


def fresh(c, cot=None):
    """the cotangent image and the pre-filled output on the device"""
    return (c["cot"] if cot is None else cot).to(DEV).contiguous(), c["G0"].to(DEV).contiguous()


def flags_of(tiles, value=1):
    return (tiles.to(torch.uint8) * value).contiguous().to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# 1 - 3: the plain, the consuming and the flagged form
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.CASES)
def test_depth_bwd_plain(name, cases):
    """harp_depth_bwd: g_ndc within the bound, g_z bit-identical afterwards; a cotangent on uncovered pixels as well changes nothing"""
    L, _ = _L()
    c = device_case(cases, name)
    for tag, cot in (("plain", c["cot"]), ("plain, cotangent on uncovered pixels too", c["cot_everywhere"])):
        gz, gn = fresh(c, cot)
        assert L.harp_depth_bwd(*head(c, gz, gn), _st()) == 0
        torch.cuda.synchronize()
        assert _same_bits(gz, cot)
        check(c, gn, tag)
    assert int((c["cot_everywhere"] != 0).sum()) > int((c["cot"] != 0).sum()) or not (c["fid"] < 0).any()


@pytest.mark.parametrize("name", D.CASES)
def test_depth_bwd_consume(name, cases):
    """harp_depth_bwd_consume: the same g_ndc, and g_z all-zero afterwards"""
    L, _ = _L()
    c = device_case(cases, name)
    gz, gn = fresh(c)
    assert L.harp_depth_bwd_consume(*head(c, gz, gn), _st()) == 0
    torch.cuda.synchronize()
    assert int((gz != 0).sum()) == 0
    check(c, gn, "consume")


@pytest.mark.parametrize("name", D.CASES)
def test_depth_bwd_tiles(name, cases):
    """harp_depth_bwd_tiles: (a) every tile that holds a cotangent flagged; (b) a checkerboard half of them: the reference with the cotangent
    zeroed in the unflagged tiles, whose g_z stays bit-identical; (c) no flag: nothing is touched; (d) no flag image: the consuming form"""
    L, p = _L()
    c = device_case(cases, name)
    # a
    gz, gn = fresh(c)
    fl = flags_of(c["holds"], 255)
    assert L.harp_depth_bwd_tiles(*head(c, gz, gn), p(fl), _st()) == 0
    torch.cuda.synchronize()
    assert int((gz != 0).sum()) == 0 and int(fl.max()) == 0
    check(c, gn, "tiles, all flagged")
    # b
    gz, gn = fresh(c)
    fl = flags_of(c["half"])
    assert L.harp_depth_bwd_tiles(*head(c, gz, gn), p(fl), _st()) == 0
    torch.cuda.synchronize()
    m = c["in_half"]
    assert int((gz.cpu()[m] != 0).sum()) == 0 and _same_bits(gz.cpu()[~m], c["cot"][~m]) and int((c["cot"][~m] != 0).sum()) > 0
    assert int(fl.max()) == 0
    check(c, gn, "tiles, checkerboard", ref=c["ref_half"])
    # c
    gz, gn = fresh(c)
    fl = flags_of(c["holds"], 0)
    assert L.harp_depth_bwd_tiles(*head(c, gz, gn), p(fl), _st()) == 0
    torch.cuda.synchronize()
    assert _same_bits(gz, c["cot"]) and _same_bits(gn, c["G0"]) and int(fl.max()) == 0
    # d
    gz, gn = fresh(c)
    assert L.harp_depth_bwd_tiles(*head(c, gz, gn), None, _st()) == 0
    torch.cuda.synchronize()
    assert int((gz != 0).sum()) == 0
    check(c, gn, "tiles, no flag image")


# ----------------------------------------------------------------------------------------------------------------------
# 4: the normal map's chain rule riding in the launch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def texels():
    """x, gy, the pre-fill and the float64 autograd gradient of F.normalize(x, dim=-1, eps=1e-12): 64 texels of length <= 1e-12 (the 1e12
    branch), at the head, around the end of the first pass of the rider's 1024 workgroups and at the tail"""
    g = torch.Generator().manual_seed(41)
    n = N_TEXELS
    x = torch.randn(n, 3, generator=g)
    unit = F.normalize(torch.randn(64, 3, generator=g), dim=-1)
    tiny = unit * torch.cat([torch.zeros(8), torch.full((24,), 1e-13), torch.full((32,), 4e-13)])[:, None]
    at = torch.cat([torch.arange(16), D.RIDER_CAP - 8 + torch.arange(16), n - 32 + torch.arange(32)])
    x[at] = tiny
    gy = torch.randn(n, 3, generator=g)
    G0 = torch.randn(n, 3, generator=g)
    x64 = x.double().requires_grad_()
    F.normalize(x64, dim=-1, eps=1e-12).backward(gy.double())
    nx = x.double().norm(dim=-1, keepdim=True)
    assert int((nx <= 1e-12).sum()) == 64
    # tests/test_gpu_building_blocks.py's bound for harp_normalize3_bwd: gx = (g - n (n . g)) / |x| (or g 1e12 under the clamp): 8 roundings of
    # |g| / max(|x|, 1e-12), one of the pre-fill
    bound = 8 * U * gy.double().abs().sum(-1, keepdim=True) / nx.clamp_min(1e-12) + 2 * U * G0.double().abs()
    L, p = _L()
    xd, gyd, alone = x.to(DEV), gy.to(DEV), G0.to(DEV)
    assert L.harp_normalize3_bwd(p(xd), p(gyd), n, p(alone), _st()) == 0
    torch.cuda.synchronize()
    t = dict(n=n, x=xd, gy=gyd, G0=G0, ref=x64.grad, bound=bound, alone=alone.cpu())
    yield t
    t.clear()


def check_texels(t, g_nmap, tag):
    err = (g_nmap.cpu().double() - t["G0"].double() - t["ref"]).abs()
    assert torch.isfinite(err).all()
    worst = (err / t["bound"]).max().item()
    differ = int((_bits(g_nmap) != _bits(t["alone"])).sum())
    print(f"[{tag}] normal-map rider err / bound {worst:.3f}; {differ} of {err.numel()} elements differ from harp_normalize3_bwd's")
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("name", D.CASES)
def test_depth_bwd_with_the_normal_map_rider(name, cases, texels):
    """harp_depth_nmap_bwd (with tile flags) and harp_depth_bwd_riders with the normal-map rider alone: n_texels one past a pass of the
    rider's workgroups, g_nmap pre-filled; the depth part within its bound in the same launch"""
    L, p = _L()
    c, t = device_case(cases, name), texels
    gz, gn = fresh(c)
    fl = flags_of(c["holds"])
    g_nmap = t["G0"].to(DEV)
    assert L.harp_depth_nmap_bwd(*head(c, gz, gn), p(t["x"]), p(t["gy"]), t["n"], p(g_nmap), p(fl), _st()) == 0
    torch.cuda.synchronize()
    assert int((gz != 0).sum()) == 0 and int(fl.max()) == 0
    check(c, gn, "nmap_bwd")
    check_texels(t, g_nmap, f"{name} nmap_bwd")
    gz, gn = fresh(c)
    g_nmap = t["G0"].to(DEV)
    assert L.harp_depth_bwd_riders(*head(c, gz, gn), None, p(t["x"]), p(t["gy"]), t["n"], p(g_nmap), None, None, None, None, _st()) == 0
    torch.cuda.synchronize()
    assert int((gz != 0).sum()) == 0
    check(c, gn, "riders, normal map")
    check_texels(t, g_nmap, f"{name} riders, normal map")


# ----------------------------------------------------------------------------------------------------------------------
# 5: the interleaved vertex gradients unpacked in the launch
# ----------------------------------------------------------------------------------------------------------------------
def vert9(c):
    g = torch.Generator().manual_seed(c["V"] + 5)
    B, V = c["B"], c["V"]
    g9 = torch.randn(B, V, 9, generator=g) * (torch.rand(B, V, 9, generator=g) >= 1.0 / 3.0)          # a third of the entries exactly zero
    dst = [torch.randn(B, V, 3, generator=g) for _ in range(3)]                                       # g_verts, g_vnormals, g_ndc_cam
    want = [d + g9[..., 3 * k:3 * k + 3] for k, d in enumerate(dst)]                                  # one float32 add per destination
    assert 0.25 < (g9 == 0).float().mean().item() < 0.42
    return g9, dst, want


@pytest.mark.parametrize("name", D.CASES)
def test_depth_bwd_with_the_vertex_rider(name, cases, texels):
    """harp_depth_bwd_riders with g_vert9 (alone; then with the normal-map rider and tile flags): every destination receives exactly one add,
    so the three arrays are bit-equal to torch's float32 dst + x, g9 is all-zero afterwards, and the light view's g_ndc — another buffer than
    g_ndc_cam — receives the depth gradient only.  B V 9 > 262 144 on `wrap`: the rider's own stride loop wraps there"""
    L, p = _L()
    c, t = device_case(cases, name), texels
    g9, dst, want = vert9(c)
    for both in (False, True):
        gz, gn = fresh(c)
        g9d, dd = g9.to(DEV), [d.to(DEV) for d in dst]
        fl = flags_of(c["holds"]) if both else None
        g_nmap = t["G0"].to(DEV) if both else None
        nm = (p(t["x"]), p(t["gy"]), t["n"], p(g_nmap)) if both else (None, None, 0, None)
        assert L.harp_depth_bwd_riders(*head(c, gz, gn), p(fl), *nm, p(g9d), p(dd[0]), p(dd[1]), p(dd[2]), _st()) == 0
        torch.cuda.synchronize()
        tag = "riders, both + flags" if both else "riders, vertex"
        assert int((g9d != 0).sum()) == 0 and int((gz != 0).sum()) == 0
        for k, what in enumerate(("g_verts", "g_vnormals", "g_ndc_cam")):
            assert _same_bits(dd[k], want[k]), (name, tag, what, int((_bits(dd[k]) != _bits(want[k])).sum()))
        check(c, gn, tag)
        if both:
            assert int(fl.max()) == 0
            check_texels(t, g_nmap, f"{name} {tag}")
    print(f"[{name}] vertex rider: {c['B'] * c['V'] * 9} floats, {'wraps' if c['B'] * c['V'] * 9 > D.RIDER_CAP else 'one pass'}")


# ----------------------------------------------------------------------------------------------------------------------
# 6: refusals, with real buffers
# ----------------------------------------------------------------------------------------------------------------------
def test_rider_refusals_leave_every_buffer_untouched(cases, texels):
    L, p = _L()
    c, t = device_case(cases, "dense"), texels
    g9, dst, _ = vert9(c)

    def buffers():
        gz, gn = fresh(c)
        return dict(gz=gz, gn=gn, fl=flags_of(c["holds"]), g_nmap=t["G0"].to(DEV), g9=g9.to(DEV), gv=dst[0].to(DEV), gnr=dst[1].to(DEV), gc=dst[2].to(DEV))

    def untouched(b):
        torch.cuda.synchronize()
        want = dict(gz=c["cot"], gn=c["G0"], fl=c["holds"].to(torch.uint8), g_nmap=t["G0"], g9=g9, gv=dst[0], gnr=dst[1], gc=dst[2])
        return all(torch.equal(b[k].cpu(), want[k]) for k in want)

    b = buffers()            # the normal-map rider without texels
    rc = L.harp_depth_bwd_riders(*head(c, b["gz"], b["gn"]), p(b["fl"]), p(t["x"]), p(t["gy"]), 0, p(b["g_nmap"]), p(b["g9"]), p(b["gv"]), p(b["gnr"]), p(b["gc"]), _st())
    assert rc == 1 and untouched(b)
    for missing in ("gv", "gnr", "gc"):                                   # the vertex rider without one of its destinations
        b = buffers()
        d = {k: (None if k == missing else p(b[k])) for k in ("gv", "gnr", "gc")}
        rc = L.harp_depth_bwd_riders(*head(c, b["gz"], b["gn"]), p(b["fl"]), p(t["x"]), p(t["gy"]), t["n"], p(b["g_nmap"]), p(b["g9"]), d["gv"], d["gnr"], d["gc"], _st())
        assert rc == 1 and untouched(b), missing
    b = buffers()            # harp_depth_nmap_bwd without the normal map
    rc = L.harp_depth_nmap_bwd(*head(c, b["gz"], b["gn"]), None, p(t["gy"]), t["n"], p(b["g_nmap"]), p(b["fl"]), _st())
    assert rc == 1 and untouched(b)
