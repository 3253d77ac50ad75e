"""-m gpu: harp_taubin_smooth (csrc/smooth.hip) and ops.taubin_smooth / ops.taubin_smoothing against the float64 restatement of
tests/_taubin_ref.py.  The bound is that module's (4 e_ref + num_iter ulp32(max |coordinate|), from the reference alone); every case also
asserts that its input tells inverse-length weights from uniform ones by >= 50 bounds.

Measured on MI355X, e_hip / e_ref (both modes gave the same bits in every case): tetra 0.160, grid2x2 0.312 (num_iter 1) / 0.209 (10),
grid5x13 0.317 / 0.238, grid33x34 0.326 / 0.262, other factors 0.183, isolated vertex 0.206, coincident pair 0.229, hand 0.422, arm 0.415,
grid65x64 (mode 2 only) 0.295: the kernel's difference form is closer to float64 than the float32 yardstick."""
import types

import numpy as np
import pytest
import torch

from tests import _taubin_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG = 1
_DEV = {}                              # device copies of a case's input and tables (the cached case itself stays as it is)


def _lib():
    from harp_amd import _lib
    return _lib


def _dev(c):
    if c["name"] not in _DEV:
        _DEV[c["name"]] = (c["verts"].to(DEV), c["nbr_off"].to(DEV), c["nbr_idx"].to(DEV))
    return _DEV[c["name"]]


def _raw(c, mode, num_iter=None, verts=None, out=None, ws="alloc"):
    """the C entry point on device buffers: returns (status, out)"""
    L = _lib()
    v, off, idx = _dev(c)
    v = v if verts is None else verts
    out = torch.full_like(v, float("nan")) if out is None else out
    if isinstance(ws, str):
        ws = torch.empty(max(1, L.lib().harp_taubin_ws_bytes(c["B"], c["V"])), dtype=torch.uint8, device=DEV)
    n = c["num_iter"] if num_iter is None else num_iter
    rc = L.lib().harp_taubin_smooth(L.ptr(v), L.ptr(off), L.ptr(idx), c["B"], c["V"], c["lambd"], c["mu"], n, mode, L.ptr(out), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    return rc, out


def _check(c, got, tag):
    got = got.cpu()
    e_hip = (got.double() - c["ref"]).abs().max().item()
    print(f"[taubin] {c['name']} {tag}: V {c['V']} B {c['B']} num_iter {c['num_iter']}  e_hip {e_hip:.3e}  e_ref {c['e_ref']:.3e}  "
          f"e_hip/e_ref {e_hip / c['e_ref']:.3f}  bound {c['bound']:.3e}  uniform gap / bound {c['uniform_gap'] / c['bound']:.0f}")
    assert c["uniform_gap"] >= 50.0 * c["bound"], (c["name"], c["uniform_gap"], c["bound"])      # on the reference alone
    assert torch.isfinite(got).all()
    assert e_hip <= c["bound"], (c["name"], tag, e_hip, c["bound"])
    return got


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", R.CASES)
def test_against_float64(name, mode):
    c = R.case(name)
    rc, out = _raw(c, mode)
    assert rc == 0
    got = _check(c, out, f"mode {mode}")
    if name == "grid5x13_isolated":
        assert torch.equal(got[:, 65], c["verts"][:, 65])                  # no neighbour: bit-unchanged (PyTorch3D: NaN)
        assert c["nbr_off"][66] == c["nbr_off"][65]
    if name == "grid5x13_coincident":
        assert torch.equal(c["verts"][:, 30], c["verts"][:, 31])


def test_past_the_lds_capacity():
    """V = 4160: mode 1 refuses, mode 2 and mode 0 (which must pick the global path) meet the bound and agree bit for bit"""
    c = R.case(R.BIG)
    assert c["V"] > 4096
    rc, _ = _raw(c, 1)
    assert rc == ERR_ARG
    rc2, out2 = _raw(c, 2)
    rc0, out0 = _raw(c, 0)
    assert rc2 == 0 and rc0 == 0
    _check(c, out2, "mode 2")
    assert torch.equal(out0, out2)
    assert _raw(c, 0, ws=None)[0] == ERR_ARG                               # the path mode 0 picks here needs the workspace
    from harp_amd import ops
    topo = types.SimpleNamespace(nbr_off=_dev(c)[1], nbr_idx=_dev(c)[2])
    assert torch.equal(ops.taubin_smooth(_dev(c)[0], topo, num_iter=1), out2)
    with pytest.raises(ValueError, match="4096"):
        ops.taubin_smooth(_dev(c)[0], topo, num_iter=1, mode=1)


@pytest.mark.parametrize("name", ["grid33x34_n10", "hand"])
def test_mode0_is_the_lds_path_where_it_fits(name):
    c = R.case(name)
    rc0, out0 = _raw(c, 0, ws=None)                                         # no workspace needed
    rc1, out1 = _raw(c, 1, ws=None)
    assert rc0 == 0 and rc1 == 0 and torch.equal(out0, out1)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_num_iter_zero_copies_bit_for_bit(mode):
    c = R.case("grid33x34_n10")
    v = _dev(c)[0].clone()
    v[0, 0, 0] = float("nan")                                               # a copy, not arithmetic: even a NaN payload survives
    v[0, 1, 1] = -0.0
    rc, out = _raw(c, mode, num_iter=0, verts=v, ws=None)
    assert rc == 0
    assert torch.equal(out.view(torch.int32), v.view(torch.int32))
    rc, same = _raw(c, mode, num_iter=0, verts=v, out=v, ws=None)           # aliased: nothing to do
    assert rc == 0 and same.data_ptr() == v.data_ptr()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["grid33x34_n10", "grid2x2_n1"])
def test_out_may_alias_verts(name, mode):
    c = R.case(name)
    _, sep = _raw(c, mode)
    v = _dev(c)[0].clone()
    rc, out = _raw(c, mode, verts=v, out=v)
    assert rc == 0 and out.data_ptr() == v.data_ptr()
    assert torch.equal(v, sep)


def test_ops_takes_views_and_single_meshes():
    from harp_amd import ops
    c = R.case("grid33x34_n10")
    v, off, idx = _dev(c)
    topo = types.SimpleNamespace(nbr_off=off, nbr_idx=idx)
    _, want = _raw(c, 0)
    wide = torch.zeros(c["B"], c["V"], 5, device=DEV)
    wide[..., 1:4] = v
    view = wide[..., 1:4]
    assert not view.is_contiguous()
    assert torch.equal(ops.taubin_smooth(view, topo), want)
    perm = v.permute(1, 0, 2).contiguous().permute(1, 0, 2)                # (B,V,3) with the frame stride inside
    assert not perm.is_contiguous()
    for mode in (0, 1, 2):
        assert torch.equal(ops.taubin_smooth(perm, topo, mode=mode), _raw(c, mode)[1])
    assert torch.equal(ops.taubin_smooth(v[1], topo), want[1])             # (V,3)
    assert torch.equal(v, c["verts"].to(DEV))                               # the input is left alone
    c5 = R.case("grid5x13_factors")
    v5, off5, idx5 = _dev(c5)
    got = ops.taubin_smooth(v5, types.SimpleNamespace(nbr_off=off5, nbr_idx=idx5), c5["lambd"], c5["mu"], c5["num_iter"])
    _check(c5, got, "ops")
    with pytest.raises(ValueError, match="neighbour table"):
        ops.taubin_smooth(v5, topo)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.taubin_smooth(c5["verts"], topo)


@pytest.mark.parametrize("kind", ["hand", "arm"])
def test_meshes_level_call_on_the_device_topology(kind):
    """ops.taubin_smoothing(Meshes) over the DeviceTopology of the real templates: its CSR lists the same neighbours as the edge list the
    reference sums over, and the new Meshes shares faces, textures and topology"""
    from harp_amd import ops
    from harp_amd.structures import Meshes, TexturesUV
    c = R.case(kind)
    tpl = R.synth.load_template(kind)
    topo = ops.DeviceTopology(c["topo"], tpl["verts_uvs"], tpl["faces_uvs"], DEV)
    assert torch.equal(topo.nbr_off.cpu(), c["nbr_off"]) and torch.equal(topo.nbr_idx.cpu(), c["nbr_idx"])
    tex = TexturesUV(torch.rand(1, 8, 8, 3, device=DEV), torch.from_numpy(tpl["faces_uvs"])[None], torch.from_numpy(tpl["verts_uvs"])[None])
    faces = topo.faces.long()[None].expand(c["B"], -1, -1)
    m = Meshes(_dev(c)[0], faces, tex, topo)
    with torch.no_grad():
        m2 = ops.taubin_smoothing(m)
    assert isinstance(m2, Meshes) and m2.textures is tex and m2.topo is topo and m2.faces_padded() is faces and len(m2) == c["B"]
    _check(c, m2.verts_padded(), "Meshes")
    assert tex.verts_uvs_padded().shape == (1, tpl["verts_uvs"].shape[0], 2) and tex.faces_uvs_padded().shape == (1, topo.F, 3)
    assert TexturesUV(None, torch.zeros(4, 3), torch.zeros(5, 2)).verts_uvs_padded().shape == (1, 5, 2)


def test_bad_arguments_are_refused_without_a_launch():
    c = R.case("grid5x13_n10")
    L = _lib()
    lib = L.lib()
    v, off, idx = _dev(c)
    B, V = c["B"], c["V"]
    big = torch.zeros(1, 4097, 3, device=DEV)
    out = torch.full_like(v, 7.0)
    ws = torch.empty(lib.harp_taubin_ws_bytes(B, V), dtype=torch.uint8, device=DEV)
    p = L.ptr
    ok = (p(v), p(off), p(idx), B, V, 0.53, -0.53, 10, 0, p(out), p(ws), None)

    def call(**kw):
        names = ("verts", "nbr_off", "nbr_idx", "B", "V", "lambd", "mu", "num_iter", "mode", "out", "ws", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return lib.harp_taubin_smooth(*[a[n] for n in names])
    for kw in (dict(B=0), dict(B=-1), dict(V=0), dict(V=-1), dict(num_iter=-1), dict(verts=None), dict(nbr_off=None), dict(nbr_idx=None),
               dict(out=None), dict(mode=3), dict(mode=-1), dict(mode=2, ws=None), dict(mode=1, V=4097, B=1, verts=p(big), out=p(big))):
        for mode in ((kw["mode"],) if "mode" in kw else (0, 1, 2)):
            assert call(**dict(kw, mode=mode)) == ERR_ARG, (kw, mode)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                         # nothing ran
    assert call(ws=None) == 0 and call(mode=1, ws=None) == 0 and call(mode=2) == 0      # and the good calls do
    torch.cuda.synchronize()


def test_forward_only():
    from harp_amd import ops
    c = R.case("grid5x13_n10")
    v, off, idx = _dev(c)
    topo = types.SimpleNamespace(nbr_off=off, nbr_idx=idx)
    leaf = v.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="forward-only"):
        ops.taubin_smooth(leaf, topo)
    with torch.no_grad():
        got = ops.taubin_smooth(leaf, topo)
    assert not got.requires_grad and torch.equal(got, ops.taubin_smooth(v, topo))


@pytest.mark.parametrize("mode", [1, 2])
def test_inside_a_captured_graph(mode):
    """stream-ordered, no allocation, no synchronisation: captured once, replayed on new vertices"""
    c = R.case("grid33x34_n10")
    L = _lib()
    v, off, idx = _dev(c)
    _, want = _raw(c, mode)
    moved = v + 0.001
    _, want_moved = _raw(c, mode, verts=moved)
    src, out = v.clone(), torch.zeros_like(v)
    ws = torch.empty(L.lib().harp_taubin_ws_bytes(c["B"], c["V"]), dtype=torch.uint8, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = L.lib().harp_taubin_smooth(L.ptr(src), L.ptr(off), L.ptr(idx), c["B"], c["V"], c["lambd"], c["mu"], c["num_iter"], mode, L.ptr(out),
                                        L.ptr(ws), L.stream())
    assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    src.copy_(moved)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_moved)
