"""CPU checks of self-contact's parts, no device: the geodesic exclusion against a float64 Floyd-Warshall, the bit table
against its documented layout, harp_mesh_contact_excl's argument errors (fake pointers, no launch, after tests/test_contact_abi.py), the
wind > 1 rule on known geometry, and the caps of tests/test_gpu_contact_excl.py counted on the reference alone."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import _contact_excl_ref as XR
from tests import _contact_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20                                                 # a fake device pointer, 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


# ---- geodesic_exclusion --------------------------------------------------------------------------------------------------------------------
def _meshes():
    v, f = CR.icosphere(1)
    yield "ico1", v, f
    v, f, _ = CR.open_icosphere(2)
    yield "open2", v, f
    v, f = CR.multi_mesh(11, 3)
    yield "multi127", v, f


@pytest.mark.parametrize("name,verts,faces", list(_meshes()), ids=lambda x: x if isinstance(x, str) else "")
def test_geodesic_exclusion_is_floyd_warshall(name, verts, faces):
    from harp_amd.playback.selfcontact import geodesic_exclusion
    P = XR.edge_paths(verts, faces)
    V, F = len(verts), len(faces)
    incident = np.zeros((V, F), bool)
    for k in range(3):
        incident[faces[:, k], np.arange(F)] = True
    for radius in (0.0, 0.3, 0.8, np.inf):
        got = geodesic_exclusion(torch.from_numpy(verts), torch.from_numpy(faces), radius)
        assert got.dtype == torch.bool and tuple(got.shape) == (V, F)
        got = got.numpy()
        want = XR.exclusion(P, faces, radius)
        with np.errstate(invalid="ignore"):
            clear = ~(np.abs(P[:, faces.astype(np.int64)] - radius) <= 1e-9).any(-1)
        assert np.array_equal(got[clear], want[clear]), (name, radius)
        assert radius == 0.0 or clear.mean() > 0.99, (name, radius)        # (at radius 0 the incident faces sit AT the radius: exact below)
        assert (got | ~incident).all(), ("a vertex's own faces are always excluded", name, radius)
        if radius == 0.0:
            assert np.array_equal(got, incident), name
        if radius == np.inf:
            assert np.array_equal(got, np.isfinite(P)[:, faces.astype(np.int64)].any(-1)), name
    # float32 vertices and int32 faces are taken as they are
    got32 = geodesic_exclusion(torch.from_numpy(verts).float(), torch.from_numpy(faces).int(), 0.3).numpy()
    assert (got32 != XR.exclusion(P, faces, 0.3)).mean() < 0.01
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            geodesic_exclusion(torch.from_numpy(verts), torch.from_numpy(faces), bad)


def test_geodesic_exclusion_on_the_hand_template():
    """the real 778-vertex template at rest, 3 cm: 8.18 % of the (vertex, face) pairs are excluded"""
    from harp_amd.playback.selfcontact import geodesic_exclusion
    with np.load(os.path.join(ROOT, "harp_amd", "assets", "hand_template.npz")) as z:
        verts, faces = z["base_verts"].astype(np.float64), z["faces0"].astype(np.int64)
    got = geodesic_exclusion(torch.from_numpy(verts), torch.from_numpy(faces), 0.03).numpy()
    assert got.shape == (778, len(faces)) and abs(got.mean() - 0.08) <= 0.01, got.mean()
    print(f"[geodesic_exclusion] hand template, 0.03 m: excluded share {got.mean():.4f}")


def test_the_conventions_on_the_hand_template_at_rest():
    """SELF_GEODESIC and SELF_CONTACT_DIST on the real template at rest, float64 brute force: no vertex has a counting face within 4 mm
    (the nearest is at 4.56 mm), 39 are within 1 cm and 336 within 2 cm, so the between-avatars 2 cm is not usable within one hand; the
    unmasked winding number of a vertex on its own surface is 0.14 .. 0.82, below the inside threshold of 1"""
    from harp_amd.playback import CONTACT_DIST, SELF_CONTACT_DIST, SELF_GEODESIC
    from harp_amd.playback.selfcontact import geodesic_exclusion
    with np.load(os.path.join(ROOT, "harp_amd", "assets", "hand_template.npz")) as z:
        verts, faces = z["base_verts"].astype(np.float64), z["faces0"].astype(np.int64)
    mask = geodesic_exclusion(torch.from_numpy(verts), torch.from_numpy(faces), SELF_GEODESIC).numpy()
    side = dict(verts=verts[None], cam_R=np.eye(3).reshape(1, 9), cam_T=np.zeros((1, 3)), faces=faces)
    ref = XR.masked(CR.mesh_contact(side, side), mask)
    d, w = ref["d_min"][0], ref["wind_all"][0]
    assert (d > SELF_CONTACT_DIST).all() and abs(d.min() - 0.00456) < 1e-5, d.min()
    assert (d <= 0.01).sum() == 39 and (d <= CONTACT_DIST).sum() == 336
    assert 0.14 < w.min() and w.max() < 0.83 and (w < 0.95).all(), (w.min(), w.max())
    assert (CR.mesh_contact(side, side)["d_min"] == 0).all(), "without the exclusion every vertex is at distance 0 from its own faces"


# ---- the bit table -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 127, 128, 129, 320])
def test_pack_round_trip_and_size(lib, F):
    from harp_amd.playback.selfcontact import pack_exclusion, unpack_exclusion
    V = 7
    mask = np.random.default_rng(F).random((V, F)) < 0.4
    mask[0], mask[1] = True, False
    table = pack_exclusion(torch.from_numpy(mask))
    C = -(-F // 128)
    assert table.dtype == torch.int32 and tuple(table.shape) == (C, V, 4) and table.is_contiguous()
    assert np.array_equal(table.numpy().view(np.uint32), XR.pack(mask))
    assert np.array_equal(unpack_exclusion(table, F).numpy(), mask)
    assert lib.harp_contact_excl_words(V, F) == table.numel() == C * V * 4
    # the bits past F are zero
    full = unpack_exclusion(table, C * 128).numpy()
    assert not full[:, F:].any()


def test_pack_bit_positions(lib):
    from harp_amd.playback.selfcontact import pack_exclusion
    V, F = 3, 300
    for i, f in ((0, 0), (1, 31), (2, 32), (0, 127), (1, 128), (2, 163), (0, 299)):
        mask = np.zeros((V, F), bool)
        mask[i, f] = True
        t = pack_exclusion(torch.from_numpy(mask)).numpy().view(np.uint32)
        c, k = divmod(f, 128)
        want = np.zeros((3, V, 4), np.uint32)
        want[c, i, k >> 5] = np.uint32(1) << np.uint32(k & 31)
        assert np.array_equal(t, want), (i, f)
        # the flat word the header names: excl[(c * V + i) * 4 + (k >> 5)]
        assert t.reshape(-1)[(c * V + i) * 4 + (k >> 5)] == 1 << (k & 31)
    f = lib.harp_contact_excl_words
    assert f(0, 10) == 0 and f(5, 0) == 0 and f(-1, 3) == 0 and f(3, -1) == 0
    assert f(3093, 6152) == 49 * 3093 * 4


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------------
def _mesh(**over):
    from harp_amd import _lib
    m = dict(verts=FAKE, cam_R=FAKE, cam_T=FAKE, faces=FAKE, V=5, F=7, flip_x=0, reserved=0)
    m.update(over)
    return _lib.ContactMesh(**m)


def _call(lib, q, t, excl=FAKE, B=2, max_dist=0.02, ws=FAKE, dist=FAKE, face=FAKE, wind=FAKE):
    ref = lambda m: None if m is None else ctypes.byref(m)      # noqa: E731
    return lib.harp_mesh_contact_excl(ref(q), ref(t), excl, B, max_dist, ws, dist, face, wind, None)


def test_argument_errors_return_before_any_launch(lib):
    ok = _mesh()
    assert _call(lib, None, ok) == 1 and _call(lib, ok, None) == 1
    assert _call(lib, ok, ok, ws=None) == 1 and _call(lib, ok, ok, excl=None) == 1
    for field in ("verts", "cam_R", "cam_T"):
        assert _call(lib, _mesh(**{field: None}), ok) == 1, ("query", field)
        assert _call(lib, ok, _mesh(**{field: None})) == 1, ("target", field)
    assert _call(lib, ok, _mesh(faces=None)) == 1
    for bad in (0, -1):
        assert _call(lib, _mesh(V=bad), ok) == 1 and _call(lib, ok, _mesh(V=bad)) == 1 and _call(lib, ok, _mesh(F=bad)) == 1
        assert _call(lib, ok, ok, B=bad) == 1
    assert _call(lib, _mesh(reserved=1), ok) == 1 and _call(lib, ok, _mesh(reserved=-3)) == 1
    for bad in (-0.001, -math.inf, math.nan):
        assert _call(lib, ok, ok, max_dist=bad) == 1, bad
    assert _call(lib, ok, ok, dist=None, face=None, wind=None) == 1
    for off in (4, 8, 12):
        assert _call(lib, ok, ok, excl=FAKE + off) == 1, off                  # not 16-byte aligned
    assert _call(lib, ok, ok, ws=FAKE + 4) == 1


def test_signatures_and_constant():
    from harp_amd import _lib, ops
    assert {"harp_contact_excl_words", "harp_mesh_contact_excl"} <= set(_lib.SIGNATURES)
    with open(os.path.join(ROOT, "include", "harp_hip.h")) as f:
        assert "#define HARP_CONTACT_EXCL_FACES 128" in f.read()
    assert ops.CONTACT_EXCL_FACES == XR.EXCL_FACES == 128


# ---- the wind > 1 rule on known geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [1.6, 1.9])
def test_two_spheres_inside_is_wind_above_one(gap):
    """two overlapping unit spheres as one mesh, each sphere's own faces excluded: the vertices inside the other sphere are exactly those
    whose UNMASKED winding number exceeds 1, and none is near 1"""
    side, mask = XR.self_case(gap)
    ref = XR.masked(CR.mesh_contact(side, side), mask)
    verts, faces, vs, fs = XR.two_spheres(gap)
    centre = np.array([[0.0, 0.0, 0.0], [gap, 0.0, 0.0]])
    r_other = np.linalg.norm(verts - centre[1 - vs], axis=1)
    # inside the other sphere, without a winding number: an icosphere is convex, so a point is inside it iff it lies behind every face
    a, b, c = (verts[faces[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    height = ((verts[:, None, :] - a[None]) * n[None]).sum(-1) / np.linalg.norm(n, axis=1)      # (324,640): above the face's plane
    other = vs[:, None] != fs[None, :]
    inside = np.where(other, height, -np.inf).max(1) < 0
    assert (ref["d_min"][0] > 1e-3 * CR.SCALE).all(), "no vertex lies on the other sphere's surface"
    assert inside.any() and (~inside).any()
    w = ref["wind_all"][0]
    assert np.array_equal(w > 1.0, inside)
    assert (np.abs(w - 1.0) >= 0.05).all(), np.abs(w - 1.0).min()
    assert (w[~inside] > 0.3).all() and (w[~inside] < 0.6).all() and (w[inside] > 1.3).all() and (w[inside] < 1.6).all()
    # the masked distance of an inside vertex is its depth under the other sphere's surface, within the polyhedron's sag
    depth = 1.0 - r_other[inside]
    assert (np.abs(ref["d_min"][0][inside] / CR.SCALE - depth) < 0.02).all()
    print(f"[two spheres] gap {gap}: wind outside {w[~inside].min():.3f} .. {w[~inside].max():.3f}, inside {w[inside].min():.3f} .. {w[inside].max():.3f}")


# ---- the players' composition, on the CPU ---------------------------------------------------------------------------------------------------
def test_compose_self_contact_is_the_documented_rule():
    from harp_amd.playback.player import SelfContact, compose_self_contact
    rng = np.random.default_rng(3)
    n, V, F, P = 3, 200, 90, 6
    f = np.where(rng.random((n, V)) < 0.3, rng.integers(0, F, (n, V)), -1).astype(np.int32)
    d = np.where(f >= 0, rng.random((n, V)) * 0.004, np.inf).astype(np.float32)
    w = np.where(f >= 0, rng.random((n, V)) * 1.6, 0.0).astype(np.float32)
    w[0, 0], f[0, 0], d[0, 0] = 1.0, 5, 0.001                                  # exactly 1: not inside
    f[2], d[2], w[2] = -1, np.inf, 0.0                                         # a frame without contact
    part_table, own = rng.integers(1, P, F).astype(np.uint8), rng.integers(1, P, V).astype(np.uint8)
    t = torch.from_numpy
    got = compose_self_contact(t(d), t(f), t(w), t(part_table), t(own), P)
    assert isinstance(got, SelfContact)
    want = XR.compose_self(d, f, w, part_table, own, P)
    for name, a, b in zip(SelfContact._fields, got, want):
        assert a.numpy().dtype == b.dtype and np.array_equal(a.numpy(), b), name
    assert got.dist[0, 0] > 0 and np.isposinf(got.min_dist[2].item()) and got.max_penetration[2] == 0 and not got.touch[2].any()
    assert got.max_penetration.min() >= 0 and (got.dist[got.wind > 1] < 0).all()
    for a, src in ((got.face, f), (got.wind, w), (got.own_part, own)):           # every tensor is new
        assert a.data_ptr() != t(src).data_ptr()


def test_what_the_arguments_refuse():
    from harp_amd.playback.player import _self_contact_args
    assert _self_contact_args(0.004, 0.03) == (0.004, 0.03) and _self_contact_args(0, float("inf")) == (0.0, float("inf"))
    for md, geo in ((0.03, 0.03), (0.01, 0.005), (0.0, 0.0)):
        with pytest.raises(ValueError, match="geodesic"):
            _self_contact_args(md, geo)
    for bad in (-0.001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_dist"):
            _self_contact_args(bad, 0.03)
    from harp_amd.playback.cli import parse_args
    base = ["--config", "c", "--motion", "m", "--out", "o"]
    a = parse_args(base + ["--self-contacts"])
    assert a.self_contacts and (a.self_contact_dist, a.self_geodesic) == (0.004, 0.03) and not parse_args(base).self_contacts
    assert parse_args(base + ["--self-contacts", "--also", "c:m", "--contacts"]).contacts
    for extra in (["--self-contact-dist", "0.05"], ["--self-contact-dist", "-1"], ["--self-contact-dist", "inf"], ["--self-geodesic", "0.004"]):
        with pytest.raises(SystemExit):
            parse_args(base + ["--self-contacts"] + extra)


def test_vertex_parts_of_the_subdivided_mesh():
    from harp_amd.playback.labels import face_part_labels, subdivided_vertex_part_labels, vertex_part_labels
    rng = np.random.default_rng(1)
    w = rng.random((6, 4))
    edges0 = np.array([[0, 1], [1, 2], [2, 0], [3, 4], [4, 5]])
    got = subdivided_vertex_part_labels(w, edges0)
    assert got.dtype == np.uint8 and got.shape == (11,) and np.array_equal(got[:6], vertex_part_labels(w))
    assert np.array_equal(got[6:], 1 + (w[edges0[:, 0]] + w[edges0[:, 1]]).argmax(1))
    assert np.array_equal(subdivided_vertex_part_labels(w, np.zeros((0, 2), int)), vertex_part_labels(w))
    # the face rule is untouched: corner sub-faces take their corner's vertex part
    faces0 = np.array([[0, 1, 2], [3, 4, 5]])
    assert np.array_equal(face_part_labels(w, faces0, 6)[:2], vertex_part_labels(w)[faces0[:, 0]])


# ---- the caps of the GPU test, on the reference alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Vq", CR.QUERY_V)
@pytest.mark.parametrize("B", [1, 3])
def test_caps_of_the_gpu_grid(B, Vq):
    worst = [0.0, 0.0]
    for k, (name, q, t) in enumerate(CR.grid_cases(B, Vq)):
        ref = CR.mesh_contact(q, t)
        for tag, mask in XR.masks(ref, 7 * k + Vq):
            ref_m = XR.masked(ref, mask)
            for md in CR.MAX_DISTS:
                maybe, band, n = XR.caps(ref_m, md)
                assert maybe <= 0.02 * n and band <= 0.02 * n, (name, tag, md, maybe, band, n)
                worst = [max(worst[0], maybe / n), max(worst[1], band / n)]
    for qf, tf in ((False, False), (True, True), (False, True), (True, False)):
        q, t = CR.degenerate_case(B, qf, tf)
        ref = CR.mesh_contact(q, t)
        tag, mask = list(XR.masks(ref, 11))[1]
        for md in CR.MAX_DISTS:
            maybe, band, n = XR.caps(XR.masked(ref, mask), md)
            assert maybe <= 0.02 * n and band <= 0.02 * n, ("degenerate", qf, tf, md, maybe, band, n)
    print(f"[caps] B={B} Vq={Vq}: largest undecided share {worst[0]:.4f}, largest share with wind near 0.5 {worst[1]:.4f} (caps 0.02)")
