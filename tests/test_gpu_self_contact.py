"""-m gpu: AvatarPlayer.self_contact and ScenePlayer.self_contact (harp_amd/playback/player.py) on synthetic hand players at
img_size 64 and batch_size 2, built as tests/test_gpu_scene_contact.py builds its players.  The motion has one open-hand row (every finger
rotation zero: the shaped template) and two rows with every finger joint flexed by 0.6 and 1.2 rad about z, chosen on the CPU with
oracle.harp_ref.mano_forward: the flexed hands touch and penetrate themselves.

The synthetic model's random shape basis roughens the surface by about a millimetre, so its OPEN hand already has 13 (seed 31) and 6
(seed 57) vertices within SELF_CONTACT_DIST = 4 mm of a counting face, the nearest at 2.40 and 2.69 mm in float64 (the real template: none,
nearest 4.56 mm).  The tests therefore use max_dist = 2 mm, at which the open row has no contact and the flexed rows do (nearest 0.02 mm);
each asserts that from a float64 reference on the players' own buffers, so it is never vacuous.  The synthetic fist does penetrate itself
(wind > 1 at near vertices), which is asserted from the reference too; what wind > 1 MEANS rests on the spheres of
tests/test_contact_excl_cpu.py.

Checked: bit for bit ops.mesh_contact(..., exclude=) on the player's buffers composed by the documented rule restated in numpy vertex by
vertex, touch included; the same against float64: the near set, the distance and the winding number on every vertex, the face on every
64th; the exclusion table and own_part against their definitions; a mirrored player; replay = eager, reversed rows, one graph per key,
other passes' graphs undisturbed; a scene of two against each player's own; what is refused; the command line's self_contacts.npz; and,
through the op, the default distances on the REAL template at rest: no contact at 4 mm."""
import numpy as np
import pytest
import torch

from tests import _contact_excl_ref as XR
from tests import _contact_ref as CR
from tests.test_gpu_evaluate import _setup
from tests.test_gpu_scene_player import _players

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, T = 64, 3
MD, GEO = 0.002, 0.03
FLEX = (0.0, 0.6, 1.2)                                                          # rad about z on every finger joint, per row
_FITS = {}


def _hands(tmp_path_factory):
    """two synthetic fits, each with the open / flexed / fist motion (cfg, layer, params, motion); the second's camera is the first's"""
    from harp_amd.playback import Motion
    if "fits" not in _FITS:
        fits = []
        for seed in (31, 57):
            tmp = tmp_path_factory.mktemp(f"self_contact_hand_{seed}")
            _, cfg, layer, params, _ = _setup(T, S, seed, tmp, self_shadow=False, share_light_position=True)
            fits.append((cfg, layer, params))
        _FITS["fits"] = fits
    hands = []
    for cfg, layer, params in _FITS["fits"]:
        m = Motion.from_params(params)
        pose = torch.zeros(T, 15, 3)
        pose[:, :, 2] = torch.tensor(FLEX)[:, None]
        hm = torch.from_numpy(np.asarray(layer._model_np["hands_mean"], np.float32)).reshape(1, 45)
        m.pose = (pose.reshape(T, 45) - hm).to(m.pose.device).contiguous()
        hands.append((cfg, layer, params, m))
    hands[1][3].cam = hands[0][3].cam.clone().contiguous()
    return tuple(hands)


def _avatar(h, use_graph=True, keep_depth=False):
    p = _players((h,), 1, keep_depth, use_graph=use_graph)[0]
    p.load_motion(h[3])
    return p


def _np(c):
    return [t.cpu().numpy().copy() for t in c]


def _equal(a, b, sl=slice(None), rev=False):
    """two SelfContacts as _np lists; b's rows sl, reversed with rev (own_part has no rows)"""
    pick = lambda k, x: x if k == 3 else (x[sl][::-1] if rev else x[sl])      # noqa: E731
    return all(np.array_equal(x, pick(k, y)) for k, (x, y) in enumerate(zip(a, b)))


def _op(pl, flip, md, geo):
    """ops.mesh_contact with the player's exclusion table on the buffers it holds (its last batch)"""
    from harp_amd import ops
    side = ops.ContactMesh(pl.s["vd"], pl.s["cam_R"], pl.s["cam_T"], pl.topo.faces, flip)
    return tuple(x.cpu().numpy() for x in ops.mesh_contact(side, side, md, exclude=pl._exclusion_table(geo)))


def _own_part(pl):
    """1 + the skinning joint of every vertex, restated: a base vertex by its largest weight, a midpoint by the mean of its two ends'"""
    w = np.asarray(pl._skin_weights, np.float64)
    e = pl.topo.edges0.cpu().numpy().astype(np.int64)[:pl.topo.E0]
    return (1 + np.concatenate([w.argmax(1), (0.5 * (w[e[:, 0]] + w[e[:, 1]])).argmax(1)])).astype(np.uint8)


def _host(pl, flip):
    return dict(verts=pl.s["vd"].cpu().numpy(), cam_R=pl.s["cam_R"].cpu().numpy(), cam_T=pl.s["cam_T"].cpu().numpy(), faces=pl.topo.faces.cpu().numpy(),
                flip=flip)


def _near64(view, faces, mask, md, slack):
    """float64, one frame, every vertex: the distance to the nearest face that counts where it is <= md + slack, otherwise +inf.  Exact:
    a face is left out for a vertex only when its centroid is farther than md + slack + the face's radius about the centroid"""
    tri = view[faces.astype(np.int64)]
    c = tri.mean(1)
    R = np.linalg.norm(tri - c[:, None], axis=-1).max(1)
    dmin = np.full(view.shape[0], np.inf)
    for lo in range(0, view.shape[0], 256):
        dc = np.linalg.norm(view[lo:lo + 256, None, :] - c[None], axis=-1)
        i, f = np.nonzero((dc <= md + slack + R[None]) & ~mask[lo:lo + 256])
        np.minimum.at(dmin, lo + i, CR.point_triangle(view[lo + i], tri[f, 0], tri[f, 1], tri[f, 2]))
    return np.where(dmin <= md + slack, dmin, np.inf)


def _against_float64(pl, flip, got, mask, rows_flex):
    """the op's outputs (numpy, the player's last batch) against float64: the near set, the distance and the winding number on every
    vertex, the face on every 64th -> the near vertices that are inside (wind64 > 1.05); rows_flex: FLEX of the batch's rows — the open
    row has no contact, the flexed rows have"""
    h = _host(pl, flip)
    view = CR.view_space(h["verts"], h["cam_R"], h["cam_T"], flip)
    bound = CR.dist_bound(float(np.abs(view).max()))
    d, f, w = got
    deep = 0
    for b, flex in enumerate(rows_flex):
        d64 = _near64(view[b], h["faces"], mask, MD, bound)
        sure_near, sure_far = d64 <= MD - bound, ~(d64 <= MD + bound)
        assert sure_near.any() if flex > 0 else sure_far.all(), ("the flexed rows touch, the open row does not", flex, d64.min())
        assert np.isfinite(d[b][sure_near]).all() and np.isinf(d[b][sure_far]).all(), flex
        near = np.isfinite(d[b])
        assert (np.abs(d[b][near] - d64[near]) <= bound).all(), (flex, np.abs(d[b][near] - d64[near]).max(), bound)
        # the winding number of every near vertex over ALL faces; 6152 terms of a float32 atan2: the bound of tests/test_gpu_contact.py,
        # derived for 320, scaled by the number of terms
        tri = view[b][h["faces"].astype(np.int64)]
        w64 = (-1.0 if flip else 1.0) * (2.0 * CR.half_solid_angle(view[b][near][:, None], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])).sum(-1) / (4.0 * np.pi)
        assert (np.abs(w[b][near] - w64) <= CR.WIND_TOL * 6152 / 320).all(), (flex, np.abs(w[b][near] - w64).max())
        deep += int((w64 > 1.05).sum())
    q = dict(h, verts=h["verts"][:, ::64])
    ref = XR.masked(CR.mesh_contact(q, h), mask[::64])
    for b, flex in enumerate(rows_flex):
        near = np.isfinite(d[b, ::64])
        i = np.nonzero(near)[0]
        assert not mask[::64][i, f[b, ::64][i]].any()
        assert (ref["D"][b, i, f[b, ::64][i]] - ref["d_min"][b, i] <= bound).all(), flex
        werr = np.abs(w[b, ::64][near] - ref["wind_all"][b][near])
        assert (werr <= CR.WIND_TOL * 6152 / 320).all(), (flex, werr.max())
        assert (w[b, ::64][~near] == 0).all() and (f[b, ::64][~near] == -1).all()
    return deep


def test_tables_are_their_definitions(tmp_path_factory):
    from harp_amd.playback.selfcontact import geodesic_exclusion, unpack_exclusion
    hA, _ = _hands(tmp_path_factory)
    pl = _avatar(hA)
    tp = pl.topo
    m = pl.dm
    rest = m.v_template.double().cpu().numpy().reshape(-1, 3) + (m.shapedirs_T.double().cpu().numpy().T @ pl.fit["shape"].double().cpu().numpy()).reshape(-1, 3)
    e = tp.edges0.cpu().numpy().astype(np.int64)
    rest = np.concatenate([rest, 0.5 * (rest[e[:, 0]] + rest[e[:, 1]])])
    assert np.abs(pl._rest_vertices().cpu().numpy() - rest).max() < 1e-7 and rest.shape == (tp.V, 3)
    table = pl._exclusion_table(GEO)
    assert table.dtype == torch.int32 and tuple(table.shape) == (-(-tp.F // 128), tp.V, 4) and table.is_cuda and pl._exclusion_table(GEO) is table
    mask = unpack_exclusion(table, tp.F).cpu().numpy()
    faces = tp.faces.cpu().numpy()
    want = geodesic_exclusion(torch.from_numpy(rest), torch.from_numpy(faces), GEO).numpy()
    assert (mask != want).mean() < 1e-4                                          # (device and host float64 sums may round a path at the radius apart)
    assert mask[faces.reshape(-1), np.repeat(np.arange(tp.F), 3)].all(), "a vertex's own faces are excluded"
    assert 0.05 < mask.mean() < 0.12, mask.mean()
    assert np.array_equal(pl._own_part_table().cpu().numpy(), _own_part(pl))


def test_self_contact_is_the_op_composed(tmp_path_factory):
    from harp_amd.playback import SELF_CONTACT_DIST, SELF_GEODESIC, SelfContact
    from harp_amd.playback.selfcontact import unpack_exclusion
    hA, _ = _hands(tmp_path_factory)
    pl = _avatar(hA)
    V, F, P = pl.topo.V, pl.topo.F, 17
    mask = unpack_exclusion(pl._exclusion_table(GEO), F).cpu().numpy()
    part_table, own = pl._part_table().cpu().numpy(), _own_part(pl)
    deep, rows_of = 0, {}
    for rows in ([0, 1], [2]):                                                  # batch by batch: the player holds the batch's geometry
        c = pl.self_contact(rows, MD, GEO)
        assert isinstance(c, SelfContact)
        got = _np(c)
        n = len(rows)
        op = tuple(x[:n] for x in _op(pl, False, MD, GEO))
        want = XR.compose_self(*op, part_table, own, P)
        for k, (name, dt, shape) in enumerate((("dist", np.float32, (n, V)), ("face", np.int32, (n, V)), ("part", np.uint8, (n, V)),
                                               ("own_part", np.uint8, (V,)), ("wind", np.float32, (n, V)), ("touch", bool, (n, P, P)),
                                               ("min_dist", np.float32, (n,)), ("max_penetration", np.float32, (n,)))):
            assert got[k].dtype == dt and got[k].shape == shape, name
            assert np.array_equal(got[k], want[k]), (name, rows)
        deep += _against_float64(pl, False, op, mask, [FLEX[r] for r in rows])
        for i, r in enumerate(rows):
            rows_of[r] = [g if k == 3 else g[i] for k, g in enumerate(got)]
    assert deep > 0, "the synthetic fist penetrates itself"
    # the open row: nothing; the flexed rows: contact, parts touching, the fist inside itself
    d0, f0, p0, _, w0, t0, m0, x0 = rows_of[0]
    assert np.isposinf(d0).all() and (f0 == -1).all() and not p0.any() and not w0.any() and not t0.any() and np.isposinf(m0) and x0 == 0
    for r in (1, 2):
        d, f, p, _, w, t, m, x = rows_of[r]
        assert np.isfinite(d).any() and t.any() and not t[0].any() and not t[:, 0].any() and abs(m) <= MD
        assert ((p > 0) == (f >= 0)).all()
    assert rows_of[2][7] > 0 and rows_of[2][6] < 0, "penetration in the fist"
    # three rows are two batches, the second padded: the rows are those of the calls one batch at a time
    three = _np(pl.self_contact([0, 1, 2], MD, GEO))
    for r in range(T):
        assert all(np.array_equal(g if k == 3 else g[r], rows_of[r][k]) for k, g in enumerate(three)), r
    # every tensor is new: a later call does not change an earlier result
    first = pl.self_contact([2], MD, GEO)
    keep = _np(first)
    pl.self_contact([0], MD, GEO)
    assert _equal(_np(first), keep)
    # the defaults are the conventions
    assert (SELF_CONTACT_DIST, SELF_GEODESIC) == (0.004, 0.03)
    c = _np(pl.self_contact([1]))
    want = XR.compose_self(*(x[:1] for x in _op(pl, False, SELF_CONTACT_DIST, SELF_GEODESIC)), part_table, own, P)
    assert all(np.array_equal(a, b) for a, b in zip(c, want))


def test_a_mirrored_player(tmp_path_factory):
    from harp_amd.playback import ScenePlayer
    hA, _ = _hands(tmp_path_factory)
    rows = np.arange(T)
    plain = _np(_avatar(hA).self_contact(rows, MD, GEO))
    scene = ScenePlayer(_players((hA,), 1, True), flip=[True])
    scene.load_motions([hA[3]])
    got = scene.self_contact(rows, MD, GEO)
    assert isinstance(got, tuple) and len(got) == 1
    got = _np(got[0])
    for k in (0, 1, 2, 3, 5, 6, 7):                                              # dist, face, part, own_part, touch and the per-frame values
        assert np.array_equal(got[k], plain[k]), k
    # the winding number is negated twice (the mirrored target, the mirrored view): the same up to the order of rounding
    assert np.abs(got[4] - plain[4]).max() <= CR.WIND_TOL * 6152 / 320
    op = _op(scene.players[0], True, MD, GEO)                                    # the buffers hold the last batch: row 2, padded
    assert np.array_equal(got[4][2], op[2][0]) and np.array_equal(got[1][2], op[1][0])


def test_replay_is_eager_and_rows_reverse(tmp_path_factory):
    hA, _ = _hands(tmp_path_factory)
    rows = np.arange(T)
    pl = _avatar(hA, keep_depth=True)
    first = _np(pl.self_contact(rows, MD, GEO))
    assert len(pl._graphs) == 1 and _equal(first, _np(pl.self_contact(rows, MD, GEO))) and len(pl._graphs) == 1
    eager = _avatar(hA, use_graph=False)
    assert _equal(_np(eager.self_contact(rows, MD, GEO)), first) and not eager._graphs
    assert _equal(_np(pl.self_contact(rows[::-1].copy(), MD, GEO)), first, rev=True) and len(pl._graphs) == 1
    part = pl.annotate(rows).part.clone()                                       # a graph key of its own, beside the labels'
    assert len(pl._graphs) == 2 and _equal(_np(pl.self_contact(rows, MD, GEO)), first)
    assert torch.equal(pl.annotate(rows).part, part) and len(pl._graphs) == 2
    pl.self_contact(rows, 0.004, GEO)
    pl.self_contact(rows, MD, 0.05)
    assert len(pl._graphs) == 4 and set(pl._excl) == {GEO, 0.05}


def test_a_scene_of_two_is_each_players_own(tmp_path_factory):
    from harp_amd.playback import ScenePlayer
    hA, hB = _hands(tmp_path_factory)
    rows = np.arange(T)
    own = [_np(_avatar(h).self_contact(rows, MD, GEO)) for h in (hA, hB)]
    scene = ScenePlayer(_players((hA, hB), 1, True), flip=[False, False])
    scene.load_motions([hA[3], hB[3]])
    between = [t.clone() for t in scene.contact(rows).dist]
    assert len(scene._graphs) == 1
    got = scene.self_contact(rows, MD, GEO)
    assert len(got) == 2 and len(scene._graphs) == 2
    for k in range(2):
        assert _equal(_np(got[k]), own[k]), k
    again = scene.contact(rows).dist                                             # the contact pass's graph and buffers are undisturbed
    assert all(torch.equal(a, b) for a, b in zip(again, between)) and len(scene._graphs) == 2


def test_what_self_contact_refuses(tmp_path_factory):
    hA, _ = _hands(tmp_path_factory)
    pl = _avatar(hA)
    for md, geo in ((0.03, 0.03), (0.004, 0.004), (0.01, 0.005), (0.0, 0.0)):
        with pytest.raises(ValueError, match="geodesic"):
            pl.self_contact([0], md, geo)
    for bad in (-0.001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_dist"):
            pl.self_contact([0], bad)
    with pytest.raises(IndexError):
        pl.self_contact([0, T])
    with pytest.raises(ValueError, match="geodesic"):
        pl.play(hA[3], str(tmp_path_factory.mktemp("refused")), self_contacts=True, self_contact_dist=0.05)
    with pytest.raises(RuntimeError, match="load_motion"):
        _players((hA,), 1, False)[0].self_contact([0])


def test_command_line_writes_self_contacts(tmp_path_factory, tmp_path, monkeypatch):
    """python -m harp_amd.playback's main() (the loaders replaced by the synthetic ones, as tests/test_gpu_scene_contact.py does):
    --self-contacts with ONE avatar writes self_contacts.npz with self_contact()'s arrays; with --also ... --contacts both files"""
    import yaml
    from harp_amd import playback
    from harp_amd.playback.player import part_names_of
    from harp_amd.utils import file_utils, hand_model_utils
    hA, hB = _hands(tmp_path_factory)
    by_dir = {h[0]["base_output_dir"]: h for h in (hA, hB)}
    monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda c: (by_dir[c["base_output_dir"]][1], by_dir[c["base_output_dir"]][2]["verts_uvs"],
                                                                         by_dir[c["base_output_dir"]][2]["faces_uvs"], None))
    monkeypatch.setattr(file_utils, "load_result", lambda base, device="cuda", test=False: dict(by_dir[base][2]))
    for name, h in (("a", hA), ("b", hB)):
        with open(tmp_path / f"{name}.yaml", "w") as f:
            yaml.safe_dump({k: h[0][k] for k in ("use_arm", "img_size", "focal_length", "self_shadow", "share_light_position", "base_output_dir")}, f)
        h[3].save(tmp_path / f"{name}.npz")
    base = ["--config", str(tmp_path / "a.yaml"), "--motion", str(tmp_path / "a.npz"), "--batch-size", "2"]
    with pytest.raises(SystemExit, match="--self-geodesic"):
        playback.main(base + ["--out", str(tmp_path / "no"), "--self-contacts", "--self-contact-dist", "0.05"])
    out = tmp_path / "one"
    paths = playback.main(base + ["--out", str(out), "--self-contacts", "--self-contact-dist", str(MD)])
    assert len(paths) == T and (out / "self_contacts.npz").exists() and not (out / "contacts.npz").exists()
    pl = _avatar(hA)
    want = _np(pl.self_contact(np.arange(T), MD))
    V, P = pl.topo.V, 17
    spec = (("dist", np.float32, (T, V)), ("face", np.int32, (T, V)), ("part", np.uint8, (T, V)), ("own_part", np.uint8, (V,)),
            ("wind", np.float32, (T, V)), ("touch", bool, (T, P, P)))
    with np.load(out / "self_contacts.npz") as z:
        assert set(z.files) == {f"{n}_0" for n, _, _ in spec} | {"part_names_0", "min_dist", "max_penetration", "max_dist", "geodesic"}
        for k, (name, dt, shape) in enumerate(spec):
            a = z[f"{name}_0"]
            assert a.shape == shape and a.dtype == dt and np.array_equal(a, want[k]), name
        assert list(z["part_names_0"]) == part_names_of(pl) and len(z["part_names_0"]) == P
        assert z["min_dist"].shape == (T,) and z["min_dist"].dtype == np.float32 and np.array_equal(z["min_dist"], want[6])
        assert z["max_penetration"].shape == (T,) and z["max_penetration"].dtype == np.float32 and np.array_equal(z["max_penetration"], want[7])
        assert z["max_dist"].dtype == np.float32 and float(z["max_dist"]) == np.float32(MD) and float(z["geodesic"]) == np.float32(0.03)
        pinch = z["touch_0"][:, list(z["part_names_0"]).index("thumb3"), list(z["part_names_0"]).index("index3")]
        assert pinch.shape == (T,) and not pinch[0]
    both = tmp_path / "both"
    playback.main(base + ["--out", str(both), "--also", f"{tmp_path / 'b.yaml'}:{tmp_path / 'b.npz'}:flip", "--contacts", "--self-contacts",
                          "--self-contact-dist", str(MD)])
    assert (both / "contacts.npz").exists() and (both / "self_contacts.npz").exists()
    wantB = _np(_avatar(hB).self_contact(np.arange(T), MD))
    with np.load(both / "self_contacts.npz") as z:
        assert {f"{n}_{k}" for n, _, _ in spec for k in (0, 1)} <= set(z.files)
        for k, w in enumerate((want, wantB)):
            for i in (0, 1, 2, 3, 5):                                           # (wind of the flipped player: the order of rounding differs)
                assert np.array_equal(z[f"{spec[i][0]}_{k}"], w[i]), (spec[i][0], k)
        assert np.array_equal(z["wind_0"], want[4])
        assert np.array_equal(z["min_dist"], np.minimum(want[6], wantB[6])) and np.array_equal(z["max_penetration"], np.maximum(want[7], wantB[7]))


def test_the_real_template_at_rest_has_no_contact_at_the_defaults():
    """the conventions on the real 778-vertex template at rest through the op: under SELF_GEODESIC no vertex is within SELF_CONTACT_DIST
    of a counting face (float64: the nearest at 4.56 mm), while 336 are within CONTACT_DIST — against the float64 brute force"""
    import os
    from harp_amd import ops
    from harp_amd.playback import CONTACT_DIST, SELF_CONTACT_DIST, SELF_GEODESIC
    from harp_amd.playback.selfcontact import geodesic_exclusion, pack_exclusion
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with np.load(os.path.join(root, "harp_amd", "assets", "hand_template.npz")) as z:
        verts, faces = z["base_verts"].astype(np.float32), z["faces0"].astype(np.int32)
    cam_R, cam_T = CR.cameras(np.random.default_rng(3), 2)
    h = dict(verts=np.repeat(verts[None], 2, 0), cam_R=cam_R, cam_T=cam_T, faces=faces, flip=False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    side = ops.ContactMesh(t(h["verts"]), t(cam_R), t(cam_T), t(faces), False)
    mask = geodesic_exclusion(t(verts), t(faces), SELF_GEODESIC)
    ref = XR.masked(CR.mesh_contact(h, h), mask.cpu().numpy())
    bound = CR.dist_bound(ref["M"])
    assert ref["d_min"].min() > SELF_CONTACT_DIST + bound and abs(ref["d_min"].min() - 0.00456) < 1e-5
    got = ops.mesh_contact(side, side, SELF_CONTACT_DIST, exclude=pack_exclusion(mask))
    assert torch.isinf(got.dist).all() and (got.face == -1).all() and (got.wind == 0).all()
    got = ops.mesh_contact(side, side, CONTACT_DIST, exclude=pack_exclusion(mask))
    d, w = got.dist.cpu().numpy(), got.wind.cpu().numpy()
    sure = ~CR.undecided(ref, CONTACT_DIST)
    near = np.isfinite(d)
    assert np.array_equal(near[sure], (ref["d_min"] <= CONTACT_DIST)[sure]) and abs(int(near[0].sum()) - 336) <= int((~sure[0]).sum())
    assert (np.abs(d[near] - ref["d_min"][near]) <= bound).all()
    assert (np.abs(w[near] - ref["wind_all"][near]) <= CR.WIND_TOL * len(faces) / 320).all() and (w < 1.0).all()
    assert (ops.mesh_contact(side, side, SELF_CONTACT_DIST).dist == 0).all(), "without the exclusion every vertex touches its own faces"
