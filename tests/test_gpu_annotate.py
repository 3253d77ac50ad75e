"""-m gpu: labelled playback (csrc/annotate.hip, harp_amd/playback/player.py annotate).  harp_annotate_layers against the
float64 restatement of its contract (tests/_annotate_ref.py): owner, part, face, depth and the boxes bit for bit on synthetic layers at
every ss, and owner bit for bit against harp_composite_layers_u8; uv on a small mesh rasterised by harp_rasterize_fwd itself;
harp_keypoint_visibility on seeded joints; the bindings' argument errors; and the players on two synthetic hands at 64 pixels.

Measured on the MI355X (profiles/annotate_errors.txt); each bound below is 4 x the measured value, the project's convention."""
import os

import numpy as np
import pytest
import torch

from tests import _annotate_ref as AR
from tests import test_gpu_scene_player as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
UV_MEASURED, UVZ_MEASURED = 1.652e-7, 1.294e-5          # the largest of each on the MI355X: uv in texture units; pixels / metres at 64 pixels
UV_BOUND, UVZ_BOUND = 4 * UV_MEASURED, 4 * UVZ_MEASURED
UNDECIDABLE_CAP = 0.02


def _dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_layers(layers):
    return [{k: (v if k == "flip" else _dv(v)) for k, v in l.items()} for l in layers]


def _record(line):
    """a figure the run measured, printed before anything is asserted on it (pytest -s shows it: profiles/annotate_errors.txt)"""
    print(line)


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_exact_maps_against_float64_and_the_composite(ss):
    from harp_amd import ops
    rng = np.random.default_rng(320 + ss)
    S, B = 9, 3                                            # 243 pixels: four waves, the last one partial, waves that straddle two frames
    seen_owner, labelled = set(), 0
    for L in (1, 2, 4):
        for kind in ("none", "one", "per_row", "rows"):
            lay = AR.label_case(rng, L, B, S, ss)
            flips = [False, True, True, False][:L] if kind in ("none", "rows") else [bool(f) for f in rng.integers(0, 2, size=L)]
            for l, f in zip(lay, flips):
                l["flip"] = f
            sz, rows = AR.scene_case(rng, kind, B, S)
            ref = AR.annotate_layers(lay, ss, sz, rows)
            dev = _dev_layers(lay)
            got = ops.annotate_layers(dev, ss, _dv(sz), _dv(rows))
            what = (ss, L, kind, flips)
            assert got.uv is None and got.owner.dtype == torch.uint8 and got.part.dtype == torch.uint8 and got.face.dtype == torch.int32
            assert np.array_equal(got.owner.cpu().numpy(), ref["owner"]), what
            assert np.array_equal(got.part.cpu().numpy(), ref["part"]), what
            assert np.array_equal(got.face.cpu().numpy(), ref["face"]), what
            assert np.array_equal(got.depth.cpu().numpy().astype(np.float64), ref["depth"]), what      # (a float32 depth, copied)
            assert np.array_equal(got.bbox.cpu().numpy(), ref["bbox"]), what
            # THE test of the feature: the owner of the labels is the owner of the frames, bit for bit
            rgb = torch.zeros(B, S * ss, S * ss, 3, device=DEV)
            _, own = ops.composite_layers_u8([(rgb, d["zbuf"], d["flip"]) for d in dev], ss, _dv(sz), _dv(rows), owner=True)
            assert torch.equal(got.owner, own), what
            # outputs are independent: one alone gives the same bits
            alone = ops.annotate_layers(dev, ss, _dv(sz), _dv(rows), owner=False, depth=False, face=False, bbox=False)
            assert alone.owner is None and alone.bbox is None and torch.equal(alone.part, got.part)
            seen_owner |= set(np.unique(ref["owner"]).tolist())
            labelled += int(((ref["part"] > 0) & (ref["owner"] > 0)).sum())
    assert seen_owner == {0, 1, 2, 3, 4} and labelled > 100


def _uv_mesh(rng, B):
    """a 3 x 3 grid of vertices as 8 triangles, every vertex at its own depth, tilted differently per frame; every face has its own three
    rows of verts_uvs (seams everywhere)"""
    g = np.linspace(-0.75, 0.75, 3)
    xy = np.stack(np.meshgrid(g, g, indexing="xy"), -1).reshape(9, 2)
    ndc = np.zeros((B, 9, 3), np.float32)
    for b in range(B):
        ndc[b, :, :2] = xy + rng.uniform(-0.08, 0.08, size=(9, 2))
        ndc[b, :, 2] = rng.uniform(0.4, 0.9, size=9)
    faces = []
    for r in range(2):
        for c in range(2):
            a = 3 * r + c
            faces += [[a, a + 1, a + 4], [a, a + 4, a + 3]]
    faces = np.array(faces, np.int32)
    return ndc, faces, rng.uniform(0.0, 1.0, size=(24, 2)).astype(np.float32), rng.permutation(24).reshape(8, 3).astype(np.int32)


@pytest.mark.parametrize("ss", [1, 2])
def test_uv_against_float64(ss):
    from harp_amd import ops
    rng = np.random.default_rng(410 + ss)
    S, B = 16, 2
    Sh = S * ss
    lay = []
    for flip in (False, True):
        ndc, faces, vuv, fuv = _uv_mesh(rng, B)
        ndc[..., :2] *= 0.8 if flip else 1.0               # the second mesh is smaller: both show, and they interleave in depth
        fid, zbuf, _, _ = ops.rasterize_fwd(_dv(ndc), _dv(faces), Sh)
        lab = rng.integers(1, 4, size=8).astype(np.uint8)
        lay.append(dict(face_id=fid.cpu().numpy(), zbuf=zbuf.cpu().numpy(), face_label=lab, flip=flip, ndc=ndc, faces=faces, verts_uvs=vuv, faces_uvs=fuv))
    ref = AR.annotate_layers(lay, ss, uv=True)              # (the device's own face ids: no pixel is undecidable)
    got = ops.annotate_layers(_dev_layers(lay), ss, uv=True)
    for k in ("owner", "part", "face"):
        assert np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), k
    assert {1, 2} <= set(np.unique(ref["owner"]).tolist()) and (ref["owner"] > 0).mean() > 0.3
    uv = got.uv.cpu().numpy().astype(np.float64)
    assert not uv[ref["owner"] == 0].any()
    err = float(np.abs(uv - ref["uv"]).max())
    inside = ref["uv"][ref["owner"] > 0]
    _record(f"[annotate uv] ss={ss}: largest |uv - float64| = {err:.3e} over {int((ref['owner'] > 0).sum())} pixels (bound {UV_BOUND:.3e}); uv spans "
            f"[{inside.min():.3f}, {inside.max():.3f}]")
    assert err <= UV_BOUND


@pytest.mark.parametrize("ss", [1, 2])
def test_keypoint_visibility_against_float64(ss):
    from harp_amd import ops
    c = AR.keypoint_case(ss)
    layers = [dict(zbuf=_dv(z), flip=f) for z, f in zip(c["zs"], AR.KP_FLIPS)]
    skipped = total = 0
    for self_layer in (0, 1):                              # (layer 1 is flipped)
        ref = AR.keypoint_visibility(c["joints"], c["R"], c["T"], AR.KP_FOCAL, AR.KP_S, ss, self_layer, c["zs"], AR.KP_FLIPS, c["scene_z"], None, 0.02)
        got = ops.keypoint_visibility(_dv(c["joints"]), _dv(c["R"]), _dv(c["T"]), AR.KP_FOCAL, AR.KP_S, layers, self_layer=self_layer, ss=ss,
                                      scene_depth=_dv(c["scene_z"]), tol=0.02)
        uvz, vis = got.uvz.cpu().numpy().astype(np.float64), got.vis.cpu().numpy()
        err = float(np.abs(uvz - ref["uvz"]).max())
        _record(f"[keypoints] ss={ss} self_layer={self_layer}: largest |(u, v, Z) - float64| = {err:.3e} (bound {UVZ_BOUND:.3e}); "
                f"{int((~ref['decidable']).sum())} of {ref['decidable'].size} joints undecidable")
        assert err <= UVZ_BOUND
        assert not uvz[:, 7].any() and not vis[:, 7].any() and not vis[:, 3].any()          # behind the camera; outside the image
        ok = ref["decidable"]
        assert np.array_equal(vis[ok], ref["vis"][ok]), (ss, self_layer)
        skipped, total = skipped + int((~ok).sum()), total + ok.size
    assert skipped <= UNDECIDABLE_CAP * total              # (tests/test_annotate_cpu.py proves it for these inputs, and that every case occurs)


def test_binding_checks():
    from harp_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)      # noqa: E731
    lay = lambda **kw: dict(dict(face_id=z(3, 8, 8, dt=torch.int32), zbuf=z(3, 8, 8), face_label=torch.ones(5, dtype=torch.uint8, device=DEV), flip=False), **kw)      # noqa: E731
    uvk = dict(ndc=z(3, 7, 3), faces=z(5, 3, dt=torch.int32), verts_uvs=z(9, 2), faces_uvs=z(5, 3, dt=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.annotate_layers([lay(zbuf=torch.zeros(3, 8, 8))], 2)
    for bad, exc in [([], ValueError), ([lay()] * 5, ValueError), ([lay(extra=1)], ValueError), ([lay(), lay(zbuf=z(3, 8, 4))], ValueError),
                     ([lay(zbuf=z(3, 8, 8, dt=torch.float64))], TypeError), ([lay(face_id=z(3, 8, 8))], TypeError),
                     ([lay(face_id=z(3, 4, 4, dt=torch.int32))], ValueError), ([lay(face_label=z(5))], TypeError),
                     ([lay(face_label=torch.ones(5, 1, dtype=torch.uint8, device=DEV))], ValueError)]:
        with pytest.raises(exc):
            ops.annotate_layers(bad, 2)
    with pytest.raises(ValueError):
        ops.annotate_layers([lay()], 5)
    with pytest.raises(TypeError):
        ops.annotate_layers([lay()], 3)                                                   # 8 is no multiple of 3
    with pytest.raises(ValueError):
        ops.annotate_layers([lay()], 2, scene_depth=z(2, 4, 4))                           # 2 depths for 3 frames
    with pytest.raises(TypeError):
        ops.annotate_layers([lay()], 2, scene_depth=z(3, 8, 8))                           # supersampled, not output resolution
    with pytest.raises(ValueError):
        ops.annotate_layers([lay()], 2, scene_rows=z(3, dt=torch.int32))
    with pytest.raises(ValueError):
        ops.annotate_layers([lay()], 2, owner=False, part=False, depth=False, face=False, bbox=False)
    with pytest.raises(ValueError):
        ops.annotate_layers([lay()], 2, uv=True)                                          # uv without its tables
    for k, v, exc in [("ndc", z(2, 7, 3), ValueError), ("ndc", z(3, 7, 3, dt=torch.float64), TypeError), ("faces", z(4, 3, dt=torch.int32), ValueError),
                      ("faces_uvs", z(5, 3), TypeError), ("verts_uvs", z(9, 3), ValueError)]:
        with pytest.raises(exc):
            ops.annotate_layers([lay(**dict(uvk, **{k: v}))], 2, uv=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.annotate_layers([lay(zbuf=z(3, 8, 8).requires_grad_())], 2)
    out = ops.annotate_layers([lay(**uvk)], 2, scene_depth=z(1, 4, 4), uv=True)
    assert tuple(out.uv.shape) == (3, 4, 4, 2) and not out.owner.any() and (out.face == -1).all() and (out.bbox == -1).all() and tuple(out.bbox.shape) == (3, 1, 4)
    # keypoint_visibility
    j, R, T = z(3, 21, 3), z(3, 9), z(3, 3)
    kp = lambda **kw: ops.keypoint_visibility(**dict(dict(joints=j, cam_R=R, cam_T=T, focal=50.0, S=4, layers=[lay()], ss=2), **kw))      # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU path"):
        kp(joints=j.cpu())
    for kw, exc in [(dict(joints=z(2, 21, 3)), ValueError), (dict(joints=z(3, 21, 3, dt=torch.float64)), TypeError), (dict(cam_R=z(3, 3, 3)), ValueError),
                    (dict(cam_T=z(3, 4)), ValueError), (dict(S=8), ValueError), (dict(ss=5), ValueError), (dict(self_layer=1), ValueError),
                    (dict(self_layer=-1), ValueError), (dict(focal=0.0), ValueError), (dict(tol=-1.0), ValueError), (dict(tol=float("nan")), ValueError),
                    (dict(layers=[]), ValueError), (dict(layers=[lay(zbuf=z(3, 8, 8, dt=torch.float64))]), TypeError),
                    (dict(scene_depth=z(2, 4, 4)), ValueError), (dict(scene_depth=z(1, 8, 8)), TypeError)]:
        with pytest.raises(exc):
            kp(**kw)
    out = kp(layers=[dict(zbuf=z(3, 8, 8), flip=True)])
    assert tuple(out.uvz.shape) == (3, 21, 3) and tuple(out.vis.shape) == (3, 21, 2) and not out.vis.any() and not out.uvz.any()      # Z = 0


# ---- the players: the synthetic fits of tests/test_gpu_scene_player.py at 64 pixels ---------------------------------------------------
S64 = 64


@pytest.fixture(scope="module")
def hands(tmp_path_factory):
    """sp._two_hands at img_size 64 with a cache of its own (the scene player's tests keep theirs at 32)"""
    old = sp.S, sp._HANDS
    sp.S, sp._HANDS = S64, {}
    try:
        return sp._two_hands(tmp_path_factory)
    finally:
        sp.S, sp._HANDS = old


@pytest.mark.parametrize("ss,use_graph", [(1, True), (1, False), (2, True), (2, False)])
def test_players(hands, ss, use_graph, tmp_path, monkeypatch):
    from PIL import Image
    from harp_amd import playback
    from harp_amd.playback import ScenePlayer, load_scene_depth, project_pixels
    hA, hB, bg = hands
    T, rows = sp.T, np.arange(sp.T)
    focal = float(hA[0]["focal_length"])
    players = sp._players((hA, hB), ss, True, use_graph=use_graph)
    scene = ScenePlayer(players, flip=[False, True])
    scene.load_motions([hA[3], hB[3]])
    # before annotate was ever called on these players: the parent's bytes
    before, own_before = (t.clone() for t in scene.render(rows, background=bg, alpha=True, owner=True))
    alone_before = players[0].render(rows, background=bg).clone()
    a = scene.annotate(rows, uv=True)
    owner, part, face, depth, bbox = (getattr(a, k).cpu().numpy() for k in ("owner", "part", "face", "depth", "bbox"))
    assert np.array_equal(owner, own_before.cpu().numpy()) and {0, 1, 2} <= set(np.unique(owner).tolist())
    # every labelled pixel's face carries its part in the owner's table
    for k, pl in enumerate(players):
        tab = pl._part_table().cpu().numpy()
        m = owner == k + 1
        assert m.any() and (face[m] >= 0).all() and np.array_equal(tab[face[m]], part[m]) and part[m].min() >= 1 and part[m].max() <= 16
        assert (depth[m] > 0).all()
    assert not part[owner == 0].any() and (face[owner == 0] == -1).all() and not depth[owner == 0].any()
    # the boxes: the extent of the owner map, with torch
    own_t = a.owner
    for b in range(T):
        for k in range(2):
            ys, xs = torch.nonzero(own_t[b] == k + 1, as_tuple=True)
            want = [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if ys.numel() else [-1] * 4
            assert bbox[b, k].tolist() == want, (b, k)
    uv = a.uv.cpu().numpy()
    assert uv[owner > 0].min() >= -1e-3 and uv[owner > 0].max() <= 1 + 1e-3 and not uv[owner == 0].any()
    # render without labels: what it was before annotate, and the replay after it
    after, own_after = scene.render(rows, background=bg, alpha=True, owner=True)
    assert torch.equal(after, before) and torch.equal(own_after, own_before)
    assert torch.equal(players[0].render(rows, background=bg), alone_before)
    assert torch.equal(scene.annotate(rows, uv=True).part, torch.from_numpy(part).to(DEV))      # (a replay)
    assert len(scene._graphs) == (2 if use_graph else 0)
    # the single player: its owner is its coverage, its labels the scene's where it is not hidden
    one = players[0].annotate(rows)
    assert one.uv is None and tuple(one.bbox.shape) == (T, 4) and tuple(one.uvz.shape) == (T, 21, 3)
    cov = players[0].render(rows, alpha=True)[..., 3] > 0
    assert torch.equal(one.owner > 0, cov)
    shown = torch.from_numpy(owner == 1).to(DEV)
    assert torch.equal(one.part[shown], torch.from_numpy(part).to(DEV)[shown])
    with pytest.raises(ValueError, match="keep_depth"):
        sp._players((hA,), ss, False, use_graph=False)[0].annotate([0])
    # the files of play(labels=True)
    out = tmp_path / "frames"
    scene.play([hA[3], hB[3]], str(out), backgrounds=bg, fmt="png", labels=True)
    names = sorted(os.listdir(out))
    assert names == sorted(["%04d.png" % i for i in range(T)] + [f"{k}_%04d.png" % i for i in range(T) for k in ("part", "depth", "iuv")] +
                           ["keypoints_0.npz", "keypoints_1.npz"])
    for i in (0, T - 1):
        assert np.array_equal(np.asarray(Image.open(out / ("part_%04d.png" % i))), part[i])
        iuv = np.asarray(Image.open(out / ("iuv_%04d.png" % i)))
        assert iuv.shape == (S64, S64, 3) and np.array_equal(iuv[..., 0], part[i])
        assert np.array_equal(iuv[..., 1:], np.clip(np.floor(255.0 * uv[i].astype(np.float64) + 0.5), 0, 255).astype(np.uint8))
    (tmp_path / "depth").mkdir()
    for i in range(T):
        os.rename(out / ("depth_%04d.png" % i), tmp_path / "depth" / ("depth_%04d.png" % i))
    back = load_scene_depth(str(tmp_path / "depth"), S64, DEV).cpu().numpy()
    assert np.abs(back.astype(np.float64) - depth).max() <= 0.5e-3 + 1e-7 and (back[owner == 0] == 0).all()      # (1e-7: the float32 of k / 1000)
    # keypoints.npz against project_pixels of the players' own joints
    worst = 0.0
    for k, (pl, h, flip) in enumerate(zip(players, (hA, hB), (False, True))):
        z = np.load(out / f"keypoints_{k}.npz")
        assert z["keypoints"].shape == (T, 21, 2) and z["weights"].shape == (T, 21) and z["bbox"].shape == (T, 4) and len(z["part_names"]) == 17
        assert np.array_equal(z["bbox"], bbox[:, k]) and np.array_equal(z["weights"], (z["visible"] == 2).astype(np.float32))
        assert set(np.unique(z["occluder"]).tolist()) <= {0, 1, 2} and z["visible"].min() >= 0 and z["visible"].max() <= 2
        eager = sp._players((h,), ss, True, use_graph=False)[0]
        eager.load_motion(h[3])
        for lo in range(0, T, sp.BATCH):
            r = np.arange(lo, min(T, lo + sp.BATCH))
            eager.annotate(r, parts=False, depth=False)
            j = eager.s["joints_m"][:len(r)].cpu().numpy()
            want = project_pixels(j, h[3].cam[r].cpu().numpy(), focal, S64)
            if flip:
                want[..., 0] = S64 - want[..., 0]
            worst = max(worst, float(np.abs(z["keypoints"][r] - want[..., :2]).max()), float(np.abs(z["depth"][r] - want[..., 2]).max()))
    _record(f"[players] ss={ss} graph={use_graph}: keypoints.npz against project_pixels: largest difference {worst:.3e} (bound {UVZ_BOUND:.3e})")
    assert worst <= UVZ_BOUND
    # the far hand B never hides a joint of the near hand A
    zA, zB = np.load(out / "keypoints_0.npz"), np.load(out / "keypoints_1.npz")
    print(f"[players] ss={ss}: visible joints A {(zA['visible'] == 2).mean():.0%}, B {(zB['visible'] == 2).mean():.0%}; B hidden by A {(zB['occluder'] == 1).mean():.0%}")
    assert not (zA["occluder"] == 2).any()
    if ss == 1 and use_graph:
        # the file of a hand is what --keypoints2d reads: the command line end to end on it
        import yaml
        from harp_amd.utils import file_utils, hand_model_utils
        monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda c: (hA[1], hA[2]["verts_uvs"], hA[2]["faces_uvs"], None))
        monkeypatch.setattr(file_utils, "load_result", lambda base, device="cuda", test=False: dict(hA[2]))
        with open(tmp_path / "a.yaml", "w") as f:
            yaml.safe_dump({k: hA[0][k] for k in ("use_arm", "img_size", "focal_length", "self_shadow", "share_light_position", "base_output_dir")}, f)
        paths = playback.main(["--config", str(tmp_path / "a.yaml"), "--keypoints2d", str(out / "keypoints_0.npz"), "--out", str(tmp_path / "again"),
                               "--labels", "--batch-size", "4"])
        assert len(paths) == T and os.path.exists(tmp_path / "again" / "keypoints.npz") and os.path.exists(tmp_path / "again" / "part_0000.png")
        z2 = np.load(tmp_path / "again" / "keypoints.npz")
        seen = zA["weights"] > 0
        print(f"[players] --keypoints2d on the written file: the joints it saw come back within {np.abs(z2['keypoints'] - zA['keypoints'])[seen].max():.3f} px")
        assert z2["keypoints"].shape == (T, 21, 2) and np.isfinite(z2["keypoints"]).all()
