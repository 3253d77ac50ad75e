"""-m gpu: several avatars in one frame (csrc/composite.hip, harp_amd/playback/player.py ScenePlayer).  harp_composite_layers_u8
against the float64 restatement of its contract (tests/_layers_ref.py) at its edges and byte for byte against harp_resolve_u8 where the
two contracts coincide; ScenePlayer on two synthetic hands — exact at ss = 1, where a pixel is one sample: every pixel of the scene is
the nearer avatar's, the other's mirrored, or the background's — with a scene depth between, in front of and absent; at ss = 2 against the
yardstick fed with the players' own buffers; graph = eager, replay, reversed rows; and the command line end to end."""
import itertools
import os

import numpy as np
import pytest
import torch

from tests import _layers_ref as LR
from tests.test_gpu_evaluate import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _layers(rng, L, B, Sh):
    """rgb uniform in [-0.1, 1.1] with 2 % NaN; depths uniform in [0.2, 1.0] with ~40 % holes of -1 and a sprinkle of 0, NaN and +inf; on
    10 % of the sub-samples one layer's depth is copied into another (half at the same place, half at the mirrored one, so that exact ties
    occur between layers of equal and of different flip)"""
    out = []
    for _ in range(L):
        rgb = rng.uniform(-0.1, 1.1, size=(B, Sh, Sh, 3)).astype(np.float32)
        rgb.reshape(-1)[rng.integers(0, rgb.size, size=max(1, rgb.size // 50))] = np.nan
        z = rng.uniform(0.2, 1.0, size=(B, Sh, Sh)).astype(np.float32)
        z[rng.uniform(size=z.shape) < 0.4] = -1.0
        for v in (0.0, np.nan, np.inf):
            z.reshape(-1)[rng.integers(0, z.size, size=max(1, z.size // 100))] = v
        out.append([rgb, z])
    for l in range(1, L):
        src = out[rng.integers(0, l)][1]
        same, mirrored = rng.uniform(size=src.shape) < 0.05, rng.uniform(size=src.shape) < 0.05
        out[l][1] = np.where(same, src, np.where(mirrored, src[:, :, ::-1], out[l][1])).astype(np.float32)
    return out


def _check_exactness(got, own, ref, channels, what):
    """test 4's rule: alpha, owner and pixels with n == 0 bit-exact; a colour further than 0.01 from a rounding boundary exact, the others
    within one level -> (undecided values, values)"""
    assert got.shape == ref["out"].shape and got.dtype == np.uint8, what
    if channels == 4:
        assert np.array_equal(got[..., 3], ref["out"][..., 3]), ("alpha is the integer formula, bit for bit", what)
    if own is not None:
        assert np.array_equal(own, ref["owner"]), ("owner", what)
    empty = ref["n"] == 0
    assert np.array_equal(got[..., :3][empty], ref["out"][..., :3][empty]), ("an uncovered pixel is the background byte", what)
    dist = np.abs(ref["v255"] - np.floor(ref["v255"]) - 0.5)               # to the nearest rounding boundary k + 0.5
    decided = (dist > 0.01) | empty[..., None]
    d = np.abs(got[..., :3].astype(np.int64) - ref["out"][..., :3].astype(np.int64))
    assert (d[decided] == 0).all(), (what, int(d[decided].max()))
    assert d.max() <= 1, what
    return int((~decided).sum()), decided.size


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_composite_against_float64(ss):
    from harp_amd import ops
    rng = np.random.default_rng(140 + ss)
    undecided = total = n_cases = 0
    for S in (1, 7, 16, 33):
        for B in (1, 3):
            Sh = S * ss
            data = _layers(rng, 4, B, Sh)
            dev = [(_dv(c), _dv(z)) for c, z in data]
            for L in (1, 2, 4):
                flips = list(itertools.product((False, True), repeat=L)) if L <= 2 else [tuple(bool(f) for f in rng.integers(0, 2, size=4))]
                for flip in flips:
                    for depth in ("none", "one", "per_row", "rows"):
                        n_sc = {"none": 0, "one": 1, "per_row": B, "rows": 4}[depth]
                        sz = None
                        if n_sc:
                            sz = rng.uniform(0.2, 1.0, size=(n_sc, S, S)).astype(np.float32)
                            sz[rng.uniform(size=sz.shape) < 0.2] = 0.0
                            sz.reshape(-1)[rng.integers(0, sz.size, size=max(1, sz.size // 50))] = np.nan
                        srows = None
                        if depth == "rows":
                            srows = rng.integers(0, 4, size=B).astype(np.int32)
                            srows[rng.integers(0, B)] = [-1, 4][n_cases % 2]          # one entry out of range: no scene depth
                        for bgk in ("color", "one", "per_row", "rows"):
                            n_bg = {"color": 0, "one": 1, "per_row": B, "rows": 4}[bgk]
                            bg = rng.integers(0, 256, size=(n_bg, S, S, 3)).astype(np.uint8) if n_bg else None
                            rows = None
                            if bgk == "rows":
                                rows = rng.integers(0, 4, size=B).astype(np.int32)
                                rows[rng.integers(0, B)] = [-1, 4][(n_cases // 2) % 2]   # one entry out of range: the constant colour
                            color = rng.uniform(0.0, 1.0, size=3).astype(np.float32)
                            for channels in (3, 4):
                                got, own = ops.composite_layers_u8([(dev[l][0], dev[l][1], flip[l]) for l in range(L)], ss, _dv(sz), _dv(srows), _dv(bg),
                                                                   _dv(rows), _dv(color), alpha=channels == 4, owner=True)
                                ref = LR.composite_layers([(data[l][0], data[l][1], flip[l]) for l in range(L)], ss, sz, srows, bg, rows, color, channels)
                                u, t = _check_exactness(got.cpu().numpy(), own.cpu().numpy(), ref, channels, (S, B, L, flip, depth, bgk, channels))
                                undecided, total, n_cases = undecided + u, total + t, n_cases + 1
    share = undecided / total
    print(f"[composite_layers_u8] ss={ss}: {n_cases} cases, {undecided} of {total} colour values ({share:.2%}) within 0.01 of a rounding boundary (one level allowed there)")
    assert share <= 0.05


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_composite_is_the_resolve_for_one_layer_and_a_flip_is_a_mirror(ss):
    from harp_amd import ops
    rng = np.random.default_rng(240 + ss)
    S, B = 33, 3
    Sh = S * ss
    rgb = rng.uniform(-0.1, 1.1, size=(B, Sh, Sh, 3)).astype(np.float32)
    rgb.reshape(-1)[rng.integers(0, rgb.size, size=rgb.size // 50)] = np.nan
    fid = np.where(rng.uniform(size=(B, Sh, Sh)) < 0.6, rng.integers(0, 5000, size=(B, Sh, Sh)), -1).astype(np.int32)
    z = np.where(fid >= 0, 1.0, -1.0).astype(np.float32)
    rgb_d, fid_d, z_d = _dv(rgb), _dv(fid), _dv(z)
    bg4 = _dv(rng.integers(0, 256, size=(4, S, S, 3)).astype(np.uint8))
    color = _dv(rng.uniform(0, 1, size=3).astype(np.float32))
    kinds = [dict(), dict(background=bg4[:1]), dict(background=bg4[:B]), dict(background=bg4, bg_rows=_dv(np.array([3, -1, 0], np.int32)))]
    (c1, z1), = [(_dv(c), _dv(zz)) for c, zz in _layers(rng, 1, B, Sh)]
    sz = _dv(rng.uniform(0.2, 1.0, size=(B, S, S)).astype(np.float32))
    for kw in kinds:
        for alpha in (False, True):
            want = ops.resolve_u8(rgb_d, fid_d, ss, bg_color=color, alpha=alpha, **kw)
            got, own = ops.composite_layers_u8([(rgb_d, z_d, False)], ss, bg_color=color, alpha=alpha, owner=True, **kw)
            assert torch.equal(got, want), (ss, sorted(kw), alpha)
            assert torch.equal(own, (want[..., 3] > 0).to(torch.uint8)) if alpha else True
            # a flipped layer = the same call on arrays mirrored beforehand (under another, unflipped layer and a scene depth)
            a = ops.composite_layers_u8([(c1, z1, False), (rgb_d, z_d, True)], ss, scene_depth=sz, bg_color=color, alpha=alpha, owner=True, **kw)
            b = ops.composite_layers_u8([(c1, z1, False), (torch.flip(rgb_d, dims=[2]).contiguous(), torch.flip(z_d, dims=[2]).contiguous(), False)],
                                        ss, scene_depth=sz, bg_color=color, alpha=alpha, owner=True, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (ss, sorted(kw), alpha)
            assert not torch.equal(a[0], got)


def test_composite_binding_checks():
    from harp_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    rgb, zb = z(3, 8, 8, 3), z(3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.composite_layers_u8([(rgb.cpu(), zb.cpu(), False)], 2)
    with pytest.raises(ValueError):
        ops.composite_layers_u8([], 2)
    with pytest.raises(ValueError):
        ops.composite_layers_u8([(rgb, zb, False)] * 5, 2)
    with pytest.raises(ValueError):
        ops.composite_layers_u8([(rgb, zb, False), (rgb, z(3, 8, 4), False)], 2)
    with pytest.raises(ValueError):
        ops.composite_layers_u8([(rgb, zb, False), (z(2, 8, 8, 3), z(2, 8, 8), True)], 2)
    with pytest.raises(TypeError):
        ops.composite_layers_u8([(rgb, zb.to(torch.int32), False)], 2)
    with pytest.raises(ValueError):
        ops.composite_layers_u8([(rgb, zb, False)], 5)
    with pytest.raises(ValueError):
        ops.composite_layers_u8([(rgb, zb, False)], 2, scene_depth=z(2, 4, 4))          # 2 depths for 3 frames
    with pytest.raises(TypeError):
        ops.composite_layers_u8([(rgb, zb, False)], 2, scene_depth=z(3, 8, 8))          # supersampled, not output resolution
    with pytest.raises(ValueError):
        ops.composite_layers_u8([(rgb, zb, False)], 2, background=z(2, 4, 4, 3, dt=torch.uint8))
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.composite_layers_u8([(rgb.clone().requires_grad_(), zb, False)], 2)
    out = ops.composite_layers_u8([(rgb, zb, False)], 2, scene_depth=z(1, 4, 4), alpha=True)
    assert tuple(out.shape) == (3, 4, 4, 4) and not out[..., 3].any() and (out[..., :3] == 255).all()


# ---- two hands -------------------------------------------------------------------------------------------------------------------
S, T, BATCH = 32, 5, 2
# the second hand's motion: cam[:, 0] (the weak-perspective scale: depth = 2 focal / (S scale)) scaled down, so it is 1 / B_SCALE times
# as far away — wholly behind the first hand, whose depth spans 0.88 .. 1.24 over the five frames while the second's starts at
# 0.81 / B_SCALE = 1.47 (test_scene_depth_ss1_exact asserts the gap) — and
# cam[:, 1] shifted by B_SHIFT_PX pixels at its depth, so that the mirrored silhouette overlaps the first hand's partly
B_SCALE, B_SHIFT_PX = 0.55, 6.0
_HANDS = {}


def _two_hands(tmp_path_factory, scale=B_SCALE, shift_px=B_SHIFT_PX):
    """two synthetic fits with their motions (cfg, layer, params, motion) and T random backgrounds, built once"""
    from harp_amd.playback import Motion
    if "fits" not in _HANDS:
        fits = []
        for seed in (31, 57):
            tmp = tmp_path_factory.mktemp(f"scene_hand_{seed}")
            _, cfg, layer, params, _ = _setup(T, S, seed, tmp, self_shadow=True, share_light_position=True)
            fits.append((cfg, layer, params))
        g = torch.Generator().manual_seed(78)
        _HANDS["fits"] = fits
        _HANDS["bg"] = torch.randint(0, 256, (T, S, S, 3), generator=g, dtype=torch.uint8).to(DEV)
    (cfgA, layerA, paramsA), (cfgB, layerB, paramsB) = _HANDS["fits"]
    assert cfgA["focal_length"] == cfgB["focal_length"]    # one camera
    mA, mB = Motion.from_params(paramsA), Motion.from_params(paramsB)
    cam = mB.cam.clone()
    cam[:, 0] *= scale
    cam[:, 1] += shift_px * 2.0 / (S * cam[:, 0])            # (a pixel is 2 / (S scale) model units wide)
    mB.cam = cam.contiguous()
    return (cfgA, layerA, paramsA, mA), (cfgB, layerB, paramsB, mB), _HANDS["bg"]


def _players(hands, ss, keep_depth, use_graph=True):
    from harp_amd.playback import AvatarPlayer
    ps = [AvatarPlayer(cfg, params, layer, batch_size=BATCH, ss=ss, use_graph=use_graph, device=DEV, keep_depth=keep_depth) for cfg, layer, params, _ in hands]
    return ps


def _eager_buffers(hands, ss, bg):
    """the players' own buffers, batch by batch (they hold the last batch only): per hand rgb, z_c, face_c of all T frames, as numpy"""
    ps = _players(hands, ss, True, use_graph=False)
    out = []
    for p, h in zip(ps, hands):
        p.load_motion(h[3])
        parts = {"rgb": [], "z_c": [], "face_c": []}
        for lo in range(0, T, BATCH):
            rows = np.arange(lo, min(T, lo + BATCH))
            p.render(rows, background=bg[rows])
            for k in parts:
                parts[k].append(p.s[k][:len(rows)].cpu().numpy().copy())
        out.append({k: np.concatenate(v) for k, v in parts.items()})
    return out


def _scene_ss1(tmp_path_factory, scale=B_SCALE, shift_px=B_SHIFT_PX):
    """everything tests 6 and 7 share, rendered once"""
    from harp_amd.playback import ScenePlayer
    key = ("ss1", scale, shift_px)
    if key not in _HANDS:
        hA, hB, bg = _two_hands(tmp_path_factory, scale, shift_px)
        rows = np.arange(T)
        alone = []
        for p, h in zip(_players((hA, hB), 1, False), (hA, hB)):
            p.load_motion(h[3])
            alone.append(p.render(rows, background=bg, alpha=True).cpu().numpy().copy())
        scene = ScenePlayer(_players((hA, hB), 1, True), flip=[False, True])
        scene.load_motions([hA[3], hB[3]])
        frames, owner = scene.render(rows, background=bg, alpha=True, owner=True)
        _HANDS[key] = dict(hands=(hA, hB), bg=bg, A=alone[0], Bm=alone[1][:, :, ::-1], scene=scene, frames=frames.cpu().numpy().copy(),
                           owner=owner.cpu().numpy().copy(), buf=_eager_buffers((hA, hB), 1, bg))
    return _HANDS[key]


def test_two_hands_ss1_exact(tmp_path_factory):
    r = _scene_ss1(tmp_path_factory)
    A, Bm, frames, owner, bg = r["A"], r["Bm"], r["frames"], r["owner"], r["bg"].cpu().numpy()
    covA, covB = A[..., 3] > 0, Bm[..., 3] > 0
    assert set(np.unique(A[..., 3])) <= {0, 255} and set(np.unique(Bm[..., 3])) <= {0, 255}
    print(f"[two hands] owned by A {int((owner == 1).sum())}, by B {int((owner == 2).sum())}, both covered {int((covA & covB).sum())}")
    assert (owner == 1).sum() >= 20 and (owner == 2).sum() >= 20 and (covA & covB).sum() >= 20, "the scene must show both hands, overlapping"
    assert np.array_equal(frames[..., :3][owner == 1], A[..., :3][owner == 1])
    assert np.array_equal(frames[..., :3][owner == 2], Bm[..., :3][owner == 2])
    assert np.array_equal(frames[..., :3][owner == 0], bg[owner == 0])
    assert np.array_equal(owner == 0, ~covA & ~covB)
    assert (owner[covA & covB] == 1).all(), "where both are covered the nearer hand, A, shows"
    assert np.array_equal(frames[..., 3], np.where(owner > 0, 255, 0))
    # the players' own depth: covered exactly where a face is, and the owner map is the yardstick's
    bA, bB = r["buf"]
    for b in (bA, bB):
        assert np.array_equal(b["z_c"] > 0, b["face_c"] >= 0)
    ref = LR.composite_layers([(bA["rgb"], bA["z_c"], False), (bB["rgb"], bB["z_c"], True)], 1, bg=bg, channels=4)
    assert np.array_equal(owner, ref["owner"])
    _check_exactness(frames, owner, ref, 4, "two hands, ss = 1")


def test_scene_depth_ss1_exact(tmp_path_factory):
    r = _scene_ss1(tmp_path_factory)
    scene, bg, rows = r["scene"], r["bg"], np.arange(T)
    zA, zB = r["buf"][0]["z_c"], r["buf"][1]["z_c"]
    nearA, farA, nearB = float(zA[zA > 0].min()), float(zA[zA > 0].max()), float(zB[zB > 0].min())
    print(f"[scene depth] A spans [{nearA:.4f}, {farA:.4f}], B starts at {nearB:.4f}")
    assert farA < nearB, "the second hand lies wholly behind the first"
    plane = lambda v, n=1: torch.full((n, S, S), v, dtype=torch.float32, device=DEV)
    # a plane between the two: A alone over the backgrounds
    between = scene.render(rows, background=bg, alpha=True, scene_depth=plane(0.5 * (farA + nearB))).cpu().numpy()
    assert np.array_equal(between, r["A"])
    # a plane nearer than both: the backgrounds themselves
    front, own = scene.render(rows, background=bg, scene_depth=plane(0.5 * nearA, T), owner=True)
    assert torch.equal(front, bg) and not own.any()
    # zeros: no measurement, test 6's frames; one graph per (channels, depth?, owner?) so far
    zeros = scene.render(rows, background=bg, alpha=True, scene_depth=plane(0.0), owner=True)
    assert np.array_equal(zeros[0].cpu().numpy(), r["frames"]) and np.array_equal(zeros[1].cpu().numpy(), r["owner"])
    # per-frame rows: the front plane for frames 1 and 3 only, a row out of range elsewhere
    mixed = scene.render(rows, background=bg, alpha=True, scene_depth=plane(0.5 * nearA), depth_rows=[-1, 0, 1, 0, 7], owner=True)[0].cpu().numpy()
    assert np.array_equal(mixed[[0, 2, 4]], r["frames"][[0, 2, 4]]) and np.array_equal(mixed[[1, 3]][..., :3], bg.cpu().numpy()[[1, 3]])


def test_scene_player_ss2_plumbing(tmp_path_factory):
    from harp_amd.playback import AvatarPlayer, Motion, ScenePlayer
    hA, hB, bg = _two_hands(tmp_path_factory)
    rows = np.arange(T)
    scene = ScenePlayer(_players((hA, hB), 2, True), flip=[False, True])
    scene.load_motions([hA[3], hB[3]])
    bA, bB = _eager_buffers((hA, hB), 2, bg)
    near, far = float(bA["z_c"][bA["z_c"] > 0].min()), float(bB["z_c"][bB["z_c"] > 0].max())
    g = torch.Generator().manual_seed(5)                   # a depth map with no measurement on 20 %, hits and misses around the hands' depths
    depth = ((0.9 * near + (1.1 * far - 0.9 * near) * torch.rand(T, S, S, generator=g)) * (torch.rand(T, S, S, generator=g) > 0.2)).to(DEV)
    frames, owner = scene.render(rows, background=bg, alpha=True, scene_depth=depth, owner=True)
    frames, owner = frames.cpu().numpy().copy(), owner.cpu().numpy().copy()
    ref = LR.composite_layers([(bA["rgb"], bA["z_c"], False), (bB["rgb"], bB["z_c"], True)], 2, scene_z=depth.cpu().numpy(), bg=bg.cpu().numpy(), channels=4)
    u, t = _check_exactness(frames, owner, ref, 4, "two hands, ss = 2")
    assert {0, 1, 2} <= set(np.unique(owner)) and (ref["n"] % 4 != 0).any(), "partly covered pixels are what ss = 2 is about"
    print(f"[scene player] ss=2: {u} of {t} colour values within 0.01 of a rounding boundary")
    # a replay, the eager sequence, rows in reverse order: equal bytes, one graph
    again = scene.render(rows, background=bg, alpha=True, scene_depth=depth, owner=True)
    assert np.array_equal(again[0].cpu().numpy(), frames) and np.array_equal(again[1].cpu().numpy(), owner) and len(scene._graphs) == 1
    eager = ScenePlayer(_players((hA, hB), 2, True, use_graph=False), flip=[False, True])
    eager.load_motions([hA[3], hB[3]])
    e = eager.render(rows, background=bg, alpha=True, scene_depth=depth, owner=True)
    assert np.array_equal(e[0].cpu().numpy(), frames) and np.array_equal(e[1].cpu().numpy(), owner) and not eager._graphs
    back = scene.render(rows[::-1].copy(), background=bg, bg_rows=rows[::-1].copy(), alpha=True, scene_depth=depth, depth_rows=rows[::-1].copy(), owner=True)
    assert np.array_equal(back[0].cpu().numpy(), frames[::-1]) and np.array_equal(back[1].cpu().numpy(), owner[::-1]) and len(scene._graphs) == 1
    # rows beyond the motions: refused on the host, and the next render is what it was
    for bad in ([0, T], [-1], [2, 1, 7]):
        with pytest.raises(IndexError):
            scene.render(bad, background=bg)
    again = scene.render(rows, background=bg, alpha=True, scene_depth=depth, owner=True)
    assert np.array_equal(again[0].cpu().numpy(), frames)
    # what a scene refuses
    (cfgA, layerA, paramsA, mA), (cfgB, layerB, paramsB, mB) = hA, hB
    kd = lambda cfg, layer, params, **kw: AvatarPlayer(cfg, params, layer, device=DEV, **dict(dict(batch_size=BATCH, ss=2, keep_depth=True), **kw))
    ok = kd(cfgA, layerA, paramsA)
    with pytest.raises(ValueError):
        ScenePlayer([ok, kd(cfgB, layerB, paramsB, ss=1)])
    with pytest.raises(ValueError):
        ScenePlayer([ok, kd(dict(cfgB, img_size=S // 2), layerB, paramsB)])
    with pytest.raises(ValueError):
        ScenePlayer([ok, kd(cfgB, layerB, paramsB, batch_size=BATCH + 1)])
    with pytest.raises(ValueError):
        ScenePlayer([ok, kd(cfgB, layerB, paramsB, keep_depth=False)])
    with pytest.raises(ValueError):
        ScenePlayer([ok] * 5)
    with pytest.raises(ValueError):
        ScenePlayer([ok], flip=[False, True])
    with pytest.raises(ValueError):
        scene.load_motions([mA, Motion.from_params(paramsB, rows=[0, 1, 2])])
    with pytest.raises(ValueError):
        scene.load_motions([mA])


def test_scene_command_line(tmp_path_factory, tmp_path, monkeypatch):
    """python -m harp_amd.playback's main() with two fits (the loaders of licensed / fitted files replaced by the synthetic ones, chosen by
    the config's base_output_dir): --also ...:flip, --masks and --scene-depth in, one frame and one owner map per motion row out"""
    import yaml
    from PIL import Image
    from harp_amd import playback
    from harp_amd.utils import file_utils, hand_model_utils
    hA, hB, bg = _two_hands(tmp_path_factory)
    by_dir = {h[0]["base_output_dir"]: h for h in (hA, hB)}
    assert len(by_dir) == 2
    monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda c: (by_dir[c["base_output_dir"]][1], by_dir[c["base_output_dir"]][2]["verts_uvs"],
                                                                         by_dir[c["base_output_dir"]][2]["faces_uvs"], None))
    monkeypatch.setattr(file_utils, "load_result", lambda base, device="cuda", test=False: dict(by_dir[base][2]))
    for name, h in (("a", hA), ("b", hB)):
        with open(tmp_path / f"{name}.yaml", "w") as f:
            yaml.safe_dump({k: h[0][k] for k in ("use_arm", "img_size", "focal_length", "self_shadow", "share_light_position", "base_output_dir")}, f)
        h[3].save(tmp_path / f"{name}.npz")
    zA = _scene_ss1(tmp_path_factory)["buf"][0]["z_c"]
    g = torch.Generator().manual_seed(9)
    depth = (torch.rand(2, S, S, generator=g) < 0.5).float() * float(zA[zA > 0].min()) * 0.5     # half the pixels hidden by something near
    (tmp_path / "depth").mkdir()
    np.save(tmp_path / "depth" / "00.npy", depth[0].numpy())
    Image.fromarray(np.round(depth[1].numpy() * 1000.0).astype(np.uint16)).save(tmp_path / "depth" / "01.png")       # millimetres
    depth[1] = torch.from_numpy(np.round(depth[1].numpy() * 1000.0).astype(np.uint16).astype(np.float32) * 1e-3)
    out = tmp_path / "frames"
    paths = playback.main(["--config", str(tmp_path / "a.yaml"), "--motion", str(tmp_path / "a.npz"), "--out", str(out), "--alpha", "--masks",
                           "--also", f"{tmp_path / 'b.yaml'}:{tmp_path / 'b.npz'}:flip", "--scene-depth", str(tmp_path / "depth"), "--batch-size", "4"])
    assert len(paths) == T and sorted(os.listdir(out)) == ["%04d.png" % i for i in range(T)] + ["mask_%04d.png" % i for i in range(T)]
    masks = np.stack([np.asarray(Image.open(out / ("mask_%04d.png" % i))) for i in range(T)])
    assert masks.shape == (T, S, S) and set(np.unique(masks)) <= {0, 1, 2} and {1, 2} <= set(np.unique(masks))
    scene = playback.ScenePlayer(_players((hA, hB), 1, True), flip=[False, True])
    scene.load_motions([hA[3], hB[3]])
    for i in (0, 1):
        want, own = scene.render([i], alpha=True, scene_depth=depth.to(DEV), depth_rows=[i % 2], owner=True)
        assert np.array_equal(np.asarray(Image.open(paths[i])), want.cpu().numpy()[0]) and np.array_equal(masks[i], own.cpu().numpy()[0])
    # --flip alone takes the scene path with one avatar: the single player's frames, mirrored
    one = playback.main(["--config", str(tmp_path / "b.yaml"), "--motion", str(tmp_path / "b.npz"), "--out", str(tmp_path / "flip"), "--alpha", "--flip"])
    plain = playback.main(["--config", str(tmp_path / "b.yaml"), "--motion", str(tmp_path / "b.npz"), "--out", str(tmp_path / "plain"), "--alpha"])
    assert np.array_equal(np.asarray(Image.open(one[0])), np.asarray(Image.open(plain[0]))[:, ::-1])
