"""-m gpu: playback of a fitted avatar (harp_amd/playback/, csrc/playback.hip).  harp_motion_resample and harp_resolve_u8 against the
float64 restatements of tests/_playback_ref.py at their edges; AvatarPlayer against an expectation built independently of it — the
reference-API mirror (`mirror_render`) at img_size * ss on a parameter dict that holds the motion's rows, resolved in float64 over a random
background; the exact properties of the player (graph = eager, replay, a shorter motion on the same graph, rows checked on the host); and
Motion.resample / AvatarPlayer.play end to end.  (tests/test_gpu_playback.py is the older turntable playback of the post-fit pass.)"""
import os

import numpy as np
import pytest
import torch

from tests import _playback_ref as R
from tests.test_gpu_evaluate import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"

# worst deviation of a rotation-matrix entry of harp_motion_resample from the float64 slerp over all cases below, MEASURED on MI355X
# (profiles/playback_errors.txt); the test asserts 4 x this and in no case more than 2e-5: a wrong branch (long arc, missing
# offset, flipped sign) shows as >= 1e-2
ROT_DEV_MEASURED = 5.549e-07
ROT_BOUND = min(2e-5, 4.0 * ROT_DEV_MEASURED)
# three float32 roundings of magnitude <= 1 in (1 - f) a + f b, each <= 2^-25, and the sum's: <= 2^-23; asserted with a factor 2
LIN_BOUND = 2.0 ** -22
# uint8 values of the player more than one level off the mirror's float64-resolved frames, per scene, MEASURED on MI355X;
# the test asserts 2 x this + 8 and never more than 0.5 % of the values of pixels with any coverage
PLAYER_OFF_MEASURED = {"hand_ss1_shadow1": 6, "hand_ss1_shadow0": 6, "hand_ss2_shadow1": 9, "hand_ss2_shadow0": 9, "arm_ss1_shadow1": 3}

N_PATTERNS = 9


def _unit(rng):
    u = rng.normal(size=3)
    return u / np.linalg.norm(u)


def _rot_keys(rng, Tk, n_rot, shift):
    """the TRUE rotations (axis-angle, float64) of the keys, one pattern per rotation channel: zero | 1e-9 | 1e-5 | pi - 1e-3 next to a
    neighbour 1 rad further along the same axis (not near the identity: random axes against zeros are often 180 degrees apart) | 4 and 6 rad |
    identical neighbours | neighbours 1e-4 relative apart | a key and its 2 pi complement | random up to 3 rad"""
    out = np.zeros((Tk, n_rot, 3))
    for j in range(n_rot):
        p, u = (j + shift) % N_PATTERNS, _unit(rng)
        for k in range(Tk):
            if p == 1:
                out[k, j] = 1e-9 * _unit(rng)
            elif p == 2:
                out[k, j] = 1e-5 * _unit(rng)
            elif p == 3:
                out[k, j] = (np.pi - 1e-3 - (k % 2)) * u
            elif p == 4:
                out[k, j] = (4.0 if k % 2 == 0 else 6.0) * _unit(rng)
            elif p == 5:
                out[k, j] = 1.3 * u
            elif p == 6:
                out[k, j] = 0.8 * u * (1.0 + 1e-4 * k)
            elif p == 7:
                out[k, j] = (2.2 - 2.0 * np.pi * (k % 2)) * u
            elif p == 8:
                out[k, j] = rng.uniform(0.0, 3.0) * _unit(rng)
    return out


def _resample_case(Tk, n_rot, n_lin, Tn, with_off, shift, seed):
    """keys / offset / times (float32) of one case; key pairs within |q0 . q1| < 1e-3 of 180 degrees apart are ambiguous for any slerp
    and are redrawn (checked on the float64 side, on the float32 values the kernel sees)"""
    for attempt in range(50):
        rng = np.random.default_rng(seed + 7919 * attempt)
        true = _rot_keys(rng, Tk, n_rot, shift)
        off = (rng.normal(size=3 * n_rot) * 0.5).astype(np.float32) if with_off else None
        rot = true.reshape(Tk, 3 * n_rot) - (0.0 if off is None else off.astype(np.float64))
        keys = np.concatenate([rot, rng.uniform(-1.0, 1.0, size=(Tk, n_lin))], 1).astype(np.float32)
        if R.ambiguous_pairs(keys, n_rot, off) >= 1e-3:
            break
    else:
        raise AssertionError("no unambiguous keys drawn")
    if Tn == 1:
        times = np.array([0.37 * (Tk - 1)])
    else:
        special = [float(k) for k in range(Tk)] + [-0.5, -3.0, Tk - 1 + 0.25, Tk + 7.0] + [k + 1e-6 for k in range(Tk - 1)] + [np.nan]
        times = np.concatenate([special, rng.uniform(0.0, Tk - 1, size=Tn - len(special))])
    return keys, off, times.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("n_rot,n_lin", [(1, 0), (0, 9), (16, 9), (17, 9)])
def test_motion_resample_against_float64(n_rot, n_lin):
    from harp_amd import _lib, ops
    L, W = _lib.lib(), 3 * n_rot + n_lin
    worst = worst_lin = 0.0
    n_cases = 0
    for Tk in (1, 2, 5):
        for Tn in (1, 63, 65, 257):
            for with_off in (False, True):
                for shift in (range(N_PATTERNS) if n_rot == 1 else (0,)):
                    keys, off, times = _resample_case(Tk, n_rot, n_lin, Tn, with_off, shift, seed=1000 * Tk + 10 * Tn + shift)
                    kd, td = torch.from_numpy(keys).to(DEV), torch.from_numpy(times).to(DEV)
                    od = None if off is None else torch.from_numpy(off).to(DEV)
                    got_t = ops.motion_resample(kd, td, n_rot, od)
                    raw = torch.full((Tn, W), float("nan"), device=DEV)
                    assert L.harp_motion_resample(_lib.ptr(kd), Tk, n_rot, n_lin, _lib.ptr(od), _lib.ptr(td), Tn, _lib.ptr(raw), _lib.stream()) == 0
                    got = got_t.cpu().numpy()
                    assert np.array_equal(_bits(got), _bits(raw.cpu().numpy())), "ops and the C entry point differ"
                    rows, Rref, lin = R.motion_resample(keys, n_rot, times, off)
                    on_key = rows >= 0
                    if Tn > 1:                           # 0, Tk - 1, every integer, the clamped times and the NaN (-> row 0) are all there
                        assert on_key[:Tk + 4].all() and (rows[:Tk] == np.arange(Tk)).all()
                        assert rows[Tk] == 0 and rows[Tk + 1] == 0 and rows[Tk + 2] == Tk - 1 and rows[Tk + 3] == Tk - 1 and rows[2 * Tk + 3] == 0
                    assert np.array_equal(_bits(got[on_key]), _bits(keys[rows[on_key]])), "a time on a key must copy the row bit for bit"
                    assert np.isfinite(got).all()
                    if n_rot:
                        o64 = np.zeros(3 * n_rot) if off is None else off.astype(np.float64)
                        Rgot = R.rotation_matrix((got[:, :3 * n_rot].astype(np.float64) + o64).reshape(Tn, n_rot, 3))
                        worst = max(worst, float(np.abs(Rgot - Rref).max()))
                        for j in range(n_rot):           # a key and its 2 pi complement: that same rotation at every time
                            if (j + shift) % N_PATTERNS == 7:
                                R0 = R.rotation_matrix(keys[0, 3 * j:3 * j + 3].astype(np.float64) + o64[3 * j:3 * j + 3])
                                worst = max(worst, float(np.abs(Rgot[:, j] - R0).max()))
                    if n_lin:
                        worst_lin = max(worst_lin, float(np.abs(got[:, 3 * n_rot:] - lin).max()))
                    n_cases += 1
    print(f"[motion_resample] n_rot={n_rot} n_lin={n_lin}: worst rotation-matrix entry deviation {worst:.3e}, worst linear channel {worst_lin:.3e} "
          f"over {n_cases} cases (bounds {ROT_BOUND:.1e}, {LIN_BOUND:.1e})")
    assert worst <= ROT_BOUND and worst_lin <= LIN_BOUND


def test_motion_resample_binding_checks():
    from harp_amd import ops
    k, t = torch.zeros(3, 12, device=DEV), torch.zeros(4, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.motion_resample(k.cpu(), t.cpu(), 1)
    with pytest.raises(TypeError):
        ops.motion_resample(k.double(), t, 1)
    with pytest.raises(ValueError):
        ops.motion_resample(k, t, 5)                     # 15 rotation columns of 12
    with pytest.raises(ValueError):
        ops.motion_resample(k, t, 2, torch.zeros(5, device=DEV))
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.motion_resample(k.clone().requires_grad_(), t, 1)


def _coverage(rng, kind, B, Sh):
    if kind == "none":
        c = np.zeros((B, Sh, Sh), bool)
    elif kind == "all":
        c = np.ones((B, Sh, Sh), bool)
    elif kind == "checker":
        c = np.broadcast_to((np.add.outer(np.arange(Sh), np.arange(Sh)) % 2 == 0), (B, Sh, Sh))
    else:
        c = rng.uniform(size=(B, Sh, Sh)) < 0.6
    return np.where(c, rng.integers(0, 5000, size=(B, Sh, Sh)), -1).astype(np.int32)


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_resolve_u8_against_float64(ss):
    from harp_amd import _lib, ops
    L = _lib.lib()
    rng = np.random.default_rng(40 + ss)
    undecided = total = n_cases = 0
    for S in (1, 7, 16, 33):
        for B in (1, 3):
            for channels in (3, 4):
                for cov in ("none", "all", "checker", "random"):
                    for bgk in ("color", "one", "per_row", "rows"):
                        Sh = S * ss
                        rgb = rng.uniform(-0.1, 1.1, size=(B, Sh, Sh, 3)).astype(np.float32)
                        rgb.reshape(-1)[rng.integers(0, rgb.size, size=max(1, rgb.size // 50))] = np.nan
                        fid = _coverage(rng, cov, B, Sh)
                        color = rng.uniform(0.0, 1.0, size=3).astype(np.float32)
                        n_bg = {"color": 0, "one": 1, "per_row": B, "rows": 4}[bgk]
                        bg = rng.integers(0, 256, size=(n_bg, S, S, 3)).astype(np.uint8) if n_bg else None
                        rows = None
                        if bgk == "rows":
                            rows = rng.integers(0, 4, size=B).astype(np.int32)
                            rows[rng.integers(0, B)] = [-1, 4][n_cases % 2]          # one entry out of range: the constant colour
                        dv = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
                        got = ops.resolve_u8(dv(rgb), dv(fid), ss, dv(bg), dv(rows), dv(color), alpha=channels == 4).cpu().numpy()
                        ref = R.resolve_u8(rgb, fid, ss, bg, rows, color, channels)
                        assert got.shape == (B, S, S, channels) and got.dtype == np.uint8
                        if channels == 4:
                            assert np.array_equal(got[..., 3], ref["out"][..., 3]), "alpha is the integer formula, bit for bit"
                        empty = ref["n"] == 0
                        assert np.array_equal(got[..., :3][empty], ref["out"][..., :3][empty]), "an uncovered pixel is the background byte"
                        dist = np.abs(ref["v255"] - np.floor(ref["v255"]) - 0.5)       # to the nearest rounding boundary k + 0.5
                        decided = (dist > 0.01) | empty[..., None]
                        d = np.abs(got[..., :3].astype(np.int64) - ref["out"][..., :3].astype(np.int64))
                        assert (d[decided] == 0).all(), (S, B, channels, cov, bgk, int(d[decided].max()))
                        assert d.max() <= 1
                        undecided += int((~decided).sum())
                        total += decided.size
                        n_cases += 1
    # refused: no bg_rows and a number of backgrounds that is neither 1 nor B
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    rgb, fid, bg, col, out = z(3, 4 * ss, 4 * ss, 3), z(3, 4 * ss, 4 * ss, dt=torch.int32), z(2, 4, 4, 3, dt=torch.uint8), z(3), z(3, 4, 4, 3, dt=torch.uint8)
    assert L.harp_resolve_u8(_lib.ptr(rgb), _lib.ptr(fid), 3, 4, ss, _lib.ptr(bg), 2, None, _lib.ptr(col), 3, _lib.ptr(out), _lib.stream()) == 1
    with pytest.raises(ValueError):
        ops.resolve_u8(rgb, fid, ss, bg)
    share = undecided / total
    print(f"[resolve_u8] ss={ss}: {n_cases} cases, {undecided} of {total} colour values ({share:.2%}) within 0.01 of a rounding boundary (one level allowed there)")
    assert share <= 0.05


# ---- the player ------------------------------------------------------------------------------------------------------------------
S, T = 32, 5
PERM = [3, 0, 4, 1, 2]


def _arm_setup(T, S, seed, tmp_path, **cfg_kw):
    """the arm counterpart of tests/test_gpu_evaluate._setup: synthetic SMPL-X arm model, the mirror's layer and parameter dict"""
    from harp_amd import synth
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    from harp_amd.optimize_sequence import init_params
    from harp_amd.utils.config_utils import get_config
    tpl = synth.load_template("arm")
    m = synth.make_smplx_arm_model(tpl, seed=seed)
    corr = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "harp_amd", "assets", "arm_corr.npz"))
    layer = SMPLXARM(m, m["faces"], corr["mano_vert_from_arm"], device=DEV)
    focal = 1000.0 * S / 224.0
    g = torch.Generator().manual_seed(seed)
    c = m["v_template"].mean(0)
    seq = dict(pose=torch.randn(T, 45, generator=g) * 0.15, rot=torch.randn(T, 3, generator=g) * 0.2, trans=torch.randn(T, 3, generator=g) * 0.01,
               shape=torch.randn(T, 10, generator=g) * 0.3, joints=torch.zeros(T, 21, 3),
               cam=torch.tensor([[2 * focal / (S * 1.6), -float(c[0]), -float(c[1])]]).repeat(T, 1) + torch.randn(T, 3, generator=g) * 0.005)
    cfg = get_config(write_yaml=False, use_arm=True, img_size=S, focal_length=focal, base_output_dir=str(tmp_path) + "/", **cfg_kw)
    uv_mask = torch.from_numpy(tpl["uv_mask"]).double() / 255
    params = init_params(seq, True, True, None, layer.right_arm_faces_tensor, False, torch.from_numpy(tpl["verts_uvs"])[None],
                         torch.from_numpy(tpl["faces_uvs"])[None], use_arm=True, configs=cfg, device=DEV, uv_mask=uv_mask)
    with torch.no_grad():
        params["texture"].copy_(torch.rand(1, 512, 512, 3, generator=g) * 0.5 + 0.3)
        params["wrist_pose"].copy_(torch.randn(T, 3, generator=g) * 0.2)
        params["verts_disps"].copy_(torch.randn(4083, 1, generator=g) * 0.0006)
        params["light_positions"].copy_(params["light_positions"] + 0.1 * torch.randn(T, 3, generator=g).to(DEV))
    return cfg, layer, params


_SCENES = {}


def _scene(kind, shadow, tmp_path_factory):
    """(cfg, layer, params, motion, background) of a scene, built once: the motion's rows are a permutation of the fit's (hand) and it
    carries its own light — not the identity replay"""
    from harp_amd.playback import Motion
    key = (kind, shadow)
    if key not in _SCENES:
        tmp = tmp_path_factory.mktemp(f"player_{kind}_{int(shadow)}")
        g = torch.Generator().manual_seed(77)
        if kind == "hand":
            _, cfg, layer, params, _ = _setup(T, S, 31, tmp, self_shadow=shadow, share_light_position=True)
            with torch.no_grad():
                params["normal_map"].copy_(torch.tensor([0., 0., 1.]).repeat(1, 512, 512, 1) + torch.randn(1, 512, 512, 3, generator=g) * 0.15)
                params["verts_disps"].copy_((torch.randn(params["verts_disps"].shape, generator=g) * 0.0006).to(DEV))
            rows = PERM
        else:
            cfg, layer, params = _arm_setup(2, S, 32, tmp, self_shadow=shadow)
            rows = [1, 0]
        motion = Motion.from_params(params, rows=rows)
        assert motion.light_positions is None            # (a shared-light fit: only row 0 of its table means anything)
        motion.light_positions = (params["light_positions"].detach()[rows].cpu() + 0.2 * torch.randn(len(rows), 3, generator=g)).contiguous()
        bg = torch.randint(0, 256, (len(rows), S, S, 3), generator=g, dtype=torch.uint8).to(DEV)
        _SCENES[key] = (cfg, layer, params, motion, bg)
    return _SCENES[key]


def _mirror_expectation(cfg, layer, params, motion, bg, ss):
    """the frames the player should produce, without the player: mirror_render at img_size * ss and focal * ss on a parameter dict whose
    per-frame tables are the motion's rows, its image and its silhouette >= 0.5 through the float64 resolve over `bg`"""
    from harp_amd.evaluate import mirror_render
    from harp_amd.utils.visualize import get_mesh_subdivider, params_on
    n = len(motion)
    P = params_on(params, DEV)
    own_light = motion.light_positions is not None       # without it: the fit's light table as it is, shared as the fit's config says
    for k in ("pose", "rot", "trans", "cam") + (("light_positions",) if own_light else ()) + (("wrist_pose",) if cfg["use_arm"] else ()):
        P[k] = getattr(motion, k).to(DEV)
    cfg2 = dict(cfg, img_size=cfg["img_size"] * ss, focal_length=cfg["focal_length"] * ss)
    if own_light:
        cfg2["share_light_position"] = False
    with torch.no_grad():
        m = mirror_render(cfg2, P, torch.arange(n), layer, get_mesh_subdivider(layer, use_arm=bool(cfg["use_arm"]), device=DEV), device=DEV)
    cover = np.where(m.y_sil_pred.cpu().numpy() >= 0.5, 0, -1).astype(np.int32)
    return R.resolve_u8(m.y_pred.cpu().numpy(), cover, ss, bg.cpu().numpy(), None, (1.0, 1.0, 1.0), 3)


def _check_against_mirror(tag, got, ref):
    d = np.abs(got.astype(np.int64) - ref["out"].astype(np.int64))
    off = int((d > 1).sum())
    covered_values = int((ref["n"] > 0).sum()) * 3
    cap = int(0.005 * covered_values)
    rec = PLAYER_OFF_MEASURED.get(tag)
    bound = cap if rec is None else min(2 * rec + 8, cap)
    print(f"[player vs mirror] {tag}: {off} of {d.size} values more than one level off ({covered_values} values of covered pixels, "
          f"{int((d == 1).sum())} one level off; bound {bound}, 0.5 % cap {cap})")
    assert covered_values > 300, "the scene must show the avatar"
    assert off <= bound, (tag, off, bound)


@pytest.mark.parametrize("ss,shadow", [(1, True), (1, False), (2, True), (2, False)])
def test_player_hand_against_mirror(tmp_path_factory, ss, shadow):
    from harp_amd.playback import AvatarPlayer, Motion
    cfg, layer, params, motion, bg = _scene("hand", shadow, tmp_path_factory)
    player = AvatarPlayer(cfg, params, layer, batch_size=2, ss=ss, use_graph=True, device=DEV)      # batches of 2, 2, 1
    player.load_motion(motion)
    rows = np.arange(T)
    got = player.render(rows, background=bg).cpu().numpy()
    assert got.shape == (T, S, S, 3) and got.dtype == np.uint8
    _check_against_mirror(f"hand_ss{ss}_shadow{int(shadow)}", got, _mirror_expectation(cfg, layer, params, motion, bg, ss))
    # exact: a replay, the eager sequence, rows in another order
    assert np.array_equal(player.render(rows, background=bg).cpu().numpy(), got)
    eager = AvatarPlayer(cfg, params, layer, batch_size=2, ss=ss, use_graph=False, device=DEV)
    eager.load_motion(motion)
    assert np.array_equal(eager.render(rows, background=bg).cpu().numpy(), got)
    assert not eager._graphs and len(player._graphs) == 1
    back = player.render(rows[::-1].copy(), background=bg, bg_rows=rows[::-1].copy()).cpu().numpy()
    assert np.array_equal(back, got[::-1]) and len(player._graphs) == 1
    # rows beyond the motion: refused on the host, and the next render is what it was
    for bad in ([0, T], [-1], [2, 1, 7]):
        with pytest.raises(IndexError):
            player.render(bad, background=bg)
    assert np.array_equal(player.render(rows, background=bg).cpu().numpy(), got)
    # a shorter motion (the fit's own light this time) reuses the tables and the captured graph
    short = Motion.from_params(params, rows=[2, 1, 0])
    short.light_positions = None
    graph = next(iter(player._graphs.values()))
    player.load_motion(short)
    eager.load_motion(short)
    with pytest.raises(IndexError):
        player.render(rows, background=bg)               # row 3 and 4 are gone
    r5 = [0, 1, 2, 1, 0]
    a, b = player.render(r5, background=bg).cpu().numpy(), eager.render(r5, background=bg).cpu().numpy()
    assert len(player._graphs) == 1 and next(iter(player._graphs.values())) is graph
    assert np.array_equal(a, b) and not np.array_equal(a, got)
    # RGBA over the constant colour: the colour planes of an opaque pixel do not depend on the background
    rgba = player.render(r5, alpha=True).cpu().numpy()
    assert rgba.shape == (5, S, S, 4) and set(np.unique(rgba[..., 3])) <= ({0, 255} if ss == 1 else set(range(256)))
    opaque = rgba[..., 3] == 255
    assert opaque.any() and np.array_equal(rgba[..., :3][opaque], a[opaque]) and (rgba[..., :3][rgba[..., 3] == 0] == 255).all()


def test_player_replays_a_shared_light_fit_with_its_row_0(tmp_path_factory):
    """Motion.from_params of a fit with share_light_position: the light table's rows differ (only row 0 was ever fitted), the replay
    must light every frame with row 0 as mirror_render and the fit do — against the mirror with share_light_position=True; a fresh
    background tensor per call is served by the one captured graph; a per-frame-light fit asks the motion for its light"""
    from harp_amd.playback import AvatarPlayer, Motion
    cfg, layer, params, _, bg = _scene("hand", True, tmp_path_factory)
    lp = params["light_positions"].detach()
    assert cfg["share_light_position"] and float((lp[1:] - lp[0]).abs().max()) > 0.05
    replay = Motion.from_params(params)
    assert replay.light_positions is None and len(replay) == T
    player = AvatarPlayer(cfg, params, layer, batch_size=2, ss=1, device=DEV)
    player.load_motion(replay)
    got = player.render(np.arange(T), background=bg).cpu().numpy()
    _check_against_mirror("hand_ss1_shadow1_replay", got, _mirror_expectation(cfg, layer, params, replay, bg, 1))
    for shift in (1, 2):                                 # other tensors, other contents: the same graph, the right frames
        other = torch.roll(bg, shift, 0).contiguous()
        again = player.render(np.arange(T), background=other, bg_rows=(np.arange(T) + shift) % T).cpu().numpy()
        assert np.array_equal(again, got) and len(player._graphs) == 1
    # with the rows' own lights (what a per-frame-light fit replays) the frames differ from the shared-light ones
    per_frame = Motion.from_params(params, per_frame_light=True)
    assert np.array_equal(per_frame.light_positions.cpu().numpy(), lp.cpu().numpy())
    player.load_motion(per_frame)
    lit = player.render(np.arange(T), background=bg).cpu().numpy()
    assert np.array_equal(lit[0], got[0]) and not np.array_equal(lit[1:], got[1:])
    unshared = AvatarPlayer(dict(cfg, share_light_position=False), params, layer, batch_size=2, device=DEV)
    with pytest.raises(ValueError, match="light_positions"):
        unshared.load_motion(replay)
    unshared.load_motion(per_frame)
    assert np.array_equal(unshared.render(np.arange(T), background=bg).cpu().numpy(), lit)


def test_player_arm_against_mirror(tmp_path_factory):
    from harp_amd.playback import AvatarPlayer
    cfg, layer, params, motion, bg = _scene("arm", True, tmp_path_factory)
    player = AvatarPlayer(cfg, params, layer, batch_size=2, ss=1, use_graph=True, device=DEV)
    player.load_motion(motion)
    got = player.render([0, 1], background=bg).cpu().numpy()
    _check_against_mirror("arm_ss1_shadow1", got, _mirror_expectation(cfg, layer, params, motion, bg, 1))
    eager = AvatarPlayer(cfg, params, layer, batch_size=2, ss=1, use_graph=False, device=DEV)
    eager.load_motion(motion)
    assert np.array_equal(eager.render([0, 1], background=bg).cpu().numpy(), got)


def test_resample_and_play_end_to_end(tmp_path_factory, tmp_path):
    from PIL import Image
    from harp_amd.playback import AvatarPlayer
    cfg, layer, params, motion, bg = _scene("hand", True, tmp_path_factory)
    player = AvatarPlayer(cfg, params, layer, batch_size=2, ss=2, device=DEV)
    player.load_motion(motion)
    want = player.render(np.arange(T), background=bg).cpu().numpy()
    # resampling at the key times is the identity, bit for bit, and so are the frames
    same = motion.resample(np.arange(T), layer, device=DEV)
    for k in ("pose", "rot", "trans", "cam", "wrist_pose", "light_positions"):
        assert np.array_equal(_bits(getattr(same, k).cpu().numpy()), _bits(getattr(motion, k).cpu().numpy())), k
    player.load_motion(same)
    assert np.array_equal(player.render(np.arange(T), background=bg).cpu().numpy(), want)
    # retimed to 9 frames: the odd ones are in-betweens, the even ones the keys
    slow = motion.resample(np.linspace(0, T - 1, 2 * T - 1), layer, device=DEV)
    assert len(slow) == 2 * T - 1 and np.array_equal(_bits(slow.pose.cpu().numpy()[::2]), _bits(motion.pose.cpu().numpy()))
    player.load_motion(slow)
    frames = player.render(np.arange(len(slow)), background=bg, bg_rows=np.arange(len(slow)) // 2).cpu().numpy()
    assert np.array_equal(frames[::2], want) and not np.array_equal(frames[1], frames[0])
    # play: %04d.png that decode to render's bytes, over backgrounds cycled i mod N; RGBA with alpha
    paths = player.play(slow, str(tmp_path / "rgb"), backgrounds=bg, fmt="png")
    assert [os.path.basename(p) for p in paths] == ["%04d.png" % i for i in range(len(slow))] and sorted(os.listdir(tmp_path / "rgb")) == ["%04d.png" % i for i in range(len(slow))]
    want_play = player.render(np.arange(len(slow)), background=bg, bg_rows=np.arange(len(slow)) % T).cpu().numpy()
    for i, p in enumerate(paths):
        im = Image.open(p)
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), want_play[i]), i
    paths = player.play(slow, str(tmp_path / "rgba"), fmt="png", alpha=True)
    want_a = player.render(np.arange(len(slow)), alpha=True).cpu().numpy()
    for i, p in enumerate(paths):
        im = Image.open(p)
        assert im.mode == "RGBA" and np.array_equal(np.asarray(im), want_a[i]), i
    assert len(os.listdir(tmp_path / "rgba")) == len(slow)
    jp = player.play(motion, str(tmp_path / "jpg"))
    assert [os.path.basename(p) for p in jp] == ["%04d.jpg" % i for i in range(T)] and Image.open(jp[0]).size == (S, S)
    with pytest.raises(ValueError):
        player.play(motion, str(tmp_path / "bad"), fmt="jpg", alpha=True)


def test_command_line_writes_the_frames(tmp_path_factory, tmp_path, monkeypatch):
    """python -m harp_amd.playback's main() with the two loaders of licensed / fitted files replaced by the synthetic scene: a config, a
    motion file and a background directory in, retimed frames out"""
    import yaml
    from PIL import Image
    from harp_amd import playback
    from harp_amd.utils import file_utils, hand_model_utils
    cfg, layer, params, motion, bg = _scene("hand", True, tmp_path_factory)
    monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda c: (layer, params["verts_uvs"], params["faces_uvs"], None))
    monkeypatch.setattr(file_utils, "load_result", lambda base, device="cuda", test=False: dict(params))
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump({k: cfg[k] for k in ("use_arm", "img_size", "focal_length", "self_shadow", "share_light_position", "base_output_dir")}, f)
    motion.save(tmp_path / "motion.npz")
    (tmp_path / "bg").mkdir()
    for i in range(2):
        Image.fromarray(bg[i].cpu().numpy()).save(tmp_path / "bg" / ("%02d.png" % i))
    out = tmp_path / "frames"
    paths = playback.main(["--config", str(tmp_path / "cfg.yaml"), "--motion", str(tmp_path / "motion.npz"), "--out", str(out), "--fps-scale", "2",
                           "--ss", "2", "--background", str(tmp_path / "bg"), "--batch-size", "4"])
    assert sorted(os.listdir(out)) == ["%04d.jpg" % i for i in range(2 * T - 1)] and len(paths) == 2 * T - 1
    assert Image.open(paths[0]).size == (S, S)
    # the same frames as PNG with alpha: frame 0 is the motion's frame 0 over the constant colour
    paths = playback.main(["--config", str(tmp_path / "cfg.yaml"), "--motion", str(tmp_path / "motion.npz"), "--out", str(tmp_path / "rgba"), "--alpha"])
    player = playback.AvatarPlayer(cfg, params, layer, batch_size=2, device=DEV)
    player.load_motion(motion)
    assert len(paths) == T and np.array_equal(np.asarray(Image.open(paths[0])), player.render([0], alpha=True).cpu().numpy()[0])
