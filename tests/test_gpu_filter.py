"""-m gpu: the motion filter (csrc/filter.hip: harp_motion_filter; harp_amd/playback/motion.py Motion.smooth, smooth_keypoints, motion_jitter;
DESIGN.md §25) against the float64 yardstick of tests/_filter_ref.py on the fixtures of tests/_filter_cases.py, its exact (bitwise)
properties, its manifold properties, what trimming does to a spike, and the layer above it.  Every figure is printed before it is
asserted; the bounds are 4 x the values measured on MI355X (profiles/filter_errors.txt), the project's convention for float32 against
float64."""
import numpy as np
import pytest
import torch

from tests import _filter_cases as C
from tests import _filter_ref as F
from tests._playback_ref import quat_of, rotation_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 4.0
RESAMPLE_BOUND = 2e-5               # what harp_motion_resample's test allows for the same conversions: no bound here may exceed it
# worst deviation from the yardstick over the 24 cases of each channel mix, MEASURED on MI355X:
ROT_MEASURED = 6.658e-07            # ... of a rotation-matrix entry of (out + offset)
VEC_MEASURED = 4.196e-07            # ... of a vector or scalar value, relative to the largest magnitude among the window's used samples
# manifold properties, MEASURED on MI355X (rotation-matrix entry; value relative to the track's largest magnitude):
COMPLEMENT_MEASURED = 5.001e-07     # track 1: a constant rotation written alternately as a triple and its 2 pi complement
GEODESIC_MEASURED = 4.761e-07       # track 2: R0 exp(t w), |w| = 0.05 rad per frame
AFFINE_MEASURED = 2.347e-07         # track 3: affine vector and scalar tracks
# through the layer, MEASURED on MI355X: largest joint distance (mm) of the motion solved from smoothed noisy keypoints to the clean motion's
LAYER_DIST_MEASURED_MM = 3.132


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _filter(rows, n_rot, n_vec, taps, weights=None, segment=None, trim=None, rot_offset=None, iters=2):
    from harp_amd import ops
    out, used = ops.motion_filter(_dev(rows), n_rot, n_vec, taps, weights=_dev(weights), segment=_dev(segment, torch.int32), trim=_dev(trim),
                                  rot_offset=_dev(rot_offset), iters=iters)
    return out, used


def _channels(a, n3):
    """(T, W) -> (T, nch, 3): a scalar channel in column 0"""
    T, W = a.shape
    o = np.zeros((T, n3 + W - 3 * n3, 3), a.dtype)
    o[:, :n3] = a[:, :3 * n3].reshape(T, n3, 3)
    o[:, n3:, 0] = a[:, 3 * n3:]
    return o


def _angle(a, b):
    """geodesic angle between the rotations of two axis-angle arrays (..., 3), float64"""
    return np.linalg.norm(F.qlog(F.qmul(F.qconj(quat_of(a)), quat_of(b))), axis=-1)


@pytest.mark.parametrize("mix", C.MIXES, ids=lambda m: "rot%d_vec%d_lin%d" % m)
def test_against_the_float64_yardstick(mix):
    """TS x RS per channel mix with the weights, segments, offset, iters and trim of tests/_filter_cases.py: `used` exactly, copied channels
    bit for bit, rotations by their matrices, values relative to the window's largest magnitude; float32-undecidable cases left out,
    at most 2 % of the test's"""
    n_rot, n_vec, n_lin = mix
    n3 = n_rot + n_vec
    worst_r = worst_v = 0.0
    pairs = left_out = 0
    for c in C.yardstick_cases(mix):
        kw = {k: c[k] for k in ("weights", "segment", "trim", "rot_offset", "iters")}
        ref = F.motion_filter(c["rows"], n_rot, n_vec, c["taps"], **kw)
        out_t, used_t = _filter(c["rows"], n_rot, n_vec, c["taps"], **kw)
        out, used = out_t.cpu().numpy(), used_t.cpu().numpy()
        ok = ~ref["undecidable"]
        pairs += ok.size
        left_out += int((~ok).sum())
        assert np.array_equal(used[ok], ref["used"][ok]), (c["name"], np.argwhere((used != ref["used"]) & ok)[:4])
        o3, i3 = _channels(out, n3), _channels(c["rows"], n3)
        cp = ref["copy"] & ok
        assert np.array_equal(o3[cp].view(np.int32), i3[cp].view(np.int32)), c["name"]
        m = ok & ~ref["copy"]
        assert np.isfinite(o3[m]).all(), c["name"]
        if n_rot and m[:, :n_rot].any():
            off = np.zeros((n_rot, 3)) if c["rot_offset"] is None else c["rot_offset"].astype(np.float64).reshape(n_rot, 3)
            d = np.abs(rotation_matrix(o3[:, :n_rot].astype(np.float64) + off) - ref["R"]).max((-1, -2))
            worst_r = max(worst_r, float(d[m[:, :n_rot]].max()))
        if m[:, n_rot:].any():
            d = np.abs(o3.astype(np.float64) - _channels(ref["out"], n3)).max(-1)[:, n_rot:] / np.maximum(ref["scale"][:, n_rot:], 1e-30)
            worst_v = max(worst_v, float(d[m[:, n_rot:]].max()))
    print(f"[motion_filter] rot={n_rot} vec={n_vec} lin={n_lin}: worst rotation-matrix entry deviation {worst_r:.3e}, worst vector / scalar value "
          f"{worst_v:.3e} relative, {left_out} of {pairs} (row, channel) pairs undecidable (bounds {MARGIN * ROT_MEASURED:.1e}, {MARGIN * VEC_MEASURED:.1e})")
    assert MARGIN * ROT_MEASURED <= RESAMPLE_BOUND and MARGIN * VEC_MEASURED <= RESAMPLE_BOUND
    assert left_out <= C.MAX_UNDECIDABLE * pairs
    assert worst_r <= MARGIN * ROT_MEASURED
    assert worst_v <= MARGIN * VEC_MEASURED


def test_exact_properties():
    """bit for bit: R = 0 is the identity; all-zero weights return the input with used = 0; a row whose only used sample is its centre
    returns the input; clips concatenated with segment ids equal each clip filtered alone; two calls give equal bits"""
    rng = np.random.default_rng(21)
    n_rot, n_vec, n_lin = 17, 2, 3
    nch = n_rot + n_vec + n_lin
    off = (rng.normal(size=3 * n_rot) * 0.2).astype(np.float32)
    rows = C.make_rows(rng, 64, n_rot, n_vec, n_lin, off.astype(np.float64))
    taps = C.gaussian(2.0, 6)
    trim = np.full(nch, C.TRIM, np.float32)
    # R = 0
    out, used = _filter(rows, n_rot, n_vec, [1.0], rot_offset=off, trim=trim)
    assert torch.equal(_bits(out), _bits(torch.as_tensor(rows))) and bool((used == 1).all())
    # all-zero weights (and negatives, NaN: they count as zero)
    for w in (np.zeros(64, np.float32), np.zeros((64, nch), np.float32), np.full(64, -1.0, np.float32), np.full((64, nch), np.nan, np.float32)):
        out, used = _filter(rows, n_rot, n_vec, taps, weights=w, rot_offset=off, trim=trim)
        assert torch.equal(_bits(out), _bits(torch.as_tensor(rows))) and bool((used == 0).all())
    # the centre alone: every second row has a weight, R = 1, so each weighted row sees only itself and each other row two neighbours
    w = (np.arange(64) % 2 == 0).astype(np.float32)
    out, used = _filter(rows, n_rot, n_vec, C.gaussian(1.0, 1), weights=w, rot_offset=off)
    assert torch.equal(_bits(out[::2]), _bits(torch.as_tensor(rows[::2]))) and bool((used[::2] == 1).all())
    assert bool((used[1:-1:2] == 2).all()) and bool((used[-1] == 0).all())
    assert not torch.equal(_bits(out[1:-1:2]), _bits(torch.as_tensor(rows[1:-1:2])))
    # clips concatenated with segment ids (a single-row clip among them) against each clip alone
    lens, ids = (7, 1, 30, 2, 24), (3, 9, 3, -4, 0)
    seg = np.concatenate([np.full(n, i, np.int32) for n, i in zip(lens, ids)])
    wc = C.make_weights(rng, 64, nch, 6, True)
    both, used_b = _filter(rows, n_rot, n_vec, taps, weights=wc, segment=seg, rot_offset=off, trim=trim)
    lo = 0
    for n in lens:
        alone, used_a = _filter(rows[lo:lo + n], n_rot, n_vec, taps, weights=wc[lo:lo + n], rot_offset=off, trim=trim)
        assert torch.equal(_bits(alone), _bits(both[lo:lo + n])) and torch.equal(used_a, used_b[lo:lo + n]), (lo, n)
        lo += n
    again, used_2 = _filter(rows, n_rot, n_vec, taps, weights=wc, segment=seg, rot_offset=off, trim=trim)
    assert torch.equal(_bits(again), _bits(both)) and torch.equal(used_2, used_b)


def test_graph_replay_equals_the_eager_call():
    """ONE captured call of the C entry point (a single kernel node: it allocates nothing and has no second launch), replayed on fresh
    output buffers, equals the eager call"""
    from harp_amd import _lib
    rng = np.random.default_rng(22)
    n_rot, n_vec, n_lin, T, R = 16, 1, 3, 257, 6
    nch, W = n_rot + n_vec + n_lin, 3 * (n_rot + n_vec) + n_lin
    off = (rng.normal(size=3 * n_rot) * 0.2).astype(np.float32)
    rows = C.make_rows(rng, T, n_rot, n_vec, n_lin, off.astype(np.float64))
    w, trim, taps = C.make_weights(rng, T, nch, R, False), np.full(nch, C.TRIM, np.float32), C.gaussian(2.0, R)
    eager, used_e = _filter(rows, n_rot, n_vec, taps, weights=w, rot_offset=off, trim=trim)
    d_rows, d_off, d_taps, d_w, d_trim = _dev(rows), _dev(off), _dev(np.array(taps, np.float32)), _dev(w), _dev(trim)
    out, used = torch.empty(T, W, device=DEV), torch.empty(T, nch, dtype=torch.int32, device=DEV)
    p = _lib.ptr

    def launch():
        assert _lib.lib().harp_motion_filter(p(d_rows), T, n_rot, n_vec, n_lin, p(d_off), p(d_taps), R, p(d_w), 1, None, p(d_trim), 2, p(out), p(used),
                                             _lib.stream()) == 0

    launch()                                              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        out.fill_(-1.0)
        used.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(eager)) and torch.equal(used, used_e)


def test_binding_checks():
    from harp_amd import ops
    r = torch.zeros(6, 10, device=DEV)                    # 2 rotations, 1 vector, 1 scalar
    ok = dict(n_rot=2, n_vec=1, taps=[1.0, 0.5])
    ops.motion_filter(r, **ok)
    with pytest.raises(RuntimeError):
        ops.motion_filter(r.cpu(), **ok)
    with pytest.raises(RuntimeError):
        ops.motion_filter(r.clone().requires_grad_(), **ok)
    with pytest.raises(TypeError):
        ops.motion_filter(r.double(), **ok)
    with pytest.raises(TypeError):
        ops.motion_filter(r, segment=torch.zeros(6, dtype=torch.int64, device=DEV), **ok)
    with pytest.raises(TypeError):
        ops.motion_filter(r, 2, 1, torch.ones(2, device=DEV))
    for bad in (dict(n_rot=3, n_vec=1), dict(n_rot=-1), dict(weights=torch.ones(5, device=DEV)), dict(weights=torch.ones(6, 3, device=DEV)),
                dict(segment=torch.zeros(5, dtype=torch.int32, device=DEV)), dict(trim=torch.zeros(3, device=DEV)),
                dict(rot_offset=torch.zeros(5, device=DEV)), dict(iters=9), dict(iters=-1), dict(taps=[0.0, 1.0]), dict(taps=[1.0, float("nan")]),
                dict(taps=[1.0] * 66)):
        with pytest.raises(ValueError):
            ops.motion_filter(r, **dict(ok, **bad))


def test_manifold_properties():
    """track 1: a constant rotation written alternately as a triple and its 2 pi complement returns that rotation; track 2: a
    constant-velocity track R0 exp(t w), |w| = 0.05 rad per frame, under a symmetric Gaussian window with unit weights returns itself (ends
    included: the window shrinks symmetrically); track 3: affine vector and scalar tracks return themselves"""
    rng = np.random.default_rng(23)
    T, taps = 64, C.gaussian(2.0, 6)
    # 1: six rotations of 0.5 .. 6 rad
    axis = rng.normal(size=(6, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    const = axis * np.array([0.5, 1.5, 3.0, np.pi - 1e-3, 4.0, 6.0])[:, None]
    track = np.where((np.arange(T) % 2 == 1)[:, None, None], C.complement(const)[None], const[None]).astype(np.float32).reshape(T, 18)
    assert float(np.abs(track[1] - track[0]).max()) > 1.0                  # (the numbers do alternate)
    out, used = _filter(track, 6, 0, taps)
    d1 = float(np.abs(rotation_matrix(out.cpu().numpy().astype(np.float64).reshape(T, 6, 3)) - rotation_matrix(track.astype(np.float64).reshape(T, 6, 3))).max())
    assert bool((used[6:-6] == 13).all())
    # 2: R0 exp(t w) as quaternions, written as axis-angle with an angle in [0, pi]
    w = rng.normal(size=(4, 3))
    w = 0.05 * w / np.linalg.norm(w, axis=-1, keepdims=True)
    q0 = quat_of(rng.normal(size=(4, 3)))
    q = F.qmul(q0[None], quat_of(np.arange(T)[:, None, None] * w[None]))
    geo = F.qlog(q).astype(np.float32).reshape(T, 12)
    out, _ = _filter(geo, 4, 0, taps)
    d2 = float(np.abs(rotation_matrix(out.cpu().numpy().astype(np.float64).reshape(T, 4, 3)) - rotation_matrix(geo.astype(np.float64).reshape(T, 4, 3))).max())
    # 3: two vectors and three scalars, affine in t
    a, b = rng.normal(size=(1, 9)), rng.normal(size=(1, 9)) * 0.05
    aff = (a + b * np.arange(T)[:, None]).astype(np.float32)
    out, _ = _filter(aff, 0, 2, taps)
    d3 = float((np.abs(out.cpu().numpy().astype(np.float64) - aff) / np.abs(aff).max(0)).max())
    print(f"[motion_filter] manifold: 2 pi complements {d1:.3e}, constant velocity {d2:.3e} (rotation-matrix entry), affine tracks {d3:.3e} relative "
          f"(bounds {MARGIN * COMPLEMENT_MEASURED:.1e}, {MARGIN * GEODESIC_MEASURED:.1e}, {MARGIN * AFFINE_MEASURED:.1e})")
    assert d1 <= MARGIN * COMPLEMENT_MEASURED
    assert d2 <= MARGIN * GEODESIC_MEASURED
    assert d3 <= MARGIN * AFFINE_MEASURED


def test_spike_and_gap():
    """a 64-frame smooth rotation track with 0.02 rad noise and two one-frame spikes of about 1 rad, sigma = 2, R = 6, trim = 0.5: the
    trimmed output's worst error against the clean track is no larger than that of filtering the spike-free noisy track and below the noisy
    input's own; untrimmed it is several times worse.  A keypoint track with a joint missing for 3 frames comes back finite there."""
    from harp_amd.playback import smooth_keypoints
    clean, noisy, spiky = C.spike_track()
    taps = C.gaussian(2.0, 6)
    run = lambda rows, trim: _filter(rows, 1, 0, taps, trim=trim)[0].cpu().numpy().astype(np.float64)      # noqa: E731
    err = lambda a: float(_angle(a, clean.astype(np.float64)).max())                                        # noqa: E731
    tr = np.array([0.5], np.float32)
    e_trim, e_free, e_noisy, e_untrimmed = err(run(spiky, tr)), err(run(noisy, None)), err(noisy.astype(np.float64)), err(run(spiky, None))
    print(f"[motion_filter] spikes: worst error against the clean track — trimmed {e_trim:.4f}, spike-free filtered {e_free:.4f}, noisy input "
          f"{e_noisy:.4f}, untrimmed {e_untrimmed:.4f} rad")
    assert e_trim <= e_free
    assert e_trim < e_noisy
    assert e_untrimmed > 2.0 * e_trim
    rng = np.random.default_rng(24)
    T = 16
    track = rng.normal(size=(1, 21, 3)) * 0.05 + 0.002 * np.arange(T)[:, None, None]      # affine: the filter reproduces it, what is left is noise
    kp = (track + rng.normal(size=(T, 21, 3)) * 1e-3).astype(np.float32)
    gone = kp.copy()
    gone[6:9, 7] = np.nan
    out, used = smooth_keypoints(gone, sigma=2.0, device=DEV)
    assert tuple(out.shape) == (T, 21, 3) and bool(torch.isfinite(out).all()) and bool((used[6:9, 7] > 0).all())
    assert int(used[7, 7]) == 13 - 3 and int(used[7, 8]) == 13
    # frame 7's window is symmetric without its three missing rows, so the affine track drops out there (6 and 8 lean to one side)
    fill = float((out[7, 7].cpu().double() - torch.as_tensor(track[7, 7])).norm())
    a = np.array([t for d, t in enumerate(taps) for _ in range(2) if d >= 2])      # the middle frame's window without its three missing rows
    sigma = 1e-3 * np.sqrt((a * a).sum()) / a.sum()      # of one coordinate of the weighted mean of 1 mm noise: 0.44 mm
    print(f"[motion_filter] gap: the middle of a joint's 3 missing frames is filled within {1e3 * fill:.3f} mm of its noise-free track (4 sigma sqrt 3 = {4e3 * sigma * np.sqrt(3):.3f} mm)")
    assert fill <= 4.0 * sigma * np.sqrt(3.0)


def test_through_the_layer(tmp_path):
    """the synthetic hand of tests/test_gpu_ik.py's layer test: a smooth 24-frame motion -> keypoints + 1 mm of noise ->
    Motion.from_keypoints(smooth=2.0) shakes less (motion_jitter) than without, and its joints stay within the recorded distance of the
    clean motion's; smooth=None is today's motion bit for bit; Motion.smooth -> AvatarPlayer.render runs at S = 32"""
    from harp_amd.playback import AvatarPlayer, Motion, motion_jitter
    from tests.test_gpu_evaluate import _setup
    T, S = 24, 32
    _, cfg, layer, params, _ = _setup(5, S, 3, tmp_path)
    base = Motion.from_params(params)
    t = torch.linspace(0, 1, T)[:, None]
    mix = lambda a, b: (1 - t) * a[None] + t * b[None] + 0.05 * torch.sin(6.28 * t) * (b - a)[None]      # noqa: E731
    clean = Motion(mix(base.pose[0].cpu(), base.pose[1].cpu()), mix(base.rot[0].cpu(), base.rot[1].cpu()), mix(base.trans[0].cpu(), base.trans[1].cpu()),
                   base.cam[0:1].cpu().expand(T, 3))
    betas = params["shape"].detach().reshape(1, 10).expand(T, 10).contiguous()
    with torch.no_grad():
        joints = layer(torch.cat([clean.rot, clean.pose], 1).to(DEV), betas, clean.trans.to(DEV))[1]
    g = torch.Generator().manual_seed(5)
    noisy = joints / 1000.0 + (torch.randn(T, 21, 3, generator=g) * 1e-3).to(DEV)
    plain = Motion.from_keypoints(noisy, params, layer)
    same = Motion.from_keypoints(noisy, params, layer, smooth=None)
    for k in ("pose", "rot", "trans", "cam"):
        assert torch.equal(_bits(getattr(plain, k)), _bits(getattr(same, k))), k
    smooth = Motion.from_keypoints(noisy, params, layer, smooth=2.0)
    j_clean, j_plain = motion_jitter(clean, params, layer), motion_jitter(plain, params, layer, other=clean)
    j_smooth = motion_jitter(smooth, params, layer, other=clean)
    print(f"[motion_filter] layer: joint acceleration mean / max (mm per frame^2) clean {j_clean['accel_mean_mm']:.3f} / {j_clean['accel_max_mm']:.3f}, "
          f"solved from noisy keypoints {j_plain['accel_mean_mm']:.3f} / {j_plain['accel_max_mm']:.3f}, with smooth=2 {j_smooth['accel_mean_mm']:.3f} / "
          f"{j_smooth['accel_max_mm']:.3f}; largest joint distance to the clean motion {j_plain['disp_max_mm']:.3f} -> {j_smooth['disp_max_mm']:.3f} mm")
    assert j_smooth["accel_mean_mm"] < j_plain["accel_mean_mm"] and j_smooth["accel_max_mm"] < j_plain["accel_max_mm"]
    assert j_smooth["disp_max_mm"] <= MARGIN * LAYER_DIST_MEASURED_MM
    # a dropped joint is filled and then counts as used: the solve sees 21 points in every frame
    holes = noisy.clone()
    holes[10:13, 8] = float("nan")
    filled = Motion.from_keypoints(holes, params, layer, smooth=2.0)
    assert float((filled.pose - smooth.pose).abs().max()) < 0.1 and bool(torch.isfinite(filled.pose).all())
    # Motion.smooth on the solved rows, then the player
    sm = plain.smooth(layer, sigma=2.0, trim_rot=0.5, device=DEV)
    j_sm = motion_jitter(sm, params, layer)
    print(f"[motion_filter] layer: Motion.smooth(sigma=2) of the plain solve: joint acceleration mean {j_plain['accel_mean_mm']:.3f} -> {j_sm['accel_mean_mm']:.3f}")
    assert j_sm["accel_mean_mm"] < j_plain["accel_mean_mm"]
    keep = plain.smooth(layer, sigma=2.0, fields=["pose"], device=DEV)
    assert torch.equal(_bits(keep.rot), _bits(plain.rot)) and torch.equal(_bits(keep.trans), _bits(plain.trans)) and not torch.equal(keep.pose.cpu(), plain.pose.cpu())
    player = AvatarPlayer(cfg, params, layer, batch_size=8, ss=1, device=DEV)
    player.load_motion(sm)
    frames = player.render(np.arange(T))
    assert tuple(frames.shape) == (T, S, S, 3) and int((frames.cpu() != 255).any(-1).sum()) > 0


def test_command_line_takes_the_smoothing_flags(tmp_path, monkeypatch, capsys):
    """python -m harp_amd.playback's main() with --smooth, --smooth-trim and --smooth-keypoints on a handful of frames (the two loaders of
    licensed / fitted files replaced by the synthetic scene, as tests/test_gpu_ik.py does)"""
    import os
    import yaml
    from harp_amd import playback
    from harp_amd.utils import file_utils, hand_model_utils
    from tests.test_gpu_evaluate import _setup
    T, S = 5, 32
    _, cfg, layer, params, _ = _setup(T, S, 3, tmp_path)
    monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda c: (layer, params["verts_uvs"], params["faces_uvs"], None))
    monkeypatch.setattr(file_utils, "load_result", lambda base, device="cuda", test=False: dict(params))
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump({k: cfg[k] for k in ("use_arm", "img_size", "focal_length", "self_shadow", "share_light_position", "base_output_dir")}, f)
    true = playback.Motion.from_params(params)
    true.save(tmp_path / "motion.npz")
    with torch.no_grad():
        kp = layer(torch.cat([true.rot, true.pose], 1).to(DEV), params["shape"].detach().reshape(1, 10).expand(T, 10).contiguous(), true.trans.to(DEV))[1] / 1000.0
    np.savez(tmp_path / "kp.npz", keypoints=kp.cpu().numpy(), cam=true.cam.cpu().numpy())
    common = ["--config", str(tmp_path / "cfg.yaml"), "--batch-size", "4"]
    paths = playback.main(common + ["--out", str(tmp_path / "a"), "--motion", str(tmp_path / "motion.npz"), "--smooth", "1.5", "--smooth-trim", "0.5",
                                    "--fps-scale", "2"])
    assert len(paths) == 2 * T - 1 and "smoothed 5 frames" in capsys.readouterr().out
    paths = playback.main(common + ["--out", str(tmp_path / "b"), "--keypoints", str(tmp_path / "kp.npz"), "--smooth-keypoints", "1.0", "--smooth", "1.0"])
    assert sorted(os.listdir(tmp_path / "b")) == ["%04d.jpg" % i for i in range(T)] and len(paths) == T
    for bad in (["--motion", str(tmp_path / "motion.npz"), "--smooth-trim", "0.5"], ["--motion", str(tmp_path / "motion.npz"), "--smooth-keypoints", "1.0"],
                ["--motion", str(tmp_path / "motion.npz"), "--smooth", "0"]):
        with pytest.raises(SystemExit):
            playback.main(common + ["--out", str(tmp_path / "c")] + bad)
