"""CPU checks of the image-keypoint playback: the projection convention of csrc/reproj_ik.hip pinned against the
rasteriser's pixel centres and the camera the player uses, the float64 yardstick of tests/_reproj_ik_ref.py against itself (Jacobian
against central differences, the prototype's figures on the three seeded scenes, the float32 emulation of one step), the host side of
Motion.from_image_keypoints (harp_amd/playback/keypoints.py: the two planar starts, argument errors) and harp_mano_reproj_ik's argument
errors, which return before any launch.  Every test prints its figures before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _ik_ref as R3
from tests import _reproj_ik_ref as R

SEEDS = (0, 1, 2)
T = 24


def _solve(sc, mode, iters, **kw):
    """the issue's run: both planar starts (48 problems, frame-major), pose prior 40 px^2/rad^2, trans_z prior 100 px^2/m^2"""
    x0, zbar = R.planar_x0(sc)
    xs = x0.reshape(2 * T, 51)
    tg = sc["rows"].repeat_interleave(2, 0).clone()
    dw = None
    if mode == "pixels":
        tg[..., 2] = float("nan")
    else:
        dw = ((sc["focal"] / zbar) ** 2).repeat_interleave(2)[:, None].expand(2 * T, 21).contiguous()
    out = R.lm(sc["model"], xs, sc["betas"], sc["cam"], sc["focal"], sc["S"], tg, depth_weights=dw, pose_prior_weight=R.POSE_PRIOR_PX,
               z_prior=xs[:, 50].clone(), z_prior_weight=R.Z_PRIOR_PX, iters=iters, conds=True, **kw)
    out["x0"], out["targets"], out["depth_weights"] = xs, tg, dw
    return out


def _picked(sc, x, cost):
    """per frame the candidate with the lower cost: its largest pixel error (T,), its joint errors in mm (T,21), and the pick"""
    pick = cost.reshape(T, 2).argmin(1)
    xf = x.reshape(T, 2, 51)[torch.arange(T), pick]
    with torch.no_grad():
        p, _ = R.rows(sc["model"], xf, sc["betas"], sc["cam"], sc["focal"], sc["S"])
        j = R3.joints(sc["model"], xf, sc["betas"])
    return (p[..., :2] - sc["rows"][..., :2]).norm(dim=-1).amax(1), (j - sc["targets"]).norm(dim=-1) * 1000, pick


@pytest.fixture(scope="module")
def runs():
    """seed 0 (the GPU tests' scene): 40 iterations with their history; seeds 1 and 2: the 20 of the prototype"""
    out = {}
    for seed in SEEDS:
        sc = R.scene(T, seed)
        out[seed] = dict(sc=sc, **{m: _solve(sc, m, 40 if seed == 0 else 20, history=(seed == 0)) for m in ("pixels", "depth")})
    return out


def test_projection_convention_against_the_camera_and_the_pixel_centres():
    """u = S/2 + focal (x + cam1) / Z is the player's camera (R = diag(-1,-1,1), T = (-cam1, -cam2, t_z), tests/_chain_ref.project =
    ops.project's restatement) read at the rasteriser's pixel centres (oracle/p3d_like.pixel_centers): x_ndc = 1 - 2 u / S, the centre of
    column i at u = i + 0.5, u with the column and v with the row — and the oracle's rasteriser covers pixel [floor(v), floor(u)]."""
    from harp_amd import playback
    from oracle import p3d_like as P
    from tests import _chain_ref as C
    rng = np.random.default_rng(0)
    S, focal = 16, 60.0
    cam = np.array([7.0, 0.013, -0.021])
    j = rng.uniform(-0.03, 0.03, size=(1, 21, 3))
    rows = playback.project_pixels(j, cam, focal, S)
    mine, _ = R.project(torch.as_tensor(j), torch.as_tensor(cam), focal, S)
    assert float((torch.as_tensor(rows) - mine).abs().max()) < 1e-12
    Rm = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=torch.float64))[None]
    Tv = torch.tensor([[-cam[1], -cam[2], 2 * focal / (S * cam[0] + 1e-9)]], dtype=torch.float64)
    ndc = C.project(torch.as_tensor(j), Rm, Tv, S, focal)
    assert float((ndc[..., 0] - (1.0 - 2.0 * mine[..., 0] / S)).abs().max()) < 1e-12
    assert float((ndc[..., 1] - (1.0 - 2.0 * mine[..., 1] / S)).abs().max()) < 1e-12
    assert float((ndc[..., 2] - (torch.as_tensor(j)[..., 2] + Tv[0, 2])).abs().max()) < 1e-12
    i = torch.arange(S, dtype=torch.float64)
    assert float((P.pixel_centers(S, torch.float64) - (1.0 - 2.0 * (i + 0.5) / S)).abs().max()) < 1e-15
    # a small triangle around a joint's ndc covers exactly the pixel that holds (u, v): x with the column, y with the row
    for k in (0, 7, 20):
        u, v = float(mine[0, k, 0]), float(mine[0, k, 1])
        assert 0 <= u < S and 0 <= v < S
        cu, cv = np.floor(u) + 0.5, np.floor(v) + 0.5            # that pixel's centre, in ndc:
        cx, cy = 1.0 - 2.0 * cu / S, 1.0 - 2.0 * cv / S
        e = 0.4 * 2.0 / S
        tri = torch.tensor([[[cx - e, cy - e, 1.0], [cx + e, cy - e, 1.0], [cx, cy + e, 1.0]]], dtype=torch.float64)
        p2f = P.rasterize_meshes(tri, torch.tensor([[0, 1, 2]]), S)[0][0, :, :, 0]
        hit = torch.nonzero(p2f >= 0)
        assert hit.tolist() == [[int(np.floor(v)), int(np.floor(u))]], (k, u, v, hit.tolist())


def test_yardstick_jacobian_against_central_differences():
    sc = R.scene(3, 0)
    x = sc["x_true"].clone()
    x[1, :48] = 0.0
    args = (sc["betas"], sc["cam"], sc["focal"], sc["S"])
    J = R.jacobian(sc["model"], x, *args)
    h, worst = 1e-6, 0.0
    with torch.no_grad():
        for i in range(51):
            e = torch.zeros(51, dtype=torch.float64)
            e[i] = h
            d = (R.rows(sc["model"], x + e, *args)[0] - R.rows(sc["model"], x - e, *args)[0]).reshape(3, 63) / (2 * h)
            worst = max(worst, float((d - J[:, :, i]).abs().max()))
    scale = float(J.abs().max())
    print(f"[reproj_ik] yardstick Jacobian vs central differences: {worst:.3e} of {scale:.3e}")
    # h = 1e-6 in float64: rounding 1e-16 |u| / h ~ 5e-8 on rows of ~ 450 px, truncation h^2 |u'''| ~ 1e-8; entries up to focal / Z ~ 2e3
    assert worst < 1e-6
    # the depth rows do not move with trans, the wrist's own never
    assert float(J[:, 2::3, 48:].abs().max()) == 0.0 and float(J[:, 2].abs().max()) == 0.0


PALM_BOUND_PX = 20.0          # measured 14.8 / 17.0 / 14.3 px on seeds 0 / 1 / 2 (weak perspective of a palm 0.1 m wide at 1 m, and it is not flat)


def test_planar_palm_starts(runs):
    from harp_amd import playback
    for seed in SEEDS:
        sc = runs[seed]["sc"]
        x0, zbar = R.planar_x0(sc)
        with torch.no_grad():
            p, Z = R.rows(sc["model"], x0.reshape(2 * T, 51), sc["betas"], sc["cam"], sc["focal"], sc["S"])
        err = (p[..., :2] - sc["rows"].repeat_interleave(2, 0)[..., :2]).norm(dim=-1).reshape(T, 2, 21)
        palm = err[:, :, list(R3.PALM)].amax(-1).amin(1)
        print(f"[reproj_ik] planar starts seed {seed}: palm {float(palm.min()):.2f} .. {float(palm.max()):.2f} px, all joints "
              f"{float(err.amax(-1).amin(1).min()):.1f} .. {float(err.amax(-1).amin(1).max()):.1f} px, depth {float(zbar.min()):.3f} .. {float(zbar.max()):.3f} m")
        assert float(palm.max()) <= PALM_BOUND_PX
        true_z = Z.reshape(T, 2, 21)[:, 0][:, list(R3.PALM)].mean(1)
        assert float((zbar / true_z - 1).abs().max()) < 1e-9          # depth is the start's own palm depth
        # the two starts are different rotations that put the palm on the same pixels to within the bound
        assert float((x0[:, 0, :3] - x0[:, 1, :3]).norm(dim=-1).min()) > 1e-3
    sc = runs[0]["sc"]
    px = sc["rows"][..., :2].numpy().copy()
    rest = playback.rest_chain_joints(sc["model_np"], sc["betas"].numpy())
    used = np.ones((T, 21), bool)
    used[1, 5] = False
    args = (rest, sc["cam"].numpy(), sc["focal"], sc["S"])
    full = playback.planar_palm_starts(px, np.ones((T, 21), bool), *args)
    held = playback.planar_palm_starts(px, used, *args)
    assert np.array_equal(held[0][1], full[0][0]) and np.array_equal(held[1][1], full[1][0]) and np.array_equal(held[0][2], full[0][2])
    used[0, 0] = False
    none = playback.planar_palm_starts(px, used, *args)
    assert not none[0][0].any() and not none[1][0].any() and np.isfinite(none[2]).all()


def test_yardstick_reproduces_the_prototype(runs):
    """what the float64 prototype of the issue showed, redone: 20 iterations from both planar starts, the lower final cost per frame.
    Figures of this run (all 24 frames counted, seeds 0 / 1 / 2):
      pixels only   largest joint error 2.34 / 2.43 / 3.56 px (at 40 iterations 2.19 / - / -), 24 / 23 / 23 frames within 2.4 px; 3-D joint
                    error median 7.6 / 6.6 / 6.0 mm, largest 45 / 59 / 89 mm (the mirror ambiguity); scaled condition <= 1.12e4
      depth rows    largest joint error 1.83 / 2.12 / 1.56 px; 3-D median 1.2 / 1.8 / 0.9 mm, largest 6.3 / 8.9 / 2.9 mm; scaled condition
                    <= 4.3e5 in transients, <= 2.2e4 at the end
    The issue's prototype ended every pixels-only frame within 2.4 px; this run, which adds the trans_z prior and picks by cost, leaves
    one frame of seeds 1 and 2 above it at 20 iterations (3.56 px at most): the bounds below are this run's."""
    for seed in SEEDS:
        sc = runs[seed]["sc"]
        for mode in ("pixels", "depth"):
            out = runs[seed][mode]
            x20, c20 = (out["xs"][20], out["cost"][20]) if seed == 0 else (out["x"], out["cost"][-1])
            px, mm, _ = _picked(sc, x20, c20)
            cond = out["cond"][:20]
            print(f"[reproj_ik] yardstick seed {seed} {mode}: largest pixel error {float(px.max()):.3f} px, {int((px <= 2.4).sum())} of {T} within 2.4; "
                  f"3-D median {float(mm.median()):.2f} mm, largest {float(mm.max()):.1f} mm; cond <= {float(cond.max()):.3e}, last {float(cond[-1].max()):.3e}")
            assert bool((out["status"] >= 1).all())
            if mode == "pixels":
                assert int((px <= 2.4).sum()) >= T - 1 and float(px.max()) <= 3.6
                assert 5.0 <= float(mm.median()) <= 20.0                # the reprojection is right, the 3-D pose is not unique
                assert float(cond.max()) <= 1.2e4
            else:
                assert float(px.max()) <= 2.2
                assert float(mm.median()) <= 2.3 and float(mm.max()) <= 10.0
                assert float(cond.max()) <= 7e5 and float(cond[-1].max()) <= 3e4


def test_yardstick_leaves_out_at_most_two_frames_on_the_gpu_scene(runs):
    """GPU test 3 may leave out a frame only when the yardstick's own last accepted step (of 40 iterations, the candidate it picks)
    still lowered the cost by more than 1e-6 relative: at most 2 of 24 on the committed seed"""
    for mode in ("pixels", "depth"):
        out = runs[0][mode]
        pick = out["cost"][-1].reshape(T, 2).argmin(1)
        drop = out["last_drop"].reshape(T, 2)[torch.arange(T), pick]
        n = int((drop > 1e-6).sum())
        print(f"[reproj_ik] yardstick seed 0 {mode}: {n} of {T} picked candidates still moving after 40 iterations")
        assert n <= 2


def test_float32_normal_equations_and_cholesky(runs):
    """the first step from the planar starts with A, g, the scaling, the factorisation and both solves in float32 against float64 from the
    same J: the step's error relative to its largest entry stays under cond(scaled matrix) x 2^-24 — the defaults survive float32.
    Measured 5.1e-5 / 9.4e-5 / 4.9e-5 (pixels) and 6.1e-5 / 7.9e-5 / 6.4e-5 (depth rows) on seeds 0 / 1 / 2."""
    for seed in SEEDS:
        sc = runs[seed]["sc"]
        for mode in ("pixels", "depth"):
            out = runs[seed][mode]
            d32, d64 = R.step_float32(sc["model"], out["x0"], sc["betas"], sc["cam"], sc["focal"], sc["S"], out["targets"], 1e-3,
                                      depth_weights=out["depth_weights"], pose_prior_weight=R.POSE_PRIOR_PX, z_prior=out["x0"][:, 50].clone(),
                                      z_prior_weight=R.Z_PRIOR_PX)
            err = (d32 - d64).abs().amax(1) / d64.abs().amax(1)
            cond = out["cond"][0]
            print(f"[reproj_ik] float32 step seed {seed} {mode}: {float(err.max()):.3e} (cond {float(cond.max()):.3e})")
            assert bool((err <= cond * 2.0 ** -24).all())
            assert float(err.max()) <= 1e-3                          # GPU test 2 has room for a step that agrees to four digits


def test_a_weak_pose_prior_loses_float32(runs):
    """the issue's second finding: with the pose prior at 1e-3 px^2/rad^2 instead of 40 the scaled matrix reaches 1e8 — past 1 / 2^-24"""
    sc, out = runs[0]["sc"], runs[0]["pixels"]
    x = out["xs"][10]
    J = R.jacobian(sc["model"], x, sc["betas"], sc["cam"], sc["focal"], sc["S"])
    W, _, _ = R.used_masks(out["targets"], None, None)
    A, _ = R.normal_equations(J, W, torch.zeros(2 * T, 21, 3, dtype=torch.float64), x, None, 1e-3, None, 0.0)
    cond = torch.linalg.cond(R.scaled(A, torch.full((2 * T,), 1e-9, dtype=torch.float64))[0])
    print(f"[reproj_ik] pose prior 1e-3: scaled condition up to {float(cond.max()):.3e}")
    assert float(cond.max()) > 2.0 ** 24


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: an entry point that lost a check would launch on them")
def test_mano_reproj_ik_argument_errors_without_a_launch(lib):
    from harp_amd import _lib
    f = 1 << 20
    mano = _lib.ManoModel(*([f] * len(_lib.ManoModel._fields_)))
    good = dict(m=ctypes.byref(mano), betas=f, cam=f, targets=f, weights=None, depth_weights=None, prior=None, z_prior=f, N=4, pose48=f, trans=f,
                cost=f, status=f, proj=None, jac=None)
    O = _lib.ReprojIkOptions
    default = O(20, 1e-3, 40.0, 100.0, 0, 0, 2000.0, 448)

    def call(opt=default, **kw):
        a = dict(good, **kw)
        o = None if opt is None else ctypes.byref(opt)
        return lib.harp_mano_reproj_ik(a["m"], a["betas"], a["cam"], a["targets"], a["weights"], a["depth_weights"], a["prior"], a["z_prior"],
                                       a["N"], o, a["pose48"], a["trans"], a["cost"], a["status"], a["proj"], a["jac"], None)

    for name in ("m", "betas", "cam", "targets", "pose48", "trans", "cost", "status", "z_prior"):
        assert call(**{name: None}) == 1, name
    assert call(opt=None) == 1
    for N in (0, -1):
        assert call(N=N) == 1, N
    assert call(O(-1, 1e-3, 40.0, 100.0, 0, 0, 2000.0, 448)) == 1
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert call(O(20, bad, 40.0, 100.0, 0, 0, 2000.0, 448)) == 1, ("lambda0", bad)
        assert call(O(20, 1e-3, bad, 100.0, 0, 0, 2000.0, 448)) == 1, ("pose_prior_weight", bad)
        assert call(O(20, 1e-3, 40.0, bad, 0, 0, 2000.0, 448)) == 1, ("z_prior_weight", bad)
        assert call(O(20, 1e-3, 40.0, 100.0, 0, 0, bad, 448)) == 1, ("focal", bad)
    assert call(O(20, 1e-3, 40.0, 100.0, 0, 0, 0.0, 448)) == 1
    for S in (0, -448):
        assert call(O(20, 1e-3, 40.0, 100.0, 0, 0, 2000.0, S)) == 1, S
    assert ctypes.sizeof(O) == 32 and lib.harp_mano_reproj_ik_frames_per_block() >= 1


def test_reproj_ik_options_layout_matches_c(tmp_path):
    import os
    import subprocess
    from harp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [n for n, _ in _lib.ReprojIkOptions._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu' + " %zu" * len(names)
                   + '\\n", sizeof(harp_reproj_ik_options),' + ",".join(f"offsetof(harp_reproj_ik_options, {n})" for n in names) + "); return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.ReprojIkOptions)] + [getattr(_lib.ReprojIkOptions, n).offset for n in names]


def test_from_image_keypoints_argument_errors():
    from harp_amd import ops
    from harp_amd.playback import Motion
    sc = R3.scene(T=4, seed=0)
    layer = R3._Layer(sc["model_np"])
    params = dict(shape=torch.zeros(10), cam=torch.tensor([[8.9, 0.0, 0.0]]).repeat(4, 1))
    cfg = dict(focal_length=2000.0, img_size=448)
    kp = np.full((4, 21, 2), 224.0)
    assert ops.ReprojIkResult._fields == ("pose48", "trans", "cost", "status", "proj", "jac")
    with pytest.raises(ValueError, match="configs"):
        Motion.from_image_keypoints(kp, params, layer)
    with pytest.raises(ValueError, match="keypoints"):
        Motion.from_image_keypoints(np.zeros((4, 21, 3)), params, layer, configs=cfg)
    with pytest.raises(ValueError, match="keypoints"):
        Motion.from_image_keypoints(np.zeros((21, 2)), params, layer, configs=cfg)
    with pytest.raises(TypeError, match="keypoints"):
        Motion.from_image_keypoints(np.zeros((4, 21, 2), np.int64), params, layer, configs=cfg)
    with pytest.raises(ValueError, match="weights"):
        Motion.from_image_keypoints(kp, params, layer, weights=np.ones((4, 20)), configs=cfg)
    with pytest.raises(TypeError, match="weights"):
        Motion.from_image_keypoints(kp, params, layer, weights=np.ones((4, 21), np.int32), configs=cfg)
    with pytest.raises(ValueError, match="depth"):
        Motion.from_image_keypoints(kp, params, layer, depth=np.zeros((4, 21, 1)), configs=cfg)
    with pytest.raises(ValueError, match="cam"):
        Motion.from_image_keypoints(kp, params, layer, cam=np.zeros((3, 3)), configs=cfg)
    with pytest.raises(ValueError, match="init"):
        Motion.from_image_keypoints(kp, params, layer, configs=cfg, init=Motion(np.zeros((3, 45)), np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))))
    for name in ("depth_weight", "prior_weight", "depth_prior_weight"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                Motion.from_image_keypoints(kp, params, layer, configs=cfg, **{name: bad})


def test_from_image_keypoints_refuses_the_arm():
    from harp_amd.playback import Motion
    sc = R3.scene(T=2, seed=0)
    arm = R3._Layer(dict(sc["model_np"], pose_mean=np.zeros(165)))
    with pytest.raises(NotImplementedError, match="SMPL-X arm"):
        Motion.from_image_keypoints(np.zeros((2, 21, 2)), dict(shape=torch.zeros(10), cam=torch.zeros(2, 3)), arm,
                                    configs=dict(focal_length=2000.0, img_size=448))


def test_command_line_takes_one_source():
    from harp_amd.playback import cli
    base = ["--config", "c.yaml", "--out", "o"]
    assert cli.parse_args(base + ["--keypoints2d", "k.npz"]).keypoints2d == "k.npz"
    for other in ("--keypoints", "--vertices", "--motion"):
        with pytest.raises(SystemExit):
            cli.parse_args(base + ["--keypoints2d", "k.npz", other, "x.npz"])
