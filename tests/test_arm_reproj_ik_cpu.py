"""No GPU: the image-keypoint playback of the SMPL-X arm.  The yardstick of tests/_arm_reproj_ik_ref.py against itself — its
projection against the player's camera, its Jacobian against central differences on both synthetic arm models, the exact zeros of the
elbow's rows and of d d / d trans, the prototype's table on the three seeded scenes, the float32 emulation of a step — the caps that the
GPU tests rest on (the committed scene leaves no problem out of the one-step test and at most 0 / 2 of 8 frames out of the full solve),
the argument errors of harp_arm_reproj_ik, which return before any launch, the options struct's layout, the argument errors of
Motion.from_arm_image_keypoints and the command line.  Every test prints its figures before it asserts."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import _arm_ik_ref as A
from tests import _arm_reproj_ik_ref as R
from tests import _ik_ref
from tests import _reproj_ik_ref as P

SEEDS = (0, 1, 2)
T = 24


@pytest.fixture(scope="module")
def arm():
    return dict(model=A.arm_model()[1], model2=A.mean_model()[1])


@pytest.fixture(scope="module")
def runs():
    """the issue's table: 20 iterations from both starts of the layer, four cases, seeds 0 / 1 / 2"""
    out = {}
    for seed in SEEDS:
        sc = R.scene(T, seed)
        out[seed] = dict(sc=sc)
        for mode in R.MODES:
            c = R.case(sc, mode)
            out[seed][mode] = dict(case=c, **R.solve(sc, c, 20))
    return out


@pytest.fixture(scope="module")
def gpu_scene():
    """the committed scene of the GPU tests' steps and full solves, 40 iterations of the yardstick"""
    sc = R.scene(**R.GPU_SCENE)
    out = dict(sc=sc)
    for mode in ("pixels22", "depth22"):
        c = R.case(sc, mode)
        out[mode] = dict(case=c, **R.solve(sc, c, 40))
    return out


# ---- 1 .. 3: the yardstick's rows and Jacobian ---------------------------------------------------------------------------------------------
def test_projection_of_22_rows_is_the_players_and_the_hands_convention():
    """the 22 rows through project_pixels (the player's camera at the rasteriser's pixel centres, which tests/test_reproj_ik_cpu.py pins
    for 21) and through §30's formulas written out: one convention, the elbow's d included"""
    from harp_amd import playback
    sc = R.scene(3, 0)
    with torch.no_grad():
        p, Z = R.rows(sc["model"], sc["x_true"], sc["betas"], sc["cam"], sc["focal"], sc["S"])
    j = sc["targets"]
    assert tuple(p.shape) == (3, 22, 3)
    mine = playback.project_pixels(j.numpy(), sc["cam"].numpy(), sc["focal"], sc["S"])
    assert mine.shape == (3, 22, 3) and float(np.abs(mine - p.numpy()).max()) < 1e-10
    cam, focal, S = sc["cam"], sc["focal"], sc["S"]
    tz = 2.0 * focal / (S * cam[0] + 1e-9)
    u = S / 2.0 + focal * (j[..., 0] + cam[1]) / (j[..., 2] + tz)
    v = S / 2.0 + focal * (j[..., 1] + cam[2]) / (j[..., 2] + tz)
    d = j[..., 2] - j[:, :1, 2]
    err = float((torch.stack([u, v, d], -1) - p).abs().max())
    print(f"[arm_reproj_ik_cpu] projection against the formulas {err:.3e}; elbow d {p[:, R.ELBOW, 2].tolist()}")
    assert err < 1e-10 and float(p[:, R.ELBOW, 2].abs().min()) > 1e-3 and bool((p[:, 0, 2] == 0).all())
    # per-problem cams project like the shared one
    with torch.no_grad():
        p2, _ = R.rows(sc["model"], sc["x_true"], sc["betas"], sc["cam"][None].expand(3, 3).contiguous(), focal, S)
    assert torch.equal(p, p2)


@pytest.mark.parametrize("which", ["model", "model2"])
def test_jacobian_against_central_differences(arm, which):
    sc = R.scene(3, 5, model=arm[which])
    x = sc["x_true"].clone()
    x[1, :R.XT] = 0.0
    args = (sc["betas"], sc["cam"], sc["focal"], sc["S"])
    J = R.jacobian(sc["model"], x, *args)
    assert tuple(J.shape) == (3, 66, R.NX)
    h, worst = 1e-6, 0.0
    with torch.no_grad():
        for i in range(R.NX):
            e = torch.zeros(R.NX, dtype=torch.float64)
            e[i] = h
            d = (R.rows(sc["model"], x + e, *args)[0] - R.rows(sc["model"], x - e, *args)[0]).reshape(3, 66) / (2 * h)
            worst = max(worst, float((d - J[:, :, i]).abs().max()))
    scale = float(J.abs().max())
    print(f"[arm_reproj_ik_cpu] Jacobian vs central differences ({which}): {worst:.3e} of {scale:.3e}")
    # h = 1e-6 in float64: rounding 1e-16 |u| / h ~ 5e-8 on rows of ~ 450 px, truncation h^2 |u'''| ~ 1e-8; entries up to focal / Z ~ 2e3
    assert worst < 1e-6
    assert all(float(J[:, :, c].abs().max()) > 0 for c in range(R.NX))


@pytest.mark.parametrize("which", ["model", "model2"])
def test_elbow_and_trans_structure(arm, which):
    """the elbow is an ancestor of the centre joint: its three rows in the 48 wrist and finger columns are exactly 0; no depth row moves
    with trans; the wrist's own depth row never moves.  What the kernel must keep bit for bit."""
    sc = R.scene(6, 7, model=arm[which])
    J = R.jacobian(sc["model"], sc["x_true"], sc["betas"], sc["cam"], sc["focal"], sc["S"])
    e = slice(3 * R.ELBOW, 3 * R.ELBOW + 3)
    assert bool((J[:, e, R.XW:R.XT] == 0).all())
    assert bool((J[:, 2::3, R.XT:] == 0).all()) and bool((J[:, 2] == 0).all())
    assert float(J[:, e, :3].abs().max()) > 1.0           # ... while the root turns the elbow by pixels per radian
    assert bool((J[:, 0::3, R.XT] > 1e3).all()) and bool((J[:, 1::3, R.XT + 1] > 1e3).all())      # focal / Z pixels per metre of trans


# ---- 4, 5: the prototype's table and float32 -----------------------------------------------------------------------------------------------
# This run's own figures, seeds 0 / 1 / 2 (largest pixel error, frames within 2.4 px, 3-D median and largest, scaled condition worst / end):
#   pixels22      2.86 / 2.60 / 3.19 px; 21 / 22 / 20; 12.6 / 11.3 / 7.9 mm, up to 227 mm; <= 4.5e4
#   depth22       2.04 / 2.38 / 1.94 px; 24 / 24 / 24;  1.4 /  1.4 / 1.2 mm, <= 7.1 mm;   <= 1.3e5 / <= 4.3e4
#   pixels21held  2.13 / 2.94 / 3.18 px; 24 / 23 / 23;  7.3 /  7.0 / 6.0 mm, <= 87 mm;    <= 1.6e4
#   depth21held   1.48 / 2.35 / 1.65 px; 24 / 24 / 24;  2.1 /  1.8 / 2.7 mm, <= 7.7 mm;   <= 3.1e4 / <= 5.0e3
# The 22-wide rows are the issue's prototype to its digits.  The held rows differ from it a little: the layer takes the rest joints at the
# HELD wrist (the prototype took them at zero wrist), and with that start the prototype's one 3.9e6 transient (seed 1) does not occur.
TABLE = {"pixels22": dict(px=3.3, within=20, med=(7.0, 14.0), far=240.0, cond=5e4, end=5e4),
         "depth22": dict(px=2.4, within=24, med=(0.5, 1.6), far=7.5, cond=2.4e5, end=4.7e4),
         "pixels21held": dict(px=3.3, within=23, med=(5.0, 8.0), far=95.0, cond=2.1e4, end=2.1e4),
         "depth21held": dict(px=2.4, within=24, med=(0.5, 3.0), far=8.0, cond=5.3e4, end=7.5e4)}


def test_yardstick_reproduces_the_prototype(runs):
    for seed in SEEDS:
        sc = runs[seed]["sc"]
        for mode in R.MODES:
            out, b = runs[seed][mode], TABLE[mode]
            n = 21 if mode.endswith("held") else 22
            px, mm, _ = R.picked(sc, out["x"], out["cost"][-1], n)
            cond = out["cond"]
            print(f"[arm_reproj_ik_cpu] yardstick seed {seed} {mode}: largest pixel error {float(px.max()):.3f} px, {int((px <= 2.4).sum())} of "
                  f"{T} within 2.4; 3-D median {float(mm.median()):.2f} mm, largest {float(mm.max()):.1f} mm; cond <= {float(cond.max()):.3e}, "
                  f"last {float(cond[-1].max()):.3e}")
            assert bool((out["status"] >= 1).all())
            assert float(px.max()) <= b["px"] and int((px <= 2.4).sum()) >= b["within"]
            assert b["med"][0] <= float(mm.median()) <= b["med"][1] and float(mm.max()) <= b["far"]
            assert float(cond.max()) <= b["cond"] and float(cond[-1].max()) <= b["end"]
            assert float(cond.max()) < 2.0 ** 24              # the priors keep the float32 solve meaningful
            if mode.endswith("held"):                         # a held wrist comes back as it went in
                assert torch.equal(out["x"][:, R.XW:R.XP], out["case"]["x0"][:, R.XW:R.XP])


def test_float32_first_step(runs):
    """the first step from both starts with A, g, the scaling, the factorisation and both solves in float32 against float64 from the same
    J: the step's error relative to its largest entry stays under cond(scaled matrix) x 2^-24 on every one of the 576 problems.  The
    float32 half runs in a fixed order, the kernel's, on elementwise operations alone: through the machine's BLAS and LAPACK the same
    check came out at 0.8 of the bound on one machine and above it on another for the best-conditioned case (the held wrist with depth
    rows, cond 1.3e3 .. 2.2e3: the error there is rounding of order cond x 2^-24 itself, whatever the priors — raising them tenfold and
    a hundredfold moved cond and the error together, the ratio stayed 0.6 .. 1.1), which says nothing about the defaults.  In the fixed
    order the worst problem of each case is at 0.30 .. 0.72 of the bound (0.72: seed 0 depth21held, seed 2 pixels21held).  The defaults
    are kept: no prior had to be raised."""
    for seed in SEEDS:
        sc = runs[seed]["sc"]
        for mode in R.MODES:
            c = runs[seed][mode]["case"]
            d32, d64, cond = R.step_float32(sc["model"], c["x0"], sc["betas"], sc["cam"], sc["focal"], sc["S"], c["targets"], 1e-3,
                                            weights=c["weights"], depth_weights=c["depth_weights"], **c["kw"])
            err = (d32 - d64).abs().amax(1) / d64.abs().amax(1)
            print(f"[arm_reproj_ik_cpu] float32 first step seed {seed} {mode}: {float(err.max()):.3e} (cond {float(cond.min()):.3e} .. "
                  f"{float(cond.max()):.3e}), at most {float((err / (cond * 2.0 ** -24)).max()):.2f} of the bound")
            assert bool((err <= cond * 2.0 ** -24).all())
            assert float(err.max()) <= 1e-3                          # GPU test 2 has room for a step that agrees to three digits


def test_float32_step_of_the_prototypes_transient(runs):
    """The prototype's one badly conditioned step: seed 1, depth rows, the wrist held, from the starts the PROTOTYPE took (the rest joints
    at zero wrist; the layer takes them at the held wrist, and the transient does not occur from there: 3.0e4 at most, the table above).
    Redone here: the scaled matrix reaches 3.0e6 once, at iteration 3 of problem 30 — a step of 90 units that the iteration rejects —
    which stays below 2^24, and the float32 emulation of exactly that step is off by 2.7e-2 of its largest entry, under cond x 2^-24 =
    0.18.  The held-wrist case keeps the defaults."""
    sc, c = runs[1]["sc"], runs[1]["depth21held"]["case"]
    x0, _ = R.layer_start(sc, None, c["targets"][::2].numpy(), c["weights"][::2].numpy())
    x0 = x0.reshape(2 * T, R.NX).clone()
    x0[:, R.XW:R.XP] = c["x0"][:, R.XW:R.XP]
    c = dict(c, x0=x0, kw=dict(c["kw"], z_prior=x0[:, R.XZ].clone()))
    out = R.solve(sc, c, 20)
    k, p = divmod(int(out["cond"].argmax()), 2 * T)
    d32, d64, cond = R.step_float32(sc["model"], out["xs"][k], sc["betas"], sc["cam"], sc["focal"], sc["S"], c["targets"], out["lams"][k],
                                    weights=c["weights"], depth_weights=c["depth_weights"], **c["kw"])
    err = float((d32[p] - d64[p]).abs().max() / d64[p].abs().max())
    print(f"[arm_reproj_ik_cpu] the transient: cond {float(out['cond'].max()):.3e} at iteration {k} of problem {p} (accepted: "
          f"{bool(out['ok'][k, p])}), end {float(out['cond'][-1].max()):.3e}; float32 step off by {err:.3e}, bound {float(cond[p]) * 2.0 ** -24:.3e}")
    assert 1e6 < float(out["cond"].max()) < 2.0 ** 24 and float(cond[p]) == float(out["cond"].max())
    assert err <= float(cond[p]) * 2.0 ** -24


# ---- 6: the caps of the GPU tests ----------------------------------------------------------------------------------------------------------
def test_gpu_scene_first_step_counts_every_problem(gpu_scene):
    """GPU test 2 counts a problem when the yardstick's first step lowers its cost by more than 1e-3 relative: all 16, in both modes
    (the issue's prototype: at least 0.49)"""
    for mode in ("pixels22", "depth22"):
        c = gpu_scene[mode]["cost"]
        drop = (c[0] - c[1]) / c[0]
        print(f"[arm_reproj_ik_cpu] gpu scene {mode}: first step lowers the cost by {float(drop.min()):.3f} .. {float(drop.max()):.3f}")
        assert drop.numel() == 16 and bool((drop > 1e-3).all()) and bool(gpu_scene[mode]["ok"][0].all())


def test_gpu_scene_leaves_out_at_most_the_caps(gpu_scene):
    """GPU test 3 may leave out a frame only when the yardstick's own last accepted step (of 40 iterations, the candidate it picks) still
    lowered the cost by more than 1e-6 relative: 0 of 8 with depth rows, at most 2 of 8 with pixels only, on the committed seed 2 — the
    seed the issue names; no other had to be taken."""
    Tg = R.GPU_SCENE["T"]
    for mode, cap in (("pixels22", 2), ("depth22", 0)):
        out = gpu_scene[mode]
        pick = out["cost"][-1].reshape(Tg, 2).argmin(1)
        drop = out["last_drop"].reshape(Tg, 2)[torch.arange(Tg), pick]
        c20 = out["cost"][20].reshape(Tg, 2).amin(1)
        c40 = out["cost"][40].reshape(Tg, 2).amin(1)
        n = int((drop > 1e-6).sum())
        print(f"[arm_reproj_ik_cpu] gpu scene {mode}: {n} of {Tg} picked candidates still moving after 40 iterations; cost at 20 over cost "
              f"at 40 - 1 up to {float((c20 / c40 - 1).max()):.3e}")
        assert n <= cap


# ---- 7: refusals and layout ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def _tree(f, **kw):
    from harp_amd import _lib
    t = _lib.TreeModel()
    t.NV, t.NJ, t.NB, t.n_pose_in, t.center_joint, t.n_joints_out = 1026, 55, 20, 17, 21, 22
    for n in ("v_template", "shapedirs_T", "posedirs_T", "posedirs", "J_template", "J_dirs", "weights", "pose_mean", "parents", "pose_src", "joint_src"):
        setattr(t, n, f)
    for k, v in kw.items():
        setattr(t, k, v)
    return t


DEFAULT_OPT = [20, 1e-3, 40.0, 400.0, 100.0, 1, 0, 0, 2000.0, 448]


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: an entry point that lost a check would launch on them")
def test_arm_reproj_ik_argument_errors_without_a_launch(lib):
    """every refusal of the contract with FAKE pointers: a call that got as far as a launch would fault, so returning 1 shows it did not"""
    from harp_amd import _lib
    f = 1 << 20                                            # a fake device pointer, never dereferenced
    good = dict(m=_tree(f), betas=f, cam=f, targets=f, z_prior=f, N=2, in_pose=f, trans=f, cost=f, status=f)
    O = _lib.ArmReprojIkOptions

    def call(opt=None, **kw):
        a = dict(good, **kw)
        o = ctypes.byref(O(*DEFAULT_OPT)) if opt is None else opt
        m = None if a["m"] is None else ctypes.byref(a["m"])
        return lib.harp_arm_reproj_ik(m, a["betas"], a["cam"], a["targets"], None, None, None, None, a["z_prior"], a["N"], o, a["in_pose"],
                                      a["trans"], a["cost"], a["status"], None, None, None)

    for name in ("m", "betas", "cam", "targets", "in_pose", "trans", "cost", "status", "z_prior"):
        assert call(**{name: None}) == 1, name
    assert call(opt=ctypes.POINTER(O)()) == 1
    assert call(N=0) == 1 and call(N=-1) == 1
    nan, inf = float("nan"), float("inf")

    def with_(pos, v):
        o = list(DEFAULT_OPT)
        o[pos] = v
        return ctypes.byref(O(*o))

    assert call(opt=with_(0, -1)) == 1
    for pos in (1, 2, 3, 4, 8):                            # lambda0, the three prior weights, focal
        for bad in (-1.0, nan, inf, -inf):
            assert call(opt=with_(pos, bad)) == 1, (pos, bad)
    assert call(opt=with_(8, 0.0)) == 1
    for S in (0, -448):
        assert call(opt=with_(9, S)) == 1, S
    for kw in (dict(n_joints_out=0), dict(n_joints_out=23), dict(center_joint=-1), dict(center_joint=55), dict(n_pose_in=16), dict(NB=9),
               dict(NB=33), dict(NJ=65)):
        assert call(m=_tree(f, **kw)) == 1, kw
    assert ctypes.sizeof(O) == 40 and lib.harp_arm_reproj_ik_frames_per_block() >= 1


def test_arm_reproj_ik_options_layout_matches_c(tmp_path):
    import os
    import subprocess
    from harp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [n for n, _ in _lib.ArmReprojIkOptions._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) +
                   '\\n", sizeof(harp_arm_reproj_ik_options),' + ",".join(f"offsetof(harp_arm_reproj_ik_options, {n})" for n in fields) +
                   "); return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.ArmReprojIkOptions)] + [getattr(_lib.ArmReprojIkOptions, n).offset for n in fields]
    assert fields == ["iters", "lambda0", "pose_prior_weight", "wrist_prior_weight", "z_prior_weight", "solve_wrist", "betas_per_frame",
                      "cam_per_frame", "focal", "S"]


def test_ops_arm_reproj_ik_signature():
    from harp_amd import ops
    p = inspect.signature(ops.arm_reproj_ik).parameters
    assert list(p) == ["dm", "betas", "targets", "in_pose", "trans", "cam", "focal", "S", "weights", "depth_weights", "prior", "wrist_prior",
                       "z_prior", "solve_wrist", "iters", "lambda0", "pose_prior_weight", "wrist_prior_weight", "z_prior_weight", "proj", "jac",
                       "out"]
    want = dict(weights=None, depth_weights=None, prior=None, wrist_prior=None, z_prior=None, solve_wrist=True, iters=20, lambda0=1e-3,
                pose_prior_weight=0.0, wrist_prior_weight=0.0, z_prior_weight=0.0, proj=False, jac=False, out=None)
    assert {k: p[k].default for k in want} == want
    assert ops.ArmReprojIkResult._fields == ("in_pose", "trans", "cost", "status", "proj", "jac")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.arm_reproj_ik(None, torch.zeros(10), torch.zeros(1, 22, 3), torch.zeros(1, 17, 3), torch.zeros(1, 3), torch.zeros(3), 2000.0, 448)


def test_from_arm_image_keypoints_signature_and_errors():
    from harp_amd import playback
    from harp_amd.playback import Motion
    p = inspect.signature(Motion.from_arm_image_keypoints).parameters
    assert list(p) == ["keypoints", "params", "arm_layer", "cam", "weights", "depth", "depth_weight", "prior_weight", "wrist_prior_weight",
                       "depth_prior_weight", "wrist_pose", "iters", "init", "smooth", "device", "configs"]
    assert (p["depth_weight"].default, p["prior_weight"].default, p["wrist_prior_weight"].default, p["depth_prior_weight"].default,
            p["iters"].default) == (1.0, 1e-5, 1e-4, 2.5e-5, 20)
    assert all(p[k].default is None for k in ("cam", "weights", "depth", "wrist_pose", "init", "smooth", "device", "configs"))
    for name in ("arm_image_ik_inputs", "arm_image_starts"):
        assert name in playback.__all__ and callable(getattr(playback, name))
    mano, armL = _ik_ref._Layer({"hands_mean": np.zeros(45)}), _ik_ref._Layer({"pose_mean": np.zeros(165)})
    cfg = dict(focal_length=2000.0, img_size=448)
    params = dict(cam=torch.tensor([[8.9, 0.0, 0.0]]).repeat(2, 1), shape=torch.zeros(10))
    kp = np.full((2, 22, 2), 224.0)
    with pytest.raises(ValueError, match="from_image_keypoints"):         # a MANO layer is not what it solves
        Motion.from_arm_image_keypoints(kp, params, mano, configs=cfg)
    # from_image_keypoints keeps refusing the arm, and now names the way
    with pytest.raises(NotImplementedError, match="from_arm_image_keypoints"):
        Motion.from_image_keypoints(kp[:, :21], params, armL, configs=cfg)
    with pytest.raises(ValueError, match="configs"):
        Motion.from_arm_image_keypoints(kp, params, armL)
    for bad in (np.zeros((2, 20, 2)), np.zeros((2, 23, 2)), np.zeros((22, 2)), np.zeros((2, 22, 3))):
        with pytest.raises(ValueError, match="keypoints"):
            Motion.from_arm_image_keypoints(bad, params, armL, configs=cfg)
    with pytest.raises(TypeError, match="keypoints"):
        Motion.from_arm_image_keypoints(np.zeros((2, 22, 2), np.int64), params, armL, configs=cfg)
    with pytest.raises(ValueError, match="weights"):
        Motion.from_arm_image_keypoints(kp, params, armL, weights=np.ones((2, 21)), configs=cfg)
    with pytest.raises(TypeError, match="weights"):
        Motion.from_arm_image_keypoints(kp[:, :21], params, armL, weights=np.ones((2, 21), np.int32), configs=cfg)
    with pytest.raises(ValueError, match="depth"):
        Motion.from_arm_image_keypoints(kp, params, armL, depth=np.zeros((2, 21)), configs=cfg)
    with pytest.raises(ValueError, match="wrist_pose"):
        Motion.from_arm_image_keypoints(kp, params, armL, wrist_pose=np.zeros((3, 3)), configs=cfg)
    with pytest.raises(ValueError, match="cam"):
        Motion.from_arm_image_keypoints(kp, params, armL, cam=np.zeros(4), configs=cfg)
    no_wrist = Motion(np.zeros((2, 45)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)))
    short = Motion(np.zeros((1, 45)), np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), wrist_pose=np.zeros((1, 3)))
    for init in (no_wrist, short):
        with pytest.raises(ValueError, match="wrist_pose"):
            Motion.from_arm_image_keypoints(kp, params, armL, init=init, configs=cfg)
    for name in ("depth_weight", "prior_weight", "wrist_prior_weight", "depth_prior_weight"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                Motion.from_arm_image_keypoints(kp, params, armL, configs=cfg, **{name: bad})


def test_arm_image_ik_inputs_widths_and_starts():
    """the host side: 21 wide is the 22-wide problem with the elbow unused and the wrist held; the starts put the palm near its pixels, and
    a per-frame wrist goes frame by frame to planar_palm_starts"""
    from harp_amd import playback
    sc = R.scene(4, 1)
    params = dict(cam=sc["cam"].float()[None], shape=sc["betas"].float())
    px = sc["rows"][..., :2].numpy()
    a22 = playback.arm_image_ik_inputs(px, None, sc["rows"][..., 2].numpy(), None, None, None, params)
    a21 = playback.arm_image_ik_inputs(px[:, :21], None, None, None, None, sc["x_true"][:, R.XW:R.XP].numpy(), params)
    assert a22["solve_wrist"] and not a21["solve_wrist"]
    assert a22["targets"].shape == a21["targets"].shape == (4, 22, 3) and a21["weights"].shape == (4, 22)
    assert np.all(a22["weights"] == 1) and np.all(a21["weights"][:, :21] == 1) and np.all(a21["weights"][:, 21] == 0)
    assert np.isnan(a21["targets"][:, 21]).all() and np.isnan(a21["targets"][..., 2]).all() and np.isfinite(a22["targets"]).all()
    assert np.array_equal(a21["in_pose"][:, 1], sc["x_true"][:, R.XW:R.XP].numpy()) and not a22["in_pose"].any() and not a21["trans"].any()
    for a, wrist in ((a22, None), (a21, sc["x_true"][:, R.XW:R.XP])):
        x0, zbar = R.layer_start(sc, wrist, a["targets"], a["weights"])
        with torch.no_grad():
            p, Z = R.rows(sc["model"], x0.reshape(8, R.NX), sc["betas"], sc["cam"], sc["focal"], sc["S"])
        err = (p[:, :21, :2] - sc["rows"].repeat_interleave(2, 0)[:, :21, :2]).norm(dim=-1).reshape(4, 2, 21)
        palm = err[:, :, list(playback.PALM)].amax(-1).amin(1)
        true_z = Z.reshape(4, 2, 22)[:, 0][:, list(playback.PALM)].mean(1)
        print(f"[arm_reproj_ik_cpu] starts: palm within {float(palm.max()):.2f} px, depth off by {float((zbar / true_z - 1).abs().max()):.2e}")
        # (the hand's bound, tests/test_reproj_ik_cpu.py PALM_BOUND_PX: weak perspective of a palm 0.1 m wide at 1 m, and it is not flat)
        # the depth is the start's own palm depth (to smplx's Rodrigues, which divides r by |r + 1e-8|: a rotation to ~1e-8 / |r| only)
        assert float(palm.max()) <= 20.0 and float((zbar / true_z - 1).abs().max()) < 1e-6
        assert float((x0[:, 0, :3] - x0[:, 1, :3]).norm(dim=-1).min()) > 1e-3


def test_command_line_describes_both_widths(capsys):
    from harp_amd.playback import cli
    common = ["--config", "c.yaml", "--out", "o"]
    assert cli.parse_args(common + ["--keypoints2d", "k.npz"]).keypoints2d == "k.npz"
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "from_arm_image_keypoints" in text and "(T,22,2)" in text and "(T,21,2)" in text and "elbow" in text
    assert "the MANO hand only" not in text
    src = inspect.getsource(cli.main)
    assert "from_arm_image_keypoints" in src and "from_image_keypoints" in src and 'opt("wrist_pose")' in src
