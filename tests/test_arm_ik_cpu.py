"""No GPU: the yardstick of the SMPL-X arm inverse kinematics itself (tests/_arm_ik_ref.py: its Jacobian against central differences, the
structure of the elbow row, what the float64 iteration does from the layer's start in the three ways Motion.from_arm_keypoints calls the
solver, and that the one-step scenes of the GPU tests leave no frame out), the host side of the layer (arm_palm_start, rest_arm_joints,
the forearm-length rule), the signatures and argument errors of the Python entry points, the command line, and harp_arm_ik's argument
errors, which return before any launch."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import _arm_ik_ref as R
from tests import _ik_ref


@pytest.fixture(scope="module")
def arm():
    m_np, m, _ = R.arm_model()
    m2_np, m2 = R.mean_model()
    return dict(np=m_np, model=m, np2=m2_np, model2=m2)


# ---- (a) the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["model", "model2"])
def test_jacobian_against_central_differences(arm, which):
    sc = R.scene(T=2, seed=5, per_frame_betas=True, model=arm[which])
    x, b = sc["x_true"], sc["betas"]
    J = R.jacobian(sc["model"], x, b)
    assert tuple(J.shape) == (2, 66, R.NX)
    h = 1e-6
    worst = 0.0
    for c in range(R.NX):
        e = torch.zeros(R.NX, dtype=torch.float64)
        e[c] = h
        with torch.no_grad():
            fd = (R.joints(sc["model"], x + e, b) - R.joints(sc["model"], x - e, b)).reshape(2, -1) / (2 * h)
        worst = max(worst, float((fd - J[:, :, c]).abs().max()))
    scale = float(J.abs().max())
    print(f"[arm_ik_cpu] jacobian vs central differences ({which}) {worst:.3e} of {scale:.3e}")
    assert worst <= 1e-8 * scale                          # (h^2 f''' ~ 1e-12 and rounding 1e-16 / h ~ 1e-10, both of order one lever arm)
    assert all(float(J[:, :, c].abs().max()) > 0 for c in range(R.NX))
    assert torch.equal(J[0, :, R.XT:].reshape(22, 3, 3), torch.eye(3, dtype=torch.float64).expand(22, 3, 3))


@pytest.mark.parametrize("which", ["model", "model2"])
def test_elbow_row_structure(arm, which):
    """the elbow is an ancestor of the centre joint: only the root (and trans) move it, and its distance from the wrist is the shape's"""
    sc = R.scene(T=6, seed=7, model=arm[which])
    J = R.jacobian(sc["model"], sc["x_true"], sc["betas"])
    e = slice(3 * R.ELBOW, 3 * R.ELBOW + 3)
    assert bool((J[:, e, R.XW:R.XT] == 0).all())
    assert float(J[:, e, :3].abs().max()) > 1e-2 and bool((J[:, 0:3, :R.XT] == 0).all())      # the wrist row: trans only
    with torch.no_grad():
        j = R.joints(sc["model"], sc["x_true"], sc["betas"])
    d = (j[:, R.ELBOW] - j[:, 0]).norm(dim=-1)
    from harp_amd import playback
    rest = playback.rest_arm_joints(arm["np" if which == "model" else "np2"], sc["betas"].numpy())
    L = float(np.linalg.norm(rest[R.ELBOW] - rest[0]))
    print(f"[arm_ik_cpu] forearm ({which}) {d.tolist()} rest {L}")
    # (smplx's Rodrigues divides r by |r + 1e-8|: its matrices are rotations to 1e-8 / |r| only, so a bone keeps its length to ~1e-8 of it)
    assert float((d - L).abs().max()) < 1e-7 * L and L > 0.05
    # the mean of joints 17 and 19 turns the elbow about the wrist (model2), by far more than any bound of the GPU tests
    if which == "model2":
        with torch.no_grad():
            j1 = R.joints(arm["model"], sc["x_true"], sc["betas"])
        assert float((j1[:, R.ELBOW] - j[:, R.ELBOW]).norm(dim=-1).min()) > 1e-3
        assert float((j1[:, :R.ELBOW] - j[:, :R.ELBOW]).abs().max()) > 1e-6     # ... and the constant corrective rows move the tips


@pytest.mark.parametrize("case", ["22", "21", "22_no_elbow"])
def test_float64_yardstick_from_the_layers_start(arm, case):
    """24 of 24 frames reach the prior's floor within 15 iterations from the layer's start.  At the floor means: 15 FURTHER iterations
    together are no counted decrease (the cost falls by less than 1e-3 of itself, the threshold below which a step counts as a tie in
    the one-step tests) and move no frame's largest joint distance by more than 1 % of it; the floor itself is the priors' bias, which
    the float64 prototype put at 1.1 mm for the worst joint: the joints sit within 2 mm of their targets."""
    sc = R.scene(T=24, seed=0)
    w, kw, x0 = R.case(case, sc)
    y = R.lm(sc["model"], x0, sc["betas"], sc["targets"], iters=30, **kw)
    c15, c30 = y["cost"][15], y["cost"][30]
    mean, worst = R.joint_dist_mm(sc["model"], y["x"], sc["betas"], sc["targets"], w)
    with torch.no_grad():
        x15 = R.lm(sc["model"], x0, sc["betas"], sc["targets"], iters=15, **kw)["x"]
    mean15, worst15 = R.joint_dist_mm(sc["model"], x15, sc["betas"], sc["targets"], w)
    cond = y["cond"][:15]
    print(f"[arm_ik_cpu] {case}: accepted {y['accepted'].tolist()} joint distance after 15: mean {float(mean15.mean()):.3f} largest "
          f"{float(worst15.max()):.3f} mm (after 30: {float(worst.max()):.3f}); cost15/cost30 - 1 largest {float((c15 / c30 - 1).max()):.2e}; "
          f"condition of the scaled matrix {float(cond.min()):.1e} .. {float(cond.max()):.1e}")
    converged = ((c15 / c30 - 1.0) < 1e-3) & ((worst15 - worst).abs() <= 0.01 * worst)
    assert int(converged.sum()) == 24
    assert float(worst15.max()) < 2.0
    if case == "21":
        assert torch.equal(y["x"][:, R.XW:R.XP], sc["x_true"][:, R.XW:R.XP])


@pytest.mark.parametrize("name", sorted(R.ONE_STEP))
def test_gpu_scenes_leave_no_frame_out(name):
    sc = R.scene32(name, **R.ONE_STEP[name])
    counted, y1, y1_32 = R.counted_first_step(sc)
    print(f"[arm_ik_cpu] one-step scene {name}: counted {int(counted.sum())} of {counted.numel()}")
    T = R.ONE_STEP[name]["T"]
    assert counted.numel() == T and bool(counted.all())
    assert y1["accepted"].tolist() == [1] * T and y1_32["accepted"].tolist() == [1] * T
    if name == "22_priors":                               # the priors' share of the step is far above the one-step bounds
        kw0 = dict(sc["kw"], pose_prior_weight=0.0, wrist_prior_weight=0.0)
        y0 = R.lm(sc["model"], sc["x0_32"].double(), sc["betas32"].double(), sc["targets32"].double(), iters=1, **kw0)
        step = (y1["x"] - sc["x0_32"].double()).abs().amax(1)
        assert float(((y0["x"] - y1["x"]).abs().amax(1) / step).min()) > 1e-2


# ---- (b) the host side of the layer -------------------------------------------------------------------------------------------------------
def test_arm_palm_start_and_rest_joints(arm):
    from harp_amd import playback
    sc = R.scene(T=6, seed=3)
    b = sc["betas"]
    rest = playback.rest_arm_joints(arm["np"], b.numpy())
    assert rest.shape == (22, 3) and bool(np.isnan(rest[[4, 8, 12, 16, 20]]).all()) and bool(np.isfinite(np.delete(rest, [4, 8, 12, 16, 20], 0)).all())
    Jm = arm["np"]["J_template"].astype(np.float64) + arm["np"]["J_shapedirs"].astype(np.float64)[:, :, :10] @ b.numpy()
    assert np.allclose(rest[0], Jm[21], atol=1e-15) and np.allclose(rest[21], Jm[19], atol=1e-15) and np.allclose(rest[5], Jm[40], atol=1e-15)
    assert playback.ARM_JOINT_IDX[R.ELBOW] == 19 and playback.ELBOW == R.ELBOW
    # a pose with zero wrist and fingers is reproduced by the start exactly (up to rounding): rigid motion of palm and elbow
    x = sc["x_true"].clone()
    x[:, R.XW:R.XT] = 0.0
    with torch.no_grad():
        tg = R.joints(sc["model"], x, b)
    for width in (22, 21):
        x0 = R.layer_start(sc["model"], b, tg, width=width)
        with torch.no_grad():
            err = float((R.joints(sc["model"], x0, b) - tg).abs().max())
        assert err < 1e-7, (width, err)                   # (smplx's Rodrigues is a rotation to 1e-8 / |r| only; the Kabsch rotation is exact)
    # an unusable frame takes the last one that could be aligned; the elbow is left out where it is unused
    tg2 = tg.clone()
    tg2[2, [1, 5, 9, 13]] = float("nan")
    tg2[2, R.ELBOW] = float("nan")                        # two palm points left: no alignment
    tg2[4, R.ELBOW] = float("nan")                        # six left: aligned without the elbow
    x0 = R.layer_start(sc["model"], b, tg2)
    ref = R.layer_start(sc["model"], b, tg)
    assert torch.equal(x0[2], x0[1]) and float((x0[4] - ref[4]).abs().max()) < 1e-6 and torch.equal(x0[[0, 1, 3, 5]], ref[[0, 1, 3, 5]])


def test_forearm_length_rule(arm):
    """keypoints of a 1.3 x larger arm: the hand comes back at the model's size about the wrist, the elbow on its ray at the MODEL's forearm"""
    from harp_amd import playback
    sc = R.scene(T=5, seed=4)
    tg = sc["targets"].numpy()
    rest = playback.rest_arm_joints(arm["np"], sc["betas"].numpy())
    big = tg[:, :1] + 1.3 * (tg - tg[:, :1])
    used = np.ones((5, 22), bool)
    kp, scale = playback.match_arm_lengths(big, used, rest)
    # (the posed bones have the rest lengths to ~1e-8 of them: smplx's Rodrigues divides r by |r + 1e-8|)
    assert abs(scale - 1.0 / 1.3) < 1e-7 and np.allclose(kp, tg, atol=1e-7)
    # an elbow that is too far on its own (a longer forearm on a hand of the model's size) is pulled in along its ray only
    odd = tg.copy()
    odd[:, 21] = tg[:, 0] + 1.7 * (tg[:, 21] - tg[:, 0])
    kp, scale = playback.match_arm_lengths(odd, used, rest)
    assert abs(scale - 1.0) < 1e-7 and np.allclose(kp, tg, atol=1e-7)
    # a missing elbow or wrist: left as it came; 21 wide: the hand only
    gone = big.copy()
    gone[1, 21] = np.nan
    gone[3, 0] = np.nan
    u = np.isfinite(gone).all(-1)
    kp, _ = playback.match_arm_lengths(gone, u, rest)
    assert np.isnan(kp[1, 21]).all() and np.allclose(kp[1, :21], tg[1, :21], atol=1e-7)
    assert np.array_equal(kp[3, 1:], gone[3, 1:]) and np.isnan(kp[3, 0]).all()
    kp21, s21 = playback.match_arm_lengths(big[:, :21], used[:, :21], rest)
    assert kp21.shape == (5, 21, 3) and np.allclose(kp21, tg[:, :21], atol=1e-7)


# ---- (c) signatures, command line, argument errors ----------------------------------------------------------------------------------------
def test_ops_arm_ik_signature():
    from harp_amd import ops
    p = inspect.signature(ops.arm_ik).parameters
    assert list(p) == ["dm", "betas", "targets", "in_pose", "trans", "weights", "prior", "wrist_prior", "solve_wrist", "iters", "lambda0",
                       "pose_prior_weight", "wrist_prior_weight", "joints", "jac", "out"]
    want = dict(weights=None, prior=None, wrist_prior=None, solve_wrist=True, iters=15, lambda0=1e-3, pose_prior_weight=0.0,
                wrist_prior_weight=0.0, joints=False, jac=False, out=None)
    assert {k: p[k].default for k in want} == want
    assert ops.ArmIkResult._fields == ("in_pose", "trans", "cost", "status", "joints", "jac")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.arm_ik(None, torch.zeros(10), torch.zeros(1, 22, 3), torch.zeros(1, 17, 3), torch.zeros(1, 3))


def test_from_arm_keypoints_signature_and_errors():
    from harp_amd import playback
    from harp_amd.playback import Motion
    p = inspect.signature(Motion.from_arm_keypoints).parameters
    assert list(p) == ["keypoints", "params", "arm_layer", "cam", "weights", "match_bone_lengths", "iters", "prior_weight", "wrist_prior_weight",
                       "wrist_pose", "init", "device", "smooth"]
    assert p["iters"].default == 15 and p["prior_weight"].default == 1e-5 and p["wrist_prior_weight"].default == 1e-4
    assert p["match_bone_lengths"].default is True
    assert all(p[k].default is None for k in ("cam", "weights", "wrist_pose", "init", "device", "smooth"))
    for name in ("arm_palm_start", "rest_arm_joints", "match_arm_lengths"):
        assert name in playback.__all__ and callable(getattr(playback, name))
    mano, armL = _ik_ref._Layer({"hands_mean": np.zeros(45)}), _ik_ref._Layer({"pose_mean": np.zeros(165)})
    with pytest.raises(ValueError, match="from_keypoints"):  # a MANO layer is not what it solves
        Motion.from_arm_keypoints(np.zeros((1, 22, 3)), {}, mano)
    # from_keypoints keeps refusing the arm, and now names the way
    with pytest.raises(NotImplementedError, match="from_arm_keypoints"):
        Motion.from_keypoints(np.zeros((1, 21, 3)), {}, armL)
    params = dict(cam=torch.zeros(2, 3), shape=torch.zeros(10))
    for bad in (np.zeros((2, 20, 3)), np.zeros((2, 23, 3)), np.zeros((22, 3)), np.zeros((2, 22, 2))):
        with pytest.raises(ValueError, match="keypoints"):
            Motion.from_arm_keypoints(bad, params, armL)
    with pytest.raises(TypeError, match="keypoints"):
        Motion.from_arm_keypoints(np.zeros((2, 22, 3), np.int64), params, armL)
    with pytest.raises(ValueError, match="weights"):
        Motion.from_arm_keypoints(np.zeros((2, 22, 3)), params, armL, weights=np.ones((2, 21)))
    with pytest.raises(TypeError, match="weights"):
        Motion.from_arm_keypoints(np.zeros((2, 21, 3)), params, armL, weights=np.ones((2, 21), np.int32))
    with pytest.raises(ValueError, match="wrist_pose"):
        Motion.from_arm_keypoints(np.zeros((2, 21, 3)), params, armL, wrist_pose=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="cam"):
        Motion.from_arm_keypoints(np.zeros((2, 21, 3)), params, armL, cam=np.zeros(4))
    no_wrist = Motion(np.zeros((2, 45)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)))
    short = Motion(np.zeros((1, 45)), np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), wrist_pose=np.zeros((1, 3)))
    for init in (no_wrist, short):
        with pytest.raises(ValueError, match="wrist_pose"):
            Motion.from_arm_keypoints(np.zeros((2, 22, 3)), params, armL, init=init)


def test_smooth_keypoints_takes_the_elbow_row(monkeypatch):
    from harp_amd import ops, playback
    from tests.test_filter_cpu import _stub
    calls = []
    monkeypatch.setattr(ops, "motion_filter", _stub(calls))
    kp = np.random.default_rng(1).normal(size=(6, 22, 3))
    kp[2, 21] = np.nan
    out, used = playback.smooth_keypoints(kp, sigma=1.0, device="cpu", joints=22)
    c = calls[-1]
    assert (c["n_rot"], c["n_vec"]) == (0, 22) and c["rows"].shape == (6, 66) and c["weights"].shape == (6, 22) and c["weights"][2, 21] == 0
    assert tuple(out.shape) == (6, 22, 3) and tuple(used.shape) == (6, 22)
    with pytest.raises(ValueError):
        playback.smooth_keypoints(kp, device="cpu")       # 21 wide unless told


def test_command_line_describes_arm_keypoints(capsys):
    from harp_amd.playback import cli
    common = ["--config", "c.yaml", "--out", "o"]
    args = cli.parse_args(common + ["--keypoints", "k.npz", "--smooth-keypoints", "1.5"])
    assert args.keypoints == "k.npz" and args.smooth_keypoints == 1.5
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "from_arm_keypoints" in text and "(T,22,3)" in text and "elbow" in text
    assert "from_arm_keypoints" in inspect.getsource(cli.main)


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


def test_arm_ik_argument_errors_without_a_launch(lib):
    """every refusal of the contract with FAKE pointers: a call that got as far as a launch would fault, so returning 1 shows it did not"""
    from harp_amd import _lib
    f = 1 << 20                                            # a fake device pointer, never dereferenced
    good = dict(m=_tree(f), betas=f, targets=f, T=2, in_pose=f, trans=f, cost=f, status=f)
    O = _lib.ArmIkOptions

    def call(opt=None, **kw):
        a = dict(good, **kw)
        o = ctypes.byref(O(15, 1e-3, 0.0, 0.0, 1, 0)) if opt is None else opt
        m = None if a["m"] is None else ctypes.byref(a["m"])
        return lib.harp_arm_ik(m, a["betas"], a["targets"], None, None, None, a["T"], o, a["in_pose"], a["trans"], a["cost"], a["status"],
                               None, None, None)

    for name in ("m", "betas", "targets", "in_pose", "trans", "cost", "status"):
        assert call(**{name: None}) == 1, name
    assert call(opt=ctypes.POINTER(O)()) == 1
    assert call(T=0) == 1 and call(T=-1) == 1
    nan, inf = float("nan"), float("inf")
    assert call(opt=ctypes.byref(O(-1, 1e-3, 0.0, 0.0, 1, 0))) == 1
    for pos in range(1, 4):                               # lambda0 and the two prior weights
        for bad in (-1.0, nan, inf):
            o = [15, 1e-3, 0.0, 0.0, 1, 0]
            o[pos] = bad
            assert call(opt=ctypes.byref(O(*o))) == 1, (pos, bad)
    for kw in (dict(n_joints_out=0), dict(n_joints_out=23), dict(center_joint=-1), dict(center_joint=55), dict(n_pose_in=16), dict(NB=9),
               dict(NB=33), dict(NJ=65)):
        assert call(m=_tree(f, **kw)) == 1, kw
    assert ctypes.sizeof(O) == 24 and lib.harp_arm_ik_frames_per_block() >= 1 and _lib.ARM_IK_MAX_JOINTS == 22


def test_arm_ik_options_layout_matches_c(tmp_path):
    import os
    import subprocess
    from harp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [n for n, _ in _lib.ArmIkOptions._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) +
                   ' %d\\n", sizeof(harp_arm_ik_options),' + ",".join(f"offsetof(harp_arm_ik_options, {n})" for n in fields) +
                   ", HARP_ARM_IK_MAX_JOINTS); return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.ArmIkOptions)] + [getattr(_lib.ArmIkOptions, n).offset for n in fields] + [_lib.ARM_IK_MAX_JOINTS]
