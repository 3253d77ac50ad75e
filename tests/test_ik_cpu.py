"""CPU checks of the keypoint-driven playback: the float64 yardstick of tests/_ik_ref.py against itself (Jacobian against
central differences, convergence from the palm start), the host side of Motion.from_keypoints (harp_amd/playback/keypoints.py: Kabsch start, bone-length scale, argument
errors) and harp_mano_ik's argument errors, which return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _ik_ref as R


@pytest.fixture(scope="module")
def sc():
    return R.scene(T=24, seed=0)


def test_yardstick_jacobian_against_central_differences(sc):
    x = sc["x_true"][:3].clone()
    x[1, :48] = 0.0                                        # every joint at aa = 0 (the pose mean is still added to the fingers)
    J = R.jacobian(sc["model"], x, sc["betas"])
    h = 1e-6
    worst = 0.0
    with torch.no_grad():
        for i in range(51):
            e = torch.zeros(51, dtype=torch.float64)
            e[i] = h
            d = (R.joints(sc["model"], x + e, sc["betas"]) - R.joints(sc["model"], x - e, sc["betas"])).reshape(3, 63) / (2 * h)
            worst = max(worst, float((d - J[:, :, i]).abs().max()))
    scale = float(J.abs().max())
    print(f"yardstick Jacobian vs central differences: {worst:.3e} of {scale:.3e}")
    # central differences at h = 1e-6 in float64: truncation h^2 |j'''| ~ 1e-12 and rounding 1e-16 / h ~ 1e-10, on entries of ~0.1
    assert worst < 1e-8 * max(scale, 1.0)
    assert torch.equal(J[:, :, 48:].reshape(3, 21, 3, 3), torch.eye(3, dtype=torch.float64).expand(3, 21, 3, 3))


def test_yardstick_converges_from_the_palm_start(sc):
    x0 = R.palm_x0(sc)
    out = R.lm(sc["model"], x0, sc["betas"], sc["targets"], prior_weight=1e-5, iters=20)
    c10, c20 = out["cost"][10], out["cost"][20]
    print(f"sum of cost at 10 / 20 iterations: {float(c10.sum()):.5e} {float(c20.sum()):.5e}")
    assert float(((c10 - c20).abs() / c20).max()) < 1e-3
    with torch.no_grad():
        err = (R.joints(sc["model"], out["x"], sc["betas"]) - sc["targets"]).norm(dim=-1) * 1000
    print(f"joint error mm: mean {float(err.mean()):.3f} max {float(err.max()):.3f}")
    assert float(err.max()) < 2.0                          # the prior's bias (0.89 mm in the issue's run), far from a failed solve's 100s of mm
    assert int(out["accepted"].min()) >= 1
    # every first step from the palm start is a large decrease (GPU test 2 counts on it)
    assert bool(((out["cost"][0] - out["cost"][1]) / out["cost"][0] > 1e-3).all())


def test_kabsch_returns_a_rotation_on_a_mirrored_set():
    from harp_amd import playback
    rng = np.random.default_rng(0)
    P = rng.normal(size=(6, 3))
    P -= P.mean(0)
    Q = P * np.array([1.0, 1.0, -1.0])                     # a reflection: the unconstrained optimum has det -1
    Rm = playback.kabsch_rotation(P, Q)
    assert abs(np.linalg.det(Rm) - 1.0) < 1e-12 and np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12)
    Rt = R.axis_angle_to_matrix([0.3, -2.0, 1.1])
    got = playback.kabsch_rotation(P, P @ Rt.T)
    assert np.allclose(got, Rt, atol=1e-12)
    assert np.allclose(R.axis_angle_to_matrix(playback.axis_angle_of(Rt)), Rt, atol=1e-12)
    near_pi = R.axis_angle_to_matrix(np.array([0.6, 0.0, 0.8]) * (np.pi - 1e-9))
    assert np.allclose(R.axis_angle_to_matrix(playback.axis_angle_of(near_pi)), near_pi, atol=1e-9)


def test_palm_start_recovers_root_and_trans(sc):
    """the palm joints move with the root and trans only: the start reproduces them exactly, and a frame without its palm joints takes
    the previous frame's rotation"""
    x0 = R.palm_x0(sc)
    with torch.no_grad():
        j = R.joints(sc["model"], x0, sc["betas"])
    idx = list(R.PALM)
    assert float((j[:, idx] - sc["targets"][:, idx]).abs().max()) < 1e-9
    tg = sc["targets"].clone()
    tg[1, 5] = float("nan")
    x1 = R.palm_x0(sc, tg)
    assert torch.equal(x1[1, :3], x1[0, :3]) and torch.equal(x1[2], x0[2])
    tg[0, 0] = float("nan")
    assert torch.equal(R.palm_x0(sc, tg)[0, :3], torch.zeros(3, dtype=torch.float64))


def test_bone_length_scale(sc):
    from harp_amd import playback
    tg = sc["targets"].numpy()
    rest = playback.rest_chain_joints(sc["model_np"], sc["betas"].numpy())
    used = np.ones(tg.shape[:2], bool)
    assert abs(playback.bone_length_scale(tg, used, rest) - 1.0) < 1e-12          # chain bones do not depend on the pose
    big = tg[:, :1] + 1.2 * (tg - tg[:, :1])
    assert abs(playback.bone_length_scale(big, used, rest) - 1.0 / 1.2) < 1e-12
    assert playback.bone_length_scale(big, np.zeros_like(used), rest) == 1.0
    assert len(playback.CHAIN_BONES) == 15 and not any(b in (4, 8, 12, 16, 20) for _, b in playback.CHAIN_BONES)


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: an entry point that lost a check would launch on them")
def test_mano_ik_argument_errors_without_a_launch(lib):
    """HARP_ERR_ARG (1) for every listed error, with fake pointers that are never dereferenced (tests/test_abi.py's way): the model struct
    and the options are read on the host"""
    from harp_amd import _lib
    f = 1 << 20
    mano = _lib.ManoModel(*([f] * len(_lib.ManoModel._fields_)))
    good = dict(m=ctypes.byref(mano), betas=f, targets=f, weights=None, prior=None, T=4, pose48=f, trans=f, cost=f, status=f, joints=None, jac=None)

    default = _lib.IkOptions(15, 1e-3, 1e-5, 0)

    def call(opt=default, **kw):
        a = dict(good, **kw)
        o = None if opt is None else ctypes.byref(opt)
        return lib.harp_mano_ik(a["m"], a["betas"], a["targets"], a["weights"], a["prior"], a["T"], o, a["pose48"], a["trans"], a["cost"],
                                a["status"], a["joints"], a["jac"], None)

    for name in ("m", "betas", "targets", "pose48", "trans", "cost", "status"):
        assert call(**{name: None}) == 1, name
    assert call(opt=None) == 1
    for T in (0, -1):
        assert call(T=T) == 1, T
    assert call(_lib.IkOptions(-1, 1e-3, 0.0, 0)) == 1
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert call(_lib.IkOptions(15, bad, 0.0, 0)) == 1, ("lambda0", bad)
        assert call(_lib.IkOptions(15, 1e-3, bad, 0)) == 1, ("prior_weight", bad)
    assert ctypes.sizeof(_lib.IkOptions) == 16 and lib.harp_mano_ik_frames_per_block() >= 1


def test_ik_options_layout_matches_c(tmp_path):
    import os
    import subprocess
    from harp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(harp_ik_options),'
                   'offsetof(harp_ik_options, iters), offsetof(harp_ik_options, lambda0), offsetof(harp_ik_options, prior_weight),'
                   'offsetof(harp_ik_options, betas_per_frame)); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    o = _lib.IkOptions
    assert got == [ctypes.sizeof(o), o.iters.offset, o.lambda0.offset, o.prior_weight.offset, o.betas_per_frame.offset]


def test_from_keypoints_shape_and_type_errors(sc):
    from harp_amd.playback import Motion
    layer = R._Layer(sc["model_np"])
    params = dict(shape=torch.zeros(10), cam=torch.zeros(4, 3))
    kp = np.zeros((4, 21, 3))
    with pytest.raises(ValueError, match="keypoints"):
        Motion.from_keypoints(np.zeros((4, 20, 3)), params, layer)
    with pytest.raises(ValueError, match="keypoints"):
        Motion.from_keypoints(np.zeros((21, 3)), params, layer)
    with pytest.raises(TypeError, match="keypoints"):
        Motion.from_keypoints(np.zeros((4, 21, 3), np.int64), params, layer)
    with pytest.raises(ValueError, match="weights"):
        Motion.from_keypoints(kp, params, layer, weights=np.ones((4, 20)))
    with pytest.raises(TypeError, match="weights"):
        Motion.from_keypoints(kp, params, layer, weights=np.ones((4, 21), np.int32))
    with pytest.raises(ValueError, match="cam"):
        Motion.from_keypoints(kp, params, layer, cam=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="init"):
        Motion.from_keypoints(kp, params, layer, init=Motion(np.zeros((3, 45)), np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))))
    arm = R._Layer(dict(sc["model_np"], pose_mean=np.zeros(165)))
    with pytest.raises(NotImplementedError):
        Motion.from_keypoints(kp, params, arm)
