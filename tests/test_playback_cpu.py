"""CPU checks of the playback feature (harp_amd/playback/, csrc/playback.hip): the two entry points refuse empty sizes and NULL pointers
before any launch, a Motion survives its .npz, the module imports without the built library, and the float64 slerp that the GPU tests
measure against is the geodesic of rotation matrices."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _playback_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def test_entry_points_refuse_bad_arguments_without_launch(lib):
    """HARP_ERR_ARG (1) for sizes 0 / -1 and NULL pointers; `f` is a fake device pointer that no kernel may reach (an entry point without
    the check would fail its empty launch with status 2 + the HIP error, or need a device)"""
    f = 1 << 20
    ok = dict(keys=f, Tk=3, n_rot=2, n_lin=1, off=None, times=f, Tn=4, out=f)
    order = ("keys", "Tk", "n_rot", "n_lin", "off", "times", "Tn", "out")
    for bad in (dict(Tk=0), dict(Tk=-1), dict(Tn=0), dict(Tn=-1), dict(n_rot=-1), dict(n_lin=-1), dict(n_rot=0, n_lin=0), dict(keys=None),
                dict(times=None), dict(out=None)):
        a = dict(ok, **bad)
        assert lib.harp_motion_resample(*[a[k] for k in order], None) == 1, bad
    ok = dict(rgb=f, face_id=f, B=2, S=4, ss=2, bg=None, n_bg=0, bg_rows=None, bg_color=f, channels=3, out=f)
    order = ("rgb", "face_id", "B", "S", "ss", "bg", "n_bg", "bg_rows", "bg_color", "channels", "out")
    for bad in (dict(B=0), dict(B=-1), dict(S=0), dict(S=-1), dict(ss=0), dict(ss=5), dict(ss=-1), dict(channels=2), dict(channels=5), dict(rgb=None),
                dict(face_id=None), dict(out=None), dict(bg_color=None), dict(bg=f, n_bg=0), dict(bg=f, n_bg=-1), dict(bg=f, n_bg=3),
                dict(bg=f, n_bg=5, B=3)):
        a = dict(ok, **bad)
        assert lib.harp_resolve_u8(*[a[k] for k in order], None) == 1, bad


def test_motion_npz_round_trip(tmp_path):
    from harp_amd.playback import Motion
    rng = np.random.default_rng(0)
    T = 7
    full = Motion(rng.normal(size=(T, 45)), rng.normal(size=(T, 3)), rng.normal(size=(T, 3)), rng.normal(size=(T, 3)),
                  wrist_pose=rng.normal(size=(T, 3)), light_positions=rng.normal(size=(T, 3)))
    bare = Motion(full.pose, full.rot, full.trans, full.cam)
    for m, name in ((full, "full.npz"), (bare, "bare.npz")):
        m.save(tmp_path / name)
        back = Motion.load(tmp_path / name)
        assert len(back) == T
        for k in Motion.FIELDS:
            a, b = getattr(m, k), getattr(back, k)
            assert (a is None) == (b is None), k
            if a is not None:
                assert b.dtype == a.dtype and np.array_equal(a.numpy(), b.numpy()), k
    with pytest.raises(ValueError):
        Motion(full.pose, full.rot[:3], full.trans, full.cam)
    fit = dict(pose=full.pose, rot=full.rot, trans=full.trans, cam=full.cam, light_positions=full.light_positions)
    sub = Motion.from_params(fit, rows=[4, 0, 4])
    assert len(sub) == 3 and sub.wrist_pose is None and np.array_equal(sub.pose.numpy(), full.pose.numpy()[[4, 0, 4]])
    assert sub.light_positions is None                   # a shared-light fit's rows past 0 are not lights: left out unless asked for
    sub = Motion.from_params(fit, rows=[4, 0, 4], per_frame_light=True)
    assert np.array_equal(sub.light_positions.numpy(), full.light_positions.numpy()[[4, 0, 4]])


def test_module_imports_without_the_library(tmp_path):
    env = dict(os.environ, HARP_LIB_PATH=str(tmp_path / "no_such_library.so"))
    code = ("import sys; sys.path.insert(0, %r); import harp_amd.playback as P; import numpy as np; "
            "m = P.Motion(np.zeros((2, 45)), np.zeros((2, 3)), np.zeros((2, 3)), np.ones((2, 3))); assert len(m) == 2; "
            "assert callable(P.AvatarPlayer) and callable(P.main)" % ROOT)
    subprocess.check_call([sys.executable, "-c", code], env=env)


def _log(Rm):
    """rotation matrix (...,3,3) -> axis-angle, float64"""
    v = 0.5 * np.stack([Rm[..., 2, 1] - Rm[..., 1, 2], Rm[..., 0, 2] - Rm[..., 2, 0], Rm[..., 1, 0] - Rm[..., 0, 1]], -1)
    s = np.linalg.norm(v, axis=-1, keepdims=True)
    th = np.arctan2(s, 0.5 * (np.trace(Rm, axis1=-2, axis2=-1)[..., None] - 1.0))
    return np.where(s < 1e-10, v, v * th / np.where(s < 1e-10, 1.0, s))


def _exp(a):
    """Rodrigues, float64"""
    th = np.linalg.norm(a, axis=-1)[..., None, None]
    K = np.zeros(a.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -a[..., 2], a[..., 1], a[..., 2], -a[..., 0], -a[..., 1], a[..., 0]
    small = th < 1e-6
    A = np.where(small, 1.0 - th * th / 6.0, np.sin(th) / np.where(small, 1.0, th))
    Bc = np.where(small, 0.5 - th * th / 24.0, (1.0 - np.cos(th)) / np.where(small, 1.0, th * th))
    return np.eye(3) + A * K + Bc * (K @ K)


def test_reference_slerp_is_the_geodesic_of_rotation_matrices():
    """R0 exp(f log(R0^T R1)) on 1000 seeded pairs, to 1e-12.  Pairs whose relative rotation is beyond 3 rad are redrawn: the matrix
    logarithm (not the slerp) loses digits towards pi, its axis comes from (R - R^T) / (2 sin theta)."""
    rng = np.random.default_rng(5)
    a0, a1 = np.zeros((1000, 3)), np.zeros((1000, 3))
    i = 0
    while i < 1000:
        u = rng.normal(size=(2, 3))
        ang = rng.choice([0.0, 1e-9, 1e-5, 0.3, 1.0, 2.5, np.pi - 1e-3, 4.0, 6.0], size=2) * (1.0 if i % 3 else rng.uniform(0.5, 1.0))
        c = u / np.linalg.norm(u, axis=1, keepdims=True) * ang[:, None]
        if i % 10 == 0:
            c[1] = c[0] * (1.0 + 1e-4)
        if abs((R.quat_of(c[0]) * R.quat_of(c[1])).sum()) < np.cos(1.5):
            continue
        a0[i], a1[i] = c
        i += 1
    f = rng.uniform(0.0, 1.0, size=1000)
    got = R.quat_to_matrix(R.slerp(R.quat_of(a0), R.quat_of(a1), f))
    R0, R1 = _exp(a0), _exp(a1)
    assert np.abs(R0 - R.rotation_matrix(a0)).max() < 1e-14
    want = R0 @ _exp(f[:, None] * _log(np.swapaxes(R0, -1, -2) @ R1))
    dev = np.abs(got - want).max()
    print(f"[slerp vs matrix geodesic] worst entry deviation {dev:.2e} over 1000 pairs")
    assert dev < 1e-12
    # ... and its ends are the two rotations
    for ff, Rm in ((0.0, R0), (1.0, R1)):
        assert np.abs(R.quat_to_matrix(R.slerp(R.quat_of(a0), R.quat_of(a1), np.full(1000, ff))) - Rm).max() < 1e-14
