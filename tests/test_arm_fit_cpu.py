"""No GPU: the yardstick of the SMPL-X arm vertex fit itself (tests/_arm_fit_ref.py: its Jacobian against central differences, the algebra
of frozen columns, what the float64 iteration does from the rigid start for each target set, and that the scenes of the GPU tests leave no
frame out), the signatures of the three Python entry points, the command line, and harp_arm_vertex_fit's argument errors, which return
before any launch."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import _arm_fit_ref as R
from tests import _ik_ref


@pytest.fixture(scope="module")
def arm():
    m_np, m, mano = R.arm_model()
    return dict(np=m_np, model=m, mano=mano)


# ---- (a) the yardstick ------------------------------------------------------------------------------------------------------------------
def test_jacobian_against_central_differences(arm):
    rng = np.random.default_rng(2)
    idx = np.concatenate([arm["mano"][:30], rng.permutation(1026)[:35]])
    sc = R.scene(T=2, seed=5, idx=idx)
    x = sc["x_true"]
    J = R.jacobian(sc["model"], x, idx)
    assert tuple(J.shape) == (2, 3 * 65, 64)
    h = 1e-6
    worst = 0.0
    for c in range(R.NX):
        e = torch.zeros(R.NX, dtype=torch.float64)
        e[c] = h
        with torch.no_grad():
            fd = (R.verts(sc["model"], x + e, idx) - R.verts(sc["model"], x - e, idx)).reshape(2, -1) / (2 * h)
        worst = max(worst, float((fd - J[:, :, c]).abs().max()))
    scale = float(J.abs().max())
    print(f"[arm_fit_cpu] jacobian vs central differences {worst:.3e} of {scale:.3e}")
    assert worst <= 1e-8 * scale                          # (h^2 f''' ~ 1e-12 and rounding 1e-16 / h ~ 1e-10, both of order one lever arm)
    # every kind of column is there: the wrist moves hand vertices, a finger column few of them, a shape column all
    assert all(float(J[:, :, c].abs().max()) > 0 for c in range(R.NX))
    assert torch.equal(J[0, :, R.XT:].reshape(65, 3, 3), torch.eye(3, dtype=torch.float64).expand(65, 3, 3))


def test_frozen_column_algebra(arm):
    sc = R.scene(T=2, seed=6, idx=arm["mano"])
    x0 = R.rigid_x0(sc)
    x0[:, R.XW:R.XP] = 0.1
    kw = dict(idx=sc["idx"], pose_prior_weight=1e-3, wrist_prior_weight=2e-3, shape_prior_weight=3e-3)
    free = R.normal(sc["model"], x0, sc["targets"], **kw)
    for solve_shape, solve_wrist in ((False, True), (True, False), (False, False)):
        fz = R.frozen_columns(solve_shape, solve_wrist)
        keep = [c for c in range(R.NX) if c not in fz]
        assert len(fz) == 10 * (not solve_shape) + 3 * (not solve_wrist)
        n = R.normal(sc["model"], x0, sc["targets"], solve_shape=solve_shape, solve_wrist=solve_wrist, **kw)
        off = n["A"].clone()
        off[:, fz, fz] -= 1.0
        assert bool((off[:, fz, :] == 0).all() and (off[:, :, fz] == 0).all() and (n["g"][:, fz] == 0).all())
        assert torch.equal(n["A"][:, keep][:, :, keep], free["A"][:, keep][:, :, keep]) and torch.equal(n["g"][:, keep], free["g"][:, keep])
        assert torch.equal(n["J"], free["J"]) and torch.equal(n["C"], free["C"])       # always all 64 columns; the priors stay in the cost
        y = R.lm(sc["model"], x0, sc["targets"], solve_shape=solve_shape, solve_wrist=solve_wrist, iters=3, **kw)
        assert int(y["accepted"].min()) >= 1 and torch.equal(y["x"][:, fz], x0[:, fz]) and not torch.equal(y["x"][:, keep], x0[:, keep])
    # the priors are where the contract puts them
    P = torch.diagonal(free["A"] - R.normal(sc["model"], x0, sc["targets"], idx=sc["idx"])["A"], dim1=1, dim2=2)[0]
    want = torch.zeros(R.NX, dtype=torch.float64)
    want[R.XP:R.XB], want[R.XW:R.XP], want[R.XB:R.XT] = 1e-3, 2e-3, 3e-3
    assert float((P - want).abs().max()) < 1e-12


@pytest.mark.parametrize("case", ["all_wrist_solved", "mano_wrist_frozen", "mano_wrist_solved"])
def test_float64_yardstick_from_the_rigid_start(arm, case):
    """All 1026 vertices with the wrist solved, and the 778 hand vertices with the wrist held, converge to < 1e-9 mm RMS within 10
    iterations; the 778 with the wrist solved converge as well, at a far larger condition number of the scaled matrix: from hand vertices
    alone the root and the wrist rotation are nearly interchangeable, which is why that is not the default."""
    idx = None if case.startswith("all") else arm["mano"]
    solve_wrist = case != "mano_wrist_frozen"
    sc = R.scene(T=4, seed=0, idx=idx, wrist=solve_wrist)
    x0 = R.rigid_x0(sc)
    y = R.lm(sc["model"], x0, sc["targets"], idx=idx, solve_wrist=solve_wrist, iters=10)
    rms = R.rms_mm(sc["model"], y["x"], sc["targets"], idx)
    print(f"[arm_fit_cpu] {case}: accepted {y['accepted'].tolist()} rms {rms.tolist()} mm cond {['%.1e' % c for c in y['cond'].tolist()]}")
    assert float(rms.max()) < 1e-9
    assert int(y["accepted"].min()) >= 4
    if case == "mano_wrist_solved":
        assert float(y["cond"].min()) > 3e3               # (measured 3e4 .. 5e4 against 2e2 .. 5e2 of the other two)
    else:
        assert float(y["cond"].max()) < 3e3
    if not solve_wrist:
        assert bool((y["x"][:, R.XW:R.XP] == 0).all())


@pytest.mark.parametrize("name", sorted(R.GPU_SCENES))
def test_gpu_scenes_leave_no_frame_out(name):
    """the scenes of the GPU tests: float32 decides every frame's first step as float64 does, and by a margin (no tie), so the GPU tests
    compare all 8 frames"""
    sc, kw = R.gpu_scene(name)
    counted, y1, y1_32 = R.counted_first_step(sc, kw)
    assert counted.numel() == 8 and bool(counted.all())
    assert y1["accepted"].tolist() == [1] * 8 and y1_32["accepted"].tolist() == [1] * 8


# ---- (b) signatures, command line, argument errors ----------------------------------------------------------------------------------------
def test_optimize_for_mano_arm_param_takes_a_method():
    from harp_amd.metro_modifications import hand_utils
    p = inspect.signature(hand_utils.optimize_for_mano_arm_param).parameters
    assert list(p) == ["pred_vertices", "mano_arm_layer", "idx", "vert_rgb", "method"] and p["method"].default == "adam"

    class Never:                                           # touching the layer (or a device) before the check would raise AttributeError
        def __getattr__(self, name):
            raise AttributeError(name)
    with pytest.raises(ValueError, match="method"):
        hand_utils.optimize_for_mano_arm_param(torch.zeros(1, 778, 3), Never(), method="newton")


def test_ops_arm_vertex_fit_signature():
    from harp_amd import ops
    p = inspect.signature(ops.arm_vertex_fit).parameters
    assert list(p) == ["dm", "targets", "in_pose", "betas", "trans", "vert_idx", "weights", "prior", "solve_shape", "solve_wrist", "iters", "lambda0",
                       "pose_prior_weight", "wrist_prior_weight", "shape_prior_weight", "verts", "jac", "normal", "out"]
    want = dict(vert_idx=None, weights=None, prior=None, solve_shape=True, solve_wrist=True, iters=10, lambda0=1e-3, pose_prior_weight=0.0,
                wrist_prior_weight=0.0, shape_prior_weight=0.0, verts=False, jac=False, normal=False, out=None)
    assert {k: p[k].default for k in want} == want
    assert ops.ArmVertexFitResult._fields == ("in_pose", "betas", "trans", "cost", "status", "verts", "jac", "A", "g")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.arm_vertex_fit(None, torch.zeros(1, 1026, 3), torch.zeros(1, 17, 3), torch.zeros(1, 10), torch.zeros(1, 3))


def test_from_arm_vertices_signature():
    from harp_amd import playback
    from harp_amd.playback import Motion
    p = inspect.signature(Motion.from_arm_vertices).parameters
    assert list(p) == ["vertices", "params", "arm_layer", "cam", "weights", "iters", "pose_prior_weight", "wrist_prior_weight", "wrist_pose", "init",
                       "device"]
    assert p["iters"].default == 10 and p["pose_prior_weight"].default == 0.0 and p["wrist_prior_weight"].default == 0.0
    assert all(p[k].default is None for k in ("cam", "weights", "wrist_pose", "init", "device"))
    assert playback.Motion is Motion and "Motion" in playback.__all__
    with pytest.raises(ValueError, match="SMPL-X arm"):      # a MANO layer is not what it fits
        Motion.from_arm_vertices(np.zeros((1, 778, 3)), {}, _ik_ref._Layer({"hands_mean": np.zeros(45)}))
    # from_vertices keeps refusing the arm, and now names the way
    with pytest.raises(NotImplementedError, match="from_arm_vertices"):
        Motion.from_vertices(np.zeros((1, 778, 3)), {}, _ik_ref._Layer({"pose_mean": np.zeros(165)}))


def test_command_line_describes_arm_vertices(capsys):
    from harp_amd.playback import cli
    common = ["--config", "c.yaml", "--out", "o"]
    args = cli.parse_args(common + ["--vertices", "v.npz"])
    assert args.vertices == "v.npz" and args.motion is None and args.keypoints is None
    with pytest.raises(SystemExit):
        cli.parse_args(common + ["--vertices", "v.npz", "--motion", "m.npz"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "from_arm_vertices" in text and "1026" in text
    assert "from_arm_vertices" in inspect.getsource(cli.main)


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


def test_arm_vertex_fit_argument_errors_without_a_launch(lib):
    """every refusal of the contract with FAKE pointers: a call that got as far as a launch would fault, so returning 1 shows it did not"""
    from harp_amd import _lib
    f = 1 << 20                                            # a fake device pointer, never dereferenced
    good = dict(m=_tree(f), vert_idx=None, n_t=1026, targets=f, T=2, in_pose=f, betas=f, trans=f, cost=f, status=f)

    def call(opt=None, **kw):
        a = dict(good, **kw)
        o = ctypes.byref(_lib.ArmVertexFitOptions(10, 1e-3, 0.0, 0.0, 0.0, 1, 1, 0)) if opt is None else opt
        m = None if a["m"] is None else ctypes.byref(a["m"])
        return lib.harp_arm_vertex_fit(m, a["vert_idx"], a["n_t"], a["targets"], None, None, a["T"], o, a["in_pose"], a["betas"], a["trans"],
                                       a["cost"], a["status"], None, None, None, None, None)

    for name in ("m", "targets", "in_pose", "betas", "trans", "cost", "status"):
        assert call(**{name: None}) == 1, name
    assert call(opt=ctypes.POINTER(_lib.ArmVertexFitOptions)()) == 1
    assert call(T=0) == 1 and call(T=-1) == 1
    assert call(n_t=0) == 1 and call(n_t=1027, vert_idx=f) == 1 and call(n_t=778) == 1 and call(n_t=1025) == 1
    nan, inf = float("nan"), float("inf")
    assert call(opt=ctypes.byref(_lib.ArmVertexFitOptions(-1, 1e-3, 0.0, 0.0, 0.0, 1, 1, 0))) == 1
    for pos in range(1, 5):                               # lambda0 and the three prior weights
        for bad in (-1.0, nan, inf):
            o = [10, 1e-3, 0.0, 0.0, 0.0, 1, 1, 0]
            o[pos] = bad
            assert call(opt=ctypes.byref(_lib.ArmVertexFitOptions(*o))) == 1, (pos, bad)
    for kw in (dict(n_pose_in=16), dict(n_pose_in=18), dict(NB=9), dict(NB=33), dict(NJ=65), dict(NV=_lib.ARM_VERTEX_FIT_MAX_VERTS + 1),
               dict(center_joint=-1), dict(center_joint=55)):
        nv = kw.get("NV", 1026)
        assert call(m=_tree(f, **kw), n_t=nv) == 1, kw
    assert ctypes.sizeof(_lib.ArmVertexFitOptions) == 32 and lib.harp_arm_vertex_fit_frames_per_block() >= 1


def test_arm_vertex_fit_options_layout_matches_c(tmp_path):
    import os
    import re
    import subprocess
    from harp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [n for n, _ in _lib.ArmVertexFitOptions._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) +
                   ' %d\\n", sizeof(harp_arm_vertex_fit_options),' + ",".join(f"offsetof(harp_arm_vertex_fit_options, {n})" for n in fields) +
                   ", HARP_ARM_VERTEX_FIT_MAX_VERTS); return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.ArmVertexFitOptions)] + [getattr(_lib.ArmVertexFitOptions, n).offset for n in fields] + \
        [_lib.ARM_VERTEX_FIT_MAX_VERTS]
    with open(os.path.join(root, "harp_amd", "csrc", "arm_vertex_fit.hip")) as fh:
        assert re.search(r"MAXV = HARP_ARM_VERTEX_FIT_MAX_VERTS;", fh.read())
