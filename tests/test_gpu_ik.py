"""-m gpu: harp_mano_ik (csrc/ik.hip) and Motion.from_keypoints against the float64 yardstick of tests/_ik_ref.py.
Every bound below is the error MEASURED on an MI355X against float64 times 4 (the margin §22 gives its resampler); measured values and
bounds are recorded in DESIGN.md §24 and profiles/ik_errors.txt.  Every test prints its figures before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _ik_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 4.0

# test 1, iters = 0: worst deviation over all its cases of ...
JAC_MEASURED = 6.194e-08            # ... a Jacobian entry, relative to the frame's largest Jacobian entry (1: the trans columns)
JOINTS_MEASURED = 3.801e-07         # ... a joint coordinate, relative to the frame's largest joint coordinate
COST0_MEASURED = 1.021e-07          # ... cost[:, 0], relative
# test 2, iters = 1 from the palm start
STEP_MEASURED = 6.605e-05           # x after the step, relative to the yardstick step's largest entry of the frame
COST1_MEASURED = 2.004e-05          # cost[:, 1], relative
# test 3, iters = 15 against the yardstick's 30 iterations
CONV_COST_MEASURED = 1.363e-06      # m: cost[:, 1] / yardstick cost - 1, where positive
CONV_DIST_MEASURED_MM = 2.865e-04   # m': |largest joint distance to the target - the yardstick's|, millimetres
YARDSTICK_DIST_MM = 1.2       # the yardstick's own largest joint distance on that scene (the prior's bias; 1.197 mm, tests/test_ik_cpu.py)

PRIOR_W = 1e-5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _f32(t):
    return t.to(torch.float32).to(DEV).contiguous()


@pytest.fixture(scope="module")
def sc():
    s = R.scene(T=24, seed=0)
    from harp_amd.manopth.manolayer import ManoDeviceModel
    s["dm"] = ManoDeviceModel(s["model_np"], torch.device(DEV))
    # what the kernel sees: float32 inputs; the yardstick runs in float64 from exactly those numbers
    s["betas32"], s["targets32"], s["x0_32"] = s["betas"].float(), s["targets"].float(), R.palm_x0(s).float()
    return s


@pytest.fixture(scope="module")
def yard(sc):
    """the yardstick's 30 iterations from the palm start (its first one is test 2's), once for the module"""
    return R.lm(sc["model"], sc["x0_32"].double(), sc["betas32"].double(), sc["targets32"].double(), prior_weight=PRIOR_W, iters=30)


def _solve(sc, x0, targets, betas=None, **kw):
    from harp_amd import ops
    betas = sc["betas32"] if betas is None else betas
    return ops.mano_ik(sc["dm"], _f32(betas), _f32(targets), _f32(x0[:, :48]), _f32(x0[:, 48:]), **kw)


def _poses(kind, T, hands_mean, rng):
    x = np.zeros((T, 51), np.float32)
    if kind == "zero":
        pass
    elif kind == "aa_zero":                               # stored pose = -hands_mean: every joint's axis-angle is exactly 0
        x[:, 3:48] = -hands_mean
    elif kind == "tiny":
        x[:, :48] = 1e-6
    elif kind == "random":
        x[:, :48] = rng.normal(size=(T, 48)) * 0.3
    elif kind == "near_pi":
        x[:, 3:48] = rng.normal(size=(T, 45)) * 0.3
        u = rng.normal(size=(T, 3))
        x[:, :3] = (np.pi - 1e-3) * u / np.linalg.norm(u, axis=1, keepdims=True)
    return x


@pytest.mark.parametrize("kind", ["zero", "aa_zero", "tiny", "random", "near_pi"])
def test_jacobian_joints_and_cost_at_the_input(sc, kind):
    """iters = 0 evaluates at the input: jac, joints and cost[:, 0] against float64; pose48 and trans come back bit for bit.  T = 1, 2,
    F and F + 1 frames for F frames per workgroup; betas zero / random, shared / per frame; trans zero / non-zero."""
    from harp_amd import ops
    F = ops.mano_ik_frames_per_block()
    rng = np.random.default_rng(7)
    hm = np.asarray(sc["model_np"]["hands_mean"], np.float32)
    worst = dict(jac=0.0, joints=0.0, cost=0.0)
    for T in sorted({1, 2, F, F + 1}):
        for beta_kind in ("zero", "shared", "per_frame"):
            for with_trans in (False, True):
                x = _poses(kind, T, hm, rng)
                if with_trans:
                    x[:, 48:] = rng.uniform(-0.3, 0.3, size=(T, 3))
                betas = {"zero": np.zeros(10), "shared": rng.normal(size=10) * 0.5, "per_frame": rng.normal(size=(T, 10)) * 0.5}[beta_kind]
                x, betas = torch.as_tensor(x), torch.as_tensor(betas, dtype=torch.float32)
                targets = torch.as_tensor(rng.uniform(-0.3, 0.3, size=(T, 21, 3)), dtype=torch.float32)
                out = _solve(sc, x, targets, betas, iters=0, prior_weight=PRIOR_W, joints=True, jac=True)
                assert torch.equal(_bits(out.pose48), _bits(x[:, :48])) and torch.equal(_bits(out.trans), _bits(x[:, 48:]))
                assert out.status.tolist() == [0] * T
                xd, bd = x.double(), betas.double()
                J = R.jacobian(sc["model"], xd, bd)
                with torch.no_grad():
                    j = R.joints(sc["model"], xd, bd)
                    C, _ = R.cost(sc["model"], xd, bd, targets.double(), None, None, PRIOR_W)
                jd = (out.jac.cpu().double().reshape(T, 63, 51) - J).abs().amax((1, 2)) / J.abs().amax((1, 2))
                pd = (out.joints.cpu().double() / 1000.0 - j).abs().amax((1, 2)) / j.abs().amax((1, 2))
                cd = (out.cost[:, 0].cpu().double() - C).abs() / C
                assert torch.equal(_bits(out.cost[:, 0]), _bits(out.cost[:, 1]))
                worst = dict(jac=max(worst["jac"], float(jd.max())), joints=max(worst["joints"], float(pd.max())), cost=max(worst["cost"], float(cd.max())))
    print(f"[mano_ik] jacobian[{kind}] jac {worst['jac']:.3e} joints {worst['joints']:.3e} cost0 {worst['cost']:.3e}")
    assert worst["jac"] <= MARGIN * JAC_MEASURED
    assert worst["joints"] <= MARGIN * JOINTS_MEASURED
    assert worst["cost"] <= MARGIN * COST0_MEASURED


def test_one_step_from_the_palm_start(sc, yard):
    out = _solve(sc, sc["x0_32"], sc["targets32"], iters=1, prior_weight=PRIOR_W)
    c0, c1 = yard["cost"][0], yard["cost"][1]
    counted = (c0 - c1) / c0 > 1e-3                        # a float32 accept / reject cannot be expected to agree on a tie
    assert int((~counted).sum()) <= 0.1 * counted.numel()
    # the yardstick's one step: its accepted candidate (every counted frame accepted it: the cost fell)
    x1 = R.lm(sc["model"], sc["x0_32"].double(), sc["betas32"].double(), sc["targets32"].double(), prior_weight=PRIOR_W, iters=1)["x"]
    step = (x1 - sc["x0_32"].double()).abs().amax(1)
    got = torch.cat([out.pose48, out.trans], 1).cpu().double()
    dx = ((got - x1).abs().amax(1) / step)[counted]
    dc = ((out.cost[:, 1].cpu().double() - c1).abs() / c1)[counted]
    print(f"[mano_ik] one_step x {float(dx.max()):.3e} cost1 {float(dc.max()):.3e} counted {int(counted.sum())} of {counted.numel()}")
    assert out.status.cpu()[counted].tolist() == [1] * int(counted.sum())
    assert float(dx.max()) <= MARGIN * STEP_MEASURED
    assert float(dc.max()) <= MARGIN * COST1_MEASURED


def test_convergence_in_15_iterations(sc, yard):
    out = _solve(sc, sc["x0_32"], sc["targets32"], iters=15, prior_weight=PRIOR_W, joints=True)
    c30 = yard["cost"][30]
    m = float((out.cost[:, 1].cpu().double() / c30 - 1.0).clamp_min(0.0).max())
    with torch.no_grad():
        ref_d = (R.joints(sc["model"], yard["x"], sc["betas32"].double()) - sc["targets32"].double()).norm(dim=-1).amax(1) * 1000
    got_d = (out.joints.cpu().double() - sc["targets32"].double() * 1000).norm(dim=-1).amax(1)
    md = float((got_d - ref_d).abs().max())
    print(f"[mano_ik] convergence m {m:.3e} m' {md:.3e} mm; largest distance {float(got_d.max()):.4f} mm (yardstick {float(ref_d.max()):.4f} mm); "
          f"status {out.status.min().item()}..{out.status.max().item()}")
    assert int(out.status.min()) >= 1
    assert m <= MARGIN * CONV_COST_MEASURED
    assert md <= MARGIN * CONV_DIST_MEASURED_MM
    assert float(ref_d.max()) <= YARDSTICK_DIST_MM


def _all_bits(out):
    return [_bits(t) for t in out if t is not None]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_all_bits(a), _all_bits(b)))


def test_unused_joints_never_enter(sc):
    T = 3
    x0, tg = sc["x0_32"][:T], sc["targets32"][:T]
    w = torch.ones(T, 21)
    w[:, [4, 8, 20]] = 0.0
    outs = []
    for fill in (float("nan"), 1e6, None):
        t = tg.clone()
        if fill is not None:
            t[:, [4, 8, 20]] = fill
        outs.append(_solve(sc, x0, t, weights=_f32(w), iters=6, prior_weight=PRIOR_W, joints=True, jac=True))
    assert _same(outs[0], outs[2]) and _same(outs[1], outs[2])
    # a non-finite target is unused whatever its weight
    t = tg.clone()
    t[:, [4, 8, 20]] = float("inf")
    assert _same(_solve(sc, x0, t, iters=6, prior_weight=PRIOR_W, joints=True, jac=True), outs[2])
    assert int(outs[2].status.min()) >= 1

    for n_used in (0, 2):                                  # the middle frame is not solved; its neighbours do not notice
        w = torch.ones(T, 21)
        w[1] = 0.0
        w[1, :n_used] = 1.0
        out = _solve(sc, x0, tg, weights=_f32(w), iters=6, prior_weight=PRIOR_W, joints=True, jac=True)
        assert out.status.tolist()[1] == -1 and min(out.status.tolist()[0], out.status.tolist()[2]) >= 1
        assert torch.equal(_bits(out.pose48[1]), _bits(x0[1, :48])) and torch.equal(_bits(out.trans[1]), _bits(x0[1, 48:]))
        assert torch.equal(_bits(out.cost[1, 0]), _bits(out.cost[1, 1]))
        for f in (0, 2):
            alone = _solve(sc, x0[f:f + 1], tg[f:f + 1], weights=_f32(w[f:f + 1]), iters=6, prior_weight=PRIOR_W, joints=True, jac=True)
            assert all(torch.equal(_bits(a[f]), _bits(b[0])) for a, b in zip(out, alone)), (n_used, f)


def test_rejected_steps_never_raise_the_cost():
    """from zero (no palm start) on targets rotated by 3 rad the first steps overshoot: some are rejected, in the yardstick too"""
    from harp_amd.manopth.manolayer import ManoDeviceModel
    iters = 15
    s = R.scene(T=6, seed=1, root_lo=3.0, root_hi=3.0)
    s["dm"], s["betas32"] = ManoDeviceModel(s["model_np"], torch.device(DEV)), s["betas"].float()
    x0, tg = torch.zeros(6, 51), s["targets"].float()
    ref = R.lm(s["model"], x0.double(), s["betas32"].double(), tg.double(), prior_weight=PRIOR_W, iters=iters)
    assert int(ref["accepted"].min()) < iters            # the scene does what it is for
    out = _solve(s, x0, tg, iters=iters, prior_weight=PRIOR_W, joints=True, jac=True)
    print(f"[mano_ik] rejected status {out.status.tolist()} yardstick {ref['accepted'].tolist()} cost {out.cost.cpu().tolist()}")
    assert bool((out.cost[:, 1] <= out.cost[:, 0]).all())
    assert all(bool(torch.isfinite(t.float()).all()) for t in out)
    assert int(out.status.min()) < iters and int(out.status.min()) >= 0


def test_repeatable_and_capturable(sc):
    """two calls give equal bytes; ONE captured call of the C entry point (a single kernel node: it allocates nothing, copies nothing and
    has no second launch), replayed on fresh inputs, equals the eager call"""
    from harp_amd import _lib
    kw = dict(iters=15, prior_weight=PRIOR_W, joints=True, jac=True)
    a = _solve(sc, sc["x0_32"], sc["targets32"], **kw)
    b = _solve(sc, sc["x0_32"], sc["targets32"], **kw)
    assert _same(a, b)
    T = 24
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=DEV)
    pose48, trans, cost, status, joints, jac = e(T, 48), e(T, 3), e(T, 2), e(T, dt=torch.int32), e(T, 21, 3), e(T, 63, 51)
    betas, targets = _f32(sc["betas32"]), _f32(sc["targets32"])
    opt = _lib.IkOptions(15, 1e-3, PRIOR_W, 0)
    p = _lib.ptr

    def launch():
        rc = _lib.lib().harp_mano_ik(ctypes.byref(sc["dm"].struct), p(betas), p(targets), None, None, T, ctypes.byref(opt), p(pose48), p(trans),
                                     p(cost), p(status), p(joints), p(jac), _lib.stream())
        assert rc == 0

    def reset():
        pose48.copy_(_f32(sc["x0_32"][:, :48])); trans.copy_(_f32(sc["x0_32"][:, 48:]))
        for t in (cost, joints, jac):
            t.fill_(-1.0)
        status.fill_(-7)

    reset()
    launch()                                              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    reset()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        launch()
    for _ in range(2):
        reset()
        g.replay()
        torch.cuda.synchronize()
        assert _same(a, (pose48, trans, cost, status, joints, jac))


def test_motion_from_keypoints_drives_the_player(tmp_path):
    """keypoints made by the forward from a seeded 5-frame motion -> Motion.from_keypoints -> the forward again: the joints are back
    within the recorded distance of test 3 (the yardstick's prior bias + m'); the same keypoints 1.2 x about the wrist with
    match_bone_lengths give the same motion; the arm layer raises; the recovered motion renders."""
    from harp_amd.playback import AvatarPlayer, Motion
    from tests.test_gpu_evaluate import _setup
    T, S = 5, 32
    _, cfg, layer, params, _ = _setup(T, S, 3, tmp_path)
    true = Motion.from_params(params)
    betas = params["shape"].detach().reshape(1, 10).expand(T, 10).contiguous()

    def forward(m):
        with torch.no_grad():
            return layer(torch.cat([m.rot, m.pose], 1).to(DEV), betas, m.trans.to(DEV))[1]

    kp = forward(true) / 1000.0
    rec = Motion.from_keypoints(kp, params, layer)
    assert len(rec) == T and rec.light_positions is None and torch.equal(rec.cam.cpu(), params["cam"][0].detach().cpu().expand(T, 3))
    dist = float((forward(rec) - kp * 1000.0).norm(dim=-1).max())
    print(f"[mano_ik] layer largest joint distance {dist:.4f} mm")
    assert dist <= YARDSTICK_DIST_MM + MARGIN * CONV_DIST_MEASURED_MM

    big = kp[:, :1] + 1.2 * (kp - kp[:, :1])
    rec2 = Motion.from_keypoints(big, params, layer)
    dpose = max(float((getattr(rec2, k) - getattr(rec, k)).abs().max()) for k in ("pose", "rot", "trans"))
    print(f"[mano_ik] layer scaled-keypoints motion difference {dpose:.3e}")
    # float32 rounding of the scaled targets: <= 2 ulp of 0.5 m = 1.2e-7 m per coordinate, 1e-6 m over the 63; the least determined direction
    # of the solve is held by the prior alone, sqrt(1e-5) = 3.2e-3 per unit: 1e-6 / 3.2e-3
    assert dpose <= 3.2e-4
    off = Motion.from_keypoints(big, params, layer, match_bone_lengths=False)
    assert float((off.trans - rec.trans).abs().max()) > 1e-3 or float((off.pose - rec.pose).abs().max()) > 1e-2      # (the switch does something)

    with pytest.raises(NotImplementedError):
        Motion.from_keypoints(kp, params, R._Layer(dict(layer._model_np, pose_mean=np.zeros(165))))

    player = AvatarPlayer(cfg, params, layer, batch_size=T, ss=1, device=DEV)
    white = lambda fr: int((fr.cpu() != 255).any(-1).sum())
    player.load_motion(true)
    n_true = white(player.render(np.arange(T)))
    player.load_motion(Motion(rec.pose, rec.rot, rec.trans, true.cam))      # the true motion's per-frame cam: the two renders are comparable
    n_rec = white(player.render(np.arange(T)))
    print(f"[mano_ik] layer covered pixels true {n_true} recovered {n_rec}")
    assert n_true > 0 and abs(n_rec - n_true) <= 0.02 * n_true


def test_command_line_takes_keypoints(tmp_path, monkeypatch):
    """python -m harp_amd.playback's main() with --keypoints instead of --motion (the two loaders of licensed / fitted files replaced by
    the synthetic scene, as tests/test_gpu_avatar_player.py does): keypoints, weights and cam in, retimed frames out"""
    import os
    import yaml
    from PIL import Image
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
    with torch.no_grad():
        kp = layer(torch.cat([true.rot, true.pose], 1).to(DEV), params["shape"].detach().reshape(1, 10).expand(T, 10).contiguous(), true.trans.to(DEV))[1] / 1000.0
    np.savez(tmp_path / "kp.npz", keypoints=kp.cpu().numpy(), weights=np.ones((T, 21), np.float32), cam=true.cam.cpu().numpy())
    out = tmp_path / "frames"
    common = ["--config", str(tmp_path / "cfg.yaml"), "--out", str(out)]
    paths = playback.main(common + ["--keypoints", str(tmp_path / "kp.npz"), "--fps-scale", "2", "--batch-size", "4"])
    assert sorted(os.listdir(out)) == ["%04d.jpg" % i for i in range(2 * T - 1)] and len(paths) == 2 * T - 1
    assert Image.open(paths[0]).size == (S, S)
    for bad in ([], ["--keypoints", str(tmp_path / "kp.npz"), "--motion", str(tmp_path / "kp.npz")]):
        with pytest.raises(SystemExit):
            playback.main(common + bad)
