"""-m gpu: harp_arm_ik (csrc/arm_ik.hip), ops.arm_ik and Motion.from_arm_keypoints against the yardstick of tests/_arm_ik_ref.py (DESIGN.md
§29).

No bound here is a number fixed in advance.  Each is computed in the test from the yardstick itself:

    bound = 8 x the float32 yardstick's error against the float64 yardstick on the same inputs            (R.FACTOR)

— the same code in float32 (forward, J^T W J, Cholesky of the Jacobi-scaled system) is the error model of a correct float32 solver, and the
factor covers what the kernel does differently: its dots summed in another order, the root column as a rotation of the centre-relative
joint, the tangents walked down the tree, and the device's sinf / cosf.  Both sides of every comparison are the worst over all the frames
that the test runs, never one frame's.  Measured errors and bounds are recorded side by side in profiles/arm_ik_errors.txt and DESIGN.md
§29.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import _arm_ik_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO = R.NO


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _f32(t):
    return None if t is None else t.to(torch.float32).to(DEV).contiguous()


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b) if x is not None)


def _x(out):
    T = out.in_pose.shape[0]
    return torch.cat([out.in_pose.reshape(T, 51), out.trans], 1).cpu().double()


@pytest.fixture(scope="module")
def arm():
    from harp_amd.hand_models_harp.body_models import TreeDeviceModel
    m_np, m, _ = R.arm_model()
    m2_np, m2 = R.mean_model()
    dev = torch.device(DEV)
    return dict(np=m_np, model=m, dm=TreeDeviceModel(m_np, dev), np2=m2_np, model2=m2, dm2=TreeDeviceModel(m2_np, dev))


def _solve(dm, x0, betas, targets, weights=None, prior=None, wrist_prior=None, **kw):
    """x0 (T,54) holds the start"""
    from harp_amd import ops
    T = x0.shape[0]
    return ops.arm_ik(dm, _f32(betas), _f32(targets), _f32(x0[:, :R.XT].reshape(T, 17, 3)), _f32(x0[:, R.XT:]), weights=_f32(weights),
                      prior=_f32(prior), wrist_prior=_f32(wrist_prior), **kw)


def _rel(got, ref):
    """per frame: the largest deviation relative to the frame's largest entry of the quantity"""
    T = ref.shape[0]
    d, m = (got.double() - ref.double()).abs().reshape(T, -1).amax(1), ref.double().abs().reshape(T, -1).amax(1)
    return float((d / m).max())


def _yard(name, iters64=30, iters32=15, **skw):
    sc = R.scene32(name, **skw)
    sc["y64"] = R.lm(sc["model"], sc["x0_32"].double(), sc["betas32"].double(), sc["targets32"].double(), iters=iters64, **sc["kw"])
    sc["y32"] = R.lm(sc["model"], sc["x0_32"], sc["betas32"], sc["targets32"], iters=iters32, dtype=torch.float32, **sc["kw"])
    return sc


@pytest.fixture(scope="module")
def exact22():
    return _yard("22", T=8, seed=0)


# ---- 1. iters = 0 at the input ----------------------------------------------------------------------------------------------------------
def _driven_mean(pm):
    """the pose mean of the 17 driven joints as a row of in_pose (51,)"""
    return np.concatenate([pm[0:3], pm[63:66], pm[120:165]])


def _poses(kind, T, pm, rng):
    x = np.zeros((T, R.NX), np.float32)
    if kind == "aa_zero":                                 # stored pose = -pose_mean: every driven joint's axis-angle is exactly 0
        x[:, :R.XT] = -_driven_mean(pm)
    elif kind == "tiny":
        x[:, :R.XT] = 1e-6
    elif kind == "random":
        x[:, :R.XT] = rng.normal(size=(T, 51)) * 0.3
    elif kind == "near_pi":
        x[:, R.XW:R.XT] = rng.normal(size=(T, 48)) * 0.3
        u = rng.normal(size=(T, 3))
        x[:, :3] = (np.pi - 1e-3) * u / np.linalg.norm(u, axis=1, keepdims=True)
    return x


# (model, T, betas, trans, weights)
_CASES = [("model", 1, "zero", False, None), ("model", 2, "shared", True, "zeros"), ("model2", 3, "per_frame", True, "nan_unused"),
          ("model2", 2, "shared", False, "no_elbow"), ("model", 3, "per_frame", True, "nan_weighted"), ("model2", 1, "zero", True, None)]


@pytest.mark.parametrize("kind", ["zero", "aa_zero", "tiny", "random", "near_pi"])
def test_everything_at_the_input(arm, kind):
    """iters = 0 evaluates at the input: joints, jac and cost[:, 0] against float64, each relative to the frame's largest entry of that
    quantity; in_pose and trans come back bit for bit.  T = 1, 2, 3 around the frames per workgroup; betas zero / (10,) / (T,10); trans zero
    / not; weights None / all zero (status -1) / a NaN target under a zero weight / the elbow unused / a NaN target under a weight of one;
    the synthetic model and the one whose undriven joints 17, 19 and 25..39 have a pose mean."""
    from harp_amd import ops
    F = ops.arm_ik_frames_per_block()
    rng = np.random.default_rng(11)
    assert {c[1] for c in _CASES} >= {F, F + 1} and {c[0] for c in _CASES} == {"model", "model2"}
    pm2 = arm["np2"]["pose_mean"]
    assert bool((pm2[51:54] != 0).all() and (pm2[57:60] != 0).all() and (pm2[75:120] != 0).all() and (pm2[120:165] != 0).all())
    names = ("joints", "jac", "cost")
    worst, worst32 = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0)
    for which, T, bkind, with_trans, wkind in _CASES:
        model, dm = arm[which], arm["dm" if which == "model" else "dm2"]
        pm = arm["np" if which == "model" else "np2"]["pose_mean"].astype(np.float32)
        x = _poses(kind, T, pm, rng)
        if kind == "aa_zero":
            assert bool((_driven_mean(pm) + x[0, :R.XT] == 0).all())
        if with_trans:
            x[:, R.XT:] = rng.uniform(-0.3, 0.3, size=(T, 3))
        x = torch.as_tensor(x)
        betas = {"zero": torch.zeros(10), "shared": torch.as_tensor(rng.normal(size=10) * 0.5, dtype=torch.float32),
                 "per_frame": torch.as_tensor(rng.normal(size=(T, 10)) * 0.5, dtype=torch.float32)}[bkind]
        targets = torch.as_tensor(rng.uniform(-0.3, 0.3, size=(T, NO, 3)), dtype=torch.float32)
        w, n_used = None, NO
        if wkind == "zeros":
            w, n_used = torch.zeros(T, NO), 0
        elif wkind == "nan_unused":
            w = torch.as_tensor(rng.uniform(0.5, 1.5, size=(T, NO)), dtype=torch.float32)
            w[:, [0, 7, 20]] = 0.0
            targets[:, 7] = float("nan")
            n_used = NO - 3
        elif wkind == "no_elbow":
            w = torch.ones(T, NO)
            w[:, R.ELBOW] = 0.0
            n_used = NO - 1
        elif wkind == "nan_weighted":
            targets[:, 3, 1] = float("nan")               # unused although its weight is one
            targets[:, 12] = float("inf")
            n_used = NO - 2
        prior = torch.as_tensor(rng.normal(size=(T, 45)) * 0.1, dtype=torch.float32)
        wprior = torch.as_tensor(rng.normal(size=(T, 3)) * 0.1, dtype=torch.float32)
        kw = dict(pose_prior_weight=1e-3, wrist_prior_weight=3e-3)
        out = _solve(dm, x, betas, targets, weights=w, prior=prior, wrist_prior=wprior, iters=0, joints=True, jac=True, **kw)
        assert torch.equal(_bits(out.in_pose.reshape(T, 51)), _bits(x[:, :R.XT])) and torch.equal(_bits(out.trans), _bits(x[:, R.XT:]))
        assert out.status.tolist() == [0 if n_used >= 3 else -1] * T
        assert torch.equal(_bits(out.cost[:, 0]), _bits(out.cost[:, 1]))
        assert tuple(out.joints.shape) == (T, NO, 3) and tuple(out.jac.shape) == (T, 3 * NO, R.NX)
        jac = out.jac.cpu()
        e = slice(3 * R.ELBOW, 3 * R.ELBOW + 3)
        assert bool((jac[:, e, R.XW:R.XT] == 0).all())     # the elbow: an ancestor of the centre, exactly zero
        n64 = R.normal(model, x.double(), betas.double(), targets, weights=w, prior=prior, wrist_prior=wprior, **kw)
        n32 = R.normal(model, x, betas, targets, weights=w, prior=prior, wrist_prior=wprior, dtype=torch.float32, **kw)
        with torch.no_grad():
            j64, j32 = R.joints(model, x.double(), betas.double()), R.joints(model, x, betas, torch.float32)
        got = dict(joints=out.joints.cpu() / 1000.0, jac=jac, cost=out.cost[:, :1].cpu())
        ref = dict(joints=j64, jac=n64["J"], cost=n64["C"][:, None])
        f32 = dict(joints=j32, jac=n32["J"], cost=n32["C"][:, None])
        for k in names:
            worst[k], worst32[k] = max(worst[k], _rel(got[k], ref[k])), max(worst32[k], _rel(f32[k], ref[k]))
    print(f"[arm_ik] input[{kind}] " + " ".join(f"{k} {worst[k]:.3e} (bound {R.FACTOR * worst32[k]:.3e})" for k in names))
    for k in names:
        assert worst[k] <= R.FACTOR * worst32[k], k


# ---- 2. one step from the layer's start ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.ONE_STEP))
def test_one_step_from_the_layers_start(arm, name):
    sc = R.scene32(name, **R.ONE_STEP[name])
    counted, y1, y1_32 = R.counted_first_step(sc)
    T = counted.numel()
    assert bool(counted.all())                            # (no frame left out, asserted on the CPU as well)
    x0 = sc["x0_32"].double()
    out = _solve(arm["dm"], sc["x0_32"], sc["betas32"], sc["targets32"], iters=1, **sc["kw"])
    step = (y1["x"] - x0).abs().amax(1)
    c1 = y1["cost"][1]
    dx = float(((_x(out) - y1["x"]).abs().amax(1) / step).max())
    dx32 = float(((y1_32["x"].double() - y1["x"]).abs().amax(1) / step).max())
    dc = float(((out.cost[:, 1].cpu().double() - c1).abs() / c1).max())
    dc32 = float(((y1_32["cost"][1].double() - c1).abs() / c1).max())
    print(f"[arm_ik] one_step[{name}] x {dx:.3e} (bound {R.FACTOR * dx32:.3e}) cost1 {dc:.3e} (bound {R.FACTOR * dc32:.3e}) "
          f"counted {int(counted.sum())} of {T}")
    assert out.status.cpu().tolist() == [1] * T
    assert dx <= R.FACTOR * dx32
    assert dc <= R.FACTOR * dc32
    if name == "21":
        assert torch.equal(_bits(out.in_pose[:, 1]), _bits(sc["x0_32"][:, R.XW:R.XP]))


# ---- 3. fifteen iterations against the float64 yardstick's thirty ---------------------------------------------------------------------------
def _after_15(arm, sc, label):
    out = _solve(arm["dm"], sc["x0_32"], sc["betas32"], sc["targets32"], iters=15, joints=True, **sc["kw"])
    c30 = sc["y64"]["cost"][30]
    m = float((out.cost[:, 1].cpu().double() / c30 - 1.0).max())
    m32 = float((sc["y32"]["cost"][15].double() / c30 - 1.0).abs().max())
    w = sc["kw"]["weights"]
    used, _, tg = R.used_mask(sc["targets32"].double(), w)
    d = float(((out.joints.cpu().double() / 1000.0 - tg).norm(dim=-1) * used).max() * 1000.0)
    d32 = float(R.joint_dist_mm(sc["model"], sc["y32"]["x"], sc["betas32"], sc["targets32"], w, torch.float32)[1].max())
    d64 = float(R.joint_dist_mm(sc["model"], sc["y64"]["x"], sc["betas32"].double(), sc["targets32"], w)[1].max())
    print(f"[arm_ik] fifteen[{label}] cost/yardstick - 1 {m:.3e} (bound {R.FACTOR * m32:.3e}) largest joint distance {d:.3e} mm "
          f"(bound {R.FACTOR * d32:.3e}; float64 yardstick {d64:.3e}) status {out.status.tolist()}")
    assert int(out.status.min()) >= 1
    assert m <= R.FACTOR * m32
    assert d <= R.FACTOR * d32
    return out


def test_fifteen_iterations_on_exact_keypoints(arm, exact22):
    _after_15(arm, exact22, "22")


def test_fifteen_iterations_with_the_wrist_held(arm):
    sc = _yard("21", T=8, seed=0)
    out = _after_15(arm, sc, "21")
    assert torch.equal(_bits(out.in_pose[:, 1]), _bits(sc["x0_32"][:, R.XW:R.XP]))


def test_fifteen_iterations_on_noisy_keypoints(arm):
    _after_15(arm, _yard("22", T=8, seed=1, noise=0.002), "22, 2 mm noise")


def test_fifteen_iterations_with_another_arms_shape(arm):
    """keypoints of one arm, solved with another's shape, given per frame and as (10,): the same bits, and the yardstick's cost"""
    sc = R.scene32("22", T=8, seed=2)
    avatar = torch.as_tensor(np.random.default_rng(3).normal(size=10) * 0.5, dtype=torch.float32)
    sc["betas32"] = avatar
    sc["x0_32"] = R.layer_start(sc["model"], avatar.double(), sc["targets32"]).float()
    sc["y64"] = R.lm(sc["model"], sc["x0_32"].double(), avatar.double(), sc["targets32"].double(), iters=30, **sc["kw"])
    sc["y32"] = R.lm(sc["model"], sc["x0_32"], avatar, sc["targets32"], iters=15, dtype=torch.float32, **sc["kw"])
    a = _after_15(arm, sc, "another shape (10,)")
    sc["betas32"] = avatar[None].expand(8, 10).contiguous()
    b = _after_15(arm, sc, "another shape (T,10)")
    assert _same(a, b) and float(a.cost[:, 1].min()) > 0.0


# ---- 4. rejections --------------------------------------------------------------------------------------------------------------------------
def test_status_counts_the_strict_decreases(arm):
    """from zero (no start) on keypoints rotated by 3 rad the first steps overshoot: status is the number of strict decreases in the
    yardstick's cost history, and in the kernel's own (the kernel is deterministic: the run with k iterations is the prefix of the run
    with k + 1); the optional outputs are those of the x that was kept"""
    iters, T = 6, 6
    s = R.scene(T=T, seed=1, root_lo=3.0, root_hi=3.0)
    assert bool(((s["x_true"][:, :3].norm(dim=1) - 3.0).abs() < 1e-12).all())
    x0, tg, b = torch.zeros(T, R.NX), s["targets"].float(), s["betas"].float()
    y = R.lm(s["model"], x0.double(), b.double(), tg.double(), iters=iters, **R.PRIORS)
    y32 = R.lm(s["model"], x0, b, tg, iters=iters, dtype=torch.float32, **R.PRIORS)
    falls64 = (y["cost"][1:] < y["cost"][:-1]).sum(0)
    hist = [_solve(arm["dm"], x0, b, tg, iters=0, **R.PRIORS).cost[:, 0].cpu()]
    for k in range(1, iters + 1):
        out = _solve(arm["dm"], x0, b, tg, iters=k, **R.PRIORS)
        assert torch.equal(_bits(out.cost[:, 0]), _bits(hist[0]))
        hist.append(out.cost[:, 1].cpu())
    hist = torch.stack(hist)
    falls = (hist[1:] < hist[:-1]).sum(0)
    print(f"[arm_ik] status {out.status.tolist()} strict decreases {falls.tolist()} yardstick float64 {falls64.tolist()} float32 "
          f"{y32['accepted'].tolist()} cost {out.cost.cpu().tolist()}")
    assert bool((hist[1:] <= hist[:-1]).all())
    assert out.status.cpu().tolist() == falls.tolist()
    assert out.status.cpu().tolist() == falls64.tolist() and y["accepted"].tolist() == falls64.tolist()
    assert int(falls64.min()) < iters                     # some step was rejected
    assert bool(torch.isfinite(_x(out)).all())
    rejected = hist[1:] == hist[:-1]
    k = int(torch.nonzero(rejected.any(1))[0]) + 1
    fr = torch.nonzero(rejected[k - 1]).reshape(-1)
    out = _solve(arm["dm"], x0, b, tg, iters=k, joints=True, jac=True, **R.PRIORS)
    xk = _x(out)[fr]
    n64 = R.normal(s["model"], xk, b.double(), tg[fr], **R.PRIORS)
    n32 = R.normal(s["model"], xk.float(), b, tg[fr], dtype=torch.float32, **R.PRIORS)
    got = dict(joints=out.joints.cpu()[fr] / 1000.0, jac=out.jac.cpu()[fr], cost=out.cost[:, 1:].cpu()[fr])
    with torch.no_grad():
        ref = dict(joints=R.joints(s["model"], xk, b.double()), jac=n64["J"], cost=n64["C"][:, None])
        f32 = dict(joints=R.joints(s["model"], xk.float(), b, torch.float32), jac=n32["J"], cost=n32["C"][:, None])
    print(f"[arm_ik] kept x after a rejected step {k} frames {fr.tolist()} " +
          " ".join(f"{q} {_rel(got[q], ref[q]):.3e} (bound {R.FACTOR * _rel(f32[q], ref[q]):.3e})" for q in got))
    for q in got:
        assert _rel(got[q], ref[q]) <= R.FACTOR * _rel(f32[q], ref[q]), q


# ---- 5. what is not written ---------------------------------------------------------------------------------------------------------------
def test_held_wrist_and_too_few_joints(arm, exact22):
    sc = exact22
    T = 3
    x0, tg, b = sc["x0_32"][:T].clone(), sc["targets32"][:T], sc["betas32"]
    x0[:, R.XW:R.XP] = torch.as_tensor(np.random.default_rng(5).normal(size=(T, 3)) * 0.2, dtype=torch.float32)
    kw = dict(R.PRIORS, iters=4, joints=True, jac=True)
    held = _solve(arm["dm"], x0, b, tg, solve_wrist=False, **kw)
    assert torch.equal(_bits(held.in_pose[:, 1]), _bits(x0[:, R.XW:R.XP])) and int(held.status.min()) >= 1
    assert not torch.equal(_bits(held.in_pose[:, 0]), _bits(x0[:, :3]))
    for n_used, solved in ((2, False), (3, True)):        # the middle frame; its neighbours do not notice
        w = torch.ones(T, NO)
        w[1] = 0.0
        w[1, [0, 9, 21][:n_used]] = 1.0
        out = _solve(arm["dm"], x0, b, tg, weights=w, **kw)
        st = out.status.tolist()
        assert (st[1] >= 0) == solved and (solved or st[1] == -1) and min(st[0], st[2]) >= 1
        if not solved:
            assert torch.equal(_bits(_x(out)[1].float()), _bits(x0[1])) and torch.equal(_bits(out.cost[1, 0]), _bits(out.cost[1, 1]))
        else:
            assert float(out.cost[1, 1]) <= float(out.cost[1, 0]) and bool(torch.isfinite(_x(out)).all())
        for f in (0, 2):
            alone = _solve(arm["dm"], x0[f:f + 1], b, tg[f:f + 1], weights=w[f:f + 1], **kw)
            assert all(torch.equal(_bits(p[f]), _bits(q[0])) for p, q in zip(out, alone) if p is not None), (n_used, f)
    # unused joints never enter: whatever stands under a zero weight, and a NaN under a weight of one
    zero = [2, 11, 21]
    w = torch.ones(T, NO)
    w[:, zero] = 0.0
    outs = []
    for fill in (1e30, float("nan"), 0.0):
        t = tg.clone()
        t[:, zero] = fill
        outs.append(_solve(arm["dm"], x0, b, t, weights=w, **kw))
    t = tg.clone()
    t[:, zero] = float("nan")
    assert _same(outs[0], outs[2]) and _same(outs[1], outs[2]) and _same(_solve(arm["dm"], x0, b, t, **kw), outs[2])


# ---- 6. repeatable and capturable -------------------------------------------------------------------------------------------------------
def test_repeatable_and_capturable(arm, exact22):
    from harp_amd import ops
    sc = exact22
    T = sc["x0_32"].shape[0]
    wp = torch.as_tensor(np.random.default_rng(6).normal(size=(T, 3)) * 0.1, dtype=torch.float32)
    kw = dict(R.PRIORS, iters=6, joints=True, jac=True)
    a = _solve(arm["dm"], sc["x0_32"], sc["betas32"], sc["targets32"], wrist_prior=wp, **kw)
    b = _solve(arm["dm"], sc["x0_32"], sc["betas32"], sc["targets32"], wrist_prior=wp, **kw)
    assert _same(a, b) and int(a.status.min()) >= 1
    # one captured call through out=, replayed on fresh inputs
    x0 = sc["x0_32"]
    targets, in_pose, trans, wprior = (_f32(t).clone() for t in (sc["targets32"], x0[:, :R.XT].reshape(T, 17, 3), x0[:, R.XT:], wp))
    betas = _f32(sc["betas32"])
    out = ops.arm_ik(arm["dm"], betas, targets, in_pose, trans, wrist_prior=wprior, **kw)     # warm-up outside the capture; its tensors are reused
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.arm_ik(arm["dm"], betas, targets, in_pose, trans, wrist_prior=wprior, out=out, **kw)
    for order in (torch.arange(T), torch.arange(T - 1, -1, -1)):                              # fresh inputs: the frames in another order
        targets.copy_(_f32(sc["targets32"][order])); in_pose.copy_(_f32(x0[order, :R.XT].reshape(T, 17, 3)))
        trans.copy_(_f32(x0[order, R.XT:])); wprior.copy_(_f32(wp[order]))
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(p[order]), _bits(q)) for p, q in zip(a, out)), order[:4]


def test_refusals_with_real_buffers(arm):
    from harp_amd import ops
    dm, dev = arm["dm"], torch.device(DEV)
    T = 2
    z = lambda *s: torch.zeros(*s, device=dev)
    tg, ip, b, tr = z(T, NO, 3), z(T, 17, 3), z(10), z(T, 3)
    assert ops.arm_ik(dm, b, tg, ip, tr, iters=0).status.tolist() == [0, 0]
    with pytest.raises(ValueError, match="targets"):
        ops.arm_ik(dm, b, tg[:, :21].contiguous(), ip, tr)
    with pytest.raises(ValueError, match="in_pose"):
        ops.arm_ik(dm, b, tg, ip.reshape(T, 51), tr)
    with pytest.raises(ValueError, match="betas"):
        ops.arm_ik(dm, z(3, 10), tg, ip, tr)
    with pytest.raises(ValueError, match="wrist_prior"):
        ops.arm_ik(dm, b, tg, ip, tr, wrist_prior=z(3))
    with pytest.raises(ValueError):
        ops.arm_ik(dm, b, tg, ip, tr, wrist_prior_weight=-1.0)
    with pytest.raises(TypeError):
        ops.arm_ik(dm, b, tg.double(), ip, tr)
    with pytest.raises(RuntimeError):
        ops.arm_ik(dm, b, tg, ip.clone().requires_grad_(), tr)
    with pytest.raises(ValueError, match="out.joints"):
        ops.arm_ik(dm, b, tg, ip, tr, joints=True, out=ops.arm_ik(dm, b, tg, ip, tr, iters=0))


# ---- 7. the layer ---------------------------------------------------------------------------------------------------------------------------
def _playback_scene(tmp_path, T=5, S=32):
    from harp_amd.playback import Motion
    from tests.test_gpu_avatar_player import _arm_setup
    cfg, layer, params = _arm_setup(T, S, 3, tmp_path)
    true = Motion.from_params(params)
    betas = params["shape"].detach().reshape(1, 10).expand(T, 10).contiguous()

    def forward(m):
        with torch.no_grad():
            return layer(betas=betas, global_orient=m.rot.to(DEV), transl=m.trans.to(DEV), right_hand_pose=m.pose.to(DEV),
                         right_wrist_pose=m.wrist_pose.to(DEV))[1]

    return cfg, layer, params, true, forward


def test_motion_from_arm_keypoints_drives_the_player(tmp_path, exact22):
    from harp_amd.playback import AvatarPlayer, Motion
    T = 5
    cfg, layer, params, true, forward = _playback_scene(tmp_path, T)
    assert true.wrist_pose is not None and bool((true.wrist_pose != 0).any())
    kp = forward(true) / 1000.0
    assert tuple(kp.shape) == (T, 22, 3)
    player = AvatarPlayer(cfg, params, layer, batch_size=T, ss=1, device=DEV)
    white = lambda fr: int((fr.cpu() != 255).any(-1).sum())
    player.load_motion(true)
    n_true = white(player.render(np.arange(T)))
    sc = exact22
    bound = R.FACTOR * float(R.joint_dist_mm(sc["model"], sc["y32"]["x"], sc["betas32"], sc["targets32"], None, torch.float32)[1].max())
    dist = lambda a, b: float((a - b).double().norm(dim=-1).max() * 1000.0)
    for width, targets, kw in ((22, kp, {}), (21, kp[:, :21], dict(wrist_pose=true.wrist_pose))):
        rec = Motion.from_arm_keypoints(targets, params, layer, **kw)
        assert len(rec) == T and rec.light_positions is None and rec.wrist_pose is not None
        assert torch.equal(rec.cam.cpu(), params["cam"][0].detach().cpu().expand(T, 3))
        if width == 21:
            assert torch.equal(_bits(rec.wrist_pose), _bits(true.wrist_pose))
        got = forward(rec) / 1000.0
        d = dist(got[:, :width], targets)
        print(f"[arm_ik] layer[{width}] largest joint distance {d:.3e} mm (bound {bound:.3e}, test 3's)")
        assert d <= bound
        # someone else's proportions: 1.2 x about the wrist gives the same motion; without the match it does not
        big = targets[:, :1] + 1.2 * (targets - targets[:, :1])
        same = forward(Motion.from_arm_keypoints(big, params, layer, **kw)) / 1000.0
        off = forward(Motion.from_arm_keypoints(big, params, layer, match_bone_lengths=False, **kw)) / 1000.0
        d_same, d_off = dist(same, got), dist(off[:, :width], targets)
        print(f"[arm_ik] layer[{width}] 1.2 x keypoints: joints moved {d_same:.3e} mm (bound {bound:.3e}); unmatched {d_off:.3e} mm from the targets")
        assert d_same <= bound and d_off > bound
        player.load_motion(Motion(rec.pose, rec.rot, rec.trans, true.cam, wrist_pose=rec.wrist_pose))   # the true motion's per-frame cam
        n_rec = white(player.render(np.arange(T)))
        print(f"[arm_ik] layer[{width}] covered pixels true {n_true} recovered {n_rec}")
        assert n_true > 0 and abs(n_rec - n_true) <= 0.01 * n_true
        warm = Motion.from_arm_keypoints(targets, params, layer, init=rec, iters=1, **(dict(wrist_pose=np.zeros(3)) if width == 22 else kw))
        assert float((warm.pose - rec.pose).abs().max()) < 1e-3
    # a frame without its elbow is still solved; smoothing takes both widths
    w = torch.ones(T, 22)
    w[2, 21] = 0.0
    gone = kp.clone()
    gone[3, 21] = float("nan")
    rec = Motion.from_arm_keypoints(gone, params, layer, weights=w)
    d = dist((forward(rec) / 1000.0)[:, :21], kp[:, :21])
    print(f"[arm_ik] layer elbow missing in two frames: largest hand joint distance {d:.3e} mm (bound {bound:.3e})")
    assert d <= bound and bool(torch.isfinite(rec.wrist_pose).all())
    for targets in (kp, kp[:, :21]):
        sm = Motion.from_arm_keypoints(targets, params, layer, smooth=1.0)
        assert len(sm) == T and bool(torch.isfinite(sm.pose).all())
    with pytest.raises(NotImplementedError, match="from_arm_keypoints"):
        Motion.from_keypoints(kp[:, :21], params, layer)


@pytest.mark.parametrize("width", [21, 22])
def test_command_line_takes_arm_keypoints(tmp_path, monkeypatch, width):
    """python -m harp_amd.playback's main() with --keypoints on a use_arm config (the two loaders of licensed / fitted files replaced by the
    synthetic scene, as tests/test_gpu_avatar_player.py does): keypoints of either width in, frames out"""
    import os
    import yaml
    from PIL import Image
    from harp_amd import playback
    from harp_amd.utils import file_utils, hand_model_utils
    T, S = 5, 32
    cfg, layer, params, true, forward = _playback_scene(tmp_path, T, S)
    assert cfg["use_arm"]
    monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda c: (layer, params["verts_uvs"], params["faces_uvs"], None))
    monkeypatch.setattr(file_utils, "load_result", lambda base, device="cuda", test=False: dict(params))
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump({k: cfg[k] for k in ("use_arm", "img_size", "focal_length", "self_shadow", "share_light_position", "base_output_dir")}, f)
    kp = (forward(true) / 1000.0).cpu().numpy()
    extra = {} if width == 22 else dict(wrist_pose=true.wrist_pose.cpu().numpy())
    np.savez(tmp_path / "k.npz", keypoints=kp[:, :width], cam=true.cam.cpu().numpy(), weights=np.ones((T, width), np.float32), **extra)
    out = tmp_path / "frames"
    paths = playback.main(["--config", str(tmp_path / "cfg.yaml"), "--out", str(out), "--keypoints", str(tmp_path / "k.npz"), "--batch-size", "4",
                           "--smooth-keypoints", "0.5"])
    assert sorted(os.listdir(out)) == ["%04d.jpg" % i for i in range(T)] and len(paths) == T
    assert Image.open(paths[0]).size == (S, S)
