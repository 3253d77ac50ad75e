"""-m gpu: harp_arm_vertex_fit (csrc/arm_vertex_fit.hip), optimize_for_mano_arm_param(method="lm") and Motion.from_arm_vertices against the
yardstick of tests/_arm_fit_ref.py.

No bound here is a number fixed in advance.  Each is computed in the test from the yardstick itself:

    bound = 8 x the float32 yardstick's error against the float64 yardstick on the same inputs            (R.FACTOR)

— the same code in float32 (forward, J^T W J, Cholesky of the Jacobi-scaled system) is the error model of a correct float32 solver, and the
factor covers what the kernel does differently: its dots summed in another order, the root column as a rotation of the wrist-relative
vertex, and the device's sinf / cosf.  Both sides of every comparison are the worst over all the frames that the test runs, never one
frame's.  Measured errors and bounds are recorded side by side in profiles/arm_vertex_fit_errors.txt and DESIGN.md §28.  Every test prints
its figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import _arm_fit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NV, TILE = 1026, 64
# targets whose weight is zero in the weighted cases: both sides of the kernel's 64-target tile boundaries, of the 256-target rounds of its
# forward, and (with all 1026) both targets of the last, 17th tile
W_ZERO = [0, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 511, 512, 575, 576, 767, 768, 769, 1023, 1024, 1025]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _f32(t):
    return None if t is None else t.to(torch.float32).to(DEV).contiguous()


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b) if x is not None)


def _x(out):
    T = out.in_pose.shape[0]
    b = out.betas if out.betas.dim() == 2 else out.betas[None].expand(T, 10)
    return torch.cat([out.in_pose.reshape(T, 51), b, out.trans], 1).cpu().double()


@pytest.fixture(scope="module")
def arm():
    from harp_amd.hand_models_harp.body_models import TreeDeviceModel
    m_np, m, mano = R.arm_model()
    return dict(np=m_np, model=m, mano=mano, dm=TreeDeviceModel(m_np, torch.device(DEV)))


def _solve(arm, x0, targets, idx=None, betas=None, **kw):
    """x0 (T,64) holds the start; betas: None = x0's own (T,10), else what is passed for a frozen shape"""
    from harp_amd import ops
    T = x0.shape[0]
    b = x0[:, R.XB:R.XT] if betas is None else betas
    vi = None if idx is None else torch.as_tensor(np.asarray(idx)).to(DEV)
    return ops.arm_vertex_fit(arm["dm"], _f32(targets), _f32(x0[:, :R.XB].reshape(T, 17, 3)), _f32(b), _f32(x0[:, R.XT:]), vert_idx=vi, **kw)


def _yard(name, iters64, iters32=10):
    sc, kw = R.gpu_scene(name)
    sc["kw"] = kw
    sc["y64"] = R.lm(sc["model"], sc["x0_32"].double(), sc["targets32"].double(), idx=sc["idx"], iters=iters64, **kw)
    sc["y32"] = R.lm(sc["model"], sc["x0_32"], sc["targets32"], idx=sc["idx"], iters=iters32, dtype=torch.float32, **kw)
    return sc


@pytest.fixture(scope="module")
def exact_all():
    return _yard("exact_all", 10)


@pytest.fixture(scope="module")
def exact_mano():
    return _yard("exact_mano", 10)


@pytest.fixture(scope="module")
def noisy_all():
    return _yard("noisy_all", 20)


# ---- 1. iters = 0 at the input ----------------------------------------------------------------------------------------------------------
def _poses(kind, T, pose_mean, rng):
    x = np.zeros((T, R.NX), np.float32)
    if kind == "aa_zero":                                 # stored pose = -pose_mean: every hand joint's axis-angle is exactly 0
        x[:, R.XP:R.XB] = -pose_mean[120:165]
    elif kind == "tiny":
        x[:, :R.XB] = 1e-6
    elif kind == "random":
        x[:, :R.XB] = rng.normal(size=(T, 51)) * 0.3
    elif kind == "near_pi":
        x[:, R.XW:R.XB] = rng.normal(size=(T, 48)) * 0.3
        u = rng.normal(size=(T, 3))
        x[:, :3] = (np.pi - 1e-3) * u / np.linalg.norm(u, axis=1, keepdims=True)
    return x


def _rel(got, ref):
    """per frame: the largest deviation relative to the frame's largest entry of the quantity"""
    T = ref.shape[0]
    d, m = (got.double() - ref.double()).abs().reshape(T, -1).amax(1), ref.double().abs().reshape(T, -1).amax(1)
    return float((d / m).max())


# (targets, T, betas: solved / frozen given as, wrist solved or frozen non-zero, trans, weights)
_CASES = [("all", 1, (True, "per_frame"), True, False, False), ("mano", 2, (False, "shared"), False, True, True),
          (65, 3, (False, "per_frame"), True, True, True), (64, 2, (True, "per_frame"), False, False, False),
          (22, 1, (True, "per_frame"), True, True, False), ("all", 3, (False, "shared"), True, True, True)]


@pytest.mark.parametrize("kind", ["zero", "aa_zero", "tiny", "random", "near_pi"])
def test_everything_at_the_input(arm, kind):
    """iters = 0 evaluates at the input: verts, jac, A, g and cost[:, 0] against float64, each relative to the frame's largest entry of
    that quantity; the in/out rows come back bit for bit; the frozen columns of A and g are exactly the contract's.  T = 1, 2, 3 around
    the frames per workgroup; all 1026 targets (a 17th tile with 2), the 778 of right_mano_idx (unsorted), 65, 64 and 22 random ones;
    betas solved / frozen as (10,) / frozen as (T,10); the wrist solved / frozen at a non-zero value; trans zero / not; weights None / a
    pattern of zeros across the tile boundaries with a NaN target under a weight of 1."""
    from harp_amd import ops
    F = ops.arm_vertex_fit_frames_per_block()
    model, mano = arm["model"], arm["mano"]
    pm = arm["np"]["pose_mean"].astype(np.float32)
    rng = np.random.default_rng(11)
    # the edges this test is about, from its own arguments
    assert NV % TILE == 2 and NV // TILE == 16 and bool((np.diff(mano) < 0).any()) and len(mano) == 778
    assert {c[1] for c in _CASES} >= {F, F + 1} and bool((pm[120:165] != 0).all())
    if kind == "aa_zero":
        assert bool((pm[120:165] + _poses(kind, 1, pm, rng)[0, R.XP:R.XB] == 0).all())
    names = ("verts", "jac", "A", "g", "cost")
    worst, worst32 = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0)
    for tset, T, (solve_shape, given), solve_wrist, with_trans, with_w in _CASES:
        idx = None if tset == "all" else (mano if tset == "mano" else rng.permutation(NV)[:tset])
        n_t = NV if idx is None else len(idx)
        x = _poses(kind, T, pm, rng)
        x[:, R.XB:R.XT] = rng.normal(size=10 if given == "shared" else (T, 10)) * 0.5
        if not solve_wrist:
            x[:, R.XW:R.XP] = rng.normal(size=(T, 3)) * 0.3
            assert bool((x[:, R.XW:R.XP] != 0).all())
        if with_trans:
            x[:, R.XT:] = rng.uniform(-0.3, 0.3, size=(T, 3))
        x = torch.as_tensor(x)
        targets = torch.as_tensor(rng.uniform(-0.3, 0.3, size=(T, n_t, 3)), dtype=torch.float32)
        w = None
        if with_w:
            zero = [i for i in W_ZERO if i < n_t]
            w = torch.as_tensor(rng.uniform(0.5, 1.5, size=(T, n_t)), dtype=torch.float32)
            w[:, zero] = 0.0
            targets[:, 30] = float("nan")                 # unused although its weight is positive
            targets[:, zero[:3]] = float("nan")           # ... and NaN under a zero weight
            assert {i // TILE for i in zero} >= set(range(min(4, n_t // TILE))) and n_t - len(zero) - 1 >= R.MIN_USED
        betas = x[0, R.XB:R.XT].clone() if given == "shared" else x[:, R.XB:R.XT].clone()
        kw = dict(pose_prior_weight=1e-3, wrist_prior_weight=3e-3, shape_prior_weight=2e-3, solve_shape=solve_shape, solve_wrist=solve_wrist)
        out = _solve(arm, x, targets, idx=idx, betas=betas, weights=_f32(w), iters=0, verts=True, jac=True, normal=True, **kw)
        assert torch.equal(_bits(out.in_pose.reshape(T, 51)), _bits(x[:, :R.XB])) and torch.equal(_bits(out.trans), _bits(x[:, R.XT:]))
        assert torch.equal(_bits(out.betas), _bits(betas)) and out.status.tolist() == [0] * T
        assert torch.equal(_bits(out.cost[:, 0]), _bits(out.cost[:, 1]))
        assert tuple(out.verts.shape) == (T, NV, 3) and tuple(out.jac.shape) == (T, 3 * n_t, 64)
        A, g = out.A.cpu(), out.g.cpu()
        fz = R.frozen_columns(solve_shape, solve_wrist)
        if fz:
            off = A.clone()
            off[:, fz, fz] -= 1.0
            assert bool((off[:, fz, :] == 0).all() and (off[:, :, fz] == 0).all() and (g[:, fz] == 0).all())
        assert torch.equal(A, A.transpose(1, 2))
        n64 = R.normal(model, x.double(), targets, idx=idx, weights=w, **kw)
        n32 = R.normal(model, x, targets, idx=idx, weights=w, dtype=torch.float32, **kw)
        with torch.no_grad():
            v64, v32 = R.verts(model, x.double()), R.verts(model, x, None, torch.float32)
        got = dict(verts=out.verts.cpu() / 1000.0, jac=out.jac.cpu(), A=A, g=g, cost=out.cost[:, :1].cpu())
        ref = dict(verts=v64, jac=n64["J"], A=n64["A"], g=n64["g"], cost=n64["C"][:, None])
        f32 = dict(verts=v32, jac=n32["J"], A=n32["A"], g=n32["g"], cost=n32["C"][:, None])
        for k in names:
            worst[k], worst32[k] = max(worst[k], _rel(got[k], ref[k])), max(worst32[k], _rel(f32[k], ref[k]))
    print(f"[arm_vertex_fit] input[{kind}] " + " ".join(f"{k} {worst[k]:.3e} (bound {R.FACTOR * worst32[k]:.3e})" for k in names))
    for k in names:
        assert worst[k] <= R.FACTOR * worst32[k], k


# ---- 2. one step from the rigid start -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["exact_all", "exact_mano"])
def test_one_step_from_the_rigid_start(arm, name):
    sc, kw = R.gpu_scene(name)
    counted, y1, y1_32 = R.counted_first_step(sc, kw)
    assert bool(counted.all())                            # (8 frames: the yardstick leaves out none, asserted on the CPU as well)
    x0 = sc["x0_32"].double()
    out = _solve(arm, sc["x0_32"], sc["targets32"], idx=sc["idx"], iters=1, **kw)
    step = (y1["x"] - x0).abs().amax(1)
    c1 = y1["cost"][1]
    dx = float(((_x(out) - y1["x"]).abs().amax(1) / step).max())
    dx32 = float(((y1_32["x"].double() - y1["x"]).abs().amax(1) / step).max())
    dc = float(((out.cost[:, 1].cpu().double() - c1).abs() / c1).max())
    dc32 = float(((y1_32["cost"][1].double() - c1).abs() / c1).max())
    print(f"[arm_vertex_fit] one_step[{name}] x {dx:.3e} (bound {R.FACTOR * dx32:.3e}) cost1 {dc:.3e} (bound {R.FACTOR * dc32:.3e}) "
          f"counted {int(counted.sum())} of {counted.numel()}")
    assert out.status.cpu().tolist() == [1] * 8
    assert dx <= R.FACTOR * dx32
    assert dc <= R.FACTOR * dc32


# ---- 3. ten iterations ------------------------------------------------------------------------------------------------------------------
def _rms_of(out, sc):
    v = out.verts.cpu().double() / 1000.0
    v = v if sc["idx"] is None else v[:, torch.as_tensor(sc["idx"])]
    return float((v - sc["targets32"].double()).pow(2).sum(-1).mean(1).sqrt().max() * 1000.0)


@pytest.mark.parametrize("name", ["exact_all", "exact_mano"])
def test_convergence_on_exact_frames(arm, name, request):
    sc = request.getfixturevalue(name)
    out = _solve(arm, sc["x0_32"], sc["targets32"], idx=sc["idx"], iters=10, verts=True, **sc["kw"])
    rms = _rms_of(out, sc)
    rms32 = float(R.rms_mm(sc["model"], sc["y32"]["x"], sc["targets32"], sc["idx"], torch.float32).max())
    rms64 = float(R.rms_mm(sc["model"], sc["y64"]["x"], sc["targets32"], sc["idx"]).max())
    print(f"[arm_vertex_fit] convergence[{name}] rms {rms:.3e} mm (bound {R.FACTOR * rms32:.3e}; float64 yardstick {rms64:.3e}) "
          f"status {out.status.tolist()}")
    assert int(out.status.min()) >= 1
    assert rms <= R.FACTOR * rms32
    if not sc["kw"]["solve_wrist"]:
        assert bool((out.in_pose[:, 1] == 0).all())      # held at the zero it came with


def test_convergence_on_noisy_frames(arm, noisy_all):
    sc = noisy_all
    out = _solve(arm, sc["x0_32"], sc["targets32"], iters=10, **sc["kw"])
    c20 = sc["y64"]["cost"][20]
    m = float((out.cost[:, 1].cpu().double() / c20 - 1.0).max())
    m32 = float((sc["y32"]["cost"][10].double() / c20 - 1.0).abs().max())
    print(f"[arm_vertex_fit] convergence noisy cost/yardstick - 1 {m:.3e} (bound {R.FACTOR * m32:.3e}) "
          f"rms {float((c20 / NV).sqrt().mean() * 1000):.3f} mm")
    assert m <= R.FACTOR * m32


def test_fixed_shape_on_another_arm(arm, exact_all):
    sc = exact_all
    avatar = torch.as_tensor(np.random.default_rng(3).normal(size=10) * 0.5, dtype=torch.float32)
    x0 = R.rigid_x0(sc, targets=sc["targets32"], betas=avatar.double()[None]).float()
    kw = dict(solve_shape=False)
    y64 = R.lm(sc["model"], x0.double(), sc["targets32"].double(), iters=20, **kw)
    y32 = R.lm(sc["model"], x0, sc["targets32"], iters=10, dtype=torch.float32, **kw)
    c20 = y64["cost"][20]
    for betas in (avatar, avatar[None].expand(8, 10).contiguous()):
        out = _solve(arm, x0, sc["targets32"], betas=betas, iters=10, **kw)
        assert torch.equal(_bits(out.betas), _bits(betas))
        m = float((out.cost[:, 1].cpu().double() / c20 - 1.0).abs().max())
        m32 = float((y32["cost"][10].double() / c20 - 1.0).abs().max())
        print(f"[arm_vertex_fit] fixed shape {tuple(betas.shape)} cost/yardstick - 1 {m:.3e} (bound {R.FACTOR * m32:.3e}) "
              f"rms {float((c20 / NV).sqrt().mean() * 1000):.3f} mm")
        assert float(out.cost[:, 1].min()) > 0.0
        assert m <= R.FACTOR * m32


# ---- 4. status ----------------------------------------------------------------------------------------------------------------------------
def test_too_few_targets_are_returned_as_they_came(arm, exact_all):
    sc = exact_all
    T = 3
    x0, tg = sc["x0_32"][:T], sc["targets32"][:T]
    kw = dict(iters=4, verts=True, jac=True, normal=True)
    assert R.MIN_USED == 22 and 3 * 21 < R.NX <= 3 * 22
    for n_used, solved in ((21, False), (22, True)):      # the middle frame; its neighbours do not notice
        w = torch.ones(T, NV)
        w[1] = 0.0
        w[1, 47 * torch.arange(n_used)] = 1.0
        assert int((w[1] > 0).sum()) == n_used
        out = _solve(arm, x0, tg, weights=_f32(w), **kw)
        st = out.status.tolist()
        assert (st[1] >= 0) == solved and (solved or st[1] == -1) and min(st[0], st[2]) >= 1
        if not solved:
            assert torch.equal(_bits(_x(out)[1].float()), _bits(x0[1])) and torch.equal(_bits(out.cost[1, 0]), _bits(out.cost[1, 1]))
        else:
            assert float(out.cost[1, 1]) <= float(out.cost[1, 0]) and bool(torch.isfinite(_x(out)).all())
        for f in (0, 2):
            alone = _solve(arm, x0[f:f + 1], tg[f:f + 1], weights=_f32(w[f:f + 1]), **kw)
            assert all(torch.equal(_bits(a[f]), _bits(b[0])) for a, b in zip(out, alone) if a is not None), (n_used, f)
    # unused targets never enter: whatever stands under a zero weight, and a NaN under a weight of one
    w = torch.ones(T, NV)
    w[:, W_ZERO] = 0.0
    outs = []
    for fill in (1e30, float("nan"), 0.0):
        t = tg.clone()
        t[:, W_ZERO] = fill
        outs.append(_solve(arm, x0, t, weights=_f32(w), **kw))
    t = tg.clone()
    t[:, W_ZERO] = float("nan")
    assert _same(outs[0], outs[2]) and _same(outs[1], outs[2]) and _same(_solve(arm, x0, t, **kw), outs[2])


def test_status_counts_the_strict_decreases(arm):
    """from zero (no rigid start) on targets rotated by 3 rad the first steps overshoot.  The kernel is deterministic, so the run with k
    iterations is the prefix of the run with k + 1: the cost after every iteration is read from 12 calls, and the status must be the
    number of strict decreases in that history."""
    iters = 12
    s = R.scene(T=6, seed=1, root_lo=3.0, root_hi=3.0)
    assert bool(((s["x_true"][:, :3].norm(dim=1) - 3.0).abs() < 1e-12).all())
    x0, tg = torch.zeros(6, R.NX), s["targets"].float()
    hist = [_solve(arm, x0, tg, iters=0).cost[:, 0].cpu()]
    for k in range(1, iters + 1):
        out = _solve(arm, x0, tg, iters=k)
        assert torch.equal(_bits(out.cost[:, 0]), _bits(hist[0]))
        hist.append(out.cost[:, 1].cpu())
    hist = torch.stack(hist)
    falls = (hist[1:] < hist[:-1]).sum(0)
    print(f"[arm_vertex_fit] status {out.status.tolist()} strict decreases {falls.tolist()} cost {out.cost.cpu().tolist()}")
    assert bool((hist[1:] <= hist[:-1]).all())
    assert out.status.cpu().tolist() == falls.tolist()
    assert bool(torch.isfinite(_x(out)).all())
    # the optional outputs are at the FINAL x, also when the last step was rejected: the first k whose step some frame rejected far from
    # convergence, those frames, against the yardstick's normal equations at the x that came back
    rejected = (hist[1:] == hist[:-1]) & (hist[1:] > 1e-2 * hist[0])
    k = int(torch.nonzero(rejected.any(1))[0]) + 1
    fr = torch.nonzero(rejected[k - 1]).reshape(-1)
    assert len(fr) >= 1 and k < iters
    out = _solve(arm, x0, tg, iters=k, verts=True, jac=True, normal=True)
    xk = _x(out)[fr]
    n64 = R.normal(s["model"], xk, tg[fr])
    n32 = R.normal(s["model"], xk.float(), tg[fr], dtype=torch.float32)
    with torch.no_grad():
        v64, v32 = R.verts(s["model"], xk), R.verts(s["model"], xk.float(), None, torch.float32)
    got = dict(verts=out.verts.cpu()[fr] / 1000.0, jac=out.jac.cpu()[fr], A=out.A.cpu()[fr], g=out.g.cpu()[fr], cost=out.cost[:, 1:].cpu()[fr])
    ref = dict(verts=v64, jac=n64["J"], A=n64["A"], g=n64["g"], cost=n64["C"][:, None])
    f32 = dict(verts=v32, jac=n32["J"], A=n32["A"], g=n32["g"], cost=n32["C"][:, None])
    print(f"[arm_vertex_fit] final x after a rejected step {k} frames {fr.tolist()} " +
          " ".join(f"{q} {_rel(got[q], ref[q]):.3e} (bound {R.FACTOR * _rel(f32[q], ref[q]):.3e})" for q in got))
    for q in got:
        assert _rel(got[q], ref[q]) <= R.FACTOR * _rel(f32[q], ref[q]), q


def test_constant_corrective_rows(arm):
    """A model whose undriven joints have a pose mean (the real model's left hand: pose_src < 0, pose_mean != 0): their corrective rows are
    constant and NOT zero — they belong in every forward and never in the Jacobian — while the rows of an undriven joint with a zero mean
    are exactly zero (Rodrigues of 0 is the identity exactly, in float32 as well)."""
    from harp_amd.hand_models_harp.body_models import TreeDeviceModel
    from oracle import harp_ref
    m_np = dict(arm["np"])
    pm = m_np["pose_mean"].copy()
    pm[75:120] = (np.random.default_rng(8).normal(size=45) * 0.05).astype(np.float32)        # joints 25..39: the left hand
    m_np["pose_mean"] = pm
    model = dict(arm["model"], pose_mean=torch.from_numpy(pm).double())
    rot = harp_ref.smplx_batch_rodrigues(torch.from_numpy(pm).reshape(55, 3))
    eye = torch.eye(3)
    undriven = [j for j in range(1, 55) if j != 21 and j < 40]
    assert all((not torch.equal(rot[j], eye)) == (25 <= j < 40) for j in undriven)            # non-zero rows, and exactly zero rows
    arm2 = dict(arm, np=m_np, model=model, dm=TreeDeviceModel(m_np, torch.device(DEV)))
    rng = np.random.default_rng(9)
    names = ("verts", "jac", "g", "cost")
    worst, worst32, moved = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0), 0.0
    for idx, T in ((None, 2), (arm["mano"], 1)):
        x = torch.as_tensor(rng.normal(size=(T, R.NX)) * 0.3, dtype=torch.float32)
        n_t = NV if idx is None else len(idx)
        targets = torch.as_tensor(rng.uniform(-0.3, 0.3, size=(T, n_t, 3)), dtype=torch.float32)
        out = _solve(arm2, x, targets, idx=idx, iters=0, verts=True, jac=True, normal=True)
        n64 = R.normal(model, x.double(), targets, idx=idx)
        n32 = R.normal(model, x, targets, idx=idx, dtype=torch.float32)
        with torch.no_grad():
            v64, v32 = R.verts(model, x.double()), R.verts(model, x, None, torch.float32)
            moved = max(moved, float((v64 - R.verts(arm["model"], x.double())).abs().max()) * 1000.0)
        got = dict(verts=out.verts.cpu() / 1000.0, jac=out.jac.cpu(), g=out.g.cpu(), cost=out.cost[:, :1].cpu())
        ref = dict(verts=v64, jac=n64["J"], g=n64["g"], cost=n64["C"][:, None])
        f32 = dict(verts=v32, jac=n32["J"], g=n32["g"], cost=n32["C"][:, None])
        for k in names:
            worst[k], worst32[k] = max(worst[k], _rel(got[k], ref[k])), max(worst32[k], _rel(f32[k], ref[k]))
    print(f"[arm_vertex_fit] constant rows (they move a vertex by up to {moved:.3f} mm) " +
          " ".join(f"{k} {worst[k]:.3e} (bound {R.FACTOR * worst32[k]:.3e})" for k in names))
    assert moved > 0.01                                   # far above every bound below: leaving the rows out cannot pass
    for k in names:
        assert worst[k] <= R.FACTOR * worst32[k], k


# ---- 5. repeatable and capturable -------------------------------------------------------------------------------------------------------
def test_repeatable_and_capturable(arm, exact_mano):
    from harp_amd import ops
    sc = exact_mano
    x0 = sc["x0_32"].clone()
    x0[:, R.XW:R.XP] = torch.as_tensor(np.random.default_rng(5).normal(size=(8, 3)) * 0.2, dtype=torch.float32)
    avatar = x0[:, R.XB:R.XT].clone() + 0.1
    kw = dict(iters=6, verts=True, jac=True, normal=True, solve_wrist=False, solve_shape=False)
    a = _solve(arm, x0, sc["targets32"], idx=sc["idx"], betas=avatar, **kw)
    b = _solve(arm, x0, sc["targets32"], idx=sc["idx"], betas=avatar, **kw)
    assert _same(a, b) and int(a.status.min()) >= 1
    # the rows of a frozen wrist and a frozen shape come back bit for bit
    assert torch.equal(_bits(a.in_pose[:, 1]), _bits(x0[:, R.XW:R.XP])) and torch.equal(_bits(a.betas), _bits(avatar))
    assert not torch.equal(_bits(a.in_pose[:, 0]), _bits(x0[:, :3]))
    # one captured call through out=, replayed on fresh inputs
    vi = torch.as_tensor(sc["idx"]).to(torch.int32).to(DEV)
    targets, in_pose, betas, trans = (_f32(t).clone() for t in (sc["targets32"], x0[:, :R.XB].reshape(8, 17, 3), avatar, x0[:, R.XT:]))
    out = ops.arm_vertex_fit(arm["dm"], targets, in_pose, betas, trans, vert_idx=vi, **kw)   # warm-up outside the capture; its tensors are reused
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.arm_vertex_fit(arm["dm"], targets, in_pose, betas, trans, vert_idx=vi, out=out, **kw)
    for order in (torch.arange(8), torch.arange(7, -1, -1)):                                # fresh inputs: the frames in another order
        targets.copy_(_f32(sc["targets32"][order])); in_pose.copy_(_f32(x0[order, :R.XB].reshape(8, 17, 3)))
        betas.copy_(_f32(avatar[order])); trans.copy_(_f32(x0[order, R.XT:]))
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(x[order]), _bits(y)) for x, y in zip(a, out)), order[:4]


# ---- 6. refusals with real buffers --------------------------------------------------------------------------------------------------------
def test_refusals_with_real_buffers(arm):
    import ctypes
    from harp_amd import _lib, ops
    from harp_amd.hand_models_harp.body_models import TreeDeviceModel
    dm, dev = arm["dm"], torch.device(DEV)
    T = 2
    z = lambda *s: torch.zeros(*s, device=dev)
    tg, ip, b, tr = z(T, NV, 3), z(T, 17, 3), z(T, 10), z(T, 3)
    cost, status = z(T, 2), torch.zeros(T, dtype=torch.int32, device=dev)
    idx = torch.arange(778, dtype=torch.int32, device=dev)
    p = _lib.ptr

    def call(m=None, vi=None, n_t=NV, T_=T, opt=(10, 1e-3, 0.0, 0.0, 0.0, 1, 1, 0), **null):
        a = dict(targets=p(tg), in_pose=p(ip), betas=p(b), trans=p(tr), cost=p(cost), status=p(status))
        a.update(null)
        return _lib.lib().harp_arm_vertex_fit(ctypes.byref((m or dm).struct), vi, n_t, a["targets"], None, None, T_,
                                              ctypes.byref(_lib.ArmVertexFitOptions(*opt)), a["in_pose"], a["betas"], a["trans"], a["cost"],
                                              a["status"], None, None, None, None, _lib.stream())

    assert call() == 0 and call(vi=p(idx), n_t=778) == 0
    torch.cuda.synchronize()
    for name in ("targets", "in_pose", "betas", "trans", "cost", "status"):
        assert call(**{name: None}) == 1, name
    assert call(T_=0) == 1 and call(n_t=0) == 1 and call(n_t=NV + 1, vi=p(idx)) == 1 and call(n_t=778) == 1
    nan, inf = float("nan"), float("inf")
    for pos in range(1, 5):
        for bad in (-1.0, nan, inf):
            o = [10, 1e-3, 0.0, 0.0, 0.0, 1, 1, 0]
            o[pos] = bad
            assert call(opt=tuple(o)) == 1, (pos, bad)
    assert call(opt=(-1, 1e-3, 0.0, 0.0, 0.0, 1, 1, 0)) == 1

    def changed(**kw):
        m = TreeDeviceModel(arm["np"], dev)
        for k, v in kw.items():
            setattr(m.struct, k, v)
        return m
    for kw in (dict(n_pose_in=16), dict(NB=9), dict(NB=33), dict(NJ=65), dict(NV=_lib.ARM_VERTEX_FIT_MAX_VERTS + 1), dict(center_joint=-1)):
        assert call(m=changed(**kw), vi=p(idx), n_t=778) == 1, kw
    # ops checks what the ABI cannot: the range of vert_idx, shapes, dtypes
    bad = idx.clone()
    bad[5] = NV
    with pytest.raises(ValueError, match="vert_idx"):
        ops.arm_vertex_fit(dm, tg[:, :778].contiguous(), ip, b, tr, vert_idx=bad)
    with pytest.raises(ValueError, match="vert_idx"):
        ops.arm_vertex_fit(dm, tg[:, :778].contiguous(), ip, b, tr, vert_idx=-idx - 1)
    with pytest.raises(ValueError, match="without vert_idx"):
        ops.arm_vertex_fit(dm, tg[:, :778].contiguous(), ip, b, tr)
    with pytest.raises(ValueError, match="in_pose"):
        ops.arm_vertex_fit(dm, tg, ip.reshape(T, 51), b, tr)
    with pytest.raises(TypeError):
        ops.arm_vertex_fit(dm, tg.double(), ip, b, tr)
    with pytest.raises(RuntimeError):
        ops.arm_vertex_fit(dm, tg, ip.requires_grad_(), b, tr)


# ---- 7. the layers ------------------------------------------------------------------------------------------------------------------------
def test_preprocessing_lm_against_adam(arm, capsys):
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    from harp_amd.metro_modifications import hand_utils as hu
    layer = SMPLXARM(arm["np"], arm["np"]["faces"], arm["mano"], device=DEV)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        verts, _ = layer(betas=torch.randn(4, 10, generator=g).to(DEV) * 0.3, global_orient=torch.randn(4, 3, generator=g).to(DEV) * 0.2,
                         transl=torch.randn(4, 3, generator=g).to(DEV) * 0.02, right_hand_pose=torch.randn(4, 45, generator=g).to(DEV) * 0.2,
                         return_type="mano")
    pred = verts.cpu() / 1000.0
    adam = hu.optimize_for_mano_arm_param(pred, layer)
    first = capsys.readouterr().out.splitlines()
    lm = hu.optimize_for_mano_arm_param(pred, layer, method="lm")
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 2 and len(first) == 2 and [l.split(":")[0] for l in lines] == [l.split(":")[0] for l in first]
    assert lines[0].startswith("After coarse alignment: ") and lines[1].startswith("After fine alignment: ")
    assert sorted(lm) == sorted(adam)
    for k in adam:
        assert lm[k].shape == adam[k].shape and lm[k].dtype == adam[k].dtype, k
    rms = lambda o: float(np.sqrt(((o["verts"].astype(np.float64) - pred.numpy().astype(np.float64) * 1000.0) ** 2).sum(-1).mean()))
    print(f"[arm_vertex_fit] preprocessing rms lm {rms(lm):.3e} mm adam {rms(adam):.3e} mm; printed {lines}")
    assert rms(lm) <= rms(adam)
    assert abs(float(lines[1].split(":")[1]) - rms(lm) ** 2 / 3.0) <= 1e-5 + 0.05 * rms(lm) ** 2


def _playback_scene(tmp_path, T=5, S=32):
    from harp_amd.playback import Motion
    from tests.test_gpu_avatar_player import _arm_setup
    cfg, layer, params = _arm_setup(T, S, 3, tmp_path)
    true = Motion.from_params(params)
    betas = params["shape"].detach().reshape(1, 10).expand(T, 10).contiguous()

    def forward(m):
        with torch.no_grad():
            return layer(betas=betas, global_orient=m.rot.to(DEV), transl=m.trans.to(DEV), right_hand_pose=m.pose.to(DEV),
                         right_wrist_pose=m.wrist_pose.to(DEV))[0]

    return cfg, layer, params, true, forward


def test_motion_from_arm_vertices_drives_the_player(tmp_path, exact_all, exact_mano):
    from harp_amd.playback import AvatarPlayer, Motion
    T = 5
    cfg, layer, params, true, forward = _playback_scene(tmp_path, T)
    assert true.wrist_pose is not None and bool((true.wrist_pose != 0).any())
    v = forward(true) / 1000.0
    mano = layer.right_mano_idx
    player = AvatarPlayer(cfg, params, layer, batch_size=T, ss=1, device=DEV)
    white = lambda fr: int((fr.cpu() != 255).any(-1).sum())
    player.load_motion(true)
    n_true = white(player.render(np.arange(T)))
    for width, sc, targets, kw in ((1026, exact_all, v, {}), (778, exact_mano, v[:, mano], dict(wrist_pose=true.wrist_pose))):
        rec = Motion.from_arm_vertices(targets, params, layer, **kw)
        assert len(rec) == T and rec.light_positions is None and rec.wrist_pose is not None
        assert torch.equal(rec.cam.cpu(), params["cam"][0].detach().cpu().expand(T, 3))
        if width == 778:
            assert torch.equal(_bits(rec.wrist_pose), _bits(true.wrist_pose))
        got = forward(rec) / 1000.0
        rms = float(((got if width == 1026 else got[:, mano]) - targets).double().pow(2).sum(-1).mean(1).sqrt().max() * 1000.0)
        bound = R.FACTOR * float(R.rms_mm(sc["model"], sc["y32"]["x"], sc["targets32"], sc["idx"], torch.float32).max())
        print(f"[arm_vertex_fit] layer[{width}] rms {rms:.3e} mm (bound {bound:.3e}, test 3's)")
        assert rms <= bound
        player.load_motion(Motion(rec.pose, rec.rot, rec.trans, true.cam, wrist_pose=rec.wrist_pose))   # the true motion's per-frame cam
        n_rec = white(player.render(np.arange(T)))
        print(f"[arm_vertex_fit] layer[{width}] covered pixels true {n_true} recovered {n_rec}")
        assert n_true > 0 and abs(n_rec - n_true) <= 0.01 * n_true
        warm = Motion.from_arm_vertices(targets, params, layer, init=rec, iters=1)
        assert float((warm.pose - rec.pose).abs().max()) < 1e-3
    with pytest.raises(NotImplementedError, match="from_arm_vertices"):
        Motion.from_vertices(v[:, mano], params, layer)
    with pytest.raises(ValueError):
        Motion.from_arm_vertices(v, params, layer, wrist_pose=np.zeros(3))
    with pytest.raises(ValueError):
        Motion.from_arm_vertices(v[:, :500], params, layer)


@pytest.mark.parametrize("width", [778, 1026])
def test_command_line_takes_arm_vertices(tmp_path, monkeypatch, width):
    """python -m harp_amd.playback's main() with --vertices on a use_arm config (the two loaders of licensed / fitted files replaced by the
    synthetic scene, as tests/test_gpu_avatar_player.py does): vertices of either width in, frames out"""
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
    v = (forward(true) / 1000.0).cpu().numpy()
    extra = {} if width == 1026 else dict(wrist_pose=true.wrist_pose.cpu().numpy())
    np.savez(tmp_path / "v.npz", vertices=v if width == 1026 else v[:, layer.right_mano_idx.cpu().numpy()], cam=true.cam.cpu().numpy(), **extra)
    out = tmp_path / "frames"
    paths = playback.main(["--config", str(tmp_path / "cfg.yaml"), "--out", str(out), "--vertices", str(tmp_path / "v.npz"), "--batch-size", "4"])
    assert sorted(os.listdir(out)) == ["%04d.jpg" % i for i in range(T)] and len(paths) == T
    assert Image.open(paths[0]).size == (S, S)
