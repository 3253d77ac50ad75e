"""-m gpu: harp_arm_reproj_ik (csrc/arm_reproj_ik.hip), ops.arm_reproj_ik and Motion.from_arm_image_keypoints against the yardstick of
tests/_arm_reproj_ik_ref.py.

No bound here is a number fixed in advance.  Each is computed in the test from the yardstick itself, by tests/_arm_ik_ref.py's rule:

    bound = 8 x the float32 yardstick's error against the float64 yardstick on the same float32 inputs            (R.FACTOR)

— the same code in float32 (forward, projection, J^T W J, Cholesky of the Jacobi-scaled system) is the error model of a correct float32
solver, and the factor covers what the kernel does differently: its dots summed in another order, the root column as a rotation of the
centre-relative joint, the tangents walked down the tree, the rows converted lane by lane, and the device's sinf / cosf.  Both sides of
every comparison are the worst over all the problems that the test runs, never one problem's.  The kernel's figures and the bounds are
printed side by side (profiles/arm_reproj_ik_errors.txt) before anything is asserted.  The yardstick runs are module-scoped
fixtures; the caps on what may be left out are asserted without a GPU in tests/test_arm_reproj_ik_cpu.py."""
import numpy as np
import pytest
import torch

from tests import _arm_ik_ref as A
from tests import _arm_reproj_ik_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO, NX = R.NO, R.NX
ITERS = 20
E = slice(3 * R.ELBOW, 3 * R.ELBOW + 3)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _f32(t):
    return None if t is None else t.to(torch.float32).to(DEV).contiguous()


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b) if x is not None)


def _x(out):
    N = out.in_pose.shape[0]
    return torch.cat([out.in_pose.reshape(N, 51), out.trans], 1).cpu().double()


def _rel(got, ref):
    """per problem: the largest deviation relative to the problem's largest entry of the quantity"""
    N = ref.shape[0]
    d, m = (got.double() - ref.double()).abs().reshape(N, -1).amax(1), ref.double().abs().reshape(N, -1).amax(1)
    return float((d / m).max())


@pytest.fixture(scope="module")
def arm():
    from harp_amd.hand_models_harp.body_models import TreeDeviceModel
    m_np, m, _ = A.arm_model()
    m2_np, m2 = A.mean_model()
    dev = torch.device(DEV)
    return dict(np=m_np, model=m, dm=TreeDeviceModel(m_np, dev), np2=m2_np, model2=m2, dm2=TreeDeviceModel(m2_np, dev))


def _call(dm, x0, betas, cam, focal, S, targets, weights=None, depth_weights=None, prior=None, wrist_prior=None, z_prior=None, **kw):
    """x0 (N,54) holds the start"""
    from harp_amd import ops
    N = x0.shape[0]
    return ops.arm_reproj_ik(dm, _f32(betas), _f32(targets), _f32(x0[:, :R.XT].reshape(N, 17, 3)), _f32(x0[:, R.XT:]), _f32(cam), focal, S,
                             weights=_f32(weights), depth_weights=_f32(depth_weights), prior=_f32(prior), wrist_prior=_f32(wrist_prior),
                             z_prior=_f32(z_prior), **kw)


def _solve(arm, sc, c, x0=None, **kw):
    """a case of the yardstick (float32 tensors) through the kernel"""
    return _call(arm["dm"], c["x0"] if x0 is None else x0, sc["betas32"], sc["cam32"], sc["focal"], sc["S"], c["targets"], c["weights"],
                 c["depth_weights"], **dict(c["kw"], **kw))


def _yard(sc, c, iters, dtype=torch.float64, x0=None, **over):
    """the yardstick on the same float32 numbers, in float64 (the truth) or float32 (the error model)"""
    up = (lambda t: t) if dtype == torch.float32 else (lambda t: None if t is None else t.double())
    kw = {k: (up(v) if torch.is_tensor(v) else v) for k, v in dict(c["kw"], **over).items()}
    return R.lm(sc["model"], up(c["x0"] if x0 is None else x0), up(sc["betas32"]), up(sc["cam32"]), sc["focal"], sc["S"], up(c["targets"]),
                up(c["weights"]), up(c["depth_weights"]), iters=iters, dtype=dtype, **kw)


def _prior_case(sc, c):
    """depth rows with all three priors' centres away from the start: the pose prior on seeded poses (sigma 0.2), the wrist prior on
    seeded rotations (sigma 0.1), the trans_z prior 20 mm behind the start — every centre enters the step's gradient, not only the cost"""
    g = torch.Generator().manual_seed(5)
    N = c["x0"].shape[0]
    kw = dict(c["kw"], prior=torch.randn(N, 45, generator=g) * 0.2, wrist_prior=torch.randn(N, 3, generator=g) * 0.1, z_prior=c["kw"]["z_prior"] + 0.02)
    return dict(c, kw=kw)


@pytest.fixture(scope="module")
def yard():
    """the committed scene (T = 8, seed 2; 16 problems) as the kernel sees it, and every yardstick run the tests below share: 40 iterations
    in float64 and 20 in float32 of both modes (their histories hold the first step and the run of 20), the first step of the case with
    the priors' centres moved, and the held wrist's 20"""
    sc = R.scene(**R.GPU_SCENE)
    sc["betas32"], sc["cam32"] = sc["betas"].float(), sc["cam"].float()
    out = dict(sc=sc)
    for mode in ("pixels22", "depth22", "depth21held"):
        c = R.as32(sc, R.case(sc, mode))
        out[mode] = dict(case=c, y64=_yard(sc, c, 40 if mode != "depth21held" else ITERS), y32=_yard(sc, c, ITERS, torch.float32))
    c = _prior_case(sc, out["depth22"]["case"])
    out["priors"] = dict(case=c, y64=_yard(sc, c, 1), y32=_yard(sc, c, 1, torch.float32))
    return out


# ---- 1. iters = 0 at the input ----------------------------------------------------------------------------------------------------------
def _driven_mean(pm):
    return np.concatenate([pm[0:3], pm[63:66], pm[120:165]])


def _poses(kind, N, pm, rng):
    x = np.zeros((N, NX), np.float32)
    if kind == "aa_zero":                                 # stored pose = -pose_mean: every driven joint's axis-angle is exactly 0
        x[:, :R.XT] = -_driven_mean(pm)
    elif kind == "tiny":
        x[:, :R.XT] = 1e-6
    elif kind == "random":
        x[:, :R.XT] = rng.normal(size=(N, 51)) * 0.3
    elif kind == "near_pi":
        x[:, R.XW:R.XT] = rng.normal(size=(N, 48)) * 0.3
        u = rng.normal(size=(N, 3))
        x[:, :3] = (np.pi - 1e-3) * u / np.linalg.norm(u, axis=1, keepdims=True)
    return x


# (model, N, betas, cam, weights, depth rows, outside the image)
_CASES = [("model", 1, "zero", "shared", None, False, False), ("model", 2, "shared", "per", "zeros", True, False),
          ("model2", 3, "per", "per", "nan_unused", True, False), ("model2", 2, "shared", "shared", "no_elbow", False, False),
          ("model", 3, "per", "shared", None, True, True), ("model2", 1, "zero", "per", "no_elbow", True, False)]
DEPTH_ROWS = [0, 3, 8, 14, 21]                            # depth rows on five joints (the wrist's own is never used), NaN elsewhere


@pytest.mark.parametrize("kind", ["zero", "aa_zero", "tiny", "random", "near_pi"])
def test_everything_at_the_input(arm, kind):
    """iters = 0 evaluates at the input: proj, jac and cost[:, 0] against float64, each relative to the problem's largest entry of that
    quantity; in_pose and trans come back bit for bit.  N = 1, 2, 3 around the problems per workgroup; betas zero / (10,) / (N,10); cam
    shared / per problem; weights None / all zero (status -1) / a NaN target under a zero weight / the elbow unused; depth rows on five
    joints and NaN elsewhere; every joint outside the image; both synthetic models.  The elbow's rows in the 48 wrist and finger columns
    and d d / d trans are exactly zero."""
    from harp_amd import ops
    F = ops.arm_reproj_ik_frames_per_block()
    rng = np.random.default_rng(11)
    assert {c[1] for c in _CASES} >= {F, F + 1} and {c[0] for c in _CASES} == {"model", "model2"}
    names = ("proj", "jac", "cost")
    worst, worst32 = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0)
    focal, S = R.FOCAL, R.S
    for which, N, bkind, ckind, wkind, with_depth, outside in _CASES:
        model, dm = arm[which], arm["dm" if which == "model" else "dm2"]
        pm = arm["np" if which == "model" else "np2"]["pose_mean"].astype(np.float32)
        x = _poses(kind, N, pm, rng)
        x[:, R.XT:] = rng.uniform(-0.05, 0.05, size=(N, 3))
        x = torch.as_tensor(x)
        betas = {"zero": torch.zeros(10), "shared": torch.as_tensor(rng.normal(size=10) * 0.5, dtype=torch.float32),
                 "per": torch.as_tensor(rng.normal(size=(N, 10)) * 0.5, dtype=torch.float32)}[bkind]
        cam = torch.tensor(R.CAM, dtype=torch.float32)
        if outside:
            cam = cam + torch.tensor([0.0, 0.6, -0.7])      # 2000 x 0.6 px off the centre of a 448 px image
        if ckind == "per":
            cam = cam[None] + torch.as_tensor(rng.normal(size=(N, 3)) * 0.01, dtype=torch.float32)
        targets = torch.as_tensor(np.concatenate([rng.uniform(100, 350, size=(N, NO, 2)), rng.uniform(-0.1, 0.1, size=(N, NO, 1))], -1),
                                  dtype=torch.float32)
        w, n_used = None, NO
        if wkind == "zeros":
            w, n_used = torch.zeros(N, NO), 0
        elif wkind == "nan_unused":
            w = torch.as_tensor(rng.uniform(0.5, 1.5, size=(N, NO)), dtype=torch.float32)
            w[:, [0, 7, 20]] = 0.0
            targets[:, 7, :2] = float("nan")
            n_used = NO - 3
        elif wkind == "no_elbow":
            w = torch.ones(N, NO)
            w[:, R.ELBOW] = 0.0
            n_used = NO - 1
        dw = None
        if with_depth:
            dw = torch.as_tensor(rng.uniform(1e6, 4e6, size=(N, NO)), dtype=torch.float32)
            keep = torch.zeros(NO, dtype=torch.bool)
            keep[DEPTH_ROWS] = True
            targets[:, ~keep, 2] = float("nan")
        kw = dict(prior=torch.as_tensor(rng.normal(size=(N, 45)) * 0.1, dtype=torch.float32),
                  wrist_prior=torch.as_tensor(rng.normal(size=(N, 3)) * 0.1, dtype=torch.float32),
                  z_prior=torch.as_tensor(rng.normal(size=N) * 0.02, dtype=torch.float32), pose_prior_weight=40.0, wrist_prior_weight=400.0,
                  z_prior_weight=100.0)
        out = _call(dm, x, betas, cam, focal, S, targets, w, dw, iters=0, proj=True, jac=True, **kw)
        assert torch.equal(_bits(out.in_pose.reshape(N, 51)), _bits(x[:, :R.XT])) and torch.equal(_bits(out.trans), _bits(x[:, R.XT:]))
        assert out.status.tolist() == [0 if n_used >= 4 else -1] * N
        assert torch.equal(_bits(out.cost[:, 0]), _bits(out.cost[:, 1]))
        assert tuple(out.proj.shape) == (N, NO, 3) and tuple(out.jac.shape) == (N, 3 * NO, NX)
        jac, proj = out.jac.cpu(), out.proj.cpu()
        zero = torch.zeros((), dtype=torch.int32)
        assert bool((_bits(jac[:, E, R.XW:R.XT]) == zero).all())        # the elbow: an ancestor of the centre, exactly +0
        assert bool((_bits(jac[:, 2::3, R.XT:]) == zero).all())         # d d / d trans
        assert bool((_bits(proj[:, 0, 2]) == zero).all())
        if outside:
            assert bool(((proj[..., :2] < 0) | (proj[..., :2] > S)).any(-1).all())
        d = lambda t: None if t is None else t.double()
        kw64 = {k: (d(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
        n64 = R.normal(model, x.double(), betas.double(), cam.double(), focal, S, targets.double(), d(w), d(dw), **kw64)
        n32 = R.normal(model, x, betas, cam, focal, S, targets, w, dw, dtype=torch.float32, **kw)
        got = dict(proj=proj, jac=jac, cost=out.cost[:, :1].cpu())
        ref = dict(proj=n64["p"], jac=n64["J"], cost=n64["C"][:, None])
        f32 = dict(proj=n32["p"], jac=n32["J"], cost=n32["C"][:, None])
        for k in names:
            worst[k], worst32[k] = max(worst[k], _rel(got[k], ref[k])), max(worst32[k], _rel(f32[k], ref[k]))
    print(f"[arm_reproj_ik] input[{kind}] " + " ".join(f"{k} {worst[k]:.3e} (bound {R.FACTOR * worst32[k]:.3e})" for k in names))
    for k in names:
        assert worst[k] <= R.FACTOR * worst32[k], k


# ---- 2. one step from both planar starts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pixels22", "depth22", "priors"])
def test_one_step_from_both_planar_starts(arm, yard, mode):
    sc, c, y, y32 = yard["sc"], yard[mode]["case"], yard[mode]["y64"], yard[mode]["y32"]
    if mode == "priors":
        plain = yard["depth22"]["y64"]["xs"][1]
        moved = (y["xs"][1] - plain).abs().amax(1) / (plain - c["x0"].double()).abs().amax(1)
        print(f"[arm_reproj_ik] one_step[priors] the centres move the yardstick's step by {float(moved.min()):.3e} .. {float(moved.max()):.3e} of it")
        assert float(moved.min()) > 1e-3
    out = _solve(arm, sc, c, iters=1)
    c0, c1, x1 = y["cost"][0], y["cost"][1], y["xs"][1]
    counted = (c0 - c1) / c0 > 1e-3                        # a float32 accept / reject cannot be expected to agree on a tie
    assert int((~counted).sum()) <= 0.1 * counted.numel()
    step = (x1 - c["x0"].double()).abs().amax(1)
    dx = float(((_x(out) - x1).abs().amax(1) / step)[counted].max())
    dx32 = float(((y32["xs"][1].double() - x1).abs().amax(1) / step)[counted].max())
    dc = float(((out.cost[:, 1].cpu().double() - c1).abs() / c1)[counted].max())
    dc32 = float(((y32["cost"][1].double() - c1).abs() / c1)[counted].max())
    print(f"[arm_reproj_ik] one_step[{mode}] x {dx:.3e} (bound {R.FACTOR * dx32:.3e}) cost1 {dc:.3e} (bound {R.FACTOR * dc32:.3e}) "
          f"counted {int(counted.sum())} of {counted.numel()}")
    assert out.status.cpu()[counted].tolist() == [1] * int(counted.sum())
    assert bool((out.cost[:, 1] <= out.cost[:, 0]).all())
    assert dx <= R.FACTOR * dx32
    assert dc <= R.FACTOR * dc32


# ---- 3. twenty iterations against the yardstick's forty ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,cap", [("pixels22", 2), ("depth22", 0)])
def test_full_solve_in_20_iterations(arm, yard, mode, cap):
    """20 iterations on the device against the float64 yardstick's 40, per frame: each side takes, of a frame's two candidates, the one
    with ITS lower final cost, as the layer does.  A frame is left out only if the yardstick ALONE says it has not converged (the last
    accepted step of its candidate still lowered its cost by more than 1e-6 relative): at most 2 of 8 with pixels only, none with depth
    rows (tests/test_arm_reproj_ik_cpu.py).  Then the same at equal iteration counts with every frame counted."""
    sc, c, y, y32 = yard["sc"], yard[mode]["case"], yard[mode]["y64"], yard[mode]["y32"]
    T = R.GPU_SCENE["T"]
    out = _solve(arm, sc, c, iters=ITERS, proj=True)
    best = lambda cost: torch.arange(T) * 2 + cost.reshape(T, 2).argmin(1)
    rows, mine, rows32 = best(y["cost"][-1]), best(out.cost[:, 1].cpu()), best(y32["cost"][-1])
    keep = y["last_drop"][rows] <= 1e-6
    assert int((~keep).sum()) <= cap
    args = (sc["betas32"].double(), sc["cam32"].double(), sc["focal"], sc["S"])

    def pixels(x):
        with torch.no_grad():
            return R.rows(sc["model"], x.double(), *args)[0][..., :2]

    cy, py = y["cost"][-1][rows], pixels(y["x"][rows])
    m = float((out.cost[:, 1].cpu().double()[mine] / cy - 1.0).clamp_min(0.0)[keep].max())
    m32 = float((y32["cost"][-1].double()[rows32] / cy - 1.0).abs()[keep].max())
    got_px = out.proj.cpu().double()[mine][..., :2]
    dpx = float((got_px - py).norm(dim=-1).amax(1)[keep].max())
    dpx32 = float((pixels(y32["x"][rows32]) - py).norm(dim=-1).amax(1)[keep].max())
    err = (got_px - c["targets"].double()[mine][..., :2]).norm(dim=-1).amax(1)
    print(f"[arm_reproj_ik] full_solve[{mode}] cost/yardstick - 1 {m:.3e} (bound {R.FACTOR * m32:.3e}) pixels {dpx:.3e} px (bound "
          f"{R.FACTOR * dpx32:.3e}); {int(keep.sum())} of {T} frames counted; largest pixel error to the targets {float(err.max()):.3f} px; status "
          f"{out.status.min().item()}..{out.status.max().item()}")
    c20 = y["cost"][ITERS]
    rows20 = best(c20)
    p20 = pixels(y["xs"][ITERS][rows20])
    m20 = float((out.cost[:, 1].cpu().double()[mine] / c20[rows20] - 1.0).abs().max())
    m20_32 = float((y32["cost"][-1].double()[rows32] / c20[rows20] - 1.0).abs().max())
    d20 = float((got_px - p20).norm(dim=-1).amax(1).max())
    d20_32 = float((pixels(y32["x"][rows32]) - p20).norm(dim=-1).amax(1).max())
    print(f"[arm_reproj_ik] full_solve[{mode}] against the yardstick's own {ITERS}: cost {m20:.3e} (bound {R.FACTOR * m20_32:.3e}) pixels "
          f"{d20:.3e} px (bound {R.FACTOR * d20_32:.3e})")
    assert int(out.status.min()) >= 1
    assert bool((out.cost[:, 1] <= out.cost[:, 0]).all())
    assert m <= R.FACTOR * m32 and dpx <= R.FACTOR * dpx32
    assert m20 <= R.FACTOR * m20_32 and d20 <= R.FACTOR * d20_32


# ---- 4. 21 wide, the wrist held ---------------------------------------------------------------------------------------------------------
def test_21_wide_with_the_wrist_held(arm, yard):
    sc, c, y, y32 = yard["sc"], yard["depth21held"]["case"], yard["depth21held"]["y64"], yard["depth21held"]["y32"]
    out = _solve(arm, sc, c, iters=ITERS, proj=True, jac=True)
    assert torch.equal(_bits(out.in_pose[:, 1]), _bits(c["x0"][:, R.XW:R.XP]))      # read, never written
    assert not torch.equal(_bits(out.in_pose[:, 0]), _bits(c["x0"][:, :3])) and int(out.status.min()) >= 1
    assert bool((out.cost[:, 1] <= out.cost[:, 0]).all())
    T = R.GPU_SCENE["T"]
    best = lambda cost: cost.reshape(T, 2).amin(1)
    cy = best(y["cost"][-1])
    m = float((best(out.cost[:, 1].cpu().double()) / cy - 1.0).abs().max())
    m32 = float((best(y32["cost"][-1].double()) / cy - 1.0).abs().max())
    print(f"[arm_reproj_ik] held wrist: cost against the yardstick's own {ITERS} {m:.3e} (bound {R.FACTOR * m32:.3e}) status {out.status.tolist()}")
    assert m <= R.FACTOR * m32


# ---- 5. status and guards -----------------------------------------------------------------------------------------------------------------
def _sub(c, rows):
    take = lambda v: v[rows] if torch.is_tensor(v) else v
    return dict(c, x0=c["x0"][rows], targets=c["targets"][rows], weights=take(c["weights"]), depth_weights=take(c["depth_weights"]),
                kw={k: take(v) for k, v in c["kw"].items()})


def test_status_and_guards(arm, yard):
    sc = yard["sc"]
    N, it = 3, 6
    c = _sub(yard["depth22"]["case"], slice(0, N))
    kw = dict(iters=it, proj=True, jac=True)

    def alone_equal(out, cc, f):
        a = _solve(arm, sc, _sub(cc, slice(f, f + 1)), **kw)
        return all(torch.equal(_bits(p[f]), _bits(q[0])) for p, q in zip(out, a) if p is not None)

    # unused entries never enter: whatever stands under a zero weight, and a non-finite target under a weight of one
    w = torch.ones(N, NO)
    w[:, [4, 8, 21]] = 0.0
    dw = c["depth_weights"].clone()
    dw[:, [3, 7]] = 0.0
    outs = []
    for fill in (float("nan"), 1e6, None):
        t = c["targets"].clone()
        if fill is not None:
            t[:, [4, 8, 21], :2] = fill
            t[:, [3, 7], 2] = fill
        outs.append(_solve(arm, sc, dict(c, targets=t, weights=w, depth_weights=dw), **kw))
    t = c["targets"].clone()
    t[:, [4, 8, 21], :2] = float("inf")
    t[:, [3, 7], 2] = float("nan")
    assert _same(outs[0], outs[2]) and _same(outs[1], outs[2]) and _same(_solve(arm, sc, dict(c, targets=t), **kw), outs[2])
    assert int(outs[2].status.min()) >= 1
    for n_used in (0, 3):                                  # status -1: the middle problem is not solved; its neighbours do not notice
        w = torch.ones(N, NO)
        w[1] = 0.0
        w[1, [0, 9, 21][:n_used]] = 1.0
        cc = dict(c, weights=w)
        out = _solve(arm, sc, cc, **kw)
        st = out.status.tolist()
        assert st[1] == -1 and min(st[0], st[2]) >= 1
        assert torch.equal(_bits(_x(out)[1].float()), _bits(c["x0"][1])) and torch.equal(_bits(out.cost[1, 0]), _bits(out.cost[1, 1]))
        assert alone_equal(out, cc, 0) and alone_equal(out, cc, 2)
    w = torch.ones(N, NO)
    w[1, 4:] = 0.0                                         # exactly 4 used pixel joints are enough
    assert _solve(arm, sc, dict(c, weights=w), **kw).status.tolist()[1] >= 0
    # status -3: the middle problem's arm is behind the camera at the input
    xb = c["x0"].clone()
    xb[1, R.XZ] = -float(R.P.tz_of(sc["cam32"].double(), sc["focal"], sc["S"])) - 0.5
    cc = dict(c, x0=xb)
    out = _solve(arm, sc, cc, **kw)
    ref = _yard(sc, cc, it)
    print(f"[arm_reproj_ik] guards status {out.status.tolist()} yardstick {ref['status'].tolist()}")
    assert out.status.tolist()[1] == -3 and ref["status"].tolist()[1] == -3 and min(out.status.tolist()[0], out.status.tolist()[2]) >= 1
    assert torch.equal(_bits(_x(out)[1].float()), _bits(xb[1])) and torch.equal(_bits(out.cost[1, 0]), _bits(out.cost[1, 1]))
    assert alone_equal(out, cc, 0) and alone_equal(out, cc, 2)
    # a joint that is neither used nor in front: zeros in proj and jac (the elbow, pushed behind the camera by a far-away root turn is
    # hard to arrange; the whole arm behind it with every weight zero but four does the same for the unused joints)
    w = torch.zeros(N, NO)
    w[:, :4] = 1.0
    w[1] = 0.0
    at0 = _solve(arm, sc, dict(cc, weights=w), **dict(kw, iters=0))
    assert at0.status.tolist() == [0, -1, 0]
    assert float(at0.proj[1, :, :2].abs().max()) == 0.0 and float(at0.jac.reshape(N, NO, 3, NX)[1, :, :2].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t.float()).all()) for t in at0)


def test_rejected_steps_never_raise_the_cost(arm, yard):
    """from zero (no planar start) the first steps overshoot and some are rejected: status counts the strict decreases of the kernel's own
    cost history (the run with k iterations is the prefix of the run with k + 1), the cost never rises, and after a rejected LAST step
    proj, jac and cost are those of the x that was kept"""
    sc, c = yard["sc"], yard["pixels22"]["case"]
    iters = 8
    x0 = torch.zeros_like(c["x0"])
    over = dict(z_prior=torch.zeros(x0.shape[0]))
    hist = [_solve(arm, sc, c, x0=x0, iters=0, **over).cost[:, 0].cpu()]
    for k in range(1, iters + 1):
        out = _solve(arm, sc, c, x0=x0, iters=k, **over)
        assert torch.equal(_bits(out.cost[:, 0]), _bits(hist[0]))
        hist.append(out.cost[:, 1].cpu())
    hist = torch.stack(hist)
    falls = (hist[1:] < hist[:-1]).sum(0)
    print(f"[arm_reproj_ik] rejected: status {out.status.tolist()} strict decreases {falls.tolist()}")
    assert bool((hist[1:] <= hist[:-1]).all()) and out.status.cpu().tolist() == falls.tolist()
    assert int(falls.min()) < iters and bool(torch.isfinite(_x(out)).all())
    rejected = hist[1:] == hist[:-1]
    k = int(torch.nonzero(rejected.any(1))[0]) + 1
    fr = torch.nonzero(rejected[k - 1]).reshape(-1)
    out = _solve(arm, sc, c, x0=x0, iters=k, proj=True, jac=True, **over)
    xk = _x(out)[fr]
    cf = _sub(dict(c, kw=dict(c["kw"], **over)), fr)
    d = lambda t: None if t is None else t.double()
    args = (sc["cam32"], sc["focal"], sc["S"])
    kw = {k_: v for k_, v in cf["kw"].items()}
    kw64 = {k_: (d(v) if torch.is_tensor(v) else v) for k_, v in kw.items()}
    n64 = R.normal(sc["model"], xk, sc["betas32"].double(), args[0].double(), *args[1:], cf["targets"].double(), d(cf["weights"]), None, **kw64)
    n32 = R.normal(sc["model"], xk.float(), sc["betas32"], *args, cf["targets"], cf["weights"], None, dtype=torch.float32, **kw)
    got = dict(proj=out.proj.cpu()[fr], jac=out.jac.cpu()[fr], cost=out.cost[:, 1:].cpu()[fr])
    ref = dict(proj=n64["p"], jac=n64["J"], cost=n64["C"][:, None])
    f32 = dict(proj=n32["p"], jac=n32["J"], cost=n32["C"][:, None])
    print(f"[arm_reproj_ik] kept x after a rejected step {k} problems {fr.tolist()} " +
          " ".join(f"{q} {_rel(got[q], ref[q]):.3e} (bound {R.FACTOR * _rel(f32[q], ref[q]):.3e})" for q in got))
    for q in got:
        assert _rel(got[q], ref[q]) <= R.FACTOR * _rel(f32[q], ref[q]), q


# ---- 6. repeat, capture, front ------------------------------------------------------------------------------------------------------------
def test_repeatable_and_capturable(arm, yard):
    from harp_amd import ops
    sc, c = yard["sc"], yard["priors"]["case"]
    N = c["x0"].shape[0]
    kw = dict(iters=6, proj=True, jac=True)
    a = _solve(arm, sc, c, **kw)
    b = _solve(arm, sc, c, **kw)
    assert _same(a, b) and int(a.status.min()) >= 1 and isinstance(a, ops.ArmReprojIkResult)
    # one captured call through out=, replayed on the problems in another order
    x0, k = c["x0"], c["kw"]
    dev = lambda t: _f32(t).clone()
    targets, in_pose, trans = dev(c["targets"]), dev(x0[:, :R.XT].reshape(N, 17, 3)), dev(x0[:, R.XT:])
    w, dw, prior, wprior, zp = dev(c["weights"]), dev(c["depth_weights"]), dev(k["prior"]), dev(k["wrist_prior"]), dev(k["z_prior"])
    betas, cam = _f32(sc["betas32"]), _f32(sc["cam32"])
    sk = dict(kw, solve_wrist=k["solve_wrist"], pose_prior_weight=k["pose_prior_weight"], wrist_prior_weight=k["wrist_prior_weight"],
              z_prior_weight=k["z_prior_weight"])
    run = lambda **o: ops.arm_reproj_ik(arm["dm"], betas, targets, in_pose, trans, cam, sc["focal"], sc["S"], weights=w, depth_weights=dw,
                                        prior=prior, wrist_prior=wprior, z_prior=zp, **sk, **o)
    out = run()                                           # warm-up outside the capture; its tensors are reused
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(out=out)
    for order in (torch.arange(N), torch.arange(N - 1, -1, -1)):
        for dst, src in ((targets, c["targets"]), (in_pose, x0[:, :R.XT].reshape(N, 17, 3)), (trans, x0[:, R.XT:]), (w, c["weights"]),
                         (dw, c["depth_weights"]), (prior, k["prior"]), (wprior, k["wrist_prior"]), (zp, k["z_prior"])):
            dst.copy_(_f32(src[order]))
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(p[order]), _bits(q)) for p, q in zip(a, out)), order[:4]
    # out= written in place gives the first call's bits
    again = _solve(arm, sc, c, out=b, **kw)
    assert again is b and _same(a, b)
    with pytest.raises(ValueError, match="out"):
        _solve(arm, sc, c, out=b, **dict(kw, jac=False))


def test_refusals_with_real_buffers(arm):
    """the front's shared refusals (tests/test_gpu_solver_front.py holds this case for the five older solvers) and the wrapper's own"""
    from harp_amd import ops
    dm, dev = arm["dm"], torch.device(DEV)
    N = 2
    z = lambda *s: torch.zeros(*s, device=dev)
    tg, ip, b, tr = z(N, NO, 3), z(N, 17, 3), z(10), z(N, 3)
    tg[..., :2] = 224.0
    cam = torch.tensor(R.CAM, device=dev)
    f = lambda *a, **k: ops.arm_reproj_ik(dm, *a, **k)
    assert f(b, tg, ip, tr, cam, R.FOCAL, R.S, iters=0).status.tolist() == [0, 0]
    with pytest.raises(ValueError, match="targets"):
        f(b, tg[:, :21].contiguous(), ip, tr, cam, R.FOCAL, R.S)
    with pytest.raises(ValueError, match="in_pose"):
        f(b, tg, ip.reshape(N, 51), tr, cam, R.FOCAL, R.S)
    with pytest.raises(ValueError, match="betas"):
        f(z(3, 10), tg, ip, tr, cam, R.FOCAL, R.S)
    with pytest.raises(ValueError, match="cam"):
        f(b, tg, ip, tr, z(3, 3), R.FOCAL, R.S)
    with pytest.raises(ValueError, match="wrist_prior"):
        f(b, tg, ip, tr, cam, R.FOCAL, R.S, wrist_prior=z(3))
    with pytest.raises(ValueError, match="depth_weights"):
        f(b, tg, ip, tr, cam, R.FOCAL, R.S, depth_weights=z(N, 21))
    with pytest.raises(ValueError, match="z_prior"):
        f(b, tg, ip, tr, cam, R.FOCAL, R.S, z_prior=z(N, 1))
    with pytest.raises(ValueError, match="z_prior_weight needs z_prior"):
        f(b, tg, ip, tr, cam, R.FOCAL, R.S, z_prior_weight=1.0)
    for bad in (dict(wrist_prior_weight=-1.0), dict(z_prior_weight=float("inf"), z_prior=z(N)), dict(iters=-1), dict(lambda0=float("nan"))):
        with pytest.raises(ValueError):
            f(b, tg, ip, tr, cam, R.FOCAL, R.S, **bad)
    for focal, S in ((0.0, R.S), (float("inf"), R.S), (R.FOCAL, 0), (R.FOCAL, 448.5)):
        with pytest.raises(ValueError, match="focal"):
            f(b, tg, ip, tr, cam, focal, S)
    with pytest.raises(TypeError, match="targets"):
        f(b, tg.double(), ip, tr, cam, R.FOCAL, R.S)
    with pytest.raises(RuntimeError):
        f(b, tg, ip.clone().requires_grad_(), tr, cam, R.FOCAL, R.S)
    with pytest.raises(RuntimeError):
        f(b, tg.cpu(), ip, tr, cam, R.FOCAL, R.S)
    with pytest.raises(ValueError, match="out.proj"):
        f(b, tg, ip, tr, cam, R.FOCAL, R.S, proj=True, out=f(b, tg, ip, tr, cam, R.FOCAL, R.S, iters=0))
    # a non-contiguous input is read through a contiguous copy, the caller's start stays untouched
    wide = z(N, NO, 4)
    wide[..., :2] = 224.0
    a, c = f(b, tg, ip, tr, cam, R.FOCAL, R.S, iters=2), f(b, wide[..., :3], ip, tr, cam, R.FOCAL, R.S, iters=2)
    assert _same(a, c) and not bool(ip.any()) and not bool(tr.any())


# ---- 7. the layer ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """the smallest arm fit fixture tests/test_gpu_arm_ik.py's player test uses (5 frames, 32 px), its true motion and that motion's image
    keypoints (pixels, wrist-relative depth), and the float64 model of its layer"""
    from harp_amd import playback, synth
    from tests.test_gpu_avatar_player import _arm_setup
    n, S = 5, 32
    cfg, layer, params = _arm_setup(n, S, 3, tmp_path_factory.mktemp("arm_reproj"))
    true = playback.Motion.from_params(params)
    betas = params["shape"].detach().reshape(1, 10).expand(n, 10).contiguous()

    def forward(m):
        with torch.no_grad():
            return layer(betas=betas, global_orient=m.rot.to(DEV), transl=m.trans.to(DEV), right_hand_pose=m.pose.to(DEV),
                         right_wrist_pose=m.wrist_pose.to(DEV))[1]

    rows = playback.project_pixels(forward(true).cpu().double().numpy() / 1000.0, true.cam.cpu().double().numpy(), float(cfg["focal_length"]), S)
    m_np = synth.make_smplx_arm_model(synth.load_template("arm"), seed=3)
    model = {k: torch.from_numpy(v).double() if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in m_np.items()}
    return dict(n=n, S=S, cfg=cfg, layer=layer, params=params, true=true, forward=forward, kp=rows[..., :2].astype(np.float32),
                depth=rows[..., 2].astype(np.float32), model=model)


def _layer_yardstick(clip, depth, cam, dtype=torch.float64):
    """the yardstick on exactly what the layer passes to ops.arm_reproj_ik"""
    from harp_amd import ops
    from harp_amd.playback import keypoints as K
    from harp_amd.playback.motion import _arm_device_model
    cfg, params, layer, n = clip["cfg"], clip["params"], clip["layer"], clip["n"]
    focal, S = float(cfg["focal_length"]), clip["S"]
    a = K.arm_image_ik_inputs(clip["kp"], None, depth, cam, None, None, params)
    f32 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32))
    zero = ops.arm_ik(_arm_device_model(layer, torch.device(DEV)), _f32(f32(a["shape"])), torch.zeros(n, 22, 3, device=DEV), _f32(f32(a["in_pose"])),
                      _f32(f32(a["trans"])), iters=0, joints=True).joints
    in_pose, trans, zbar = K.arm_image_starts(a, zero.cpu().numpy().astype(np.float64) / 1000.0, None, focal, S)
    scale = (focal / zbar) ** 2
    med = float(np.median(scale))
    x0 = torch.cat([f32(in_pose.reshape(2 * n, 51)), f32(trans.reshape(2 * n, 3))], 1)
    rep = lambda v: f32(np.repeat(v, 2, axis=0))
    fl = lambda v: float(np.float32(v))
    up = (lambda t: t) if dtype == torch.float32 else (lambda t: None if t is None else t.double())
    dw = None if depth is None else rep(np.broadcast_to(scale[:, None], (n, 22)))
    return R.lm(clip["model"], up(x0), up(f32(a["shape"])), up(rep(a["cam"])), focal, S, up(rep(a["targets"])), up(rep(a["weights"])), up(dw),
                wrist_prior=up(rep(a["wrist"])), z_prior=up(x0[:, R.XZ].clone()), pose_prior_weight=fl(1e-5 * med),
                wrist_prior_weight=fl(1e-4 * med), z_prior_weight=fl(2.5e-5 * med), iters=ITERS, dtype=dtype)


def _motion_x(m):
    return torch.cat([m.rot, m.wrist_pose, m.pose, m.trans], 1).cpu().double()


def test_layer_picks_the_yardsticks_candidate(clip):
    from harp_amd import playback
    from harp_amd.playback import Motion
    n = clip["n"]
    rec = Motion.from_arm_image_keypoints(clip["kp"], clip["params"], clip["layer"], configs=clip["cfg"])
    assert len(rec) == n and rec.light_positions is None and rec.wrist_pose is not None
    assert torch.equal(rec.cam.cpu(), clip["params"]["cam"][0].detach().cpu().expand(n, 3))
    y = _layer_yardstick(clip, None, None)
    pick = y["cost"][-1].reshape(n, 2).argmin(1)
    xs = y["x"].reshape(n, 2, NX)
    apart = (xs[:, 0] - xs[:, 1]).abs().amax(1) > 1e-3     # where both candidates reached one minimum, either is the yardstick's
    got = _motion_x(rec)
    d_pick = (got - xs[torch.arange(n), pick]).abs().amax(1)
    d_other = (got - xs[torch.arange(n), 1 - pick]).abs().amax(1)
    print(f"[arm_reproj_ik] layer pick {pick.tolist()} apart {apart.tolist()} distance to the picked {d_pick.tolist()} to the other {d_other.tolist()}")
    assert bool((d_pick <= d_other)[apart].all())
    j = clip["forward"](rec).cpu().double().numpy() / 1000.0
    px = playback.project_pixels(j, rec.cam.cpu().double().numpy(), float(clip["cfg"]["focal_length"]), clip["S"])[..., :2]
    print(f"[arm_reproj_ik] layer pixels only: largest reprojection error {float(np.linalg.norm(px - clip['kp'], axis=-1).max()):.4f} px")
    with pytest.raises(NotImplementedError, match="from_arm_image_keypoints"):
        Motion.from_image_keypoints(clip["kp"][:, :21], clip["params"], clip["layer"], configs=clip["cfg"])


def test_layer_with_depth_drives_the_player(clip):
    """with depth rows (and the frames' own cam) the joints come back as far from the truth as the float64 yardstick's own result is (the
    priors' bias), to within the rule's bound: 8 x what the float32 yardstick's distance differs from it; the covered pixels of the
    player's render of the recovered motion are printed beside the true motion's"""
    from harp_amd.playback import AvatarPlayer, Motion
    n, true = clip["n"], clip["true"]
    cam = true.cam.cpu().numpy()                           # the keypoints were projected with every frame's own cam
    rec = Motion.from_arm_image_keypoints(clip["kp"], clip["params"], clip["layer"], cam=cam, depth=clip["depth"], configs=clip["cfg"])
    assert torch.equal(rec.cam.cpu(), true.cam.cpu())
    truth = clip["forward"](true).cpu().double()
    dist = (clip["forward"](rec).cpu().double() - truth).norm(dim=-1).amax(1)
    shape = clip["params"]["shape"].detach().cpu().float().reshape(10)

    def yard_dist(dtype):
        y = _layer_yardstick(clip, clip["depth"], cam, dtype)
        pick = y["cost"][-1].reshape(n, 2).argmin(1)
        xy = y["x"].reshape(n, 2, NX)[torch.arange(n), pick]
        with torch.no_grad():
            jy = A.joints(clip["model"], xy, shape.to(dtype), dtype).double() * 1000.0
        return (jy - truth).norm(dim=-1).amax(1)

    dy, dy32 = yard_dist(torch.float64), yard_dist(torch.float32)
    off, bound = float((dist - dy).abs().max()), R.FACTOR * float((dy32 - dy).abs().max())
    print(f"[arm_reproj_ik] layer with depth: largest joint distance per frame {dist.tolist()} mm (yardstick {dy.tolist()} mm): off by "
          f"{off:.3e} mm (bound {bound:.3e})")
    assert off <= bound
    # 21 wide: the wrist held at the truth comes back bit for bit
    held = Motion.from_arm_image_keypoints(clip["kp"][:, :21], clip["params"], clip["layer"], cam=cam, depth=clip["depth"][:, :21],
                                           wrist_pose=true.wrist_pose, configs=clip["cfg"])
    assert torch.equal(_bits(held.wrist_pose), _bits(true.wrist_pose)) and bool(torch.isfinite(held.pose).all())
    # a frame without its elbow is still solved; init= is the only candidate; smoothing takes both widths
    w = np.ones((n, 22), np.float32)
    w[2, 21] = 0.0
    gone = clip["kp"].copy()
    gone[3, 21] = np.nan
    rec2 = Motion.from_arm_image_keypoints(gone, clip["params"], clip["layer"], cam=cam, weights=w, depth=clip["depth"], configs=clip["cfg"])
    assert bool(torch.isfinite(_motion_x(rec2)).all())
    warm = Motion.from_arm_image_keypoints(clip["kp"], clip["params"], clip["layer"], cam=cam, depth=clip["depth"], configs=clip["cfg"], init=rec,
                                           iters=2)
    assert len(warm) == n and float((clip["forward"](warm).cpu().double() - truth).norm(dim=-1).max()) <= 2.0 * float(dist.max()) + 1.0
    for kp in (clip["kp"], clip["kp"][:, :21]):
        sm = Motion.from_arm_image_keypoints(kp, clip["params"], clip["layer"], cam=cam, smooth=1.0, configs=clip["cfg"])
        assert len(sm) == n and bool(torch.isfinite(sm.pose).all())
    player = AvatarPlayer(clip["cfg"], clip["params"], clip["layer"], batch_size=n, ss=1, device=DEV)
    white = lambda fr: int((fr.cpu() != 255).any(-1).sum())
    player.load_motion(true)
    n_true = white(player.render(np.arange(n)))
    player.load_motion(Motion(rec.pose, rec.rot, rec.trans, true.cam, wrist_pose=rec.wrist_pose))
    n_rec = white(player.render(np.arange(n)))
    print(f"[arm_reproj_ik] layer covered pixels true {n_true} recovered {n_rec}")
    assert n_true > 0 and n_rec > 0


@pytest.mark.parametrize("width", [22, 21])
def test_command_line_reads_a_labelled_arm_playback(clip, tmp_path, monkeypatch, width):
    """the open loop closed: a labelled arm playback's keypoints.npz goes back in through --keypoints2d (main() with the two loaders of
    licensed / fitted files replaced by the synthetic scene, as tests/test_gpu_arm_ik.py does), 22 wide as written and cut to the hand's 21
    with the wrist held, and plays"""
    import os
    import yaml
    from PIL import Image
    from harp_amd import playback
    from harp_amd.utils import file_utils, hand_model_utils
    n, S, cfg, layer, params = clip["n"], clip["S"], clip["cfg"], clip["layer"], clip["params"]
    assert cfg["use_arm"]
    monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda c: (layer, params["verts_uvs"], params["faces_uvs"], None))
    monkeypatch.setattr(file_utils, "load_result", lambda base, device="cuda", test=False: dict(params))
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump({k: cfg[k] for k in ("use_arm", "img_size", "focal_length", "self_shadow", "share_light_position", "base_output_dir")}, f)
    clip["true"].save(tmp_path / "true.npz")
    common = ["--config", str(tmp_path / "cfg.yaml"), "--batch-size", "4"]
    playback.main(common + ["--motion", str(tmp_path / "true.npz"), "--out", str(tmp_path / "labelled"), "--labels"])
    with np.load(tmp_path / "labelled" / "keypoints.npz") as z:
        kp = {k: z[k] for k in ("keypoints", "weights", "depth")}
    assert kp["keypoints"].shape == (n, 22, 2) and kp["depth"].shape == (n, 22)
    print(f"[arm_reproj_ik] labelled playback: {int(kp['weights'].sum())} of {kp['weights'].size} joints visible; pixels off the projected "
          f"truth by {float(np.abs(kp['keypoints'] - clip['kp']).max()):.3e} px")
    extra = dict(cam=clip["true"].cam.cpu().numpy())
    if width == 21:
        kp = {k: v[:, :21] for k, v in kp.items()}
        extra["wrist_pose"] = clip["true"].wrist_pose.cpu().numpy()
    np.savez(tmp_path / "kp.npz", **kp, **extra)
    out = tmp_path / "frames"
    paths = playback.main(common + ["--keypoints2d", str(tmp_path / "kp.npz"), "--out", str(out)])
    assert sorted(os.listdir(out)) == ["%04d.jpg" % i for i in range(n)] and len(paths) == n
    assert Image.open(paths[0]).size == (S, S)
