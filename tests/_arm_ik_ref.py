"""TEST INFRASTRUCTURE ONLY — the yardstick of the batched SMPL-X arm inverse kinematics (csrc/arm_ik.hip, include/harp_hip.h harp_arm_ik):
the 22 output joints through oracle.harp_ref.smplxarm_forward, the Jacobian by forward mode (torch.func.jvp under vmap: one tangent per
column, every frame at once), and the Levenberg-Marquardt iteration of the contract written out plainly with a dense solve of the
Jacobi-scaled system — tests/_arm_fit_ref.py with the shape given, joints for vertices, a centre for the wrist prior and 54 columns.
Everything is parameterised by dtype: float64 is the truth, and THE SAME CODE in float32 is the error model from which the GPU tests compute
their bounds.  Also the seeded scenes the CPU and GPU tests share and the start as the playback layer computes it.
x = [rot 3 | wrist 3 | pose 45 | trans 3] per frame; betas (10,) or (T,10) beside it."""
import numpy as np
import torch

from oracle import harp_ref
from tests._arm_fit_ref import arm_model, model_as

NX = 54
XW, XP, XT = 3, 6, 51
NO = 22
ELBOW = 21
FACTOR = 8.0           # bound = FACTOR x the float32 yardstick's error against the float64 one on the same inputs (the issue's rule)
MIN_USED = 3
PRIORS = dict(pose_prior_weight=1e-5, wrist_prior_weight=1e-4)       # Motion.from_arm_keypoints' defaults


def mean_model():
    """(model_np, model float64 tensors) of the synthetic arm with a non-zero pose mean on the undriven joints 17 and 19 (ancestors of
    the wrist: they turn the elbow about the wrist) and 25..39 (the left hand: constant corrective rows)"""
    m_np, m, _ = arm_model()
    m_np = dict(m_np)
    pm = m_np["pose_mean"].copy()
    rng = np.random.default_rng(8)
    pm[75:120] = (rng.normal(size=45) * 0.05).astype(np.float32)
    pm[51:54] = (rng.normal(size=3) * 0.2).astype(np.float32)
    pm[57:60] = (rng.normal(size=3) * 0.2).astype(np.float32)
    m_np["pose_mean"] = pm
    return m_np, dict(m, pose_mean=torch.from_numpy(pm).double())


def _betas(betas, T, dtype):
    b = torch.as_tensor(betas).to(dtype)
    return b[None].expand(T, 10) if b.dim() == 1 else b


def joints(model, x, betas, dtype=torch.float64):
    """x (T,54), betas (10,) or (T,10) -> the 22 output joints (T,22,3) in metres, computed in `dtype` (trans is added here, outside the
    forward, as _arm_fit_ref.verts does)"""
    x = x.to(dtype)
    T = x.shape[0]
    _, j = harp_ref.smplxarm_forward(model_as(model, dtype), _betas(betas, T, dtype), x[:, :3], torch.zeros(T, 3, dtype=dtype), x[:, XP:XT],
                                     x[:, XW:XP])
    return j / 1000.0 + x[:, None, XT:]


def jacobian(model, x, betas, dtype=torch.float64):
    """(T,66,54) in `dtype`, forward mode: column c of every frame from ONE tangent that is e_c in every frame"""
    x = x.to(dtype)
    T = x.shape[0]
    m = model_as(model, dtype)
    f = lambda y: joints(m, y, betas, dtype)
    basis = torch.eye(NX, dtype=dtype)[:, None, :].expand(NX, T, NX)
    cols = torch.func.vmap(lambda tan: torch.func.jvp(f, (x,), (tan,))[1])(basis)                        # (54,T,22,3)
    return cols.reshape(NX, T, -1).permute(1, 2, 0).contiguous()


def used_mask(targets, weights, dtype=torch.float64):
    """(T,22) bool and the weights / targets in `dtype` with every unused entry zeroed"""
    w = torch.ones(targets.shape[:2], dtype=dtype) if weights is None else weights.to(dtype)
    used = (w > 0) & torch.isfinite(targets).all(-1)
    return used, torch.where(used, w, torch.zeros_like(w)), torch.where(used[..., None], targets.to(dtype), torch.zeros(targets.shape, dtype=dtype))


def _priors(x, prior, wrist_prior, pose_w, wrist_w, dtype):
    """P (54,) the prior diagonal and dx (T,54) = x - x_prior on the columns that have a prior"""
    P = torch.zeros(NX, dtype=dtype)
    P[XP:XT], P[XW:XP] = pose_w, wrist_w
    dx = torch.zeros_like(x)
    dx[:, XP:XT] = x[:, XP:XT] - (0.0 if prior is None else prior.to(dtype))
    dx[:, XW:XP] = x[:, XW:XP] - (0.0 if wrist_prior is None else wrist_prior.to(dtype))
    return P, dx


def cost(model, x, betas, targets, weights=None, prior=None, wrist_prior=None, pose_prior_weight=0.0, wrist_prior_weight=0.0,
         dtype=torch.float64):
    """C (T,) and the residuals (T,22,3), zero where unused"""
    x = x.to(dtype)
    used, w, tg = used_mask(targets, weights, dtype)
    r = (joints(model, x, betas, dtype) - tg) * used[..., None]
    P, dx = _priors(x, prior, wrist_prior, pose_prior_weight, wrist_prior_weight, dtype)
    return (w[..., None] * r * r).sum((1, 2)) + (P * dx * dx).sum(1), r


def normal(model, x, betas, targets, weights=None, prior=None, wrist_prior=None, pose_prior_weight=0.0, wrist_prior_weight=0.0,
           solve_wrist=True, dtype=torch.float64):
    """dict(J (T,66,54), A (T,54,54), g (T,54), C (T,), r) at x: the contract's normal equations, frozen columns included"""
    x = x.to(dtype)
    T = x.shape[0]
    used, w, tg = used_mask(targets, weights, dtype)
    kw = dict(weights=weights, prior=prior, wrist_prior=wrist_prior, pose_prior_weight=pose_prior_weight,
              wrist_prior_weight=wrist_prior_weight, dtype=dtype)
    C, r = cost(model, x, betas, targets, **kw)
    J = jacobian(model, x, betas, dtype)
    W = w[:, :, None].expand(*w.shape, 3).reshape(T, -1)
    P, dx = _priors(x, prior, wrist_prior, pose_prior_weight, wrist_prior_weight, dtype)
    A = torch.einsum("tki,tk,tkj->tij", J, W, J) + torch.diag(P)
    g = torch.einsum("tki,tk->ti", J, W * r.reshape(T, -1)) + P * dx
    if not solve_wrist:
        fz = list(range(XW, XP))
        A[:, fz, :] = 0.0
        A[:, :, fz] = 0.0
        A[:, fz, fz] = 1.0
        g[:, fz] = 0.0
    return dict(J=J, A=A, g=g, C=C, r=r)


def lm(model, x0, betas, targets, weights=None, prior=None, wrist_prior=None, pose_prior_weight=0.0, wrist_prior_weight=0.0, solve_wrist=True,
       iters=15, lambda0=1e-3, dtype=torch.float64):
    """The iteration of include/harp_hip.h in `dtype`.  Returns dict(x (T,54), cost (iters + 1, T) = C after k iterations, accepted (T,)
    (-1: fewer than 3 used joints, not solved), trial (iters, T) = C(x') of every iteration's candidate, ok (iters, T) accepted flags,
    cond (iters, T) the condition number of every iteration's scaled matrix)."""
    x = x0.to(dtype).clone()
    T = x.shape[0]
    used, _, _ = used_mask(targets, weights, dtype)
    solve = used.sum(1) >= MIN_USED
    lam = torch.full((T,), float(lambda0), dtype=dtype)
    kw = dict(weights=weights, prior=prior, wrist_prior=wrist_prior, pose_prior_weight=pose_prior_weight,
              wrist_prior_weight=wrist_prior_weight, dtype=dtype)
    C, _ = cost(model, x, betas, targets, **kw)
    hist, trial, oks, conds = [C.clone()], [], [], []
    acc = torch.zeros(T, dtype=torch.int64)
    eye = torch.eye(NX, dtype=dtype).expand(T, NX, NX)
    for _ in range(iters):
        n = normal(model, x, betas, targets, solve_wrist=solve_wrist, **kw)
        D = torch.diagonal(n["A"], dim1=1, dim2=2)
        s = 1.0 / torch.sqrt(D * (1.0 + lam[:, None]))
        good = (D > 0).all(1) & torch.isfinite(s).all(1)
        s = torch.where(good[:, None], s, torch.ones_like(s))
        S = s[:, :, None] * (n["A"] + torch.diag_embed(lam[:, None] * D)) * s[:, None, :]
        good = good & torch.isfinite(S).all((1, 2))
        S = torch.where(good[:, None, None], S, eye)
        conds.append(torch.linalg.cond(S.double()))
        L, info = torch.linalg.cholesky_ex(S)
        good = good & (info == 0) & torch.isfinite(L).all((1, 2))
        L = torch.where(good[:, None, None], L, eye)
        z = torch.cholesky_solve((-n["g"] * s)[:, :, None], L)[:, :, 0]
        xn = x + s * z
        Cn, _ = cost(model, xn, betas, targets, **kw)
        ok = solve & good & (Cn < C)
        x = torch.where(ok[:, None], xn, x)
        C = torch.where(ok, Cn, C)
        lam = torch.where(ok, (0.1 * lam).clamp_min(1e-9), (10.0 * lam).clamp_max(1e6))
        acc += ok.long()
        hist.append(C.clone()); trial.append(Cn); oks.append(ok)
    return dict(x=x, cost=torch.stack(hist), accepted=torch.where(solve, acc, torch.full_like(acc, -1)),
                trial=torch.stack(trial) if trial else torch.zeros(0, T, dtype=dtype),
                ok=torch.stack(oks) if oks else torch.zeros(0, T, dtype=torch.bool),
                cond=torch.stack(conds) if conds else torch.zeros(0, T, dtype=torch.float64))


def joint_dist_mm(model, x, betas, targets, weights=None, dtype=torch.float64):
    """(mean, largest) distance of the used joints to their targets per frame, millimetres (float64 arithmetic on the joints computed in
    `dtype`)"""
    used, _, tg = used_mask(targets.double(), weights)
    with torch.no_grad():
        d = (joints(model, x, betas, dtype).double() - tg).norm(dim=-1) * used * 1000.0
    return d.sum(1) / used.sum(1).clamp_min(1), d.amax(1)


def scene(T=24, seed=0, noise=0.0, per_frame_betas=False, model=None, root_lo=0.2, root_hi=3.1):
    """Seeded poses on make_smplx_arm_model() (or `model`): a root rotation about a random axis by root_lo .. root_hi rad, wrist and pose
    sigma 0.3, betas sigma 0.5 (one for all frames, or per frame), trans within +-0.3 m, and the 22 joints they give plus Gaussian noise
    of `noise` metres per coordinate.  Returns dict(model (float64), x_true (T,54), betas (10,) or (T,10), targets (T,22,3) float64)."""
    m = arm_model()[1] if model is None else model
    rng = np.random.default_rng(9300 + seed)
    axis = rng.normal(size=(T, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    x = np.zeros((T, NX))
    x[:, :3] = axis * rng.uniform(root_lo, root_hi, (T, 1))
    x[:, XW:XT] = rng.normal(size=(T, 48)) * 0.3
    x[:, XT:] = rng.uniform(-0.3, 0.3, (T, 3))
    betas = torch.as_tensor(rng.normal(size=(T, 10) if per_frame_betas else 10) * 0.5)
    x_true = torch.as_tensor(x)
    with torch.no_grad():
        targets = joints(m, x_true, betas)
    if noise:
        targets = targets + torch.as_tensor(rng.normal(size=tuple(targets.shape)) * noise)
    return dict(model=m, x_true=x_true, betas=betas, targets=targets)


def layer_start(model, betas, targets, weights=None, wrist=None, width=22):
    """the start as Motion.from_arm_keypoints computes it, x0 (T,54) float64: the wrist at `wrist` (T,3) (default zeros: the prior's
    centre, or what it is held at), pose zero, root and trans from harp_amd.playback.arm_palm_start on the first `width` keypoints with
    the model's joints at that shape and wrist"""
    from harp_amd import playback
    tg = targets.double()
    T = tg.shape[0]
    x0 = torch.zeros(T, NX, dtype=torch.float64)
    if wrist is not None:
        x0[:, XW:XP] = torch.as_tensor(wrist).double()
    with torch.no_grad():
        j0 = joints(model, x0, betas)
    used, _, _ = used_mask(tg, weights)
    rot, trans = playback.arm_palm_start(tg[:, :width].numpy(), used[:, :width].numpy(), j0.numpy())
    x0[:, :3], x0[:, XT:] = torch.as_tensor(rot), torch.as_tensor(trans)
    return x0


# The three ways Motion.from_arm_keypoints calls the solver: name -> (weights of the 22 joints, wrist solved, keypoints the start sees)
def case(name, sc):
    """(weights (T,22) or None, solve kwargs, x0 (T,54) float64) of a scene for "22" (the wrist solved), "21" (the elbow unused, the wrist
    held at the truth), "22_no_elbow" (22 wide, the elbow weighted 0, the wrist solved: the prior decides it) or "22_priors" (the wrist
    solved; both priors at weight 1e-2 with non-zero centres, so that their share of g and of the diagonal is far above every bound)"""
    T = sc["targets"].shape[0]
    w = None
    if name == "22_priors":
        rng = np.random.default_rng(77)
        prior, wrist = torch.as_tensor(rng.normal(size=(T, 45)) * 0.1), torch.as_tensor(rng.normal(size=(T, 3)) * 0.1)
        x0 = layer_start(sc["model"], sc["betas"], sc.get("targets32", sc["targets"]), None, wrist)
        return None, dict(pose_prior_weight=1e-2, wrist_prior_weight=1e-2, solve_wrist=True, weights=None, prior=prior, wrist_prior=wrist), x0
    if name != "22":
        w = torch.ones(T, NO, dtype=torch.float64)
        w[:, ELBOW] = 0.0
    held = name == "21"
    wrist = sc["x_true"][:, XW:XP] if held else None
    x0 = layer_start(sc["model"], sc["betas"], sc.get("targets32", sc["targets"]), w, wrist, width=21 if held else 22)
    kw = dict(PRIORS, solve_wrist=not held, weights=w, wrist_prior=wrist)
    return w, kw, x0


def scene32(name, **skw):
    """a seeded scene and one of the three cases as the kernel sees them: float32 targets and a float32 start from those targets; the
    yardstick runs from exactly those numbers.  Adds targets32, x0_32, betas32, kw (weights and wrist_prior float32)."""
    s = scene(**skw)
    s["targets32"] = s["targets"].float()
    s["betas32"] = s["betas"].float()
    w, kw, x0 = case(name, s)
    s["x0_32"] = x0.float()
    f = lambda t: None if t is None else t.float()
    s["kw"] = dict(kw, weights=f(kw["weights"]), wrist_prior=f(kw["wrist_prior"]))
    if "prior" in kw:
        s["kw"]["prior"] = f(kw["prior"])
    return s


# the scenes of tests/test_gpu_arm_ik.py's "one step" (tests/test_arm_ik_cpu.py asserts that EVERY frame of them is counted: float64's first
# step lowers the cost by more than 1e-3 of itself and the float32 yardstick takes the same accept / reject decision)
ONE_STEP = {"22": dict(T=24, seed=0), "21": dict(T=24, seed=0), "22_priors": dict(T=8, seed=3)}


def counted_first_step(sc):
    """(counted (T,) bool, y1 float64, y1 float32)"""
    kw = sc["kw"]
    d = lambda t: None if t is None else t.double()
    kw64 = dict(kw, weights=d(kw["weights"]), wrist_prior=d(kw["wrist_prior"]))
    y1 = lm(sc["model"], sc["x0_32"].double(), sc["betas32"].double(), sc["targets32"].double(), iters=1, **kw64)
    y1_32 = lm(sc["model"], sc["x0_32"], sc["betas32"], sc["targets32"], iters=1, dtype=torch.float32, **kw)
    c0, c1 = y1["cost"][0], y1["cost"][1]
    return ((c0 - c1) / c0 > 1e-3) & (y1["ok"][0] == y1_32["ok"][0]), y1, y1_32
