"""TEST INFRASTRUCTURE ONLY — float64 yardstick of the batched MANO inverse kinematics (csrc/ik.hip, include/harp_hip.h harp_mano_ik):
the joints through oracle.harp_ref.mano_forward on float64 tensors, the Jacobian by torch.autograd.functional.jacobian, and the
Levenberg-Marquardt iteration of the contract written out plainly with a dense float64 solve.  Also the seeded scene the CPU and GPU tests
share.  x = [rot 3 | pose 45 | trans 3] per frame."""
import numpy as np
import torch

from oracle import harp_ref

PALM = (0, 1, 5, 9, 13, 17)


def model64(model_np):
    return {k: torch.as_tensor(np.asarray(model_np[k], np.float64)) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_mean")}


def joints(model, x, betas):
    """x (T,51), betas (10,) or (T,10) float64 -> the 21 joints (T,21,3) in metres.  (mano_forward skips an all-zero trans, which would
    hide its derivative: trans is added here instead.)"""
    T = x.shape[0]
    b = betas.expand(T, 10) if betas.dim() == 1 else betas
    _, j = harp_ref.mano_forward(model, x[:, :48], b, x.new_zeros(T, 3))
    return j / 1000.0 + x[:, None, 48:51]


def jacobian(model, x, betas):
    """(T,63,51): frames are independent, so the derivative of the sum over the frames is every frame's own"""
    T = x.shape[0]
    J = torch.autograd.functional.jacobian(lambda y: joints(model, y, betas).reshape(T, 63).sum(0), x, vectorize=True)      # (63,T,51)
    return J.permute(1, 0, 2).contiguous()


def used_mask(targets, weights):
    """(T,21) bool and the weights / targets with every unused entry zeroed"""
    w = torch.ones(targets.shape[:2], dtype=torch.float64) if weights is None else weights.double()
    used = (w > 0) & torch.isfinite(targets).all(-1)
    return used, torch.where(used, w, torch.zeros_like(w)), torch.where(used[..., None], targets.double(), torch.zeros_like(targets, dtype=torch.float64))


def cost(model, x, betas, targets, weights, prior, prior_weight):
    used, w, tg = used_mask(targets, weights)
    r = (joints(model, x, betas) - tg) * used[..., None]
    p = x[:, 3:48] - (0.0 if prior is None else prior.double())
    return (w[..., None] * r * r).sum((1, 2)) + prior_weight * (p * p).sum(1), r


def lm(model, x0, betas, targets, weights=None, prior=None, prior_weight=0.0, iters=15, lambda0=1e-3):
    """The iteration of include/harp_hip.h in float64.  Returns dict(x (T,51), cost (iters + 1, T) = C after k iterations, accepted (T,)
    (-1: fewer than 3 used joints, not solved), trial (iters, T) = C(x') of every iteration's candidate, ok (iters, T) accepted flags)."""
    x = x0.double().clone()
    betas = betas.double()
    T = x.shape[0]
    used, w, tg = used_mask(targets, weights)
    solve = used.sum(1) >= 3
    lam = torch.full((T,), float(lambda0), dtype=torch.float64)
    W = w[:, :, None].expand(T, 21, 3).reshape(T, 63)
    P = torch.zeros(51, dtype=torch.float64)
    P[3:48] = prior_weight
    pr = torch.zeros(T, 45, dtype=torch.float64) if prior is None else prior.double()
    C, r = cost(model, x, betas, targets, weights, prior, prior_weight)
    hist, trial, oks = [C.clone()], [], []
    acc = torch.zeros(T, dtype=torch.int64)
    for _ in range(iters):
        J = jacobian(model, x, betas)
        A = torch.einsum("tki,tk,tkj->tij", J, W, J) + torch.diag(P)
        dx = torch.zeros(T, 51, dtype=torch.float64)
        dx[:, 3:48] = x[:, 3:48] - pr
        g = torch.einsum("tki,tk->ti", J, W * r.reshape(T, 63)) + P * dx
        D = torch.diagonal(A, dim1=1, dim2=2)
        delta = torch.linalg.solve(A + torch.diag_embed(lam[:, None] * D), -g)
        xn = x + delta
        Cn, rn = cost(model, xn, betas, targets, weights, prior, prior_weight)
        ok = solve & (Cn < C)
        x = torch.where(ok[:, None], xn, x)
        r = torch.where(ok[:, None, None], rn, r)
        C = torch.where(ok, Cn, C)
        lam = torch.where(ok, (0.1 * lam).clamp_min(1e-9), (10.0 * lam).clamp_max(1e6))
        acc += ok.long()
        hist.append(C.clone()); trial.append(Cn); oks.append(ok)
    return dict(x=x, cost=torch.stack(hist), accepted=torch.where(solve, acc, torch.full_like(acc, -1)),
                trial=torch.stack(trial) if trial else torch.zeros(0, T, dtype=torch.float64),
                ok=torch.stack(oks) if oks else torch.zeros(0, T, dtype=torch.bool))


def axis_angle_to_matrix(aa):
    aa = np.asarray(aa, np.float64)
    th = np.linalg.norm(aa)
    if th < 1e-300:
        return np.eye(3)
    k = aa / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(T=24, seed=0, root_lo=0.0, root_hi=3.1, pose_sigma=0.3, trans_range=0.3):
    """the seeded scene of the issue: pose sigma 0.3, root angle uniform in [root_lo, root_hi] about random axes, trans within +-0.3 m,
    a random shape.  Returns dict(model_np, model (float64), betas (10,), x_true (T,51), targets (T,21,3) float64 metres)."""
    from harp_amd import synth
    model_np = synth.make_mano_model()
    rng = np.random.default_rng(1234 + seed)
    x = np.zeros((T, 51))
    for t in range(T):
        u = rng.normal(size=3)
        x[t, :3] = rng.uniform(root_lo, root_hi) * u / np.linalg.norm(u)
    x[:, 3:48] = rng.normal(size=(T, 45)) * pose_sigma
    x[:, 48:] = rng.uniform(-trans_range, trans_range, size=(T, 3))
    betas = torch.as_tensor(rng.normal(size=10) * 0.5)
    model = model64(model_np)
    x_true = torch.as_tensor(x)
    with torch.no_grad():
        targets = joints(model, x_true, betas)
    return dict(model_np=model_np, model=model, betas=betas, x_true=x_true, targets=targets)


class _Layer:
    """what Motion.from_keypoints reads of a hand layer"""
    def __init__(self, model_np):
        self._model_np = model_np


def palm_x0(sc, targets=None):
    """the palm start of harp_amd.playback (host float64) as x0 (T,51) float64"""
    from harp_amd import playback
    tg = np.asarray(sc["targets"] if targets is None else targets, np.float64)
    rest = playback.rest_chain_joints(sc["model_np"], sc["betas"].numpy())
    rot, trans = playback.palm_start(tg, np.isfinite(tg).all(-1), rest)
    x0 = np.zeros((tg.shape[0], 51))
    x0[:, :3], x0[:, 48:] = rot, trans
    return torch.as_tensor(x0)
