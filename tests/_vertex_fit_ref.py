"""TEST INFRASTRUCTURE ONLY — the yardstick of the batched MANO vertex fit (csrc/vertex_fit.hip, include/harp_hip.h harp_mano_vertex_fit):
the vertices through oracle.harp_ref.mano_forward, the Jacobian by forward mode (torch.func.jvp under vmap: one tangent per column, every
frame at once — the frames are independent), and the Levenberg-Marquardt iteration of the contract written out plainly with a dense solve of
the Jacobi-scaled system.  Everything is parameterised by dtype: float64 is the truth, and THE SAME CODE in float32 (float32 forward,
float32 J^T W J, float32 Cholesky) is the error model from which the GPU tests compute their bounds.  Also the seeded scene the CPU and GPU
tests share.  x = [rot 3 | pose 45 | betas 10 | trans 3] per frame."""
import numpy as np
import torch

from oracle import harp_ref
from tests import _ik_ref

NX, NR = 61, 2334
FACTOR = 8.0           # bound = FACTOR x the float32 yardstick's error against the float64 one on the same inputs (the issue's rule)


def model_as(model, dtype):
    return {k: v.to(dtype) for k, v in model.items()}


def verts(model, x, dtype=torch.float64):
    """x (T,61) -> the 778 vertices (T,778,3) in metres, computed in `dtype`.  (mano_forward skips an all-zero trans, which would hide
    its derivative: trans is added here instead.)"""
    x = x.to(dtype)
    T = x.shape[0]
    v, _ = harp_ref.mano_forward(model_as(model, dtype), x[:, :48], x[:, 48:58], torch.zeros(T, 3, dtype=dtype))
    return v / 1000.0 + x[:, None, 58:61]


def jacobian(model, x, dtype=torch.float64):
    """(T,2334,61) in `dtype`, forward mode: column c of every frame from ONE tangent that is e_c in every frame"""
    x = x.to(dtype)
    T = x.shape[0]
    m = model_as(model, dtype)
    f = lambda y: verts(m, y, dtype)
    basis = torch.eye(NX, dtype=dtype)[:, None, :].expand(NX, T, NX)
    try:
        cols = torch.func.vmap(lambda tan: torch.func.jvp(f, (x,), (tan,))[1])(basis)                     # (61,T,778,3)
    except (RuntimeError, NotImplementedError, AttributeError):                                          # (a torch without forward mode for these ops)
        J = torch.autograd.functional.jacobian(lambda y: f(y).reshape(T, NR).sum(0), x, vectorize=True)   # (2334,T,61)
        return J.permute(1, 0, 2).contiguous()
    return cols.reshape(NX, T, NR).permute(1, 2, 0).contiguous()


def used_mask(targets, weights, dtype=torch.float64):
    """(T,778) bool and the weights / targets in `dtype` with every unused entry zeroed"""
    w = torch.ones(targets.shape[:2], dtype=dtype) if weights is None else weights.to(dtype)
    used = (w > 0) & torch.isfinite(targets).all(-1)
    return used, torch.where(used, w, torch.zeros_like(w)), torch.where(used[..., None], targets.to(dtype), torch.zeros(targets.shape, dtype=dtype))


def cost(model, x, targets, weights=None, prior=None, pose_prior_weight=0.0, shape_prior_weight=0.0, dtype=torch.float64):
    """C (T,) and the residuals (T,778,3), zero where unused"""
    x = x.to(dtype)
    used, w, tg = used_mask(targets, weights, dtype)
    r = (verts(model, x, dtype) - tg) * used[..., None]
    p = x[:, 3:48] - (0.0 if prior is None else prior.to(dtype))
    return (w[..., None] * r * r).sum((1, 2)) + pose_prior_weight * (p * p).sum(1) + shape_prior_weight * (x[:, 48:58] ** 2).sum(1), r


def normal(model, x, targets, weights=None, prior=None, pose_prior_weight=0.0, shape_prior_weight=0.0, solve_shape=True, dtype=torch.float64):
    """dict(J (T,2334,61), A (T,61,61), g (T,61), C (T,), r) at x: the contract's normal equations, frozen columns included"""
    x = x.to(dtype)
    T = x.shape[0]
    used, w, tg = used_mask(targets, weights, dtype)
    C, r = cost(model, x, targets, weights, prior, pose_prior_weight, shape_prior_weight, dtype)
    J = jacobian(model, x, dtype)
    W = w[:, :, None].expand(T, 778, 3).reshape(T, NR)
    P = torch.zeros(NX, dtype=dtype)
    P[3:48], P[48:58] = pose_prior_weight, shape_prior_weight
    dx = torch.zeros(T, NX, dtype=dtype)
    dx[:, 3:48] = x[:, 3:48] - (0.0 if prior is None else prior.to(dtype))
    dx[:, 48:58] = x[:, 48:58]
    A = torch.einsum("tki,tk,tkj->tij", J, W, J) + torch.diag(P)
    g = torch.einsum("tki,tk->ti", J, W * r.reshape(T, NR)) + P * dx
    if not solve_shape:
        A[:, 48:58, :] = 0.0
        A[:, :, 48:58] = 0.0
        A[:, range(48, 58), range(48, 58)] = 1.0
        g[:, 48:58] = 0.0
    return dict(J=J, A=A, g=g, C=C, r=r)


def lm(model, x0, targets, weights=None, prior=None, pose_prior_weight=0.0, shape_prior_weight=0.0, solve_shape=True, iters=10, lambda0=1e-3,
       dtype=torch.float64):
    """The iteration of include/harp_hip.h in `dtype`.  Returns dict(x (T,61), cost (iters + 1, T) = C after k iterations, accepted (T,)
    (-1: fewer than 21 used vertices, not solved), trial (iters, T) = C(x') of every iteration's candidate, ok (iters, T) accepted flags)."""
    x = x0.to(dtype).clone()
    T = x.shape[0]
    used, _, _ = used_mask(targets, weights, dtype)
    solve = used.sum(1) >= 21
    lam = torch.full((T,), float(lambda0), dtype=dtype)
    kw = dict(weights=weights, prior=prior, pose_prior_weight=pose_prior_weight, shape_prior_weight=shape_prior_weight, dtype=dtype)
    C, _ = cost(model, x, targets, **kw)
    hist, trial, oks = [C.clone()], [], []
    acc = torch.zeros(T, dtype=torch.int64)
    for _ in range(iters):
        n = normal(model, x, targets, solve_shape=solve_shape, **kw)
        D = torch.diagonal(n["A"], dim1=1, dim2=2)
        s = 1.0 / torch.sqrt(D * (1.0 + lam[:, None]))
        good = (D > 0).all(1) & torch.isfinite(s).all(1)
        s = torch.where(good[:, None], s, torch.ones_like(s))
        S = s[:, :, None] * (n["A"] + torch.diag_embed(lam[:, None] * D)) * s[:, None, :]
        S = torch.where(good[:, None, None], S, torch.eye(NX, dtype=dtype).expand(T, NX, NX))
        L, info = torch.linalg.cholesky_ex(S)
        good = good & (info == 0) & torch.isfinite(L).all((1, 2))
        L = torch.where(good[:, None, None], L, torch.eye(NX, dtype=dtype).expand(T, NX, NX))
        z = torch.cholesky_solve((-n["g"] * s)[:, :, None], L)[:, :, 0]
        xn = x + s * z
        Cn, _ = cost(model, xn, targets, **kw)
        ok = solve & good & (Cn < C)
        x = torch.where(ok[:, None], xn, x)
        C = torch.where(ok, Cn, C)
        lam = torch.where(ok, (0.1 * lam).clamp_min(1e-9), (10.0 * lam).clamp_max(1e6))
        acc += ok.long()
        hist.append(C.clone()); trial.append(Cn); oks.append(ok)
    return dict(x=x, cost=torch.stack(hist), accepted=torch.where(solve, acc, torch.full_like(acc, -1)),
                trial=torch.stack(trial) if trial else torch.zeros(0, T, dtype=dtype),
                ok=torch.stack(oks) if oks else torch.zeros(0, T, dtype=torch.bool))


def rms_mm(model, x, targets, dtype=torch.float64):
    """RMS vertex distance to the targets per frame, millimetres (float64 arithmetic on the vertices computed in `dtype`)"""
    with torch.no_grad():
        d = verts(model, x, dtype).double() - targets.double()
    return d.pow(2).sum(-1).mean(1).sqrt() * 1000.0


def scene(T=8, seed=0, noise=0.0, **kw):
    """_ik_ref.scene's poses (root angle up to 3.1 rad, pose sigma 0.3, trans within +-0.3 m) plus per-frame betas sigma 0.5, and the
    vertices they give plus Gaussian noise of `noise` metres per coordinate.  Returns dict(model_np, model (float64), x_true (T,61),
    targets (T,778,3) float64 metres)."""
    s = _ik_ref.scene(T=T, seed=seed, **kw)
    rng = np.random.default_rng(4321 + seed)
    betas = rng.normal(size=(T, 10)) * 0.5
    x_true = torch.cat([s["x_true"][:, :48], torch.as_tensor(betas), s["x_true"][:, 48:]], 1)
    with torch.no_grad():
        targets = verts(s["model"], x_true)
    if noise:
        targets = targets + torch.as_tensor(rng.normal(size=tuple(targets.shape)) * noise)
    return dict(model_np=s["model_np"], model=s["model"], x_true=x_true, targets=targets)


def rest(model, betas):
    """what playback.vertex_start takes of the model: its vertices (T,778,3) and root joint (T,3) at `betas` (T,10), zero stored pose and
    zero trans, float64 numpy, metres"""
    T = betas.shape[0]
    with torch.no_grad():
        v, j = harp_ref.mano_forward(model, torch.zeros(T, 48, dtype=torch.float64), betas.double(), torch.zeros(T, 3, dtype=torch.float64))
    return v.numpy() / 1000.0, j[:, 0].numpy() / 1000.0


def rigid_x0(sc, targets=None, betas=None, weights=None):
    """the rigid start of harp_amd.playback.vertex_start as x0 (T,61) float64: pose zero, betas as given (default zero)"""
    from harp_amd import playback
    tg = (sc["targets"] if targets is None else targets).double()
    T = tg.shape[0]
    b = torch.zeros(T, 10, dtype=torch.float64) if betas is None else betas.double().expand(T, 10)
    rv, rj = rest(sc["model"], b)
    used = np.ones((T, 778)) if weights is None else np.asarray(weights, np.float64)
    rot, trans = playback.vertex_start(tg.numpy(), used, rv, rj)
    x0 = torch.zeros(T, NX, dtype=torch.float64)
    x0[:, :3], x0[:, 48:58], x0[:, 58:] = torch.as_tensor(rot), b, torch.as_tensor(trans)
    return x0
