"""TEST INFRASTRUCTURE ONLY — float64 yardstick of the batched 2.5-D reprojection inverse kinematics (csrc/reproj_ik.hip, include/harp_hip.h
harp_mano_reproj_ik): the joints through oracle.harp_ref.mano_forward on float64 tensors (tests/_ik_ref.joints), the
projection of the contract written out, the Jacobian by torch.autograd.functional.jacobian, and the Levenberg-Marquardt iteration with a
dense float64 solve.  Also the seeded image scene the CPU and GPU tests share, and an emulation of the float32 normal equations and
Cholesky of one step.  x = [rot 3 | pose 45 | trans 3] per problem; rows (u, v, d) per joint."""
import numpy as np
import torch

from tests import _ik_ref as R3

Z_MIN = 1e-3
CAM = (8.9, 0.01, -0.02)
FOCAL, S = 2000.0, 448
POSE_PRIOR_PX = 40.0                  # px^2 / rad^2: 1e-5 (focal / Z)^2 at focal 2000 and 1 m
Z_PRIOR_PX = 100.0                    # px^2 / m^2: 2.5e-5 (focal / Z)^2


def tz_of(cam, focal, S):
    return 2.0 * focal / (S * cam[..., 0] + 1e-9)


def project(j, cam, focal, S):
    """j (T,21,3) metres, cam (3,) or (T,3) -> rows (T,21,3) = (u, v, d) and Z (T,21)"""
    cam = cam.expand(j.shape[0], 3) if cam.dim() == 1 else cam
    Z = j[..., 2] + tz_of(cam, focal, S)[:, None]
    u = S / 2.0 + focal * (j[..., 0] + cam[:, 1, None]) / Z
    v = S / 2.0 + focal * (j[..., 1] + cam[:, 2, None]) / Z
    return torch.stack([u, v, j[..., 2] - j[..., :1, 2]], -1), Z


def rows(model, x, betas, cam, focal, S):
    return project(R3.joints(model, x, betas), cam, focal, S)


def jacobian(model, x, betas, cam, focal, S):
    """(T,63,51): problems are independent, so the derivative of the sum over the problems is every problem's own"""
    T = x.shape[0]
    J = torch.autograd.functional.jacobian(lambda y: rows(model, y, betas, cam, focal, S)[0].reshape(T, 63).sum(0), x, vectorize=True)
    return J.permute(1, 0, 2).contiguous()


def used_masks(targets, weights, depth_weights):
    """row weights W (T,21,3) = (w, w, wz) with every unused row at 0, the targets with every unused entry at 0, and the pixel-used mask"""
    T = targets.shape[0]
    w = torch.ones(T, 21, dtype=torch.float64) if weights is None else weights.double()
    wz = torch.zeros(T, 21, dtype=torch.float64) if depth_weights is None else depth_weights.double().clone()
    wz[:, 0] = 0.0
    up = (w > 0) & torch.isfinite(targets[..., :2]).all(-1)
    uz = (wz > 0) & torch.isfinite(targets[..., 2])
    W = torch.stack([torch.where(up, w, torch.zeros_like(w))] * 2 + [torch.where(uz, wz, torch.zeros_like(wz))], -1)
    tg = torch.where(W > 0, targets.double(), torch.zeros_like(W))
    return W, tg, up


def cost(model, x, betas, cam, focal, S, targets, weights=None, depth_weights=None, prior=None, pose_prior_weight=0.0, z_prior=None,
         z_prior_weight=0.0):
    """C (T,), residuals (T,21,3) (0 in unused rows), behind (T,) = a used pixel joint at Z <= Z_MIN"""
    W, tg, up = used_masks(targets, weights, depth_weights)
    p, Z = rows(model, x, betas, cam, focal, S)
    r = torch.where(W > 0, p - tg, torch.zeros_like(p))
    dp = x[:, 3:48] - (0.0 if prior is None else prior.double())
    C = (W * r * r).sum((1, 2)) + pose_prior_weight * (dp * dp).sum(1)
    if z_prior is not None:
        C = C + z_prior_weight * (x[:, 50] - z_prior.double()) ** 2
    return C, r, (up & (Z <= Z_MIN)).any(1)


def normal_equations(J, W, r, x, prior, pose_prior_weight, z_prior, z_prior_weight):
    """A (T,51,51), g (T,51) of the contract"""
    T = J.shape[0]
    Wf = W.reshape(T, 63)
    P = torch.zeros(51, dtype=J.dtype)
    P[3:48] = pose_prior_weight
    P[50] = z_prior_weight if z_prior is not None else 0.0
    dx = torch.zeros(T, 51, dtype=J.dtype)
    dx[:, 3:48] = x[:, 3:48] - (0.0 if prior is None else prior.to(J.dtype))
    if z_prior is not None:
        dx[:, 50] = x[:, 50] - z_prior.to(J.dtype)
    A = torch.einsum("tki,tk,tkj->tij", J, Wf, J) + torch.diag(P)
    g = torch.einsum("tki,tk->ti", J, Wf * r.reshape(T, 63)) + P * dx
    return A, g


def scaled(A, lam):
    """s (A + lam diag A) s with s = 1 / sqrt(A_ii (1 + lam)): a unit diagonal"""
    D = torch.diagonal(A, dim1=1, dim2=2)
    s = 1.0 / torch.sqrt(D * (1.0 + lam[:, None]))
    return (A + torch.diag_embed(lam[:, None] * D)) * s[:, :, None] * s[:, None, :], s


def lm(model, x0, betas, cam, focal, S, targets, weights=None, depth_weights=None, prior=None, pose_prior_weight=0.0, z_prior=None,
       z_prior_weight=0.0, iters=20, lambda0=1e-3, conds=False, history=False):
    """The iteration of include/harp_hip.h in float64.  Returns dict(x (T,51), cost (iters + 1, T) = C after k iterations, status (T,)
    (accepted steps; -1: fewer than 4 used pixel joints; -2: behind the camera at the input), ok (iters, T) accepted flags, last_drop (T,)
    = the relative cost decrease of the last accepted step (0: none), cond (iters, T) of the scaled matrix when conds=True, xs (iters + 1,
    T, 51) and drops (iters + 1, T) = x and last_drop after k iterations when history=True)."""
    x = x0.double().clone()
    betas, cam = betas.double(), cam.double()
    T = x.shape[0]
    kw = dict(weights=weights, depth_weights=depth_weights, prior=prior, pose_prior_weight=pose_prior_weight, z_prior=z_prior,
              z_prior_weight=z_prior_weight)
    W, tg, up = used_masks(targets, weights, depth_weights)
    with torch.no_grad():
        C, r, behind0 = cost(model, x, betas, cam, focal, S, targets, **kw)
    enough = up.sum(1) >= 4
    solve = enough & ~behind0
    lam = torch.full((T,), float(lambda0), dtype=torch.float64)
    hist, oks, cds, xs, drops = [C.clone()], [], [], [x.clone()], [torch.zeros(T, dtype=torch.float64)]
    acc = torch.zeros(T, dtype=torch.int64)
    last_drop = torch.zeros(T, dtype=torch.float64)
    for _ in range(iters):
        J = jacobian(model, x, betas, cam, focal, S)
        A, g = normal_equations(J, W, r, x, prior, pose_prior_weight, z_prior, z_prior_weight)
        D = torch.diagonal(A, dim1=1, dim2=2)
        if conds:
            cds.append(torch.linalg.cond(scaled(A, lam)[0]))
        delta = torch.linalg.solve(A + torch.diag_embed(lam[:, None] * D), -g)
        xn = x + delta
        with torch.no_grad():
            Cn, rn, behind = cost(model, xn, betas, cam, focal, S, targets, **kw)
        ok = solve & ~behind & (Cn < C)
        last_drop = torch.where(ok, (C - Cn) / C, last_drop)
        x = torch.where(ok[:, None], xn, x)
        r = torch.where(ok[:, None, None], rn, r)
        C = torch.where(ok, Cn, C)
        lam = torch.where(ok, (0.1 * lam).clamp_min(1e-9), (10.0 * lam).clamp_max(1e6))
        acc += ok.long()
        hist.append(C.clone()); oks.append(ok)
        if history:
            xs.append(x.clone()); drops.append(last_drop.clone())
    status = torch.where(enough, torch.where(behind0, torch.full_like(acc, -2), acc), torch.full_like(acc, -1))
    return dict(x=x, cost=torch.stack(hist), status=status, ok=torch.stack(oks) if oks else torch.zeros(0, T, dtype=torch.bool),
                last_drop=last_drop, cond=torch.stack(cds) if cds else None, xs=torch.stack(xs) if history else None,
                drops=torch.stack(drops) if history else None)


def step_float32(model, x, betas, cam, focal, S, targets, lam, **kw):
    """One step's delta with the NORMAL EQUATIONS AND THE CHOLESKY in float32 (J, W, r rounded to float32 first; A and g accumulated, the
    matrix scaled, factored and solved in float32) beside the float64 delta from the same J: (delta32 (T,51) as float64, delta64)."""
    W, tg, _ = used_masks(targets, kw.get("weights"), kw.get("depth_weights"))
    with torch.no_grad():
        _, r, _ = cost(model, x, betas, cam, focal, S, targets, **kw)
    J = jacobian(model, x, betas, cam, focal, S)
    args = (kw.get("prior"), kw.get("pose_prior_weight", 0.0), kw.get("z_prior"), kw.get("z_prior_weight", 0.0))
    lam = torch.full((x.shape[0],), float(lam), dtype=torch.float64)
    out = []
    for dt in (torch.float32, torch.float64):
        A, g = normal_equations(J.to(dt), W.to(dt), r.to(dt), x.to(dt), *args)
        Sm, s = scaled(A, lam.to(dt))
        L = torch.linalg.cholesky(Sm)
        z = torch.cholesky_solve((-g * s)[..., None], L)[..., 0]
        out.append((z * s).double())
    return out[0], out[1]


def scene(T=24, seed=0, cam=CAM, focal=FOCAL, S=S):
    """the seeded image scene of the issue: tests/_ik_ref.scene(T, seed, trans_range=0.05) seen through cam / focal / S.  Adds cam (3,),
    focal, S, rows (T,21,3) = the true (u, v, d) float64."""
    sc = R3.scene(T=T, seed=seed, trans_range=0.05)
    sc["cam"], sc["focal"], sc["S"] = torch.as_tensor(cam, dtype=torch.float64), float(focal), int(S)
    with torch.no_grad():
        sc["rows"], _ = project(sc["targets"], sc["cam"], focal, S)
    return sc


def planar_x0(sc, rows=None):
    """the two planar starts of harp_amd.playback (host float64) as x0 (T,2,51) float64, and the start's palm depth (T,)"""
    from harp_amd import playback
    px = np.asarray(sc["rows"] if rows is None else rows, np.float64)[..., :2]
    rest = playback.rest_chain_joints(sc["model_np"], sc["betas"].numpy())
    rot, trans, depth = playback.planar_palm_starts(px, np.isfinite(px).all(-1), rest, sc["cam"].numpy(), sc["focal"], sc["S"])
    x0 = np.zeros(rot.shape[:2] + (51,))
    x0[..., :3], x0[..., 48:] = rot, trans
    return torch.as_tensor(x0), torch.as_tensor(depth)
