"""The bits of the six batched Levenberg-Marquardt solvers (csrc/ik.hip, reproj_ik.hip, arm_ik.hip, vertex_fit.hip, arm_vertex_fit.hip,
arm_reproj_ik.hip): a SHA-256 of the raw bytes of every output tensor of one small deterministic batch per solver and per setting of
solve_shape / solve_wrist.  Two builds of the library that print the same digests compute the same thing; the file touches nothing but
harp_amd.ops and the synthetic hand and arm models, so it runs unchanged against an older checkout.

Each batch: 4 problems from a start near the truth (the targets are the solver's own forward at iters = 0 of a true point), 3 iterations,
every optional output; problem 3 has fewer used targets than the solver asks for (status -1), one unused target is NaN, and problem 2 of
the reprojection solves starts with its used joints behind the camera (status -2; the arm's: -3).  The arm's reprojection solve and its
constructor (§35) come last in their parts, with random streams of their own, and are left out against a checkout that has neither: the
digests of the five older solvers stay comparable across that commit.

The second part does the same for the layer above: every field of the Motion that each of the five Motion.from_*
constructors returns for 4 frames, once from the rigid start, once with init= and, for the three keypoint constructors, once with
smooth=1.0 (a dropped joint is filled); the arm's two in both of their input layouts.  Public API only, as the first part.

    python tools/dev/gpu_solver_bits.py [--out profiles/solver_front_bits_new.json]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

T, ITERS = 4, 3
CAM, FOCAL, S = (8.9, 0.01, -0.02), 2000.0, 448
DEV = "cuda"


def up(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=DEV)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def record(res, name, out, inputs):
    res[name + "/inputs"] = hashlib.sha256("".join(digest(t) for t in inputs if t is not None).encode()).hexdigest()
    for f in out._fields:
        t = getattr(out, f)
        if t is not None:
            res[f"{name}/{f}"] = digest(t)
    res[name + "/status_values"] = out.status.cpu().tolist()


def weights_with_few(n, few, rng):
    """(T, n) weights in [0.5, 1.5], some zero; the last problem keeps only `few` targets"""
    w = rng.uniform(0.5, 1.5, size=(T, n))
    w[0, 1] = 0.0
    w[T - 1, few:] = 0.0
    return w


def hand(res):
    from harp_amd import ops, synth
    from harp_amd.manopth.manolayer import ManoLayer
    dm = ManoLayer(flat_hand_mean=False, use_pca=False, model=synth.make_mano_model(), device=DEV).device_model
    rng = np.random.default_rng(31)
    pose = np.concatenate([rng.normal(size=(T, 3)) * 0.8, rng.normal(size=(T, 45)) * 0.3], 1)
    trans = rng.uniform(-0.05, 0.05, size=(T, 3))
    betas = rng.normal(size=(T, 10)) * 0.5
    x0, t0 = up(pose + rng.normal(size=pose.shape) * 0.05), up(trans + rng.normal(size=trans.shape) * 0.01)
    prior = up(rng.normal(size=(T, 45)) * 0.1)

    # 3-D keypoints
    kp = ops.mano_ik(dm, up(betas), torch.zeros(T, 21, 3, device=DEV), up(pose), up(trans), iters=0, joints=True).joints / 1000.0
    w = weights_with_few(21, 2, rng)
    tg = kp.clone()
    tg[0, 1] = float("nan")
    args = (up(betas), tg.contiguous(), x0, t0)
    kw = dict(weights=up(w), prior=prior, prior_weight=1e-4, iters=ITERS, joints=True, jac=True)
    record(res, "mano_ik", ops.mano_ik(dm, *args, **kw), args + (kw["weights"], prior))

    # image keypoints: the camera of csrc/reproj_ik.hip's header
    j = kp.cpu().double().numpy()
    Z = j[..., 2] + 2.0 * FOCAL / (S * CAM[0] + 1e-9)
    rows = np.stack([S / 2 + FOCAL * (j[..., 0] + CAM[1]) / Z, S / 2 + FOCAL * (j[..., 1] + CAM[2]) / Z, j[..., 2] - j[:, :1, 2]], -1)
    rows[0, 1] = np.nan
    w = weights_with_few(21, 3, rng)
    wz = rng.uniform(0.5, 1.5, size=(T, 21)) * 1e6
    t0r = t0.clone()
    t0r[2, 2] = -2.0                                       # every joint of problem 2 behind the camera at the input
    args = (up(betas), up(rows), x0, t0r, up(CAM), FOCAL, S)
    kw = dict(weights=up(w), depth_weights=up(wz), prior=prior, z_prior=up(trans[:, 2]), pose_prior_weight=1e-2, z_prior_weight=1.0,
              iters=ITERS, proj=True, jac=True)
    record(res, "mano_reproj_ik", ops.mano_reproj_ik(dm, *args, **kw),
           (args[0], args[1], x0, t0r, args[4], kw["weights"], kw["depth_weights"], prior, kw["z_prior"]))

    # mesh vertices
    z = torch.zeros(T, 10, device=DEV)
    verts = ops.mano_vertex_fit(dm, torch.zeros(T, 778, 3, device=DEV), up(pose), up(betas), up(trans), iters=0, verts=True).verts / 1000.0
    w = weights_with_few(778, 20, rng)
    tg = verts.clone()
    tg[0, 1] = float("nan")
    for solve_shape in (True, False):
        b0 = z if solve_shape else up(betas)
        args = (tg.contiguous(), x0, b0, t0)
        kw = dict(weights=up(w), prior=prior, solve_shape=solve_shape, pose_prior_weight=1e-4, shape_prior_weight=1e-5, iters=ITERS,
                  verts=True, jac=True, normal=True)
        record(res, f"mano_vertex_fit/shape{int(solve_shape)}", ops.mano_vertex_fit(dm, *args, **kw), args + (kw["weights"], prior))


def arm(res):
    from harp_amd import ops, synth
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    import harp_amd
    model = synth.make_smplx_arm_model(seed=0)
    corr = np.load(os.path.join(os.path.dirname(os.path.abspath(harp_amd.__file__)), "assets", "arm_corr.npz"))
    dm = SMPLXARM(model, model["faces"], corr["mano_vert_from_arm"], device=DEV).device_model
    rng = np.random.default_rng(37)
    rows = np.concatenate([rng.normal(size=(T, 1, 3)) * 0.8, rng.normal(size=(T, 16, 3)) * 0.3], 1)
    trans = rng.uniform(-0.3, 0.3, size=(T, 3))
    betas = rng.normal(size=(T, 10)) * 0.5
    x0, t0 = up(rows + rng.normal(size=rows.shape) * 0.05), up(trans + rng.normal(size=trans.shape) * 0.01)
    prior, wprior = up(rng.normal(size=(T, 45)) * 0.1), up(rng.normal(size=(T, 3)) * 0.1)

    # 3-D keypoints
    n = int(dm.struct.n_joints_out)
    kp = ops.arm_ik(dm, up(betas), torch.zeros(T, n, 3, device=DEV), up(rows), up(trans), iters=0, joints=True).joints / 1000.0
    w = weights_with_few(n, 2, rng)
    tg = kp.clone()
    tg[0, 1] = float("nan")
    for solve_wrist in (True, False):
        args = (up(betas), tg.contiguous(), x0, t0)
        kw = dict(weights=up(w), prior=prior, wrist_prior=wprior, solve_wrist=solve_wrist, pose_prior_weight=1e-4, wrist_prior_weight=1e-3,
                  iters=ITERS, joints=True, jac=True)
        record(res, f"arm_ik/wrist{int(solve_wrist)}", ops.arm_ik(dm, *args, **kw), args + (kw["weights"], prior, wprior))

    # mesh vertices, all of the arm's
    NV = int(model["v_template"].shape[0])
    z = torch.zeros(T, 10, device=DEV)
    verts = ops.arm_vertex_fit(dm, torch.zeros(T, NV, 3, device=DEV), up(rows), up(betas), up(trans), iters=0, verts=True).verts / 1000.0
    w = weights_with_few(NV, 21, rng)
    tg = verts.clone()
    tg[0, 1] = float("nan")
    for solve_shape in (True, False):
        for solve_wrist in (True, False):
            b0 = z if solve_shape else up(betas)
            args = (tg.contiguous(), x0, b0, t0)
            kw = dict(weights=up(w), prior=prior, solve_shape=solve_shape, solve_wrist=solve_wrist, pose_prior_weight=1e-4,
                      wrist_prior_weight=1e-3, shape_prior_weight=1e-5, iters=ITERS, verts=True, jac=True, normal=True)
            record(res, f"arm_vertex_fit/shape{int(solve_shape)}_wrist{int(solve_wrist)}", ops.arm_vertex_fit(dm, *args, **kw),
                   args + (kw["weights"], prior))

    # image keypoints (csrc/arm_reproj_ik.hip): a stream of its own, so that what stands above does not move
    if not hasattr(ops, "arm_reproj_ik"):
        return
    rng = np.random.default_rng(39)
    tr = rng.uniform(-0.05, 0.05, size=(T, 3))
    j = (ops.arm_ik(dm, up(betas), torch.zeros(T, n, 3, device=DEV), up(rows), up(tr), iters=0, joints=True).joints / 1000.0).cpu().double().numpy()
    Z = j[..., 2] + 2.0 * FOCAL / (S * CAM[0] + 1e-9)
    px = np.stack([S / 2 + FOCAL * (j[..., 0] + CAM[1]) / Z, S / 2 + FOCAL * (j[..., 1] + CAM[2]) / Z, j[..., 2] - j[:, :1, 2]], -1)
    px[0, 1] = np.nan
    w = weights_with_few(n, 3, rng)
    wz = rng.uniform(0.5, 1.5, size=(T, n)) * 1e6
    t0r = up(tr + rng.normal(size=tr.shape) * 0.01)
    t0r[2, 2] = -2.0                                       # every joint of problem 2 behind the camera at the input
    for solve_wrist in (True, False):
        args = (up(betas), up(px), x0, t0r, up(CAM), FOCAL, S)
        kw = dict(weights=up(w), depth_weights=up(wz), prior=prior, wrist_prior=wprior, z_prior=up(tr[:, 2]), solve_wrist=solve_wrist,
                  pose_prior_weight=40.0, wrist_prior_weight=400.0, z_prior_weight=100.0, iters=ITERS, proj=True, jac=True)
        record(res, f"arm_reproj_ik/wrist{int(solve_wrist)}", ops.arm_reproj_ik(dm, *args, **kw),
               (args[0], args[1], x0, t0r, args[4], kw["weights"], kw["depth_weights"], prior, wprior, kw["z_prior"]))


def record_motion(res, name, m):
    for f in m.FIELDS:
        if getattr(m, f) is not None:
            res[f"Motion.{name}/{f}"] = digest(getattr(m, f))


def hand_motions(res):
    """Motion.from_keypoints, from_image_keypoints and from_vertices: from the rigid start, with init=, and (keypoints) with smooth=1.0"""
    from harp_amd import ops, synth
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.playback import Motion
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=synth.make_mano_model(), device=DEV)
    dm = layer.device_model
    rng = np.random.default_rng(41)
    pose = np.concatenate([rng.normal(size=(T, 3)) * 0.5, rng.normal(size=(T, 45)) * 0.2], 1)
    trans = rng.uniform(-0.03, 0.03, size=(T, 3))
    shape = rng.normal(size=10) * 0.5
    cam = np.array(CAM) + rng.uniform(-0.01, 0.01, size=(T, 3))
    params = dict(shape=up(shape), cam=up(cam))
    init = Motion(pose[:, 3:] + rng.normal(size=(T, 45)) * 0.05, pose[:, :3] + rng.normal(size=(T, 3)) * 0.05,
                  trans + rng.normal(size=(T, 3)) * 0.005, cam)
    w = rng.uniform(0.5, 1.5, size=(T, 21))
    w[1, 7] = 0.0                                          # a joint that the window fills under smooth=

    kp = (ops.mano_ik(dm, up(shape), torch.zeros(T, 21, 3, device=DEV), up(pose), up(trans), iters=0, joints=True).joints / 1000.0).cpu().double().numpy()
    noisy = kp * 1.07 + rng.normal(size=kp.shape) * 1e-3   # another hand's size: the bone-length scale has work to do
    noisy[2, 11] = np.nan
    record_motion(res, "from_keypoints/rigid", Motion.from_keypoints(noisy, params, layer, weights=w, device=DEV))
    record_motion(res, "from_keypoints/init", Motion.from_keypoints(noisy, params, layer, cam=cam[0], init=init, device=DEV))
    record_motion(res, "from_keypoints/smooth", Motion.from_keypoints(noisy, params, layer, weights=w, smooth=1.0, device=DEV))

    Z = kp[..., 2] + 2.0 * FOCAL / (S * cam[:, :1] + 1e-9)
    px = np.stack([S / 2 + FOCAL * (kp[..., 0] + cam[:, 1:2]) / Z, S / 2 + FOCAL * (kp[..., 1] + cam[:, 2:3]) / Z], -1)
    px = px + rng.normal(size=px.shape) * 0.3
    px[2, 11] = np.nan
    depth = kp[..., 2] - kp[:, :1, 2]
    cfg = dict(focal_length=FOCAL, img_size=S)
    record_motion(res, "from_image_keypoints/rigid", Motion.from_image_keypoints(px, params, layer, cam=cam, weights=w, depth=depth, configs=cfg, device=DEV))
    record_motion(res, "from_image_keypoints/init", Motion.from_image_keypoints(px, params, layer, cam=cam, init=init, configs=cfg, device=DEV))
    record_motion(res, "from_image_keypoints/smooth",
                  Motion.from_image_keypoints(px, params, layer, cam=cam, weights=w, depth=depth, smooth=1.0, configs=cfg, device=DEV))

    verts = (ops.mano_vertex_fit(dm, torch.zeros(T, 778, 3, device=DEV), up(pose), up(shape), up(trans), solve_shape=False, iters=0,
                                 verts=True).verts / 1000.0).cpu().double().numpy()
    verts = verts + rng.normal(size=verts.shape) * 1e-3
    verts[0, 5] = np.nan
    wv = rng.uniform(0.5, 1.5, size=(T, 778))
    record_motion(res, "from_vertices/rigid", Motion.from_vertices(verts, params, layer, weights=wv, pose_prior_weight=1e-4, device=DEV))
    record_motion(res, "from_vertices/init", Motion.from_vertices(verts, params, layer, init=init, device=DEV))


def arm_motions(res):
    """Motion.from_arm_vertices (arm and MANO topology) and from_arm_keypoints (with and without the elbow): rigid start, init=, smooth=1.0"""
    from harp_amd import ops, synth
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    from harp_amd.playback import Motion
    import harp_amd
    model = synth.make_smplx_arm_model(seed=0)
    corr = np.load(os.path.join(os.path.dirname(os.path.abspath(harp_amd.__file__)), "assets", "arm_corr.npz"))
    layer = SMPLXARM(model, model["faces"], corr["mano_vert_from_arm"], device=DEV)
    dm = layer.device_model
    rng = np.random.default_rng(43)
    rows = np.concatenate([rng.normal(size=(T, 1, 3)) * 0.5, rng.normal(size=(T, 1, 3)) * 0.1, rng.normal(size=(T, 15, 3)) * 0.2], 1)
    trans = rng.uniform(-0.2, 0.2, size=(T, 3))
    shape = rng.normal(size=10) * 0.5
    cam = np.array(CAM) + rng.uniform(-0.01, 0.01, size=(T, 3))
    params = dict(shape=up(shape), cam=up(cam))
    init = Motion(rows[:, 2:].reshape(T, 45) + rng.normal(size=(T, 45)) * 0.05, rows[:, 0] + rng.normal(size=(T, 3)) * 0.05,
                  trans + rng.normal(size=(T, 3)) * 0.005, cam, wrist_pose=rows[:, 1] + rng.normal(size=(T, 3)) * 0.02)

    n = int(dm.struct.n_joints_out)
    kp = (ops.arm_ik(dm, up(shape), torch.zeros(T, n, 3, device=DEV), up(rows), up(trans), iters=0, joints=True).joints / 1000.0).cpu().double().numpy()
    noisy = trans[:, None] + (kp - trans[:, None]) * 1.05 + rng.normal(size=kp.shape) * 1e-3
    noisy[2, 11] = np.nan
    w = rng.uniform(0.5, 1.5, size=(T, n))
    w[1, 7] = 0.0
    record_motion(res, "from_arm_keypoints/rigid", Motion.from_arm_keypoints(noisy, params, layer, weights=w, device=DEV))
    record_motion(res, "from_arm_keypoints/init", Motion.from_arm_keypoints(noisy, params, layer, cam=cam[0], init=init, wrist_pose=rows[0, 1], device=DEV))
    record_motion(res, "from_arm_keypoints/smooth", Motion.from_arm_keypoints(noisy, params, layer, weights=w, smooth=1.0, device=DEV))
    record_motion(res, "from_arm_keypoints/hand_rigid",
                  Motion.from_arm_keypoints(noisy[:, :21], params, layer, weights=w[:, :21], wrist_pose=rows[:, 1], device=DEV))
    record_motion(res, "from_arm_keypoints/hand_init", Motion.from_arm_keypoints(noisy[:, :21], params, layer, init=init, device=DEV))
    record_motion(res, "from_arm_keypoints/hand_smooth", Motion.from_arm_keypoints(noisy[:, :21], params, layer, smooth=1.0, device=DEV))

    NV = int(model["v_template"].shape[0])
    verts = (ops.arm_vertex_fit(dm, torch.zeros(T, NV, 3, device=DEV), up(rows), up(shape), up(trans), solve_shape=False, iters=0,
                                verts=True).verts / 1000.0).cpu().double().numpy()
    verts = verts + rng.normal(size=verts.shape) * 1e-3
    verts[0, 5] = np.nan
    wv = rng.uniform(0.5, 1.5, size=(T, NV))
    idx = np.asarray(corr["mano_vert_from_arm"]).reshape(-1)
    record_motion(res, "from_arm_vertices/rigid", Motion.from_arm_vertices(verts, params, layer, weights=wv, pose_prior_weight=1e-4, device=DEV))
    record_motion(res, "from_arm_vertices/init", Motion.from_arm_vertices(verts, params, layer, init=init, device=DEV))
    record_motion(res, "from_arm_vertices/mano_rigid",
                  Motion.from_arm_vertices(verts[:, idx], params, layer, weights=wv[:, idx], wrist_pose=rows[:, 1], device=DEV))
    record_motion(res, "from_arm_vertices/mano_init", Motion.from_arm_vertices(verts[:, idx], params, layer, cam=cam, init=init, device=DEV))

    # image keypoints (§35), both widths: rigid starts, init=, smooth=1.0; a stream of its own
    if not hasattr(Motion, "from_arm_image_keypoints"):
        return
    rng = np.random.default_rng(47)
    tr = rng.uniform(-0.03, 0.03, size=(T, 3))
    j = (ops.arm_ik(dm, up(shape), torch.zeros(T, n, 3, device=DEV), up(rows), up(tr), iters=0, joints=True).joints / 1000.0).cpu().double().numpy()
    Z = j[..., 2] + 2.0 * FOCAL / (S * cam[:, :1] + 1e-9)
    px = np.stack([S / 2 + FOCAL * (j[..., 0] + cam[:, 1:2]) / Z, S / 2 + FOCAL * (j[..., 1] + cam[:, 2:3]) / Z], -1)
    px = px + rng.normal(size=px.shape) * 0.3
    px[2, 11] = np.nan
    depth = j[..., 2] - j[:, :1, 2]
    cfg = dict(focal_length=FOCAL, img_size=S)
    init2 = Motion(init.pose, init.rot, tr + rng.normal(size=(T, 3)) * 0.005, cam, wrist_pose=init.wrist_pose)
    f = Motion.from_arm_image_keypoints
    record_motion(res, "from_arm_image_keypoints/rigid", f(px, params, layer, cam=cam, weights=w, depth=depth, configs=cfg, device=DEV))
    record_motion(res, "from_arm_image_keypoints/init", f(px, params, layer, cam=cam, init=init2, configs=cfg, device=DEV))
    record_motion(res, "from_arm_image_keypoints/smooth", f(px, params, layer, cam=cam, weights=w, depth=depth, smooth=1.0, configs=cfg, device=DEV))
    record_motion(res, "from_arm_image_keypoints/hand_rigid",
                  f(px[:, :21], params, layer, cam=cam, weights=w[:, :21], depth=depth[:, :21], wrist_pose=rows[:, 1], configs=cfg, device=DEV))
    record_motion(res, "from_arm_image_keypoints/hand_init", f(px[:, :21], params, layer, cam=cam, init=init2, configs=cfg, device=DEV))
    record_motion(res, "from_arm_image_keypoints/hand_smooth", f(px[:, :21], params, layer, cam=cam, smooth=1.0, configs=cfg, device=DEV))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    hand(res)
    arm(res)
    hand_motions(res)
    arm_motions(res)
    torch.cuda.synchronize()
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
