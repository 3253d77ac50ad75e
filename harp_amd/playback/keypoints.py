"""The host side of Motion.from_keypoints, numpy float64 and no device: the model's rest joints, the bone-length scale, the
Kabsch start of the root (T problems of six points each), and `ik_inputs`, which checks what a caller passed and returns the arrays that
ops.mano_ik is fed.  `checked` is the package's one coercion and check of a tensor or array-like that a caller passed.  The SMPL-X arm's
counterparts (Motion.from_arm_keypoints): `rest_arm_joints`, `match_arm_lengths`, `arm_palm_start`.  Image keypoints
(Motion.from_image_keypoints): `camera_tz` and `project_pixels` (the player's camera), `planar_palm_starts` (the two
starts that a plane's pixels allow) and `image_ik_inputs` for ops.mano_reproj_ik; the SMPL-X arm's (Motion.from_arm_image_keypoints,
DESIGN.md §35): `arm_image_ik_inputs` and `arm_image_starts` for ops.arm_reproj_ik.  What the Motion.from_* constructors set up
alike stands once, below `checked`: `frame_cam`, `avatar_shape`, `check_init`, `init_rows`, `held_wrist`, `arm_start_rows`,
`smoothed`."""
import numpy as np
import torch

JOINT_REORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)      # output joint -> model joint / tip (manolayer.py:279)
ARM_JOINT_IDX = (21, 52, 53, 54, 71, 40, 41, 42, 72, 43, 44, 45, 73, 49, 50, 51, 74, 46, 47, 48, 75, 19)      # the arm's output joint -> SMPL-X joint (71..75: tip vertices)
ELBOW = 21                                             # the arm's last output row; rows 0..20 are MANO's keypoint order
PALM = (0, 1, 5, 9, 13, 17)                            # output joints that only the root moves: the wrist and the five finger roots
# the 15 chain bones in output joints: wrist -> finger root and the two bones after it; the tip bones are left out (pose correctives move the tips)
CHAIN_BONES = tuple((0 if k == 0 else 4 * f + k, 4 * f + k + 1) for f in range(5) for k in range(3))


def checked(name, x, *shapes, kind=None, split=False, tensor=False):
    """A tensor or array-like -> a host array (tensor=True: a tensor instead, left on the device it is on) whose shape is one of `shapes`
    (None: any length >= 1; no shapes: any shape) and whose dtype is of `kind` ("f": floating point, "i": integers, None: any); else a
    ValueError that names the field.  split=True reports a dtype of the wrong kind as a TypeError of its own."""
    if tensor:
        a = x.detach() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        kinds = {None: True, "f": a.is_floating_point(), "i": not a.is_floating_point() and a.dtype != torch.bool}
    else:
        a = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x)
        kinds = {None: True, "f": np.issubdtype(a.dtype, np.floating), "i": a.dtype.kind in "iu"}
    ok_shape = not shapes or any(len(s) == len(a.shape) and all(d >= 1 if w is None else d == w for w, d in zip(s, a.shape)) for s in shapes)
    if ok_shape and kinds[kind]:
        return a
    want = " or ".join(str(tuple("T" if w is None else w for w in s)).replace("'", "") for s in shapes)
    if split and not ok_shape:
        raise ValueError(f"{name} must be {want}, got {tuple(a.shape)}")
    if split:
        raise TypeError(f"{name} must be floating point, got {a.dtype}")
    want = {None: want, "f": f"floating point {want}", "i": f"{want} integers"}[kind]
    raise ValueError(f"{name} must be {want}, got {tuple(a.shape)}" if kind is None else f"{name} must be {want}, got {a.dtype} {tuple(a.shape)}")


def frame_cam(cam, params, T):
    """the per-frame cam (T,3) float32 of a solved motion: `cam` (3,) or (T,3), or row 0 of the fit's when it is None"""
    return np.broadcast_to(checked("cam", params["cam"][0] if cam is None else cam, (3,), (T, 3)).astype(np.float32), (T, 3)).copy()


def avatar_shape(params):
    """the avatar's shape (10,) float64 from the fit's parameter dict: given to the solve, not solved"""
    return params["shape"].detach().cpu().numpy().astype(np.float64).reshape(10)


def check_init(init, T, wrist=False):
    """a warm start is None or anything with a length of T and rot / trans / pose rows (wrist=True: and wrist_pose), else a ValueError"""
    fields = ("rot", "trans", "pose") + ("wrist_pose",) * wrist
    if init is not None and (not all(getattr(init, k, None) is not None for k in fields) or len(init) != T):
        raise ValueError(f"init must be a Motion of {T} frames" + " with wrist_pose" * wrist)


def init_rows(init):
    """(rot (T,3), trans (T,3), pose (T,45)) of a warm start, on the host as the Motion stores them"""
    return init.rot.cpu().numpy(), init.trans.cpu().numpy(), init.pose.cpu().numpy()


def held_wrist(wrist_pose, init, T):
    """the arm's wrist (T,3) float64 that a solve holds, or the centre of its prior: wrist_pose (3,) or (T,3), else init's, else zeros"""
    if init is not None and wrist_pose is None:
        return init.wrist_pose.cpu().numpy().astype(np.float64)
    return np.broadcast_to(np.zeros(3) if wrist_pose is None else checked("wrist_pose", wrist_pose, (3,), (T, 3)).astype(np.float64), (T, 3))


def arm_start_rows(T, wrist, init=None):
    """the arm's start (in_pose (T,17,3) = [rot | wrist | pose(15)], trans (T,3)), float64: init's rot, pose and trans around `wrist`, or
    without init the model at the origin with that wrist — where the solver's own forward is evaluated for the rigid start, whose rot
    and trans the caller then writes in"""
    rows, trans = np.zeros((T, 17, 3)), np.zeros((T, 3))
    rows[:, 1] = wrist
    if init is not None:
        rows[:, 0], trans, pose = init_rows(init)
        rows[:, 2:] = pose.reshape(T, 15, 3)
    return rows, trans


def smoothed(smooth, points, w):
    """(points (T,n,3), weights (T,n) or None) after the window filter.  smooth: None (both as they came) or a function (points, weights)
    -> (points, used (T,n)); a joint it filled (used > 0) whose weight was <= 0 then counts as used, with weight 1; a joint with nothing
    in its window comes back as it went in."""
    if smooth is None:
        return points, w
    out, filled = smooth(points, w)
    return np.asarray(out, np.float64), None if w is None else np.where((np.asarray(filled) > 0) & ~(w > 0), 1.0, w)


def rest_chain_joints(model, shape):
    """the model's 21 joints in output order at `shape` BEFORE any rotation, (21,3) float64; the five tips are NaN (they depend on the
    pose).  The wrist, the finger roots relative to it, and every chain bone's length do not depend on the finger pose."""
    f64 = lambda k: np.asarray(model[k], np.float64)
    v = f64("v_template").reshape(778, 3) + f64("shapedirs").reshape(778, 3, 10) @ np.asarray(shape, np.float64).reshape(10)
    j16 = f64("J_regressor").reshape(16, 778) @ v
    out = np.full((21, 3), np.nan)
    for k, src in enumerate(JOINT_REORDER):
        if src < 16:
            out[k] = j16[src]
    return out


def rest_arm_joints(model, shape):
    """the SMPL-X arm's 22 joints in output order (the wrist, the five fingers root to tip, the elbow) at `shape` BEFORE any rotation,
    (22,3) float64; the five tips are NaN (skinned vertices: they depend on the pose).  rest_chain_joints' counterpart for the arm model's
    arrays (J_template (55,3), J_shapedirs (55,3,NB), the joint regressor already folded in): every chain bone's length and the forearm's,
    |row 21 - row 0|, do not depend on the pose."""
    f64 = lambda k: np.asarray(model[k], np.float64)
    b = np.zeros(f64("J_shapedirs").shape[-1])
    b[:10] = np.asarray(shape, np.float64).reshape(10)
    j55 = f64("J_template").reshape(-1, 3) + f64("J_shapedirs") @ b
    out = np.full((22, 3), np.nan)
    for k, src in enumerate(ARM_JOINT_IDX):
        if src < j55.shape[0]:
            out[k] = j55[src]
    return out


def match_arm_lengths(keypoints, used, rest):
    """(T,21|22,3) keypoints with someone else's proportions -> the avatar's: the 21 hand keypoints scaled about their wrist by
    bone_length_scale (the chain bones then sum to the model's), and the elbow, when the keypoints have one, put on its ray from the
    wrist at the MODEL's forearm length |rest[21] - rest[0]| — no unknown of the solve changes that length, so a forearm of another length
    could only be absorbed by trans.  rest: rest_arm_joints.  A frame without a finite wrist stays as it is; so does an elbow that is
    not finite or lies on the wrist.  Returns (keypoints, the hand's scale)."""
    kp = np.array(keypoints, np.float64)
    wrist = kp[:, :1]
    has_wrist = np.isfinite(wrist).all(-1, keepdims=True)
    scale = bone_length_scale(kp[:, :21], used[:, :21], rest[:21])
    kp[:, :21] = np.where(has_wrist, wrist + scale * (kp[:, :21] - wrist), kp[:, :21])
    if kp.shape[1] > ELBOW:
        ray = kp[:, ELBOW] - wrist[:, 0]
        with np.errstate(invalid="ignore"):
            n = np.linalg.norm(ray, axis=-1, keepdims=True)
            ok = has_wrist[:, 0] & np.isfinite(n) & (n > 0)
            kp[:, ELBOW] = np.where(ok, wrist[:, 0] + ray / np.where(ok, n, 1.0) * np.linalg.norm(rest[ELBOW] - rest[0]), kp[:, ELBOW])
    return kp, scale


def bone_length_scale(keypoints, used, rest):
    """the factor that makes the keypoints' 15 chain bones sum to the model's: the model's sum over the median over the frames (those with
    all 16 chain joints used) of the keypoints' sum; 1 when there is no such frame"""
    a, b = np.array([i for i, _ in CHAIN_BONES]), np.array([j for _, j in CHAIN_BONES])
    model_sum = np.linalg.norm(rest[b] - rest[a], axis=-1).sum()
    ok = used[:, np.unique(np.concatenate([a, b]))].all(1)
    if not ok.any():
        return 1.0
    kp = keypoints[ok]
    return float(model_sum / np.median(np.linalg.norm(kp[:, b] - kp[:, a], axis=-1).sum(1)))


def kabsch_rotation(P, Q):
    """the rotation R (det +1) that minimises sum |R p_i - q_i|^2 over two CENTRED point sets (n,3); a mirrored set gets the best proper
    rotation, not the reflection"""
    U, _, Vt = np.linalg.svd(np.asarray(Q, np.float64).T @ np.asarray(P, np.float64))
    d = np.sign(np.linalg.det(U @ Vt)) or 1.0
    return U @ np.diag([1.0, 1.0, d]) @ Vt


def axis_angle_of(R):
    """rotation matrix -> axis-angle with an angle in [0, pi], through the quaternion with the largest component (stable near pi)"""
    t = np.trace(R)
    cand = np.array([1.0 + t, 1.0 + 2 * R[0, 0] - t, 1.0 + 2 * R[1, 1] - t, 1.0 + 2 * R[2, 2] - t])
    i = int(np.argmax(cand))
    if i == 0:
        q = np.array([cand[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif i == 1:
        q = np.array([R[2, 1] - R[1, 2], cand[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif i == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], cand[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], cand[3]])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    vn = np.linalg.norm(q[1:])
    return np.zeros(3) if vn < 1e-15 else 2.0 * np.arctan2(vn, q[0]) * q[1:] / vn


def palm_start(keypoints, used, rest):
    """rot (T,3), trans (T,3) float64 that put the model's six palm joints (PALM, which only the root rotation and trans move:
    R (J_k - J_0) + J_0 + trans) onto the keypoints' in the least-squares sense: the Kabsch rotation, then the difference of the two
    centroids.  A frame whose six palm joints are not all used keeps the rotation of the last frame that had them (none yet: zero) and
    takes its trans from the palm joints it has (none: that frame's trans as well)."""
    T = keypoints.shape[0]
    idx = np.array(PALM)
    P0 = rest[idx] - rest[0]                            # about the wrist, where the model rotates
    rot, trans = np.zeros((T, 3)), np.zeros((T, 3))
    R, aa, tr = np.eye(3), np.zeros(3), np.zeros(3)
    for t in range(T):
        u = used[t, idx]
        if u.all():
            Q = keypoints[t, idx]
            R = kabsch_rotation(P0 - P0.mean(0), Q - Q.mean(0))
            aa = axis_angle_of(R)
        if u.any():
            tr = keypoints[t, idx[u]].mean(0) - (P0[u] @ R.T + rest[0]).mean(0)
        rot[t], trans[t] = aa, tr
    return rot, trans


def ik_inputs(keypoints, weights, cam, init, params, model, match_bone_lengths=True, smooth=None):
    """What Motion.from_keypoints passes to ops.mano_ik, checked and prepared on the host: dict(shape (10,), keypoints (T,21,3), pose48
    (T,48) = [rot | pose], trans (T,3), weights (T,21) or None, cam (T,3) float32), the others float64.  keypoints, weights, cam, init,
    params, match_bone_lengths: as Motion.from_keypoints takes them (init: anything with a length and rot / trans / pose rows); model: the
    hand layer's numpy model.  smooth: None or a function (keypoints, weights) -> (keypoints, used (T,21)) that filters the checked
    keypoints before the bone-length scale; a joint it filled (used > 0) then counts as used."""
    kp = checked("keypoints", keypoints, (None, 21, 3), kind="f", split=True).astype(np.float64)
    T = kp.shape[0]
    w = None if weights is None else checked("weights", weights, (T, 21), kind="f", split=True).astype(np.float64)
    check_init(init, T)
    kp, w = smoothed(smooth, kp, w)
    cam, shape = frame_cam(cam, params, T), avatar_shape(params)
    used = np.isfinite(kp).all(-1) & (True if w is None else (w > 0))
    rest = rest_chain_joints(model, shape)
    if match_bone_lengths:
        wrist = kp[:, :1]                               # (no wrist: the frame stays as it is)
        kp = np.where(np.isfinite(wrist).all(-1, keepdims=True), wrist + bone_length_scale(kp, used, rest) * (kp - wrist), kp)
    if init is None:
        (rot, trans), pose = palm_start(kp, used, rest), np.zeros((T, 45))
    else:
        rot, trans, pose = init_rows(init)
    return dict(shape=shape, keypoints=kp, pose48=np.concatenate([rot, pose], 1), trans=trans, weights=w, cam=cam)


def vertex_start(targets, used, rest_vertices, root_joint):
    """The rigid start of the vertex fit (Motion.from_vertices, optimize_for_mano_param(method="lm")): rot (T,3) axis-angle and
    trans (T,3), float64, that put the model's vertices at zero stored pose onto the targets in the weighted least-squares sense — ONE
    batched SVD, no loop over the frames.  targets (T,778,3); used (T,778) bool or non-negative weights (a vertex with a non-finite target
    is unused whatever it says); rest_vertices (778,3) or (T,778,3): the model's vertices at the frame's shape with zero stored pose and
    zero trans; root_joint (3,) or (T,3): its root joint, about which the model rotates, so that trans = t - (J_0 - R J_0) for the Kabsch
    fit x -> R x + t.  R has determinant +1 (a mirrored target gets the best proper rotation) and its logarithm is taken through the
    quaternion's largest component, which stays finite and right at angles near pi.  A frame that cannot be aligned (fewer than three used
    vertices) takes the start of the last frame before it that could (none yet: zeros)."""
    tg = np.asarray(targets, np.float64)
    T = tg.shape[0]
    P = np.broadcast_to(np.asarray(rest_vertices, np.float64), tg.shape)
    J0 = np.broadcast_to(np.asarray(root_joint, np.float64), (T, 3))
    fin = np.isfinite(tg).all(-1)
    w = np.where(fin, np.asarray(used, np.float64), 0.0)
    w = np.where(w > 0, w, 0.0)                            # (a NaN weight is no weight)
    ok = (w > 0).sum(1) >= 3
    tg = np.where(fin[..., None], tg, 0.0)
    n = np.where(ok, w.sum(1), 1.0)[:, None]
    pc, tc = (w[..., None] * P).sum(1) / n, (w[..., None] * tg).sum(1) / n
    H = np.einsum("tv,tvi,tvj->tij", w, tg - tc[:, None], P - pc[:, None])
    H = np.where(ok[:, None, None], H, np.eye(3))
    U, _, Vt = np.linalg.svd(H)
    d = np.where(np.linalg.det(U @ Vt) < 0, -1.0, 1.0)
    R = (U * np.stack([np.ones(T), np.ones(T), d], 1)[:, None, :]) @ Vt
    # the logarithm: the quaternion from its largest component
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    cand = np.stack([1.0 + tr, 1.0 + 2 * R[:, 0, 0] - tr, 1.0 + 2 * R[:, 1, 1] - tr, 1.0 + 2 * R[:, 2, 2] - tr], 1)
    a, b, c = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]
    e, f, g = R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1]
    variants = np.stack([np.stack([cand[:, 0], a, b, c], 1), np.stack([a, cand[:, 1], e, f], 1),
                         np.stack([b, e, cand[:, 2], g], 1), np.stack([c, f, g, cand[:, 3]], 1)], 1)          # (T, 4 variants, 4)
    q = np.take_along_axis(variants, np.argmax(cand, 1)[:, None, None], 1)[:, 0] if T else np.zeros((0, 4))
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    q = np.where(q[:, :1] < 0, -q, q)
    vn = np.linalg.norm(q[:, 1:], axis=1, keepdims=True)
    rot = np.where(vn < 1e-15, 0.0, 2.0 * np.arctan2(vn, q[:, :1]) * q[:, 1:] / np.where(vn < 1e-15, 1.0, vn))
    trans = tc - np.einsum("tij,tj->ti", R, pc) - (J0 - np.einsum("tij,tj->ti", R, J0))
    # a frame that cannot be aligned: the last one before it that could
    src = np.maximum.accumulate(np.where(ok, np.arange(T), -1))
    take = np.maximum(src, 0)
    none = (src < 0)[:, None]
    return np.where(none, 0.0, rot[take]), np.where(none, 0.0, trans[take])


def arm_palm_start(keypoints, used, joints0):
    """The rigid start of the arm's keypoint solve (Motion.from_arm_keypoints): rot (T,3) axis-angle and trans (T,3), float64,
    one batched SVD (vertex_start), no loop over the frames.  keypoints (T,21|22,3); used (T,21|22) bool or non-negative weights; joints0
    (22,3) or (T,22,3): the model's output joints in metres at the avatar's shape, the held (or prior) wrist, zero finger pose, zero root
    and zero trans — the solver's own forward.  Their palm rows (PALM) and the elbow move rigidly under the root, about the origin (the
    model is wrist-centred: trans is the wrist), so the Kabsch fit over those six points, and the elbow where the keypoints have one and
    it is used, is the start.  A frame that cannot be aligned takes the last one that could."""
    kp = np.asarray(keypoints, np.float64)
    idx = np.array(PALM + ((ELBOW,) if kp.shape[1] > ELBOW else ()))
    j0 = np.asarray(joints0, np.float64)
    return vertex_start(kp[:, idx], np.asarray(used)[:, idx], j0[..., idx, :], np.zeros(3))


def camera_tz(cam, focal, S):
    """the camera's depth of the world origin, 2 focal / (S cam0 + 1e-9) (utils/visualize.py:268), for cam (..., 3)"""
    return 2.0 * focal / (S * np.asarray(cam, np.float64)[..., 0] + 1e-9)


def project_pixels(joints, cam, focal, S):
    """joints (..., n, 3) metres in the frame of the fit's `joints` — the hand's 21 rows, or the SMPL-X arm's 22 with the elbow as row 21 —
    -> (..., n, 3) = (u, v, d) as csrc/reproj_ik.hip and csrc/arm_reproj_ik.hip state them: the player's camera (view = (-x - cam1,
    -y - cam2, z + t_z)) read at the rasteriser's pixel centres, so that the centre of column i is at u = i + 0.5 and of row i at
    v = i + 0.5, and the depth relative to the wrist (row 0).  cam (3,) or (..., 3).  numpy float64."""
    j = np.asarray(joints, np.float64)
    cam = np.asarray(cam, np.float64)
    Z = j[..., 2] + camera_tz(cam, focal, S)[..., None]
    u = S / 2.0 + focal * (j[..., 0] + cam[..., 1, None]) / Z
    v = S / 2.0 + focal * (j[..., 1] + cam[..., 2, None]) / Z
    return np.stack([u, v, j[..., 2] - j[..., :1, 2]], -1)


def planar_palm_starts(pixels, used, rest_joints, cam, focal, S):
    """The two starts of the reprojection solve (Motion.from_image_keypoints) from the six palm pixels alone, host float64:
    (rot (T,2,3) axis-angle, trans (T,2,3), depth (T,) = the palm centroid's distance along the view axis, metres).  pixels (T,21,2); used
    (T,21) bool; rest_joints: rest_chain_joints; cam (3,) or (T,3).  The palm joints (PALM) move rigidly, R (J_k - J_0) + J_0 + trans, and
    lie close to a plane, so under weak perspective their centred pixels are a 2 x 2 affine map A of their in-plane coordinates:
    A = s B with s = sigma_1(A) = focal / Z and B the top 2 x 2 block of the rotated plane basis.  The basis' third row is
    +-sqrt(lambda_max) v of I - B^T B: the two signs are the two poses (mirrored in depth) that the pixels of a plane cannot tell apart.
    Each is re-orthonormalised, completed by the cross product and turned into an axis-angle (axis_angle_of); trans puts the palm
    centroid on its pixel at depth Z — the root rotation turns about the wrist joint, not the origin.  A frame whose six palm pixels are
    not all used takes the starts of the last frame that had them (none yet: no rotation, trans zero)."""
    px = np.asarray(pixels, np.float64)
    T = px.shape[0]
    idx = np.array(PALM)
    cam = np.broadcast_to(np.asarray(cam, np.float64), (T, 3))
    tz = camera_tz(cam, focal, S)
    r0, rbar = rest_joints[0], rest_joints[idx].mean(0)
    q = rest_joints[idx] - rbar
    _, _, Vt = np.linalg.svd(q, full_matrices=False)                # the palm's best plane: its two widest directions and the normal
    e1, e2 = Vt[0], Vt[1]
    E = np.stack([e1, e2, np.cross(e1, e2)], 1)                     # (3,3), columns: a right-handed basis
    c = q @ E[:, :2]                                                # (6,2) in-plane coordinates
    pinv = np.linalg.pinv(c)                                        # (2,6)
    rot, trans, depth = np.zeros((T, 2, 3)), np.zeros((T, 2, 3)), np.zeros(T)
    cur = (np.zeros((2, 3)), np.zeros((2, 3)), None)
    for t in range(T):
        if np.asarray(used)[t, idx].all():
            p = px[t, idx]
            pbar = p.mean(0)
            A = (pinv @ (p - pbar)).T                               # (2,2): p - pbar ~ c A^T
            s = np.linalg.svd(A, compute_uv=False)[0]
            if s > 0 and np.isfinite(s):
                B = A / s
                lam, V = np.linalg.eigh(np.eye(2) - B.T @ B)
                m = np.sqrt(max(lam[1], 0.0)) * V[:, 1]
                Z = focal / s
                pc = np.array([(pbar[0] - S / 2.0) * Z / focal - cam[t, 1], (pbar[1] - S / 2.0) * Z / focal - cam[t, 2], Z - tz[t]])
                rots, trs = [], []
                for sign in (1.0, -1.0):
                    c1, c2 = np.append(B[:, 0], sign * m[0]), np.append(B[:, 1], sign * m[1])
                    c1 = c1 / np.linalg.norm(c1)
                    c2 = c2 - (c1 @ c2) * c1
                    c2 = c2 / np.linalg.norm(c2)
                    R = np.stack([c1, c2, np.cross(c1, c2)], 1) @ E.T
                    rots.append(axis_angle_of(R))
                    trs.append(pc - R @ (rbar - r0) - r0)
                cur = (np.array(rots), np.array(trs), Z)
        rot[t], trans[t] = cur[0], cur[1]
        depth[t] = tz[t] if cur[2] is None else cur[2]
    return rot, trans, depth


def image_ik_inputs(keypoints, weights, depth, cam, init, params, model, focal, S, smooth=None):
    """What Motion.from_image_keypoints passes to ops.mano_reproj_ik, checked and prepared on the host: dict(shape (10,), targets (T,21,3)
    = (u, v, d) with NaN where there is no depth, weights (T,21) or None, pose48 (T,C,48), trans (T,C,3) for C candidate starts (2: the
    planar starts; 1: init), depth (T,) = the start's palm depth, cam (T,3) float32), the others float64.  smooth: None or a function
    (points (T,21,3), weights) -> (points, used (T,21)), which the pixels (as (u, v, 0)) and the depths (as (d, 0, 0)) go through; a joint
    it filled then counts as used."""
    kp = checked("keypoints", keypoints, (None, 21, 2), kind="f", split=True).astype(np.float64)
    T = kp.shape[0]
    w = None if weights is None else checked("weights", weights, (T, 21), kind="f", split=True).astype(np.float64)
    d = None if depth is None else checked("depth", depth, (T, 21), kind="f", split=True).astype(np.float64)
    check_init(init, T)
    if smooth is not None:
        p3, w = smoothed(smooth, np.concatenate([kp, np.zeros((T, 21, 1))], -1), w)
        kp = p3[..., :2]
        if d is not None:
            d = smoothed(smooth, np.concatenate([d[..., None], np.zeros((T, 21, 2))], -1), None)[0][..., 0]
    cam, shape = frame_cam(cam, params, T), avatar_shape(params)
    used = np.isfinite(kp).all(-1) & (True if w is None else (w > 0))
    rest = rest_chain_joints(model, shape)
    rot, trans, zbar = planar_palm_starts(kp, used, rest, cam, focal, S)
    if init is None:
        pose48 = np.concatenate([rot, np.zeros((T, 2, 45))], -1)
    else:
        rot, trans, pose = init_rows(init)
        pose48, trans = np.concatenate([rot, pose], 1).astype(np.float64)[:, None], trans.astype(np.float64)[:, None]
        palm = np.array(PALM)
        # the warm start's own palm depth: the palm joints are rigid under the root rotation
        for t in range(T):
            R = _rotation_of(pose48[t, 0, :3])
            zbar[t] = ((rest[palm] - rest[0]) @ R.T + rest[0] + trans[t, 0]).mean(0)[2] + camera_tz(cam[t], focal, S)
    targets = np.concatenate([kp, np.full((T, 21, 1), np.nan) if d is None else d[..., None]], -1)
    return dict(shape=shape, targets=targets, weights=w, pose48=pose48, trans=trans, depth=zbar, cam=cam)


def arm_image_ik_inputs(keypoints, weights, depth, cam, init, wrist_pose, params, smooth=None):
    """What Motion.from_arm_image_keypoints passes to ops.arm_reproj_ik before the start is known, checked and prepared on the host:
    dict(shape (10,), targets (T,22,3) = (u, v, d) with NaN where there is no pixel or depth, weights (T,22) (0 for an unused joint),
    wrist (T,3) = what the wrist is held at or the centre of its prior, solve_wrist, in_pose (T,17,3) and trans (T,3) = the point at which
    the solver's own forward gives the joints for the rigid start (init's rows with init), cam (T,3) float32), the others float64.
    keypoints (T,22,2) with the elbow as row 21: the wrist is solved; (T,21,2): the same 22-wide problem with the elbow unused and the
    wrist held.  depth None or of the keypoints' width.  smooth: None or a function (points (T,22,3), weights) -> (points, used (T,22)),
    which the pixels (as (u, v, 0)) and the depths (as (d, 0, 0)) go through; a joint it filled then counts as used."""
    n = int(np.shape(keypoints)[1]) if np.ndim(keypoints) == 3 else -1
    if n not in (21, 22):
        raise ValueError(f"keypoints must be (T, 22, 2) with the elbow or (T, 21, 2) without, got {tuple(np.shape(keypoints))}")
    kp = checked("keypoints", keypoints, (None, n, 2), kind="f", split=True).astype(np.float64)
    T = kp.shape[0]
    w = None if weights is None else checked("weights", weights, (T, n), kind="f", split=True).astype(np.float64)
    d = None if depth is None else checked("depth", depth, (T, n), kind="f", split=True).astype(np.float64)
    check_init(init, T, wrist=True)
    if n == 21:                                             # the hand alone: the elbow's row is there and unused
        kp = np.concatenate([kp, np.full((T, 1, 2), np.nan)], 1)
        w = np.concatenate([np.ones((T, 21)) if w is None else w, np.zeros((T, 1))], 1)
        d = None if d is None else np.concatenate([d, np.full((T, 1), np.nan)], 1)
    if smooth is not None:
        p3, w = smoothed(smooth, np.concatenate([kp, np.zeros((T, 22, 1))], -1), w)
        kp = p3[..., :2]
        if d is not None:
            d = smoothed(smooth, np.concatenate([d[..., None], np.zeros((T, 22, 2))], -1), None)[0][..., 0]
        if n == 21:
            kp[:, ELBOW], w[:, ELBOW] = np.nan, 0.0
    cam, shape = frame_cam(cam, params, T), avatar_shape(params)
    used = np.isfinite(kp).all(-1) & (True if w is None else (w > 0))
    wt = used.astype(np.float64) if w is None else np.where(used, w, 0.0)
    wrist = held_wrist(wrist_pose, init, T)
    # (a solved wrist starts where init has it, whatever the centre of its prior)
    rows, trans = arm_start_rows(T, wrist if init is None or n == 21 else init.wrist_pose.cpu().numpy(), init)
    targets = np.concatenate([kp, np.full((T, 22, 1), np.nan) if d is None else d[..., None]], -1)
    return dict(shape=shape, targets=targets, weights=wt, wrist=np.array(wrist), solve_wrist=n == 22, in_pose=rows,
                trans=np.asarray(trans, np.float64), cam=cam)


def arm_image_starts(a, joints0, init, focal, S):
    """The candidate starts of the arm's reprojection solve: (in_pose (T,C,17,3), trans (T,C,3), depth (T,) = the start's palm depth along
    the view axis), float64.  a: arm_image_ik_inputs' dict; joints0 (T,22,3) metres: the solver's own joints at a's in_pose / trans.
    Without init C = 2: rows 0..20 of joints0 (the avatar's shape, the held or prior wrist, zero pose, zero root and trans; row 0 is the
    origin: the arm is wrist-centred) go to planar_palm_starts unchanged, frame by frame where the wrist differs between frames.  With
    init C = 1: its rows, and the depth of its own palm."""
    T = a["in_pose"].shape[0]
    j0 = np.asarray(joints0, np.float64)
    cam = a["cam"].astype(np.float64)
    if init is not None:
        depth = j0[:, np.array(PALM), 2].mean(1) + camera_tz(cam, focal, S)
        return a["in_pose"][:, None].copy(), a["trans"][:, None].copy(), depth
    px, used = a["targets"][:, :21, :2], a["weights"][:, :21] > 0
    if np.all(j0 == j0[:1]):
        rot, trans, depth = planar_palm_starts(px, used, j0[0, :21], cam, focal, S)
    else:
        rot, trans, depth = np.zeros((T, 2, 3)), np.zeros((T, 2, 3)), camera_tz(cam, focal, S)
        for t in range(T):                                  # (a frame without its six palm pixels: the starts of the last that had them)
            if used[t, np.array(PALM)].all():
                r, tr, z = planar_palm_starts(px[t:t + 1], used[t:t + 1], j0[t, :21], cam[t:t + 1], focal, S)
                rot[t], trans[t], depth[t] = r[0], tr[0], z[0]
            elif t > 0:
                rot[t], trans[t], depth[t] = rot[t - 1], trans[t - 1], depth[t - 1]
    in_pose = np.repeat(a["in_pose"][:, None], 2, axis=1)
    in_pose[:, :, 0] = rot
    return in_pose, trans, depth


def _rotation_of(aa):
    """axis-angle -> rotation matrix (Rodrigues), float64"""
    aa = np.asarray(aa, np.float64)
    th = np.linalg.norm(aa)
    if th < 1e-300:
        return np.eye(3)
    k = aa / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
