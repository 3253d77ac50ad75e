"""Playback of a fitted avatar: drive it with a motion it was not fitted on, at an output frame rate of the caller's choice, and composite
it over a video or a plain background as finished 8-bit frames.  Stands in for the reference's `change_pose`
(utils/visualize.py:111-143) and the render calls of :258-320 followed by the host-side `(img * 255).astype(np.uint8)`.

`Motion` holds the per-frame rows of a motion, `Motion.resample` retimes them on the device (ops.motion_resample), and `AvatarPlayer` is
the forward-only renderer: the fit's own fused front, rasterisers and shader (csrc/hand_front.hip, arm_front.hip, raster.hip, shade.hip)
without a backward, a gradient slab, Adam moments or targets, followed by harp_resolve_u8 — six calls of the C ABI per batch of frames, in
order on one stream, captured into a graph.

`ScenePlayer` shows several such avatars in one frame: each player's launches up to the shader, then ONE harp_composite_layers_u8
(csrc/composite.hip) that picks the nearest avatar per sub-sample, un-mirrors a flipped one (a left hand is a right-hand fit
of mirrored frames) and tests against an optional scene depth.

    python -m harp_amd.playback --config CFG (--motion MOTION.npz | --keypoints KP.npz) --out DIR [--fps-scale X] [--ss 2] [--background DIR] [--alpha]
                                [--flip] [--also CFG:MOTION[:flip]]... [--scene-depth DIR] [--masks]
                                [--smooth SIGMA [--smooth-trim RAD]] [--smooth-keypoints SIGMA]

`Motion.smooth` and `smooth_keypoints` take the jitter out of a motion or of the keypoints it is solved from (ops.motion_filter,
csrc/filter.hip): a confidence-weighted window filter that averages rotations on the manifold; `motion_jitter` measures it.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, ops

BG_WHITE = (1.0, 1.0, 1.0)                             # the reference's BlendParams background (renderer_helper.py:49)


def _rows_f32(name, a, width, T=None):
    t = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to(torch.float32)
    if t.dim() != 2 or t.shape[1] != width or (T is not None and t.shape[0] != T) or t.shape[0] < 1:
        raise ValueError(f"{name} must be ({'T' if T is None else T}, {width}), got {tuple(t.shape)}")
    return t.contiguous()


class Motion:
    """The per-frame rows that animate an avatar: pose (T,45) MANO finger joints (relative to the model's pose mean, as the fit stores them),
    rot, trans, cam (T,3), and optionally wrist_pose (T,3) (the arm model's wrist) and light_positions (T,3) (a light that moves with the
    motion; without it the player keeps the fit's light).  float32 tensors, on any device."""

    FIELDS = ("pose", "rot", "trans", "cam", "wrist_pose", "light_positions")

    def __init__(self, pose, rot, trans, cam, wrist_pose=None, light_positions=None):
        self.pose = _rows_f32("pose", pose, 45)
        T = self.pose.shape[0]
        self.rot, self.trans, self.cam = _rows_f32("rot", rot, 3, T), _rows_f32("trans", trans, 3, T), _rows_f32("cam", cam, 3, T)
        self.wrist_pose = None if wrist_pose is None else _rows_f32("wrist_pose", wrist_pose, 3, T)
        self.light_positions = None if light_positions is None else _rows_f32("light_positions", light_positions, 3, T)

    def __len__(self):
        return self.pose.shape[0]

    @classmethod
    def from_params(cls, params, rows=None, per_frame_light=False):
        """The fit's own frames (all of them, or `rows` of its tables, in that order): the replay case.  The motion carries no light
        unless per_frame_light=True: a fit with share_light_position (the default) reads and updates row 0 of its light table only, the
        other rows keep their initial value, and the player then uses that row 0 for every frame as the fit did.  Pass
        per_frame_light=True for a fit with share_light_position=False: its rows are the frames' lights."""
        idx = None if rows is None else torch.as_tensor(rows).long().reshape(-1)
        take = lambda k: None if params.get(k) is None else (params[k].detach() if idx is None else params[k].detach()[idx.to(params[k].device)]).clone()
        return cls(take("pose"), take("rot"), take("trans"), take("cam"), take("wrist_pose"), take("light_positions") if per_frame_light else None)

    @classmethod
    def from_keypoints(cls, keypoints, params, hand_layer, cam=None, weights=None, match_bone_lengths=True, iters=15, prior_weight=1e-5,
                       init=None, device=None, smooth=None):
        """A motion from 3-D keypoints (a hand tracker, a mocap glove, a dataset) by batched inverse kinematics on the device
        (ops.mano_ik, csrc/ik.hip).  keypoints (T,21,3) in metres, in the model's order — wrist, then thumb, index, middle,
        ring and little, each from root to tip — and in the frame of the fit's `joints`; a joint with a non-finite coordinate or a weight
        <= 0 (weights (T,21), default ones) is ignored.  params: the fit's parameter dict (its `shape` is the avatar's and is not solved;
        row 0 of its `cam` is the default cam); cam: (3,) or (T,3).
        The start (host, float64): pose zero, the root rotation and trans from the Kabsch fit of the model's palm joints (palm_start);
        init= takes a Motion of equal length instead as a warm start.  match_bone_lengths scales the keypoints about their wrist so that
        their chain bones sum to the model's (bone_length_scale): someone else's hand can drive the avatar.  prior_weight pulls the
        finger pose to the model's mean pose, which decides what the keypoints leave open (the twist of a finger's last bone).
        Every frame is solved on its own.  smooth: None, or the sigma in frames of a Gaussian window that the keypoints go through first
        (smooth_keypoints, with `weights` as the confidences, before the bone-length scale): jitter is taken out and a joint that a
        tracker dropped for a few frames is filled from its neighbours and then counts as used; Motion.smooth filters the solved rows
        instead.  None leaves the keypoints as they came.
        The result carries no light: AvatarPlayer.load_motion then uses the fit's row 0.  device: where the solve runs (default: the
        device of params["shape"] when that is a HIP device, else "cuda").  The SMPL-X arm needs a solver for its kinematic tree and raises
        NotImplementedError."""
        if "pose_mean" in hand_layer._model_np:
            raise NotImplementedError("Motion.from_keypoints solves the MANO hand; the SMPL-X arm needs a kinematic-tree solver")
        kp = np.asarray(keypoints.detach().cpu() if torch.is_tensor(keypoints) else keypoints)
        if kp.ndim != 3 or kp.shape[1:] != (21, 3) or kp.shape[0] < 1:
            raise ValueError(f"keypoints must be (T, 21, 3), got {kp.shape}")
        if not np.issubdtype(kp.dtype, np.floating):
            raise TypeError(f"keypoints must be floating point, got {kp.dtype}")
        kp = kp.astype(np.float64)
        T = kp.shape[0]
        w = None
        if weights is not None:
            w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights)
            if w.shape != (T, 21):
                raise ValueError(f"weights must be ({T}, 21), got {w.shape}")
            if not np.issubdtype(w.dtype, np.floating):
                raise TypeError(f"weights must be floating point, got {w.dtype}")
            w = w.astype(np.float64)
        if init is not None and (not isinstance(init, Motion) or len(init) != T):
            raise ValueError(f"init must be a Motion of {T} frames")
        dev = torch.device(device if device is not None else (params["shape"].device if params["shape"].is_cuda else "cuda"))
        if smooth is not None:
            kp_s, filled = smooth_keypoints(kp, weights=w, sigma=smooth, device=dev)
            kp = kp_s.cpu().numpy().astype(np.float64)                           # (a joint with nothing in its window comes back as it went in)
            w = None if w is None else np.where((filled.cpu().numpy() > 0) & ~(w > 0), 1.0, w)      # a filled joint counts as used
        cam = params["cam"][0] if cam is None else cam
        cam = np.asarray(cam.detach().cpu() if torch.is_tensor(cam) else cam, dtype=np.float32)
        if cam.shape not in ((3,), (T, 3)):
            raise ValueError(f"cam must be (3,) or ({T}, 3), got {cam.shape}")
        cam = np.broadcast_to(cam, (T, 3)).copy()
        shape = params["shape"].detach().cpu().numpy().astype(np.float64).reshape(10)
        used = np.isfinite(kp).all(-1) & (True if w is None else (w > 0))
        rest = rest_chain_joints(hand_layer._model_np, shape)
        if match_bone_lengths:
            s = bone_length_scale(kp, used, rest)
            wrist = kp[:, :1]
            kp = np.where(np.isfinite(wrist).all(-1, keepdims=True), wrist + s * (kp - wrist), kp)      # (no wrist: the frame stays as it is)
        if init is None:
            rot, trans = palm_start(kp, used, rest)
            pose = np.zeros((T, 45))
        else:
            rot, trans, pose = init.rot.cpu().numpy(), init.trans.cpu().numpy(), init.pose.cpu().numpy()
        from .manopth.manolayer import ManoDeviceModel
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        dm = ManoDeviceModel(hand_layer._model_np, dev)
        res = ops.mano_ik(dm, up(shape), up(kp), up(np.concatenate([rot, pose], 1)), up(trans), weights=None if w is None else up(w),
                          iters=iters, prior_weight=prior_weight)
        return cls(res.pose48[:, 3:], res.pose48[:, :3], res.trans, cam)

    def save(self, path):
        np.savez(path, **{k: getattr(self, k).cpu().numpy() for k in self.FIELDS if getattr(self, k) is not None})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(**{k: z[k] for k in cls.FIELDS if k in z.files})

    def resample(self, times, hand_layer, device="cuda"):
        """The motion at `times` (n,) in units of its own frames, e.g. np.linspace(0, T - 1, n) to retime it to n frames: rotations along
        the shortest arc with the model's pose mean as the offset, trans / cam / light linearly (ops.motion_resample); a time on a frame
        returns that frame bit for bit."""
        dev = torch.device(device)
        rots = [self.rot] + ([self.wrist_pose] if self.wrist_pose is not None else []) + [self.pose]
        lins = [self.trans, self.cam] + ([self.light_positions] if self.light_positions is not None else [])
        keys = torch.cat([t.to(dev) for t in rots + lins], 1).contiguous()
        n_rot = 16 + (self.wrist_pose is not None)
        off = torch.as_tensor(pose_mean_rows(hand_layer, self.wrist_pose is not None), dtype=torch.float32).to(dev)
        t = torch.as_tensor(np.asarray(times, dtype=np.float32)).reshape(-1).to(dev)
        out = ops.motion_resample(keys, t, n_rot, off)
        c = iter(out.split([3] + ([3] if self.wrist_pose is not None else []) + [45, 3, 3] + ([3] if self.light_positions is not None else []), 1))
        rot = next(c)
        wrist = next(c) if self.wrist_pose is not None else None
        pose, trans, cam = next(c), next(c), next(c)
        light = next(c) if self.light_positions is not None else None
        return Motion(pose, rot, trans, cam, wrist, light)

    def smooth(self, hand_layer, sigma=2.0, radius=None, weights=None, segments=None, trim_rot=None, trim_vec=None, iters=2, fields=None,
               device="cuda"):
        """The motion with its jitter taken out by a Gaussian window of `sigma` frames (radius: ceil(3 sigma)) on the device
        (ops.motion_filter), as a new Motion of equal length.  rot, wrist_pose and pose are filtered as ROTATIONS (the
        weighted geodesic mean of the window, `iters` iterations) with the model's pose mean as the offset, exactly as `resample` assembles
        them; trans and light_positions as 3-vectors; cam as three scalars — cam[0] is an inverse depth and is averaged as stored.
        weights: None or (T,) confidences per frame (<= 0 or not finite: the frame is not used and is filled from its neighbours).
        segments: None or (T,) integer clip ids; a window never crosses a change, and it shrinks symmetrically there and at the ends.
        trim_rot (radians) / trim_vec (the unit of trans): a sample farther than that from the window's first estimate is left out of a
        second one — a one-frame spike does not leak into its neighbours.  fields: the names to filter (default: all the motion has);
        the others pass through bit for bit."""
        names = [k for k in self.FIELDS if getattr(self, k) is not None]
        fields = names if fields is None else list(fields)
        if any(k not in names for k in fields):
            raise ValueError(f"fields must be among {names}, got {fields}")
        dev = torch.device(device)
        T, wrist, light = len(self), self.wrist_pose is not None, self.light_positions is not None
        rots = [self.rot] + ([self.wrist_pose] if wrist else []) + [self.pose]
        vecs = [self.trans] + ([self.light_positions] if light else [])
        rows = torch.cat([t.to(dev) for t in rots + vecs + [self.cam]], 1).contiguous()
        n_rot, n_vec = 16 + wrist, 1 + light
        off = torch.as_tensor(pose_mean_rows(hand_layer, wrist), dtype=torch.float32).to(dev)
        trim = None
        if trim_rot is not None or trim_vec is not None:
            trim = torch.tensor([float(trim_rot or 0.0)] * n_rot + [float(trim_vec or 0.0)] * n_vec + [0.0] * 3, dtype=torch.float32).to(dev)
        w = None
        if weights is not None:
            w = torch.as_tensor(np.asarray(weights) if not torch.is_tensor(weights) else weights).detach().to(torch.float32)
            if tuple(w.shape) != (T,):
                raise ValueError(f"weights must be ({T},), got {tuple(w.shape)}")
            w = w.contiguous().to(dev)
        seg = None if segments is None else _segment_ids(segments, T).to(dev)
        out, _ = ops.motion_filter(rows, n_rot, n_vec, ops.gaussian_taps(sigma, radius), weights=w, segment=seg, trim=trim, rot_offset=off, iters=iters)
        c = iter(out.split([3] + ([3] if wrist else []) + [45, 3] + ([3] if light else []) + [3], 1))
        got = dict(rot=next(c))
        if wrist:
            got["wrist_pose"] = next(c)
        got["pose"], got["trans"] = next(c), next(c)
        if light:
            got["light_positions"] = next(c)
        got["cam"] = next(c)
        pick = lambda k: None if getattr(self, k) is None else (got[k] if k in fields else getattr(self, k).clone())      # noqa: E731
        return Motion(pick("pose"), pick("rot"), pick("trans"), pick("cam"), pick("wrist_pose"), pick("light_positions"))


def _segment_ids(segments, T):
    s = torch.as_tensor(np.asarray(segments.cpu() if torch.is_tensor(segments) else segments))
    if s.dim() != 1 or s.shape[0] != T or s.is_floating_point() or s.dtype == torch.bool:
        raise ValueError(f"segments must be ({T},) integers, got {s.dtype} {tuple(s.shape)}")
    return s.to(torch.int32).contiguous()


def smooth_keypoints(keypoints, weights=None, sigma=2.0, radius=None, trim=None, segments=None, device="cuda"):
    """(T,21,3) keypoints through the window filter as 21 vector channels (ops.motion_filter) -> (keypoints (T,21,3) float32,
    used (T,21) int32), both on `device`.  weights: None or (T,21) confidences.  A joint with a non-finite coordinate or a weight <= 0 has
    weight 0: it does not pull on its neighbours and is FILLED from them when any lie in the window (used > 0); with none it comes back as
    it went in (used == 0).  trim: None or a distance in the keypoints' unit for the trimmed second pass; segments: as Motion.smooth."""
    kp = torch.as_tensor(np.asarray(keypoints) if not torch.is_tensor(keypoints) else keypoints).detach()
    if kp.dim() != 3 or tuple(kp.shape[1:]) != (21, 3) or kp.shape[0] < 1 or not kp.is_floating_point():
        raise ValueError(f"keypoints must be floating point (T, 21, 3), got {kp.dtype} {tuple(kp.shape)}")
    T = kp.shape[0]
    dev = torch.device(device)
    kp = kp.to(torch.float32)
    ok = torch.isfinite(kp).all(-1)
    if weights is None:
        w = ok.to(torch.float32)
    else:
        w = torch.as_tensor(np.asarray(weights) if not torch.is_tensor(weights) else weights).detach()
        if tuple(w.shape) != (T, 21) or not w.is_floating_point():
            raise ValueError(f"weights must be floating point ({T}, 21), got {w.dtype} {tuple(w.shape)}")
        w = w.to(torch.float32).to(kp.device)
        w = torch.where(ok & (w > 0) & torch.isfinite(w), w, torch.zeros_like(w))
    tr = None if trim is None else torch.full((21,), float(trim), dtype=torch.float32).to(dev)
    seg = None if segments is None else _segment_ids(segments, T).to(dev)
    out, used = ops.motion_filter(kp.reshape(T, 63).contiguous().to(dev), 0, 21, ops.gaussian_taps(sigma, radius), weights=w.contiguous().to(dev),
                                  segment=seg, trim=tr)
    return out.reshape(T, 21, 3), used


def motion_jitter(motion, params, hand_layer, other=None):
    """How much a motion shakes, from the joints of the layer's forward at the avatar's shape (plain torch on the layer's output):
    dict(accel_mean_mm, accel_max_mm) = the mean and the largest joint acceleration |j[t+1] - 2 j[t] + j[t-1]| in millimetres per frame^2
    (0 for fewer than three frames); with `other`, a second Motion of equal length, also disp_mean_mm / disp_max_mm = the mean and the
    largest distance between the two motions' joints."""
    dev = params["shape"].device

    def joints(m):
        B = len(m)
        betas = params["shape"].detach().reshape(1, -1).expand(B, -1).contiguous()
        with torch.no_grad():
            if "pose_mean" in hand_layer._model_np:          # the SMPL-X arm
                if m.wrist_pose is None:
                    raise ValueError("the arm model needs a motion with wrist_pose")
                return hand_layer(betas=betas, global_orient=m.rot.to(dev), transl=m.trans.to(dev), right_hand_pose=m.pose.to(dev),
                                  right_wrist_pose=m.wrist_pose.to(dev))[1]
            return hand_layer(torch.cat([m.rot, m.pose], 1).to(dev), betas, m.trans.to(dev))[1]

    j = joints(motion)
    acc = (j[2:] - 2.0 * j[1:-1] + j[:-2]).norm(dim=-1) if len(motion) >= 3 else torch.zeros(1, device=j.device)
    res = dict(accel_mean_mm=float(acc.mean()), accel_max_mm=float(acc.max()))
    if other is not None:
        if len(other) != len(motion):
            raise ValueError(f"the two motions must have one length, got {len(motion)} and {len(other)}")
        d = (joints(other) - j).norm(dim=-1)
        res.update(disp_mean_mm=float(d.mean()), disp_max_mm=float(d.max()))
    return res


def pose_mean_rows(hand_layer, with_wrist):
    """what the model adds to the stored rows [rot | (wrist_pose) | pose] before it turns them into rotations: zeros and MANO's hands_mean
    (csrc/lbs.hip:35), or for the SMPL-X arm the slices of its pose mean for joints 0, 21 and 40..54 (hand_models_harp/body_models.py)"""
    m = hand_layer._model_np
    if "pose_mean" in m:
        pm = np.asarray(m["pose_mean"], np.float32).reshape(-1)
        parts = [pm[0:3]] + ([pm[63:66]] if with_wrist else []) + [pm[120:165]]
    else:
        parts = [np.zeros(3, np.float32)] + ([np.zeros(3, np.float32)] if with_wrist else []) + [np.asarray(m["hands_mean"], np.float32).reshape(45)]
    return np.concatenate(parts)


# ---- the host side of Motion.from_keypoints: T problems of six points each, numpy float64 ---------------------------------------------
JOINT_REORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)      # output joint -> model joint / tip (manolayer.py:279)
PALM = (0, 1, 5, 9, 13, 17)                            # output joints that only the root moves: the wrist and the five finger roots
# the 15 chain bones in output joints: wrist -> finger root and the two bones after it; the tip bones are left out (pose correctives move the tips)
CHAIN_BONES = tuple((0 if k == 0 else 4 * f + k, 4 * f + k + 1) for f in range(5) for k in range(3))


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


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with status {rc}")


class AvatarPlayer:
    """Forward-only renderer of a fitted avatar.  configs: the fit's (img_size, focal_length, use_arm, self_shadow,
    share_light_position); params: its parameter dict (verts_disps, shape, texture, normal_map, amb_ratio, light_positions, verts_uvs,
    faces_uvs are read once, here); ss: supersampling factor 1..4 — the avatar is rasterised and shaded at img_size * ss with the focal
    length scaled alike and box-filtered down by the resolve.  Every device buffer is allocated here (or when a longer motion or a longer
    `rows` is first seen); a call only enqueues.  keep_depth=True also keeps the camera view's depth map (s["z_c"], (B, S ss, S ss) view-space z,
    -1 where empty), which a ScenePlayer needs; without it not one launch argument differs."""

    def __init__(self, configs, params, hand_layer, batch_size=32, ss=1, use_graph=True, device="cuda", keep_depth=False):
        from .synth import build_topology
        self.dev = torch.device(device)
        self.keep_depth = bool(keep_depth)             # the camera view's depth s["z_c"] is kept: a ScenePlayer composites by it
        self.S, self.ss, self.B = int(configs["img_size"]), int(ss), int(batch_size)
        if not 1 <= self.ss <= ops.RESOLVE_MAX_SS or self.B < 1 or self.S < 1:
            raise ValueError(f"ss in 1..{ops.RESOLVE_MAX_SS}, batch_size >= 1 and img_size >= 1, got {ss}, {batch_size}, {configs['img_size']}")
        self.Sh, self.focal_h = self.S * self.ss, float(configs["focal_length"]) * self.ss      # what is rasterised and shaded
        self.use_arm, self.self_shadow = bool(configs["use_arm"]), bool(configs["self_shadow"])
        self.share_light = bool(configs["share_light_position"])
        self.use_graph = bool(use_graph)
        faces0 = np.asarray((hand_layer.right_arm_faces_tensor if self.use_arm else hand_layer.th_faces).detach().cpu())
        self.topo = ops.DeviceTopology(build_topology(faces0, 1026 if self.use_arm else 778), params["verts_uvs"], params["faces_uvs"], self.dev)
        if self.topo.V > _lib.lib().harp_mesh_chain_max_vertices():
            raise ValueError(f"the fused front takes meshes of at most {_lib.lib().harp_mesh_chain_max_vertices()} vertices, got {self.topo.V}")
        if self.use_arm:
            from .hand_models_harp.body_models import TreeDeviceModel
            self.dm = TreeDeviceModel(hand_layer._model_np, self.dev)
            self.n_joints, self.pose_stride, self.n_betas = 22, 51, self.dm.NB
            self._weights_T = self.dm.weights.t().contiguous()
        else:
            from .manopth.manolayer import ManoDeviceModel
            self.dm = ManoDeviceModel(hand_layer._model_np, self.dev)
            self.n_joints, self.pose_stride, self.n_betas = 21, 48, 10
        own = lambda k, shape: params[k].detach().to(device=self.dev, dtype=torch.float32).reshape(shape).clone().contiguous()
        tex = params["texture"]
        self.Ht, self.Wt = int(tex.shape[-3]), int(tex.shape[-2])
        self.fit = dict(verts_disps=own("verts_disps", (self.topo.V, 1)), shape=own("shape", (10,)), texture=own("texture", (self.Ht, self.Wt, 3)),
                        normal_map=own("normal_map", (self.Ht, self.Wt, 3)), amb_ratio=own("amb_ratio", (1,)),
                        light_positions=own("light_positions", (-1, 3)))
        self._alloc_scratch()
        with torch.cuda.device(self.dev):
            _ck(_lib.lib().harp_normalize3_pack(_lib.ptr(self.fit["texture"]), _lib.ptr(self.fit["normal_map"]), self.Ht * self.Wt,
                                                _lib.ptr(self.nmap_n), _lib.ptr(self.texnm), _lib.stream()), "normalize3_pack")
        self.T = self._cap = self._n_cap = 0
        self.tab = self.tables = self.bg_buf = None
        self._graphs = {}
        self.bg_color = BG_WHITE

    @property
    def bg_color(self):
        """the constant background colour, three numbers in [0,1] (white); kept on the device, written when it is set"""
        return self._bg_color

    @bg_color.setter
    def bg_color(self, rgb):
        self._bg_color = tuple(float(c) for c in rgb)
        if len(self._bg_color) != 3:
            raise ValueError("bg_color is three numbers")
        self.bg_color_dev.copy_(torch.tensor(self._bg_color, dtype=torch.float32))

    def _alloc_scratch(self):
        """per-batch buffers for B frames at S * ss: what FitEngine keeps for a step's forward half, nothing of its backward"""
        dev, V, Sh, B, tp = self.dev, self.topo.V, self.Sh, self.B, self.topo
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        L = _lib.lib()
        s = {}
        s["pose48"], s["betas"], s["trans_b"] = f(B, self.pose_stride), f(B, self.n_betas), f(B, 3)
        s["cam_R"], s["cam_T"], s["light_pos"], s["colors"] = f(B, 9), f(B, 3), f(B, 3), f(9)
        s["lbs_ws"] = f(L.harp_lbs_tree_ws_floats(ctypes.byref(self.dm.struct), B) if self.use_arm else L.harp_lbs_mano_ws_floats(B))
        s["verts_mm"], s["joints_mm"], s["joints_m"] = f(B, tp.V0, 3), f(B, self.n_joints, 3), f(B, self.n_joints, 3)
        s["vs"], s["n1"], s["il1"], s["vd"], s["n2"], s["il2"] = f(B, V, 3), f(B, V, 3), f(B, V), f(B, V, 3), f(B, V, 3), f(B, V)
        s["ndc_c"], s["ndc_l"], s["centroid"], s["light_R"], s["light_T"] = f(B, V, 3), f(B, V, 3), f(B, 3), f(B, 9), f(B, 3)
        s["ws_c"] = ops.rasterize_workspace(B, tp.F, Sh, dev)
        s["face_c"] = torch.empty(B, Sh, Sh, dtype=torch.int32, device=dev)
        s["rgb"] = f(B, Sh, Sh, 3)
        if self.keep_depth:
            s["z_c"] = f(B, Sh, Sh)
        if self.self_shadow:
            s["ws_l"] = ops.rasterize_workspace(B, tp.F, Sh, dev)
            s["face_l"] = torch.empty(B, Sh, Sh, dtype=torch.int32, device=dev)
            s["zl"] = f(B, Sh, Sh)
            s["zl_state"] = torch.zeros(B * ((Sh + 63) // 64) ** 2, dtype=torch.int32, device=dev)      # harp_rasterize_fwd_keep's, zero before its first call
        self.s = s
        self.nmap_n = f(self.Ht, self.Wt, 3)
        self.texnm = f(self.Ht, self.Wt, 8)
        self.bg_color_dev = f(3)

    # ---- the motion's tables --------------------------------------------------------------------------------------------------
    def load_motion(self, motion):
        """Copy the motion's rows into the player's tables (harp_frame_tables); they grow when the motion is longer than any before, and
        only then are the captured graphs dropped.  The light is the motion's light_positions; without them the fit's own shared light
        (row 0 of its table, optimize_sequence.py:453-456).  A fit with share_light_position=False has no light that applies to
        another motion: such a motion must bring light_positions (Motion.from_params(params, per_frame_light=True) for a replay)."""
        T = len(motion)
        if self.use_arm and motion.wrist_pose is None:
            raise ValueError("the arm model needs a motion with wrist_pose")
        if motion.light_positions is None and not self.share_light:
            raise ValueError("the fit has one light per frame (share_light_position=False): the motion must carry light_positions "
                             "(Motion.from_params(params, per_frame_light=True) replays the fit's)")
        if T > self._cap:
            f = lambda w: torch.zeros(T, w, dtype=torch.float32, device=self.dev)
            self.tab = dict(pose=f(45), rot=f(3), trans=f(3), cam=f(3), light_positions=f(3), wrist_pose=f(3))
            t = _lib.FrameTables()                       # (every g_* pointer stays NULL)
            for k in ("pose", "rot", "trans", "cam", "light_positions"):
                setattr(t, k, _lib.ptr(self.tab[k]))
            t.shape, t.amb_ratio = _lib.ptr(self.fit["shape"]), _lib.ptr(self.fit["amb_ratio"])
            t.share_light = 0                            # the table always holds one light per row (a shared light is written to every row)
            if self.use_arm:
                t.wrist_pose = _lib.ptr(self.tab["wrist_pose"])
            t.n_betas_out = self.n_betas
            self.tables, self._cap, self._graphs = t, T, {}
        with torch.no_grad():
            for k in ("pose", "rot", "trans", "cam") + (("wrist_pose",) if self.use_arm else ()):
                self.tab[k][:T].copy_(getattr(motion, k).to(self.dev))
            light = motion.light_positions.to(self.dev) if motion.light_positions is not None else self.fit["light_positions"][0:1].expand(T, 3)
            self.tab["light_positions"][:T].copy_(light)
        self.T = T

    # ---- structs over the player's buffers (FitEngine._chain_struct / _frame_struct / _shade_struct without a gradient pointer) -----
    def _front_struct(self, fid):
        s, p, tp, arm = self.s, _lib.ptr, self.topo, self.use_arm
        h = _lib.ArmFront() if arm else _lib.HandFront()
        c = _lib.MeshChain()                             # (every g_* pointer stays NULL)
        for k, t in (("edges0", tp.edges0), ("vf_off", tp.vf_off), ("vf_tri", tp.vf_tri), ("sub_off", tp.sub_off), ("sub_idx", tp.sub_idx),
                     ("disp", self.fit["verts_disps"])):
            setattr(c, k, p(t))
        for k in ("verts_mm", "joints_mm", "cam_R", "cam_T", "light_pos", "joints_m", "vs", "n1", "il1", "vd", "n2", "il2", "ndc_c", "centroid",
                  "light_R", "light_T", "ndc_l"):
            setattr(c, k, p(s[k]))
        c.B, c.V0, c.E0, c.NJ, c.S = self.B, tp.V0, tp.E0, self.n_joints, self.Sh
        c.focal, c.shadow, c.has_normal_grad, c.light_only = self.focal_h, int(self.self_shadow), 0, 0
        h.chain, h.tables = c, self.tables
        setattr(h, "tree" if arm else "mano", self.dm.struct)
        for k, t in (("fid", fid), ("pose_in" if arm else "pose48", s["pose48"]), ("betas", s["betas"]), ("trans_b", s["trans_b"]),
                     ("cam_R", s["cam_R"]), ("cam_T", s["cam_T"]), ("light_pos", s["light_pos"]), ("colors", s["colors"]), ("lbs_ws", s["lbs_ws"])):
            setattr(h, k, p(t))
        if arm:
            h.weights_T = p(self._weights_T)
        h.self_shadow = int(self.self_shadow)
        return h

    def _shade_struct(self):
        s, sh = self.s, self.self_shadow
        a = ops._shade_args(s["face_c"], s["ws_c"], self.topo, s["vd"], s["n2"], self.fit["texture"], self.nmap_n, s["light_pos"], s["colors"],
                            s["zl"] if sh else None, s["light_R"] if sh else None, s["light_T"] if sh else None, self.Sh, self.focal_h,
                            (self.Sh / 2.0, self.Sh / 2.0), BG_WHITE)
        a.rgb, a.texnm = _lib.ptr(s["rgb"]), _lib.ptr(self.texnm)
        return a

    def _render_batch(self, fid):
        """front, rasterisers and shader of one batch of B frames, in order on the current stream: s["rgb"], s["face_c"] (and s["z_c"]
        with keep_depth) at S * ss, everything in front of the resolve"""
        L, s, p, tp, st = _lib.lib(), self.s, _lib.ptr, self.topo, _lib.stream()
        B, V, F, Sh = self.B, tp.V, tp.F, self.Sh
        z_c = p(s["z_c"]) if self.keep_depth else None
        h = self._front_struct(fid)
        _ck((L.harp_arm_front_fwd if self.use_arm else L.harp_hand_front_fwd)(ctypes.byref(h), st), "front_fwd")
        if self.self_shadow:
            _ck(L.harp_raster_setup_pair(p(s["ndc_c"]), 0.0, p(s["ws_c"]), p(s["ndc_l"]), 0.0, p(s["ws_l"]), p(tp.faces), B, V, F, Sh, st),
                "raster_setup_pair")
            _ck(L.harp_rasterize_fwd(p(s["ndc_c"]), p(tp.faces), B, V, F, Sh, 4, 0.0, 1.0, p(s["ws_c"]), p(s["face_c"]), z_c, None, st), "raster_cam")
            _ck(L.harp_rasterize_fwd_keep(p(s["ndc_l"]), p(tp.faces), B, V, F, Sh, 4, p(s["ws_l"]), p(s["face_l"]), p(s["zl"]), p(s["zl_state"]), st),
                "raster_light")
        else:                                            # one view: the rasteriser's own set-up
            _ck(L.harp_rasterize_fwd(p(s["ndc_c"]), p(tp.faces), B, V, F, Sh, 0, 0.0, 1.0, p(s["ws_c"]), p(s["face_c"]), z_c, None, st), "raster_cam")
        _ck(L.harp_shade_fwd(ctypes.byref(self._shade_struct()), st), "shade_fwd")

    def _batch(self, fid, bg, n_bg, bg_rows, out, channels):
        """the launches of one batch of B frames, in order on the current stream"""
        L, s, p = _lib.lib(), self.s, _lib.ptr
        self._render_batch(fid)
        _ck(L.harp_resolve_u8(p(s["rgb"]), p(s["face_c"]), self.B, self.S, self.ss, bg, n_bg, bg_rows, p(self.bg_color_dev), channels, out, _lib.stream()),
            "resolve_u8")

    def _grow(self, n_pad, with_bg):
        if n_pad > self._n_cap:
            # per rendered frame: its row of the motion | its row of the player's copy of the backgrounds (-1: the constant colour) | the row of
            # the caller's background tensor that is copied there; staged in pinned memory and uploaded in one copy per call
            self.idx_dev = torch.zeros(3, n_pad, dtype=torch.int32, device=self.dev)
            self.idx_pin = torch.zeros(3, n_pad, dtype=torch.int32).pin_memory()
            self.idx_done = None
            self.out = torch.empty(n_pad * self.S * self.S * 4, dtype=torch.uint8, device=self.dev)
            self.bg_buf = None
            self._n_cap, self._graphs = n_pad, {}
        if with_bg and self.bg_buf is None:              # (no graph reads it yet)
            self.bg_buf = torch.empty(self._n_cap, self.S, self.S, 3, dtype=torch.uint8, device=self.dev)

    def _enqueue(self, n_pad, with_bg, channels):
        per = self.S * self.S * channels
        for lo in range(0, n_pad, self.B):
            self._batch(self.idx_dev[0, lo:lo + self.B], self.bg_buf.data_ptr() if with_bg else None, self._n_cap if with_bg else 0,
                        self.idx_dev[1, lo:lo + self.B].data_ptr() if with_bg else None, self.out[lo * per:].data_ptr(), channels)

    @torch.no_grad()
    def render(self, rows, background=None, bg_rows=None, alpha=False):
        """Frames `rows` of the loaded motion -> (len(rows), S, S, 3) uint8 on the device ((.., 4) with alpha=True: the covered share of the
        pixel as alpha), a view of the player's buffer that the next call overwrites.  background: None (the constant `bg_color`, white) or
        a (N,S,S,3) uint8 device tensor; frame i is composited over its row bg_rows[i], without bg_rows over row i (N == len(rows)) or row
        0 (N == 1); a row outside [0, N) takes bg_color.  The rows in use are copied into a buffer of the player's in stream order, so
        one captured graph serves every background tensor and the caller's tensor is free again once the call has returned."""
        if self.tables is None:
            raise RuntimeError("load_motion() first")
        r = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows, dtype=np.int64).reshape(-1)
        n = r.shape[0]
        if n < 1:
            raise ValueError("no rows to render")
        if r.min() < 0 or r.max() >= self.T:             # (on the host, before anything is enqueued: the kernels gather rows unchecked)
            raise IndexError(f"rows span [{r.min()}, {r.max()}] but the motion holds {self.T} frames")
        C = 4 if alpha else 3
        br = None
        if background is not None:
            if (not torch.is_tensor(background) or background.dtype != torch.uint8 or background.device != self._device() or background.dim() != 4
                    or tuple(background.shape[1:]) != (self.S, self.S, 3) or background.shape[0] < 1):
                raise TypeError(f"background must be a uint8 (N, {self.S}, {self.S}, 3) tensor on {self.dev}")
            n_bg = int(background.shape[0])
            if bg_rows is None:
                if n_bg not in (1, n):
                    raise ValueError(f"{n_bg} backgrounds for {n} frames: pass bg_rows")
                br = np.arange(n, dtype=np.int64) if n_bg == n else np.zeros(n, dtype=np.int64)
            else:
                br = np.asarray(bg_rows.cpu() if torch.is_tensor(bg_rows) else bg_rows, dtype=np.int64).reshape(-1)
                if br.shape[0] != n:
                    raise ValueError("bg_rows must have one entry per row")
        elif bg_rows is not None:
            raise ValueError("bg_rows without a background")
        with_bg = br is not None
        B = self.B
        n_pad = -(-n // B) * B
        with torch.cuda.device(self.dev):
            self._grow(n_pad, with_bg)
            if self.idx_done is not None:
                self.idx_done.synchronize()              # the previous call's upload has read the staging buffer
            stage = self.idx_pin.numpy()
            stage[0, :n], stage[0, n:n_pad] = r, r[-1]   # a short last batch is padded with its last row
            if with_bg:
                inside = (br >= 0) & (br < n_bg)
                stage[1, :n], stage[1, n:n_pad] = np.where(inside, np.arange(n), -1), (n - 1 if inside[-1] else -1)
                stage[2, :n], stage[2, n:n_pad] = np.where(inside, br, 0), (br[-1] if inside[-1] else 0)
            self.idx_dev.copy_(self.idx_pin, non_blocking=True)
            self.idx_done = torch.cuda.Event()
            self.idx_done.record()
            if with_bg:
                torch.index_select(background, 0, self.idx_dev[2, :n], out=self.bg_buf[:n])
            if not self.use_graph:
                self._enqueue(n_pad, with_bg, C)
            else:
                key = (n_pad, C, with_bg)
                g = self._graphs.get(key)
                if g is None:
                    # warm-up (the first launches size their LDS with runtime calls that a capture does not allow), then capture; on the
                    # current stream: the sequence allocates nothing and has no branches, and the player takes no stream from torch's pool
                    self._enqueue(n_pad, with_bg, C)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._enqueue(n_pad, with_bg, C)
                    self._graphs[key] = g
                g.replay()
        return self.out[:n * self.S * self.S * C].view(n, self.S, self.S, C)

    def _device(self):
        return self.dev if self.dev.index is not None else torch.device(self.dev.type, torch.cuda.current_device())

    # ---- a whole motion to files ------------------------------------------------------------------------------------------------
    def play(self, motion, out_dir, backgrounds=None, fmt="jpg", alpha=False):
        """load_motion(motion), render it batch by batch and write out_dir/%04d.<fmt> (fmt "jpg" or "png"; alpha=True needs "png" and
        writes RGBA).  backgrounds: None, a (N,S,S,3) uint8 tensor or a directory of images of that size (sorted by name); frame i is
        composited over background i mod N.  The frames leave through two pinned host buffers, one per batch in flight, and are encoded on
        a thread pool while the next batch renders.  Returns the list of paths."""
        from concurrent.futures import ThreadPoolExecutor
        from .utils.data_util import default_workers
        if fmt not in ("jpg", "png") or (alpha and fmt != "png"):
            raise ValueError(f'fmt is "jpg" or "png", and alpha=True needs "png"; got {fmt!r}, alpha={alpha}')
        os.makedirs(out_dir, exist_ok=True)
        self.load_motion(motion)
        bgs = load_backgrounds(backgrounds, self.S, self.dev)
        T, B, C = self.T, self.B, 4 if alpha else 3
        pinned = [torch.empty(B, self.S, self.S, C, dtype=torch.uint8).pin_memory() for _ in range(2)]
        pending = [[], []]
        paths = [os.path.join(out_dir, "%04d.%s" % (i, fmt)) for i in range(T)]
        with ThreadPoolExecutor(max(1, min(8, default_workers()))) as pool:
            for k, lo in enumerate(range(0, T, B)):
                rows = np.arange(lo, min(T, lo + B))
                for fut in pending[k % 2]:                # the buffer's previous frames are on disk
                    fut.result()
                frames = self.render(rows, bgs, None if bgs is None else rows % bgs.shape[0], alpha)
                host = pinned[k % 2][:len(rows)]
                host.copy_(frames, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()
                arr = host.numpy()
                pending[k % 2] = [pool.submit(_encode, paths[i], arr[i - lo], fmt) for i in rows]
            for futs in pending:
                for fut in futs:
                    fut.result()
        return paths

def _host_rows(name, rows, n=None):
    r = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows, dtype=np.int64).reshape(-1)
    if n is not None and r.shape[0] != n:
        raise ValueError(f"{name} must have one entry per row")
    return r


class ScenePlayer:
    """Several avatars in one frame with depth-correct occlusion: 1 to 4 AvatarPlayers built with keep_depth=True on one
    device with equal img_size, ss and batch_size — one camera: the focal length is the players' too, the translation comes from each
    motion's cam — rendered batch by batch into their own buffers and resolved by ONE harp_composite_layers_u8 per batch: per sub-sample
    the nearest avatar in front of an optional scene depth.  flip: one bool per player; a flipped avatar is shown mirrored in x, light
    included — a LEFT hand is a right-hand fit of horizontally mirrored frames shown with flip.  The avatars cast no shadows on each
    other.  The launches are captured into a graph when every player was built with use_graph=True."""

    def __init__(self, players, flip=None):
        players = list(players)
        if not 1 <= len(players) <= ops.COMPOSITE_MAX_LAYERS:
            raise ValueError(f"a scene holds 1..{ops.COMPOSITE_MAX_LAYERS} players, got {len(players)}")
        p0 = players[0]
        for p in players:
            if not isinstance(p, AvatarPlayer) or not p.keep_depth:
                raise ValueError("a scene takes AvatarPlayers built with keep_depth=True")
            if (p.S, p.ss, p.B) != (p0.S, p0.ss, p0.B) or p._device() != p0._device():
                raise ValueError(f"the players of a scene share img_size, ss, batch_size and the device: got {(p.S, p.ss, p.B, p._device())} "
                                 f"and {(p0.S, p0.ss, p0.B, p0._device())}")
        self.flip = [False] * len(players) if flip is None else [bool(f) for f in flip]
        if len(self.flip) != len(players):
            raise ValueError("flip holds one entry per player")
        self.players, self.dev, self.S, self.ss, self.B = players, p0.dev, p0.S, p0.ss, p0.B
        self.use_graph = all(p.use_graph for p in players)
        self.bg_color_dev = torch.empty(3, dtype=torch.float32, device=self.dev)
        self.bg_color = BG_WHITE
        self.T = self._n_cap = 0
        self.bg_buf = self.depth_buf = self.idx_done = None
        self._graphs = {}

    bg_color = AvatarPlayer.bg_color
    _device = AvatarPlayer._device

    def load_motions(self, motions):
        """one motion per player, of equal length: scene row i is row i of every motion (AvatarPlayer.load_motion each)"""
        motions = list(motions)
        if len(motions) != len(self.players):
            raise ValueError(f"{len(motions)} motions for {len(self.players)} players")
        if len({len(m) for m in motions}) != 1:
            raise ValueError(f"the motions of a scene have one length, got {[len(m) for m in motions]}")
        tables = [p.tables for p in self.players]
        for p, m in zip(self.players, motions):
            p.load_motion(m)
        if any(p.tables is not t for p, t in zip(self.players, tables)):      # (tables that grew: the captured pointers are gone)
            self._graphs = {}
        self.T = len(motions[0])

    def _grow(self, n_pad, with_bg, with_depth):
        if n_pad > self._n_cap:
            # per rendered frame: its row of the motions | its row of the scene's copy of the backgrounds (-1: the constant colour) | the row of
            # the caller's background tensor copied there | the same two for the scene depth (-1: no scene depth)
            self.idx_dev = torch.zeros(5, n_pad, dtype=torch.int32, device=self.dev)
            self.idx_pin = torch.zeros(5, n_pad, dtype=torch.int32).pin_memory()
            self.idx_done = None
            self.out = torch.empty(n_pad * self.S * self.S * 4, dtype=torch.uint8, device=self.dev)
            self.owner = torch.empty(n_pad, self.S, self.S, dtype=torch.uint8, device=self.dev)
            self.bg_buf = self.depth_buf = None
            self._n_cap, self._graphs = n_pad, {}
        if with_bg and self.bg_buf is None:              # (no graph reads it yet)
            self.bg_buf = torch.empty(self._n_cap, self.S, self.S, 3, dtype=torch.uint8, device=self.dev)
        if with_depth and self.depth_buf is None:
            self.depth_buf = torch.empty(self._n_cap, self.S, self.S, dtype=torch.float32, device=self.dev)

    def _enqueue(self, n_pad, with_bg, with_depth, channels, with_owner):
        """per batch: every player's front / rasterisers / shader, then one composite"""
        L, p, B = _lib.lib(), _lib.ptr, self.B
        per = self.S * self.S
        layers = (_lib.Layer * len(self.players))(*[_lib.Layer(p(pl.s["rgb"]), p(pl.s["z_c"]), int(f), 0) for pl, f in zip(self.players, self.flip)])
        for lo in range(0, n_pad, B):
            for pl in self.players:
                pl._render_batch(self.idx_dev[0, lo:lo + B])
            _ck(L.harp_composite_layers_u8(layers, len(self.players), B, self.S, self.ss,
                                           self.depth_buf.data_ptr() if with_depth else None, self._n_cap if with_depth else 0,
                                           self.idx_dev[3, lo:lo + B].data_ptr() if with_depth else None,
                                           self.bg_buf.data_ptr() if with_bg else None, self._n_cap if with_bg else 0,
                                           self.idx_dev[1, lo:lo + B].data_ptr() if with_bg else None, p(self.bg_color_dev), channels,
                                           self.out[lo * per * channels:].data_ptr(), self.owner[lo:].data_ptr() if with_owner else None,
                                           _lib.stream()), "composite_layers_u8")

    def _staged(self, name, t, rows, n, shape, dtype):
        """a (N, *shape) device tensor of the caller's and its rows -> (the rows checked, N), as AvatarPlayer.render treats backgrounds"""
        if t is None:
            if rows is not None:
                raise ValueError(f"rows of a {name} without the {name}")
            return None, 0
        if (not torch.is_tensor(t) or t.dtype != dtype or t.device != self._device() or t.dim() != 1 + len(shape)
                or tuple(t.shape[1:]) != shape or t.shape[0] < 1):
            raise TypeError(f"{name} must be a {dtype} (N, {', '.join(map(str, shape))}) tensor on {self.dev}")
        N = int(t.shape[0])
        if rows is None:
            if N not in (1, n):
                raise ValueError(f"{N} rows of {name} for {n} frames: pass its rows")
            return (np.arange(n, dtype=np.int64) if N == n else np.zeros(n, dtype=np.int64)), N
        return _host_rows(f"the rows of {name}", rows, n), N

    @torch.no_grad()
    def render(self, rows, background=None, bg_rows=None, alpha=False, scene_depth=None, depth_rows=None, owner=False):
        """Scene rows `rows` of the loaded motions -> (len(rows), S, S, 3|4) uint8 on the device, a view of the scene's buffer that the
        next call overwrites; with owner=True (frames, owner (len(rows), S, S) uint8: 0 = background, 1 + the player that shows most of
        the pixel).  background / bg_rows / alpha: as AvatarPlayer.render.  scene_depth: None or a float32 (N,S,S) device tensor at output
        resolution in the unit of the avatars' view depth (a value > 0 is a measurement and hides what lies behind it); frame i is tested
        against its row depth_rows[i], without depth_rows against row i (N == len(rows)) or row 0 (N == 1); a row outside [0, N) means no
        scene depth.  Backgrounds and depths in use are copied into buffers of the scene's, so one captured graph per (padded length,
        channels, background?, depth?, owner?) serves every tensor."""
        if self.T < 1 or any(p.tables is None for p in self.players):
            raise RuntimeError("load_motions() first")
        r = _host_rows("rows", rows)
        n = r.shape[0]
        if n < 1:
            raise ValueError("no rows to render")
        if r.min() < 0 or r.max() >= self.T:             # (on the host, before anything is enqueued: the kernels gather rows unchecked)
            raise IndexError(f"rows span [{r.min()}, {r.max()}] but the motions hold {self.T} frames")
        C = 4 if alpha else 3
        br, n_bg = self._staged("background", background, bg_rows, n, (self.S, self.S, 3), torch.uint8)
        dr, n_d = self._staged("scene_depth", scene_depth, depth_rows, n, (self.S, self.S), torch.float32)
        with_bg, with_depth, with_owner = br is not None, dr is not None, bool(owner)
        B = self.B
        n_pad = -(-n // B) * B
        with torch.cuda.device(self.dev):
            self._grow(n_pad, with_bg, with_depth)
            if self.idx_done is not None:
                self.idx_done.synchronize()              # the previous call's upload has read the staging buffer
            stage = self.idx_pin.numpy()
            stage[0, :n], stage[0, n:n_pad] = r, r[-1]   # a short last batch is padded with its last row
            for k, rr, N in ((1, br, n_bg), (3, dr, n_d)):
                if rr is not None:
                    inside = (rr >= 0) & (rr < N)
                    stage[k, :n], stage[k, n:n_pad] = np.where(inside, np.arange(n), -1), (n - 1 if inside[-1] else -1)
                    stage[k + 1, :n], stage[k + 1, n:n_pad] = np.where(inside, rr, 0), (rr[-1] if inside[-1] else 0)
            self.idx_dev.copy_(self.idx_pin, non_blocking=True)
            self.idx_done = torch.cuda.Event()
            self.idx_done.record()
            if with_bg:
                torch.index_select(background, 0, self.idx_dev[2, :n], out=self.bg_buf[:n])
            if with_depth:
                torch.index_select(scene_depth, 0, self.idx_dev[4, :n], out=self.depth_buf[:n])
            if not self.use_graph:
                self._enqueue(n_pad, with_bg, with_depth, C, with_owner)
            else:
                key = (n_pad, C, with_bg, with_depth, with_owner)
                g = self._graphs.get(key)
                if g is None:                            # warm-up, then capture on the current stream, as AvatarPlayer.render
                    self._enqueue(n_pad, with_bg, with_depth, C, with_owner)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._enqueue(n_pad, with_bg, with_depth, C, with_owner)
                    self._graphs[key] = g
                g.replay()
        frames = self.out[:n * self.S * self.S * C].view(n, self.S, self.S, C)
        return (frames, self.owner[:n]) if with_owner else frames

    def play(self, motions, out_dir, backgrounds=None, scene_depth=None, fmt="jpg", alpha=False, masks=False):
        """load_motions(motions), render the scene batch by batch and write out_dir/%04d.<fmt> as AvatarPlayer.play does; with masks=True
        also out_dir/mask_%04d.png, the owner map (8-bit grey: 0 background, 1 + the player).  backgrounds: as AvatarPlayer.play;
        scene_depth: None, a float32 (N,S,S) tensor or a directory (load_scene_depth), frame i tested against depth i mod N.  Returns the
        list of the frames' paths."""
        from concurrent.futures import ThreadPoolExecutor
        from .utils.data_util import default_workers
        if fmt not in ("jpg", "png") or (alpha and fmt != "png"):
            raise ValueError(f'fmt is "jpg" or "png", and alpha=True needs "png"; got {fmt!r}, alpha={alpha}')
        os.makedirs(out_dir, exist_ok=True)
        self.load_motions(motions)
        bgs = load_backgrounds(backgrounds, self.S, self.dev)
        depth = load_scene_depth(scene_depth, self.S, self.dev)
        T, B, C = self.T, self.B, 4 if alpha else 3
        pinned = [torch.empty(B, self.S, self.S, C + 1, dtype=torch.uint8).pin_memory() for _ in range(2)]      # (the last plane: the owner map)
        pending = [[], []]
        paths = [os.path.join(out_dir, "%04d.%s" % (i, fmt)) for i in range(T)]
        with ThreadPoolExecutor(max(1, min(8, default_workers()))) as pool:
            for k, lo in enumerate(range(0, T, B)):
                rows = np.arange(lo, min(T, lo + B))
                for fut in pending[k % 2]:                # the buffer's previous frames are on disk
                    fut.result()
                got = self.render(rows, bgs, None if bgs is None else rows % bgs.shape[0], alpha, depth,
                                  None if depth is None else rows % depth.shape[0], owner=masks)
                host = pinned[k % 2][:len(rows)]
                if masks:
                    host[..., :C].copy_(got[0], non_blocking=True)
                    host[..., C].copy_(got[1], non_blocking=True)
                else:
                    host[..., :C].copy_(got, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()
                arr = host.numpy()
                pending[k % 2] = [pool.submit(_encode, paths[i], np.ascontiguousarray(arr[i - lo, :, :, :C]), fmt) for i in rows]
                if masks:
                    pending[k % 2] += [pool.submit(_encode, os.path.join(out_dir, "mask_%04d.png" % i), np.ascontiguousarray(arr[i - lo, :, :, C]), "png")
                                       for i in rows]
            for futs in pending:
                for fut in futs:
                    fut.result()
        return paths


def _encode(path, u8, fmt):
    if fmt == "jpg":
        from .monitor import encode_jpeg
        encode_jpeg(path, u8)
    else:                                                # uint8 RGB / RGBA as it is (harp_amd.io.encode_png quantises a float texture)
        from PIL import Image
        Image.fromarray(u8).save(path, format="PNG")


def load_backgrounds(backgrounds, S, device):
    """None, a (N,S,S,3) uint8 tensor, or a directory of S x S images (sorted by name) -> None or that tensor on `device`"""
    if backgrounds is None:
        return None
    if isinstance(backgrounds, (str, os.PathLike)):
        from PIL import Image
        names = sorted(f for f in os.listdir(backgrounds) if f.lower().endswith((".jpg", ".jpeg", ".png")))
        if not names:
            raise ValueError(f"no images in {backgrounds}")
        backgrounds = torch.from_numpy(np.stack([np.asarray(Image.open(os.path.join(backgrounds, f)).convert("RGB")) for f in names]))
    b = torch.as_tensor(backgrounds)
    if b.dtype != torch.uint8 or b.dim() != 4 or tuple(b.shape[1:]) != (S, S, 3):
        raise ValueError(f"backgrounds must be uint8 (N, {S}, {S}, 3), got {b.dtype} {tuple(b.shape)}")
    return b.to(device).contiguous()


def load_scene_depth(depth, S, device):
    """None, a float32 (N,S,S) tensor, or a directory (sorted by name) of .npy float32 (S,S) in metres and / or 16-bit PNGs in millimetres,
    0 = no measurement -> None or that tensor in metres on `device`"""
    if depth is None:
        return None
    if isinstance(depth, (str, os.PathLike)):
        from PIL import Image
        names = sorted(f for f in os.listdir(depth) if f.lower().endswith((".npy", ".png")))
        if not names:
            raise ValueError(f"no .npy or .png depth maps in {depth}")
        maps = []
        for f in names:
            path = os.path.join(depth, f)
            maps.append(np.load(path).astype(np.float32) if f.lower().endswith(".npy") else np.asarray(Image.open(path)).astype(np.float32) * 1e-3)
        depth = torch.from_numpy(np.stack(maps))
    d = torch.as_tensor(depth)
    if d.dtype != torch.float32 or d.dim() != 3 or tuple(d.shape[1:]) != (S, S):
        raise ValueError(f"scene depth must be float32 (N, {S}, {S}), got {d.dtype} {tuple(d.shape)}")
    return d.to(device).contiguous()


def main(argv=None):
    """A fit (the saved_params[_test].pkl under the config's base_output_dir, as the evaluation reads it) plus a motion file -> a directory
    of frames."""
    import argparse
    import yaml
    from .utils import file_utils, hand_model_utils
    from .utils.config_utils import get_config
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="yaml with the keys of utils/config_utils.get_config (the fit's)")
    ap.add_argument("--motion", default=None, help=".npz of pose (T,45), rot, trans, cam (T,3) [, wrist_pose, light_positions] (Motion.save)")
    ap.add_argument("--keypoints", default=None, help=".npz of keypoints (T,21,3) in metres [, weights (T,21), cam (3,) or (T,3)] instead of --motion: "
                                                      "the motion is solved from them (Motion.from_keypoints)")
    ap.add_argument("--out", required=True, help="directory for the frames %%04d.jpg / %%04d.png")
    ap.add_argument("--fps-scale", type=float, default=1.0, help="output frames per motion frame (2: twice as many frames, half the speed)")
    ap.add_argument("--ss", type=int, default=1, help="supersampling factor 1..4")
    ap.add_argument("--background", default=None, help="directory of img_size x img_size images to composite over (cycled)")
    ap.add_argument("--alpha", action="store_true", help="RGBA PNGs with the coverage as alpha")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--flip", action="store_true", help="show the avatar mirrored in x: a left hand is a right-hand fit of mirrored frames")
    ap.add_argument("--also", action="append", default=[], metavar="CFG:MOTION[:flip]",
                    help="a further avatar with its own fit and motion in the same frames, nearest surface in front (up to three times)")
    ap.add_argument("--scene-depth", default=None, help="directory of .npy float32 (img_size, img_size) depth maps in metres or 16-bit PNGs in "
                                                        "millimetres, 0 = no measurement (cycled): what is nearer hides the avatars")
    ap.add_argument("--masks", action="store_true", help="also write mask_%%04d.png: 0 background, 1 + the avatar that owns the pixel")
    ap.add_argument("--smooth", type=float, default=None, metavar="SIGMA",
                    help="filter the loaded or solved motion with a Gaussian window of SIGMA frames before --fps-scale (Motion.smooth); prints the "
                         "joint jitter before and after")
    ap.add_argument("--smooth-trim", type=float, default=None, metavar="RAD",
                    help="with --smooth: leave a rotation farther than RAD radians from its window's estimate out of a second estimate (spikes)")
    ap.add_argument("--smooth-keypoints", type=float, default=None, metavar="SIGMA",
                    help="with --keypoints: filter the keypoints with a Gaussian window of SIGMA frames before the solve, filling dropped joints")
    args = ap.parse_args(argv)
    for name in ("smooth", "smooth_trim", "smooth_keypoints"):
        v = getattr(args, name)
        if v is not None and not v > 0:
            raise SystemExit(f"--{name.replace('_', '-')} must be positive")
    if args.smooth_trim is not None and args.smooth is None:
        raise SystemExit("--smooth-trim needs --smooth")
    if args.smooth_keypoints is not None and args.keypoints is None:
        raise SystemExit("--smooth-keypoints needs --keypoints")
    if len(args.also) > ops.COMPOSITE_MAX_LAYERS - 1:
        raise SystemExit(f"--also at most {ops.COMPOSITE_MAX_LAYERS - 1} times")
    if args.fps_scale <= 0:
        raise SystemExit("--fps-scale must be positive")
    if (args.motion is None) == (args.keypoints is None):
        raise SystemExit("exactly one of --motion and --keypoints")

    def load(cfg_path, motion_path, keypoints_path=None):
        with open(cfg_path) as f:
            configs = get_config(write_yaml=False, **yaml.safe_load(f))
        configs["device"] = args.device
        hand_layer, VERTS_UVS, FACES_UVS, _ = hand_model_utils.load_hand_model(configs)
        params = file_utils.load_result(configs["base_output_dir"], device=args.device, test=bool(configs["known_appearance"]))
        params["verts_uvs"], params["faces_uvs"] = VERTS_UVS, FACES_UVS
        if keypoints_path is not None:
            with np.load(keypoints_path) as z:
                motion = Motion.from_keypoints(z["keypoints"], params, hand_layer, cam=z["cam"] if "cam" in z.files else None,
                                               weights=z["weights"] if "weights" in z.files else None, device=args.device,
                                               smooth=args.smooth_keypoints)
        else:
            motion = Motion.load(motion_path)
        if args.smooth is not None:
            raw = motion
            motion = raw.smooth(hand_layer, sigma=args.smooth, trim_rot=args.smooth_trim, device=args.device)
            before, after = motion_jitter(raw, params, hand_layer), motion_jitter(motion, params, hand_layer, other=raw)
            print(f"smoothed {len(motion)} frames (sigma {args.smooth:g}): joint acceleration mean {before['accel_mean_mm']:.3f} -> "
                  f"{after['accel_mean_mm']:.3f} mm/frame^2, largest {before['accel_max_mm']:.3f} -> {after['accel_max_mm']:.3f}; joints moved "
                  f"{after['disp_mean_mm']:.3f} mm on average, {after['disp_max_mm']:.3f} at most")
        if args.fps_scale != 1.0:
            n = max(1, int(round((len(motion) - 1) * args.fps_scale)) + 1)
            motion = motion.resample(np.linspace(0, len(motion) - 1, n), hand_layer, device=args.device)
        return configs, params, hand_layer, motion

    fmt = "png" if args.alpha else "jpg"
    if not (args.flip or args.also or args.scene_depth or args.masks):
        configs, params, hand_layer, motion = load(args.config, args.motion, args.keypoints)
        player = AvatarPlayer(configs, params, hand_layer, batch_size=args.batch_size, ss=args.ss, device=args.device)
        paths = player.play(motion, args.out, backgrounds=args.background, fmt=fmt, alpha=args.alpha)
    else:
        specs = [(args.config, args.motion, args.flip, args.keypoints)]
        for spec in args.also:
            part = spec.split(":")
            if len(part) not in (2, 3) or (len(part) == 3 and part[2] != "flip"):
                raise SystemExit(f"--also takes CFG:MOTION or CFG:MOTION:flip, got {spec!r}")
            specs.append((part[0], part[1], len(part) == 3, None))
        players, motions = [], []
        for cfg_path, motion_path, _, keypoints_path in specs:
            configs, params, hand_layer, motion = load(cfg_path, motion_path, keypoints_path)
            players.append(AvatarPlayer(configs, params, hand_layer, batch_size=args.batch_size, ss=args.ss, device=args.device, keep_depth=True))
            motions.append(motion)
        scene = ScenePlayer(players, flip=[f for _, _, f, _ in specs])
        paths = scene.play(motions, args.out, backgrounds=args.background, scene_depth=args.scene_depth, fmt=fmt, alpha=args.alpha, masks=args.masks)
    print(f"wrote {len(paths)} frames to {args.out}")
    return paths


if __name__ == "__main__":
    main()
