"""The rows of a motion and what is done to them on the device: `Motion`, its retiming (ops.motion_resample), its solve
from 3-D keypoints (ops.mano_ik, §24; the SMPL-X arm: ops.arm_ik, §29), from image keypoints (ops.mano_reproj_ik, §30; the SMPL-X arm:
ops.arm_reproj_ik, §35) or from mesh
vertices (ops.mano_vertex_fit, §27; the SMPL-X arm: ops.arm_vertex_fit, §28) and the window filter of a motion or of keypoints
(ops.motion_filter, §25).  `RowLayout` is the one description of the packed table that the resampler and the filter read.  What the
solving constructors set up alike stands once (§34): on the host in keypoints.py, where a device is involved in the private functions
below."""
import numpy as np
import torch

from .. import ops
from . import keypoints as K
from .keypoints import checked


def _rows_f32(name, a, width, T=None):
    return checked(name, a, (T, width), tensor=True).to(torch.float32).contiguous()


def _solve_on(device, params):
    """(the device a Motion.from_* solve runs on: `device`, by default that of params["shape"] when it is a HIP device, else "cuda"; the
    float32 upload of a host array to it, None staying None)"""
    dev = torch.device(device if device is not None else (params["shape"].device if params["shape"].is_cuda else "cuda"))
    return dev, lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def _hand_device_model(hand_layer, dev):
    from ..manopth.manolayer import ManoDeviceModel
    return ManoDeviceModel(hand_layer._model_np, dev)


def _arm_device_model(arm_layer, dev):
    """the layer's own TreeDeviceModel when it lives on `dev`, else one made there"""
    if arm_layer._dev == dev:
        return arm_layer.device_model
    from ..hand_models_harp.body_models import TreeDeviceModel
    return TreeDeviceModel(arm_layer._model_np, dev)


def _window(smooth, dev, joints=21):
    """smooth=sigma as the function K.smoothed takes: smooth_keypoints on `dev`, its two results brought to the host; None for None"""
    return None if smooth is None else lambda kp, w: tuple(t.cpu().numpy() for t in smooth_keypoints(kp, weights=w, sigma=smooth, device=dev, joints=joints))


class RowLayout:
    """A motion's rows as one table [rot | wrist_pose? | pose | trans | light_positions? | cam]: `fields` is the ordered list of (field,
    width, kind) for the fields the motion has, kind "rot" (axis-angle triples), "vec" (a 3-vector) or "scalar"; n_rot triples come
    first, then n_vec vectors, then cam's three scalars — what ops.motion_filter takes, and ops.motion_resample with everything behind
    the rotations as linear channels."""

    def __init__(self, motion):
        wrist, light = motion.wrist_pose is not None, motion.light_positions is not None
        self.motion = motion
        self.fields = ([("rot", 3, "rot")] + [("wrist_pose", 3, "rot")] * wrist + [("pose", 45, "rot"), ("trans", 3, "vec")]
                       + [("light_positions", 3, "vec")] * light + [("cam", 3, "scalar")])
        self.widths = [w for _, w, _ in self.fields]
        self.n_rot = sum(w // 3 for _, w, kind in self.fields if kind == "rot")
        self.n_vec = sum(kind == "vec" for _, _, kind in self.fields)

    def pack(self, device):
        """the table (T, sum of the widths) float32 on `device`"""
        return torch.cat([getattr(self.motion, k).to(device) for k, _, _ in self.fields], 1).contiguous()

    def unpack(self, table):
        """a table of this layout -> dict of every Motion field: its columns, None for a field the motion does not have"""
        got = dict.fromkeys(Motion.FIELDS)
        got.update(zip((k for k, _, _ in self.fields), table.split(self.widths, 1)))
        return got

    def trim(self, rot, vec):
        """the filter's per-channel trim distances as a list: `rot` for every rotation, `vec` for every vector, 0 (off) for cam"""
        return [float(rot or 0.0)] * self.n_rot + [float(vec or 0.0)] * self.n_vec + [0.0] * 3


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
    def _from_arm_result(cls, res, cam):
        """a solved arm result's in_pose (T,17,3) = [rot | wrist | pose(15)] and trans -> the Motion with wrist_pose"""
        return cls(res.in_pose[:, 2:].reshape(-1, 45), res.in_pose[:, 0], res.trans, cam, wrist_pose=res.in_pose[:, 1])

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
        NotImplementedError: Motion.from_arm_keypoints is that solver."""
        if "pose_mean" in hand_layer._model_np:
            raise NotImplementedError("Motion.from_keypoints solves the MANO hand; the SMPL-X arm needs a kinematic-tree solver: "
                                      "Motion.from_arm_keypoints")
        dev, up = _solve_on(device, params)
        a = K.ik_inputs(keypoints, weights, cam, init, params, hand_layer._model_np, match_bone_lengths, _window(smooth, dev))
        res = ops.mano_ik(_hand_device_model(hand_layer, dev), up(a["shape"]), up(a["keypoints"]), up(a["pose48"]), up(a["trans"]),
                          weights=up(a["weights"]), iters=iters, prior_weight=prior_weight)
        return cls(res.pose48[:, 3:], res.pose48[:, :3], res.trans, a["cam"])

    @classmethod
    def from_image_keypoints(cls, keypoints, params, hand_layer, cam=None, weights=None, depth=None, depth_weight=1.0, prior_weight=1e-5,
                             depth_prior_weight=2.5e-5, iters=20, init=None, smooth=None, device=None, configs=None):
        """A motion from IMAGE keypoints (a 2-D hand tracker run on a video) by batched reprojection inverse kinematics on the device
        (ops.mano_reproj_ik, csrc/reproj_ik.hip).  keypoints (T,21,2) in pixels of the fit's img_size, in the model's
        order — wrist, then thumb, index, middle, ring and little, each from root to tip — with the centre of column i at i + 0.5 and of
        row i at i + 0.5 of the frames the player renders; a joint with a non-finite coordinate or a weight <= 0 (weights (T,21), default
        ones) is ignored.  depth: None or (T,21) metres relative to the wrist along the view axis ("2.5-D"; NaN where there is none; the
        wrist's own entry is not read).  params: the fit's parameter dict (its `shape` is the avatar's and is not solved; row 0 of its
        `cam` is the default cam); cam: (3,) or (T,3); configs (required, by keyword): the fit's config, whose focal_length and img_size
        are the camera's, as the player reads them — a Motion has no other way to know them.
        The start (host, float64): pose zero and the TWO root rotations and translations that the palm's pixels allow
        (planar_palm_starts: a plane seen under weak perspective has a mirror pose); both go through ONE solve of 2 T problems and the
        one with the lower final cost is taken per frame on the device.  init= takes a Motion of equal length as the only candidate.
        The three weights are dimensionless: each is multiplied by (focal / Z_t)^2 with Z_t the start's palm depth, so that a weight of 1
        counts a metre (a radian) like focal / Z_t pixels: depth_weight on the depth rows, prior_weight on the pull of the finger pose
        to the model's mean pose (what it means in from_keypoints), depth_prior_weight on the pull of trans_z to the start's (depth
        along the view axis is what pixels determine worst).  The depth rows take their own frame's factor; the two priors are one
        number per launch and take the median of the frames' factors.  The float32 normal equations need the two priors (§30).
        There is no bone-length matching in 2-D: a larger hand simply reads as nearer.
        THE LIMIT: without `depth`, every finger bone has a towards / away mirror pose that pixels cannot tell apart, and the prior
        picks the one nearer the mean pose.  The reprojection is then right, but the 3-D pose is not unique (on the seeded
        scenes the joints are off by 6 .. 8 mm in the median and up to 89 mm while 70 of 72 frames agree to 2.4 px and all to 3.6 px).
        With depth rows the 3-D result is defined (0.9 .. 1.8 mm in the median, 8.9 mm at most).
        smooth: None, or the sigma in frames of a Gaussian window that the pixels (and depths) go through first (smooth_keypoints, with
        `weights` as the confidences); Motion.smooth filters the solved rows instead.  The result carries no light.  device: where the
        solve runs (default: the device of params["shape"] when that is a HIP device, else "cuda").  The SMPL-X arm needs a solver for
        its kinematic tree and raises NotImplementedError: Motion.from_arm_image_keypoints is that solver."""
        if "pose_mean" in hand_layer._model_np:
            raise NotImplementedError("Motion.from_image_keypoints solves the MANO hand; the SMPL-X arm needs a kinematic-tree solver: "
                                      "Motion.from_arm_image_keypoints")
        if configs is None or "focal_length" not in configs or "img_size" not in configs:
            raise ValueError("Motion.from_image_keypoints needs configs= with the fit's focal_length and img_size")
        focal, S = float(configs["focal_length"]), int(configs["img_size"])
        for name, v in (("depth_weight", depth_weight), ("prior_weight", prior_weight), ("depth_prior_weight", depth_prior_weight)):
            if not (0.0 <= float(v) < float("inf")):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        dev, up = _solve_on(device, params)
        a = K.image_ik_inputs(keypoints, weights, depth, cam, init, params, hand_layer._model_np, focal, S, _window(smooth, dev))
        T, C = a["pose48"].shape[:2]
        rep =lambda x: None if x is None else np.repeat(x, C, axis=0)      # frame-major: problem t * C + c
        scale = (focal / a["depth"]) ** 2                               # (T,) px^2 per squared metre (radian) at the start's palm depth
        res = ops.mano_reproj_ik(_hand_device_model(hand_layer, dev), up(a["shape"]), up(rep(a["targets"])),
                                 up(a["pose48"].reshape(T * C, 48)), up(a["trans"].reshape(T * C, 3)), up(rep(a["cam"])), focal, S,
                                 weights=up(rep(a["weights"])),
                                 depth_weights=None if depth is None else up(rep(np.broadcast_to((depth_weight * scale)[:, None], (T, 21)))),
                                 z_prior=up(a["trans"].reshape(T * C, 3)[:, 2]), iters=iters,
                                 pose_prior_weight=float(prior_weight * np.median(scale)), z_prior_weight=float(depth_prior_weight * np.median(scale)))
        pick = res.cost[:, 1].reshape(T, C).argmin(1, keepdim=True)      # the candidate with the lower final cost, on the device
        take = lambda rows: rows.reshape(T, C, -1).gather(1, pick[:, :, None].expand(T, 1, rows.shape[-1]))[:, 0]      # noqa: E731
        pose48, trans = take(res.pose48), take(res.trans)
        return cls(pose48[:, 3:], pose48[:, :3], trans, a["cam"])

    @classmethod
    def from_vertices(cls, vertices, params, hand_layer, cam=None, weights=None, iters=10, pose_prior_weight=0.0, init=None, device=None):
        """A motion from per-frame mesh vertices in MANO topology (a mesh regressor's output, a dataset) by the batched vertex fit on the
        device (ops.mano_vertex_fit, csrc/vertex_fit.hip).  vertices (T,778,3) in metres, in the frame of the fit's
        `verts`; a vertex with a non-finite coordinate or a weight <= 0 (weights (T,778), default ones) is ignored.  params: the fit's
        parameter dict — its `shape` is the avatar's and is held fixed, so someone else's hand drives the avatar with the avatar's own
        proportions; row 0 of its `cam` is the default cam; cam: (3,) or (T,3).
        The start: pose zero, the root rotation and trans from the weighted Kabsch fit of the model's vertices at that shape
        (vertex_start, host float64, one batched SVD); init= takes a Motion of equal length instead as a warm start.  pose_prior_weight
        pulls the finger pose to the model's mean pose (0: the plain vertex distance).  Every frame is solved on its own; Motion.smooth
        filters the result.  The result carries no light: AvatarPlayer.load_motion then uses the fit's row 0.  device: where the solve
        runs (default: the device of params["shape"] when that is a HIP device, else "cuda").  The SMPL-X arm needs a fit over its
        kinematic tree and raises NotImplementedError."""
        if "pose_mean" in hand_layer._model_np:
            raise NotImplementedError("Motion.from_vertices fits the MANO hand; the SMPL-X arm needs a fit over its kinematic tree: "
                                      "Motion.from_arm_vertices")
        dev, up = _solve_on(device, params)
        v = checked("vertices", vertices, (None, 778, 3), kind="f", split=True).astype(np.float64)
        T = v.shape[0]
        w = None if weights is None else checked("weights", weights, (T, 778), kind="f", split=True).astype(np.float64)
        K.check_init(init, T)
        cam, shape = K.frame_cam(cam, params, T), K.avatar_shape(params)
        dm = _hand_device_model(hand_layer, dev)
        targets, betas = up(v), up(shape)
        if init is None:
            # the model's vertices at this shape and zero stored pose: the solver's own forward, evaluated at the origin
            zero = ops.mano_vertex_fit(dm, targets[:1], up(np.zeros((1, 48))), betas, up(np.zeros((1, 3))), solve_shape=False, iters=0, verts=True)
            rot, trans = K.vertex_start(v, np.ones((T, 778)) if w is None else w, zero.verts[0].cpu().numpy().astype(np.float64) / 1000.0,
                                        K.rest_chain_joints(hand_layer._model_np, shape)[0])
            pose = np.zeros((T, 45))
        else:
            rot, trans, pose = K.init_rows(init)
        res = ops.mano_vertex_fit(dm, targets, up(np.concatenate([rot, pose], 1)), betas, up(trans), weights=up(w), solve_shape=False, iters=iters,
                                  pose_prior_weight=pose_prior_weight)
        return cls(res.pose48[:, 3:], res.pose48[:, :3], res.trans, cam)

    @classmethod
    def from_arm_vertices(cls, vertices, params, arm_layer, cam=None, weights=None, iters=10, pose_prior_weight=0.0, wrist_prior_weight=0.0,
                          wrist_pose=None, init=None, device=None):
        """A motion WITH wrist_pose for an SMPL-X arm avatar from per-frame mesh vertices, by the batched arm vertex fit on the device
        (ops.arm_vertex_fit, csrc/arm_vertex_fit.hip).  vertices in metres, in the frame of the fit's `verts`:
        (T,NV,3) (1026) in ARM topology — the wrist is solved; or (T,778,3) in MANO topology (a mesh regressor's output), matched to the arm's
        vertices arm_layer.right_mano_idx — the wrist is HELD at wrist_pose ((3,) or (T,3); default zeros, or init.wrist_pose): from hand
        vertices alone the root and the wrist rotation are nearly interchangeable.  wrist_pose is not taken with arm topology.  A vertex
        with a non-finite coordinate or a weight <= 0 (weights (T,n), default ones) is ignored.  params: the fit's parameter dict — its
        `shape` is the avatar's and is held fixed; row 0 of its `cam` is the default cam; cam: (3,) or (T,3).
        The start: wrist as held (or zero) and pose zero, the root rotation and trans from the weighted Kabsch fit of the model's vertices at
        that shape and wrist (vertex_start; the model is wrist-centred: it turns about the origin and trans is the wrist); init= takes a
        Motion of equal length with wrist_pose instead as a warm start.  pose_prior_weight pulls the finger pose to the model's mean pose,
        wrist_prior_weight the solved wrist to zero.  Every frame is solved on its own; Motion.smooth filters the result.  The result
        carries no light: AvatarPlayer.load_motion then uses the fit's row 0."""
        if "pose_mean" not in arm_layer._model_np:
            raise ValueError("Motion.from_arm_vertices fits the SMPL-X arm layer; Motion.from_vertices fits the MANO hand")
        dev, up = _solve_on(device, params)
        dm = _arm_device_model(arm_layer, dev)
        NV = int(dm.NV)
        n = int(np.shape(vertices)[1]) if np.ndim(vertices) == 3 else -1
        if n not in (NV, 778):
            raise ValueError(f"vertices must be (T, {NV}, 3) in arm topology or (T, 778, 3) in MANO topology, got {tuple(np.shape(vertices))}")
        arm_topology = n == NV
        v = checked("vertices", vertices, (None, n, 3), kind="f", split=True).astype(np.float64)
        T = v.shape[0]
        w = None if weights is None else checked("weights", weights, (T, n), kind="f", split=True).astype(np.float64)
        K.check_init(init, T, wrist=True)
        if arm_topology and wrist_pose is not None:
            raise ValueError("wrist_pose is what a fit to MANO-topology vertices holds the wrist at; arm-topology vertices solve it")
        cam, shape = K.frame_cam(cam, params, T), K.avatar_shape(params)
        idx = None if arm_topology else arm_layer.right_mano_idx.to(dev)
        targets, betas = up(v), up(shape)
        rows, trans = K.arm_start_rows(T, K.held_wrist(wrist_pose, init, T), init)
        if init is None:
            # the model's vertices at this shape and wrist with zero stored pose: the solver's own forward, evaluated at the origin
            zero = ops.arm_vertex_fit(dm, targets, up(rows), betas, up(trans), vert_idx=idx, solve_shape=False, iters=0, verts=True).verts
            rest = (zero if idx is None else zero[:, idx]).cpu().numpy().astype(np.float64) / 1000.0
            rows[:, 0], trans = K.vertex_start(v, np.ones((T, n)) if w is None else w, rest, np.zeros(3))
        res = ops.arm_vertex_fit(dm, targets, up(rows), betas, up(trans), vert_idx=idx, weights=up(w), solve_shape=False, solve_wrist=arm_topology,
                                 iters=iters, pose_prior_weight=pose_prior_weight, wrist_prior_weight=wrist_prior_weight)
        return cls._from_arm_result(res, cam)

    @classmethod
    def from_arm_keypoints(cls, keypoints, params, arm_layer, cam=None, weights=None, match_bone_lengths=True, iters=15, prior_weight=1e-5,
                           wrist_prior_weight=1e-4, wrist_pose=None, init=None, device=None, smooth=None):
        """A motion WITH wrist_pose for an SMPL-X arm avatar from 3-D keypoints (a hand tracker, a mocap glove, a body tracker that also
        gives the elbow) by batched inverse kinematics over the arm's joint tree on the device (ops.arm_ik, csrc/arm_ik.hip, DESIGN.md
        §29).  keypoints in metres, in the frame of the fit's `joints`:
        (T,22,3) — the 21 hand keypoints in the model's order (wrist, then thumb, index, middle, ring and little, each from root to tip)
        plus the ELBOW as row 21: the wrist is SOLVED, and wrist_pose ((3,) or (T,3); default zeros, or init.wrist_pose) is the centre
        of its prior (wrist_prior_weight); a frame whose elbow is missing is still solved, and the prior then decides its wrist;
        (T,21,3) — the hand only: the wrist is HELD at wrist_pose, because from hand points alone the root and the wrist rotation are
        interchangeable (§28 found the same for 778 vertices).
        A joint with a non-finite coordinate or a weight <= 0 (weights (T,n), default ones) is ignored.  params: the fit's parameter dict
        (its `shape` is the avatar's and is not solved; row 0 of its `cam` is the default cam); cam: (3,) or (T,3).
        The start: wrist as held (or the prior's centre) and pose zero, the root rotation and trans from the Kabsch fit of the model's palm
        joints and elbow (arm_palm_start; host float64, one batched SVD) onto the keypoints', the model's joints taken from the solver's
        own forward; init= takes a Motion of equal length with wrist_pose instead as a warm start.  match_bone_lengths scales the hand
        keypoints about their wrist so that their chain bones sum to the model's and puts the elbow on its ray from the wrist at the
        model's forearm length (match_arm_lengths): someone else's arm can drive the avatar.  prior_weight pulls the finger pose to the
        model's mean pose.  smooth: None, or the sigma in frames of a Gaussian window that the keypoints go through first
        (smooth_keypoints), as in from_keypoints.  Every frame is solved on its own; Motion.smooth filters the solved rows.
        What keypoints cannot see: with the joints matched to a fraction of a millimetre the recovered VERTICES can still differ from the
        true ones by centimetres — the twist of a finger's last bone and of the forearm about its own axis is not in 22 points; the
        priors decide it.  The result carries no light: AvatarPlayer.load_motion then uses the fit's row 0.  A MANO layer raises
        ValueError: Motion.from_keypoints solves that model."""
        if "pose_mean" not in arm_layer._model_np:
            raise ValueError("Motion.from_arm_keypoints solves the SMPL-X arm layer; Motion.from_keypoints solves the MANO hand")
        n = int(np.shape(keypoints)[1]) if np.ndim(keypoints) == 3 else -1
        if n not in (21, 22):
            raise ValueError(f"keypoints must be (T, 22, 3) with the elbow or (T, 21, 3) without, got {tuple(np.shape(keypoints))}")
        kp = checked("keypoints", keypoints, (None, n, 3), kind="f", split=True).astype(np.float64)
        T = kp.shape[0]
        w = None if weights is None else checked("weights", weights, (T, n), kind="f", split=True).astype(np.float64)
        K.check_init(init, T, wrist=True)
        cam, shape = K.frame_cam(cam, params, T), K.avatar_shape(params)
        wrist = K.held_wrist(wrist_pose, init, T)
        dev, up = _solve_on(device, params)
        kp, w = K.smoothed(_window(smooth, dev, n), kp, w)
        used = np.isfinite(kp).all(-1) & (True if w is None else (w > 0))
        if match_bone_lengths:
            kp, _ = K.match_arm_lengths(kp, used, K.rest_arm_joints(arm_layer._model_np, shape))
        dm = _arm_device_model(arm_layer, dev)
        # the hand alone is the 22-wide problem with the elbow unused and the wrist held
        tg = kp if n == 22 else np.concatenate([kp, np.full((T, 1, 3), np.nan)], 1)
        wt = used.astype(np.float64) if w is None else np.where(used, w, 0.0)
        wt = wt if n == 22 else np.concatenate([wt, np.zeros((T, 1))], 1)
        targets, betas = up(tg), up(shape)
        # (a solved wrist starts where init has it, whatever the centre of its prior)
        rows, trans = K.arm_start_rows(T, wrist if init is None or n == 21 else init.wrist_pose.cpu().numpy(), init)
        if init is None:
            # the model's joints at this shape and wrist with zero stored pose: the solver's own forward, evaluated at the origin
            zero = ops.arm_ik(dm, betas, targets, up(rows), up(trans), iters=0, joints=True).joints
            rows[:, 0], trans = K.arm_palm_start(kp, used, zero.cpu().numpy().astype(np.float64) / 1000.0)
        res = ops.arm_ik(dm, betas, targets, up(rows), up(trans), weights=up(wt), wrist_prior=up(wrist), solve_wrist=n == 22, iters=iters,
                         pose_prior_weight=prior_weight, wrist_prior_weight=wrist_prior_weight)
        return cls._from_arm_result(res, cam)

    @classmethod
    def from_arm_image_keypoints(cls, keypoints, params, arm_layer, cam=None, weights=None, depth=None, depth_weight=1.0, prior_weight=1e-5,
                                 wrist_prior_weight=1e-4, depth_prior_weight=2.5e-5, wrist_pose=None, iters=20, init=None, smooth=None,
                                 device=None, configs=None):
        """A motion WITH wrist_pose for an SMPL-X arm avatar from IMAGE keypoints (a 2-D hand or body tracker run on a video) by batched
        reprojection inverse kinematics over the arm's joint tree on the device (ops.arm_reproj_ik, csrc/arm_reproj_ik.hip, DESIGN.md
        §35).  keypoints in pixels of the fit's img_size, with the centre of column i at i + 0.5 and of row i at i + 0.5 of the frames the
        player renders:
        (T,22,2) — the 21 hand keypoints in the model's order (wrist, then thumb, index, middle, ring and little, each from root to tip)
        plus the ELBOW as row 21: the wrist is SOLVED, and wrist_pose ((3,) or (T,3); default zeros, or init.wrist_pose) is the centre
        of its prior (wrist_prior_weight); a frame whose elbow is missing is still solved, and the prior then decides its wrist;
        (T,21,2) — the hand only: the same launch with the elbow's weight 0 and the wrist HELD at wrist_pose.
        A joint with a non-finite coordinate or a weight <= 0 (weights (T,n), default ones) is ignored.  depth: None or (T,n) metres
        relative to the wrist along the view axis ("2.5-D"; NaN where there is none; the wrist's own entry is not read) — what a labelled
        arm playback writes into keypoints.npz beside the pixels.  params, cam, configs (required, by keyword): as
        Motion.from_image_keypoints takes them.
        The start: wrist as held (or the prior's centre) and pose zero; the model's joints there come from the solver's own forward, and
        rows 0..20 of them go to planar_palm_starts, which gives the TWO root rotations and translations that the palm's pixels allow; both
        go through ONE solve of 2 T problems and the one with the lower final cost is taken per frame on the device.  init= takes a Motion
        of equal length with wrist_pose as the only candidate.
        The four weights are dimensionless and multiplied by (focal / Z_t)^2 with Z_t the start's palm depth, as in
        from_image_keypoints: depth_weight on the depth rows (their own frame's factor), prior_weight on the pull of the finger pose to
        the model's mean pose, wrist_prior_weight on the pull of a solved wrist to wrist_pose, depth_prior_weight on the pull of trans_z
        to the start's (the three priors take the median of the frames' factors).  There is no bone-length matching in 2-D.
        THE LIMIT is from_image_keypoints': without `depth` the reprojection is right and the 3-D pose is not unique (on the
        seeded scenes the joints are off by 8 .. 13 mm in the median and up to 227 mm at under 3.2 px; with depth rows 1.2 .. 1.4 mm in
        the median and 7.1 mm at most).
        smooth: None, or the sigma in frames of a Gaussian window that the pixels (and depths) go through first (smooth_keypoints with
        joints=22).  The result carries no light.  A MANO layer raises ValueError: Motion.from_image_keypoints solves that model."""
        if "pose_mean" not in arm_layer._model_np:
            raise ValueError("Motion.from_arm_image_keypoints solves the SMPL-X arm layer; Motion.from_image_keypoints solves the MANO hand")
        if configs is None or "focal_length" not in configs or "img_size" not in configs:
            raise ValueError("Motion.from_arm_image_keypoints needs configs= with the fit's focal_length and img_size")
        focal, S = float(configs["focal_length"]), int(configs["img_size"])
        for name, v in (("depth_weight", depth_weight), ("prior_weight", prior_weight), ("wrist_prior_weight", wrist_prior_weight),
                        ("depth_prior_weight", depth_prior_weight)):
            if not (0.0 <= float(v) < float("inf")):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        dev, up = _solve_on(device, params)
        a = K.arm_image_ik_inputs(keypoints, weights, depth, cam, init, wrist_pose, params, _window(smooth, dev, 22))
        dm = _arm_device_model(arm_layer, dev)
        T = a["in_pose"].shape[0]
        betas = up(a["shape"])
        # the model's joints at this shape and wrist with zero stored pose (or at init): the solver's own forward, nothing solved
        zero = ops.arm_ik(dm, betas, up(np.zeros((T, 22, 3))), up(a["in_pose"]), up(a["trans"]), iters=0, joints=True).joints
        in_pose, trans, zbar = K.arm_image_starts(a, zero.cpu().numpy().astype(np.float64) / 1000.0, init, focal, S)
        C = in_pose.shape[1]
        rep = lambda x: np.repeat(x, C, axis=0)                          # frame-major: problem t * C + c
        scale = (focal / zbar) ** 2                                     # (T,) px^2 per squared metre (radian) at the start's palm depth
        med = float(np.median(scale))
        res = ops.arm_reproj_ik(dm, betas, up(rep(a["targets"])), up(in_pose.reshape(T * C, 17, 3)), up(trans.reshape(T * C, 3)),
                                up(rep(a["cam"])), focal, S, weights=up(rep(a["weights"])),
                                depth_weights=None if depth is None else up(rep(np.broadcast_to((depth_weight * scale)[:, None], (T, 22)))),
                                wrist_prior=up(rep(a["wrist"])), z_prior=up(trans.reshape(T * C, 3)[:, 2]), solve_wrist=a["solve_wrist"],
                                iters=iters, pose_prior_weight=prior_weight * med, wrist_prior_weight=wrist_prior_weight * med,
                                z_prior_weight=depth_prior_weight * med)
        pick = res.cost[:, 1].reshape(T, C).argmin(1, keepdim=True)      # the candidate with the lower final cost, on the device
        take = lambda rows, n: rows.reshape(T, C, n).gather(1, pick[:, :, None].expand(T, 1, n))[:, 0]      # noqa: E731
        return cls._from_arm_result(ops.ArmReprojIkResult(take(res.in_pose, 51).reshape(T, 17, 3), take(res.trans, 3), None, None, None, None),
                                    a["cam"])

    def save(self, path):
        np.savez(path, **{k: getattr(self, k).cpu().numpy() for k in self.FIELDS if getattr(self, k) is not None})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(**{k: z[k] for k in cls.FIELDS if k in z.files})

    def _table(self, hand_layer, device):
        """(the row layout, the packed table, the model's pose mean for its rotations), the last two on `device`"""
        lay = RowLayout(self)
        off = torch.as_tensor(pose_mean_rows(hand_layer, self.wrist_pose is not None), dtype=torch.float32).to(device)
        return lay, lay.pack(device), off

    def resample(self, times, hand_layer, device="cuda"):
        """The motion at `times` (n,) in units of its own frames, e.g. np.linspace(0, T - 1, n) to retime it to n frames: rotations along
        the shortest arc with the model's pose mean as the offset, trans / cam / light linearly (ops.motion_resample); a time on a frame
        returns that frame bit for bit."""
        dev = torch.device(device)
        lay, keys, off = self._table(hand_layer, dev)
        t = torch.as_tensor(np.asarray(times, dtype=np.float32)).reshape(-1).to(dev)
        return Motion(**lay.unpack(ops.motion_resample(keys, t, lay.n_rot, off)))

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
        T = len(self)
        lay, rows, off = self._table(hand_layer, dev)
        trim = None if trim_rot is None and trim_vec is None else torch.tensor(lay.trim(trim_rot, trim_vec), dtype=torch.float32).to(dev)
        w = None if weights is None else checked("weights", weights, (T,), tensor=True).to(torch.float32).contiguous().to(dev)
        seg = None if segments is None else _segment_ids(segments, T).to(dev)
        out, _ = ops.motion_filter(rows, lay.n_rot, lay.n_vec, ops.gaussian_taps(sigma, radius), weights=w, segment=seg, trim=trim, rot_offset=off,
                                   iters=iters)
        got = lay.unpack(out)
        return Motion(**{k: got[k] if k in fields or got[k] is None else getattr(self, k).clone() for k in self.FIELDS})


def _segment_ids(segments, T):
    return checked("segments", segments, (T,), kind="i", tensor=True).to(torch.int32).contiguous()


def smooth_keypoints(keypoints, weights=None, sigma=2.0, radius=None, trim=None, segments=None, device="cuda", joints=21):
    """(T,21,3) keypoints through the window filter as 21 vector channels (ops.motion_filter) -> (keypoints (T,21,3) float32,
    used (T,21) int32), both on `device`.  weights: None or (T,21) confidences.  A joint with a non-finite coordinate or a weight <= 0 has
    weight 0: it does not pull on its neighbours and is FILLED from them when any lie in the window (used > 0); with none it comes back as
    it went in (used == 0).  trim: None or a distance in the keypoints' unit for the trimmed second pass; segments: as Motion.smooth.
    joints=22: the SMPL-X arm's layout, the elbow as one more point row of the same call."""
    n = int(joints)
    kp = checked("keypoints", keypoints, (None, n, 3), kind="f", tensor=True).to(torch.float32)
    T = kp.shape[0]
    dev = torch.device(device)
    ok = torch.isfinite(kp).all(-1)
    if weights is None:
        w = ok.to(torch.float32)
    else:
        w = checked("weights", weights, (T, n), kind="f", tensor=True).to(torch.float32).to(kp.device)
        w = torch.where(ok & (w > 0) & torch.isfinite(w), w, torch.zeros_like(w))
    tr = None if trim is None else torch.full((n,), float(trim), dtype=torch.float32).to(dev)
    seg = None if segments is None else _segment_ids(segments, T).to(dev)
    out, used = ops.motion_filter(kp.reshape(T, 3 * n).contiguous().to(dev), 0, n, ops.gaussian_taps(sigma, radius), weights=w.contiguous().to(dev),
                                  segment=seg, trim=tr)
    return out.reshape(T, n, 3), used


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
