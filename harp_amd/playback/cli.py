"""The command line of the playback package: python -m harp_amd.playback (the package's docstring lists the options)."""
import numpy as np

from .. import ops
from .motion import Motion, motion_jitter
from .player import CONTACT_DIST, FLOW_TOL, LABEL_TOL, SELF_CONTACT_DIST, SELF_GEODESIC, AvatarPlayer, ScenePlayer


def parse_args(argv=None):
    """the command line's arguments, checked: what `main` runs on (SystemExit for a combination it does not take)"""
    import argparse
    from . import __doc__ as package_doc
    ap = argparse.ArgumentParser(prog="python -m harp_amd.playback", description=package_doc.split("\n\n")[0])
    ap.add_argument("--config", required=True, help="yaml with the keys of utils/config_utils.get_config (the fit's)")
    ap.add_argument("--motion", default=None, help=".npz of pose (T,45), rot, trans, cam (T,3) [, wrist_pose, light_positions] (Motion.save)")
    ap.add_argument("--keypoints", default=None, help=".npz of keypoints (T,21,3) in metres [, weights (T,21), cam (3,) or (T,3)] instead of --motion: "
                                                      "the motion is solved from them (Motion.from_keypoints); with a use_arm config (T,22,3) = "
                                                      "the 21 hand keypoints plus the elbow as row 21 (the wrist is solved) or (T,21,3) (the "
                                                      "wrist is held) [, weights (T,22) or (T,21), wrist_pose (3,) or (T,3)] "
                                                      "(Motion.from_arm_keypoints)")
    ap.add_argument("--keypoints2d", default=None, help=".npz of keypoints (T,21,2) in pixels of the fit's img_size [, weights (T,21), depth (T,21) "
                                                        "metres relative to the wrist, cam (3,) or (T,3)] instead of --motion: the motion is "
                                                        "solved from them by reprojection (Motion.from_image_keypoints); with a use_arm config "
                                                        "(T,22,2) = the 21 hand keypoints plus the elbow as row 21 (the wrist is solved) or "
                                                        "(T,21,2) (the wrist is held) [, weights and depth of that width, wrist_pose (3,) or "
                                                        "(T,3)] (Motion.from_arm_image_keypoints): what --labels writes for either avatar")
    ap.add_argument("--vertices", default=None, help=".npz of vertices (T,778,3) in metres, MANO topology [, weights (T,778), cam (3,) or (T,3)] "
                                                     "instead of --motion: the motion is fitted to them (Motion.from_vertices); with a use_arm "
                                                     "config (T,778,3) or the arm's (T,1026,3) [, wrist_pose (3,) or (T,3) for 778] "
                                                     "(Motion.from_arm_vertices)")
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
    ap.add_argument("--labels", action="store_true",
                    help="also write part_%%04d.png (the part of the hand), depth_%%04d.png (16-bit millimetres, what --scene-depth reads), "
                         "iuv_%%04d.png (part, u, v) and keypoints.npz per avatar (pixels, visibility, occluder, box: what --keypoints2d reads)")
    ap.add_argument("--label-tol", type=float, default=LABEL_TOL, metavar="M",
                    help="with --labels: a joint counts as visible when the nearest surface is no nearer than its depth minus M metres "
                         "(a joint lies under the skin)")
    ap.add_argument("--flow", choices=("fw", "bw", "both"), default=None,
                    help="also write the optical flow of every pixel's surface point to the next frame (fw: flow_%%04d.flo, Middlebury format), "
                         "to the previous frame (bw: flow_bw_%%04d.flo) or both, with flow_status_%%04d.png / flow_bw_status_%%04d.png (0 nothing, "
                         "1 not trackable, 2 leaves the image, 3 hidden in the other frame, 4 visible there)")
    ap.add_argument("--flow-tol", type=float, default=FLOW_TOL, metavar="M",
                    help="with --flow: a point counts as visible in the other frame when the nearest surface where it lands is no nearer than "
                         "its depth minus M metres")
    ap.add_argument("--contacts", action="store_true",
                    help="with --also: also write contacts.npz, per avatar and vertex the signed distance to the nearest other avatar's "
                         "surface (negative inside it), which avatar, face and part that is, and per frame the smallest distance and the "
                         "deepest penetration")
    ap.add_argument("--contact-dist", type=float, default=CONTACT_DIST, metavar="M",
                    help="with --contacts: a vertex farther than M metres from every other avatar has no contact")
    ap.add_argument("--self-contacts", action="store_true",
                    help="also write self_contacts.npz, per avatar and vertex the signed distance to the nearest face of the avatar's OWN "
                         "surface that lies beyond a geodesic radius of it (negative inside another part of the avatar), that face and its "
                         "part, which parts touch which (a pinch: thumb3 and index3) and per frame the smallest distance and the deepest "
                         "penetration; one avatar is enough")
    ap.add_argument("--self-contact-dist", type=float, default=SELF_CONTACT_DIST, metavar="M",
                    help="with --self-contacts: a vertex farther than M metres from every counting face of its avatar has no contact")
    ap.add_argument("--self-geodesic", type=float, default=SELF_GEODESIC, metavar="M",
                    help="with --self-contacts: the faces within M metres of a vertex along the mesh's edges do not count for it; above "
                         "--self-contact-dist")
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
    if not args.label_tol >= 0:
        raise SystemExit("--label-tol must not be negative")
    if not (args.flow_tol >= 0 and np.isfinite(args.flow_tol)):
        raise SystemExit("--flow-tol must not be negative and must be finite")
    if not args.contact_dist >= 0:
        raise SystemExit("--contact-dist must not be negative")
    if args.contacts and not args.also:
        raise SystemExit("--contacts needs a second avatar: give --also CFG:MOTION[:flip]")
    if args.self_contacts and not (args.self_contact_dist >= 0 and np.isfinite(args.self_contact_dist)):
        raise SystemExit("--self-contact-dist must not be negative and must be finite")
    if args.self_contacts and not args.self_geodesic > args.self_contact_dist:
        raise SystemExit("--self-geodesic must exceed --self-contact-dist")
    if args.smooth_trim is not None and args.smooth is None:
        raise SystemExit("--smooth-trim needs --smooth")
    if args.smooth_keypoints is not None and args.keypoints is None:
        raise SystemExit("--smooth-keypoints needs --keypoints")
    if len(args.also) > ops.COMPOSITE_MAX_LAYERS - 1:
        raise SystemExit(f"--also at most {ops.COMPOSITE_MAX_LAYERS - 1} times")
    if args.fps_scale <= 0:
        raise SystemExit("--fps-scale must be positive")
    if sum(v is not None for v in (args.motion, args.keypoints, args.keypoints2d, args.vertices)) != 1:
        raise SystemExit("exactly one of --motion, --keypoints, --keypoints2d and --vertices")
    return args


def main(argv=None):
    """A fit (the saved_params[_test].pkl under the config's base_output_dir, as the evaluation reads it) plus a motion file -> a directory
    of frames."""
    args = parse_args(argv)
    import yaml
    from ..utils import file_utils, hand_model_utils
    from ..utils.config_utils import get_config

    def load(cfg_path, motion_path, keypoints_path=None, vertices_path=None, keypoints2d_path=None):
        with open(cfg_path) as f:
            configs = get_config(write_yaml=False, **yaml.safe_load(f))
        configs["device"] = args.device
        hand_layer, VERTS_UVS, FACES_UVS, _ = hand_model_utils.load_hand_model(configs)
        params = file_utils.load_result(configs["base_output_dir"], device=args.device, test=bool(configs["known_appearance"]))
        params["verts_uvs"], params["faces_uvs"] = VERTS_UVS, FACES_UVS
        if keypoints_path is not None:
            with np.load(keypoints_path) as z:
                opt = lambda k: z[k] if k in z.files else None            # noqa: E731
                if "pose_mean" in hand_layer._model_np:                     # the SMPL-X arm (use_arm)
                    motion = Motion.from_arm_keypoints(z["keypoints"], params, hand_layer, cam=opt("cam"), weights=opt("weights"),
                                                       wrist_pose=opt("wrist_pose"), device=args.device, smooth=args.smooth_keypoints)
                else:
                    motion = Motion.from_keypoints(z["keypoints"], params, hand_layer, cam=opt("cam"), weights=opt("weights"),
                                                   device=args.device, smooth=args.smooth_keypoints)
        elif keypoints2d_path is not None:
            with np.load(keypoints2d_path) as z:
                opt = lambda k: z[k] if k in z.files else None            # noqa: E731
                if "pose_mean" in hand_layer._model_np:                     # the SMPL-X arm (use_arm)
                    motion = Motion.from_arm_image_keypoints(z["keypoints"], params, hand_layer, cam=opt("cam"), weights=opt("weights"),
                                                             depth=opt("depth"), wrist_pose=opt("wrist_pose"), device=args.device,
                                                             configs=configs)
                else:
                    motion = Motion.from_image_keypoints(z["keypoints"], params, hand_layer, cam=opt("cam"), weights=opt("weights"),
                                                         depth=opt("depth"), device=args.device, configs=configs)
        elif vertices_path is not None:
            with np.load(vertices_path) as z:
                opt = lambda k: z[k] if k in z.files else None            # noqa: E731
                if "pose_mean" in hand_layer._model_np:                     # the SMPL-X arm (use_arm)
                    motion = Motion.from_arm_vertices(z["vertices"], params, hand_layer, cam=opt("cam"), weights=opt("weights"),
                                                      wrist_pose=opt("wrist_pose"), device=args.device)
                else:
                    motion = Motion.from_vertices(z["vertices"], params, hand_layer, cam=opt("cam"), weights=opt("weights"), device=args.device)
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
        configs, params, hand_layer, motion = load(args.config, args.motion, args.keypoints, args.vertices, args.keypoints2d)
        player = AvatarPlayer(configs, params, hand_layer, batch_size=args.batch_size, ss=args.ss, device=args.device, keep_depth=args.labels or args.flow is not None)
        paths = player.play(motion, args.out, backgrounds=args.background, fmt=fmt, alpha=args.alpha, labels=args.labels, label_tol=args.label_tol,
                            flow=args.flow, flow_tol=args.flow_tol, self_contacts=args.self_contacts, self_contact_dist=args.self_contact_dist,
                            self_geodesic=args.self_geodesic)
    else:
        specs = [(args.config, args.motion, args.flip, args.keypoints, args.vertices, args.keypoints2d)]
        for spec in args.also:
            part = spec.split(":")
            if len(part) not in (2, 3) or (len(part) == 3 and part[2] != "flip"):
                raise SystemExit(f"--also takes CFG:MOTION or CFG:MOTION:flip, got {spec!r}")
            specs.append((part[0], part[1], len(part) == 3, None, None, None))
        players, motions = [], []
        for cfg_path, motion_path, _, keypoints_path, vertices_path, keypoints2d_path in specs:
            configs, params, hand_layer, motion = load(cfg_path, motion_path, keypoints_path, vertices_path, keypoints2d_path)
            players.append(AvatarPlayer(configs, params, hand_layer, batch_size=args.batch_size, ss=args.ss, device=args.device, keep_depth=True))
            motions.append(motion)
        scene = ScenePlayer(players, flip=[spec[2] for spec in specs])
        paths = scene.play(motions, args.out, backgrounds=args.background, scene_depth=args.scene_depth, fmt=fmt, alpha=args.alpha, masks=args.masks,
                           labels=args.labels, label_tol=args.label_tol, flow=args.flow, flow_tol=args.flow_tol, contacts=args.contacts,
                           contact_dist=args.contact_dist, self_contacts=args.self_contacts, self_contact_dist=args.self_contact_dist,
                           self_geodesic=args.self_geodesic)
    print(f"wrote {len(paths)} frames to {args.out}")
    return paths
