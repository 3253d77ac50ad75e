"""The two forward-only renderers on one base.  `_Player` owns what a render call and a play loop need whatever is drawn:
the index stage, the copies of the caller's tensors, the output buffer, the graphs and the double-buffered way to disk.  `AvatarPlayer`
adds one avatar's launches and the resolve (§22), `ScenePlayer` several avatars and the composite (§23)."""
import collections
import ctypes
import os

import numpy as np
import torch

from .. import _lib, ops
from .keypoints import checked

BG_WHITE = (1.0, 1.0, 1.0)                             # the reference's BlendParams background (renderer_helper.py:49)
LABEL_TOL = 0.02                                       # metres: how far under the nearest surface a joint still counts as visible
# what annotate() returns: device tensors over the rows asked for, views of the player's buffers that the next annotate
# overwrites (bbox is computed from one); None for a map that was not asked for.  owner, part (n,S,S) uint8; depth (n,S,S) float32 view
# depth in metres, 0 = empty; face (n,S,S) int32, -1 = empty; uv (n,S,S,2) float32; bbox (xmin, ymin, xmax, ymax) int32, -1 = nothing:
# (n,4) of an AvatarPlayer, (n,P,4) of a scene of P players; uvz (n,NJ,3) float32 = (u, v, view depth) and vis (n,NJ,2) uint8 =
# (0 not in the image | 1 hidden | 2 visible, the occluder: 0 nothing, 1 + the player, 255 the scene depth) — of a scene, one per player
Annotation = collections.namedtuple("Annotation", "owner part depth face uv bbox uvz vis")
FLOW_TOL = ops.FLOW_TOL                                # metres: how far under the nearest target surface a tracked surface point still counts as visible
# what flow() returns: device tensors over the rows asked for, views of the player's buffers that the next flow overwrites.
# flow (n,S,S,2) float32: where the surface point a pixel shows lies in the target frame, minus the pixel's own place, in output pixels
# (x, y); dz (n,S,S) float32: its view depth there minus its depth here, metres; status (n,S,S,2) uint8 = (0 nothing | 1 not trackable |
# 2 lands outside the image | 3 hidden at the target | 4 visible there, what hides it: 0 nothing, 1 + the player, 255 the scene depth)
Flow = collections.namedtuple("Flow", "flow dz status")
CONTACT_DIST = 0.02                                    # metres: how near another avatar's surface counts as contact; about a finger's thickness
# what ScenePlayer.contact returns: per player k a device tensor over the rows asked for and its V_k vertices, in tuples
# with one entry per player.  dist (n,V_k) float32, SIGNED: the distance to the nearest other player's surface, negative where the vertex
# is inside it (wind > 0.5), +inf beyond max_dist; other (n,V_k) uint8: 0 none, 1 + that nearest player; face (n,V_k) int32: the face of
# it that is touched, -1 none; part (n,V_k) uint8: that face's part (face_part_labels), 0 none; wind (n,V_k) float32: the winding number
# of that player's surface about the vertex.  Per frame: min_dist (n,) float32, the smallest signed distance of any vertex (+inf: no
# contact), and max_penetration (n,) float32, the largest -dist over the inside vertices, or 0.  Unlike Annotation and Flow, every tensor
# is new (compose_contact): a later contact() does not change an earlier result
Contact = collections.namedtuple("Contact", "dist other face part wind min_dist max_penetration")


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with status {rc}")


def _host_rows(name, rows, n=None):
    r = checked(name, rows).astype(np.int64).reshape(-1)
    if n is not None and r.shape[0] != n:
        raise ValueError(f"{name} must have one entry per row")
    return r


def stage_table(rows, n_pad, inputs=()):
    """The index table of one render call, on the host: rows (n,) of the motion and, per staged input, (its rows (n,) or None when the
    call does not use it, the N rows of the caller's tensor) -> int32 (1 + 2 len(inputs), n_pad).  Row 0: the motion's row of every
    frame; per input its SLOT in the player's copy (the frame's own index; -1 for a row outside [0, N): the constant colour, no depth) and
    the SOURCE row of the caller's tensor that is copied there (0 where there is none).  A short last batch is padded with its last row."""
    n = len(rows)
    tab = np.zeros((1 + 2 * len(inputs), n_pad), np.int32)
    tab[0, :n], tab[0, n:] = rows, rows[-1]
    for k, (rr, N) in enumerate(inputs):
        if rr is not None:
            inside = (rr >= 0) & (rr < N)
            tab[1 + 2 * k, :n], tab[1 + 2 * k, n:] = np.where(inside, np.arange(n), -1), (n - 1 if inside[-1] else -1)
            tab[2 + 2 * k, :n], tab[2 + 2 * k, n:] = np.where(inside, rr, 0), (rr[-1] if inside[-1] else 0)
    return tab


class _Player:
    """What AvatarPlayer and ScenePlayer share.  A subclass declares the caller tensors it stages (`_inputs`: name, per-row shape, dtype)
    and supplies `_enqueue(n_pad, channels, *flags)`, the launches of a whole call in order on the current stream; `flags` begins with one
    bool per staged input.  Nothing is allocated after the constructor except when a longer `rows` is first seen (`_grow`)."""

    _holds = "the motion holds"

    def __init__(self, device, S, ss, B, use_graph, inputs):
        self.dev, self.S, self.ss, self.B, self.use_graph = torch.device(device), S, ss, B, bool(use_graph)
        self._inputs = inputs
        self.T = self._n_cap = 0
        self.idx_done, self._bufs, self._graphs = None, {}, {}
        self._flow = None                                # what flow() adds, allocated on its first call (_grow_flow)
        self.bg_color_dev = torch.empty(3, dtype=torch.float32, device=self.dev)
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

    def _device(self):
        return self.dev if self.dev.index is not None else torch.device(self.dev.type, torch.cuda.current_device())

    def _grow(self, n_pad, used):
        if n_pad > self._n_cap:
            # per rendered frame: its row of the motion, then per staged input its row of the player's copy (-1: none) and the row of the
            # caller's tensor that is copied there (stage_table); staged in pinned memory and uploaded in one copy per call
            rows = 1 + 2 * len(self._inputs)
            self.idx_dev = torch.zeros(rows, n_pad, dtype=torch.int32, device=self.dev)
            self.idx_pin = torch.zeros(rows, n_pad, dtype=torch.int32).pin_memory()
            self.idx_done = None
            self.out = torch.empty(n_pad * self.S * self.S * 4, dtype=torch.uint8, device=self.dev)
            self._n_cap, self._bufs, self._graphs = n_pad, {}, {}
        for (name, shape, dtype), u in zip(self._inputs, used):
            if u and name not in self._bufs:             # (no graph reads it yet)
                self._bufs[name] = torch.empty(self._n_cap, *shape, dtype=dtype, device=self.dev)

    def _staged(self, name, t, rows, n, shape, dtype):
        """a (N, *shape) device tensor of the caller's and its rows -> (the rows checked, N), or (None, 0) without the tensor"""
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

    def _upload(self, table, tensors, n):
        """the index table to the device in one copy, then the rows in use of every caller tensor into the player's copy, in stream order"""
        if self.idx_done is not None:
            self.idx_done.synchronize()                  # the previous call's upload has read the staging buffer
        self.idx_pin.numpy()[:, :table.shape[1]] = table
        self.idx_dev.copy_(self.idx_pin, non_blocking=True)
        self.idx_done = torch.cuda.Event()
        self.idx_done.record()
        for k, ((name, _, _), t) in enumerate(zip(self._inputs, tensors)):
            if t is not None:
                torch.index_select(t, 0, self.idx_dev[2 + 2 * k, :n], out=self._bufs[name][:n])

    def _grow_flow(self, n_inputs, used):
        """What flow() needs beside render's buffers, allocated on its first call and again when a longer `rows` has grown the player: the
        index table of the TARGET rows (stage_table's layout over n_inputs staged inputs, beside idx_dev, which keeps its own) with its
        pinned stage, the three outputs, and a copy of its own for every staged input the target rows use"""
        if self._flow is None or self._flow["cap"] != self._n_cap:
            n, S, rows = self._n_cap, self.S, 1 + 2 * n_inputs
            new = lambda dt, *shape: torch.empty(n, *shape, dtype=dt, device=self.dev)      # noqa: E731
            self._flow = dict(cap=n, idx_dev=torch.zeros(rows, n, dtype=torch.int32, device=self.dev),
                              idx_pin=torch.zeros(rows, n, dtype=torch.int32).pin_memory(), flow=new(torch.float32, S, S, 2),
                              dz=new(torch.float32, S, S), status=new(torch.uint8, S, S, 2), bufs={})
        for (name, shape, dtype), u in zip(self._inputs[len(self._inputs) - n_inputs:], used):
            if u and name not in self._flow["bufs"]:     # (no graph reads it yet)
                self._flow["bufs"][name] = torch.empty(self._n_cap, *shape, dtype=dtype, device=self.dev)

    def _upload_to(self, table, tensors, n):
        """_upload for the target rows' table, enqueued in front of it: the event that _upload records covers both copies"""
        fl = self._flow
        if self.idx_done is not None:
            self.idx_done.synchronize()
        fl["idx_pin"].numpy()[:, :table.shape[1]] = table
        fl["idx_dev"].copy_(fl["idx_pin"], non_blocking=True)
        for k, ((name, _, _), t) in enumerate(zip(self._inputs[len(self._inputs) - len(tensors):], tensors)):
            if t is not None:
                torch.index_select(t, 0, fl["idx_dev"][2 + 2 * k, :n], out=fl["bufs"][name][:n])

    def _staged_to_args(self, k, name, lo, used):
        """_staged_args of the target rows' copy of staged input `name`, k-th of the target table"""
        if not used:
            return None, 0, None
        return self._flow["bufs"][name].data_ptr(), self._n_cap, self._flow["idx_dev"][1 + 2 * k, lo:lo + self.B].data_ptr()

    def _flow_view(self, n):
        return Flow(self._flow["flow"][:n], self._flow["dz"][:n], self._flow["status"][:n])

    def _run(self, key):
        """_enqueue(*key) as it is, or as the replay of its graph, captured when the key is first seen"""
        if not self.use_graph:
            return self._enqueue(*key)
        g = self._graphs.get(key)
        if g is None:
            # warm-up (the first launches size their LDS with runtime calls that a capture does not allow), then capture; on the
            # current stream: the sequence allocates nothing and has no branches, and the player takes no stream from torch's pool
            self._enqueue(*key)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._enqueue(*key)
            self._graphs[key] = g
        g.replay()

    def _staged_args(self, k, lo, used):
        """what a kernel takes of staged input k for the batch at `lo`: (the player's copy, its rows, the batch's slots), or (None, 0, None)"""
        if not used:
            return None, 0, None
        return self._bufs[self._inputs[k][0]].data_ptr(), self._n_cap, self.idx_dev[1 + 2 * k, lo:lo + self.B].data_ptr()

    def _render(self, rows, alpha, inputs, *flags, to=None):
        """The render path of both players: `rows` checked on the host, padded to whole batches, staged with `inputs` (per declared input
        the caller's (tensor, rows)), and enqueued or replayed under the key (padded length, channels, input used?..., *flags)
        -> (frames (n, S, S, channels), n).  to (flow only): (the target rows, [the caller's (tensor, rows) of the staged inputs the target
        frames use, the last of the declared ones]); they travel in a table of their own (_grow_flow)."""
        r = _host_rows("rows", rows)
        n = r.shape[0]
        if n < 1:
            raise ValueError("no rows to render")
        if r.min() < 0 or r.max() >= self.T:             # (on the host, before anything is enqueued: the kernels gather rows unchecked)
            raise IndexError(f"rows span [{r.min()}, {r.max()}] but {self._holds} {self.T} frames")
        C = 4 if alpha else 3
        staged = [self._staged(name, t, rr, n, shape, dtype) for (name, shape, dtype), (t, rr) in zip(self._inputs, inputs)]
        used = tuple(rr is not None for rr, _ in staged)
        n_pad = -(-n // self.B) * self.B
        if to is not None:
            r_to = _host_rows("to_rows", to[0], n)
            if r_to.min() < 0 or r_to.max() >= self.T:
                raise IndexError(f"to_rows span [{r_to.min()}, {r_to.max()}] but {self._holds} {self.T} frames")
            decl = self._inputs[len(self._inputs) - len(to[1]):]
            staged_to = [self._staged(name, t, rr, n, shape, dtype) for (name, shape, dtype), (t, rr) in zip(decl, to[1])]
        with torch.cuda.device(self.dev):
            self._grow(n_pad, used)
            if to is not None:
                self._grow_flow(len(staged_to), [rr is not None for rr, _ in staged_to])
                self._upload_to(stage_table(r_to, n_pad, staged_to), [t for t, _ in to[1]], n)
            self._upload(stage_table(r, n_pad, staged), [t for t, _ in inputs], n)
            self._run((n_pad, C) + used + flags)
        return self.out[:n * self.S * self.S * C].view(n, self.S, self.S, C), n

    def _play(self, out_dir, fmt, alpha, prepare, masks=False):
        """The way to disk of both players: the format checked, out_dir made, then render = prepare() (which loads the motion and the
        caller's inputs) called batch by batch: render(rows) -> frames, or (frames, owner) with masks.  Each leaves through a pinned host
        buffer of its own, two of each for the two batches in flight, and is encoded on a thread pool while the next batch renders."""
        from concurrent.futures import ThreadPoolExecutor
        from ..utils.data_util import default_workers
        if fmt not in ("jpg", "png") or (alpha and fmt != "png"):
            raise ValueError(f'fmt is "jpg" or "png", and alpha=True needs "png"; got {fmt!r}, alpha={alpha}')
        os.makedirs(out_dir, exist_ok=True)
        render = prepare()
        T, B, S = self.T, self.B, self.S
        pin = lambda *shape: torch.empty(*shape, dtype=torch.uint8).pin_memory()      # noqa: E731
        pinned = [[pin(B, S, S, 4 if alpha else 3)] + ([pin(B, S, S)] if masks else []) for _ in range(2)]
        pending = [[], []]
        paths = [os.path.join(out_dir, "%04d.%s" % (i, fmt)) for i in range(T)]
        with ThreadPoolExecutor(max(1, min(8, default_workers()))) as pool:
            for k, lo in enumerate(range(0, T, B)):
                rows = np.arange(lo, min(T, lo + B))
                for fut in pending[k % 2]:                # the buffers' previous frames are on disk
                    fut.result()
                got = render(rows)
                host = [h[:len(rows)] for h in pinned[k % 2]]
                for h, g in zip(host, got if masks else (got,)):
                    h.copy_(g, non_blocking=True)
                done = torch.cuda.Event()
                done.record()
                done.synchronize()
                arr = [h.numpy() for h in host]
                pending[k % 2] = [pool.submit(_encode, paths[i], arr[0][i - lo], fmt) for i in rows]
                if masks:
                    pending[k % 2] += [pool.submit(_encode, os.path.join(out_dir, "mask_%04d.png" % i), arr[1][i - lo], "png") for i in rows]
            for futs in pending:
                for fut in futs:
                    fut.result()
        return paths


class AvatarPlayer(_Player):
    """Forward-only renderer of a fitted avatar.  configs: the fit's (img_size, focal_length, use_arm, self_shadow,
    share_light_position); params: its parameter dict (verts_disps, shape, texture, normal_map, amb_ratio, light_positions, verts_uvs,
    faces_uvs are read once, here); ss: supersampling factor 1..4 — the avatar is rasterised and shaded at img_size * ss with the focal
    length scaled alike and box-filtered down by the resolve.  Every device buffer is allocated here (or when a longer motion or a longer
    `rows` is first seen); a call only enqueues.  keep_depth=True also keeps the camera view's depth map (s["z_c"], (B, S ss, S ss) view-space z,
    -1 where empty), which a ScenePlayer needs; without it not one launch argument differs."""

    def __init__(self, configs, params, hand_layer, batch_size=32, ss=1, use_graph=True, device="cuda", keep_depth=False):
        from ..synth import build_topology
        S, ss_, B = int(configs["img_size"]), int(ss), int(batch_size)
        if not 1 <= ss_ <= ops.RESOLVE_MAX_SS or B < 1 or S < 1:
            raise ValueError(f"ss in 1..{ops.RESOLVE_MAX_SS}, batch_size >= 1 and img_size >= 1, got {ss}, {batch_size}, {configs['img_size']}")
        super().__init__(device, S, ss_, B, use_graph, (("background", (S, S, 3), torch.uint8),))
        self.keep_depth = bool(keep_depth)             # the camera view's depth s["z_c"] is kept: a ScenePlayer composites by it
        self.Sh, self.focal_h = self.S * self.ss, float(configs["focal_length"]) * self.ss      # what is rasterised and shaded
        self.use_arm, self.self_shadow = bool(configs["use_arm"]), bool(configs["self_shadow"])
        self.share_light = bool(configs["share_light_position"])
        faces0 = np.asarray((hand_layer.right_arm_faces_tensor if self.use_arm else hand_layer.th_faces).detach().cpu())
        self.topo = ops.DeviceTopology(build_topology(faces0, 1026 if self.use_arm else 778), params["verts_uvs"], params["faces_uvs"], self.dev)
        if self.topo.V > _lib.lib().harp_mesh_chain_max_vertices():
            raise ValueError(f"the fused front takes meshes of at most {_lib.lib().harp_mesh_chain_max_vertices()} vertices, got {self.topo.V}")
        if self.use_arm:
            from ..hand_models_harp.body_models import TreeDeviceModel
            self.dm = TreeDeviceModel(hand_layer._model_np, self.dev)
            self.n_joints, self.pose_stride, self.n_betas = 22, 51, self.dm.NB
            self._weights_T = self.dm.weights.t().contiguous()
        else:
            from ..manopth.manolayer import ManoDeviceModel
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
        self._cap = 0
        self.tab = self.tables = None
        self._skin_weights = np.asarray(hand_layer._model_np["weights"])      # (V0, NJ): the part table is made from it on first use
        self._face_label, self._labels_wanted, self.lab, self.kp = None, False, None, None
        self.s_to = None                                 # the target frames' ndc_c and z_c of a batch, allocated on the first flow()

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

    def _render_batch(self, fid, shade=True, front_only=False):
        """front, rasterisers and shader of one batch of B frames, in order on the current stream: s["rgb"], s["face_c"] (and s["z_c"]
        with keep_depth) at S * ss, everything in front of the resolve; shade=False stops before the shader (labels need no colour),
        front_only=True after the front (contacts need the vertices s["vd"] and the camera only)"""
        L, s, p, tp, st = _lib.lib(), self.s, _lib.ptr, self.topo, _lib.stream()
        B, V, F, Sh = self.B, tp.V, tp.F, self.Sh
        z_c = p(s["z_c"]) if self.keep_depth else None
        h = self._front_struct(fid)
        _ck((L.harp_arm_front_fwd if self.use_arm else L.harp_hand_front_fwd)(ctypes.byref(h), st), "front_fwd")
        if front_only:
            return
        if self.self_shadow:
            _ck(L.harp_raster_setup_pair(p(s["ndc_c"]), 0.0, p(s["ws_c"]), p(s["ndc_l"]), 0.0, p(s["ws_l"]), p(tp.faces), B, V, F, Sh, st),
                "raster_setup_pair")
            _ck(L.harp_rasterize_fwd(p(s["ndc_c"]), p(tp.faces), B, V, F, Sh, 4, 0.0, 1.0, p(s["ws_c"]), p(s["face_c"]), z_c, None, st), "raster_cam")
            _ck(L.harp_rasterize_fwd_keep(p(s["ndc_l"]), p(tp.faces), B, V, F, Sh, 4, p(s["ws_l"]), p(s["face_l"]), p(s["zl"]), p(s["zl_state"]), st),
                "raster_light")
        else:                                            # one view: the rasteriser's own set-up
            _ck(L.harp_rasterize_fwd(p(s["ndc_c"]), p(tp.faces), B, V, F, Sh, 0, 0.0, 1.0, p(s["ws_c"]), p(s["face_c"]), z_c, None, st), "raster_cam")
        if shade:
            _ck(L.harp_shade_fwd(ctypes.byref(self._shade_struct()), st), "shade_fwd")

    # ---- labels ---------------------------------------------------------------------------------------------------
    def _part_table(self):
        """the part of every face on the device, made on first use (host integer work, once per player)"""
        if self._face_label is None:
            from .labels import face_part_labels
            tab = face_part_labels(self._skin_weights, self.topo.faces0.cpu().numpy(), self.topo.V0)
            if tab.shape[0] != self.topo.F:
                raise RuntimeError(f"{tab.shape[0]} part labels for {self.topo.F} faces")
            self._face_label = torch.from_numpy(tab).to(self.dev)
        return self._face_label

    def _label_layer(self, flip, uv):
        """this player's harp_label_layer over its batch buffers (annotate() has made the part table)"""
        s, p, tp = self.s, _lib.ptr, self.topo
        a = _lib.LabelLayer(face_id=p(s["face_c"]), zbuf=p(s["z_c"]), face_label=p(self._face_label), F=tp.F, flip_x=int(flip), reserved=0)
        if uv:
            a.ndc, a.faces, a.verts_uvs, a.faces_uvs, a.V, a.Vt = p(s["ndc_c"]), p(tp.faces), p(tp.verts_uvs), p(tp.faces_uvs), tp.V, tp.verts_uvs.shape[0]
        return a

    def _flow_layer(self, flip):
        """this player's harp_flow_layer over its batch buffers and its copies of the target frames' (flow() has made them)"""
        s, p, tp = self.s, _lib.ptr, self.topo
        return _lib.FlowLayer(face_id=p(s["face_c"]), zbuf=p(s["z_c"]), face_label=p(self._face_label), ndc=p(s["ndc_c"]), faces=p(tp.faces),
                              ndc_to=p(self.s_to["ndc"]), zbuf_to=p(self.s_to["z"]), V=tp.V, F=tp.F, flip_x=int(flip), reserved=0)

    def _flow_targets(self):
        """the copies of a batch's ndc_c and z_c that hold the target frames while the source frames are rendered, made once"""
        if self.s_to is None:
            self.s_to = dict(ndc=torch.empty_like(self.s["ndc_c"]), z=torch.empty_like(self.s["z_c"]))
        self._part_table()

    def _keep_targets(self):
        """the batch just rendered is the flow's target: device copies of its ndc_c and z_c, in stream order"""
        self.s_to["ndc"].copy_(self.s["ndc_c"])
        self.s_to["z"].copy_(self.s["z_c"])

    def _contact_mesh(self, flip):
        """this player's side of a harp_mesh_contact over its batch buffers"""
        s, p, tp = self.s, _lib.ptr, self.topo
        return _lib.ContactMesh(verts=p(s["vd"]), cam_R=p(s["cam_R"]), cam_T=p(s["cam_T"]), faces=p(tp.faces), V=tp.V, F=tp.F, flip_x=int(flip),
                                reserved=0)

    def _keypoint_buffers(self, n):
        """(uvz, vis) for n frames of this player's joints; whoever runs the launches owns them (the player itself, or its scene)"""
        return dict(uvz=torch.empty(n, self.n_joints, 3, dtype=torch.float32, device=self.dev),
                    vis=torch.empty(n, self.n_joints, 2, dtype=torch.uint8, device=self.dev))

    def _enqueue_keypoints(self, kp, lo, layers, n_layers, self_layer, scene, tol):
        """harp_keypoint_visibility of this player's batch into rows lo.. of the buffers kp; scene: _staged_args of the scene depth"""
        s, p = self.s, _lib.ptr
        _ck(_lib.lib().harp_keypoint_visibility(p(s["joints_m"]), p(s["cam_R"]), p(s["cam_T"]), self.B, self.n_joints, self.focal_h / self.ss, self.S,
                                                self.ss, self_layer, layers, n_layers, *scene, tol, kp["uvz"][lo:].data_ptr(),
                                                kp["vis"][lo:].data_ptr(), _lib.stream()), "keypoint_visibility")

    def _grow(self, n_pad, used):
        grew = n_pad > self._n_cap
        super()._grow(n_pad, used)
        if grew:
            self.lab = None
        if self._labels_wanted and self.lab is None:
            self.lab = _label_buffers(self._n_cap, self.S, 1, self.dev)
            self.kp = self._keypoint_buffers(self._n_cap)

    def _enqueue(self, n_pad, channels, with_bg, labels=None, flow=None):
        """per batch of B frames: its launches up to the shader, then the resolve; with labels = (part, depth, uv, keypoints, tol) the
        launches up to the rasterisers, then the labels of the batch; with flow = ("flow", tol) the launches up to the rasterisers of the
        TARGET rows, copies of their ndc_c and z_c, the same of the source rows, then the flow of the batch"""
        L, s, p = _lib.lib(), self.s, _lib.ptr
        per = self.S * self.S * channels
        if flow is not None:
            layer = (_lib.FlowLayer * 1)(self._flow_layer(False))
            for lo in range(0, n_pad, self.B):
                self._render_batch(self._flow["idx_dev"][0, lo:lo + self.B], shade=False)
                self._keep_targets()
                self._render_batch(self.idx_dev[0, lo:lo + self.B], shade=False)
                _enqueue_flow(self._flow, lo, layer, 1, self.B, self.S, self.ss, (None, 0, None), (None, 0, None), flow[1])
            return
        if labels is not None:
            layer = (_lib.LabelLayer * 1)(self._label_layer(False, labels[2]))
            for lo in range(0, n_pad, self.B):
                self._render_batch(self.idx_dev[0, lo:lo + self.B], shade=False)
                _enqueue_labels(self.lab, lo, layer, 1, self.B, self.S, self.ss, (None, 0, None), labels)
                if labels[3]:
                    self._enqueue_keypoints(self.kp, lo, layer, 1, 0, (None, 0, None), labels[4])
            return
        for lo in range(0, n_pad, self.B):
            self._render_batch(self.idx_dev[0, lo:lo + self.B])
            _ck(L.harp_resolve_u8(p(s["rgb"]), p(s["face_c"]), self.B, self.S, self.ss, *self._staged_args(0, lo, with_bg), p(self.bg_color_dev),
                                  channels, self.out[lo * per:].data_ptr(), _lib.stream()), "resolve_u8")

    @torch.no_grad()
    def render(self, rows, background=None, bg_rows=None, alpha=False):
        """Frames `rows` of the loaded motion -> (len(rows), S, S, 3) uint8 on the device ((.., 4) with alpha=True: the covered share of the
        pixel as alpha), a view of the player's buffer that the next call overwrites.  background: None (the constant `bg_color`, white) or
        a (N,S,S,3) uint8 device tensor; frame i is composited over its row bg_rows[i], without bg_rows over row i (N == len(rows)) or row
        0 (N == 1); a row outside [0, N) takes bg_color.  The rows in use are copied into a buffer of the player's in stream order, so
        one captured graph serves every background tensor and the caller's tensor is free again once the call has returned."""
        if self.tables is None:
            raise RuntimeError("load_motion() first")
        return self._render(rows, alpha, [(background, bg_rows)])[0]

    @torch.no_grad()
    def annotate(self, rows, parts=True, depth=True, uv=False, keypoints=True, tol=LABEL_TOL):
        """What the frames `rows` of the loaded motion show -> Annotation (above) of device tensors: always owner (1 where the avatar
        is), face and bbox; part with parts=True, depth with depth=True, uv with uv=True, uvz and vis with keypoints=True.  Needs
        keep_depth=True.  The batch's front and rasterisers run as in render (the shader does not: labels need no colour), then
        harp_annotate_layers and harp_keypoint_visibility, under the same graph path.  tol: a joint lies INSIDE the hand, a finger's
        radius or half the palm's thickness under the skin, so a joint counts as visible when the nearest surface at its pixel is no
        nearer than its own depth minus tol metres; 0.02 is that convention, not a tuned value."""
        if not self.keep_depth:
            raise ValueError("annotate needs a player built with keep_depth=True")
        if self.tables is None:
            raise RuntimeError("load_motion() first")
        labels = _label_flags(parts, depth, uv, keypoints, tol)
        self._part_table()
        self._labels_wanted = True
        n = self._render(rows, False, [(None, None)], labels)[1]
        return _annotation(self.lab, n, self.S, labels, self.kp["uvz"][:n] if labels[3] else None, self.kp["vis"][:n] if labels[3] else None, one=True)

    @torch.no_grad()
    def flow(self, rows, to_rows, tol=FLOW_TOL):
        """Where the surface point that each pixel of frame rows[i] shows lies in frame to_rows[i] of the loaded motion -> Flow (above) of
        device tensors.  Needs keep_depth=True.  Per batch the front and the rasterisers of the target rows, device copies of their ndc_c
        and z_c, the front and the rasterisers of the source rows and one harp_flow_layers, under a graph key of its own.  tol: the point
        lies on the surface, so the tolerance only absorbs the depth difference between where it lands and the centre of the sub-pixel
        it is tested at; 0.005 is that convention, not a tuned value."""
        if not self.keep_depth:
            raise ValueError("flow needs a player built with keep_depth=True")
        if self.tables is None:
            raise RuntimeError("load_motion() first")
        tol = _flow_tol(tol)
        self._flow_targets()
        n = self._render(rows, False, [(None, None)], None, ("flow", tol), to=(to_rows, []))[1]
        return self._flow_view(n)

    # ---- a whole motion to files ------------------------------------------------------------------------------------------------
    def play(self, motion, out_dir, backgrounds=None, fmt="jpg", alpha=False, labels=False, label_tol=LABEL_TOL, flow=None, flow_tol=FLOW_TOL):
        """load_motion(motion), render it batch by batch and write out_dir/%04d.<fmt> (fmt "jpg" or "png"; alpha=True needs "png" and
        writes RGBA).  backgrounds: None, a (N,S,S,3) uint8 tensor or a directory of images of that size (sorted by name); frame i is
        composited over background i mod N.  The frames leave through two pinned host buffers, one per batch in flight, and are encoded on
        a thread pool while the next batch renders.  labels=True (needs keep_depth=True) also writes part_%04d.png, depth_%04d.png,
        iuv_%04d.png and keypoints.npz (write_labels).  flow="fw" | "bw" | "both" (needs keep_depth=True) also writes flow_%04d.flo and /
        or flow_bw_%04d.flo with their status PNGs (write_flow).  Returns the list of paths."""
        _flow_mode(flow), _flow_tol(flow_tol)

        def prepare():
            self.load_motion(motion)
            bgs = load_backgrounds(backgrounds, self.S, self.dev)
            return lambda rows: self.render(rows, bgs, None if bgs is None else rows % bgs.shape[0], alpha)
        paths = self._play(out_dir, fmt, alpha, prepare)
        if labels:
            write_labels(out_dir, self.T, self.B, lambda rows: self.annotate(rows, uv=True, tol=label_tol), [part_names_of(self)])
        if flow:
            write_flow(out_dir, self.T, self.B, lambda rows, to: self.flow(rows, to, tol=flow_tol), flow)
        return paths


class ScenePlayer(_Player):
    """Several avatars in one frame with depth-correct occlusion: 1 to 4 AvatarPlayers built with keep_depth=True on one
    device with equal img_size, ss and batch_size — one camera: the focal length is the players' too, the translation comes from each
    motion's cam — rendered batch by batch into their own buffers and resolved by ONE harp_composite_layers_u8 per batch: per sub-sample
    the nearest avatar in front of an optional scene depth.  flip: one bool per player; a flipped avatar is shown mirrored in x, light
    included — a LEFT hand is a right-hand fit of horizontally mirrored frames shown with flip.  The avatars cast no shadows on each
    other.  The launches are captured into a graph when every player was built with use_graph=True."""

    _holds = "the motions hold"

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
        self.players = players
        super().__init__(p0.dev, p0.S, p0.ss, p0.B, all(p.use_graph for p in players),
                         (("background", (p0.S, p0.S, 3), torch.uint8), ("scene_depth", (p0.S, p0.S), torch.float32)))
        self._labels_wanted, self.lab, self.kp = False, None, None
        self._contacts_wanted, self._contact = False, None      # what contact() adds, allocated on its first call (_grow)

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

    def _grow(self, n_pad, used):
        if n_pad > self._n_cap:
            self.owner = torch.empty(n_pad, self.S, self.S, dtype=torch.uint8, device=self.dev)
            self.lab = None
        super()._grow(n_pad, used)
        if self._labels_wanted and self.lab is None:
            self.lab = _label_buffers(self._n_cap, self.S, len(self.players), self.dev)
            self.kp = [pl._keypoint_buffers(self._n_cap) for pl in self.players]
        if self._contacts_wanted and (self._contact is None or self._contact["cap"] != self._n_cap):
            # per ordered pair (query k, target j) the three outputs of harp_mesh_contact over every padded row; one workspace, for the
            # target with the most faces (the calls follow each other on one stream)
            n, P = self._n_cap, len(self.players)
            new = lambda dt, V: torch.empty(n, V, dtype=dt, device=self.dev)      # noqa: E731
            pairs = {(k, j): (new(torch.float32, q.topo.V), new(torch.int32, q.topo.V), new(torch.float32, q.topo.V))
                     for k, q in enumerate(self.players) for j in range(P) if j != k}
            ws = torch.empty(max(_lib.lib().harp_mesh_contact_ws_floats(self.B, pl.topo.F) for pl in self.players), dtype=torch.float32, device=self.dev)
            self._contact = dict(cap=n, pairs=pairs, ws=ws)

    def _enqueue(self, n_pad, channels, with_bg, with_depth, with_owner, labels=None, flow=None, contact=None):
        """per batch: every player's front / rasterisers / shader, then one composite; with labels = (part, depth, uv, keypoints, tol)
        every player's front / rasterisers, then the labels of the batch and every player's keypoints; with flow = ("flow", tol)
        every player's front / rasterisers of the TARGET rows and copies of their ndc_c and z_c, the same of the source rows, then
        the flow of the batch; with contact = ("contact", max_dist) every player's front only, then one harp_mesh_contact per ordered
        pair of players into the pair's rows of self._contact.  max_dist is part of the graph key, as flow's and the labels' tol are: every
        distinct value captures a graph of its own, kept until the scene grows or new tables are loaded"""
        L, p, B = _lib.lib(), _lib.ptr, self.B
        per = self.S * self.S
        if contact is not None:                          # ("contact", max_dist): every player's front, then one call per ordered pair
            meshes = [pl._contact_mesh(f) for pl, f in zip(self.players, self.flip)]
            for lo in range(0, n_pad, B):
                for pl in self.players:
                    pl._render_batch(self.idx_dev[0, lo:lo + B], front_only=True)
                for (k, j), (d, f, w) in self._contact["pairs"].items():
                    _ck(L.harp_mesh_contact(ctypes.byref(meshes[k]), ctypes.byref(meshes[j]), B, contact[1], p(self._contact["ws"]),
                                            d[lo:].data_ptr(), f[lo:].data_ptr(), w[lo:].data_ptr(), _lib.stream()), "mesh_contact")
            return
        if flow is not None:
            P = len(self.players)
            layers = (_lib.FlowLayer * P)(*[pl._flow_layer(f) for pl, f in zip(self.players, self.flip)])
            for lo in range(0, n_pad, B):
                for pl in self.players:
                    pl._render_batch(self._flow["idx_dev"][0, lo:lo + B], shade=False)
                    pl._keep_targets()
                for pl in self.players:
                    pl._render_batch(self.idx_dev[0, lo:lo + B], shade=False)
                _enqueue_flow(self._flow, lo, layers, P, B, self.S, self.ss, self._staged_args(1, lo, with_depth),
                              self._staged_to_args(0, "scene_depth", lo, with_depth), flow[1])
            return
        if labels is not None:
            P = len(self.players)
            layers = (_lib.LabelLayer * P)(*[pl._label_layer(f, labels[2]) for pl, f in zip(self.players, self.flip)])
            for lo in range(0, n_pad, B):
                scene = self._staged_args(1, lo, with_depth)
                for pl in self.players:
                    pl._render_batch(self.idx_dev[0, lo:lo + B], shade=False)
                _enqueue_labels(self.lab, lo, layers, P, B, self.S, self.ss, scene, labels)
                if labels[3]:
                    for k, pl in enumerate(self.players):
                        pl._enqueue_keypoints(self.kp[k], lo, layers, P, k, scene, labels[4])
            return
        layers = (_lib.Layer * len(self.players))(*[_lib.Layer(p(pl.s["rgb"]), p(pl.s["z_c"]), int(f), 0) for pl, f in zip(self.players, self.flip)])
        for lo in range(0, n_pad, B):
            for pl in self.players:
                pl._render_batch(self.idx_dev[0, lo:lo + B])
            _ck(L.harp_composite_layers_u8(layers, len(self.players), B, self.S, self.ss, *self._staged_args(1, lo, with_depth),
                                           *self._staged_args(0, lo, with_bg), p(self.bg_color_dev), channels,
                                           self.out[lo * per * channels:].data_ptr(), self.owner[lo:].data_ptr() if with_owner else None,
                                           _lib.stream()), "composite_layers_u8")

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
        frames, n = self._render(rows, alpha, [(background, bg_rows), (scene_depth, depth_rows)], bool(owner))
        return (frames, self.owner[:n]) if owner else frames

    @torch.no_grad()
    def annotate(self, rows, parts=True, depth=True, uv=False, keypoints=True, tol=LABEL_TOL, scene_depth=None, depth_rows=None):
        """What the scene's frames `rows` show -> Annotation, as AvatarPlayer.annotate: owner is bit for bit render(owner=True)'s, bbox is
        (n, players, 4), and uvz and vis are tuples with one tensor per player (its own joints; the occluder 1 + k is player k, 255 the
        scene depth).  scene_depth, depth_rows: as render."""
        if self.T < 1 or any(p.tables is None for p in self.players):
            raise RuntimeError("load_motions() first")
        labels = _label_flags(parts, depth, uv, keypoints, tol)
        for pl in self.players:
            pl._part_table()
        self._labels_wanted = True
        n = self._render(rows, False, [(None, None), (scene_depth, depth_rows)], False, labels)[1]
        kp = lambda key: tuple(b[key][:n] for b in self.kp) if labels[3] else None      # noqa: E731
        return _annotation(self.lab, n, self.S, labels, kp("uvz"), kp("vis"), one=False)

    @torch.no_grad()
    def flow(self, rows, to_rows, tol=FLOW_TOL, scene_depth=None, depth_rows=None, depth_to_rows=None):
        """Where the surface point that each pixel of scene frame rows[i] shows lies in scene frame to_rows[i] -> Flow, as
        AvatarPlayer.flow: the source point is annotate's (the same owner, face and uv), the occluder 1 + k is player k, 255 the scene
        depth.  scene_depth: as render; frame rows[i] is composited against its row depth_rows[i] and the point is tested at the target
        against its row depth_to_rows[i] (each without its rows: row i when N == len(rows), row 0 when N == 1)."""
        if self.T < 1 or any(p.tables is None for p in self.players):
            raise RuntimeError("load_motions() first")
        tol = _flow_tol(tol)
        for pl in self.players:
            pl._flow_targets()
        n = self._render(rows, False, [(None, None), (scene_depth, depth_rows)], False, None, ("flow", tol),
                         to=(to_rows, [(scene_depth, depth_to_rows)]))[1]
        return self._flow_view(n)

    @torch.no_grad()
    def contact(self, rows, max_dist=CONTACT_DIST):
        """Where the avatars of the scene's frames `rows` touch -> Contact (above): per player and vertex the signed distance to the nearest
        OTHER player's surface, which player, face and part that is, and the winding number about it; per frame the smallest distance and
        the deepest penetration.  Needs at least two players.  Per batch every player's front only (no rasteriser runs) and one
        harp_mesh_contact per ordered pair of players, under a graph key of its own; the minimum over the others is taken afterwards
        with torch ops on the device (the lower player wins a tie).  max_dist metres: beyond it a vertex has no contact (+inf, 0, -1, 0,
        0); CONTACT_DIST = 0.02 is about a finger's thickness, a convention, not a tuned value.  A vertex is INSIDE another avatar when
        the winding number of that avatar's surface about it exceeds 0.5; the hand and arm meshes are open at the wrist or shoulder, so
        near that opening the value is fractional."""
        if len(self.players) < 2:
            raise ValueError("contact needs a scene of at least two players")
        if self.T < 1 or any(p.tables is None for p in self.players):
            raise RuntimeError("load_motions() first")
        max_dist = float(max_dist)
        if not max_dist >= 0:
            raise ValueError(f"max_dist must not be negative or NaN, got {max_dist}")
        tabs = [pl._part_table() for pl in self.players]
        self._contacts_wanted = True
        n = self._render(rows, False, [(None, None), (None, None)], False, None, None, ("contact", max_dist))[1]
        return compose_contact([{j: tuple(t[:n] for t in self._contact["pairs"][k, j]) for j in range(len(self.players)) if j != k}
                                for k in range(len(self.players))], tabs)

    def play(self, motions, out_dir, backgrounds=None, scene_depth=None, fmt="jpg", alpha=False, masks=False, labels=False, label_tol=LABEL_TOL,
             flow=None, flow_tol=FLOW_TOL, contacts=False, contact_dist=CONTACT_DIST):
        """load_motions(motions), render the scene batch by batch and write out_dir/%04d.<fmt> as AvatarPlayer.play does; with masks=True
        also out_dir/mask_%04d.png, the owner map (8-bit grey: 0 background, 1 + the player).  backgrounds: as AvatarPlayer.play;
        scene_depth: None, a float32 (N,S,S) tensor or a directory (load_scene_depth), frame i tested against depth i mod N.  labels=True
        also writes the label files (write_labels), one keypoints_<k>.npz per player k when there are several.  Returns the list of the
        frames' paths.  flow="fw" | "bw" | "both" also writes the flow files (write_flow).  contacts=True (at least two players) also
        writes contacts.npz (write_contacts) with contact(rows, contact_dist) of every frame."""
        _flow_mode(flow), _flow_tol(flow_tol)
        if contacts and len(self.players) < 2:
            raise ValueError("contacts need a scene of at least two players")
        if contacts and not float(contact_dist) >= 0:
            raise ValueError(f"contact_dist must not be negative or NaN, got {contact_dist}")

        def prepare():
            self.load_motions(motions)
            bgs, depth = load_backgrounds(backgrounds, self.S, self.dev), load_scene_depth(scene_depth, self.S, self.dev)
            prepare.depth = depth
            return lambda rows: self.render(rows, bgs, None if bgs is None else rows % bgs.shape[0], alpha, depth,
                                            None if depth is None else rows % depth.shape[0], owner=masks)
        paths = self._play(out_dir, fmt, alpha, prepare, masks)
        if labels:
            d = prepare.depth
            write_labels(out_dir, self.T, self.B, lambda rows: self.annotate(rows, uv=True, tol=label_tol, scene_depth=d,
                                                                             depth_rows=None if d is None else rows % d.shape[0]),
                         [part_names_of(pl) for pl in self.players])
        if flow:
            d = prepare.depth
            dr = lambda rows: None if d is None else rows % d.shape[0]      # noqa: E731
            write_flow(out_dir, self.T, self.B, lambda rows, to: self.flow(rows, to, tol=flow_tol, scene_depth=d, depth_rows=dr(rows),
                                                                          depth_to_rows=dr(to)), flow)
        if contacts:
            write_contacts(out_dir, self.T, self.B, lambda rows: self.contact(rows, contact_dist), [part_names_of(pl) for pl in self.players],
                           float(contact_dist))
        return paths


def part_names_of(player):
    """the label names of an AvatarPlayer's model, index = label (labels.part_names of its hand layer)"""
    from .labels import joint_part_names
    return joint_part_names(player._skin_weights.shape[1])


def _label_flags(parts, depth, uv, keypoints, tol):
    import math
    tol = float(tol)
    if not (tol >= 0 and math.isfinite(tol)):
        raise ValueError(f"tol must be non-negative and finite, got {tol}")
    return (bool(parts), bool(depth), bool(uv), bool(keypoints), tol)


def _label_buffers(n, S, P, dev):
    new = lambda dt, *shape: torch.empty(n, *shape, dtype=dt, device=dev)      # noqa: E731
    return dict(owner=new(torch.uint8, S, S), part=new(torch.uint8, S, S), depth=new(torch.float32, S, S), face=new(torch.int32, S, S),
                uv=new(torch.float32, S, S, 2), bbox=new(torch.int32, P, 4))


def _enqueue_labels(lab, lo, layers, n_layers, B, S, ss, scene, labels):
    """the clear of the batch's boxes and harp_annotate_layers into rows lo.. of the label buffers, on the current stream"""
    at = lambda k, on=True: lab[k][lo:].data_ptr() if on else None      # noqa: E731
    lab["bbox"][lo:lo + B].zero_()                       # (inside the captured sequence: the boxes are accumulated by atomic max)
    _ck(_lib.lib().harp_annotate_layers(layers, n_layers, B, S, ss, *scene, at("owner"), at("part", labels[0]), at("depth", labels[1]), at("face"),
                                        at("uv", labels[2]), at("bbox"), _lib.stream()), "annotate_layers")


def compose_contact(pairs, part_tables):
    """The documented rule from the pairwise results to Contact, in torch ops on the device.  pairs: per player k a dict {other player j:
    (dist, face, wind) of harp_mesh_contact with k as the query and j as the target}; part_tables: per player its (F,) uint8 part of every
    face.  Per vertex the other with the smallest unsigned distance wins, the lower player a tie; the distance is negated where that
    player's winding number exceeds 0.5.  A pair beyond max_dist brings (+inf, -1, 0) and never wins over a finite one.  A player's part
    table is indexed by ITS faces only (the players of a scene may have meshes of different sizes), and every tensor returned is new:
    none is a view of `pairs`."""
    dist, other, face, part, wind = [], [], [], [], []
    for mine in pairs:
        d = f = w = o = pt = None
        for j in sorted(mine):
            dj, fj, wj = mine[j]
            hit = fj >= 0
            oj = torch.where(hit, torch.full_like(fj, j + 1, dtype=torch.uint8), torch.zeros_like(fj, dtype=torch.uint8))
            pj = torch.where(hit, part_tables[j][fj.clamp(min=0).long()], torch.zeros_like(oj))
            if d is None:
                d, f, w, o, pt = dj, fj.clone(), wj.clone(), oj, pj
            else:
                m = dj < d
                d, f, w, o, pt = (torch.where(m, new, old) for new, old in ((dj, d), (fj, f), (wj, w), (oj, o), (pj, pt)))
        dist.append(torch.where(w > 0.5, -d, d)); other.append(o); face.append(f); part.append(pt); wind.append(w)
    min_dist = torch.stack([d.amin(1) for d in dist]).amin(0)
    deep = torch.stack([torch.where(w > 0.5, -d, torch.zeros_like(d)).amax(1) for d, w in zip(dist, wind)]).amax(0)
    return Contact(tuple(dist), tuple(other), tuple(face), tuple(part), tuple(wind), min_dist, deep.clamp(min=0))


def write_contacts(out_dir, T, B, contact, names, max_dist):
    """contacts.npz of a played scene beside its frames, batch by batch: per player k dist_k (T,V_k) float32 signed metres (+inf: none),
    other_k (T,V_k) uint8, face_k (T,V_k) int32, part_k (T,V_k) uint8, wind_k (T,V_k) float32 and part_names_k; min_dist (T,),
    max_penetration (T,) float32; max_dist, the contact distance used.  contact(rows) -> Contact; names: one list of part names per player."""
    P = len(names)
    keys = ("dist", "other", "face", "part", "wind")
    got = {f"{key}_{k}": [] for key in keys for k in range(P)}
    per_frame = dict(min_dist=[], max_penetration=[])
    for lo in range(0, T, B):
        c = contact(np.arange(lo, min(T, lo + B)))
        for key in keys:
            for k in range(P):
                got[f"{key}_{k}"].append(getattr(c, key)[k].cpu().numpy())
        for key in per_frame:
            per_frame[key].append(getattr(c, key).cpu().numpy())
    path = os.path.join(out_dir, "contacts.npz")
    np.savez(path, max_dist=np.float32(max_dist), **{k: np.concatenate(v) for k, v in {**got, **per_frame}.items()},
             **{f"part_names_{k}": np.array(names[k]) for k in range(P)})
    return path


def _flow_tol(tol):
    import math
    tol = float(tol)
    if not (tol >= 0 and math.isfinite(tol)):
        raise ValueError(f"tol must be non-negative and finite, got {tol}")
    return tol


def _flow_mode(flow):
    if flow not in (None, "fw", "bw", "both"):
        raise ValueError(f'flow is None, "fw", "bw" or "both", got {flow!r}')
    return flow


def _enqueue_flow(fl, lo, layers, n_layers, B, S, ss, scene, scene_to, tol):
    """harp_flow_layers into rows lo.. of the flow buffers, on the current stream"""
    _ck(_lib.lib().harp_flow_layers(layers, n_layers, B, S, ss, *scene, *scene_to, tol, fl["flow"][lo:].data_ptr(), fl["dz"][lo:].data_ptr(),
                                    fl["status"][lo:].data_ptr(), _lib.stream()), "flow_layers")


def _annotation(lab, n, S, labels, uvz, vis, one):
    bbox = ops.bbox_from_extents(lab["bbox"][:n], S)
    view = lambda k, on=True: lab[k][:n] if on else None      # noqa: E731
    return Annotation(view("owner"), view("part", labels[0]), view("depth", labels[1]), view("face"), view("uv", labels[2]),
                      bbox[:, 0] if one else bbox, uvz, vis)


def write_labels(out_dir, T, B, annotate, names):
    """The label files of a played motion beside its frames, batch by batch: part_%04d.png (8-bit grey, the part), depth_%04d.png (16-bit,
    millimetres (int)(1000 z + 0.5) clamped to 65535, 0 = empty: what load_scene_depth reads), iuv_%04d.png (8-bit RGB (part,
    floor(255 u + 0.5), floor(255 v + 0.5)), the DensePose convention) and per player keypoints.npz (keypoints_<k>.npz when there are
    several): keypoints (T,NJ,2) pixels, weights (T,NJ) = 1 for a visible joint and 0 otherwise, depth (T,NJ) = Z_k - Z_0 metres, z (T,NJ),
    visible, occluder (T,NJ) uint8, bbox (T,4) = (xmin, ymin, xmax, ymax) or -1, part_names.  The file of a MANO hand is what
    --keypoints2d reads.  annotate(rows) -> Annotation with every map; names: one list of part names per player."""
    from concurrent.futures import ThreadPoolExecutor
    from ..utils.data_util import default_workers
    P = len(names)
    kp = [dict(uvz=[], vis=[], bbox=[]) for _ in range(P)]
    pool, pending = ThreadPoolExecutor(max(1, min(8, default_workers()))), []
    for lo in range(0, T, B):
        rows = np.arange(lo, min(T, lo + B))
        a = annotate(rows)
        part, depth, uv = a.part.cpu().numpy(), a.depth.cpu().numpy(), a.uv.cpu().numpy()
        single = torch.is_tensor(a.uvz)                   # an AvatarPlayer's: one player, bbox (n,4)
        uvz, vis, bbox = ((a.uvz,), (a.vis,), a.bbox[:, None]) if single else (a.uvz, a.vis, a.bbox)
        for k in range(P):
            kp[k]["uvz"].append(uvz[k].cpu().numpy()); kp[k]["vis"].append(vis[k].cpu().numpy()); kp[k]["bbox"].append(bbox[:, k].cpu().numpy())
        mm = np.clip((1000.0 * depth.astype(np.float64) + 0.5).astype(np.int64), 0, 65535).astype(np.uint16)
        q = np.clip(np.floor(255.0 * uv.astype(np.float64) + 0.5), 0, 255).astype(np.uint8)
        for i, r in enumerate(rows):                     # (host copies of this batch: encoded while the next batch is labelled)
            pending += [pool.submit(_encode, os.path.join(out_dir, "part_%04d.png" % r), part[i], "png"),
                        pool.submit(_encode, os.path.join(out_dir, "depth_%04d.png" % r), mm[i], "png"),
                        pool.submit(_encode, os.path.join(out_dir, "iuv_%04d.png" % r), np.concatenate([part[i][..., None], q[i]], -1), "png")]
    with pool:
        for fut in pending:
            fut.result()
    for k in range(P):
        uvz, vis, bbox = (np.concatenate(kp[k][key]) for key in ("uvz", "vis", "bbox"))
        np.savez(os.path.join(out_dir, "keypoints.npz" if P == 1 else "keypoints_%d.npz" % k), keypoints=uvz[..., :2], weights=(vis[..., 0] == 2).astype(np.float32),
                 depth=uvz[..., 2] - uvz[:, :1, 2], z=uvz[..., 2], visible=vis[..., 0], occluder=vis[..., 1], bbox=bbox, part_names=np.array(names[k]))


def write_flow(out_dir, T, B, flow, mode):
    """The motion labels of a played motion beside its frames, batch by batch.  mode "fw" or "both": flow_%04d.flo, frame t -> t + 1, for
    t = 0 .. T - 2; "bw" or "both": flow_bw_%04d.flo, frame t -> t - 1, for t = 1 .. T - 1; with each flow_status_%04d.png /
    flow_bw_status_%04d.png, 8-bit grey of status[0].  .flo is the Middlebury format in output pixels (harp_amd.io.save_flo); a pixel
    with status 0 or 1 carries that format's unknown value.  flow(rows, to_rows) -> Flow."""
    from concurrent.futures import ThreadPoolExecutor
    from ..io import save_flo
    from ..utils.data_util import default_workers
    pool, pending = ThreadPoolExecutor(max(1, min(8, default_workers()))), []
    for stem, step, first, last in (("flow", 1, 0, T - 1), ("flow_bw", -1, 1, T)):
        if mode not in ("both", "fw" if step > 0 else "bw"):
            continue
        for lo in range(first, last, B):
            rows = np.arange(lo, min(last, lo + B))
            got = flow(rows, rows + step)
            fl, st = got.flow.cpu().numpy(), got.status[..., 0].cpu().numpy()      # (host copies of this batch: encoded while the next runs)
            for i, r in enumerate(rows):
                pending += [pool.submit(save_flo, os.path.join(out_dir, "%s_%04d.flo" % (stem, r)), fl[i], st[i] >= 2),
                            pool.submit(_encode, os.path.join(out_dir, "%s_status_%04d.png" % (stem, r)), st[i], "png")]
    with pool:
        for fut in pending:
            fut.result()


def _encode(path, u8, fmt):
    if fmt == "jpg":
        from ..monitor import encode_jpeg
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
