"""The two forward-only renderers on one base.  `_Player` owns what a call and a play loop need whatever is drawn: the
index stage (`_Stage`) with the copies of the caller's tensors, the buffers of each kind of pass, the graphs, the labels and flow passes
over the player's layers, and the double-buffered way to disk.  `AvatarPlayer` adds one avatar's launches and the resolve (§22),
`ScenePlayer` several avatars, the composite (§23) and the contact pass (§36); the self-contact pass (§37) is the base's, over the layers."""
import collections
import ctypes
import math
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
# self-contact within ONE avatar.  Both are conventions, not tuned values.  SELF_GEODESIC: the faces within 3 cm of a vertex
# along the mesh's edges (about a finger's segment and a half) do not count for it — its own neighbourhood is always near.
# SELF_CONTACT_DIST: 4 mm; on the hand template at rest with that exclusion no vertex has a counting face within 4 mm (the nearest is at
# 4.56 mm), while 336 of 778 lie within 2 cm (the facing sides of neighbouring fingers): CONTACT_DIST is not usable within one hand
SELF_GEODESIC = 0.03
SELF_CONTACT_DIST = 0.004
# what self_contact returns per avatar: device tensors over the rows asked for and the avatar's V vertices, every one new.
# dist (n,V) float32, SIGNED: the distance to the nearest face of the avatar's own surface that is not excluded for the vertex, negative
# where the vertex is inside another part of the avatar (wind > 1.0), +inf beyond max_dist; face (n,V) int32: that face, -1 none; part
# (n,V) uint8: that face's part, 0 none; own_part (V,) uint8: the vertex's own part (labels.subdivided_vertex_part_labels); wind (n,V)
# float32: the winding number of the WHOLE surface about the vertex (not masked), 0 where dist is +inf; touch (n,P,P) bool, P = 1 + the
# skinning joints: touch[t, p, q] = some vertex of part p is within max_dist of a face of part q (a pinch: touch[t, thumb3, index3]);
# min_dist (n,) float32: the smallest signed distance (+inf: no contact); max_penetration (n,) float32: the largest -dist, or 0
SelfContact = collections.namedtuple("SelfContact", "dist face part own_part wind touch min_dist max_penetration")


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


class _Stage:
    """One index table of a render call (stage_table's layout over `inputs`, a player's declared (name, per-row shape, dtype)) on the
    device, its pinned host copy, and the player's own copy of every staged input the calls have used so far."""

    def __init__(self, inputs, dev, B):
        self.inputs, self.dev, self.B, self.cap, self.bufs = inputs, dev, B, 0, {}

    def alloc(self, n, used):
        """the tables for n padded rows when that is not their length, and a copy of every input of `used` (one bool per input) that
        has none yet (no graph reads it: the key of a graph says which inputs it uses)"""
        if n != self.cap:
            rows = 1 + 2 * len(self.inputs)
            self.idx_dev = torch.zeros(rows, n, dtype=torch.int32, device=self.dev)
            self.idx_pin = torch.zeros(rows, n, dtype=torch.int32).pin_memory()
            self.cap, self.bufs = n, {}
        for (name, shape, dtype), u in zip(self.inputs, used):
            if u and name not in self.bufs:
                self.bufs[name] = torch.empty(n, *shape, dtype=dtype, device=self.dev)

    def upload(self, table, tensors, n, done=None):
        """the host table into the pinned copy and from there to the device in one copy (`done`, an event, is recorded behind it), then
        the rows in use of every caller tensor into the player's copy, in stream order.  The caller has waited for the previous upload."""
        self.idx_pin.numpy()[:, :table.shape[1]] = table
        self.idx_dev.copy_(self.idx_pin, non_blocking=True)
        if done is not None:
            done.record()
        for k, ((name, _, _), t) in enumerate(zip(self.inputs, tensors)):
            if t is not None:
                torch.index_select(t, 0, self.idx_dev[2 + 2 * k, :n], out=self.bufs[name][:n])

    def rows(self, lo):
        """the motion's rows of the batch at `lo`, on the device"""
        return self.idx_dev[0, lo:lo + self.B]

    def args(self, name, lo, used):
        """what a kernel takes of staged input `name` for the batch at `lo`: (the player's copy, its rows, the batch's slots), or
        (None, 0, None) when the call does not use it (used: {name: bool}) or the player declares no such input"""
        if not used.get(name):
            return None, 0, None
        k = [i[0] for i in self.inputs].index(name)
        return self.bufs[name].data_ptr(), self.cap, self.idx_dev[1 + 2 * k, lo:lo + self.B].data_ptr()


class _Player:
    """What AvatarPlayer and ScenePlayer share.  A subclass declares the caller tensors it stages (`_inputs`: name, per-row shape, dtype),
    says what it draws (`_layers`) and supplies `_enqueue_frames`.  A call is one PASS, a hashable (kind, *what it carries): ("frames",
    channels, owner), ("labels", _label_flags' tuple), ("flow", tol), ("contact", max_dist) or ("selfcontact", max_dist, geodesic).  Per kind there is one `_enqueue_<kind>`,
    the launches of a whole call in order on the current stream, and one `_alloc_<kind>`, its output buffers.  Nothing is allocated
    after the constructor except when a pass is first used or a longer `rows` is first seen (`_grow`)."""

    _holds, _load = "the motion holds", "load_motion"

    def __init__(self, device, S, ss, B, use_graph, inputs):
        self.dev, self.S, self.ss, self.B, self.use_graph = torch.device(device), S, ss, B, bool(use_graph)
        self._inputs = inputs
        self.T = self._n_cap = 0
        self._stage, self._stage_to = _Stage(inputs, self.dev, B), None      # the source rows'; the target rows' of flow(), made on its first call
        self.idx_done, self._out, self._graphs = None, {}, {}
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

    def _ready(self, need_depth=False):
        """the preconditions of a call; need_depth: the name of a call that reads the layers' depth maps"""
        layers = [pl for pl, _ in self._layers()]
        if need_depth and not all(pl.keep_depth for pl in layers):
            raise ValueError(f"{need_depth} needs a player built with keep_depth=True")
        if any(pl.tables is None for pl in layers) or (self.T < 1 and self not in layers):      # (a scene's own T is 0 until ITS motions are loaded)
            raise RuntimeError(f"{self._load}() first")

    def _grow(self, n_pad, used, decl_to=None, used_to=None):
        """A longer call than any before drops every graph and every pass's buffers with the capacity they were made for; then the
        index table(s) are made for the capacity (decl_to, used_to: the inputs of flow's target rows; their table is made on first use)"""
        if n_pad > self._n_cap:
            self._n_cap, self._out, self._graphs = n_pad, {}, {}
        self._stage.alloc(self._n_cap, used)
        if decl_to is not None:
            self._stage_to = self._stage_to or _Stage(decl_to, self.dev, self.B)
            self._stage_to.alloc(self._n_cap, used_to)

    def _buffers(self, kind):
        """The output buffers of a pass, the one rule for every kind: made by `_alloc_<kind>(capacity)` on the pass's first use, and again
        after _grow has dropped them — together with the graphs, so no graph outlives a buffer it points at"""
        if kind not in self._out:
            self._out[kind] = getattr(self, "_alloc_" + kind)(self._n_cap)
        return self._out[kind]

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

    def _upload(self, table, tensors, n, to=None):
        """The one host wait and the one event of a call: the previous call's upload has read the pinned table(s) before either is
        written again; then the target rows' table (to: its (table, tensors), flow only) and the source rows', each with its gathers,
        the event behind the source table's copy and so behind both"""
        if self.idx_done is not None:
            self.idx_done.synchronize()
        if to is not None:
            self._stage_to.upload(*to, n)
        self.idx_done = torch.cuda.Event()
        self._stage.upload(table, tensors, n, self.idx_done)

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

    def _checked_rows(self, name, rows, n=None):
        r = _host_rows(name, rows, n)
        if r.shape[0] < 1:
            raise ValueError("no rows to render")
        if r.min() < 0 or r.max() >= self.T:             # (on the host, before anything is enqueued: the kernels gather rows unchecked)
            raise IndexError(f"{name} span [{r.min()}, {r.max()}] but {self._holds} {self.T} frames")
        return r

    def _render(self, rows, inputs, pass_, to=None):
        """The path of every call of both players: `rows` checked on the host, padded to whole batches, staged with `inputs` ({name of a
        declared input: the caller's (tensor, rows)}; one that is not named is not used), and `pass_` enqueued or replayed under the key
        (padded length, input used?..., pass_) into its buffers -> n, the rows asked for.  to (flow only): (the target rows, the
        `inputs` of the target frames); they travel in a table of their own, over the inputs named there."""
        r = self._checked_rows("rows", rows)
        n = r.shape[0]
        n_pad = -(-n // self.B) * self.B
        tensors, staged = self._staged_all(self._inputs, inputs, n)
        used = tuple(rr is not None for rr, _ in staged)
        with torch.cuda.device(self.dev):
            if to is None:
                self._grow(n_pad, used)
            else:
                r_to = self._checked_rows("to_rows", to[0], n)
                decl = [i for i in self._inputs if i[0] in to[1]]
                tensors_to, staged_to = self._staged_all(decl, to[1], n)
                self._grow(n_pad, used, decl, [rr is not None for rr, _ in staged_to])
                to = stage_table(r_to, n_pad, staged_to), tensors_to
            self._buffers(pass_[0])
            self._upload(stage_table(r, n_pad, staged), tensors, n, to)
            self._run((n_pad,) + used + (pass_,))
        return n

    def _staged_all(self, decl, inputs, n):
        """_staged of every declared input of `decl` -> (the caller's tensors, [(rows, N)]), in the order of the declaration"""
        given = [inputs.get(name, (None, None)) for name, _, _ in decl]
        return [t for t, _ in given], [self._staged(name, t, rr, n, shape, dtype) for (name, shape, dtype), (t, rr) in zip(decl, given)]

    def _enqueue(self, n_pad, *key):
        """the launches of a whole call: the pass's own method, told which staged inputs the call uses"""
        kind, *carried = key[-1]
        getattr(self, "_enqueue_" + kind)(n_pad, dict(zip((i[0] for i in self._inputs), key[:-1])), *carried)

    def _frames(self, rows, inputs, alpha, owner=False):
        """the frames pass -> (frames (n, S, S, channels), n)"""
        C = 4 if alpha else 3
        n = self._render(rows, inputs, ("frames", C, bool(owner)))
        return self._out["frames"]["out"][:n * self.S * self.S * C].view(n, self.S, self.S, C), n

    def _alloc_frames(self, n):
        return dict(out=torch.empty(n * self.S * self.S * 4, dtype=torch.uint8, device=self.dev))

    def _scene_depth_args(self, lo, used, to=False):
        """the scene depth arguments of the batch at `lo`, of the source frames or (to=True) of the flow's target frames; (None, 0, None)
        for a call without a scene depth and for a player that declares none"""
        return (self._stage_to if to else self._stage).args("scene_depth", lo, used)

    # ---- labels and flow, over the layers: an avatar is a scene of one unflipped layer without a scene depth ------
    def _alloc_labels(self, n):
        """the maps over every padded row, the boxes per layer, and per layer the (uvz, vis) of its joints"""
        S, layers = self.S, self._layers()
        new = lambda dt, *shape: torch.empty(n, *shape, dtype=dt, device=self.dev)      # noqa: E731
        return dict(owner=new(torch.uint8, S, S), part=new(torch.uint8, S, S), depth=new(torch.float32, S, S), face=new(torch.int32, S, S),
                    uv=new(torch.float32, S, S, 2), bbox=new(torch.int32, len(layers), 4),
                    kp=[dict(uvz=new(torch.float32, pl.n_joints, 3), vis=new(torch.uint8, pl.n_joints, 2)) for pl, _ in layers])

    def _enqueue_labels(self, n_pad, used, flags):
        """per batch every layer's front / rasterisers (no shader: labels need no colour), the clear of the batch's boxes and
        harp_annotate_layers, then with keypoints every layer's harp_keypoint_visibility; flags = (part, depth, uv, keypoints, tol)"""
        lab, layers, B = self._out["labels"], self._layers(), self.B
        P = len(layers)
        arr = (_lib.LabelLayer * P)(*[pl._label_layer(f, flags[2]) for pl, f in layers])
        for lo in range(0, n_pad, B):
            at = lambda k, on=True: lab[k][lo:].data_ptr() if on else None      # noqa: E731
            scene = self._scene_depth_args(lo, used)
            for pl, _ in layers:
                pl._render_batch(self._stage.rows(lo), shade=False)
            lab["bbox"][lo:lo + B].zero_()                # (inside the captured sequence: the boxes are accumulated by atomic max)
            _lib.check(_lib.lib().harp_annotate_layers(arr, P, B, self.S, self.ss, *scene, at("owner"), at("part", flags[0]), at("depth", flags[1]),
                                                       at("face"), at("uv", flags[2]), at("bbox"), _lib.stream()), "annotate_layers")
            if flags[3]:
                for k, (pl, _) in enumerate(layers):
                    pl._keypoints_batch(lab["kp"][k], lo, arr, P, k, scene, flags[4])

    def _annotate(self, rows, inputs, flags):
        """the labels pass -> Annotation in the scene's form: bbox (n, layers, 4), uvz and vis tuples with one tensor per layer"""
        for pl, _ in self._layers():
            pl._part_table()
        n = self._render(rows, inputs, ("labels", flags))
        lab = self._out["labels"]
        view = lambda k, on=True: lab[k][:n] if on else None      # noqa: E731
        kp = lambda key: tuple(b[key][:n] for b in lab["kp"]) if flags[3] else None      # noqa: E731
        return Annotation(view("owner"), view("part", flags[0]), view("depth", flags[1]), view("face"), view("uv", flags[2]),
                          ops.bbox_from_extents(lab["bbox"][:n], self.S), kp("uvz"), kp("vis"))

    def _alloc_flow(self, n):
        S = self.S
        new = lambda dt, *shape: torch.empty(n, *shape, dtype=dt, device=self.dev)      # noqa: E731
        return dict(flow=new(torch.float32, S, S, 2), dz=new(torch.float32, S, S), status=new(torch.uint8, S, S, 2))

    def _enqueue_flow(self, n_pad, used, tol):
        """per batch every layer's front / rasterisers of the TARGET rows and copies of their ndc_c and z_c, the same of the source rows,
        then one harp_flow_layers"""
        fl, layers, B = self._out["flow"], self._layers(), self.B
        P = len(layers)
        arr = (_lib.FlowLayer * P)(*[pl._flow_layer(f) for pl, f in layers])
        for lo in range(0, n_pad, B):
            for pl, _ in layers:
                pl._render_batch(self._stage_to.rows(lo), shade=False)
                pl._keep_targets()
            for pl, _ in layers:
                pl._render_batch(self._stage.rows(lo), shade=False)
            _lib.check(_lib.lib().harp_flow_layers(arr, P, B, self.S, self.ss, *self._scene_depth_args(lo, used), *self._scene_depth_args(lo, used, to=True),
                                                   tol, fl["flow"][lo:].data_ptr(), fl["dz"][lo:].data_ptr(), fl["status"][lo:].data_ptr(),
                                                   _lib.stream()), "flow_layers")

    def _flow(self, rows, inputs, to, tol):
        """the flow pass -> Flow"""
        tol = _tol(tol)
        for pl, _ in self._layers():
            pl._flow_targets()
        n = self._render(rows, inputs, ("flow", tol), to=to)
        fl = self._out["flow"]
        return Flow(fl["flow"][:n], fl["dz"][:n], fl["status"][:n])

    # ---- self-contact, over the layers: every layer against itself, an avatar is a scene of one ------------------------
    def _alloc_selfcontact(self, n):
        """per layer the three outputs of harp_mesh_contact_excl over every padded row; one workspace, for the layer with the most faces
        (the calls follow each other on one stream)"""
        layers = [pl for pl, _ in self._layers()]
        new = lambda dt, V: torch.empty(n, V, dtype=dt, device=self.dev)      # noqa: E731
        ws = torch.empty(max(_lib.lib().harp_mesh_contact_ws_floats(self.B, pl.topo.F) for pl in layers), dtype=torch.float32, device=self.dev)
        return dict(out=[(new(torch.float32, pl.topo.V), new(torch.int32, pl.topo.V), new(torch.float32, pl.topo.V)) for pl in layers], ws=ws)

    def _enqueue_selfcontact(self, n_pad, used, max_dist, geodesic):
        """per batch every layer's front only, then one harp_mesh_contact_excl per layer with the layer as query AND target (its own flip
        on both sides) under its exclusion table of `geodesic` (made by _self_contact before: nothing is built inside a capture).
        max_dist and geodesic are part of the pass and so of the graph key"""
        p, B, bufs, layers = _lib.ptr, self.B, self._out["selfcontact"], self._layers()
        meshes = [pl._contact_mesh(f) for pl, f in layers]
        tables = [pl._exclusion_table(geodesic) for pl, _ in layers]
        for lo in range(0, n_pad, B):
            for pl, _ in layers:
                pl._render_batch(self._stage.rows(lo), front_only=True)
            for m, tab, (d, f, w) in zip(meshes, tables, bufs["out"]):
                _lib.check(_lib.lib().harp_mesh_contact_excl(ctypes.byref(m), ctypes.byref(m), p(tab), B, max_dist, p(bufs["ws"]),
                                                             d[lo:].data_ptr(), f[lo:].data_ptr(), w[lo:].data_ptr(), _lib.stream()),
                           "mesh_contact_excl")

    def _self_contact(self, rows, max_dist, geodesic):
        """the self-contact pass -> one SelfContact per layer"""
        max_dist, geodesic = _self_contact_args(max_dist, geodesic)
        layers = [pl for pl, _ in self._layers()]
        with torch.cuda.device(self.dev):
            static = [(pl._part_table(), pl._own_part_table(), pl._exclusion_table(geodesic)) for pl in layers]
        n = self._render(rows, {}, ("selfcontact", max_dist, geodesic))
        return tuple(compose_self_contact(*(t[:n] for t in out), part, own, 1 + pl._skin_weights.shape[1])
                     for pl, out, (part, own, _) in zip(layers, self._out["selfcontact"]["out"], static))

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
            _lib.check(_lib.lib().harp_normalize3_pack(_lib.ptr(self.fit["texture"]), _lib.ptr(self.fit["normal_map"]), self.Ht * self.Wt,
                                                _lib.ptr(self.nmap_n), _lib.ptr(self.texnm), _lib.stream()), "normalize3_pack")
        self._cap = 0
        self.tab = self.tables = None
        self._skin_weights = np.asarray(hand_layer._model_np["weights"])      # (V0, NJ): the part table is made from it on first use
        self._face_label = None
        self._own_part, self._excl = None, {}            # self-contact (§37): the vertices' own parts, the exclusion table per geodesic radius
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
        _lib.check((L.harp_arm_front_fwd if self.use_arm else L.harp_hand_front_fwd)(ctypes.byref(h), st), "front_fwd")
        if front_only:
            return
        if self.self_shadow:
            _lib.check(L.harp_raster_setup_pair(p(s["ndc_c"]), 0.0, p(s["ws_c"]), p(s["ndc_l"]), 0.0, p(s["ws_l"]), p(tp.faces), B, V, F, Sh, st),
                "raster_setup_pair")
            _lib.check(L.harp_rasterize_fwd(p(s["ndc_c"]), p(tp.faces), B, V, F, Sh, 4, 0.0, 1.0, p(s["ws_c"]), p(s["face_c"]), z_c, None, st), "raster_cam")
            _lib.check(L.harp_rasterize_fwd_keep(p(s["ndc_l"]), p(tp.faces), B, V, F, Sh, 4, p(s["ws_l"]), p(s["face_l"]), p(s["zl"]), p(s["zl_state"]), st),
                "raster_light")
        else:                                            # one view: the rasteriser's own set-up
            _lib.check(L.harp_rasterize_fwd(p(s["ndc_c"]), p(tp.faces), B, V, F, Sh, 0, 0.0, 1.0, p(s["ws_c"]), p(s["face_c"]), z_c, None, st), "raster_cam")
        if shade:
            _lib.check(L.harp_shade_fwd(ctypes.byref(self._shade_struct()), st), "shade_fwd")

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

    # ---- self-contact: what belongs to the topology and the fit's shape, made on first use -----------------------------
    def _rest_vertices(self):
        """(V,3) float64 metres, the rest geometry the exclusion is measured on: the model's template shaped by the fit's betas and
        subdivided by the topology's midpoints; not posed (the mean pose is not added either) and not displaced — the displacements
        and the pose change an edge path by far less than the radius"""
        dm, tp = self.dm, self.topo
        nb = min(int(self.fit["shape"].shape[0]), int(dm.shapedirs_T.shape[0]))
        v = dm.v_template.double().reshape(-1, 3) + (self.fit["shape"][:nb].double() @ dm.shapedirs_T[:nb].double()).view(-1, 3)
        if v.shape[0] != tp.V0:
            raise RuntimeError(f"the model's template has {v.shape[0]} vertices, the topology {tp.V0}")
        if tp.E0 == 0:
            return v
        e = tp.edges0.long()
        return torch.cat([v, 0.5 * (v[e[:, 0]] + v[e[:, 1]])])

    def _exclusion_table(self, geodesic):
        """the exclusion table of harp_mesh_contact_excl for this avatar against itself at the radius `geodesic`, on the device"""
        if geodesic not in self._excl:
            from .selfcontact import geodesic_exclusion, pack_exclusion
            self._excl[geodesic] = pack_exclusion(geodesic_exclusion(self._rest_vertices(), self.topo.faces, geodesic))
        return self._excl[geodesic]

    def _own_part_table(self):
        """the part of every vertex of the subdivided mesh on the device (labels.subdivided_vertex_part_labels)"""
        if self._own_part is None:
            from .labels import subdivided_vertex_part_labels
            tab = subdivided_vertex_part_labels(self._skin_weights, self.topo.edges0.cpu().numpy()[:self.topo.E0])
            if tab.shape[0] != self.topo.V:
                raise RuntimeError(f"{tab.shape[0]} vertex parts for {self.topo.V} vertices")
            self._own_part = torch.from_numpy(tab).to(self.dev)
        return self._own_part

    def _keypoints_batch(self, kp, lo, layers, n_layers, self_layer, scene, tol):
        """harp_keypoint_visibility of this player's batch into rows lo.. of the buffers kp; scene: the scene depth arguments of the batch"""
        s, p = self.s, _lib.ptr
        _lib.check(_lib.lib().harp_keypoint_visibility(p(s["joints_m"]), p(s["cam_R"]), p(s["cam_T"]), self.B, self.n_joints, self.focal_h / self.ss,
                                                       self.S, self.ss, self_layer, layers, n_layers, *scene, tol, kp["uvz"][lo:].data_ptr(),
                                                       kp["vis"][lo:].data_ptr(), _lib.stream()), "keypoint_visibility")

    def _layers(self):
        return [(self, False)]

    def _enqueue_frames(self, n_pad, used, channels, owner):
        """per batch of B frames: its launches up to the shader, then the resolve"""
        s, p, out = self.s, _lib.ptr, self._out["frames"]["out"]
        per = self.S * self.S * channels
        for lo in range(0, n_pad, self.B):
            self._render_batch(self._stage.rows(lo))
            _lib.check(_lib.lib().harp_resolve_u8(p(s["rgb"]), p(s["face_c"]), self.B, self.S, self.ss, *self._stage.args("background", lo, used),
                                                  p(self.bg_color_dev), channels, out[lo * per:].data_ptr(), _lib.stream()), "resolve_u8")

    @torch.no_grad()
    def render(self, rows, background=None, bg_rows=None, alpha=False):
        """Frames `rows` of the loaded motion -> (len(rows), S, S, 3) uint8 on the device ((.., 4) with alpha=True: the covered share of the
        pixel as alpha), a view of the player's buffer that the next call overwrites.  background: None (the constant `bg_color`, white) or
        a (N,S,S,3) uint8 device tensor; frame i is composited over its row bg_rows[i], without bg_rows over row i (N == len(rows)) or row
        0 (N == 1); a row outside [0, N) takes bg_color.  The rows in use are copied into a buffer of the player's in stream order, so
        one captured graph serves every background tensor and the caller's tensor is free again once the call has returned."""
        self._ready()
        return self._frames(rows, dict(background=(background, bg_rows)), alpha)[0]

    @torch.no_grad()
    def annotate(self, rows, parts=True, depth=True, uv=False, keypoints=True, tol=LABEL_TOL):
        """What the frames `rows` of the loaded motion show -> Annotation (above) of device tensors: always owner (1 where the avatar
        is), face and bbox; part with parts=True, depth with depth=True, uv with uv=True, uvz and vis with keypoints=True.  Needs
        keep_depth=True.  The batch's front and rasterisers run as in render (the shader does not: labels need no colour), then
        harp_annotate_layers and harp_keypoint_visibility, under the same graph path.  tol: a joint lies INSIDE the hand, a finger's
        radius or half the palm's thickness under the skin, so a joint counts as visible when the nearest surface at its pixel is no
        nearer than its own depth minus tol metres; 0.02 is that convention, not a tuned value."""
        self._ready(need_depth="annotate")
        a = self._annotate(rows, {}, _label_flags(parts, depth, uv, keypoints, tol))
        return a._replace(bbox=a.bbox[:, 0], uvz=a.uvz and a.uvz[0], vis=a.vis and a.vis[0])      # the one layer's, bare

    @torch.no_grad()
    def flow(self, rows, to_rows, tol=FLOW_TOL):
        """Where the surface point that each pixel of frame rows[i] shows lies in frame to_rows[i] of the loaded motion -> Flow (above) of
        device tensors.  Needs keep_depth=True.  Per batch the front and the rasterisers of the target rows, device copies of their ndc_c
        and z_c, the front and the rasterisers of the source rows and one harp_flow_layers, under a graph key of its own.  tol: the point
        lies on the surface, so the tolerance only absorbs the depth difference between where it lands and the centre of the sub-pixel
        it is tested at; 0.005 is that convention, not a tuned value."""
        self._ready(need_depth="flow")
        return self._flow(rows, {}, (to_rows, {}), tol)

    @torch.no_grad()
    def self_contact(self, rows, max_dist=SELF_CONTACT_DIST, geodesic=SELF_GEODESIC):
        """Where the avatar of the frames `rows` touches ITSELF (a pinch, a fist, crossed fingers) -> SelfContact (above): per vertex the
        signed distance to the nearest face of its own surface that does not lie within `geodesic` metres of it along the mesh's edges
        (selfcontact.geodesic_exclusion on the rest geometry, built on first use per radius), that face and its part, the winding
        number of the whole surface, which parts touch which, and per frame the smallest distance and the deepest penetration.  Per
        batch the front only and one harp_mesh_contact_excl, under a graph key of its own.  A vertex ON a closed surface sees it under
        its exterior-angle share, 0.14 .. 0.82 on the hand at rest, and 1 more when it is inside another part: INSIDE is wind > 1.0.
        max_dist is finite, >= 0 and below geodesic: otherwise the vertex's own neighbourhood just beyond the radius would always be
        "in contact".  SELF_CONTACT_DIST = 0.004 and SELF_GEODESIC = 0.03 are conventions, not tuned values."""
        self._ready()
        return self._self_contact(rows, max_dist, geodesic)[0]

    # ---- a whole motion to files ------------------------------------------------------------------------------------------------
    def play(self, motion, out_dir, backgrounds=None, fmt="jpg", alpha=False, labels=False, label_tol=LABEL_TOL, flow=None, flow_tol=FLOW_TOL,
             self_contacts=False, self_contact_dist=SELF_CONTACT_DIST, self_geodesic=SELF_GEODESIC):
        """load_motion(motion), render it batch by batch and write out_dir/%04d.<fmt> (fmt "jpg" or "png"; alpha=True needs "png" and
        writes RGBA).  backgrounds: None, a (N,S,S,3) uint8 tensor or a directory of images of that size (sorted by name); frame i is
        composited over background i mod N.  The frames leave through two pinned host buffers, one per batch in flight, and are encoded on
        a thread pool while the next batch renders.  labels=True (needs keep_depth=True) also writes part_%04d.png, depth_%04d.png,
        iuv_%04d.png and keypoints.npz (write_labels).  flow="fw" | "bw" | "both" (needs keep_depth=True) also writes flow_%04d.flo and /
        or flow_bw_%04d.flo with their status PNGs (write_flow).  self_contacts=True also writes self_contacts.npz (write_self_contacts)
        with self_contact(rows, self_contact_dist, self_geodesic) of every frame.  Returns the list of paths."""
        _flow_mode(flow), _tol(flow_tol)
        if self_contacts:
            _self_contact_args(self_contact_dist, self_geodesic)

        def prepare():
            self.load_motion(motion)
            bgs = load_backgrounds(backgrounds, self.S, self.dev)
            return lambda rows: self.render(rows, bgs, None if bgs is None else rows % bgs.shape[0], alpha)
        paths = self._play(out_dir, fmt, alpha, prepare)
        if labels:
            self._ready(need_depth="annotate")
            flags = _label_flags(True, True, True, True, label_tol)
            write_labels(out_dir, self.T, self.B, lambda rows: self._annotate(rows, {}, flags), [part_names_of(self)])
        if flow:
            write_flow(out_dir, self.T, self.B, lambda rows, to: self.flow(rows, to, tol=flow_tol), flow)
        if self_contacts:
            write_self_contacts(out_dir, self.T, self.B, lambda rows: self._self_contact(rows, self_contact_dist, self_geodesic),
                                [part_names_of(self)], self_contact_dist, self_geodesic)
        return paths


class ScenePlayer(_Player):
    """Several avatars in one frame with depth-correct occlusion: 1 to 4 AvatarPlayers built with keep_depth=True on one
    device with equal img_size, ss and batch_size — one camera: the focal length is the players' too, the translation comes from each
    motion's cam — rendered batch by batch into their own buffers and resolved by ONE harp_composite_layers_u8 per batch: per sub-sample
    the nearest avatar in front of an optional scene depth.  flip: one bool per player; a flipped avatar is shown mirrored in x, light
    included — a LEFT hand is a right-hand fit of horizontally mirrored frames shown with flip.  The avatars cast no shadows on each
    other.  The launches are captured into a graph when every player was built with use_graph=True."""

    _holds, _load = "the motions hold", "load_motions"

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

    def _layers(self):
        return list(zip(self.players, self.flip))

    def _alloc_frames(self, n):
        return dict(super()._alloc_frames(n), owner=torch.empty(n, self.S, self.S, dtype=torch.uint8, device=self.dev))

    def _enqueue_frames(self, n_pad, used, channels, owner):
        """per batch: every player's front / rasterisers / shader, then one composite"""
        p, B, bufs = _lib.ptr, self.B, self._out["frames"]
        per = self.S * self.S * channels
        layers = (_lib.Layer * len(self.players))(*[_lib.Layer(p(pl.s["rgb"]), p(pl.s["z_c"]), int(f), 0) for pl, f in self._layers()])
        for lo in range(0, n_pad, B):
            for pl in self.players:
                pl._render_batch(self._stage.rows(lo))
            _lib.check(_lib.lib().harp_composite_layers_u8(layers, len(self.players), B, self.S, self.ss, *self._scene_depth_args(lo, used),
                                                           *self._stage.args("background", lo, used), p(self.bg_color_dev), channels,
                                                           bufs["out"][lo * per:].data_ptr(), bufs["owner"][lo:].data_ptr() if owner else None,
                                                           _lib.stream()), "composite_layers_u8")

    def _alloc_contact(self, n):
        """per ordered pair (query k, target j) the three outputs of harp_mesh_contact over every padded row; one workspace, for the
        target with the most faces (the calls follow each other on one stream)"""
        new = lambda dt, V: torch.empty(n, V, dtype=dt, device=self.dev)      # noqa: E731
        pairs = {(k, j): (new(torch.float32, q.topo.V), new(torch.int32, q.topo.V), new(torch.float32, q.topo.V))
                 for k, q in enumerate(self.players) for j in range(len(self.players)) if j != k}
        ws = torch.empty(max(_lib.lib().harp_mesh_contact_ws_floats(self.B, pl.topo.F) for pl in self.players), dtype=torch.float32, device=self.dev)
        return dict(pairs=pairs, ws=ws)

    def _enqueue_contact(self, n_pad, used, max_dist):
        """per batch every player's front only, then one harp_mesh_contact per ordered pair of players into the pair's rows.  max_dist is
        part of the pass and so of the graph key, as flow's and the labels' tol are: every distinct value captures a graph of its own,
        kept until the scene grows or new tables are loaded"""
        p, B, bufs = _lib.ptr, self.B, self._out["contact"]
        meshes = [pl._contact_mesh(f) for pl, f in self._layers()]
        for lo in range(0, n_pad, B):
            for pl in self.players:
                pl._render_batch(self._stage.rows(lo), front_only=True)
            for (k, j), (d, f, w) in bufs["pairs"].items():
                _lib.check(_lib.lib().harp_mesh_contact(ctypes.byref(meshes[k]), ctypes.byref(meshes[j]), B, max_dist, p(bufs["ws"]),
                                                        d[lo:].data_ptr(), f[lo:].data_ptr(), w[lo:].data_ptr(), _lib.stream()), "mesh_contact")

    @torch.no_grad()
    def render(self, rows, background=None, bg_rows=None, alpha=False, scene_depth=None, depth_rows=None, owner=False):
        """Scene rows `rows` of the loaded motions -> (len(rows), S, S, 3|4) uint8 on the device, a view of the scene's buffer that the
        next call overwrites; with owner=True (frames, owner (len(rows), S, S) uint8: 0 = background, 1 + the player that shows most of
        the pixel).  background / bg_rows / alpha: as AvatarPlayer.render.  scene_depth: None or a float32 (N,S,S) device tensor at output
        resolution in the unit of the avatars' view depth (a value > 0 is a measurement and hides what lies behind it); frame i is tested
        against its row depth_rows[i], without depth_rows against row i (N == len(rows)) or row 0 (N == 1); a row outside [0, N) means no
        scene depth.  Backgrounds and depths in use are copied into buffers of the scene's, so one captured graph per (padded length,
        background?, depth?, channels, owner?) serves every tensor."""
        self._ready()
        frames, n = self._frames(rows, dict(background=(background, bg_rows), scene_depth=(scene_depth, depth_rows)), alpha, owner)
        return (frames, self._out["frames"]["owner"][:n]) if owner else frames

    @torch.no_grad()
    def annotate(self, rows, parts=True, depth=True, uv=False, keypoints=True, tol=LABEL_TOL, scene_depth=None, depth_rows=None):
        """What the scene's frames `rows` show -> Annotation, as AvatarPlayer.annotate: owner is bit for bit render(owner=True)'s, bbox is
        (n, players, 4), and uvz and vis are tuples with one tensor per player (its own joints; the occluder 1 + k is player k, 255 the
        scene depth).  scene_depth, depth_rows: as render."""
        self._ready()
        return self._annotate(rows, dict(scene_depth=(scene_depth, depth_rows)), _label_flags(parts, depth, uv, keypoints, tol))

    @torch.no_grad()
    def flow(self, rows, to_rows, tol=FLOW_TOL, scene_depth=None, depth_rows=None, depth_to_rows=None):
        """Where the surface point that each pixel of scene frame rows[i] shows lies in scene frame to_rows[i] -> Flow, as
        AvatarPlayer.flow: the source point is annotate's (the same owner, face and uv), the occluder 1 + k is player k, 255 the scene
        depth.  scene_depth: as render; frame rows[i] is composited against its row depth_rows[i] and the point is tested at the target
        against its row depth_to_rows[i] (each without its rows: row i when N == len(rows), row 0 when N == 1)."""
        self._ready()
        return self._flow(rows, dict(scene_depth=(scene_depth, depth_rows)), (to_rows, dict(scene_depth=(scene_depth, depth_to_rows))), tol)

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
        self._ready()
        max_dist = float(max_dist)
        if not max_dist >= 0:
            raise ValueError(f"max_dist must not be negative or NaN, got {max_dist}")
        tabs = [pl._part_table() for pl in self.players]
        n = self._render(rows, {}, ("contact", max_dist))
        pairs = self._out["contact"]["pairs"]
        return compose_contact([{j: tuple(t[:n] for t in pairs[k, j]) for j in range(len(self.players)) if j != k}
                                for k in range(len(self.players))], tabs)

    @torch.no_grad()
    def self_contact(self, rows, max_dist=SELF_CONTACT_DIST, geodesic=SELF_GEODESIC):
        """Where every avatar of the scene's frames `rows` touches itself -> a tuple of SelfContact, one per player, each what that
        player's own AvatarPlayer.self_contact gives for its motion (a flipped player is mirrored on both sides: the same distances,
        faces and parts).  One player is enough.  Contact BETWEEN the avatars is contact()."""
        self._ready()
        return self._self_contact(rows, max_dist, geodesic)

    def play(self, motions, out_dir, backgrounds=None, scene_depth=None, fmt="jpg", alpha=False, masks=False, labels=False, label_tol=LABEL_TOL,
             flow=None, flow_tol=FLOW_TOL, contacts=False, contact_dist=CONTACT_DIST, self_contacts=False, self_contact_dist=SELF_CONTACT_DIST,
             self_geodesic=SELF_GEODESIC):
        """load_motions(motions), render the scene batch by batch and write out_dir/%04d.<fmt> as AvatarPlayer.play does; with masks=True
        also out_dir/mask_%04d.png, the owner map (8-bit grey: 0 background, 1 + the player).  backgrounds: as AvatarPlayer.play;
        scene_depth: None, a float32 (N,S,S) tensor or a directory (load_scene_depth), frame i tested against depth i mod N.  labels=True
        also writes the label files (write_labels), one keypoints_<k>.npz per player k when there are several.  Returns the list of the
        frames' paths.  flow="fw" | "bw" | "both" also writes the flow files (write_flow).  contacts=True (at least two players) also
        writes contacts.npz (write_contacts) with contact(rows, contact_dist) of every frame.  self_contacts=True also writes
        self_contacts.npz (write_self_contacts) with self_contact(rows, self_contact_dist, self_geodesic) of every frame."""
        _flow_mode(flow), _tol(flow_tol)
        if self_contacts:
            _self_contact_args(self_contact_dist, self_geodesic)
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
        if self_contacts:
            write_self_contacts(out_dir, self.T, self.B, lambda rows: self.self_contact(rows, self_contact_dist, self_geodesic),
                                [part_names_of(pl) for pl in self.players], self_contact_dist, self_geodesic)
        return paths


def part_names_of(player):
    """the label names of an AvatarPlayer's model, index = label (labels.part_names of its hand layer)"""
    from .labels import joint_part_names
    return joint_part_names(player._skin_weights.shape[1])


def _tol(tol):
    import math
    tol = float(tol)
    if not (tol >= 0 and math.isfinite(tol)):
        raise ValueError(f"tol must be non-negative and finite, got {tol}")
    return tol


def _label_flags(parts, depth, uv, keypoints, tol):
    return (bool(parts), bool(depth), bool(uv), bool(keypoints), _tol(tol))


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


def _self_contact_args(max_dist, geodesic):
    """max_dist finite and >= 0, geodesic > max_dist (inf allowed: every face the vertex is connected to is excluded) -> both as floats"""
    max_dist, geodesic = float(max_dist), float(geodesic)
    if not (max_dist >= 0 and math.isfinite(max_dist)):
        raise ValueError(f"max_dist must be finite and not negative, got {max_dist}")
    if not geodesic > max_dist:
        raise ValueError(f"geodesic must exceed max_dist = {max_dist} (a vertex's own neighbourhood just beyond the radius would always be "
                         f"in contact), got {geodesic}")
    return max_dist, geodesic


def compose_self_contact(dist, face, wind, part_table, own_part, n_parts):
    """The documented rule from harp_mesh_contact_excl's outputs of a mesh against itself to SelfContact, in torch ops on the device.
    dist, face, wind (n,V); part_table (F,) uint8 the part of every face; own_part (V,) uint8 the part of every vertex; n_parts = P.
    The distance is negated where the (unmasked) winding number exceeds 1.0; touch[t, p, q] is set by every vertex of part p whose
    nearest counting face within max_dist is of part q.  Every tensor returned is new."""
    hit = face >= 0
    part = torch.where(hit, part_table[face.clamp(min=0).long()], torch.zeros_like(face, dtype=torch.uint8))
    inside = wind > 1.0
    pair = own_part.long()[None, :] * n_parts + part.long()
    touch = torch.zeros(dist.shape[0], n_parts * n_parts, dtype=torch.int32, device=dist.device)
    touch.scatter_reduce_(1, pair, hit.to(torch.int32), "amax", include_self=True)
    signed = torch.where(inside, -dist, dist)
    deep = torch.where(inside, dist, torch.zeros_like(dist)).amax(1).clamp(min=0)
    return SelfContact(signed, face.clone(), part, own_part.clone(), wind.clone(), touch.bool().view(-1, n_parts, n_parts), signed.amin(1), deep)


def write_self_contacts(out_dir, T, B, self_contact, names, max_dist, geodesic):
    """self_contacts.npz of a played motion beside its frames, batch by batch: per player k dist_k (T,V_k) float32 signed metres (+inf:
    none), face_k (T,V_k) int32, part_k (T,V_k) uint8, wind_k (T,V_k) float32, touch_k (T,P_k,P_k) bool, own_part_k (V_k,) uint8 and
    part_names_k; min_dist (T,) and max_penetration (T,) float32 over all players; max_dist and geodesic, the two distances used.
    self_contact(rows) -> one SelfContact per player; names: one list of part names per player."""
    P = len(names)
    keys = ("dist", "face", "part", "wind", "touch")
    got = {f"{key}_{k}": [] for key in keys for k in range(P)}
    per_frame = dict(min_dist=[], max_penetration=[])
    own = {}
    for lo in range(0, T, B):
        cs = self_contact(np.arange(lo, min(T, lo + B)))
        for k, c in enumerate(cs):
            for key in keys:
                got[f"{key}_{k}"].append(getattr(c, key).cpu().numpy())
            own[f"own_part_{k}"] = c.own_part.cpu().numpy()
        per_frame["min_dist"].append(torch.stack([c.min_dist for c in cs]).amin(0).cpu().numpy())
        per_frame["max_penetration"].append(torch.stack([c.max_penetration for c in cs]).amax(0).cpu().numpy())
    path = os.path.join(out_dir, "self_contacts.npz")
    np.savez(path, max_dist=np.float32(max_dist), geodesic=np.float32(geodesic), **own,
             **{k: np.concatenate(v) for k, v in {**got, **per_frame}.items()}, **{f"part_names_{k}": np.array(names[k]) for k in range(P)})
    return path


def _flow_mode(flow):
    if flow not in (None, "fw", "bw", "both"):
        raise ValueError(f'flow is None, "fw", "bw" or "both", got {flow!r}')
    return flow


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
        for k in range(P):
            kp[k]["uvz"].append(a.uvz[k].cpu().numpy()); kp[k]["vis"].append(a.vis[k].cpu().numpy()); kp[k]["bbox"].append(a.bbox[:, k].cpu().numpy())
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
