"""Fused render-and-compare step: the loop body of the reference's `optimize_hand_sequence`
(optimize_sequence.py:446-579) as one pre-planned sequence of HIP kernel launches over pre-allocated HBM buffers,
replayable as a hipGraph, with one RCCL all-reduce of the flat gradient arena between backward and Adam.

What the reference does per step with ~600 torch/PyTorch3D kernel launches, >= 8 host syncs and CPU-resident
parameters, this does with 28 launches (hand mesh, texel records; 24 in the table form; 28 + 4 for the SMPL-X arm), no host sync and everything resident:

  hand_front (schedule row, frame set-up, LBS, subdivide, normals + displace, normals, both projections, light camera; arm: 5 launches) ->
  raster(cam, K=1 + soft silhouette + its L1) || raster(light, K=1) || parameter / mesh regularisers ->
  shade_bwd (recomputes the colour, forms the photometric L1, writes y_pred when asked) || silhouette_bwd -> depth_bwd ->
  mesh chain + hand / arm layer backward on four workgroups per frame (6 / 7 launches) -> [all-reduce] -> Adam

(the building blocks behind the fused launches — frame_setup, LBS, subdivide, normals, project, centroid, light_setup, shade and
their backward passes — are separate C-ABI entry points and stay reachable through the `fused_*` switches; tests compare the two).

Layout: `SWITCHES` is the one table of switches (attributes, HARP_ENG names and the graph-cache key come from it); `FitEngine._plan` turns
them and a step's arguments into a `_StepPlan`, and `FitEngine._fb` enqueues the step from it, phase by phase (tests/test_gpu_step_trace.py).

Parameters live in ONE flat fp32 arena (and one gradient / exp_avg / exp_avg_sq arena of the same layout); the
reference's parameter dict (optimize_sequence.py:181-250) is exposed as views into it (`params`).
Multi-GPU: frames are sharded over ranks, every rank holds the full arena; gradients are summed with one all_reduce
and scaled by 1/world inside the Adam kernel (SURVEY.md §5 "Data-parallel semantics").
"""
import ctypes
import os
import weakref
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, ops
from .manopth.manolayer import ManoDeviceModel

LOSS_NAMES = ["silhouette", "kps_anchor", "vert_disp_reg", "laplacian", "normal", "arap", "photo", "albedo", "normal_reg"]
LOSS_WEIGHTS = {"silhouette": 7.0, "kps_anchor": 10.0, "vert_disp_reg": 2.0, "laplacian": 4.0, "normal": 0.1, "arap": 0.2,
                "photo": 1.0, "albedo": 0.5, "normal_reg": 0.1}                     # optimize_sequence.py:411-422 (vgg: §8f "next")
BG_COLOR = (1.0, 1.0, 1.0)          # background of the shading pass (renderer_helper.py BlendParams default)
COARSE_TERMS = LOSS_NAMES[:6]
APP_TERMS = LOSS_NAMES[6:]


class _Switch(NamedTuple):
    name: str
    default: object                  # a value, or a function of the engine (evaluated in table order, after the entries above it)
    doc: str


def _wide_ok(e):
    return bool(e.fused_front and (e.topo.V + 3) // 4 <= 1024)


# Every switch of the engine: `__init__` sets them as plain attributes (tests, bench.py and tools/dev flip them directly), HARP_ENG accepts
# exactly these names, and step() keys its graph cache on every one of them, in this order.  All on in production unless a measurement
# says otherwise; all result-neutral (tests/test_gpu_parity.py::test_schedule_switches_give_the_default_schedules_result).
SWITCHES = (
    _Switch("fused_chain", lambda e: bool(e.topo.V <= _lib.lib().harp_mesh_chain_max_vertices()), "per-frame fused mesh chain (csrc/chain.hip): 22 launches -> 2; needs the frame's mesh to fit its LDS staging"),
    _Switch("fused_front", lambda e: bool(e.fused_chain and (e.n_joints == 21 or e.use_arm)), "MANO path: frame set-up + hand layer + mesh chain + rasteriser set-up of both views as ONE launch (csrc/hand_front.hip); SMPL-X arm path: the same as "
            "three + four launches around the shared MFMA contractions (csrc/arm_front.hip)"),
    _Switch("fused_back", True, "... and the backward tail as three launches instead of six (csrc/hand_back.hip)"),
    _Switch("wide_front", lambda e: _wide_ok(e) and e.use_arm, "the front on FOUR workgroups per frame (csrc/chain_wide.hip, hand_front_wide_kernel): a quarter of the vertices per workgroup, one pass per stage, kernel boundaries where the parts "
            "meet — three launches of 4 B workgroups instead of one of B.  Measured (tools/dev/bench_ab.sh, fresh processes = the burst regime bench.py reports; tools/dev/gpu_wide_ab.py, sustained): the wide TAIL wins everywhere (hand -13 ... -16 "
            "us / step, arm -25); the wide FRONT wins on the arm (-10 ... -35 us) and in sustained runs of the hand path (-17 us), but LOSES on the hand path in a fresh process (+12 ... +20 us: three dependent nodes instead of one in front of a "
            "0.65-ms step whose second stream is the longer branch of the fork) — off there"),
    _Switch("hybrid_front", False, "hand path: hand layer on four workgroups per frame + one-workgroup mesh chain (two launches)"),
    _Switch("front_auto", lambda e: _wide_ok(e) and not e.use_arm, "hand path: the form of the front is chosen per stage (see _front_form); False: wide_front / hybrid_front as set"),
    _Switch("wide_back", _wide_ok, "the tail: mesh-chain backward + per-vertex hand / arm layer backward on four workgroups per frame"),
    _Switch("overlap", True, "second HIP stream (light view, silhouette backward, parameter-only terms); False: one stream"),
    _Switch("early_terms", True, "parameter-only terms / mesh regularisers scheduled on the second stream"),
    _Switch("packed_texels", True, "shaders read the interleaved albedo + normal-map array (harp_pack_texels)"),
    _Switch("auto_draw", True, "draw fresh texture-regulariser offsets every step (False: the caller draws)"),
    _Switch("overlap_allreduce", True, "N > 1: all-reduce of the map gradients overlapped with the mesh / LBS backward"),
    _Switch("graph_collectives", False, "N > 1 over torch.distributed (no RcclComm): capture its all-reduce into the step graph (opt-in)"),
    _Switch("force_allreduce", False, "run the N > 1 code path on a single rank (tests, bench HARP_FORCE_DIST)"),
    _Switch("fused_loss", True, "loss-only mode: photometric L1 formed inside the shader backward (no forward shading launch)"),
    _Switch("graph_order", True, "capture the critical path first at every fork (see _StepPlan.capture_critical_first)"),
    _Switch("mesh_third", False, "key-point / mesh regularisers on a third stream (their own graph branch) instead of in front of the light view.  Round 3: 0.755 vs 0.766 ms / step with the third stream (three launches incl. their clear).  Round 4, "
            "with ONE launch for the terms, the clear inside hand_front and the texture regularisers throttled: 0.6665 vs 0.6695 without it (the shader backward joins one stream instead of two; the light view has the slack), C5 1.740 vs 1.752 — off"),
    _Switch("keep_depth", True, "light-view depth map kept across steps (harp_rasterize_fwd_keep): empty super-tiles are filled with -1 once, not every step (25 MB)"),
    _Switch("consume_gzl", True, "the depth backward clears the shadow-map gradient entries it consumes: no per-step clear of that image (33.5 MB at B = 32, 512^2)"),
    _Switch("fused_keep", True, "keep_image with the fused loss: the shader backward also writes y_pred (no forward shading launch either)"),
    _Switch("keep_image", True, "shader forward writes the rendered image s['rgb'] (False: loss + gradient only)"),
    _Switch("mesh_terms_late", False, "key-point / mesh terms on the second stream behind the silhouette backward (beside the shader backward)"),
    _Switch("sil_late", False, "silhouette backward after the shader backward instead of beside it (measured: see profiles/r05_wide_ab.txt)"),
    _Switch("paired_setup", False, "rasteriser set-up of both views as three launches on the main stream (harp_raster_setup_pair; the light raster no longer waits for three set-up launches of its own on the second stream).  Measured, same box: hand "
            "+7 us / step (B = 32), +5 (B = 18), arm +15; together with wide_front -3 ... +5: off (profiles/r05_wide_ab.txt)"),
    _Switch("late_texture_terms", False, "texture regularisers (atomics-bound, 40 us) enqueued on the second stream BEHIND the light view instead of in front of it — the light view then starts at the fork, not when the regularisers are done"),
    _Switch("mesh_terms_first", True, "key-point term + mesh regularisers run before the light raster (under the raster set-up) instead of after it"),
    _Switch("fused_bwd", False, "shading + silhouette backward in ONE launch (harp_shade_sil_bwd): correct, measured SLOWER (1.05 vs 0.93 ms: the rasteriser tiles inherit 168 VGPRs / 3 waves per SIMD)"),
    _Switch("tail_side", False, "normal-map chain rule (+ early all-reduce) on the second stream: measured SLOWER (0.960 vs 0.948 ms: the extra cross-stream edge costs more than the 5-us kernel it moves)"),
    _Switch("camera_first", True, "enqueue the camera-view raster chain (the longer one) before the light-view chain: +0.75 %"),
    _Switch("zl_tile_flags", lambda e: e.S >= 1024, "the shader backward flags the light-view tiles it adds a shadow-tap gradient to and the depth backward reads only those (42 % of the tiles it visits at 512^2, 51 % at 1024^2 on the arm).  The "
            "flag is one more dependent load per tile: at 512^2, where a workgroup of the depth backward walks <= 2 tiles, it costs what it saves (0.704 vs 0.701 ms / step); at 1024^2 (8 tiles per workgroup) it wins (1.777 vs 1.788 ms / step on the "
            "arm) — on from 1024 px"),
    _Switch("texel_records", lambda e: bool(_lib.lib().harp_texel_bins(e.Ht, e.Wt) <= 1024 and e.world == 1), "the shader backward hands the texture / normal-map gradients on as one record per shaded pixel, binned by 32x32-texel UV tile, and "
            "harp_texel_reduce (csrc/texel_reduce.hip) adds them up on a branch of its own that joins in front of Adam — beside the mesh / hand backward tail instead of inside the shader backward (its LDS texel table, flush and ~12 M memory atomics "
            "per launch are gone).  N > 1: the table form — the map gradients are final ~60 us earlier, which is what their early all-reduce overlaps with; switchable"),
    _Switch("trec_cap_div", 32, "capacity of a tile's record list = B * S * S / this (>= trec_cap_min): 3.5x the fullest list of the bench scenes; a full list falls back to memory atomics"),
    _Switch("trec_cap_min", 65536, "(see trec_cap_div)"),
    _Switch("vert9", True, "the shader backward's vertex gradients as ONE interleaved (B,V,9) buffer (a 36-byte run per vertex and wave instead of three 12-byte runs: a third of the memory-atomic lines), unpacked into the three arrays by extra "
            "workgroups of the depth backward's launch"),
    _Switch("vgg_streams", 2, "perceptual term: the batch in this many parts on as many streams (harp_vgg16_term_args.side_streams; 1 - 4)"),
    _Switch("split_adam", True, "with the texel records: the maps' Adam update on the second stream behind harp_texel_finish, the step's last launch only for the small parameters"),
    _Switch("fused_sil_bwd", False, "the silhouette backward inside the camera-view raster launch (harp_rasterize_l1_fwd_bwd) instead of a launch of its own beside the shader backward.  Correct (tests) and measured SLOWER: the shader backward gains "
            "32 us without its neighbour (230 -> 198 in the graph), the camera raster pays 56 (198 -> 254: 94 VGPRs / 26 KB of LDS = 5 waves per SIMD instead of 7, and the rim walk is ~25 us of VALU work wherever it runs): step 0.665 vs 0.638 ms "
            "(profiles/r06_ab_record.txt)"),
    _Switch("sil_records", True, "silhouette records (harp_sil_records_bind): the camera raster's soft pass stores its (pixel, face) pairs per 16x16 tile and the silhouette backward walks them instead of reading alpha / g_alpha of every tile and "
            "staging the tile's faces again.  Step -19 us, geometry-only stage -24 us (profiles/r07_ab_record.txt).  Off with fused_sil_bwd / fused_bwd"),
    _Switch("sil_rec_cap", 512, "a tile with more than this many pairs takes the staged walk (512: 2.7x the fullest hand tile at 512^2, ~0.1 % of the arm's tiles at 1024^2 go over)"),
    _Switch("lean_app_stage", False, "appearance-only stage without the geometry gradients nothing reads (set by optimize_hand_sequence; off by default: g_buf then holds what autograd would).  The optimiser of that stage holds texture, normal map, "
            "light position and ambient ratio (optimize_sequence.py:264-310) — the reference's autograd still differentiates through the whole mesh chain and hand layer and throws those gradients away.  Lean: the shader backward forms no vertex "
            "gradients, the chain backward only its light-view part (-> light position), no hand-layer backward.  Same parameters after the step; g_buf's geometry segments stay zero"),
    _Switch("sil_only_raster", True, "geometry-only steps without a kept image: the camera raster forms no nearest-face ids (harp_rasterize_l1_fwd with face_id == NULL)"),
    _Switch("fold_step", True, "scheduled steps: the batch row is fetched by hand_front itself, the loss vector / schedule row / draw counter are turned over by hand_back, the slab clear + Adam tick + offset draw are ONE launch (harp_step_frame, "
            "harp_step_prologue): 31 -> 23 kernels per step, no schedule kernel in front of the hand layer"),
    _Switch("fused_terms", True, "normalise + pack, the four parameter-only regularisers, key-point + mesh terms, depth backward + normal-map chain rule: one launch each (were 2 + 4 + 2 + 2)"),
    _Switch("graph_perceptual", True, "capture the perceptual term into the step's graph (False: steps with the term run eagerly)"),
)
SWITCH_NAMES = tuple(sw.name for sw in SWITCHES)


def apply_env_switches(eng, text):
    """HARP_ENG="switch=0,other=1": switches of `eng` from the environment (A/B runs of bench.py and the tools).  Only names of the
    SWITCHES table are taken; the value is converted by the type of the switch's current value."""
    for kv in filter(None, text.split(",")):
        k, v = kv.split("=")
        if k not in SWITCH_NAMES:
            raise ValueError(f"HARP_ENG: no engine switch {k!r}")
        setattr(eng, k, type(getattr(eng, k))(int(v)))
        if k in ("wide_front", "hybrid_front"):
            eng.front_auto = False                       # an explicit form is an explicit form


class _StepPlan(NamedTuple):
    """every derived decision of one step (FitEngine._plan), written there and nowhere else"""
    lean: bool                       # appearance-only stage without the geometry gradients (`lean_app_stage`)
    fold: bool                       # the step's book-keeping rides in hand_front / hand_back / harp_step_prologue (`fold_step`)
    shadow: bool                     # the light view exists (appearance stage with self-shadowing)
    one_stream: bool                 # everything on the main stream, no waits
    fill_side: bool                  # the loss vector (all the main stream touches of the slab before the join) is clear already, by the schedule launch or hand_back: the slab clear runs on the second stream, off the head of the step
    mesh_on_third: bool              # key-point / mesh terms (and the clear of g_vd / g_joints_m) on a third stream
    capture_critical_first: bool     # hand layer before the second stream's fork, shader backward before the silhouette backward, ...
    fused_sil: bool                  # the silhouette backward inside the camera-view raster launch
    sil_records: bool                # the camera raster stores (pixel, face) pairs, the stand-alone silhouette backward walks them
    fuse_bwd: bool                   # shader + silhouette backward as ONE launch (harp_shade_sil_bwd)
    fused_loss: bool                 # no forward shading launch: the shader backward forms the photometric L1 itself
    mesh_late: bool                  # key-point / mesh terms behind the silhouette backward on the second stream
    paired: bool                     # rasteriser set-up of both views as one launch chain on the main stream
    records: bool                    # map gradients as texel records, reduced by harp_texel_reduce / harp_texel_finish
    nmap_in_depth: bool              # the normal map's chain rule rides in the depth backward's launch
    v9: bool                         # the shader backward writes interleaved vertex gradients, something unpacks them
    v9_riders: bool                  # ... the depth backward's riders do (harp_depth_bwd_riders)
    sparse: int                      # raster flag: 2 = leave images unwritten in super-tiles without a face (nothing kept reads them)
    face_ids: bool                   # the camera raster forms nearest-face ids
    front_form: Optional[str]        # "one" / "hybrid" / "wide" launch form of the fused front; None: building blocks
    back_form: str                   # "one" / "wide" fused tail; "chain": mesh-chain backward + blocks; "blocks"
    prologue: bool                   # slab clear + Adam tick + offset draw as ONE launch (harp_step_prologue)
    draw: bool                       # this step draws texture-regulariser offsets
    tex_late: bool                   # texture regularisers behind the light view (`late_texture_terms`)
    sil_where: Optional[str]         # stand-alone silhouette backward: "main" / "side" (captured before the shader backward) / "after" it, behind the join's event / "late", behind the shader backward's (`sil_late`); None
    maps_where: Optional[str]        # map gradients: "records" (second-stream branch) / "records_main" / "depth" / "side" / "main"; None
    depth_form: Optional[str]        # depth backward: "riders" / "nmap" (with the chain rule) / "tiles" / "consume" / "plain"; None: no light view
    camera_first: bool               # the camera-view chain is enqueued before the light view's
    params_where: str                # parameter-only terms: "side_first" (forked before the front) / "side" (captured behind it) / "main"
    mesh_where: str                  # key-point / mesh terms: "third_first" (captured before the light view) / "third" / "before_light" / "after_light" / "with_sil" / "main"
    clear_mesh: Optional[str]        # who clears g_vd / g_joints_m: "main" / "side" / "third"; None: hand_front (folded step)
    mark_zero: bool                  # the slab clear on the second stream is marked for the camera raster (fused silhouette backward)
    advance_draw: bool               # harp_texture_terms advances the draw counter (drawn by the prologue, not folded)
    join_side: bool                  # the main stream joins the second one in front of the geometry tail
    late_clear: bool                 # g_zl is cleared every step, on the second stream (its consumer does not: `consume_gzl` off)


class _Streams:
    """The streams of one step: `main` (current on entry), `side` (the second stream) and further named ones.  In single-stream mode
    (`overlap` off: kernels timed with events) they are all `main`, and wait / record enqueue nothing at all: a stream waiting for
    itself is legal but has crashed hipStreamEndCapture."""

    def __init__(self, eng, one):
        self.one, self.main, self._eng = one, torch.cuda.current_stream(), eng
        self.side = self.extra("side")

    def extra(self, name):                               # further graph branches (hipGraph replays four concurrently here)
        return self.main if self.one else self._eng._extra_stream(name)

    def wait(self, stream, on=None):
        """`stream` waits for an event, for another stream, or (None) for the main stream"""
        if not self.one:
            stream.wait_event(on) if isinstance(on, torch.cuda.Event) else stream.wait_stream(on or self.main)

    def record(self, stream):
        return None if self.one else stream.record_event()


# launch forms of the fused front and tail -> entry point behind "harp_hand_" / "harp_arm_" (the wide forms take the wide workspace)
_FRONT = {"one": "front_fwd", "hybrid": "front_hybrid_fwd", "wide": "front_wide_fwd"}
_BACK = {"one": "back_bwd", "wide": "back_wide_bwd"}


class _Arena:
    """Flat fp32 buffer with named, 64-float aligned segments."""

    def __init__(self, spec, device):
        self.offsets, off = {}, 0
        for name, shape in spec:
            n = int(np.prod(shape)) if len(shape) else 1
            self.offsets[name] = (off, n, tuple(shape))
            off += (n + 63) // 64 * 64
        self.size = off
        self.device = device

    def alloc(self):
        return torch.zeros(self.size, dtype=torch.float32, device=self.device)

    def view(self, buf, name):
        off, n, shape = self.offsets[name]
        return buf[off:off + n].view(shape)

    def span(self, first, last):
        o0 = self.offsets[first][0]
        o1, n1, _ = self.offsets[last]
        return o0, (o1 + n1 + 63) // 64 * 64 - o0


class FitEngine:
    """One rank's share of a HARP fitting job.

    model: MANO-shaped dict (numpy) — v_template, shapedirs, posedirs, J_regressor, weights, hands_mean.
    topo: harp_amd.synth.build_topology(...) dict; verts_uvs/faces_uvs/uv_mask: template UV data.
    input_params: dict of (T,.) tensors as `init_params` consumes (pose, rot, trans, shape, cam, joints).
    """

    def __init__(self, model, topo, verts_uvs, faces_uvs, uv_mask, input_params, img_size, focal_length, batch_size,
                 device="cuda", self_shadow=True, share_light_position=True, tex_size=512, rank=0, world_size=1, seed=0,
                 use_arm=False, opt_arm_pose=False):
        self.dev = torch.device(device)
        self.S, self.focal, self.B = int(img_size), float(focal_length), int(batch_size)
        self.self_shadow, self.share_light = bool(self_shadow), bool(share_light_position)
        self.rank, self.world = rank, world_size
        self.topo = ops.DeviceTopology(topo, verts_uvs, faces_uvs, self.dev)
        self.use_arm, self.opt_arm_pose = bool(use_arm), bool(opt_arm_pose)
        if self.use_arm:                                                              # SMPL-X right arm (config use_arm, utils/config_utils.py:6)
            from .hand_models_harp.body_models import TreeDeviceModel
            self.dm = TreeDeviceModel(model, self.dev)
            self.n_joints, self.pose_stride, self.n_betas = 22, 51, self.dm.NB
        else:
            self.dm = ManoDeviceModel(model, self.dev)
            self.n_joints, self.pose_stride, self.n_betas = 21, 48, 10
        T = input_params["pose"].shape[0]
        self.T, V = T, self.topo.V
        self.Ht = self.Wt = tex_size
        # ---- parameter arena: [coarse group | appearance group | not optimised]  (optimize_sequence.py:253-310)
        spec = [("pose", (T, 45)), ("cam", (T, 3)), ("verts_disps", (V, 1)), ("shape", (10,)), ("rot", (T, 3)), ("wrist_pose", (T, 3)),
                ("light_positions", (T, 3)), ("amb_ratio", ()), ("texture", (1, tex_size, tex_size, 3)), ("normal_map", (1, tex_size, tex_size, 3)),
                ("trans", (T, 3))]
        self.arena = _Arena(spec, self.dev)
        self.p_buf, self.m_buf, self.v_buf = (self.arena.alloc() for _ in range(3))
        # everything that is zeroed at the start of a step lives in ONE slab (a single fill kernel): the per-frame gradient scratch, the
        # normal-map gradient, the gradient arena and the loss vector (_alloc_scratch)
        self.fid = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self.tfid = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self.nmap_n = torch.empty(tex_size, tex_size, 3, dtype=torch.float32, device=self.dev)
        self.texnm = torch.empty(tex_size, tex_size, 8, dtype=torch.float32, device=self.dev)      # interleaved albedo + normal map
        self._alloc_scratch()
        self.g_buf, self.g_nmap_n, self.loss_vec = (self.s[k] for k in ("g_buf", "g_nmap_n", "loss_vec"))
        self._extra = {}                                # the step's second stream, its further ones and the communication stream by name, created when first used
        self.params = {k: self.arena.view(self.p_buf, k) for k, _ in spec}
        self.grads = {k: self.arena.view(self.g_buf, k) for k, _ in spec}
        # rot / wrist_pose join the coarse group only under use_arm & opt_arm_pose (optimize_sequence.py:264-268, 279-284)
        self.coarse_span = self.arena.span("pose", "wrist_pose" if (self.use_arm and self.opt_arm_pose) else "shape")
        self.app_span = self.arena.span("light_positions", "normal_map")
        self.opt_span = (self.coarse_span[0], self.app_span[0] + self.app_span[1] - self.coarse_span[0])
        with torch.no_grad():                                                         # init_params (optimize_sequence.py:181-250)
            for k in ("pose", "rot", "trans", "cam"):
                self.params[k].copy_(input_params[k].to(self.dev))
            self.params["shape"].copy_(input_params["shape"].mean(0).to(self.dev))
            self.params["texture"].copy_((torch.tensor([232, 190, 172]).repeat(1, tex_size, tex_size, 1) / 255.).to(self.dev))
            self.params["normal_map"].copy_(torch.tensor([0.0, 0.0, 1.0]).repeat(1, tex_size, tex_size, 1).to(self.dev))
            self.params["light_positions"].copy_(torch.tensor(((-0.5, -0.5, -0.5),)).repeat(T, 1).to(self.dev))
            self.params["amb_ratio"].fill_(0.4)
        self.uv_mask = torch.as_tensor(np.asarray(uv_mask), dtype=torch.float32).to(self.dev).contiguous() if uv_mask is not None else None
        self.init_joints = input_params["joints"].to(self.dev).float().contiguous() if "joints" in input_params else None
        # ---- frame tables struct
        t = _lib.FrameTables()
        for k in ("pose", "rot", "trans", "cam", "shape", "light_positions", "amb_ratio"):
            setattr(t, k, _lib.ptr(self.params[k]))
            setattr(t, "g_" + k, _lib.ptr(self.grads[k]))
        t.share_light = int(self.share_light)
        if self.use_arm:
            t.wrist_pose, t.g_wrist_pose = _lib.ptr(self.params["wrist_pose"]), _lib.ptr(self.grads["wrist_pose"])
        t.n_betas_out = self.n_betas
        self.tables = t
        # ---- Adam hyper-parameters on the device (coarse lr 1e-3, appearance lr 1e-2; torch defaults otherwise)
        self.hyper_np = np.zeros(2, dtype=[("lr", "f4"), ("beta1", "f4"), ("beta2", "f4"), ("eps", "f4"), ("grad_scale", "f4"),
                                           ("step", "i4"), ("step_size", "f4"), ("inv_sqrt_bc2", "f4")])
        self.hyper_np["lr"] = [1e-3, 1e-2]
        self.hyper_np["beta1"], self.hyper_np["beta2"], self.hyper_np["eps"] = 0.9, 0.999, 1e-8
        self.hyper_np["grad_scale"] = 1.0 / world_size
        self.hyper = torch.from_numpy(self.hyper_np.view(np.uint8).copy()).to(self.dev)
        self._hyper_stride = self.hyper_np.dtype.itemsize
        # ---- targets (set by set_targets) and per-step scratch
        self.y_true = self.y_sil = self.y_sil_col = None
        self.bg_sil = self.bg_photo = None
        self.target_offset = 0
        self.w_vec = torch.zeros(16, dtype=torch.float32, device=self.dev)
        # accumulate_loss: loss_total += sum_k w_k loss_k after every step — the reference's per-step `sum_loss` added up over an epoch
        # (optimize_sequence.py:553-559, :581) — by hand_back itself in a folded step, by two small torch kernels otherwise
        self.accumulate_loss = False
        self.loss_total = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.w_total = torch.zeros(16, dtype=torch.float32, device=self.dev)
        self.loss_acc = torch.zeros(16, dtype=torch.float32, device=self.dev)      # fold_step: the terms accumulate here, hand_back moves them to loss_vec and clears
        self.dist_albedo = torch.zeros(tex_size, tex_size, 2, dtype=torch.int32, device=self.dev)
        self.dist_normal = torch.zeros(tex_size, tex_size, 2, dtype=torch.int32, device=self.dev)
        self.seed = int(seed) & 0x7FFFFFFF              # SAME seed on every rank
        self.draw_counter = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.ref_verts = None
        self._graphs = {}
        if self.use_arm:
            self._weights_T = self.dm.weights.t().contiguous()                       # (NJ, NV): one coalesced row per joint for the per-frame kernels
        self._consume_gzl = self._keep_depth = None
        for sw in SWITCHES:
            setattr(self, sw.name, sw.default(self) if callable(sw.default) else sw.default)
        self._shadow_state_stale = False                 # (set by a FLIP of consume_gzl / keep_depth, not by their first values)
        self.comm = None                                 # harp_amd.dist.RcclComm: direct RCCL all-reduce on the step's stream (graph node by default), set_comm()
        self._trec = self._tacc = self._maps_pending = None
        self._lean_now = False                           # (the running step's _StepPlan.lean, for the struct builders)
        self.frozen = ()                                 # parameters kept out of the optimiser groups (known_appearance)
        self.disabled_terms = frozenset()                # loss terms left out of the objective altogether (set_disabled_terms)
        self.schedule = self.tschedule = self._stage = self._early_work = self._early_from = None
        self._loss_cleared = False
        self._lr_set = (None, None)
        self.perceptual = None                           # optional VGG feature term of the appearance stage (set_perceptual)
        apply_env_switches(self, os.environ.get("HARP_ENG", ""))
        self.compute_reference_mesh()

    def _alloc_scratch(self):
        """the step's scratch for B frames: self.s (name -> tensor) and the three cleared segments of its gradient slab"""
        dev, V, S, B = self.dev, self.topo.V, self.S, self.B
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        L = _lib.lib()
        s = {}
        s["pose48"], s["betas"], s["trans_b"] = f(B, self.pose_stride), f(B, self.n_betas), f(B, 3)
        s["cam_R"], s["cam_T"], s["light_pos"], s["colors"] = f(B, 9), f(B, 3), f(B, 3), f(9)
        V0, NJo = self.topo.V0, self.n_joints
        s["lbs_ws"] = f(L.harp_lbs_tree_ws_floats(ctypes.byref(self.dm.struct), B) if self.use_arm else L.harp_lbs_mano_ws_floats(B))
        s["verts_mm"], s["joints_mm"], s["joints_m"] = f(B, V0, 3), f(B, NJo, 3), f(B, NJo, 3)
        s["chain_parts"] = f(L.harp_mesh_chain_wide_ws_floats(B, V))
        s["vs"], s["n1"], s["il1"], s["vd"], s["n2"], s["il2"] = f(B, V, 3), f(B, V, 3), f(B, V), f(B, V, 3), f(B, V, 3), f(B, V)
        s["ndc_c"], s["ndc_l"], s["centroid"], s["light_R"], s["light_T"] = f(B, V, 3), f(B, V, 3), f(B, 3), f(B, 9), f(B, 3)
        s["ws_c"] = ops.rasterize_workspace(B, self.topo.F, S, dev)
        s["ws_l"] = ops.rasterize_workspace(B, self.topo.F, S, dev)
        s["face_c"] = torch.empty(B, S, S, dtype=torch.int32, device=dev)
        s["face_l"] = torch.empty(B, S, S, dtype=torch.int32, device=dev)
        s["alpha"], s["zl"], s["rgb"] = f(B, S, S), f(B, S, S), f(B, S, S, 3)
        s["g_v9"] = torch.zeros(B, V, 9, dtype=torch.float32, device=dev)       # harp_shade_args.g_vert9: all-zero between steps (its unpack clears it)
        s["zl_tiles"] = torch.zeros(B * ((S + 15) // 16) ** 2, dtype=torch.uint8, device=dev)     # harp_shade_args.g_zl_tiles: all-zero between steps
        s["zl_state"] = torch.zeros(B * ((S + 63) // 64) ** 2, dtype=torch.int32, device=dev)     # harp_rasterize_fwd_keep: which super-tiles of zl are all -1
        s["nmap_n"] = self.nmap_n
        # gradients (zeroed every step in ONE memset: they are carved from one flat buffer, which ends in the normal-map gradient, the
        # gradient arena and the loss vector)
        gspec = [("g_alpha", (B, S, S)), ("g_rgb", (B, S, S, 3)), ("g_zl", (B, S, S)), ("g_vd", (B, V, 3)), ("g_joints_m", (B, NJo, 3)), ("g_n2", (B, V, 3)),
                 ("g_ndc_c", (B, V, 3)), ("g_ndc_l", (B, V, 3)), ("g_n1", (B, V, 3)), ("g_vs", (B, V, 3)), ("g_tmp", (B, V, 3)),
                 ("g_v0", (B, V0, 3)), ("g_joints_mm", (B, NJo, 3)), ("g_light_pos", (B, 3)), ("g_colors", (9,)),
                 ("g_light_R", (B, 9)), ("g_light_T", (B, 3)), ("g_cam_R", (B, 9)), ("g_cam_T", (B, 3)), ("g_centroid", (B, 3)),
                 ("g_pose48", (B, self.pose_stride)), ("g_betas", (B, self.n_betas)), ("g_trans_b", (B, 3)),
                 ("g_nmap_n", (self.Ht, self.Wt, 3)), ("g_buf", (self.arena.size,)), ("loss_vec", (16,))]
        garena = _Arena(gspec, dev)
        gs_buf = garena.alloc()
        for k, _ in gspec:
            s[k] = garena.view(gs_buf, k)
        # g_alpha and g_rgb (the first two segments, 4/5 of the slab) are fully overwritten by harp_image_l1: only the rest is zeroed
        # ... and of the rest, g_zl (B*S*S floats, 9/10 of it) is first touched by the shader backward: it is cleared on the second
        # stream, off the head of the step; the small remainder is cleared first thing on the main stream
        # ... and g_vd / g_joints_m, the two the key-point / mesh terms accumulate into, are a segment of their own: those terms run on a
        # third stream, which clears the segment itself instead of depending on the clear of another branch
        self.s = s
        self.gs_zero = gs_buf[garena.offsets["g_n2"][0]:]
        self.gs_mesh = gs_buf[garena.offsets["g_vd"][0]:garena.offsets["g_n2"][0]]
        self.gs_zero_late = s["g_zl"]

    # `consume_gzl` / `keep_depth` carry invariants ACROSS steps (g_zl is all-zero between steps because its consumer clears it; zl_state
    # says which super-tiles of the kept light depth map are all -1).  A step with the switch off breaks the invariant (g_zl stays dirty, the
    # plain rasteriser fills super-tiles the state calls empty), so a flip re-establishes it before the next step.
    def _shadow_switch(attr):
        def fset(self, v):
            if getattr(self, attr) not in (None, bool(v)):
                self._shadow_state_stale = True
            setattr(self, attr, bool(v))
        return property(lambda self: getattr(self, attr), fset)

    consume_gzl, keep_depth = _shadow_switch("_consume_gzl"), _shadow_switch("_keep_depth")

    def _reset_shadow_state(self):
        for k in ("g_zl", "zl_tiles", "zl_state"):
            self.s[k].zero_()
        self._shadow_state_stale = False

    def set_targets(self, y_true, y_sil, y_sil_col, frame_offset=0):
        """(Tl,S,S,3), (Tl,S,S), (Tl,S,S) fp32 for this rank's frames [frame_offset, frame_offset+Tl): kept resident in HBM
        (the reference re-reads them from 20 DataLoader workers + H2D every step, optimize_sequence.py:446-450)."""
        self.y_true = y_true.to(self.dev).float().contiguous()
        self.y_sil = y_sil.to(self.dev).float().contiguous()
        self.y_sil_col = y_sil_col.to(self.dev).float().contiguous()
        self.target_offset = int(frame_offset)
        self._graphs = {}                               # captured graphs hold the raw pointers of the previous target buffers
        # the targets are static during a fit: what an un-rendered 64x64 super-tile contributes to the two image terms is a constant per
        # (target frame, super-tile) — sum of y_sil for the silhouette L1 (alpha = 0), sum of |bg - y| * mask for the photometric L1 —
        # tabulated once here; the loss-only kernels (keep_image = False) look it up instead of reading 3/4 of the targets every step
        T, S, nsx = self.y_sil.shape[0], self.S, (self.S + 63) // 64
        pad = nsx * 64 - S
        def tile_sums(img):                                                          # (T,S,S) -> (T, nsx*nsx), super-tile st = sy * nsx + sx
            x = torch.nn.functional.pad(img.double(), (0, pad, 0, pad))
            return x.reshape(T, nsx, 64, nsx, 64).sum((2, 4)).reshape(T, nsx * nsx).float().contiguous()
        self.bg_sil = tile_sums(self.y_sil)
        bg = torch.tensor(BG_COLOR, dtype=torch.float32, device=self.dev)
        m = self.y_sil_col.unsqueeze(-1)
        self.bg_photo = tile_sums((bg * m - self.y_true * m).abs().sum(-1))
        if self.perceptual is not None:                                              # cached target features belong to the old targets
            self.set_perceptual(self._vgg_module, self.perceptual_weight, cache_bytes=self._vgg_cache_bytes, precision=self._vgg_precision,
                                bounded=self._vgg_bounded)

    def _ck(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with status {rc}")

    def _chain_struct(self, B, shadow, has_normal_grad):
        """harp_mesh_chain over the step's scratch (fused per-frame mesh chain, csrc/chain.hip)"""
        s, p, tp = self.s, _lib.ptr, self.topo
        c = _lib.MeshChain()
        for k, t in (("edges0", tp.edges0), ("vf_off", tp.vf_off), ("vf_tri", tp.vf_tri), ("sub_off", tp.sub_off),
                     ("sub_idx", tp.sub_idx), ("disp", self.params["verts_disps"]), ("verts_mm", s["verts_mm"]), ("joints_mm", s["joints_mm"]),
                     ("cam_R", s["cam_R"]), ("cam_T", s["cam_T"]), ("light_pos", s["light_pos"]), ("joints_m", s["joints_m"]), ("vs", s["vs"]),
                     ("n1", s["n1"]), ("il1", s["il1"]), ("vd", s["vd"]), ("n2", s["n2"]), ("il2", s["il2"]), ("ndc_c", s["ndc_c"]),
                     ("centroid", s["centroid"]), ("light_R", s["light_R"]), ("light_T", s["light_T"]), ("ndc_l", s["ndc_l"]),
                     ("g_ndc_c", s["g_ndc_c"]), ("g_ndc_l", s["g_ndc_l"]), ("g_n2", s["g_n2"]), ("g_joints_m", s["g_joints_m"]), ("g_vd", s["g_vd"]),
                     ("g_light_R", s["g_light_R"]), ("g_light_T", s["g_light_T"]), ("g_v0", s["g_v0"]), ("g_joints_mm", s["g_joints_mm"]),
                     ("g_light_pos", s["g_light_pos"]), ("g_cam_T", s["g_cam_T"]), ("g_disp", self.grads["verts_disps"])):
            setattr(c, k, p(t))
        c.B, c.V0, c.E0, c.NJ, c.S = B, tp.V0, tp.E0, self.n_joints, self.S
        c.focal, c.shadow, c.has_normal_grad = self.focal, int(shadow), int(has_normal_grad)
        c.light_only = int(self._lean_now)
        return c

    def _frame_struct(self, fid, B, shadow, has_normal_grad, step=None):
        """harp_hand_front / harp_arm_front over the step's scratch: the fused front (csrc/hand_front.hip, csrc/arm_front.hip) and the
        three-launch back (csrc/hand_back.hip)"""
        s, p, arm = self.s, _lib.ptr, self.use_arm
        h = _lib.ArmFront() if arm else _lib.HandFront()
        if step is not None:
            h.step = step
        h.chain, h.tables = self._chain_struct(B, shadow, has_normal_grad), self.tables
        setattr(h, "tree" if arm else "mano", self.dm.struct)
        for k, t in (("fid", fid), ("pose_in" if arm else "pose48", s["pose48"]), ("betas", s["betas"]), ("trans_b", s["trans_b"]),
                     ("cam_R", s["cam_R"]), ("cam_T", s["cam_T"]), ("light_pos", s["light_pos"]), ("colors", s["colors"]), ("lbs_ws", s["lbs_ws"])):
            setattr(h, k, p(t))
        if arm:
            h.weights_T = p(self._weights_T)
        h.self_shadow = int(self.self_shadow)
        return h

    _hand_struct = _arm_struct = _frame_struct          # (the engine's model decides which struct it is)

    def _front_form(self, stage):
        """launch form of the fused front: "one" / "hybrid" / "wide"; None: the building blocks"""
        if not (self.fused_front and self.fused_chain):
            return None
        wide, hybrid = self.wide_front, self.hybrid_front
        if self.front_auto and not self.use_arm and stage is not None:
            # hand path, by stage (profiles/r05_wide_ab.txt item 19, fresh processes): a single-stage step (geometry only / appearance
            # only) has no long second-stream chain in front of the rasterisers, its head is on the critical path -> wide front
            # (-15 ... -25 us); the combined stage -> hybrid (hand layer wide, mesh chain one workgroup per frame: -5 us; wide: +6)
            both = bool(stage[0] and stage[1])
            wide, hybrid = (not both), both
        return "wide" if wide else ("hybrid" if hybrid and not self.use_arm else "one")

    def _mesh_forward(self, fid, B, shadow=False, front=False, step=None, stage=None):
        """frame_setup .. normals (and, fused, both projections + the light camera): fills the scratch geometry for the B frames in
        `fid` (int32 device tensor).  Returns True when the fused chain ran (projections / light camera already done).  front=True
        allows the fused front (csrc/hand_front.hip, csrc/arm_front.hip) in the form _front_form chooses; the step passes its plan's form."""
        L, s, p, st, tp = _lib.lib(), self.s, _lib.ptr, _lib.stream(), self.topo
        form = front if isinstance(front, str) else (self._front_form(stage) if front else None)
        if form is not None:
            name = "harp_%s_%s" % ("arm" if self.use_arm else "hand", _FRONT[form])
            h = ctypes.byref(self._frame_struct(fid, B, shadow, False, step))
            self._ck(getattr(L, name)(h, p(s["chain_parts"]), st) if form == "wide" else getattr(L, name)(h, st), name[5:])
            return True
        if step is not None:
            raise RuntimeError("a folded step needs the one-launch front (fused_front)")
        self._ck(L.harp_frame_setup_fwd(ctypes.byref(self.tables), p(fid), B, self.S, self.focal, int(self.self_shadow), p(s["pose48"]),
                                        p(s["betas"]), p(s["trans_b"]), p(s["cam_R"]), p(s["cam_T"]), p(s["light_pos"]), p(s["colors"]), st),
                 "frame_setup_fwd")
        lbs_fwd = L.harp_lbs_tree_fwd if self.use_arm else L.harp_lbs_mano_fwd
        self._ck(lbs_fwd(ctypes.byref(self.dm.struct), p(s["pose48"]), p(s["betas"]), p(s["trans_b"]), B, p(s["lbs_ws"]),
                         p(s["verts_mm"]), p(s["joints_mm"]), st), "lbs_fwd")
        if self.fused_chain:
            self._ck(L.harp_mesh_chain_fwd(ctypes.byref(self._chain_struct(B, shadow, False)), st), "mesh_chain_fwd")
            return True
        self._ck(L.harp_scale(p(s["joints_mm"]), 1e-3, B * self.n_joints * 3, p(s["joints_m"]), st), "scale")          # visualize.py:46
        self._ck(L.harp_subdivide_fwd(p(s["verts_mm"]), p(tp.edges0), B, tp.V0, tp.E0, 1e-3, p(s["vs"]), st), "subdivide_fwd")
        self._ck(L.harp_vertex_normals_fwd(p(s["vs"]), p(tp.faces), p(tp.vf_off), p(tp.vf_idx), B, tp.V, p(s["n1"]), p(s["il1"]),
                                           p(self.params["verts_disps"]), p(s["vd"]), st), "normals_displace_fwd")
        self._ck(L.harp_vertex_normals_fwd(p(s["vd"]), p(tp.faces), p(tp.vf_off), p(tp.vf_idx), B, tp.V, p(s["n2"]), p(s["il2"]),
                                           None, None, st), "normals_fwd")
        return False

    @torch.no_grad()
    def compute_reference_mesh(self):
        """ARAP reference = frame-0 mesh under the initial parameters (optimize_sequence.py:429-435)."""
        fid0 = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._mesh_forward(fid0, 1)
        if self.ref_verts is None:
            self.ref_verts = self.s["vd"][0].clone()
        else:
            self.ref_verts.copy_(self.s["vd"][0])       # same buffer: graphs captured against it stay valid

    def _shade_struct(self, B, app):
        s, tp = self.s, self.topo
        a = ops._shade_args(s["face_c"], s["ws_c"], tp, s["vd"][:B], s["n2"][:B], self.params["texture"][0], s["nmap_n"], s["light_pos"],
                            s["colors"], s["zl"] if self.self_shadow else None, s["light_R"] if self.self_shadow else None,
                            s["light_T"] if self.self_shadow else None, self.S, self.focal, (self.S / 2.0, self.S / 2.0), BG_COLOR)
        a.B = B
        # the fused photometric L1 needs no materialised image: with keep_image = False (fitting loops) the 4 MB / frame write is skipped
        a.rgb = _lib.ptr(s["rgb"]) if (self.keep_image or self.perceptual is not None) else None
        a.l1_bg_sums = _lib.ptr(self.bg_photo) if self.bg_photo is not None else None
        if self.packed_texels:
            a.texnm = _lib.ptr(self.texnm)
        for k, t in (("g_rgb", s["g_rgb"]), ("g_tex", self.grads["texture"]), ("g_nmap", s["g_nmap_n"]), ("g_verts", s["g_vd"]),
                     ("g_vnormals", s["g_n2"]), ("g_ndc", s["g_ndc_c"]), ("g_zl", s["g_zl"] if self.self_shadow else None),
                     ("g_light_pos", s["g_light_pos"]), ("g_colors", s["g_colors"]),
                     ("g_light_R", s["g_light_R"] if self.self_shadow else None), ("g_light_T", s["g_light_T"] if self.self_shadow else None)):
            setattr(a, k, _lib.ptr(t))
        if self.vert9:
            a.g_vert9 = _lib.ptr(s["g_v9"])
        if self._lean_now:                               # appearance-only stage: no geometry gradients out of the shader backward
            a.g_verts = a.g_vnormals = a.g_ndc = a.g_vert9 = None
        # maps kept out of the optimiser (known_appearance, optimize_sequence.py:264-289): their gradients are not formed at all
        if "texture" in self.frozen:
            a.g_tex = None
        if "normal_map" in self.frozen:
            a.g_nmap = None
        # light-view tiles that receive a shadow-tap gradient are flagged for the depth backward (which clears what it consumes)
        a.g_zl_tiles = _lib.ptr(s["zl_tiles"]) if (self.self_shadow and self.consume_gzl and self.zl_tile_flags) else None
        if self._records_on():
            rec, cnt, cap = self._texel_record_buffers()
            a.trec, a.trec_cnt, a.trec_cap = _lib.ptr(rec), _lib.ptr(cnt), cap
            a.trec_acc_tex, a.trec_acc_nmap = _lib.ptr(self._tacc[0]), _lib.ptr(self._tacc[1])
        return a

    def _records_on(self):
        return bool(self.texel_records and not ("texture" in self.frozen and "normal_map" in self.frozen))

    def _texel_record_buffers(self):
        if self._trec is None:
            nb = _lib.lib().harp_texel_bins(self.Ht, self.Wt)
            cap = ops.texel_record_capacity(self.B * self.S * self.S, self.trec_cap_div, self.trec_cap_min)
            self._trec = (torch.empty(nb * 9 * cap, dtype=torch.float32, device=self.dev),
                          torch.zeros(nb * 16 + 16, dtype=torch.int32, device=self.dev), cap)
        if self._tacc is None:                           # double accumulators of the two maps: all-zero between steps (harp_texel_finish clears what it consumes)
            self._tacc = torch.zeros(2, self.Ht * self.Wt * 3, dtype=torch.float64, device=self.dev)
        return self._trec

    def _join_maps(self):
        """the texel reduce (+ normal-map chain rule) runs on a branch of its own behind the shader backward: whoever reads the map
        gradients next (all-reduce, Adam) joins it first"""
        st, self._maps_pending = self._maps_pending, None
        if st is not None:
            torch.cuda.current_stream().wait_stream(st)

    def _can_fold(self):
        """the step's book-keeping rides in hand_front / hand_back / harp_step_prologue (`fold_step`) when those launches exist"""
        return bool(self.fold_step and self.fused_front and self.fused_chain and self.fused_back and self.overlap and self.early_terms
                    and self.schedule is not None)

    def forward_backward(self, coarse=True, app=True, B=None, tick=False, sched=False, *, _defer_maps_join=False):
        """Enqueue forward + losses + backward for the first B (default: batch_size) frames of self.fid / self.tfid; gradients land
        in self.g_buf, loss terms in loss_vec[:9] (unweighted, order LOSS_NAMES).
        On return every gradient is final on the current stream: the branch of the map gradients (texel reduce -> finish on the second
        stream) is joined before this returns.  _defer_maps_join=True (step() only) leaves that branch open for adam() to join behind
        the maps' own update (`split_adam`)."""
        self._join_maps()                                # (no-op unless a deferred branch is still open: it writes the record buffers / _tacc this step reuses)
        self._fb(coarse, app, B, tick, sched)
        if not _defer_maps_join:
            self._join_maps()

    def _plan(self, coarse, app, B, tick, sched):
        """The derived decisions of one step as a _StepPlan.  Host logic only, nothing is launched: it reads the switches, the arguments
        and the engine's state that steers a step (`_loss_cleared`, `bg_photo`, `frozen`, `perceptual`, `self_shadow`).
        sched: take the next row of the device schedule INSIDE this step's launches (step() passes it when _can_fold())."""
        fold, vgg, two = bool(sched), self.perceptual is not None, bool(self.overlap and self.early_terms)
        if fold and (B != self.B or not self._can_fold()):
            raise RuntimeError("forward_backward(sched=True) needs the full batch and _can_fold()")
        shadow = bool(app and self.self_shadow)
        lean = bool(self.lean_app_stage and app and not coarse and self.fused_chain and not vgg)
        fill_side = bool((fold or self._loss_cleared) and two)
        third = bool(self.mesh_third and two)
        # (of a node's dependants hipGraph keeps the FIRST-captured one on that node's stream, the others pay ~11 us of cross-stream wait)
        go = bool(self.graph_order and two and self.camera_first)
        fuse_bwd = bool(self.fused_bwd and coarse and app and not vgg)
        fsb = bool(self.fused_sil_bwd and coarse and not fuse_bwd)      # (its atomics into g_ndc_c need the slab clear in front of them)
        # fitting loop (no image kept, no perceptual term): the backward pass recomputes the colour anyway and forms the photometric L1 and its gradient itself
        # (harp_shade_bwd with g_rgb == NULL).  The one-launch backward pair instantiates the loss-only shader tile, which cannot write y_pred: a kept image is shaded forward there
        fused_loss = bool(app and self.fused_loss and (not self.keep_image or (self.fused_keep and not fuse_bwd)) and not vgg and self.bg_photo is not None)
        mesh_late = bool(not fsb and self.mesh_terms_late and two and coarse and app and not third and not vgg and not fuse_bwd)
        side_tail = bool(self.tail_side and self.overlap)
        records = bool(app and self._records_on() and not fuse_bwd)      # (the one-launch backward pair hosts the table form of the shader tile)
        nmap_in_depth = bool(app and self.fused_terms and self.self_shadow and self.consume_gzl and not side_tail and "normal_map" not in self.frozen and not records)
        v9 = bool(self.vert9 and not lean)
        riders = bool(v9 and self.self_shadow and self.consume_gzl)
        sil_where = None
        if coarse and not fuse_bwd and not fsb:
            # geometry-only stage: no shader backward to run next to — it stays on the critical stream (two cross-stream edges, ~6 us each, off the step); otherwise it
            # overlaps with shading on the second stream, captured right behind the shader backward (which then stays on the camera raster's stream) with `graph_order`
            sil_where = "main" if (not app and self.overlap) else ("late" if self.sil_late else "after") if (go and app) else "side"
        maps_where = depth_form = None
        if app:
            maps_where = ("records" if self.overlap else "records_main") if records else "depth" if nmap_in_depth else "side" if side_tail else "main"
        if shadow:
            depth_form = ("riders" if riders else "nmap" if nmap_in_depth else "tiles" if (self.consume_gzl and self.zl_tile_flags)
                          else "consume" if self.consume_gzl else "plain")
        prologue = bool(fold or (fill_side and self.fused_terms))
        draw = bool(app and self.auto_draw)
        front = self._front_form((coarse, app))
        return _StepPlan(
            lean=lean, fold=fold, shadow=shadow, one_stream=not self.overlap, fill_side=fill_side, mesh_on_third=third,
            capture_critical_first=go, fused_sil=fsb, fuse_bwd=fuse_bwd, fused_loss=fused_loss, mesh_late=mesh_late,
            sil_records=bool(self.sil_records and coarse and not self.fused_sil_bwd and not self.fused_bwd),
            paired=bool(self.paired_setup and shadow and self.fused_chain and self.camera_first), records=records,
            nmap_in_depth=nmap_in_depth, v9=v9, v9_riders=riders, sparse=0 if (self.keep_image or vgg) else 2,
            face_ids=bool(app or self.keep_image or not self.sil_only_raster), front_form=front,
            back_form=("wide" if self.wide_back else "one") if (front and self.fused_back) else ("chain" if self.fused_chain else "blocks"),
            prologue=prologue, draw=draw, tex_late=bool(self.late_texture_terms and two and shadow), sil_where=sil_where,
            maps_where=maps_where, depth_form=depth_form, camera_first=bool(self.camera_first),
            params_where="main" if not self.early_terms else ("side" if go else "side_first"),
            mesh_where=("main" if not self.early_terms else ("third" if go else "third_first") if third else "with_sil" if mesh_late
                        else "before_light" if self.mesh_terms_first else "after_light"),
            clear_mesh=None if fold else ("third" if third else "side" if fill_side else "main"),
            mark_zero=bool(fsb and fill_side), advance_draw=bool(draw and prologue and not fold), late_clear=not self.consume_gzl,
            join_side=bool(maps_where != "records" and (sil_where in ("late", "after", "side") or maps_where == "side")))

    def _step_context(self, pl, coarse, app, B, tick):
        """what the phases of one step share besides the plan: arguments, streams, events, the folded step's frame, loss / weight slots"""
        frame, loss = None, self.loss_vec
        if pl.fold:
            # hand_front fetches the schedule row, the terms accumulate into loss_acc (always clean between steps), hand_back moves them to
            # the loss vector, clears loss_acc and advances the schedule row and the draw counter
            frame = _lib.StepFrame()
            frame.schedule, frame.sched_row = _lib.ptr(self.schedule), _lib.ptr(self.schedule_row)
            frame.tschedule = _lib.ptr(self.tschedule) if self.tschedule is not None else None
            frame.n_rows, frame.target_offset = int(self.schedule.shape[0]), int(self.target_offset)
            frame.tfid_out, frame.clear_mesh_grads = _lib.ptr(self.tfid), 1
            frame.loss, frame.loss_out, frame.n_loss = _lib.ptr(self.loss_acc), _lib.ptr(self.loss_vec), 16
            if self.accumulate_loss:
                frame.loss_w, frame.loss_total = _lib.ptr(self.w_total), _lib.ptr(self.loss_total)
            if pl.draw:
                frame.draw_counter = _lib.ptr(self.draw_counter)
            loss = self.loss_acc
        return SimpleNamespace(coarse=coarse, app=app, B=B, tick=tick, frame=frame, loss=loss, st=_Streams(self, pl.one_stream), marks={},
                               wp=lambda i: self.w_vec.data_ptr() + 4 * i, lp=lambda i: loss.data_ptr() + 4 * i, fused=False, deferred=[],
                               pair_ev=None, pre=0, sil_after=None, ev_shade=None)

    def _fb(self, coarse, app, B, tick, sched):
        """The step, top to bottom.  Which launch, clear, fork and join exists, and where, is decided in _plan; the phases read the plan,
        and a single switch directly only where it selects the variant or an argument of one launch (keep_depth, keep_image, zl_tile_flags,
        fused_terms, packed_texels, frozen maps, disabled terms)."""
        if self._shadow_state_stale and not torch.cuda.is_current_stream_capturing():
            self._reset_shadow_state()
        B = self.B if B is None else int(B)
        pl = self._plan(coarse, app, B, tick, sched)
        c = self._step_context(pl, coarse, app, B, tick)
        self._lean_now, self._loss_cleared, st = pl.lean, False, c.st
        if not pl.fill_side:
            self.gs_zero.zero_()                         # one fill also covers g_buf, g_nmap_n and the loss vector
        if pl.clear_mesh == "main":
            self.gs_mesh.zero_()
        self._bind_sil_records(pl, B)
        # terms that depend on the parameters only go first on the second stream: under the LBS / mesh chain, a string of small latency-bound launches
        if pl.params_where == "side_first":
            st.wait(st.side)
            with torch.cuda.stream(st.side):
                self._param_terms(pl, c)
        ev0 = st.main.record_event() if pl.params_where == "side" else None
        c.fused = self._mesh_forward(self.fid, B, pl.shadow, pl.front_form, c.frame)
        if pl.params_where == "side":
            st.wait(st.side, ev0)
            with torch.cuda.stream(st.side):
                self._param_terms(pl, c)
        self._views(pl, c)
        st.wait(st.main, st.side)                        # join: light depth map, regulariser gradients, normalised normal map
        if pl.mesh_on_third:
            st.wait(st.main, st.extra("third"))
        if pl.sil_where in ("after", "late"):
            c.sil_after = st.main.record_event()
        elif pl.sil_where:
            self._silhouette_backward(pl, c, st.side if pl.sil_where == "side" else None)
        if pl.params_where == "main":
            self._param_terms(pl, c)
            self._mesh_terms(c)
        if app:
            self._shade(pl, c)
            self._map_gradients(pl, c)
            self._depth_backward(pl, c)
        if pl.maps_where == "records":
            # the texel reduce + normal-map chain rule follow the silhouette backward on the second stream (no further graph branch: a third one made the replay
            # run the silhouette backward BEHIND it); the mesh-chain backward then joins the silhouette backward's end only, and Adam (`_join_maps`) the stream
            if c.marks.get("sil") is not None:
                st.wait(st.main, c.marks["sil"])
            st.wait(st.side, c.ev_shade)
            with torch.cuda.stream(st.side):
                self._maps_branch(c)
            self._maps_pending = st.side
        elif pl.join_side:
            st.wait(st.main, st.side)                    # silhouette_bwd -> g_ndc_c (normal-map chain rule with tail_side)
        self._geometry_tail(pl, c)

    def _bind_sil_records(self, pl, B):
        """silhouette records are bound to the camera workspace: harp_rasterize_l1_fwd stores the pairs, harp_silhouette_bwd walks them"""
        L, s, p, S = _lib.lib(), self.s, _lib.ptr, self.S
        bind = (max(B, self.B), self.sil_rec_cap) if pl.sil_records else None
        if s.get("sil_rec_bound") == bind:
            return
        if bind is not None and ("sil_rec" not in s or s["sil_rec"].numel() < L.harp_sil_records_bytes(bind[0], S, bind[1])):
            # (a replaced buffer stays alive: graphs captured with it hold its address)
            s.setdefault("sil_rec_old", []).append(s.get("sil_rec"))
            s["sil_rec"] = torch.empty(L.harp_sil_records_bytes(bind[0], S, bind[1]), dtype=torch.uint8, device=self.dev)
        self._ck(L.harp_sil_records_bind(p(s["ws_c"]), p(s["sil_rec"]) if bind else None, bind[1] if bind else 0, bind[0] if bind else 0,
                                         self.topo.F, S), "sil_records_bind")
        s["sil_rec_bound"] = bind
        if bind is not None and "sil_rec_fin" not in s:
            # unbound when the workspace goes: a later workspace at the same address must not inherit the binding
            s["sil_rec_fin"] = weakref.finalize(s["ws_c"], L.harp_sil_records_bind, p(s["ws_c"]), None, 0, 0, 0, 0)

    def _param_terms(self, pl, c):
        """clears on the second stream, Adam tick, offset draw, normal-map normalisation, texture / displacement regularisers"""
        L, s, p, ST, coarse, app, wp, lp = _lib.lib(), self.s, _lib.ptr, _lib.stream, c.coarse, c.app, c.wp, c.lp
        if pl.prologue:
            # (the draw counter is advanced at the end of the step: by hand_back, or by harp_texture_terms, the launch that consumes the offsets)
            zero = self.gs_zero[:-64] if pl.fill_side else None
            hy, nh = self._hyper_block(coarse, app) if (c.tick and (coarse or app)) else (None, 0)
            self._ck(L.harp_step_prologue(p(zero), zero.numel() if pl.fill_side else 0, hy, nh, self.seed,
                                          p(self.draw_counter), self.Ht, self.Wt, 1.0, p(self.dist_albedo) if pl.draw else None, 2.0,
                                          p(self.dist_normal) if pl.draw else None, ST()), "step_prologue")
        elif pl.fill_side:
            self.gs_zero[:-64].zero_()                   # everything but the loss vector (the slab's last segment: 16 floats padded to the arena's 64-float granule — a clear that reached into the padding's front would wipe what the other streams have already added)
        if pl.clear_mesh == "side":
            self.gs_mesh.zero_()
        if c.tick and not pl.prologue:
            self._adam_tick(coarse, app)                 # only touches the hyper-parameter block: off the serial tail of the step
        if pl.late_clear:
            self.gs_zero_late.zero_()
        if pl.mark_zero:
            c.marks["zero"] = c.st.record(torch.cuda.current_stream())      # the slab clear ran on this (the second) stream
        disp_reg = coarse and "vert_disp_reg" not in self.disabled_terms
        if pl.draw and not pl.prologue:
            self.draw_texture_offsets()
        if app and self.fused_terms:
            self._ck(L.harp_normalize3_pack(p(self.params["texture"]), p(self.params["normal_map"]), self.Ht * self.Wt, p(s["nmap_n"]),
                                            p(self.texnm) if self.packed_texels else None, ST()), "normalize3_pack")
            # albedo + normal-map regularisers (+ the displacement regulariser) as one launch; frozen maps: loss values only
            tex_terms = lambda: self._ck(L.harp_texture_terms(
                p(self.params["texture"]), p(self.params["normal_map"]), p(self.uv_mask), p(self.dist_albedo), p(self.dist_normal), self.Ht, self.Wt,
                0.2, wp(7), lp(7), None if "texture" in self.frozen else p(self.grads["texture"]), wp(8), lp(8),
                None if "normal_map" in self.frozen else p(self.grads["normal_map"]), p(self.params["verts_disps"]) if disp_reg else None,
                self.topo.V, wp(2), lp(2), p(self.grads["verts_disps"]), p(self.draw_counter) if pl.advance_draw else None, ST()), "texture_terms")
            if pl.tex_late:
                c.deferred.append(tex_terms)             # runs behind the light view (_light_view)
            else:
                tex_terms()
            return
        if app:
            self._ck(L.harp_normalize3_fwd(p(self.params["normal_map"]), self.Ht * self.Wt, p(s["nmap_n"]), ST()), "normalize3")
            if self.packed_texels:
                self._ck(L.harp_pack_texels(p(self.params["texture"]), p(s["nmap_n"]), self.Ht * self.Wt, p(self.texnm), ST()), "pack_texels")
            self._texture_terms(wp, lp)
        if disp_reg:
            self._ck(L.harp_sum_squares(p(self.params["verts_disps"]), self.topo.V, wp(2), lp(2), p(self.grads["verts_disps"]), ST()), "disp_reg")

    def _mesh_terms(self, c):
        """key-point anchor + mesh regularisers (individually disabled regularisers carry weight 0)"""
        L, s, p, ST, tp, off, B, V, wp, lp = _lib.lib(), self.s, _lib.ptr, _lib.stream, self.topo, self.disabled_terms, c.B, self.topo.V, c.wp, c.lp
        kps_on, reg_on = c.coarse and "kps_anchor" not in off, c.coarse and not off.issuperset(("laplacian", "normal", "arap"))
        if kps_on and reg_on and self.fused_terms:
            self._ck(L.harp_mesh_kps_terms(p(s["vd"]), p(self.ref_verts), p(tp.nbr_off), p(tp.nbr_idx), p(tp.nc_pairs), p(tp.vp_off), p(tp.vp_idx), B, V,
                                           tp.nc_pairs.shape[0], tp.E, wp(3), lp(3), p(s["g_vd"]), p(self.init_joints), p(self.fid), p(s["joints_m"]),
                                           self.n_joints, wp(1), lp(1), p(s["g_joints_m"]), ST()), "mesh_kps_terms")
            return
        if kps_on:
            self._ck(L.harp_kps_loss(p(self.init_joints), p(self.fid), p(s["joints_m"]), B, self.n_joints, wp(1), lp(1), p(s["g_joints_m"]), ST()), "kps")
        if reg_on:
            self._ck(L.harp_mesh_regularizers(p(s["vd"]), p(self.ref_verts), p(tp.nbr_off), p(tp.nbr_idx), p(tp.nc_pairs), p(tp.vp_off), p(tp.vp_idx), B, V,
                                              tp.nc_pairs.shape[0], tp.E, wp(3), lp(3), p(s["g_vd"]), ST()), "mesh_reg")

    def _views(self, pl, c):
        """both rasterisations.  The light-view chain (centroid -> light camera -> projection -> K=1 raster) is independent of the camera-view chain: it runs on the
        second stream (fork / join is captured into the graph); the mesh regularisers and the key-point term go with it there (the light raster is the shorter of the two)"""
        s, p, tp, main = self.s, _lib.ptr, self.topo, c.st.main
        if not pl.camera_first:
            self._light_view(pl, c, None)
            self._camera_view(pl, c)
            return
        fork = main.record_event()                       # fork point = end of the mesh chain (the key-point / mesh terms need no more)
        if pl.paired:                                    # `paired_setup`: the set-up of BOTH views on the main stream, in front of the camera raster
            self._ck(_lib.lib().harp_raster_setup_pair(p(s["ndc_c"]), ops.SIL_BLUR, p(s["ws_c"]), p(s["ndc_l"]), 0.0, p(s["ws_l"]), p(tp.faces), c.B,
                                                       tp.V, tp.F, self.S, _lib.stream()), "raster_setup_pair")
            c.pre, c.pair_ev = 4, c.st.record(main)
        self._camera_view(pl, c)
        self._light_view(pl, c, fork)

    def _third_branch(self, pl, c, fork):
        third = c.st.extra("third")
        c.st.wait(third, fork)
        with torch.cuda.stream(third):
            if pl.clear_mesh == "third":                 # (a folded step: hand_front cleared its frames' slices)
                self.gs_mesh.zero_()
            self._mesh_terms(c)

    def _light_view(self, pl, c, fork):
        L, s, p, ST, tp, S, B, V, F = _lib.lib(), self.s, _lib.ptr, _lib.stream, self.topo, self.S, c.B, self.topo.V, self.topo.F
        c.st.wait(c.st.side, fork)
        if pl.mesh_where == "third_first":
            self._third_branch(pl, c, fork)
        with torch.cuda.stream(c.st.side):
            if pl.mesh_where == "before_light":
                self._mesh_terms(c)
            if pl.shadow:
                if not c.fused:
                    self._ck(L.harp_centroid(p(s["vd"]), B, V, p(s["centroid"]), ST()), "centroid")
                    self._ck(L.harp_light_setup_fwd(p(s["centroid"]), p(s["light_pos"]), B, p(s["light_R"]), p(s["light_T"]), ST()), "light_setup")
                    self._ck(L.harp_project_fwd(p(s["vd"]), p(s["light_R"]), p(s["light_T"]), B, V, self.focal, S / 2.0, S / 2.0, S, p(s["ndc_l"]), ST()),
                             "project_l")
                if c.pair_ev is not None:
                    c.st.wait(torch.cuda.current_stream(), c.pair_ev)      # both views' set-up ran on the main stream
                if self.keep_depth:      # the light depth map lives across steps: super-tiles that stay empty are not filled with -1 again
                    self._ck(L.harp_rasterize_fwd_keep(p(s["ndc_l"]), p(tp.faces), B, V, F, S, (0 if self.keep_image else 1) | c.pre, p(s["ws_l"]),
                                                       p(s["face_l"]), p(s["zl"]), p(s["zl_state"]), ST()), "raster_light")
                else:
                    self._ck(L.harp_rasterize_fwd(p(s["ndc_l"]), p(tp.faces), B, V, F, S, (0 if self.keep_image else 2) | c.pre, 0.0, 1.0, p(s["ws_l"]),
                                                  p(s["face_l"]), p(s["zl"]), None, ST()), "raster_light")
            if pl.mesh_where == "after_light":
                self._mesh_terms(c)
            for fn in c.deferred:
                fn()
            c.deferred.clear()
        if pl.mesh_where == "third":
            self._third_branch(pl, c, fork)

    def _camera_view(self, pl, c):
        """camera view: projection + fused K=1 / soft-silhouette raster; the silhouette L1 term and its gradient are fused into the raster
        epilogue (no separate pass over alpha)"""
        L, s, p, ST, tp, S, B, V, F, wp, lp = _lib.lib(), self.s, _lib.ptr, _lib.stream, self.topo, self.S, c.B, self.topo.V, self.topo.F, c.wp, c.lp
        if not c.fused:
            self._ck(L.harp_project_fwd(p(s["vd"]), p(s["cam_R"]), p(s["cam_T"]), B, V, self.focal, S / 2.0, S / 2.0, S, p(s["ndc_c"]), ST()), "project")
        # sparse: nothing reads face ids / alpha / g_alpha in super-tiles that hold no face (3/4 of the three images): they stay unwritten
        face_c = p(s["face_c"]) if pl.face_ids else None
        bg = p(self.bg_sil) if pl.sparse else None
        if pl.fused_sil:
            if c.marks.get("zero") is not None:
                c.st.wait(c.st.main, c.marks["zero"])
            self._ck(L.harp_rasterize_l1_fwd_bwd(p(s["ndc_c"]), p(tp.faces), B, V, F, S, 1 | pl.sparse | c.pre, ops.SIL_BLUR, ops.SIL_SIGMA, p(s["ws_c"]),
                                                 face_c, p(s["alpha"]), p(self.y_sil), p(self.tfid), wp(0), lp(0), p(s["g_alpha"]), bg,
                                                 p(s["g_ndc_c"]), ST()), "raster_cam_fwd_bwd")
            return
        self._ck(L.harp_rasterize_l1_fwd(p(s["ndc_c"]), p(tp.faces), B, V, F, S, 1 | pl.sparse | c.pre, ops.SIL_BLUR, ops.SIL_SIGMA, p(s["ws_c"]), face_c,
                                         None, p(s["alpha"]), p(self.y_sil) if c.coarse else None, p(self.tfid), wp(0), lp(0), p(s["g_alpha"]),
                                         bg, ST()), "raster_cam")

    def _silhouette_backward(self, pl, c, stream, ev=None):
        """The stand-alone silhouette backward, on the main stream (stream=None) or behind `ev` (default: the main stream's state) on the
        second one: it only needs g_alpha and the camera-view workspace, so it overlaps with shading there.  With `sil_records` the
        workspace has a record buffer bound: the launch walks the pairs the camera raster stored."""
        s, p, tp, st = self.s, _lib.ptr, self.topo, c.st
        if stream is not None:
            st.wait(stream, ev)
        with torch.cuda.stream(stream or st.main):
            self._ck(_lib.lib().harp_silhouette_bwd(p(tp.faces), c.B, tp.V, tp.F, self.S, ops.SIL_BLUR, ops.SIL_SIGMA, p(s["ws_c"]), p(s["alpha"]),
                                                    p(s["g_alpha"]), p(s["g_ndc_c"]), _lib.stream()), "silhouette_bwd")
            if stream is not None and pl.mesh_where == "with_sil":
                self._mesh_terms(c)      # `mesh_terms_late`: beside the (latency-bound) shader backward instead of beside the (VALU-bound) rasterisers
            if stream is not None:
                c.marks["sil"] = st.record(stream)

    def _shade(self, pl, c):
        """shade forward (unless the loss is fused into the backward) + perceptual term, then the shader backward"""
        L, s, p, ST = _lib.lib(), self.s, _lib.ptr, _lib.stream
        a = self._shade_struct(c.B, c.app)
        if pl.fuse_bwd:
            a.trec = None
        # the photometric L1 term and its gradient are fused into the shader (no separate pass over the image)
        a.l1_target, a.l1_mask, a.l1_fid = p(self.y_true), p(self.y_sil_col), p(self.tfid)
        a.l1_w, a.l1_loss, a.l1_grad = c.wp(6), c.lp(6), p(s["g_rgb"])
        if pl.fused_loss:
            a.g_rgb = None
        else:
            self._ck(L.harp_shade_fwd(ctypes.byref(a), ST()), "shade_fwd")
        if self.perceptual is not None:
            self._perceptual_term(c.B, self.tfid, c.loss)
        if pl.fuse_bwd:      # both backward passes of the camera view as ONE launch: as two kernels on two streams they cannot share a CU
            self._ck(L.harp_shade_sil_bwd(ctypes.byref(a), ops.SIL_BLUR, ops.SIL_SIGMA, p(s["alpha"]), p(s["g_alpha"]), ST()), "shade_sil_bwd")
        else:
            self._ck(L.harp_shade_bwd(ctypes.byref(a), ST()), "shade_bwd")
        if pl.sil_where == "late":                       # BEHIND the shader backward (next to the depth backward) instead of next to it
            c.sil_after = c.st.main.record_event()
        if c.sil_after is not None:
            self._silhouette_backward(pl, c, c.st.side, c.sil_after)

    def _maps_branch(self, c):
        """texel records -> exact sums -> gradient arena, the normal map's through the chain rule of its normalisation"""
        L, p, ST = _lib.lib(), _lib.ptr, _lib.stream
        rec, cnt, cap = self._texel_record_buffers()
        at = None if "texture" in self.frozen else p(self._tacc[0])
        an = None if "normal_map" in self.frozen else p(self._tacc[1])
        self._ck(L.harp_texel_reduce(p(rec), p(cnt), cap, self.Ht, self.Wt, at, an, c.B * self.S * self.S // 6, ST()), "texel_reduce")
        self._ck(L.harp_texel_finish(at, p(self.grads["texture"]), an, p(self.grads["normal_map"]), p(self.params["normal_map"]),
                                     self.Ht * self.Wt, ST()), "texel_finish")
        self._allreduce_maps_early()

    def _map_gradients(self, pl, c):
        """what only feeds the optimiser: records branch (captured BEHIND the depth backward, in _fb: the critical path keeps the shader's
        stream) | chain rule inside the depth backward (_depth_backward) | a tail of its own, with `tail_side` on the second stream, which
        is idle once the silhouette backward is done (the join in front of the mesh-chain backward already exists)"""
        st, p = c.st, _lib.ptr
        if pl.maps_where == "records":
            c.ev_shade = st.main.record_event()
        elif pl.maps_where == "records_main":
            self._maps_branch(c)
        elif pl.maps_where in ("side", "main"):
            # the normal map's chain rule as a launch of its own (and, for N > 1, the early all-reduce of the map gradients)
            on = st.side if pl.maps_where == "side" else st.main
            if on is st.side:
                st.wait(on)
            with torch.cuda.stream(on):
                if "normal_map" not in self.frozen:
                    self._ck(_lib.lib().harp_normalize3_bwd(p(self.params["normal_map"]), p(self.s["g_nmap_n"]), self.Ht * self.Wt,
                                                            p(self.grads["normal_map"]), _lib.stream()), "normalize3_bwd")
                self._allreduce_maps_early()

    def _depth_backward(self, pl, c):
        """shadow-map gradient -> light-view vertices (pl.depth_form), with its riders: the unpacking of the interleaved vertex gradients
        and (table form) the normal map's chain rule"""
        L, s, p, ST, tp, S, B, V, F, nm, form = _lib.lib(), self.s, _lib.ptr, _lib.stream, self.topo, self.S, c.B, self.topo.V, self.topo.F, pl.nmap_in_depth, pl.depth_form
        tiles = p(s["zl_tiles"]) if self.zl_tile_flags else None
        head = (p(s["face_l"]), p(s["ws_l"]), p(tp.faces), p(s["g_zl"]), B, V, F, S, p(s["g_ndc_l"]))
        nmap = (p(self.params["normal_map"]), p(s["g_nmap_n"]), self.Ht * self.Wt, p(self.grads["normal_map"])) if nm else (None, None, self.Ht * self.Wt, None)
        if form == "riders":
            self._ck(L.harp_depth_bwd_riders(*head, tiles, *nmap, p(s["g_v9"]), p(s["g_vd"]), p(s["g_n2"]), p(s["g_ndc_c"]), ST()), "depth_bwd_riders")
        elif form == "nmap":
            self._ck(L.harp_depth_nmap_bwd(*head, *nmap, tiles, ST()), "depth_nmap_bwd")
        if nm:
            self._allreduce_maps_early()
        if pl.v9 and form != "riders":
            self._ck(L.harp_vert9_unpack(p(s["g_v9"]), B * V, p(s["g_vd"]), p(s["g_n2"]), p(s["g_ndc_c"]), ST()), "vert9_unpack")
        if form == "tiles":
            self._ck(L.harp_depth_bwd_tiles(*head, tiles, ST()), "depth_bwd")
        elif form in ("consume", "plain"):
            self._ck((L.harp_depth_bwd_consume if form == "consume" else L.harp_depth_bwd)(*head, ST()), "depth_bwd")
        if form is not None and not c.fused:
            self._ck(L.harp_project_bwd(p(s["vd"]), p(s["light_R"]), p(s["light_T"]), p(s["g_ndc_l"]), B, V, self.focal, S, p(s["g_vd"]),
                                        p(s["g_light_R"]), p(s["g_light_T"]), ST()), "project_bwd_l")
            self._ck(L.harp_light_setup_bwd(p(s["centroid"]), p(s["light_pos"]), p(s["g_light_R"]), p(s["g_light_T"]), B, V, p(s["g_light_pos"]),
                                            p(s["g_centroid"]), p(s["g_vd"]), ST()), "light_setup_bwd")

    def _geometry_tail(self, pl, c):
        """mesh chain, hand / arm layer, scatter into the parameter tables' gradient rows: three launches fused, else the building blocks"""
        L, s, p, ST, tp, S, B, app, V = _lib.lib(), self.s, _lib.ptr, _lib.stream, self.topo, self.S, c.B, c.app, self.topo.V
        if pl.back_form in _BACK:
            name = "harp_%s_%s" % ("arm" if self.use_arm else "hand", _BACK[pl.back_form])
            args = [ctypes.byref(self._frame_struct(self.fid, B, pl.shadow, app, c.frame)), p(s["g_colors"]) if app else None]
            args += [p(s["g_pose48"]), p(s["g_betas"])] if self.use_arm else [p(s["g_betas"])]
            args += [p(s["chain_parts"])] if pl.back_form == "wide" else []
            self._ck(getattr(L, name)(*args, ST()), name[5:])
            return
        if pl.fold:
            raise RuntimeError("a folded step needs the fused backward tail (fused_back)")
        if pl.back_form == "chain":
            # projections, light camera, both vertex-normal passes, displacement, subdivision and the mm scaling: one launch
            self._ck(L.harp_mesh_chain_bwd(ctypes.byref(self._chain_struct(B, pl.shadow, app)), ST()), "mesh_chain_bwd")
        else:
            self._ck(L.harp_project_bwd(p(s["vd"]), p(s["cam_R"]), p(s["cam_T"]), p(s["g_ndc_c"]), B, V, self.focal, S, p(s["g_vd"]), None,
                                        p(s["g_cam_T"]), ST()), "project_bwd_c")
            if app:
                self._ck(L.harp_vertex_normals_bwd(p(s["vd"]), p(tp.faces), p(tp.vf_off), p(tp.vf_idx), B, V, p(s["n2"]), p(s["il2"]), p(s["g_n2"]),
                                                   p(s["g_tmp"]), p(s["g_vd"]), ST()), "normals_bwd2")
            self._ck(L.harp_displace_bwd(p(s["g_vd"]), p(s["n1"]), p(self.params["verts_disps"]), B, V, p(s["g_n1"]), p(self.grads["verts_disps"]), ST()),
                     "displace_bwd")
            self._ck(L.harp_vertex_normals_bwd(p(s["vs"]), p(tp.faces), p(tp.vf_off), p(tp.vf_idx), B, V, p(s["n1"]), p(s["il1"]), p(s["g_n1"]),
                                               p(s["g_tmp"]), p(s["g_vd"]), ST()), "normals_bwd1")        # g_vs aliases g_vd (vd = vs + n d)
            self._ck(L.harp_subdivide_bwd(p(s["g_vd"]), p(tp.sub_off), p(tp.sub_idx), B, tp.V0, V, 1e-3, p(s["g_v0"]), ST()), "subdivide_bwd")
            self._ck(L.harp_scale(p(s["g_joints_m"]), 1e-3, B * self.n_joints * 3, p(s["g_joints_mm"]), ST()), "scale_bwd")
        lbs_bwd = L.harp_lbs_tree_bwd if self.use_arm else L.harp_lbs_mano_bwd
        if not pl.lean:                                  # (lean: g_pose48 / g_betas / g_trans_b stay the zeros of the slab clear)
            self._ck(lbs_bwd(ctypes.byref(self.dm.struct), p(s["pose48"]), p(s["betas"]), p(s["trans_b"]), B, p(s["lbs_ws"]),
                             p(s["g_v0"]), p(s["g_joints_mm"]), p(s["g_pose48"]), p(s["g_betas"]), p(s["g_trans_b"]), ST()), "lbs_bwd")
        self._ck(L.harp_frame_setup_bwd(ctypes.byref(self.tables), p(self.fid), B, S, self.focal, int(self.self_shadow), p(s["g_pose48"]),
                                        p(s["g_betas"]), p(s["g_trans_b"]), p(s["g_cam_T"]), p(s["g_light_pos"]) if app else None,
                                        p(s["g_colors"]) if app else None, ST()), "frame_setup_bwd")

    # ---- optional perceptual term (optimize_sequence.py:405, 546-547) -------------------------------
    def set_perceptual(self, vgg, weight=1.0, cache_bytes=128 << 30, precision=0, bounded=True):
        """Add `weight * L1(vgg(y_pred * mask), vgg(y_true * mask))` to the appearance stage.  `vgg`: harp_amd.model.vgg.Vgg16Features
        (the filters; None removes the term).  The ten convolutions, their data gradients and everything between them run on the HIP
        kernels of csrc/conv.hip (harp_vgg16_term: 21 launches, captured into the step's hipGraph like every other launch).  precision:
        0 = float32 MFMA (a float32 fma chain, what the parity tests anchor on), 1 = three-term bf16 split with float32 accumulation
        (~16 mantissa bits per product), 2 = single-pass f16 with float32 accumulation (11-bit significands: the TF32 class the
        reference's own stack runs these convolutions in, at a third of mode 1's matrix-core work; include/harp_hip.h).
        The target frames' features do not change during a fit; what is kept in HBM depends on `cache_bytes`:
          * ALL 13 activation maps of every resident frame (300 floats per pixel, 307 MB per 512x512 frame — 256 frames are 79 GB of the
            288 GB) -> `bounded` mode: y_pred * mask and y_true * mask are identical outside the mask's support, so the stack runs only in
            the tiles (16 pixels a side, 8 at S/4 and S/8) the support reaches through the receptive field and reads the cached target activations next to them
            (same loss and gradient; csrc/conv.hip, model/vgg_hip.active_tiles);
          * else the four tap maps (126 MB per frame): one full forward + backward over the B rendered images per step;
          * else nothing: every step also recomputes the target features of its B frames."""
        from .model.vgg_hip import Vgg16Hip, activation_shapes, active_tiles, tap_shapes
        if vgg is not None and self.S % 8:               # (refused here, before any state changes: the kernels tile the image by 8)
            raise ValueError(f"perceptual term: image size {self.S} is not a multiple of 8")
        if int(precision) != precision or int(precision) not in (0, 1, 2):
            raise ValueError(f"perceptual term: precision must be 0, 1 or 2, got {precision!r}")
        # (the caller's arguments: set_targets re-invokes with them)
        self._vgg_module, self._vgg_cache_bytes, self._vgg_precision, self._vgg_bounded = vgg, int(cache_bytes), int(precision), bool(bounded)
        self.perceptual = None if vgg is None else Vgg16Hip(vgg, self.dev, precision)
        self.graph_perceptual, self.perceptual_weight = True, float(weight)
        self._vgg_cache = self._vgg_bound = self._vgg_step_feats = None
        self._graphs = {}
        if vgg is None or self.y_true is None:
            return
        T, S = self.y_true.shape[0], self.S
        full = 4 * sum(h * w * c for h, w, c in activation_shapes(S))
        taps = 4 * sum(h * w * c for h, w, c in tap_shapes(S))
        # the budget is the caller's figure, but never more than 80 % of what the device has free right now (a smaller device, or several
        # ranks sharing one: each would otherwise take the full default); a tier whose allocation fails anyway falls through to the next
        if self._records_on():
            self._texel_record_buffers()                 # (allocated before the cache is sized against what the device has free)
        torch.cuda.synchronize(self.dev)
        budget = min(int(cache_bytes), int(0.8 * torch.cuda.mem_get_info(self.dev)[0]))
        tiers = []
        if bounded and T * full <= budget:
            tiers.append((activation_shapes(S), True))
        if T * taps <= budget:
            tiers.append((tap_shapes(S), False))
        for shapes, all_slots in tiers:
            try:
                self._vgg_cache = [torch.empty((T,) + shp, device=self.dev) for shp in shapes]
            except torch.OutOfMemoryError:
                self._vgg_cache = None
                torch.cuda.empty_cache()
                continue
            if all_slots:
                self._vgg_bound = active_tiles(self.y_sil_col)
            break
        if self._vgg_cache is None:
            self._vgg_step_feats = [torch.empty((self.B,) + shp, device=self.dev) for shp in tap_shapes(S)]
            return
        for t0 in range(0, T, self.B):
            rows = torch.arange(t0, min(T, t0 + self.B), device=self.dev, dtype=torch.int32)
            self.perceptual.features(self.y_true, self.y_sil_col, rows, out=[c[t0:t0 + rows.shape[0]] for c in self._vgg_cache], all_slots=all_slots)

    def _perceptual_term(self, B, ltfid, lloss):
        """the term's value into slot 9 of the loss vector; its gradient joins the photometric gradient the shader backward consumes (that
        buffer is only defined at covered pixels — the fused L1 writes nothing elsewhere — hence the `covered` argument)"""
        s = self.s
        rows = ltfid[:B]
        if self._vgg_cache is not None:
            target, by_row = self._vgg_cache, 1
        else:
            target, by_row = [f[:B] for f in self._vgg_step_feats], 0
            self.perceptual.features(self.y_true, self.y_sil_col, rows, out=target)
        # (the batch in parts on as many streams: the term's 21 dependent launches fill each other's last rounds of workgroups)
        more = [self._extra_stream("vgg%d" % i) for i in range(min(self.vgg_streams, 4, B) - 1)] if (self.overlap and by_row) else []
        self.perceptual.term(s["rgb"][:B], self.y_true, self.y_sil_col, rows, target, by_row, s["g_rgb"][:B], lloss[9:10], weight=self.perceptual_weight,
                             covered=s["face_c"][:B], bound=self._vgg_bound, side_streams=more)

    def _extra_stream(self, name):
        if self._extra.get(name) is None:
            self._extra[name] = torch.cuda.Stream(device=self.dev)
        return self._extra[name]

    def _texture_terms(self, wp, lp):
        """albedo_reg + normal_reg (loss/texture_reg.py) with their gradients, straight into the gradient arena"""
        L, p, st = _lib.lib(), _lib.ptr, _lib.stream()
        self._ck(L.harp_texture_smooth_reg(p(self.params["texture"]), p(self.dist_albedo), p(self.uv_mask), self.Ht, self.Wt, wp(7), lp(7),
                                           p(self.grads["texture"]), st), "albedo_reg")
        self._ck(L.harp_close_to_z_reg(p(self.params["normal_map"]), self.Ht, self.Wt, 0.2, wp(8), lp(8), p(self.grads["normal_map"]), st), "close_z")
        self._ck(L.harp_texture_smooth_reg(p(self.params["normal_map"]), p(self.dist_normal), p(self.uv_mask), self.Ht, self.Wt, wp(8), lp(8),
                                           p(self.grads["normal_map"]), st), "normal_smooth")

    def _dist_on(self):
        return self.world > 1 or self.force_allreduce

    def set_comm(self, comm):
        """harp_amd.dist.RcclComm (or None): the gradient bucket is then reduced by `harp_allreduce_flat` on the step's own streams — a
        plain enqueue, captured into the step's hipGraph like every kernel — instead of through torch.distributed."""
        self.comm = comm
        self._graphs = {}
        if comm is not None:
            comm._engines.add(self)                      # RcclComm.destroy() un-sets itself here (captured graphs hold its raw handle)

    def _allreduce_maps_early(self):
        """The texture + normal-map gradients (6.29 of the 6.36 MB bucket) are final once the shading backward and normalize3_bwd
        are enqueued, ~0.25 ms before the mesh / LBS backward tail ends: their all-reduce is started there and overlaps with that
        tail; `allreduce()` then only has the small remainder [pose .. amb_ratio] left to send.  RcclComm: both collectives go to one
        communication stream (forked from / joined into the step's stream with events — all capturable), so the two operations on the
        communicator stay ordered.  torch.distributed: async_op on the process group's own stream."""
        if not self._dist_on() or not self.overlap_allreduce:
            return
        o = self.arena.offsets["texture"][0]
        e = self.arena.span("texture", "normal_map")
        if self.comm is not None:
            cur, cs = torch.cuda.current_stream(), self._extra_stream("comm")
            cs.wait_stream(cur)
            self.comm.allreduce(self.g_buf[o:o + e[1]], stream=cs.cuda_stream)
            self._early_from, self._early_work = o, "rccl"
            return
        if torch.cuda.is_current_stream_capturing():
            return
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        self._early_work = dist.all_reduce(self.g_buf[o:o + e[1]], async_op=True)
        self._early_from = o

    def allreduce(self):
        if not self._dist_on():
            return                                       # (the maps' branch stays open: adam() joins it — behind the maps' own update, `split_adam`)
        self._join_maps()
        from .dist import allreduce_flat
        o, n = self.opt_span
        work, self._early_work = self._early_work, None
        if self.comm is not None:
            if work is not None:
                cur, cs = torch.cuda.current_stream(), self._extra_stream("comm")
                cs.wait_stream(cur)                                 # the remainder is final only now (end of the backward tail)
                self.comm.allreduce(self.g_buf[o:self._early_from], stream=cs.cuda_stream)
                cur.wait_stream(cs)
            else:
                self.comm.allreduce(self.g_buf[o:o + n])            # one flat bucket (sum); 1/world is applied in the Adam kernel
            return
        if work is not None:
            allreduce_flat(self.g_buf[o:self._early_from])          # everything before the maps (they are the tail of the bucket)
            work.wait()                                             # current stream waits for the early collective
        else:
            allreduce_flat(self.g_buf[o:o + n])

    def _hyper_block(self, coarse, app):
        """(address, count) of the stage's Adam hyper-parameter struct(s): the two are adjacent, one launch takes both"""
        return self.hyper.data_ptr() + (0 if coarse else 1) * self._hyper_stride, 2 if (coarse and app) else 1

    def _adam_tick(self, coarse, app):
        """advance step / bias corrections of the stage's optimiser(s) — any time before `adam(..., tick=False)` of the same step"""
        if coarse or app:
            self._ck(_lib.lib().harp_adam_tick(*self._hyper_block(coarse, app), _lib.stream()), "adam_tick")

    def adam(self, coarse=True, app=True, tick=True):
        # the maps are 99.99 % of the optimised elements and their gradients are final on the second stream (texel reduce -> finish) well before
        # the backward tail ends: their Adam update runs THERE, and the launch that ends the step only carries the ~15 k other parameters
        # (8 -> 4 us at the very end of the critical path).  Single rank, nothing frozen, hyper-parameters already ticked by the prologue.
        maps, L, h1 = self._maps_pending, _lib.lib(), self.hyper.data_ptr() + self._hyper_stride
        bufs = (self.p_buf.data_ptr(), self.g_buf.data_ptr(), self.m_buf.data_ptr(), self.v_buf.data_ptr())
        if (self.split_adam and maps is not None and app and not tick and not self.frozen and not self._dist_on()):
            om, nm = self.arena.span("texture", "normal_map")
            with torch.cuda.stream(maps):
                self._ck(L.harp_adam_apply(*(b + 4 * om for b in bufs), nm, h1, _lib.stream()), "adam_apply(maps)")
            self._join_maps()
            osm, nsm = self.arena.span("light_positions", "amb_ratio")
            if coarse:
                (o0, n0) = self.coarse_span
                self._ck(L.harp_adam_apply2(*bufs, o0, n0, osm, nsm, self.hyper.data_ptr(), _lib.stream()), "adam_apply2(small)")
            else:
                self._ck(L.harp_adam_apply(*(b + 4 * osm for b in bufs), nsm, h1, _lib.stream()), "adam_apply(small)")
            return
        self._join_maps()
        st = _lib.stream()
        # parameters outside the reference's optimiser groups (known_appearance: shape / displacement / texture / normal map,
        # optimize_sequence.py:264-289) keep a zero gradient: with m = v = 0 the dense Adam update of such an element is exactly 0
        for k in self.frozen:
            self.grads[k].zero_()
        if tick:
            self._adam_tick(coarse, app)
        if coarse and app:                               # both groups in one launch
            (o0, n0), (o1, n1) = self.coarse_span, self.app_span
            self._ck(L.harp_adam_apply2(*bufs, o0, n0, o1, n1, self.hyper.data_ptr(), st), "adam_apply2")
        elif coarse or app:
            o, n = self.coarse_span if coarse else self.app_span
            self._ck(L.harp_adam_apply(*(b + 4 * o for b in bufs), n, self._hyper_block(coarse, app)[0], st), "adam_apply")

    def set_stage(self, coarse, app):
        w = torch.zeros(16)
        for i, k in enumerate(LOSS_NAMES):
            if ((coarse and k in COARSE_TERMS) or (app and k in APP_TERMS)) and k not in self.disabled_terms:
                w[i] = LOSS_WEIGHTS[k]
        self.w_vec.copy_(w.to(self.dev))
        # the weights of the step's sum_loss (optimize_sequence.py:553-559): the same, plus the perceptual term's in slot 9
        if app and self.perceptual is not None:
            w[9] = self.perceptual_weight
        self.w_total.copy_(w.to(self.dev))

    def set_disabled_terms(self, names):
        """Leave loss terms out of the objective: weight 0, kernels not launched, loss value reported as 0.  The reference fits a test
        sequence with a known appearance (`known_appearance`) WITHOUT the key-point anchor and the mesh regularisers
        (optimize_sequence.py:523, 531: kps_anchor, vert_disp_reg, laplacian, normal, arap)."""
        names = frozenset(names)
        unknown = names - set(LOSS_NAMES)
        if unknown:
            raise ValueError(f"unknown loss terms {sorted(unknown)}")
        self.disabled_terms = names
        self._stage = None                               # weights are re-uploaded by the next step()
        self._graphs = {}

    def set_lr(self, lr_coarse=None, lr_app=None):
        """host -> device hyper block (ReduceLROnPlateau lives on the host, optimize_sequence.py:309, 581-582)"""
        new = (None if lr_coarse is None else float(lr_coarse), None if lr_app is None else float(lr_app))
        last = self._lr_set
        if all(n is None or n == l for n, l in zip(new, last)):
            return                                       # unchanged since the last call (every epoch without a plateau): no D2H + H2D round trip
        h = self.hyper.cpu().numpy().view(self.hyper_np.dtype)
        for i, n in enumerate(new):
            if n is not None:
                h["lr"][i] = n
        self.hyper.copy_(torch.from_numpy(h.view(np.uint8)).to(self.dev))
        self._lr_set = tuple(n if n is not None else l for n, l in zip(new, last))

    def draw_texture_offsets(self):
        """the random neighbour offsets of albedo_reg (std 1) / smooth_texture_reg (std 2), loss/texture_reg.py:15, 51 — drawn on the
        device by a counter-based generator seeded identically on every rank (graph-replayable: the counter is device memory)."""
        L, p, st = _lib.lib(), _lib.ptr, _lib.stream()
        self._ck(L.harp_draw_texture_offsets(self.seed, p(self.draw_counter), self.Ht, self.Wt, 1.0, p(self.dist_albedo), 2.0, p(self.dist_normal), st),
                 "draw_offsets")

    def set_schedule(self, schedule, tschedule=None):
        """(n_rows, batch_size) global frame ids, kept on the device: `step(None, ...)` then takes the next row (wrapping around)
        inside the step's hipGraph, so a replay needs no host-side copy at all (the reference's DataLoader hands a host tensor over
        every step, optimize_sequence.py:399, :446).  tschedule: the rows of the resident targets these frames compare against, same
        shape (default fid - target_offset, i.e. targets stored in frame order) — for a dataset that holds a subset / another order of
        the frames.  A schedule of the SAME shape as the current one is written into the buffers the captured step graphs already read
        (a new epoch's shuffle costs two small copies, no re-capture); the row counter starts at 0 again."""
        sch = torch.as_tensor(schedule).to(torch.int32).to(self.dev).contiguous()
        if sch.dim() != 2 or sch.shape[1] != self.B:
            raise ValueError(f"schedule must be (n_rows, {self.B}), got {tuple(sch.shape)}")
        tsch = None
        if tschedule is not None:
            tsch = torch.as_tensor(tschedule).to(torch.int32).to(self.dev).contiguous()
            if tsch.shape != sch.shape:
                raise ValueError(f"tschedule must have the schedule's shape {tuple(sch.shape)}, got {tuple(tsch.shape)}")
        same = (self.schedule is not None and self.schedule.shape == sch.shape and (self.tschedule is None) == (tsch is None))
        if same:
            self.schedule.copy_(sch)
            if tsch is not None:
                self.tschedule.copy_(tsch)
            self.schedule_row.zero_()
            return
        self.schedule, self.tschedule = sch, tsch
        self.schedule_row = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._graphs = {}                               # graphs captured against an older schedule buffer are stale

    def _schedule_next(self):
        # the same launch clears the loss vector: with it gone from the slab clear, that one runs on the second stream (forward_backward)
        self._ck(_lib.lib().harp_schedule_next_rows(_lib.ptr(self.schedule), _lib.ptr(self.tschedule) if self.tschedule is not None else None,
                                                    int(self.schedule.shape[0]), self.B, self.target_offset, _lib.ptr(self.schedule_row),
                                                    _lib.ptr(self.fid), _lib.ptr(self.tfid), _lib.ptr(self.loss_vec), 16, _lib.stream()),
                 "schedule_next")
        self._loss_cleared = True

    def step(self, fid, coarse=True, app=True, use_graph=True, tfid=None):
        """One optimisation step on the frames `fid` (global frame ids = rows of the parameter tables, length <= batch_size; a shorter —
        last, partial — batch, optimize_sequence.py:396-399, replays a graph captured for its size).  fid=None: the next row of the schedule given to
        `set_schedule`.  tfid: rows of the resident targets these frames compare against (default fid - target_offset, i.e. targets
        stored in frame order); a dataset that holds a subset / another order of the frames passes its own item indices."""
        scheduled = fid is None
        if scheduled:
            if self.schedule is None:
                raise ValueError("step(None, ...) needs set_schedule() first")
            n = self.B
        else:
            fid = torch.as_tensor(fid)
            n = int(fid.shape[0])
            if n > self.B:
                raise ValueError(f"batch of {n} frames exceeds the engine's batch_size {self.B}")
            t = (fid - self.target_offset) if tfid is None else torch.as_tensor(tfid)
            if int(t.shape[0]) != n:
                raise ValueError("tfid must have one entry per frame of the batch")
            # (a device-resident batch costs no host sync at all)
            self.fid[:n].copy_(fid.to(torch.int32).to(self.dev), non_blocking=True)
            self.tfid[:n].copy_(t.to(torch.int32).to(self.dev), non_blocking=True)
        # a flipped consume_gzl / keep_depth left g_zl / zl_state in the other mode's state: a cached graph replays without passing through
        # forward_backward, so the invariant is re-established here, in front of the graph lookup
        if self._shadow_state_stale:
            self._reset_shadow_state()
        key = (coarse, app)
        if self._stage != key:
            self.set_stage(coarse, app)
            self._stage = key
        fold = scheduled and self._can_fold()
        fb0 = lambda: self.forward_backward(coarse, app, B=n, tick=True, sched=fold, _defer_maps_join=True)      # adam() joins the maps' branch
        fb = (lambda: (self._schedule_next(), fb0())) if (scheduled and not fold) else fb0
        dist_on = self._dist_on()
        graph_ok = (not dist_on) or self.comm is not None or self.graph_collectives
        # (a shorter — last, partial — batch of an epoch gets a graph of its own: the batch size is part of the key)
        if not use_graph or not graph_ok or (app and self.perceptual is not None and not self.graph_perceptual):
            fb()
            self.allreduce()
            self.adam(coarse, app, tick=False)
            if self.accumulate_loss and not fold:
                self.loss_total.add_(torch.dot(self.loss_vec, self.w_total))
            return
        # every switch is part of the key (the whole SWITCHES table: one that is added there is in the key), and so is the other state
        # the enqueued launch sequence depends on: flipping one re-captures instead of replaying a graph recorded for another configuration
        gkey = ((coarse, app, scheduled, n, fold) + tuple(getattr(self, name) for name in SWITCH_NAMES)
                + (self.self_shadow, tuple(self.frozen), self.accumulate_loss, dist_on, self.comm is not None, self.perceptual is not None and app))
        g = self._graphs.get(gkey)
        if g is None:
            # warm-up on a side stream, then capture (torch's documented recipe)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            row = self.schedule_row.clone() if scheduled else None
            hyper, draws, ltot = self.hyper.clone(), self.draw_counter.clone(), self.loss_total.clone()
            with torch.cuda.stream(side):
                fb()
                self.allreduce()                         # completes (and clears) the early all-reduce the warm-up pass started
                self._join_maps()                        # ... and the maps' branch: the capture must not start with a wait on it
            torch.cuda.current_stream().wait_stream(side)
            self.hyper.copy_(hyper)                      # the warm-up pass must not advance the optimiser's step count ...
            self.draw_counter.copy_(draws)               # ... nor the texture-offset generator (same draws as an eager run with this seed)
            self.loss_total.copy_(ltot)                  # ... nor count its losses into the epoch's sum (accumulate_loss)
            if scheduled:
                self.schedule_row.copy_(row)             # ... nor consume a schedule row
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # N > 1: other threads of the process (RCCL's proxy, torch's process-group watchdog) make HIP calls of their own while this
            # thread captures; only this thread's calls belong to the capture
            with torch.cuda.graph(g, capture_error_mode="thread_local" if dist_on else "global"):
                fb()
                self.allreduce()                         # no-op for a single rank; RCCL all-reduce is captured into the graph otherwise
                self.adam(coarse, app, tick=False)
            self._graphs[gkey] = g
            # the capture itself does not execute; fall through to the first replay
        g.replay()
        if self.accumulate_loss and not fold:
            self.loss_total.add_(torch.dot(self.loss_vec, self.w_total))

    def losses(self):
        """dict of the last step's unweighted loss terms (one D2H copy; call sparingly)."""
        v = self.loss_vec.cpu().tolist()
        out = {k: v[i] for i, k in enumerate(LOSS_NAMES)}
        if self.perceptual is not None:
            out["vgg"] = v[9]
        return out
