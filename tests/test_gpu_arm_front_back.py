"""-m gpu: the fused per-frame front and back of a fitting step, SMPL-X arm path, through the raw C ABI -- harp_arm_front_fwd / _wide_fwd,
harp_arm_back_bwd / _wide_bwd (csrc/arm_front.hip: arm_front_kernel, arm_mid_kernel, arm_skin_wide_kernel, arm_back_kernel,
arm_back_wide_kernel, arm_chain_bwd_kernel around the shared MFMA contractions) -- against the float64 composition tests/_front_ref.arm_front
(row gathers + tests/_tree_ref.tree_forward + mesh-chain reference, anchored by tests/test_front_ref_cpu.py).  The structure, the rules and
the shared helpers are those of tests/test_gpu_step_front_back.py (the MANO path); read its docstring for the two-part rule of the layer's
gradient rows, which is adopted here, not re-derived.

Models: the production arm (synth.make_smplx_arm_model: NJ = 55, NB = 20, NV = 1026, 4083 mesh vertices, center_joint = 21) and the two
synthetic trees of tests/_tree_ref.build_tree, the smallest that reach what production cannot: `twig` (NJ = 29 on one path of depth 16,
NB = 10, center_joint = -1, 6 vertices: a second kSkinBatch trip with one live row, a wide part without a vertex, two output joints on one
vertex, no shape padding; B = 17 opens a second 16-row MFMA tile) and `crown` (NJ = 64 = MAXJ, NB = 32 = MAXB, 64 output joints on 13
vertices: s_A / s_gGt at full size, the wide kernels' lanes 256..319 used to the last one).  T = 7 table rows, S = 100; batches
fid = [6], [2, 0, 1], [4, 4, 0, 6, 4] and, B = 17, (3 i + 1) mod 7.  Outputs are pre-filled with NaN, gradient rows with FILL = 2^-10.

Forward: gathered rows bit-equal to `_definition`; verts_mm / joints_mm within _skin_vertex_bound (production: as
test_tree_lbs_against_float64_at_rotation_edges calls it; a synthetic tree: theta and the joint count of its worst root-to-leaf path -- every
joint rotates, pose_mean is non-zero -- its own depth, and the blend factor 48 replaced by the longest add chain of tree_blend_mfma_kernel,
4 ceil(ceil(K / 4) / 4) + 4, where that is larger); the chain outputs through _check_forward_stages; wide against one-workgroup bit-equal;
the forward's rows of lbs_ws finite, g_vp / g_A still NaN, g_pm / g_Gt cleared.
Backward: every gradient row of every table (wrist_pose included) under the MANO file's rules; g_pose_scratch (B,51) and g_betas_scratch
(B,NB) per slot under rule (1); g_v0 (with the vertex joints' gradients folded in, as both backs leave it) and g_disp through _compare; the
lean form; the crossing stand-alone front -> fused back.  The vertex joints' share of g_v0 is also held without e_blocks: the same back with
g_joints_m = 0 leaves every other vertex bit-equal and a named vertex short of the sum of its joints' g_joints_mm, one rounding per joint
(_check_fold).  Book-keeping and refusals: known answers.
Where rule (2) falls back on 4 e_blocks (measured on the MI355X): table row 2 of the production arm (B = 3) with a normal gradient, in the
STAND-ALONE sequence as in both fused backs: g_pose 2.8e-4, g_wrist_pose 3.1e-4 of the row, g_shape 1.36e-4 (fused and blocks equal to three
digits; without the normal gradient, and on every other row, batch and model, both are below 5e-5).  It is the MANO file's conditioning: the
arm mesh has vertices whose |N| is 2.2e-6 m^2 (il up to 4.6e5); on the float64 reference alone, verts_mm rounded to float32 once, that row of
g_wrist_pose moves by 3.8e-6 of its norm, g_pose by 2.1e-6 and g_shape by 3.4e-6 (3.1e-8, 1.2e-7, 2.9e-7 without the normal gradient), and the
front's real error at 400 mm is some tens of that rounding.  Rule (1) holds on every row of every model: at most 0.36 of 1e-4.

measured on the MI355X, worst error as a fraction of its bound: see docs/NOTEBOOK.md, "B.22. The fused SMPL-X arm front and back against
float64 through the C ABI"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _front_ref as R
from tests import _tree_ref as TR
from tests import test_gpu_step_front_back as M
from tests.test_gpu_building_blocks import DEV, U, _L, _d, _keep_alive, _worst  # noqa: F401 (_keep_alive: autouse)
from tests.test_gpu_geometry_terms import _angle, _skin_vertex_bound
from tests.test_gpu_mesh_chain import (FOCAL, FWD_SHAPES, MM, S, SHADOW_ONLY, _assert_property, _bits, _case, _check_forward_stages, _compare, _Dev,
                                       _reference_grads)
from tests.test_gpu_step_front_back import CHAIN_BWD, CHAIN_FWD, CONFIGS, FILL, NAN_BITS, _Refusals, _check_rows, _check_tables, _cot

pytestmark = pytest.mark.gpu
T = 7
FIDS = {**M.FIDS, 17: [(3 * i + 1) % 7 for i in range(17)]}
GRADS = M.GRADS + ("wrist_pose",)
LAYER = ("pose", "rot", "wrist_pose", "trans", "shape")
MESH_OF = dict(arm="arm", twig="five", crown="hub")
CASES = [("arm", 1), ("arm", 3), ("arm", 5), ("twig", 1), ("twig", 3), ("twig", 17), ("crown", 1), ("crown", 3)]
FORMS = ("one", "wide")


@functools.lru_cache(maxsize=None)
def _host(name):
    """host model, float64 model, mesh tables and parameter tables of one model; cached, never modified"""
    from harp_amd import synth
    host = TR.host_from_arm(synth.make_smplx_arm_model(seed=0)) if name == "arm" else TR.build_tree(name)
    TR.assert_tree_property(host)
    cs = dict(_case(MESH_OF[name], 1))
    _assert_property(cs)
    lay = TR.device_layout(host)
    assert cs["V0"] == lay["NV"] and len(cs["comps"]) == 1
    cs["NJ"] = lay["n_joints_out"]
    return dict(name=name, host=host, m64=TR.model64(host), lay=lay, cs=cs, tb=R.arm_case_tables(host, T, **R.ARM_CASE[name]),
                edges0=torch.from_numpy(cs["edges0_np"]).long(), faces=torch.from_numpy(cs["faces_np"]).long())


@functools.lru_cache(maxsize=None)
def _device_tree(name):
    """the model on the device, filled into a _lib.TreeModel from tests/_tree_ref.device_layout; (struct, tensors)"""
    from harp_amd import _lib
    lay = _host(name)["lay"]
    t = {k: torch.from_numpy(v).to(DEV) for k, v in lay.items() if isinstance(v, np.ndarray)}
    s = _lib.TreeModel()
    for k, v in lay.items():
        if k != "weights_T":
            setattr(s, k, _lib.ptr(t[k]) if isinstance(v, np.ndarray) else int(v))
    return s, t


class _ArmRig:
    """every buffer a harp_arm_front of B frames points at, sized by the library's own *_ws_floats (tests/test_gpu_step_front_back._Rig for
    the arm path: the same attributes and methods, so that the shared test bodies run on either)"""

    def __init__(self, name, B, fid=None, extra_frames=0):
        L = _L()[0]
        H = self.H = _host(name)
        lay = H["lay"]
        self.B, self.NV, self.NJO, self.NB, self.V = B, lay["NV"], lay["n_joints_out"], lay["NB"], H["cs"]["V"]
        self.tree, self.tree_t = _device_tree(name)
        nan = lambda *s: torch.full(s, float("nan"))
        self.cs = dict(H["cs"], B=B, vertical=None, verts_mm=nan(B, self.NV, 3), joints_mm=nan(B, self.NJO, 3), cam_R=nan(B, 3, 3), cam_T=nan(B, 3),
                       light=nan(B, 3))
        self.d = _Dev(self.cs)
        t = self.d.t
        self.fid = _d(torch.tensor(FIDS[B] if fid is None else fid, dtype=torch.int32))
        self.tb = {k: _d(v) for k, v in H["tb"].items()}
        self.g_tb = {k: torch.full(H["tb"][k].shape, FILL, device=DEV) for k in GRADS}
        self.rows = {k: torch.full((B, n), float("nan"), device=DEV) for k, n in (("pose_in", 51), ("betas", self.NB), ("trans_b", 3))}
        for k in ("cam_R", "cam_T", "light_pos"):                       # chain.cam_R / cam_T / light_pos alias the gathered rows
            self.rows[k] = t[k]
        self.colors = torch.full((10,), float("nan"), device=DEV)
        self.lbs_ws = torch.full((L.harp_lbs_tree_ws_floats(ctypes.byref(self.tree), B),), float("nan"), device=DEV)
        self.part_ws = torch.full((L.harp_mesh_chain_wide_ws_floats(B, self.V),), float("nan"), device=DEV)
        self.g_pose = torch.full((B, 51), float("nan"), device=DEV)
        self.g_betas = torch.full((B, self.NB), float("nan"), device=DEV)
        t["g_vd"] = torch.full((B + extra_frames, self.V, 3), 7.0, device=DEV)
        t["g_joints_m"] = torch.full((B + extra_frames, self.NJO, 3), 7.0, device=DEV)

    def tables(self, share_light, grads=None, **over):
        from harp_amd import _lib
        ft = _lib.FrameTables(share_light=share_light, n_betas_out=self.NB)
        for k in GRADS:
            setattr(ft, k, _lib.ptr(self.tb[k]))
            setattr(ft, "g_" + k, _lib.ptr((self.g_tb if grads is None else grads)[k]))
        for k, v in over.items():
            setattr(ft, k, v)
        return ft

    def hand(self, share_light=0, self_shadow=1, shadow=1, ng=0, light_only=0, step=None, grads=None):
        from harp_amd import _lib
        p = _lib.ptr
        h = _lib.ArmFront()
        if step is not None:
            h.step = step
        h.chain, h.tree, h.tables = self.d.struct(shadow, ng, light_only), self.tree, self.tables(share_light, grads)
        h.fid, h.colors, h.lbs_ws, h.weights_T, h.self_shadow = p(self.fid), p(self.colors), p(self.lbs_ws), p(self.tree_t["weights_T"]), self_shadow
        for k in self.rows:
            setattr(h, k, p(self.rows[k]))
        return h

    def front(self, form, h):
        L, p, st, _ = _L()
        if form == "one":
            return L.harp_arm_front_fwd(ctypes.byref(h), st())
        return L.harp_arm_front_wide_fwd(ctypes.byref(h), p(self.part_ws), st())

    def back(self, wide, h, g_colors):
        L, p, st, _ = _L()
        if wide:
            return L.harp_arm_back_wide_bwd(ctypes.byref(h), p(g_colors), p(self.g_pose), p(self.g_betas), p(self.part_ws), st())
        return L.harp_arm_back_bwd(ctypes.byref(h), p(g_colors), p(self.g_pose), p(self.g_betas), st())

    def reset_outputs(self):
        for k in list(FWD_SHAPES) + ["verts_mm", "joints_mm"]:
            self.d.t[k].fill_(float("nan"))
        for v in self.rows.values():
            v.fill_(float("nan"))
        self.colors.fill_(float("nan"))
        self.lbs_ws.fill_(float("nan"))

    def run_front(self, form, tag="", **kw):
        self.reset_outputs()
        _L()[3](self.front(form, self.hand(**kw)), f"arm_front {form} {tag}")
        torch.cuda.synchronize()
        return {k: self.d.t[k].cpu() for k in list(FWD_SHAPES) + ["verts_mm", "joints_mm"]}, dict({k: v.cpu() for k, v in self.rows.items()},
                                                                                                 colors=self.colors.cpu())

    def fresh_grads(self):
        """own gradient outputs of a back: the shader's shares (+=) pre-filled by the caller's `pre`, g_v0 / g_joints_mm / scratch NaN, rows FILL"""
        for v in self.g_tb.values():
            v.fill_(FILL)
        self.g_pose.fill_(float("nan"))
        self.g_betas.fill_(float("nan"))


def _rig_of(name):
    return lambda B, fid=None, extra_frames=0: _ArmRig(name, B, fid, extra_frames)


def _arm_check_rows(H, tag, rows, fid, share_light, self_shadow):
    ref = R.arm_rows({k: v.double() for k, v in H["tb"].items()}, torch.tensor(fid), H["lay"]["NB"], share_light, self_shadow)
    return _check_rows(tag, rows, fid, share_light, self_shadow, ref=ref, exact=("pose_in", "betas", "trans_b", "light_pos"))


def _vertex_bound(H, rows, v_ref):
    """_skin_vertex_bound of the tree layer (B,1,1) [mm] for the float32 rows and the float64 vertices v_ref (module docstring)"""
    host, m64, lay = H["host"], H["m64"], H["lay"]
    B = rows["pose_in"].shape[0]
    src, par = host["pose_src"], host["parents"]
    NJ, NB = lay["NJ"], lay["NB"]
    pm = m64["pose_mean"]
    in_pose = rows["pose_in"].view(B, 17, 3).double()
    zero = torch.zeros(B, 3, dtype=torch.float64)
    th = torch.stack([_angle(pm[j][None] + (in_pose[:, src[j]] if src[j] >= 0 else zero)) for j in range(NJ)], 1)       # (B,NJ)
    vp = (m64["v_template"].abs()[None] + torch.einsum("vck,bk->bvc", m64["shapedirs"].abs(), rows["betas"].double().abs())
          + 2 * m64["posedirs"].abs().sum(0).view(-1, 3)[None]).amax((1, 2))[:, None]
    Rm = m64["J_template"].norm(dim=-1).max() + (v_ref / 1000 - rows["trans_b"].double()[:, None]).norm(dim=-1).amax(-1, keepdim=True)
    if H["name"] == "arm":
        # as test_tree_lbs_against_float64_at_rotation_edges: root + wrist + the worst finger, 11 levels, the 5 driven joints of a path rotate
        t17 = _angle(in_pose + pm[[src.index(r) for r in range(17)]])
        chain = t17[:, :2].sum(-1, keepdim=True) + t17[:, 2:].view(B, 5, 3).sum(-1).amax(-1, keepdim=True)
        return _skin_vertex_bound(2 * chain + 5 * 24, Rm, vp, 11).clamp(max=3e-3)[:, :, None]
    depth = TR.depth_of(par)
    path = torch.zeros(B, NJ, dtype=torch.float64)                       # 2 theta + 24 summed from the root down to each joint
    for j in range(NJ):
        path[:, j] = 2 * th[:, j] + 24 + (path[:, par[j]] if j > 0 else 0.0)
    K = (NJ - 1) * 9 + NB
    adds = 4 * (((K + 3) // 4 + 3) // 4) + 4                             # a wave's fmaf chain + the three wave sums + v_template
    return (_skin_vertex_bound(path.amax(1, keepdim=True), Rm, vp, max(depth) + 1) + 1000.0 * max(0, adds - 48) * U * vp)[:, :, None]


# ----------------------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,B", CASES)
def test_arm_front_forward_against_float64(name, B, form):
    H = _host(name)
    fid = FIDS[B]
    rig = _ArmRig(name, B)
    lay = H["lay"]
    NV, NJ, no = lay["NV"], lay["NJ"], lay["n_joints_out"]
    tag = f"arm_front {name} {form} B={B}"
    # ---- share_light = 0, self_shadow = 1, shadow = 1: everything
    out, rows = rig.run_front(form, tag, share_light=0, self_shadow=1, shadow=1)
    ref = _arm_check_rows(H, tag, rows, fid, 0, 1)
    assert len({tuple(r.tolist()) for r in rows["light_pos"]}) == len(set(fid)) and len({tuple(r.tolist()) for r in rows["cam_T"]}) == len(set(fid))
    v_ref, j_ref = TR.tree_forward(H["m64"], ref["pose_in"].view(B, 17, 3), ref["betas"], ref["trans_b"])
    bv = _vertex_bound(H, rows, v_ref)
    _worst(tag + " verts_mm", (out["verts_mm"].double() - v_ref).abs(), bv)
    _worst(tag + " joints_mm", (out["joints_mm"].double() - j_ref).abs(), bv)
    cs = dict(rig.cs, verts_mm=out["verts_mm"], joints_mm=out["joints_mm"], cam_R=rows["cam_R"].view(B, 3, 3), cam_T=rows["cam_T"])
    _check_forward_stages(tag, cs, out, rows["light_pos"], general_rotation=False)
    # ---- the workspace (csrc/lbs_tree_body.h: tree_ws): pose_map | A | G | Jrest | Rloc | v_posed written by the front; g_vp | g_A are the
    #      backward's and stay NaN; g_pm | g_Gt are cleared (joints_body: the backward accumulates into them)
    NP = (NJ - 1) * 9
    ws = rig.lbs_ws.cpu()
    head, mid, tail = B * (NP + NJ * 12 * 2 + NJ * 3 + NJ * 9 + NV * 3), B * (NV * 3 + NJ * 12), B * (NP + NJ * 3)
    assert ws.numel() == head + mid + tail, tag
    assert torch.isfinite(ws[:head]).all() and (_bits(ws[head:head + mid]) == NAN_BITS).all() and (_bits(ws[head + mid:]) == 0).all(), tag
    # ---- the wide form against the one-workgroup form: the same expressions, bit for bit
    if form == "wide":
        one = _ArmRig(name, B)
        out_one, rows_one = one.run_front("one", tag, share_light=0, self_shadow=1, shadow=1)
        for k in ("verts_mm", "joints_mm", "joints_m"):
            assert torch.equal(_bits(out[k]), _bits(out_one[k])), (tag, k)
        for k in rows:
            assert torch.equal(_bits(rows[k]), _bits(rows_one[k])), (tag, k)
        assert torch.equal(_bits(rig.lbs_ws[:head]), _bits(one.lbs_ws[:head])), tag
    # ---- share_light = 1, self_shadow = 0: the light of row 0 for every frame; the stages again where the batch has three frames
    out1, rows1 = rig.run_front(form, tag, share_light=1, self_shadow=0, shadow=1)
    _arm_check_rows(H, tag + " share", rows1, fid, 1, 0)
    assert torch.equal(rows1["light_pos"], H["tb"]["light_positions"][:1].repeat(B, 1)), tag
    for k in FWD_SHAPES:
        if k not in SHADOW_ONLY:
            assert torch.equal(_bits(out1[k]), _bits(out[k])), (tag, k)
    assert torch.equal(_bits(out1["verts_mm"]), _bits(out["verts_mm"])) and torch.isfinite(out1["ndc_l"]).all(), tag
    if B == 3:
        _check_forward_stages(tag + " share", cs, out1, rows1["light_pos"], general_rotation=False)
    # ---- shadow = 0 (share_light = 1, self_shadow = 1): the shadow-only outputs keep their NaN, the rest is the same
    out0, rows0 = rig.run_front(form, tag, share_light=1, self_shadow=1, shadow=0)
    _arm_check_rows(H, tag + " shadow=0", rows0, fid, 1, 1)
    for k in FWD_SHAPES:
        if k in SHADOW_ONLY:
            assert (_bits(out0[k]) == NAN_BITS).all(), (tag, k)
        else:
            assert torch.equal(_bits(out0[k]), _bits(out[k])), (tag, k)
    # ---- a zero-initialised step writes nothing: the frame ids and the two gradient segments are as they were
    assert torch.equal(rig.fid.cpu(), torch.tensor(fid, dtype=torch.int32)) and (rig.d.t["g_vd"] == 7).all() and (rig.d.t["g_joints_m"] == 7).all(), tag


# ----------------------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------------------
def _reference(rig, centroid, cot, pre, g_colors, share_light, self_shadow, shadow, ng):
    """float64 autograd of tests/_front_ref.arm_front at the float32 tables; pre g_cam_T / g_light_pos: cotangents of the cam_T / light_pos rows"""
    H = rig.H
    fid = torch.tensor(rig.fid.cpu().tolist())
    cot64 = {k: v.double() for k, v in cot.items()}

    def f(tb, disp):
        out = R.arm_front(tb, fid, disp, H["edges0"], H["faces"], H["m64"], share_light, self_shadow, mm=MM, centroid_value=centroid)
        t = R.total(out, cot64, g_colors.double() if g_colors is not None else None, shadow, ng) + (out["cam_T"] * pre["g_cam_T"].double()).sum()
        if g_colors is not None:                                       # (no appearance gradient: the light rows are not scattered)
            t = t + (out["light_pos"] * pre["g_light_pos"].double()).sum()
        return t
    return R.table_grads({k: v.double() for k, v in H["tb"].items()}, H["cs"]["disp"].double(), f)


def _own(rig, pre):
    own = {k: _d(v) for k, v in pre.items()}
    own["g_v0"] = torch.full((rig.B, rig.NV, 3), float("nan"), device=DEV)
    own["g_joints_mm"] = torch.full((rig.B, rig.NJO, 3), float("nan"), device=DEV)
    return own


def _blocks(rig, pre, g_colors_d, share_light, self_shadow, shadow, ng):
    """the pinned stand-alone sequence on the same forward outputs and the same workspace: harp_mesh_chain_bwd + harp_lbs_tree_bwd +
    harp_frame_setup_bwd, into gradient buffers of its own; (table rows, own outputs with g_v0 as harp_lbs_tree_bwd leaves it -- the vertex
    joints' gradients folded in -- and the layer's own g_pose / g_betas)"""
    L, p, st, ck = _L()
    B, r = rig.B, rig.rows
    own = _own(rig, pre)
    ch = rig.d.struct(shadow, ng, **{k: p(v) for k, v in own.items()})
    ck(L.harp_mesh_chain_bwd(ctypes.byref(ch), st()), "mesh_chain_bwd")
    gp, gb, gt = (torch.full(s, float("nan"), device=DEV) for s in ((B, 51), (B, rig.NB), (B, 3)))
    ck(L.harp_lbs_tree_bwd(ctypes.byref(rig.tree), p(r["pose_in"]), p(r["betas"]), p(r["trans_b"]), B, p(rig.lbs_ws), p(own["g_v0"]),
                           p(own["g_joints_mm"]), p(gp), p(gb), p(gt), st()), "lbs_tree_bwd")
    grads = {k: torch.full(rig.g_tb[k].shape, FILL, device=DEV) for k in GRADS}
    ft = rig.tables(share_light, grads)
    ck(L.harp_frame_setup_bwd(ctypes.byref(ft), p(rig.fid), B, S, FOCAL, self_shadow, p(gp), p(gb), p(gt), p(own["g_cam_T"]),
                              p(own["g_light_pos"]) if g_colors_d is not None else None, p(g_colors_d), st()), "frame_setup_bwd")
    torch.cuda.synchronize()
    return grads, dict(own, g_pose=gp, g_betas=gb)


def _lbs_reference(rig, rows, g_v0, g_joints_mm):
    """the tree layer alone: float64 autograd of tree_forward on the gathered rows for the float32 cotangents a backward itself formed:
    g_v0 (B,NV,3) WITH the vertex joints' gradients folded in, so g_joints_mm (B,n_out,3) counts for the chain joints only.  Summed into the
    rows of the tables in float64; slot_pose (B,51) / slot_betas (B,NB): per slot, what the scratch buffers hold"""
    H = rig.H
    fid = torch.tensor(rig.fid.cpu().tolist())
    B = rig.B
    leaves = [rows[k].double().requires_grad_() for k in ("pose_in", "betas", "trans_b")]
    v, j = TR.tree_forward(H["m64"], leaves[0].view(B, 17, 3), leaves[1], leaves[2])
    is_chain = torch.tensor([s >= 0 for s in H["host"]["joint_src"]], dtype=torch.float64)[None, :, None]
    gp, gb, gt = torch.autograd.grad((v * g_v0.cpu().double()).sum() + (j * g_joints_mm.cpu().double() * is_chain).sum(), leaves)
    z = lambda n: torch.zeros(T, n, dtype=torch.float64)
    return dict(g_pose=z(45).index_add_(0, fid, gp[:, 6:]), g_rot=z(3).index_add_(0, fid, gp[:, :3]), g_wrist_pose=z(3).index_add_(0, fid, gp[:, 3:6]),
                g_trans=z(3).index_add_(0, fid, gt), g_shape=gb[:, :10].sum(0), slot_pose=gp, slot_betas=gb)


def _check_scratch(tag, lbs, g_pose, g_betas, who):
    """g_pose_scratch (B,51) / g_betas_scratch (B,NB) per slot against the layer's float64 autograd at that backward's own cotangents: rule (1)"""
    for nm, got, want in (("g_pose_scratch", g_pose, lbs["slot_pose"]), ("g_betas_scratch", g_betas, lbs["slot_betas"])):
        assert (want.norm(dim=-1) > 0).all(), (tag, nm)
        _worst(f"{tag} {nm} per slot ({who})", (got.cpu().double() - want).norm(dim=-1), 1e-4 * want.norm(dim=-1) + 1e-300)


def _compare_chain(tag, rig, out, rows, own, blk_own, ref, cot, pre, centroid, shadow, ng):
    """what the chain part leaves behind: g_disp against the float64 autograd of the whole front, g_v0 (the layer's cotangent: the chain's
    VJP at the front's own float32 verts_mm plus g_joints_mm of the vertex joints, each on its vertex); both e_fused <= 4 e_blocks + 8 U |ref|_max"""
    B = rig.B
    cs = dict(rig.cs, verts_mm=out["verts_mm"], joints_mm=out["joints_mm"], cam_R=rows["cam_R"].view(B, 3, 3), cam_T=rows["cam_T"])
    chain_ref = _reference_grads(cs, cot, rows["light_pos"], centroid, shadow, ng)
    g_v0 = chain_ref["g_v0"].clone()
    for k, s in enumerate(rig.H["host"]["joint_src"]):
        if s < 0:
            g_v0[:, -s - 1] += chain_ref["g_joints_mm"][:, k]
    _compare(tag, cs, own, blk_own, dict(ref, g_v0=g_v0), pre, ["g_v0", "g_disp"], {})


def _check_fold(tag, rig, wide, cf, pre, gcd, own):
    """the vertex joints' share of g_v0 without e_blocks in the bound: the same back once more with g_joints_m = 0.  The chain's part of g_v0
    does not depend on g_joints_m, so the two g_v0 are bit-equal on every vertex no output joint names, and on a named vertex they differ by
    the sum of its joints' g_joints_mm: one rounding per joint added (an atomicAdd pair in arm_back_kernel, the owner's loop in
    arm_back_wide_kernel), each within U of |g_v0| + sum |g_joints_mm|"""
    _, p, st, ck = _L()
    keep = rig.d.t["g_joints_m"]
    rig.d.t["g_joints_m"] = torch.zeros_like(keep)
    own0 = _own(rig, pre)
    rig.d.t.update(own0)
    rig.fresh_grads()
    ck(rig.back(wide, rig.hand(share_light=cf["share_light"], self_shadow=cf["self_shadow"], shadow=cf["shadow"], ng=cf["ng"]), gcd), tag + " fold")
    torch.cuda.synchronize()
    rig.d.t["g_joints_m"] = keep
    a, c, gj = own["g_v0"].cpu().double(), own0["g_v0"].cpu().double(), own["g_joints_mm"].cpu().double()
    assert (own0["g_joints_mm"] == 0).all(), tag
    fold, mag, n = torch.zeros_like(a), c.abs().clone(), torch.zeros(a.shape[1])
    for k, s in enumerate(rig.H["host"]["joint_src"]):
        if s < 0:
            fold[:, -s - 1] += gj[:, k]
            mag[:, -s - 1] += gj[:, k].abs()
            n[-s - 1] += 1
    named = n > 0
    assert named.any() and torch.equal(_bits(own["g_v0"].cpu()[:, ~named]), _bits(own0["g_v0"].cpu()[:, ~named])) and fold[:, named].abs().min() > 0, tag
    _worst(tag + " g_v0, the vertex joints' fold", (a - c - fold)[:, named].abs(), (n[named, None] * U * mag[:, named]) + 1e-300)


def _back_all(tag, rig, wide, out, rows, cot, pre, g_colors, gcd, cf, lean_too):
    """one configuration on the forward outputs the rig holds: the stand-alone sequence (e_blocks), the fused back, every check; then the lean form"""
    _, p, st, ck = _L()
    sl, ss, sh, ng, col = cf["share_light"], cf["self_shadow"], cf["shadow"], cf["ng"], cf["colors"]
    H = rig.H
    centroid = out["centroid"].double() if sh else None
    ref = _reference(rig, centroid, cot, pre, g_colors if col else None, sl, ss, sh, ng)
    blk, blk_own = _blocks(rig, pre, gcd if col else None, sl, ss, sh, ng)
    own = _own(rig, pre)
    rig.d.t.update(own)
    rig.fresh_grads()
    ck(rig.back(wide, rig.hand(share_light=sl, self_shadow=ss, shadow=sh, ng=ng), gcd if col else None), tag)
    torch.cuda.synchronize()
    assert torch.isfinite(own["g_v0"]).all() and torch.equal(own["g_joints_mm"].cpu(), cot["g_joints_m"] * torch.tensor(MM, dtype=torch.float32)), tag
    lbs = tuple(_lbs_reference(rig, rows, o["g_v0"], o["g_joints_mm"]) for o in (own, blk_own))
    _check_tables(tag, rig, rig.g_tb, blk, ref, rows, cot, pre, g_colors, sl, ss, sh, light_rows=col, lbs=lbs, tb=H["tb"], layer_keys=LAYER,
                  layer="tree layer")
    _check_scratch(tag, lbs[0], rig.g_pose, rig.g_betas, "fused")
    _check_scratch(tag, lbs[1], blk_own["g_pose"], blk_own["g_betas"], "blocks")
    _compare_chain(tag, rig, out, rows, own, blk_own, ref, cot, pre, centroid, sh, ng)
    if lean_too and ng and col:
        _check_fold(tag, rig, wide, cf, pre, gcd, own)
    # the accumulators of the workspace are left cleared again (lbs_tree_body.h: chain_bwd_body consumes them)
    NJ, NP = H["lay"]["NJ"], (H["lay"]["NJ"] - 1) * 9
    assert (_bits(rig.lbs_ws[-rig.B * (NP + NJ * 3):]) == 0).all(), tag
    if lean_too and sh and col:
        # ---- lean form: light-view part, light / ambient scatter only; everything else keeps its fill
        lean = _own(rig, pre)
        rig.d.t.update(lean)
        rig.fresh_grads()
        ws0 = rig.lbs_ws.clone()
        ck(rig.back(wide, rig.hand(share_light=sl, self_shadow=ss, shadow=sh, ng=ng, light_only=1), gcd), tag + " lean")
        torch.cuda.synchronize()
        _check_tables(tag + " lean", rig, rig.g_tb, None, ref, rows, cot, pre, g_colors, sl, ss, sh, light_rows=True, lean=True, tb=H["tb"],
                      layer_keys=LAYER, layer="tree layer")
        for k, v in (("g_v0", lean["g_v0"]), ("g_joints_mm", lean["g_joints_mm"]), ("g_pose_scratch", rig.g_pose), ("g_betas_scratch", rig.g_betas)):
            assert (_bits(v) == NAN_BITS).all(), (tag, k)
        assert torch.equal(_bits(lean["g_cam_T"]), _bits(pre["g_cam_T"])) and torch.equal(_bits(lean["g_disp"]), _bits(pre["g_disp"])), tag
        assert torch.equal(_bits(rig.lbs_ws), _bits(ws0)), tag


@pytest.mark.parametrize("wide", [False, True], ids=["one_wg", "wide"])
@pytest.mark.parametrize("name,B", CASES)
def test_arm_back_every_gradient_row_against_float64(name, B, wide):
    """The fused front of the same width, then for every configuration the stand-alone backward (the crossing fused front -> harp_lbs_tree_bwd
    on the front's workspace, and e_blocks) and the fused back; last, the lean form (chain.light_only = 1) through the same entry point."""
    rig = _ArmRig(name, B)
    cot, pre, g_colors = _cot(rig)
    rig.d.t.update({k: _d(v) for k, v in cot.items()})
    gcd = _d(g_colors)
    for cf in CONFIGS:
        tag = (f"arm_back {name} {'wide' if wide else 'one_wg'} B={B} share={cf['share_light']} shadow={cf['shadow']} ng={cf['ng']} "
               f"colors={int(cf['colors'])}")
        out, rows = rig.run_front("wide" if wide else "one", tag, share_light=cf["share_light"], self_shadow=cf["self_shadow"], shadow=cf["shadow"])
        _back_all(tag, rig, wide, out, rows, cot, pre, g_colors, gcd, cf, lean_too=True)


@pytest.mark.parametrize("wide", [False, True], ids=["one_wg", "wide"])
def test_stand_alone_front_then_fused_arm_back(wide):
    """lbs_ws is an interface: harp_frame_setup_fwd + harp_lbs_tree_fwd + harp_mesh_chain_fwd fill the rows, the workspace and the chain's
    outputs, the fused back reads them; every gradient row under the same rules (production arm, B = 5, everything on)"""
    L, p, st, ck = _L()
    B = 5
    rig = _ArmRig("arm", B)
    r, t = rig.rows, rig.d.t
    tag = f"stand-alone front -> arm_back {'wide' if wide else 'one_wg'} B={B}"
    rig.reset_outputs()
    ft = rig.tables(0)
    ck(L.harp_frame_setup_fwd(ctypes.byref(ft), p(rig.fid), B, S, FOCAL, 1, *(p(r[k]) for k in ("pose_in", "betas", "trans_b", "cam_R", "cam_T", "light_pos")),
                              p(rig.colors), st()), "frame_setup_fwd")
    ck(L.harp_lbs_tree_fwd(ctypes.byref(rig.tree), p(r["pose_in"]), p(r["betas"]), p(r["trans_b"]), B, p(rig.lbs_ws), p(t["verts_mm"]), p(t["joints_mm"]),
                           st()), "lbs_tree_fwd")
    ck(L.harp_mesh_chain_fwd(ctypes.byref(rig.d.struct(1)), st()), "mesh_chain_fwd")
    torch.cuda.synchronize()
    rows = dict({k: v.cpu() for k, v in r.items()}, colors=rig.colors.cpu())
    _arm_check_rows(rig.H, tag, rows, FIDS[B], 0, 1)
    cot, pre, g_colors = _cot(rig)
    t.update({k: _d(v) for k, v in cot.items()})
    out = {k: t[k].cpu() for k in ("verts_mm", "joints_mm", "centroid")}
    _back_all(tag, rig, wide, out, rows, cot, pre, g_colors, _d(g_colors), CONFIGS[0], lean_too=False)


# ----------------------------------------------------------------------------------------------------------------------------------
# step book-keeping: known answers, no tolerance (the bodies of tests/test_gpu_step_front_back.py on the production arm)
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B", [1, 5])
def test_arm_front_prologue_takes_the_scheduled_row(B, form):
    M._prologue_body(_rig_of("arm"), lambda tag, rows, fid: _arm_check_rows(_host("arm"), tag, rows, fid, 0, 1), B, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B", [1, 3])
def test_arm_front_prologue_clears_the_batch_frames_of_the_mesh_gradients_only(B, form):
    M._clear_body(_rig_of("arm"), B, form, FIDS[B])


@pytest.mark.parametrize("form", ["one_wg", "wide", "lean_one_wg", "lean_wide"])
def test_arm_back_epilogue_turns_the_step_over(form):
    M._epilogue_body(_rig_of("arm"), form)


# ----------------------------------------------------------------------------------------------------------------------------------
# argument checks: refused on the host, nothing written
# ----------------------------------------------------------------------------------------------------------------------------------
def test_fused_arm_front_and_back_refuse_bad_arguments_untouched():
    """the rules of arm_ok, chain_fwd_ok / chain_bwd_ok, step_ok and the forms' own (scratch, kArmWide) that tests/test_abi.py cannot show
    with fake pointers, broken one at a time: HARP_ERR_ARG before any launch, with real buffers, and nothing is written"""
    from harp_amd import _lib
    L, p, st, ck = _L()
    B = 1
    rig = _ArmRig("arm", B)
    rf = _Refusals(rig, B, dict(g_pose=rig.g_pose, g_betas=rig.g_betas))
    gcd = rf.gcd
    hand = lambda **kw: rf.hand(model_field="tree", **kw)
    fronts = {f: (lambda h, f=f: rig.front(f, h)) for f in FORMS}
    backs = {"one_wg": lambda h: rig.back(False, h, gcd), "wide": lambda h: rig.back(True, h, gcd)}
    every = dict(fronts, **backs)

    def refused(calls, what, **kw):
        rf.refused(calls, what, model_field="tree", **kw)
    # ---- arm_ok: all four entry points
    for over in (dict(B=0), dict(B=-1), dict(V0=1025), dict(V0=1027), dict(E0=-1), dict(NJ=21), dict(NJ=23)):       # V0 != NV, chain.NJ != n_joints_out
        refused(every, over, chain=over)
    for over in (dict(NV=1025), dict(n_joints_out=21), dict(NB=10), dict(NB=32), dict(NJ=65), dict(NJ=0), dict(n_pose_in=16)):
        refused(every, over, model=over)
    for over in (dict(n_betas_out=10), dict(n_betas_out=21), dict(wrist_pose=None)):                             # n_betas_out != NB
        refused(every, over, tables=over)
    for k in ("fid", "pose_in", "betas", "trans_b", "cam_R", "cam_T", "light_pos", "colors", "lbs_ws", "weights_T"):
        refused(every, k, top={k: None})
    for k in ("v_template", "shapedirs_T", "posedirs_T", "posedirs", "J_template", "J_dirs", "weights", "pose_mean", "parents", "pose_src", "joint_src"):
        refused(every, k, model={k: None})
    null = ctypes.POINTER(_lib.ArmFront)()
    assert L.harp_arm_front_fwd(null, st()) == 1 and L.harp_arm_front_wide_fwd(null, p(rig.part_ws), st()) == 1
    assert L.harp_arm_back_bwd(null, p(gcd), p(rig.g_pose), p(rig.g_betas), st()) == 1
    assert L.harp_arm_back_wide_bwd(null, p(gcd), p(rig.g_pose), p(rig.g_betas), p(rig.part_ws), st()) == 1
    # ---- chain_fwd_ok / chain_bwd_ok (edges0: checked by arm_ok for all four)
    for k in CHAIN_FWD:
        refused(fronts, k, chain={k: None})
    for k in CHAIN_BWD:
        refused(backs, k, chain={k: None})
    # ---- size limits: one vertex past harp_mesh_chain_max_vertices(); NV = 1281 > 4 kArmWide = 1280, which only the wide forms refuse (the
    #      one-workgroup forms accept it and are not launched: the buffers here are sized for 1026)
    assert L.harp_mesh_chain_max_vertices() == 4096
    refused(every, "V = 4097", chain=dict(E0=4097 - rig.NV))
    wide_only = {"wide front": fronts["wide"], "wide back": backs["wide"]}
    refused(wide_only, "NV = 1281", chain=dict(V0=1281, E0=0), model=dict(NV=1281))
    # ---- step_ok
    ok_sched = dict(schedule=p(rf.sched), sched_row=p(rf.row), n_rows=2, tfid_out=p(rf.tfid))
    for bad in (dict(ok_sched, sched_row=None), dict(ok_sched, n_rows=0), dict(ok_sched, n_rows=-1)):
        refused(every, bad, step=_lib.StepFrame(**bad))
    for k in ("g_vd", "g_joints_m"):
        refused(fronts, "clear without " + k, step=_lib.StepFrame(clear_mesh_grads=1), chain={k: None})
    for n in (65, -1):
        refused(backs, f"n_loss = {n}", step=_lib.StepFrame(loss=p(rf.loss), loss_out=p(rf.loss), n_loss=n, loss_total=p(rf.total), loss_w=p(rf.loss)))
    # ---- the forms' scratch
    h = hand()
    assert L.harp_arm_front_wide_fwd(ctypes.byref(h), None, st()) == 1
    assert L.harp_arm_back_wide_bwd(ctypes.byref(h), p(gcd), p(rig.g_pose), p(rig.g_betas), None, st()) == 1
    for gp, gb in ((None, p(rig.g_betas)), (p(rig.g_pose), None)):
        assert L.harp_arm_back_bwd(ctypes.byref(h), p(gcd), gp, gb, st()) == 1
        assert L.harp_arm_back_wide_bwd(ctypes.byref(h), p(gcd), gp, gb, p(rig.part_ws), st()) == 1
    lean = hand(chain=dict(light_only=1))
    assert L.harp_arm_back_wide_bwd(ctypes.byref(lean), p(gcd), p(rig.g_pose), p(rig.g_betas), None, st()) == 1   # (before it forwards the lean form)
    for gp, gb in ((None, p(rig.g_betas)), (p(rig.g_pose), None)):
        assert L.harp_arm_back_wide_bwd(ctypes.byref(lean), p(gcd), gp, gb, p(rig.part_ws), st()) == 1
    assert rf.tried > 200
    rf.verify()
