"""-m gpu: the fused per-frame front and back of a fitting step, MANO path, through the raw C ABI -- harp_hand_front_fwd / _wide_fwd /
_hybrid_fwd (csrc/hand_front.hip), harp_hand_back_bwd / _wide_bwd (csrc/hand_back.hip) and the pieces of csrc/frame_body.h only they run
(schedule prologue, clear of the mesh gradients, table scatter, step epilogue) -- against the float64 composition tests/_front_ref.py
(row gathers + oracle MANO layer + mesh-chain reference, anchored by tests/test_front_ref_cpu.py).

T = 7 table rows, S = 100, the MANO template (778 -> 3093 vertices), batches fid = [6], [2, 0, 1] and [4, 4, 0, 6, 4] (one frame three
times: the scatter's atomics into one row).  The tables are tests/_front_ref.case_tables: rotation edges shifted per table ROW, every row
with its own cam / trans / light, shape components at +-3.  Outputs are pre-filled with NaN, gradient rows (added to) with FILL = 2^-10.

Forward: gathered rows bit-equal to their definition; verts_mm / joints_mm within the skinning bound of tests/test_gpu_geometry_terms.py;
every chain output within the stage bounds of tests/test_gpu_mesh_chain.py, each stage from the kernel's own output of the stage before.
Backward, every gradient row of every table, row by row, against float64 autograd at the float32 tables:
  * g_pose, g_rot, g_trans, g_shape: per-row rel-L2 <= 1e-4, the tolerance harp_lbs_mano_bwd is held to per frame; the rows no frame names keep
    FILL bit for bit.  harp_lbs_mano_bwd is held to it for cotangents that are given; here the cotangent g_v0 is itself float32 work on the
    float32 forward, and with a normal gradient (has_normal_grad) the composed gradient is ill-conditioned in the forward's positions: the
    template has vertices between the fingers whose |N| is 2e-6 m^2, just above the 1e-6 clamp (il up to 4.7e5).  Measured on the REFERENCE
    alone (float64, verts_mm rounded to float32 once, everything else exact): row 4 of g_pose moves by 1.2e-5 of its norm and g_shape by
    9.6e-6 (6.5e-7 and 1.8e-6 without the normal gradient); the forward's real error is ten times that rounding.  Measured on the
    STAND-ALONE sequence for that row (B = 5, has_normal_grad): 1.03e-4 behind the one-workgroup front, 0.90e-4 behind the wide front,
    0.46e-4 behind the stand-alone front -- it moves with the front's rounding, not with the backward.  So the rule is held in two parts,
    neither measured on the fused kernel: (1) the hand layer alone -- every row of the fused back AND of the stand-alone sequence against
    the float64 autograd of the MANO layer at that backward's own float32 g_v0 / g_joints_mm: rel-L2 <= 1e-4, no exception (its
    cotangent g_v0 is held to e_fused <= 4 e_blocks + 8 U |ref|_max against the chain's float64 VJP, as in tests/test_gpu_mesh_chain.py);
    (2) end to end against the float64 autograd of the whole front: rel-L2 <= 1e-4 for every row on which the stand-alone sequence, run on
    the same forward, holds it (every row but that one, and g_shape of that batch); only where e_blocks itself exceeds 1e-4 |ref| the
    bound is 4 e_blocks, the mesh chain's factor on the blocks' own error.
  * g_disp: e_fused <= 4 e_blocks + 8 U |ref|_max, e_blocks from the pinned six-launch sequence harp_mesh_chain_bwd + harp_lbs_mano_bwd +
    harp_frame_setup_bwd on the same forward outputs and workspace (which is also the crossing fused front -> stand-alone back).
  * g_cam, g_light_positions (three numbers per row): _scalar_sum_bounds of tests/test_gpu_mesh_chain.py per batch slot (value and bound of
    g_cam_T / g_light_pos from the kernel's own forward outputs), pushed through cam_row_bwd (|d row / d cam_T| times the slot's bound, 6 U
    for its own five operations) and summed over the slots of a row, plus (slots + 1) U of |FILL| + sum |terms| for the atomic adds.
  * g_amb_ratio = ((c0 + c1 + c2) - (c3 + c4 + c5)) amb (1 - amb): 2 U sum |c| + U |difference| for the two sums of three, 4 U amb for the
    sigmoid (the bound its forward is pinned to), one rounding for 1 - amb and for each product, one for the add onto FILL.
The shader's shares g_cam_T / g_light_pos (B,3) are accumulated into, so they are pre-filled with seeded values that the reference treats
as cotangents of the cam_T / light_pos rows.  Book-keeping (schedule row, clear, epilogue) and the argument checks are known-answer tests.

measured on the MI355X, worst error as a fraction of its bound: see docs/NOTEBOOK.md, "B.21. The fused MANO front and back against float64 through the C ABI"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _front_ref as R
from tests.test_gpu_building_blocks import DEV, U, _L, _d, _gen, _keep_alive, _worst  # noqa: F401 (_keep_alive: autouse)
from tests.test_gpu_frame_glue import _definition
from tests.test_gpu_geometry_terms import _mano_vertex_bound
from tests.test_gpu_mesh_chain import (FOCAL, FWD_SHAPES, MM, S, SHADOW_ONLY, _bits, _case, _check_forward_stages, _compare, _cotangents, _Dev,
                                       _reference_grads, _scalar_sum_bounds)

pytestmark = pytest.mark.gpu
T, NV, V = 7, 778, 3093
FIDS = {1: [6], 3: [2, 0, 1], 5: [4, 4, 0, 6, 4]}
FILL = 2.0 ** -10
GRADS = ("pose", "rot", "trans", "cam", "shape", "light_positions", "amb_ratio")
ROWS = dict(pose48=48, betas=10, trans_b=3, cam_R=9, cam_T=3, light_pos=3)
FRONTS = ("one", "wide", "hybrid")
NAN_BITS = int(_bits(torch.full((1,), float("nan")))[0])


@functools.lru_cache(maxsize=None)
def _host():
    """model, template tables and parameter tables; cached, never modified"""
    from harp_amd import synth
    model = synth.make_mano_model(seed=0)
    cs = _case("mano", 1)
    assert (cs["V0"], cs["V"], len(cs["comps"])) == (NV, V, 1)
    return dict(model=model, m64=R.mano_model(model), hm=torch.from_numpy(np.asarray(model["hands_mean"], np.float32)).reshape(15, 3), cs=cs,
                tb=R.case_tables(model, T), edges0=torch.from_numpy(cs["edges0_np"]).long(), faces=torch.from_numpy(cs["faces_np"]).long())


@functools.lru_cache(maxsize=None)
def _device_model():
    from harp_amd.manopth.manolayer import ManoDeviceModel
    return ManoDeviceModel(_host()["model"], DEV)


class _Rig:
    """every buffer a harp_hand_front of B frames points at, sized by the library's own *_ws_floats; front() / back() fill the structs the
    way FitEngine._frame_struct / _chain_struct / _step_context do"""
    NV, NJO = NV, 21                                                   # base vertices, output joints (the shared test bodies size buffers by them)

    def __init__(self, B, fid=None, extra_frames=0):
        L = _L()[0]
        H = _host()
        self.B = B
        cs = H["cs"]
        nan = lambda *s: torch.full(s, float("nan"))
        # (the chain's inputs of _Dev are outputs of the front here: NaN until written)
        self.cs = dict(cs, B=B, vertical=None, verts_mm=nan(B, NV, 3), joints_mm=nan(B, 21, 3), cam_R=nan(B, 3, 3), cam_T=nan(B, 3), light=nan(B, 3))
        self.d = _Dev(self.cs)
        t = self.d.t
        self.fid = _d(torch.tensor(FIDS[B] if fid is None else fid, dtype=torch.int32))
        self.tb = {k: _d(v) for k, v in H["tb"].items()}
        self.g_tb = {k: torch.full(H["tb"][k].shape, FILL, device=DEV) for k in GRADS}
        self.rows = {k: torch.full((B, n), float("nan"), device=DEV) for k, n in ROWS.items()}
        for k in ("cam_R", "cam_T", "light_pos"):                       # chain.cam_R / cam_T / light_pos alias the gathered rows
            self.rows[k] = t[k]
        self.colors = torch.full((10,), float("nan"), device=DEV)
        self.lbs_ws = torch.full((L.harp_lbs_mano_ws_floats(B),), float("nan"), device=DEV)
        self.part_ws = torch.full((L.harp_mesh_chain_wide_ws_floats(B, V),), float("nan"), device=DEV)
        self.g_betas = torch.full((B, 10), float("nan"), device=DEV)
        # the two gradient segments the prologue may clear: `extra_frames` frames behind the batch show that nothing else is cleared
        t["g_vd"] = torch.full((B + extra_frames, V, 3), 7.0, device=DEV)
        t["g_joints_m"] = torch.full((B + extra_frames, 21, 3), 7.0, device=DEV)

    def tables(self, share_light, grads=None, **over):
        from harp_amd import _lib
        ft = _lib.FrameTables(share_light=share_light, n_betas_out=10)
        for k in GRADS:
            setattr(ft, k, _lib.ptr(self.tb[k]))
            setattr(ft, "g_" + k, _lib.ptr((self.g_tb if grads is None else grads)[k]))
        for k, v in over.items():
            setattr(ft, k, v)
        return ft

    def hand(self, share_light=0, self_shadow=1, shadow=1, ng=0, light_only=0, step=None, grads=None):
        from harp_amd import _lib
        p = _lib.ptr
        h = _lib.HandFront()
        if step is not None:
            h.step = step
        h.chain, h.mano, h.tables = self.d.struct(shadow, ng, light_only), _device_model().struct, self.tables(share_light, grads)
        h.fid, h.colors, h.lbs_ws, h.self_shadow = p(self.fid), p(self.colors), p(self.lbs_ws), self_shadow
        for k in ROWS:
            setattr(h, k, p(self.rows[k]))
        return h

    def front(self, form, h):
        L, p, st, _ = _L()
        if form == "one":
            return L.harp_hand_front_fwd(ctypes.byref(h), st())
        if form == "wide":
            return L.harp_hand_front_wide_fwd(ctypes.byref(h), p(self.part_ws), st())
        return L.harp_hand_front_hybrid_fwd(ctypes.byref(h), st())

    def back(self, wide, h, g_colors):
        L, p, st, _ = _L()
        if wide:
            return L.harp_hand_back_wide_bwd(ctypes.byref(h), p(g_colors), p(self.g_betas), p(self.part_ws), st())
        return L.harp_hand_back_bwd(ctypes.byref(h), p(g_colors), p(self.g_betas), st())

    def reset_outputs(self):
        for k in FWD_SHAPES:
            self.d.t[k].fill_(float("nan"))
        for k in ("verts_mm", "joints_mm"):
            self.d.t[k].fill_(float("nan"))
        for v in self.rows.values():
            v.fill_(float("nan"))
        self.colors.fill_(float("nan"))
        self.lbs_ws.fill_(float("nan"))

    def run_front(self, form, tag="", **kw):
        self.reset_outputs()
        _L()[3](self.front(form, self.hand(**kw)), f"hand_front {form} {tag}")
        torch.cuda.synchronize()
        return {k: self.d.t[k].cpu() for k in list(FWD_SHAPES) + ["verts_mm", "joints_mm"]}, dict({k: v.cpu() for k, v in self.rows.items()},
                                                                                                 colors=self.colors.cpu())


def _check_rows(tag, rows, fid, share_light, self_shadow, ref=None, exact=("pose48", "betas", "trans_b", "light_pos")):
    """the gathered rows against _definition, bit for bit (cam_T's third component and the sigmoid colours within their pinned roundings).
    ref / exact: the definition's rows and the names of those held bit for bit (default: the MANO rows of _host()'s tables; the arm path
    of tests/test_gpu_arm_front_back.py passes its own)"""
    B = len(fid)
    if ref is None:
        ref = _definition({k: v.double() for k, v in _host()["tb"].items()}, torch.tensor(fid), False, share_light, self_shadow)
    for k in exact:
        assert torch.equal(_bits(rows[k]), _bits(ref[k].float())), (tag, k)
    assert torch.equal(rows["cam_R"], torch.tensor([-1.0, 0, 0, 0, -1, 0, 0, 0, 1]).repeat(B, 1)), tag
    # cam_T: two negations (exact) and 2 focal / (S c0 + 1e-9): 3 U, as harp_frame_setup_fwd
    assert torch.equal(_bits(rows["cam_T"][:, :2]), _bits(ref["cam_T"][:, :2].float())), tag
    _worst(tag + " cam_T", (rows["cam_T"].double() - ref["cam_T"]).abs(), 3 * U * ref["cam_T"].abs() + 1e-300)
    if self_shadow:
        _worst(tag + " colors", (rows["colors"][:9].double() - ref["colors"]).abs(), torch.tensor(4 * U))
        assert (rows["colors"][6:9] == 0).all() and torch.equal(_bits(rows["colors"][:3]), _bits(rows["colors"][:1].repeat(3))), tag
    else:
        assert torch.equal(rows["colors"][:9], torch.tensor([0.5] * 3 + [0.4] * 3 + [0.1] * 3)), tag
    assert int(_bits(rows["colors"][9:])[0]) == NAN_BITS, tag           # (the slot behind the nine colours: never written)
    return ref


# ----------------------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FRONTS)
@pytest.mark.parametrize("B", [1, 3, 5])
def test_hand_front_forward_against_float64(B, form):
    from oracle import harp_ref as Hr
    H = _host()
    fid = FIDS[B]
    rig = _Rig(B)
    tag = f"hand_front {form} B={B}"
    # ---- share_light = 0, self_shadow = 1, shadow = 1: everything
    out, rows = rig.run_front(form, tag, share_light=0, self_shadow=1, shadow=1)
    ref = _check_rows(tag, rows, fid, 0, 1)
    assert len({tuple(r.tolist()) for r in rows["light_pos"]}) == len(set(fid)) and len({tuple(r.tolist()) for r in rows["cam_T"]}) == len(set(fid))
    v_ref, j_ref = Hr.mano_forward(H["m64"], ref["pose48"], ref["betas"], ref["trans_b"])
    bv = _mano_vertex_bound(H["m64"], H["hm"], rows["pose48"], rows["betas"], v_ref)
    _worst(tag + " verts_mm", (out["verts_mm"].double() - v_ref).abs(), bv)
    _worst(tag + " joints_mm", (out["joints_mm"].double() - j_ref).abs(), bv)
    cs = dict(rig.cs, verts_mm=out["verts_mm"], joints_mm=out["joints_mm"], cam_R=rows["cam_R"].view(B, 3, 3), cam_T=rows["cam_T"])
    _check_forward_stages(tag, cs, out, rows["light_pos"], general_rotation=False)
    # the forward's rows of the workspace (csrc/lbs_body.h: lbs_ws): pose_map 135 | A 192 | j16 48 | Jrest 48 | Rloc 144 | G 192 in front, v_posed
    # 778 * 3 at the end, each times B; the backward's rows between them stay NaN
    ws, head, tail = rig.lbs_ws.cpu(), B * (135 + 192 + 48 + 48 + 144 + 192), B * NV * 3
    assert ws.numel() == head + B * (NV * 3 + NV * 12 + 192 + 135 + 48) + tail, tag
    assert torch.isfinite(ws[:head]).all() and torch.isfinite(ws[-tail:]).all() and torch.isnan(ws[head:-tail]).all(), tag
    # ---- share_light = 1, self_shadow = 0: the light of row 0 for every frame; the stages again where the batch has three frames
    out1, rows1 = rig.run_front(form, tag, share_light=1, self_shadow=0, shadow=1)
    _check_rows(tag + " share", rows1, fid, 1, 0)
    assert torch.equal(rows1["light_pos"], H["tb"]["light_positions"][:1].repeat(B, 1)), tag
    for k in FWD_SHAPES:
        if k not in SHADOW_ONLY:
            assert torch.equal(_bits(out1[k]), _bits(out[k])), (tag, k)
    assert torch.equal(_bits(out1["verts_mm"]), _bits(out["verts_mm"])) and torch.isfinite(out1["ndc_l"]).all(), tag
    if B == 3:
        _check_forward_stages(tag + " share", cs, out1, rows1["light_pos"], general_rotation=False)
    # ---- shadow = 0 (share_light = 1, self_shadow = 1): the shadow-only outputs keep their NaN, the rest is the same
    out0, rows0 = rig.run_front(form, tag, share_light=1, self_shadow=1, shadow=0)
    _check_rows(tag + " shadow=0", rows0, fid, 1, 1)
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
def _cot(rig):
    """seeded cotangents of the chain (+ g_colors and the shader's shares of g_cam_T / g_light_pos, which the back accumulates into)"""
    B = rig.B
    cot = _cotangents(rig.cs)
    g = _gen(13 + B)
    pre = {k: torch.randn(s, generator=g) * 1e-3 for k, s in (("g_light_pos", (B, 3)), ("g_cam_T", (B, 3)), ("g_disp", (rig.cs["V"],)))}
    return cot, pre, torch.randn(9, generator=g)


def _reference(rig, rows, centroid, cot, pre, g_colors, share_light, self_shadow, shadow, ng):
    """float64 autograd of tests/_front_ref.py at the float32 tables; pre g_cam_T / g_light_pos: cotangents of the cam_T / light_pos rows"""
    H = _host()
    fid = torch.tensor(rig.fid.cpu().tolist())
    cot64 = {k: v.double() for k, v in cot.items()}

    def f(tb, disp):
        out = R.front(tb, fid, disp, H["edges0"], H["faces"], H["m64"], share_light, self_shadow, mm=MM, centroid_value=centroid)
        t = R.total(out, cot64, g_colors.double() if g_colors is not None else None, shadow, ng) + (out["cam_T"] * pre["g_cam_T"].double()).sum()
        if g_colors is not None:                                       # (no appearance gradient: the light rows are not scattered)
            t = t + (out["light_pos"] * pre["g_light_pos"].double()).sum()
        return t
    return R.table_grads({k: v.double() for k, v in H["tb"].items()}, H["cs"]["disp"].double(), f)


def _blocks(rig, cotd, pre, g_colors_d, share_light, self_shadow, shadow, ng):
    """the pinned six-launch sequence on the same forward outputs and the same workspace: harp_mesh_chain_bwd + harp_lbs_mano_bwd (four
    launches) + harp_frame_setup_bwd, into gradient buffers of its own"""
    L, p, st, ck = _L()
    B, r = rig.B, rig.rows
    own = {k: _d(v) for k, v in pre.items()}
    own["g_v0"] = torch.full((B, NV, 3), float("nan"), device=DEV)
    own["g_joints_mm"] = torch.full((B, 21, 3), float("nan"), device=DEV)
    ch = rig.d.struct(shadow, ng, **{k: p(v) for k, v in own.items()})
    ck(L.harp_mesh_chain_bwd(ctypes.byref(ch), st()), "mesh_chain_bwd")
    g_v0_chain = own["g_v0"].clone()                                   # (harp_lbs_mano_bwd folds the tip joints' gradients into its g_verts)
    gp, gb, gt = (torch.full(s, float("nan"), device=DEV) for s in ((B, 48), (B, 10), (B, 3)))
    ck(L.harp_lbs_mano_bwd(ctypes.byref(_device_model().struct), p(r["pose48"]), p(r["betas"]), p(r["trans_b"]), B, p(rig.lbs_ws), p(own["g_v0"]),
                           p(own["g_joints_mm"]), p(gp), p(gb), p(gt), st()), "lbs_mano_bwd")
    grads = {k: torch.full(rig.g_tb[k].shape, FILL, device=DEV) for k in GRADS}
    ft = rig.tables(share_light, grads)
    ck(L.harp_frame_setup_bwd(ctypes.byref(ft), p(rig.fid), B, S, FOCAL, self_shadow, p(gp), p(gb), p(gt), p(own["g_cam_T"]),
                              p(own["g_light_pos"]) if g_colors_d is not None else None, p(g_colors_d), st()), "frame_setup_bwd")
    torch.cuda.synchronize()
    return grads, dict(own, g_v0=g_v0_chain)


def _lbs_reference(rig, rows, g_v0, g_joints_mm):
    """the hand layer alone: float64 autograd of oracle mano_forward on the gathered rows for the float32 cotangents g_v0 (B,778,3) /
    g_joints_mm (B,21,3) a backward itself formed, summed into the rows of the tables in float64"""
    from oracle import harp_ref as Hr
    H = _host()
    fid = torch.tensor(rig.fid.cpu().tolist())
    leaves = [rows[k].double().requires_grad_() for k in ("pose48", "betas", "trans_b")]
    v, j = Hr.mano_forward(H["m64"], *leaves)
    gp, gb, gt = torch.autograd.grad((v * g_v0.cpu().double()).sum() + (j * g_joints_mm.cpu().double()).sum(), leaves)
    z = lambda n: torch.zeros(T, n, dtype=torch.float64)
    return dict(g_pose=z(45).index_add_(0, fid, gp[:, 3:]), g_rot=z(3).index_add_(0, fid, gp[:, :3]), g_trans=z(3).index_add_(0, fid, gt), g_shape=gb.sum(0))


def _report(tag, name, e_fused, e_blocks, bound):
    print(f"[{tag} {name}] e_fused {e_fused:.3e} e_blocks {e_blocks:.3e} bound {bound:.3e}: {e_fused / bound:.3f} of it")
    assert np.isfinite(e_fused) and e_fused <= bound, (tag, name, e_fused, e_blocks, bound)


def _check_tables(tag, rig, got, blk, ref, rows, cot, pre, g_colors, share_light, self_shadow, shadow, light_rows, lean=False, lbs=None, tb=None,
                  layer_keys=("pose", "rot", "trans", "shape"), layer="hand layer"):
    """every gradient row of every table of the fused back (got) against the float64 autograd (ref) under the rules of the module docstring;
    blk: the same rows from the stand-alone sequence (None: not run).  light_rows: an appearance gradient was given.  lean: chain.light_only,
    the hand-layer and camera rows keep FILL.  lbs: (_lbs_reference at the fused back's own g_v0, at the stand-alone sequence's).
    tb: the float32 parameter tables (default: _host()'s), layer_keys: the tables the skinning layer's gradient goes to, layer: its name
    in the printed lines -- the arm path passes its own (tests/test_gpu_arm_front_back.py)."""
    tb = _host()["tb"] if tb is None else tb
    T = tb["cam"].shape[0]
    fid = rig.fid.cpu().tolist()
    B = len(fid)
    absent = [r for r in range(T) if r not in fid]
    g64 = {k: v.cpu().double() - FILL for k, v in got.items()}
    b64 = {k: v.cpu().double() - FILL for k, v in blk.items()} if blk is not None else None
    fill_bits = int(_bits(torch.full((1,), FILL))[0])
    # ---- hand-layer rows, per row: rel-L2 <= 1e-4 against the hand layer's float64 autograd at the backward's own g_v0 (fused and stand-alone),
    #      and end to end 1e-4 |ref|, replaced by 4 e_blocks only where e_blocks itself exceeds it (module docstring); rows no frame names:
    #      FILL, bit for bit
    for k in layer_keys:
        want = ref["g_" + k].reshape(-1, ref["g_" + k].shape[-1]) if k != "shape" else ref["g_shape"][None]
        have = g64[k].reshape(want.shape)
        if lean:
            assert (_bits(got[k]) == fill_bits).all(), (tag, k)
            continue
        for r in (range(T) if k != "shape" else [0]):
            if k != "shape" and r in absent:
                assert (_bits(got[k][r]) == fill_bits).all() and want[r].abs().max() == 0, (tag, k, r)
                continue
            n = want[r].norm().item()
            assert n > 0, (tag, k, r)
            e_b = (b64[k].reshape(want.shape)[r] - want[r]).norm().item()
            # 1e-4 |ref|; only where the stand-alone sequence itself misses that on the same forward, 4 times its own error
            _report(tag, f"g_{k} row {r} |ref| {n:.3e}", (have[r] - want[r]).norm().item(), e_b, 1e-4 * n if e_b <= 1e-4 * n else 4 * e_b)
            for who, mine, lref in (("fused", have, lbs[0]), ("blocks", b64[k].reshape(want.shape), lbs[1])):
                lw = lref["g_" + k].reshape(want.shape)[r]
                _worst(f"{tag} g_{k} row {r}, {layer} alone ({who})", (mine[r] - lw).norm()[None], 1e-4 * lw.norm()[None] + 1e-300)
    # ---- g_cam and g_light_positions from the per-slot derived values and bounds
    cs = dict(rig.cs, cam_R=rows["cam_R"].view(B, 3, 3), cam_T=rows["cam_T"])
    rig.d.light = rows["light_pos"]
    sums = _scalar_sum_bounds(cs, rig.d, cot, pre, shadow)
    cam = tb["cam"].double()
    want_T, bound_T = sums["g_cam_T"]
    tot_T = pre["g_cam_T"].double() + want_T                             # what the slot's g_cam_T holds after the chain
    want_c, bound_c, mag_c = torch.zeros(T, 3, dtype=torch.float64), torch.zeros(T, 3, dtype=torch.float64), torch.full((T, 3), FILL, dtype=torch.float64)
    for b, f in enumerate(fid):
        den = S * cam[f, 0] + 1e-9
        J = torch.stack([-2.0 * FOCAL * S / den ** 2, torch.tensor(-1.0, dtype=torch.float64), torch.tensor(-1.0, dtype=torch.float64)])
        term = J * tot_T[b, [2, 0, 1]]
        want_c[f] += term
        bound_c[f] += J.abs() * bound_T[b, [2, 0, 1]] + 6 * U * term.abs()
        mag_c[f] += term.abs()
    bound_c += (torch.bincount(torch.tensor(fid), minlength=T)[:, None] + 1) * U * mag_c
    rows_l = sorted(set(fid)) if not share_light else [0]
    want_l, bound_l, mag_l = torch.zeros(T, 3, dtype=torch.float64), torch.zeros(T, 3, dtype=torch.float64), torch.full((T, 3), FILL, dtype=torch.float64)
    cnt_l = torch.zeros(T, 1, dtype=torch.float64)
    for b, f in enumerate(fid):
        lf = 0 if share_light else f
        tot = pre["g_light_pos"].double()[b] + (sums["g_light_pos"][0][b] if shadow else 0.0)
        want_l[lf] += tot
        bound_l[lf] += (sums["g_light_pos"][1][b] if shadow else 0.0)
        mag_l[lf] += tot.abs()
        cnt_l[lf] += 1
    bound_l += (cnt_l + 1) * U * mag_l
    for k, want, bound, named in (("cam", want_c, bound_c, [] if lean else sorted(set(fid))), ("light_positions", want_l, bound_l, rows_l if light_rows else [])):
        for r in range(T):
            if r not in named:
                assert (_bits(got[k][r]) == fill_bits).all(), (tag, k, r)
                continue
            rmax = ref["g_" + k][r].abs().max().item()
            assert rmax > 0, (tag, k, r)
            # the derived value (from the kernel's own float32 forward) is the composed reference's row up to the forward's error: 1e-4 of the
            # row, the tolerance the gradients of a step are held to (measured: the kernels themselves are within 1.1e-5 of the autograd)
            assert (want[r] - ref["g_" + k][r]).abs().max().item() <= 1e-4 * rmax, (tag, k, r, want[r], ref["g_" + k][r])
            e_b = (b64[k][r] - ref["g_" + k][r]).abs().max().item() if b64 is not None else float("nan")
            print(f"[{tag} g_{k} row {r}] against the float64 autograd: e_fused {(g64[k][r] - ref['g_' + k][r]).abs().max().item():.3e} e_blocks {e_b:.3e} "
                  f"|ref| {ref['g_' + k][r].abs().max().item():.3e}")
            _worst(f"{tag} g_{k} row {r} (derived)", (g64[k][r] - want[r]).abs(), bound[r] + 1e-300)
    # ---- g_amb_ratio
    if light_rows and self_shadow:
        c = g_colors.double()
        amb = torch.sigmoid(tb["amb_ratio"].double())[0].item()
        ga = (c[:3].sum() - c[3:6].sum()).item()
        s_ = amb * (1 - amb)
        d_s = 4 * U * amb * (1 - amb) + amb * (4 * U * amb + U * (1 - amb)) + U * s_
        bound = (2 * U * c[:6].abs().sum().item() + U * abs(ga)) * s_ + abs(ga) * d_s + 2 * U * abs(ga * s_) + U * (FILL + abs(ga * s_))
        want = ref["g_amb_ratio"][0].item()
        assert abs(want - ga * s_) <= 1e-13 * abs(want) and want != 0
        e_b = abs(b64["amb_ratio"][0].item() - want) if b64 is not None else float("nan")
        _report(tag, "g_amb_ratio", abs(g64["amb_ratio"][0].item() - want), e_b, bound)
    else:
        assert (_bits(got["amb_ratio"]) == fill_bits).all(), tag


def _compare_chain(tag, rig, out, rows, own, blk_own, ref, cot, pre, centroid, shadow, ng):
    """what the chain part leaves behind: g_disp against the float64 autograd of the whole front, g_v0 (the hand layer's cotangent) against
    the float64 VJP of the chain at the front's own float32 verts_mm; both e_fused <= 4 e_blocks + 8 U |ref|_max"""
    B = rig.B
    cs = dict(rig.cs, verts_mm=out["verts_mm"], joints_mm=out["joints_mm"], cam_R=rows["cam_R"].view(B, 3, 3), cam_T=rows["cam_T"])
    chain_ref = _reference_grads(cs, cot, rows["light_pos"], centroid, shadow, ng)
    _compare(tag, cs, own, blk_own, dict(ref, g_v0=chain_ref["g_v0"]), pre, ["g_v0", "g_disp"], {})


CONFIGS = [dict(share_light=0, self_shadow=1, shadow=1, ng=1, colors=True),      # everything
           dict(share_light=1, self_shadow=1, shadow=1, ng=0, colors=False),     # g_colors = NULL: the light and ambient rows stay untouched
           dict(share_light=1, self_shadow=0, shadow=0, ng=1, colors=True)]      # the shared light: row 0 takes every slot's share; fixed colours


@pytest.mark.parametrize("wide", [False, True], ids=["one_wg", "wide"])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_hand_back_every_gradient_row_against_float64(B, wide):
    """The fused front of the same width, then for every configuration the stand-alone six-launch backward (the crossing fused front ->
    harp_lbs_mano_bwd on the front's workspace, and e_blocks) and the fused back; last, the lean form (chain.light_only = 1) through the
    same entry point: only g_light_positions and g_amb_ratio move."""
    L, p, st, ck = _L()
    rig = _Rig(B)
    form = "wide" if wide else "one"
    cot, pre, g_colors = _cot(rig)
    cotd = {k: _d(v) for k, v in cot.items()}
    rig.d.t.update(cotd)
    gcd = _d(g_colors)
    for cf in CONFIGS:
        sl, ss, sh, ng, col = cf["share_light"], cf["self_shadow"], cf["shadow"], cf["ng"], cf["colors"]
        tag = f"hand_back {'wide' if wide else 'one_wg'} B={B} share={sl} shadow={sh} ng={ng} colors={int(col)}"
        out, rows = rig.run_front(form, tag, share_light=sl, self_shadow=ss, shadow=sh)
        centroid = out["centroid"].double() if sh else None
        ref = _reference(rig, rows, centroid, cot, pre, g_colors if col else None, sl, ss, sh, ng)
        blk, blk_own = _blocks(rig, cotd, pre, gcd if col else None, sl, ss, sh, ng)
        own = {k: _d(v) for k, v in pre.items()}
        own["g_v0"] = torch.full((B, NV, 3), float("nan"), device=DEV)
        own["g_joints_mm"] = torch.full((B, 21, 3), float("nan"), device=DEV)
        rig.d.t.update(own)
        for v in rig.g_tb.values():
            v.fill_(FILL)
        rig.g_betas.fill_(float("nan"))
        ck(rig.back(wide, rig.hand(share_light=sl, self_shadow=ss, shadow=sh, ng=ng), gcd if col else None), tag)
        torch.cuda.synchronize()
        assert torch.isfinite(own["g_v0"]).all() and torch.equal(own["g_joints_mm"].cpu(), cot["g_joints_m"] * torch.tensor(MM, dtype=torch.float32)), tag
        lbs = tuple(_lbs_reference(rig, rows, o["g_v0"], o["g_joints_mm"]) for o in (own, blk_own))
        _check_tables(tag, rig, rig.g_tb, blk, ref, rows, cot, pre, g_colors, sl, ss, sh, light_rows=col, lbs=lbs)
        _compare_chain(tag, rig, out, rows, own, blk_own, ref, cot, pre, centroid, sh, ng)
        if sh and col:
            # ---- lean form: light-view part, light / ambient scatter only; everything else keeps its fill
            lean = {k: _d(v) for k, v in pre.items()}
            lean["g_v0"] = torch.full((B, NV, 3), float("nan"), device=DEV)
            lean["g_joints_mm"] = torch.full((B, 21, 3), float("nan"), device=DEV)
            rig.d.t.update(lean)
            for v in rig.g_tb.values():
                v.fill_(FILL)
            rig.g_betas.fill_(float("nan"))
            ws0 = rig.lbs_ws.clone()
            ck(rig.back(wide, rig.hand(share_light=sl, self_shadow=ss, shadow=sh, ng=ng, light_only=1), gcd), tag + " lean")
            torch.cuda.synchronize()
            _check_tables(tag + " lean", rig, rig.g_tb, None, ref, rows, cot, pre, g_colors, sl, ss, sh, light_rows=True, lean=True)
            assert (_bits(lean["g_v0"]) == NAN_BITS).all() and (_bits(lean["g_joints_mm"]) == NAN_BITS).all() and (_bits(rig.g_betas) == NAN_BITS).all(), tag
            assert torch.equal(_bits(lean["g_cam_T"]), _bits(pre["g_cam_T"])) and torch.equal(_bits(lean["g_disp"]), _bits(pre["g_disp"])), tag
            assert torch.equal(_bits(rig.lbs_ws), _bits(ws0)), tag


@pytest.mark.parametrize("wide", [False, True], ids=["one_wg", "wide"])
def test_stand_alone_front_then_fused_back(wide):
    """lbs_ws is an interface: harp_frame_setup_fwd + harp_lbs_mano_fwd + harp_mesh_chain_fwd fill the rows, the workspace and the chain's
    outputs, the fused back reads them; every gradient row under the same rules (B = 5, everything on)"""
    L, p, st, ck = _L()
    B = 5
    rig = _Rig(B)
    r, t = rig.rows, rig.d.t
    tag = f"stand-alone front -> hand_back {'wide' if wide else 'one_wg'} B={B}"
    rig.reset_outputs()
    ft = rig.tables(0)
    ck(L.harp_frame_setup_fwd(ctypes.byref(ft), p(rig.fid), B, S, FOCAL, 1, *(p(r[k]) for k in ("pose48", "betas", "trans_b", "cam_R", "cam_T", "light_pos")),
                              p(rig.colors), st()), "frame_setup_fwd")
    ck(L.harp_lbs_mano_fwd(ctypes.byref(_device_model().struct), p(r["pose48"]), p(r["betas"]), p(r["trans_b"]), B, p(rig.lbs_ws), p(t["verts_mm"]),
                           p(t["joints_mm"]), st()), "lbs_mano_fwd")
    ch = rig.d.struct(1)
    ck(L.harp_mesh_chain_fwd(ctypes.byref(ch), st()), "mesh_chain_fwd")
    torch.cuda.synchronize()
    rows = dict({k: v.cpu() for k, v in r.items()}, colors=rig.colors.cpu())
    _check_rows(tag, rows, FIDS[B], 0, 1)
    cot, pre, g_colors = _cot(rig)
    cotd = {k: _d(v) for k, v in cot.items()}
    t.update(cotd)
    gcd = _d(g_colors)
    ref = _reference(rig, rows, t["centroid"].cpu().double(), cot, pre, g_colors, 0, 1, 1, 1)
    blk, blk_own = _blocks(rig, cotd, pre, gcd, 0, 1, 1, 1)
    own = {k: _d(v) for k, v in pre.items()}
    own["g_v0"] = torch.full((B, NV, 3), float("nan"), device=DEV)
    own["g_joints_mm"] = torch.full((B, 21, 3), float("nan"), device=DEV)
    t.update(own)
    ck(rig.back(wide, rig.hand(share_light=0, self_shadow=1, shadow=1, ng=1), gcd), tag)
    torch.cuda.synchronize()
    lbs = tuple(_lbs_reference(rig, rows, o["g_v0"], o["g_joints_mm"]) for o in (own, blk_own))
    _check_tables(tag, rig, rig.g_tb, blk, ref, rows, cot, pre, g_colors, 0, 1, 1, light_rows=True, lbs=lbs)
    out = {k: t[k].cpu() for k in ("verts_mm", "joints_mm", "centroid")}
    _compare_chain(tag, rig, out, rows, own, blk_own, ref, cot, pre, out["centroid"].double(), 1, 1)


# ----------------------------------------------------------------------------------------------------------------------------------
# step book-keeping: known answers, no tolerance
# ----------------------------------------------------------------------------------------------------------------------------------
SCHED = {1: [[3], [5]], 3: [[1, 6, 3], [0, 4, 4]], 5: [[6, 5, 4, 3, 2], [1, 1, 0, 5, 1]]}


def _prologue_body(make_rig, check_rows, B, form):
    """shared with tests/test_gpu_arm_front_back.py.  make_rig(B, fid=None, extra_frames=0): a rig with run_front / front / hand / reset_outputs,
    fid, rows, colors and d.t; check_rows(tag, rows, fid): its `_check_rows` at share_light = 0, self_shadow = 1"""
    from harp_amd import _lib
    L, p, st, ck = _L()
    sched = torch.tensor(SCHED[B], dtype=torch.int32)
    # the target schedule is the head of a four-row buffer of distinct values: a row index that lost its wrap stays inside it and shows
    tbuf = (1000 + torch.arange(4 * B, dtype=torch.int32)).reshape(4, B)
    for counter, row in ((3, 1), (2, 0)):
        plain = make_rig(B, fid=SCHED[B][row])
        want_out, want_rows = plain.run_front(form, "plain")
        for with_t in (True, False):
            tag = f"prologue {form} B={B} sched_row={counter} tschedule={int(with_t)}"
            rig = make_rig(B, fid=[-1] * B)
            sd, td, rowd, tfid = _d(sched), _d(tbuf), _d(torch.tensor([counter], dtype=torch.int32)), torch.full((B,), -7, dtype=torch.int32, device=DEV)
            step = _lib.StepFrame(schedule=p(sd), tschedule=p(td) if with_t else None, sched_row=p(rowd), n_rows=2, target_offset=2, tfid_out=p(tfid))
            rig.reset_outputs()
            ck(rig.front(form, rig.hand(step=step)), tag)
            torch.cuda.synchronize()
            # ---- fid / tfid_out as harp_schedule_next_rows defines them, and as known answers; the row counter is the epilogue's to bump
            c2, fid2, tfid2 = _d(torch.tensor([counter], dtype=torch.int32)), torch.full((B,), -1, dtype=torch.int32, device=DEV), torch.full(
                (B,), -7, dtype=torch.int32, device=DEV)
            ck(L.harp_schedule_next_rows(p(sd), p(td) if with_t else None, 2, B, 2, p(c2), p(fid2), p(tfid2), None, 0, st()), "schedule_next_rows")
            torch.cuda.synchronize()
            assert torch.equal(rig.fid.cpu(), fid2.cpu()) and torch.equal(tfid.cpu(), tfid2.cpu()), tag
            assert rig.fid.cpu().tolist() == SCHED[B][row], tag
            assert tfid.cpu().tolist() == (tbuf[row].tolist() if with_t else [f - 2 for f in SCHED[B][row]]), tag
            assert rowd.cpu().tolist() == [counter] and c2.cpu().tolist() == [row + 1], tag
            # ---- the forward outputs are those of the scheduled row
            rows = dict({k: v.cpu() for k, v in rig.rows.items()}, colors=rig.colors.cpu())
            check_rows(tag, rows, SCHED[B][row])
            for k, v in want_rows.items():
                assert torch.equal(_bits(rows[k]), _bits(v)), (tag, k)
            for k, v in want_out.items():
                assert torch.equal(_bits(rig.d.t[k].cpu()), _bits(v)), (tag, k)
            assert (rig.d.t["g_vd"] == 7).all() and (rig.d.t["g_joints_m"] == 7).all(), tag               # no clear asked for


@pytest.mark.parametrize("form", FRONTS)
@pytest.mark.parametrize("B", [1, 5])
def test_front_prologue_takes_the_scheduled_row(B, form):
    _prologue_body(_Rig, lambda tag, rows, fid: _check_rows(tag, rows, fid, 0, 1), B, form)


def _clear_body(make_rig, B, form, fids):
    """shared with tests/test_gpu_arm_front_back.py; fids: the frames the rig's batch of B names by default"""
    from harp_amd import _lib
    _, p, st, ck = _L()
    rig = make_rig(B, extra_frames=1)
    rig.reset_outputs()
    ck(rig.front(form, rig.hand(step=_lib.StepFrame(clear_mesh_grads=1))), f"clear {form} B={B}")
    torch.cuda.synchronize()
    for k in ("g_vd", "g_joints_m"):
        g = rig.d.t[k].cpu()
        assert (_bits(g[:B]) == 0).all() and (g[B:] == 7).all(), (form, B, k)          # +0.0 in all B frames, the frame behind them untouched
    assert torch.isfinite(rig.d.t["ndc_c"]).all() and torch.equal(rig.fid.cpu(), torch.tensor(fids, dtype=torch.int32))


@pytest.mark.parametrize("form", FRONTS)
@pytest.mark.parametrize("B", [1, 3])
def test_front_prologue_clears_the_batch_frames_of_the_mesh_gradients_only(B, form):
    _clear_body(_Rig, B, form, FIDS[B])


def _epilogue_body(make_rig, form):
    """shared with tests/test_gpu_arm_front_back.py.
    loss_out receives the vector and loss is cleared; loss_total += sum loss_w loss within the float32 bound of a 64-term wave sum
    (one rounding per product, six levels of the tree, one for the add: 7 U sum |w l| + U (|total| + |sum|)); sched_row becomes row + 1,
    draw_counter goes up by one; each of them is left alone when its pointer is NULL"""
    from harp_amd import _lib
    _, p, st, ck = _L()
    B = 3
    wide, lean = form.endswith("wide"), form.startswith("lean")
    rig = make_rig(B)
    cot, pre, g_colors = _cot(rig)
    rig.d.t.update({k: _d(v) for k, v in cot.items()})
    gcd = _d(g_colors)
    rig.run_front("wide" if wide else "one", form)
    g = _gen(77)
    loss0, w = torch.randn(64, generator=g), torch.randn(64, generator=g)
    sched = _d(torch.tensor(SCHED[B], dtype=torch.int32))
    for n_loss in (0, 9, 64):
        for null in (None, "loss_out", "loss_w", "loss_total", "schedule", "draw_counter", "loss"):
            tag = f"epilogue {form} n_loss={n_loss} NULL={null}"
            rig.d.t.update({k: _d(v) for k, v in pre.items()})
            rig.d.t.update(g_v0=torch.empty(B, rig.NV, 3, device=DEV), g_joints_mm=torch.empty(B, rig.NJO, 3, device=DEV))
            loss, out, wd = _d(loss0), torch.full((64,), float("nan"), device=DEV), _d(w)
            total, row, draw = _d(torch.tensor([0.5])), _d(torch.tensor([5], dtype=torch.int32)), _d(torch.tensor([41], dtype=torch.int32))
            on = lambda k, v: None if null == k else p(v)
            step = _lib.StepFrame(schedule=on("schedule", sched), sched_row=p(row), n_rows=2, loss=on("loss", loss), loss_out=on("loss_out", out), n_loss=n_loss,
                                  draw_counter=on("draw_counter", draw), loss_w=on("loss_w", wd), loss_total=on("loss_total", total))
            ck(rig.back(wide, rig.hand(shadow=1, ng=1, light_only=int(lean), step=step), gcd), tag)
            torch.cuda.synchronize()
            live = null != "loss"
            want_loss = loss0.clone()
            if live:
                want_loss[:n_loss] = 0
            assert torch.equal(_bits(loss.cpu()), _bits(want_loss)), tag
            want_out = torch.full((64,), float("nan"))
            if live and null != "loss_out":
                want_out[:n_loss] = loss0[:n_loss]
            assert torch.equal(_bits(out.cpu()), _bits(want_out)), tag
            if null in ("loss_w", "loss_total"):
                assert total.cpu().tolist() == [0.5], tag
            else:
                terms = (w[:n_loss].double() * loss0[:n_loss].double()) if live else torch.zeros(0, dtype=torch.float64)
                want, mag = 0.5 + terms.sum().item(), terms.abs().sum().item()
                bound = 7 * U * mag + U * (0.5 + abs(terms.sum().item()))
                err = abs(total.cpu().double().item() - want)
                print(f"[{tag}] loss_total err {err:.3e} bound {bound:.3e}")
                assert err <= bound and (n_loss == 0 or not live or mag > 0), (tag, err, bound)
                if n_loss == 0 or not live:
                    assert total.cpu().tolist() == [0.5], tag
            assert row.cpu().tolist() == ([5] if null == "schedule" else [5 % 2 + 1]), tag
            assert draw.cpu().tolist() == ([41] if null == "draw_counter" else [42]), tag


@pytest.mark.parametrize("form", ["one_wg", "wide", "lean_one_wg", "lean_wide"])
def test_back_epilogue_turns_the_step_over(form):
    _epilogue_body(_Rig, form)


# ----------------------------------------------------------------------------------------------------------------------------------
# argument checks: refused on the host, nothing written
# ----------------------------------------------------------------------------------------------------------------------------------
CHAIN_FWD = ("edges0", "vf_off", "vf_tri", "disp", "verts_mm", "joints_mm", "joints_m", "vs", "n1", "il1", "vd", "n2", "il2", "ndc_c", "centroid", "light_R",
             "light_T", "ndc_l")
CHAIN_BWD = ("vf_off", "vf_tri", "disp", "sub_off", "sub_idx", "vd", "vs", "n1", "il1", "cam_R", "cam_T", "g_vd", "g_ndc_c", "g_joints_m", "g_joints_mm", "g_v0",
             "g_cam_T", "g_disp", "n2", "il2", "g_n2", "light_pos", "centroid", "light_R", "light_T", "g_ndc_l", "g_light_R", "g_light_T", "g_light_pos")


class _Refusals:
    """the "refused, untouched" harness, shared with tests/test_gpu_arm_front_back.py: every buffer a rig's entry points could write is
    filled with 5.0 (the integer ones keep their values) and watched; refused() breaks one rule in a fresh struct and wants
    HARP_ERR_ARG from every call; verify() wants every watched bit as it was"""

    def __init__(self, rig, B, scratch):
        self.rig = rig
        for k, v in _cotangents(rig.cs).items():
            rig.d.t[k] = _d(v)
        for k, s in (("g_v0", (B, rig.NV, 3)), ("g_joints_mm", (B, rig.NJO, 3)), ("g_light_pos", (B, 3)), ("g_cam_T", (B, 3)), ("g_disp", (rig.cs["V"],))):
            rig.d.t[k] = torch.full(s, 5.0, device=DEV)
        for k in list(FWD_SHAPES) + ["verts_mm", "joints_mm"]:
            rig.d.t[k].fill_(5.0)
        for v in list(rig.rows.values()) + [rig.colors, rig.lbs_ws, rig.part_ws] + list(scratch.values()):
            v.fill_(5.0)
        self.loss, self.total = torch.full((64,), 5.0, device=DEV), torch.full((1,), 5.0, device=DEV)
        self.row, self.tfid = _d(torch.tensor([1], dtype=torch.int32)), _d(torch.tensor([9], dtype=torch.int32))
        self.sched = _d(torch.tensor(SCHED[B], dtype=torch.int32))
        self.gcd = torch.full((9,), 5.0, device=DEV)
        self.watched = dict(rig.d.t, **{"row_" + k: v for k, v in rig.rows.items()}, **{"g_tb_" + k: v for k, v in rig.g_tb.items()}, colors=rig.colors,
                            lbs_ws=rig.lbs_ws, part_ws=rig.part_ws, loss=self.loss, total=self.total, row=self.row, tfid=self.tfid, fid=rig.fid, **scratch)
        self.before = {k: v.clone() for k, v in self.watched.items()}
        self.tried = 0

    def hand(self, chain=None, top=None, tables=None, step=None, model=None, model_field="mano"):
        h = self.rig.hand(shadow=1, ng=1, step=step)
        for k, v in (chain or {}).items():
            setattr(h.chain, k, v)
        for k, v in (top or {}).items():
            setattr(h, k, v)
        for k, v in (tables or {}).items():
            setattr(h.tables, k, v)
        for k, v in (model or {}).items():
            setattr(getattr(h, model_field), k, v)
        return h

    def refused(self, calls, what, **kw):
        for name, call in calls.items():
            assert call(self.hand(**kw)) == 1, (name, what)
            self.tried += 1

    def verify(self):
        torch.cuda.synchronize()
        for k, v in self.watched.items():
            assert torch.equal(_bits(v), _bits(self.before[k])), k


def test_fused_front_and_back_refuse_bad_arguments_untouched():
    """every rule of hand_ok, hand_rows_ok, chain_fwd_ok / chain_bwd_ok, step_ok and the forms' own (scratch, size limits) broken one at a
    time: HARP_ERR_ARG before any launch, with real buffers, and nothing is written.  (The hybrid front leaves the chain's own pointers to
    harp_mesh_chain_fwd, behind its first launch: only the rules it checks itself are tried on it.)"""
    from harp_amd import _lib
    L, p, st, ck = _L()
    B = 1
    rig = _Rig(B)
    rf = _Refusals(rig, B, dict(g_betas=rig.g_betas))
    hand, refused = rf.hand, rf.refused
    loss, total, row, tfid, sched, gcd = rf.loss, rf.total, rf.row, rf.tfid, rf.sched, rf.gcd

    fronts = {f: (lambda h, f=f: rig.front(f, h)) for f in FRONTS}
    backs = {"one_wg": lambda h: rig.back(False, h, gcd), "wide": lambda h: rig.back(True, h, gcd)}
    every = dict(fronts, **backs)
    # ---- hand_ok: all five entry points
    for over in (dict(B=0), dict(B=-1), dict(V0=777), dict(V0=779), dict(E0=-1), dict(NJ=20), dict(NJ=22)):
        refused(every, over, chain=over)
    for k in ("fid", "pose48", "lbs_ws"):
        refused(every, k, top={k: None})
    refused(every, "wrist_pose", tables=dict(wrist_pose=p(rig.tb["rot"])))
    null = ctypes.POINTER(_lib.HandFront)()
    assert L.harp_hand_front_fwd(null, st()) == 1 and L.harp_hand_front_wide_fwd(null, p(rig.part_ws), st()) == 1 and L.harp_hand_front_hybrid_fwd(null, st()) == 1
    assert L.harp_hand_back_bwd(null, p(gcd), p(rig.g_betas), st()) == 1 and L.harp_hand_back_wide_bwd(null, p(gcd), p(rig.g_betas), p(rig.part_ws), st()) == 1
    # ---- hand_rows_ok: the three fronts
    for k in ("betas", "trans_b", "cam_R", "cam_T", "light_pos", "colors"):
        refused(fronts, k, top={k: None})
    # ---- chain_fwd_ok: the one-workgroup and the wide front; what the hybrid front checks itself
    for k in CHAIN_FWD:
        refused({f: fronts[f] for f in ("one", "wide")}, k, chain={k: None})
    for k in ("verts_mm", "joints_mm"):
        refused({"hybrid": fronts["hybrid"]}, k, chain={k: None})
    # ---- chain_bwd_ok: both backs (edges0: the one-workgroup back only)
    for k in CHAIN_BWD:
        refused(backs, k, chain={k: None})
    refused({"one_wg": backs["one_wg"]}, "edges0", chain=dict(edges0=None))
    # ---- size limits: one vertex past harp_mesh_chain_max_vertices() (one workgroup), where also (V + 3) / 4 > 1024 (the wide forms; their
    #      LDS limits lie above it and are never the first to refuse)
    assert L.harp_mesh_chain_max_vertices() == 4096
    refused({"one": fronts["one"], "wide": fronts["wide"], "back one_wg": backs["one_wg"], "back wide": backs["wide"]}, "V = 4097", chain=dict(E0=4097 - NV))
    # ---- step_ok
    ok_sched = dict(schedule=p(sched), sched_row=p(row), n_rows=2, tfid_out=p(tfid))
    for bad in (dict(ok_sched, sched_row=None), dict(ok_sched, n_rows=0), dict(ok_sched, n_rows=-1)):
        refused(every, bad, step=_lib.StepFrame(**bad))
    for k in ("g_vd", "g_joints_m"):
        refused(fronts, "clear without " + k, step=_lib.StepFrame(clear_mesh_grads=1), chain={k: None})
    for n in (65, -1):
        refused(backs, f"n_loss = {n}", step=_lib.StepFrame(loss=p(loss), loss_out=p(loss), n_loss=n, loss_total=p(total), loss_w=p(loss)))
    # ---- the forms' scratch
    h = hand()
    assert L.harp_hand_front_wide_fwd(ctypes.byref(h), None, st()) == 1
    assert L.harp_hand_back_wide_bwd(ctypes.byref(h), p(gcd), p(rig.g_betas), None, st()) == 1
    assert L.harp_hand_back_bwd(ctypes.byref(h), p(gcd), None, st()) == 1 and L.harp_hand_back_wide_bwd(ctypes.byref(h), p(gcd), None, p(rig.part_ws), st()) == 1
    lean = hand(chain=dict(light_only=1))
    assert L.harp_hand_back_wide_bwd(ctypes.byref(lean), p(gcd), p(rig.g_betas), None, st()) == 1                 # (before it forwards the lean form)
    assert L.harp_hand_back_wide_bwd(ctypes.byref(lean), p(gcd), None, p(rig.part_ws), st()) == 1
    assert rf.tried > 150
    rf.verify()
