"""CPU: tests/_front_ref.py, the float64 composition the fused MANO front and back are held to (tests/test_gpu_step_front_back.py), is itself
checked: it is the three pinned pieces called one after another, its autograd agrees with central differences, and its gradient rows add up
over a repeated frame and over the shared light the way the table scatter of the fused back has to.  The same for the SMPL-X arm
composition (tests/test_gpu_arm_front_back.py), whose skinning layer tests/_tree_ref.tree_forward is first held to the oracle's arm layer,
and whose tables are held to the input condition of the float64 comparison: no vertex normal within a factor 2 of the 1e-6 clamp."""
import functools

import torch

from tests import _chain_ref as C
from tests import _front_ref as R

F64 = torch.float64
FID = torch.tensor([4, 4, 0, 6, 4])                        # one frame three times, rows 1, 2, 3, 5 absent


@functools.lru_cache(maxsize=None)
def _setup():
    from harp_amd import synth
    from tests.test_gpu_mesh_chain import _case, _cotangents
    model = synth.make_mano_model(seed=0)
    cs = _case("mano", 1)                                  # the MANO template's tables (host side only)
    B = FID.shape[0]
    cot = {k: v.double() for k, v in _cotangents(dict(cs, B=B, vertical=None)).items()}
    return dict(m64=R.mano_model(model), edges0=torch.from_numpy(cs["edges0_np"]).long(), faces=torch.from_numpy(cs["faces_np"]).long(),
                tb={k: v.double() for k, v in R.case_tables(model).items()}, disp=cs["disp"].double(), cot=cot,
                g_colors=torch.randn(9, generator=torch.Generator().manual_seed(5), dtype=F64))


def _front(s, tb, fid, disp, share_light=0, self_shadow=1):
    return R.front(tb, fid, disp, s["edges0"], s["faces"], s["m64"], share_light, self_shadow)


def _slot(cot, b):
    return {k: v[b:b + 1] for k, v in cot.items()}


def test_front_is_the_three_pieces_one_after_another_bit_for_bit():
    from oracle import harp_ref as H
    from tests.test_gpu_frame_glue import FOCAL, S, _definition
    s = _setup()
    for share_light, self_shadow in ((0, 1), (1, 0)):
        out = _front(s, s["tb"], FID, s["disp"], share_light, self_shadow)
        d = _definition(s["tb"], FID, False, share_light, self_shadow)
        v, j = H.mano_forward(s["m64"], d["pose48"], d["betas"], d["trans_b"])
        cam_R = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=F64)).repeat(FID.shape[0], 1, 1)
        ch = C.chain(v, j, cam_R, d["cam_T"], d["light_pos"], s["disp"], s["edges0"], s["faces"], S, FOCAL)
        want = dict(d, cam_R=cam_R, verts_mm=v, joints_mm=j, **ch)
        assert set(out) == set(want) == set(R.ROW_KEYS) | {"verts_mm", "joints_mm"} | set(C.FWD_KEYS)
        for k in want:
            assert out[k].dtype == F64 and torch.equal(out[k], want[k]), k
        # the geometry the GPU test's bounds assume: the hand in front of both cameras, (almost) no clamped normal
        assert out["ndc_c"][..., 2].min() > 0.3 and out["ndc_l"][..., 2].min() > 1.0
        assert (out["il1"] == 0).sum() <= 3 and (out["il2"] == 0).sum() <= 3


def test_table_gradients_agree_with_central_differences():
    """Four entries per table (three of rows in FID, chosen by a seeded generator, and one of an absent row, whose gradient and difference
    quotient are both exactly 0) and four of disp, central differences in float64.

    Measured conditioning (this scene, |f| = 1.46): the error of the quotient falls as h^2 down to h = 1e-5 for the tables (worst
    3.2 h^2: a finger joint at angle 1e-5) and, for disp, whose length scale is the 1 mm displacement, as 4e4 h^2 down to h = 1e-7; below
    that the rounding of f takes over (<= 5e-16 / h).  So h = 1e-5 for the tables (truncation <= 3.2e-10, rounding <= 5e-11) and
    h = 1e-7 for disp (4e-10 and 5e-9), and the tolerance is ten times the sum: 4e-9 and 5e-8, absolute; the gradients compared lie
    between 2e-3 and 1 (one finger entry at 2e-9, which the absolute bound covers)."""
    s = _setup()
    f = lambda tb, disp: R.total(_front(s, tb, FID, disp), s["cot"], s["g_colors"])
    g = R.table_grads(s["tb"], s["disp"], f)
    gen = torch.Generator().manual_seed(7)
    pick = lambda n: int(torch.randint(0, n, (1,), generator=gen))
    worst = {}
    for k in R.TABLE_KEYS + ("disp",):
        src = s["disp"] if k == "disp" else s["tb"][k]
        h, tol = (1e-7, 5e-8) if k == "disp" else (1e-5, 4e-9)
        entries = [(r, pick(src.shape[1])) for r in (4, 0, 6, 2)] if src.dim() == 2 else sorted({(pick(src.numel()),) for _ in range(4)})
        for idx in entries:
            vals = []
            for sign in (1.0, -1.0):
                tb, disp = {kk: v.clone() for kk, v in s["tb"].items()}, s["disp"].clone()
                (disp if k == "disp" else tb[k])[idx] += sign * h
                with torch.no_grad():
                    vals.append(f(tb, disp).item())
            fd, an = (vals[0] - vals[1]) / (2 * h), g["g_" + k][idx].item()
            worst[k] = max(worst.get(k, 0.0), abs(fd - an) / tol)
            if src.dim() == 2 and idx[0] == 2:
                assert fd == 0.0 and an == 0.0, (k, idx)                   # a row no frame names
            else:
                assert an != 0.0 and abs(fd - an) <= tol, (k, idx, fd, an)
    print("[front_ref central differences] worst |fd - autograd| / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_a_repeated_frame_gets_the_sum_of_its_slots_and_the_shared_light_everything():
    s = _setup()
    B = FID.shape[0]
    per_row = ("g_pose", "g_rot", "g_trans", "g_cam", "g_light_positions")
    for share_light in (0, 1):
        g = R.table_grads(s["tb"], s["disp"], lambda tb, disp: R.total(_front(s, tb, FID, disp, share_light), s["cot"], s["g_colors"]))
        slots = [R.table_grads(s["tb"], s["disp"], lambda tb, disp, b=b: R.total(_front(s, tb, FID[b:b + 1], disp, share_light), _slot(s["cot"], b)))
                 for b in range(B)]
        for k in per_row:
            for r in range(7):
                if k == "g_light_positions" and share_light:
                    want = sum(sl[k][0] for sl in slots) if r == 0 else torch.zeros(3, dtype=F64)      # row 0 takes the whole sum
                else:
                    want = sum((sl[k][r] for b, sl in enumerate(slots) if int(FID[b]) == r), torch.zeros_like(g[k][r]))
                assert torch.allclose(g[k][r], want, rtol=1e-12, atol=1e-15), (share_light, k, r)
                assert (want.abs().max() > 0) == (r in (0, 4, 6) if not (k == "g_light_positions" and share_light) else r == 0), (k, r)
        # row 4 is three slots: no single slot explains it
        assert all((g["g_pose"][4] - sl["g_pose"][4]).abs().max() > 1e-6 for sl in slots)
        # the tables without rows sum over every slot (the slots' terms of an element may cancel: absolute, on the table's scale)
        for k in ("g_shape", "g_disp"):
            assert torch.allclose(g[k], sum(sl[k] for sl in slots), rtol=0, atol=1e-12 * g[k].abs().max().item()), k


# ----------------------------------------------------------------------------------------------------------------------------------
# SMPL-X arm path: tests/_tree_ref.py and the arm composition of tests/_front_ref.py (tests/test_gpu_arm_front_back.py)
# ----------------------------------------------------------------------------------------------------------------------------------
ARM_MESH = dict(arm="arm", twig="five", crown="hub")
ARM_ROWS = list(range(7))                                    # every table row: the batches and the schedules of the GPU tests name all of them


@functools.lru_cache(maxsize=None)
def _arm_setup(name):
    from harp_amd import synth
    from tests import _tree_ref as TR
    from tests.test_gpu_mesh_chain import _case, _cotangents
    host = TR.host_from_arm(synth.make_smplx_arm_model(seed=0)) if name == "arm" else TR.build_tree(name)
    TR.assert_tree_property(host)
    cs = dict(_case(ARM_MESH[name], 1), NJ=len(host["joint_src"]))
    B = FID.shape[0]
    cot = {k: v.double() for k, v in _cotangents(dict(cs, B=B, vertical=None)).items()}
    return dict(host=host, m64=TR.model64(host), edges0=torch.from_numpy(cs["edges0_np"]).long(), faces=torch.from_numpy(cs["faces_np"]).long(),
                tb={k: v.double() for k, v in R.arm_case_tables(host, 7, **R.ARM_CASE[name]).items()}, disp=cs["disp"].double(), cot=cot,
                g_colors=torch.randn(9, generator=torch.Generator().manual_seed(5), dtype=F64), cs=cs)


def _arm_front(s, tb, fid, disp, share_light=0, self_shadow=1):
    return R.arm_front(tb, fid, disp, s["edges0"], s["faces"], s["m64"], share_light, self_shadow)


def test_tree_forward_is_the_oracle_arm_layer_on_the_production_model():
    """tests/_tree_ref.tree_forward, written from the harp_tree_model contract, against oracle.harp_ref.smplxarm_forward (restated from
    smplx.lbs): outputs and the autograd gradients of all inputs, the ten expression coefficients included, to 1e-12 relative, both float64"""
    from harp_amd import synth
    from oracle import harp_ref as H
    from tests import _tree_ref as TR
    m = synth.make_smplx_arm_model(seed=0)
    mt = {k: torch.from_numpy(v).double() if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in m.items()}
    m64 = TR.model64(TR.host_from_arm(m))
    g = torch.Generator().manual_seed(3)
    B = 3
    in_pose = torch.randn(B, 17, 3, generator=g, dtype=F64) * 0.5
    betas, transl = torch.randn(B, 20, generator=g, dtype=F64), torch.randn(B, 3, generator=g, dtype=F64) * 0.05
    gv, gj = torch.randn(B, 1026, 3, generator=g, dtype=F64), torch.randn(B, 22, 3, generator=g, dtype=F64)
    a = [t.clone().requires_grad_() for t in (in_pose, betas, transl)]
    v, j = TR.tree_forward(m64, *a)
    ga = torch.autograd.grad((v * gv).sum() + (j * gj).sum(), a)
    b = [t.clone().requires_grad_() for t in (betas[:, :10], in_pose[:, 0], transl, in_pose[:, 2:].reshape(B, 45), in_pose[:, 1], betas[:, 10:])]
    v2, j2 = H.smplxarm_forward(mt, *b[:5], expression=b[5])
    gb = torch.autograd.grad((v2 * gv).sum() + (j2 * gj).sum(), b)
    rel = lambda x, y: ((x - y).norm() / y.norm()).item()
    want_pose = torch.cat([gb[1][:, None], gb[4][:, None], gb[3].view(B, 15, 3)], 1)
    errs = dict(verts=rel(v, v2), joints=rel(j, j2), g_in_pose=rel(ga[0], want_pose), g_betas=rel(ga[1], torch.cat([gb[0], gb[5]], 1)), g_transl=rel(ga[2], gb[2]))
    print("[tree_forward against smplxarm_forward] " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert all(e <= 1e-12 for e in errs.values()) and gb[5].abs().min() > 0, errs


def test_arm_front_is_its_three_pieces_one_after_another_bit_for_bit():
    from tests import _tree_ref as TR
    from tests.test_gpu_frame_glue import FOCAL, S, _definition
    for name in ("arm", "twig", "crown"):
        s = _arm_setup(name)
        NB = s["m64"]["shapedirs"].shape[-1]
        for share_light, self_shadow in ((0, 1), (1, 0)):
            out = _arm_front(s, s["tb"], FID, s["disp"], share_light, self_shadow)
            d = _definition(s["tb"], FID, True, share_light, self_shadow)
            d["pose_in"] = d.pop("pose48")
            assert d["betas"].shape[1] == 20 and (d["betas"][:, 10:] == 0).all()
            d["betas"] = torch.cat([d["betas"][:, :10], torch.zeros(FID.shape[0], NB - 10, dtype=F64)], 1)
            v, j = TR.tree_forward(s["m64"], d["pose_in"].view(-1, 17, 3), d["betas"], d["trans_b"])
            cam_R = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=F64)).repeat(FID.shape[0], 1, 1)
            ch = C.chain(v, j, cam_R, d["cam_T"], d["light_pos"], s["disp"], s["edges0"], s["faces"], S, FOCAL)
            want = dict(d, cam_R=cam_R, verts_mm=v, joints_mm=j, **ch)
            assert set(out) == set(want) == set(R.ARM_ROW_KEYS) | {"verts_mm", "joints_mm"} | set(C.FWD_KEYS)
            for k in want:
                assert out[k].dtype == F64 and torch.equal(out[k], want[k]), (name, k)
            # the geometry the GPU test's bounds assume: the mesh in front of both cameras
            assert out["ndc_c"][..., 2].min() > 0.3 and out["ndc_l"][..., 2].min() > 1.0, name


def test_arm_tables_hold_every_edge_angle_and_keep_the_normals_clear_of_the_clamp():
    """(a) every value of ANGLES occurs on a finger row and, between them, on the two arm rows (root and wrist: seven table rows cannot hold
    nine values on one joint; the root takes 0, 1e-7, 1e-5, pi - 1e-3, pi + 1e-3, 3 pi, the wrist the other three and four of those again).
    (b) the input condition of the float64 comparison: the clamp n = N / max(|N|, 1e-6) is a discontinuity float32 cannot decide near 1e-6,
    so for every table row, both normal passes and the tests' disp, no vertex has |N| in (0.5e-6, 2e-6) m^2."""
    from tests.test_gpu_building_blocks import _cond
    from tests.test_gpu_geometry_terms import ANGLES
    for name in ("arm", "twig", "crown"):
        s = _arm_setup(name)
        src = s["host"]["pose_src"]
        pm = s["m64"]["pose_mean"][[src.index(r) for r in range(17)]]
        in_pose = torch.cat([s["tb"]["rot"][:, None], s["tb"]["wrist_pose"][:, None], s["tb"]["pose"].view(7, 15, 3)], 1)
        th = (in_pose + pm).norm(dim=-1)                                              # (7,17) the angles the joints take
        # (the tables are float32: the angle of pose + pose_mean is the edge value within the rounding of that sum; exactly 0 where it is 0)
        near = lambda t, a: bool(((t - a).abs() <= 2e-8 + 1e-6 * a).any()) if a > 0 else bool((t == 0).any())
        for a in ANGLES:
            assert near(th[:, 2:], a), (name, "finger", a)
            assert near(th[:, :2], a), (name, "root / wrist", a)
        assert sum(near(th[:, 0], a) for a in ANGLES) >= 6 and sum(near(th[:, 1], a) for a in ANGLES) >= 7, name
        rows = ARM_ROWS
        o = _arm_front(s, s["tb"], torch.tensor(rows), s["disp"])
        for pos in ("vs", "vd"):
            _, Nlen = _cond(o[pos], s["cs"]["faces_np"])
            inside = (Nlen > 0.5e-6) & (Nlen < 2e-6)
            print(f"[clamp margin {name} {pos}] rows {rows}: smallest |N| {Nlen.min().item():.3e}, under the clamp {int((Nlen <= 1e-6).sum())}, "
                  f"within a factor 2 of it {int(inside.sum())}")
            assert not inside.any(), (name, pos, Nlen[inside])


def test_arm_table_gradients_agree_with_central_differences():
    """As test_table_gradients_agree_with_central_differences, on the production arm with wrist_pose among the tables: four entries per
    table (three of rows in FID, one of an absent row: gradient and quotient exactly 0) and four of disp, the same steps and tolerances
    (h = 1e-5 / 4e-9 for the tables, h = 1e-7 / 5e-8 for disp: the scene, the cotangents and |f| are of the same size as the MANO ones)."""
    s = _arm_setup("arm")
    f = lambda tb, disp: R.total(_arm_front(s, tb, FID, disp), s["cot"], s["g_colors"])
    g = R.table_grads(s["tb"], s["disp"], f)
    gen = torch.Generator().manual_seed(7)
    pick = lambda n: int(torch.randint(0, n, (1,), generator=gen))
    worst = {}
    for k in R.ARM_TABLE_KEYS + ("disp",):
        src = s["disp"] if k == "disp" else s["tb"][k]
        h, tol = (1e-7, 5e-8) if k == "disp" else (1e-5, 4e-9)
        entries = [(r, pick(src.shape[1])) for r in (4, 0, 6, 2)] if src.dim() == 2 else sorted({(pick(src.numel()),) for _ in range(4)})
        for idx in entries:
            vals = []
            for sign in (1.0, -1.0):
                tb, disp = {kk: v.clone() for kk, v in s["tb"].items()}, s["disp"].clone()
                (disp if k == "disp" else tb[k])[idx] += sign * h
                with torch.no_grad():
                    vals.append(f(tb, disp).item())
            fd, an = (vals[0] - vals[1]) / (2 * h), g["g_" + k][idx].item()
            worst[k] = max(worst.get(k, 0.0), abs(fd - an) / tol)
            if src.dim() == 2 and idx[0] == 2:
                assert fd == 0.0 and an == 0.0, (k, idx)                   # a row no frame names
            else:
                assert an != 0.0 and abs(fd - an) <= tol, (k, idx, fd, an)
    print("[arm_front central differences] worst |fd - autograd| / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_a_repeated_arm_frame_gets_the_sum_of_its_slots():
    s = _arm_setup("arm")
    B = FID.shape[0]
    g = R.table_grads(s["tb"], s["disp"], lambda tb, disp: R.total(_arm_front(s, tb, FID, disp), s["cot"], s["g_colors"]))
    slots = [R.table_grads(s["tb"], s["disp"], lambda tb, disp, b=b: R.total(_arm_front(s, tb, FID[b:b + 1], disp), _slot(s["cot"], b))) for b in range(B)]
    for k in ("g_pose", "g_rot", "g_wrist_pose", "g_trans", "g_cam", "g_light_positions"):
        for r in range(7):
            want = sum((sl[k][r] for b, sl in enumerate(slots) if int(FID[b]) == r), torch.zeros_like(g[k][r]))
            print(f"[arm slots {k} row {r}] |sum of slots - batch| {(g[k][r] - want).abs().max().item():.2e} of {g[k].abs().max().item():.2e}")
            # (absolute, on the table's scale, as g_shape / g_disp below: the root and the wrist move 4083 vertices at up to 0.4 m, and the
            # terms of an element cancel -- measured 5.9e-15 of 0.16 on g_rot)
            assert torch.allclose(g[k][r], want, rtol=0, atol=1e-12 * g[k].abs().max().item()), (k, r)
            assert (want.abs().max() > 0) == (r in (0, 4, 6)), (k, r)
    assert all((g["g_wrist_pose"][4] - sl["g_wrist_pose"][4]).abs().max() > 1e-6 for sl in slots)      # row 4 is three slots
    for k in ("g_shape", "g_disp"):
        assert torch.allclose(g[k], sum(sl[k] for sl in slots), rtol=0, atol=1e-12 * g[k].abs().max().item()), k
