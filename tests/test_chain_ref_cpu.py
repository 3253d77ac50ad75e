"""CPU: tests/_chain_ref.py, the float64 reference the fused mesh chain is held to (tests/test_gpu_mesh_chain.py), is itself checked: it
reproduces the oracle's own sequence on the hand template, and its autograd passes gradcheck on a small mesh with a general rotation."""
import numpy as np
import torch

from tests import _chain_ref as C

F64 = torch.float64
FIVE = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [1, 5, 2]], np.int64)      # a fan + one face off its rim: 6 vertices


def test_reference_reproduces_the_oracle_sequence_on_the_hand_template():
    from harp_amd import synth
    from oracle import harp_ref as H
    from oracle import p3d_like as P
    tpl = synth.load_template("hand")
    tp = synth.build_topology(tpl["faces0"], 778)
    topo = {"edges0": torch.from_numpy(tp["edges0"]).long(), "faces": torch.from_numpy(tp["faces"]).long()}
    model = {k: torch.from_numpy(v).to(F64) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in synth.make_mano_model(tpl, seed=0).items()}
    g = torch.Generator().manual_seed(3)
    T, S, focal = 4, 100, 446.4
    V = tp["n_verts"]
    params = dict(pose=torch.randn(T, 45, generator=g, dtype=F64) * 0.2, rot=torch.randn(T, 3, generator=g, dtype=F64) * 0.3,
                  trans=torch.randn(T, 3, generator=g, dtype=F64) * 0.02, shape=torch.randn(10, generator=g, dtype=F64) * 0.4,
                  verts_disps=torch.randn(V, 1, generator=g, dtype=F64) * 1e-3)
    cam = torch.tensor([[1.1, 0.02, -0.03]], dtype=F64).repeat(T, 1) + torch.randn(T, 3, generator=g, dtype=F64) * 0.01
    light = torch.randn(T, 3, generator=g, dtype=F64) * 0.5 + torch.tensor([0.2, -0.9, -0.4], dtype=F64)
    fid = torch.tensor([2, 0, 2])
    B = fid.shape[0]
    # ---- the oracle's sequence
    joints, verts = H.prepare_mesh(params, fid, model, topo)
    light_R, light_T, cam_R, cam_T = H.process_info_for_shadow(cam[fid], light[fid], verts.mean(1), S, focal)
    pp = (S / 2.0, S / 2.0)
    ndc_c = P.world_to_ndc(verts, cam_R, cam_T, focal, pp, S)[1]
    ndc_l = P.world_to_ndc(verts, light_R, light_T, focal, pp, S)[1]
    n2 = P.verts_normals(verts, topo["faces"])
    # ---- the reference, from the hand layer's millimetres
    verts_mm, joints_mm = H.mano_forward(model, torch.cat((params["rot"][fid], params["pose"][fid]), 1), params["shape"].repeat([B, 1]),
                                         params["trans"][fid])
    out = C.chain(verts_mm, joints_mm, cam_R, cam_T, light[fid], params["verts_disps"][:, 0], topo["edges0"], topo["faces"], S, focal)
    assert set(out) == set(C.FWD_KEYS)
    # v / 1000.0 and v * 1e-3 differ by one float64 rounding; everything after is the same sequence of operations
    for k, want in (("joints_m", joints), ("vd", verts), ("n2", n2), ("ndc_c", ndc_c), ("centroid", verts.mean(1)), ("light_R", light_R),
                    ("light_T", light_T), ("ndc_l", ndc_l)):
        err = (out[k] - want).abs().max().item()
        print(f"[chain_ref vs oracle] {k}: {err:.3e}")
        assert err < 1e-11, (k, err)
    assert out["vs"].shape == (B, V, 3) and torch.equal(out["vs"][:, :778], verts_mm * 1e-3)
    # il = 1 / |N| of the un-normalised normal, 0 under the clamp (a few vertices between the fingers of a posed hand get there:
    # the template's smallest |N| is 6e-6)
    for k in ("il1", "il2"):
        assert (out[k] >= 0).all() and (out[k] > 0).double().mean() > 0.99 and out[k].max() <= 1e6
    vs_n = P.verts_normals(out["vs"], topo["faces"])
    assert torch.equal(out["n1"], vs_n) and torch.allclose(out["vd"], out["vs"] + vs_n * params["verts_disps"][None, :, 0, None], rtol=0, atol=1e-15)


def test_reference_passes_gradcheck_on_the_five_mesh():
    from harp_amd import synth
    tp = synth.build_topology(FIVE, 6)
    edges0, faces = torch.from_numpy(tp["edges0"]).long(), torch.from_numpy(tp["faces"]).long()
    V = tp["n_verts"]
    assert V == 16                                   # 6 vertices + 10 edge midpoints
    g = torch.Generator().manual_seed(4)
    P0 = torch.tensor([(0, 0, 1), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (1, 1, -0.5)], dtype=F64)
    B, S, focal = 2, 97, 433.0
    verts_mm = (40.0 * P0[None] + torch.randn(B, 6, 3, generator=g, dtype=F64) * 4.0 + torch.tensor([10.0, -20.0, 450.0], dtype=F64)).requires_grad_()
    joints_mm = (torch.randn(B, 2, 3, generator=g, dtype=F64) * 50).requires_grad_()
    cam_R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, dtype=F64))[0]
    cam_R[0] = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=F64))
    centre = (verts_mm.detach() * 1e-3).mean(1)
    # cam_T puts the mesh 0.5 m in front of the camera whatever the rotation
    cam_T = (torch.tensor([0.01, -0.02, 0.5], dtype=F64) - torch.bmm(centre[:, None], cam_R)[:, 0]).requires_grad_()
    light_pos = (centre + torch.tensor([[0.4, -0.8, -0.3], [-0.5, 0.6, 0.4]], dtype=F64)).requires_grad_()
    disp = (torch.randn(V, generator=g, dtype=F64) * 1e-3).requires_grad_()
    keys = [k for k in C.FWD_KEYS if k not in ("il1", "il2")]                    # the saved inverse lengths are not differentiable outputs

    def f(v, j, t, lp, d):
        out = C.chain(v, j, cam_R, t, lp, d, edges0, faces, S, focal)
        assert (out["il1"] > 0).all() and (out["il2"] > 0).all() and out["ndc_c"][..., 2].min() > 0.3
        return tuple(out[k] for k in keys)
    assert torch.autograd.gradcheck(f, (verts_mm, joints_mm, cam_T, light_pos, disp), eps=1e-6, atol=1e-6, rtol=1e-5)
