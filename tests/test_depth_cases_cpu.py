"""tests/_depth_cases.py (the float64 reference tests/test_gpu_depth_bwd_paths.py holds the depth map's backward to) anchored on the oracle,
and the cases of that GPU test checked on the reference alone — no GPU.

Anchor, on frame 0 of every case (B = 1): the nearest face per decided pixel is oracle/p3d_like.rasterize_meshes' (K = 1, no blur), the depth
agrees to 1e-12, and the gradient of sum(cot * zbuf) equals autograd through the oracle's zbuf to 1e-12 relative.  Conditions, on every case
at full size: at most 2 % of the covered pixels undecided, at least 200 covered pixels with a non-zero cotangent, the case's own edge reached;
the float32 rasterisation finds the same face on every decided pixel; A_i bounds |ref_i|; the float32 evaluation of the gradient stays within
1e-3 of the float64 one's largest entry (E32 of the GPU test's bound is a yardstick only while it is small against the gradient itself)."""
import pytest
import torch

from tests import _depth_cases as D

F64 = torch.float64


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            c = D.build(name)
            cache[name] = (c, D.raster(c))
        return cache[name]
    yield get
    cache.clear()


@pytest.mark.parametrize("name", D.CASES)
def test_zbuf_gradient_matches_the_oracle(name, built):
    from oracle import p3d_like as P
    c = D.frame(built(name)[0])
    S, F = c["S"], c["faces"].shape[0]
    ras = D.raster(c)
    cot = D.cotangent(c, ras)
    leaf = c["ndc"].double().requires_grad_()
    p2f, zbuf, _, _ = P.rasterize_meshes(leaf, c["faces"], S, blur_radius=0.0, faces_per_pixel=1)
    want_id = torch.where(p2f[..., 0] >= 0, p2f[..., 0] % F, p2f[..., 0])
    keep = ~ras["undecided"]
    assert torch.equal(ras["face_id"][keep], want_id[keep])
    zb = zbuf[..., 0].detach()
    assert ((ras["z"] - zb).abs() <= 1e-12 * zb.abs())[keep].all()
    want, = torch.autograd.grad((zbuf[..., 0] * cot.double() * (p2f[..., 0] >= 0)).sum(), leaf)
    got = D.zbuf_gradient(c, ras["face_id"], cot)
    worst = (got["ref"] - want).abs().max().item() / want.abs().max().item()
    print(f"[{name}] zbuf gradient against the oracle: {worst:.2e} relative, {int((cot != 0).sum())} pixels")
    assert want.abs().max() > 0 and worst <= 1e-12
    assert (got["A"] + 1e-300 >= got["ref"].abs() * (1 - 1e-9)).all()


@pytest.mark.parametrize("name", D.CASES)
def test_case_conditions_on_the_reference(name, built):
    c, ras = built(name)
    cot = D.cotangent(c, ras)
    D.conditions(c, ras["face_id"], cot, ras["undecided"])
    r32 = D.raster(c, dtype=torch.float32)
    keep = ~ras["undecided"]
    assert torch.equal(ras["face_id"][keep], r32["face_id"][keep])
    r = D.reference(c, ras["face_id"], cot)
    print(f"[{name}] E32 {r['E32']:.2e}, max |ref| {r['ref'].abs().max().item():.2e}, max A {r['A'].max().item():.2e}")
    assert (r["A"] + 1e-300 >= r["ref"].abs() * (1 - 1e-9)).all() and r["E32"] <= 1e-3 * r["ref"].abs().max().item()
