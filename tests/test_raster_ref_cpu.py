"""tests/_raster_ref.py (the float64 restatement tests/test_gpu_raster_paths.py holds the tile rasteriser to) anchored on the oracle, and the
cases of that GPU test checked on the reference alone — no GPU.

Anchor, on three cases: against oracle/p3d_like.rasterize_meshes with K = 1 and no blur the nearest face per pixel is identical and the depth
agrees to 1e-12; against rasterize_meshes with the blur radius and K = the largest candidate count + sigmoid_alpha_blend, alpha and the
autograd gradient of sum(g * alpha) agree to 1e-12 relative.  Conditions, on every case: the path the case is for is reached (candidate
counts per tile / super-tile / pixel, face ids in the last bitmap words, culled faces, empty frames ...) and at most 2 % of its covered pixels
are undecided; the float32 evaluation of the restatement finds the same face on every decided pixel."""
import pytest
import torch

from tests import _raster_cases as C
from tests import _raster_ref as R

F64 = torch.float64


@pytest.fixture(scope="module")
def refs():
    built = {}

    def get(name):
        if name not in built:
            c = C.build(name)
            built[name] = (c,) + C.references(c)
        return built[name]
    yield get
    built.clear()


@pytest.mark.parametrize("name", ["one_face", "fan", "layers"])
def test_restatement_matches_the_oracle(name, refs):
    from oracle import p3d_like as P
    c, hard, soft = refs(name)
    B, S, F = c["B"], c["S"], c["faces"].shape[0]
    ndc = c["ndc"].double()
    p2f, zbuf, _, _ = P.rasterize_meshes(ndc, c["faces"], S, blur_radius=0.0, faces_per_pixel=1)
    want = torch.where(p2f[..., 0] >= 0, p2f[..., 0] % F, p2f[..., 0])
    assert torch.equal(R.dense(hard, "face_id", -1), want)
    z = R.dense(hard, "z", -1.0)
    assert ((z - zbuf[..., 0]).abs() <= 1e-12 * zbuf[..., 0].abs()).all()
    K = int(soft["ncand"].max())
    leaf = ndc.clone().requires_grad_()
    p2f, _, _, dists = P.rasterize_meshes(leaf, c["faces"], S, blur_radius=c["blur"], faces_per_pixel=K)
    assert int((p2f >= 0).sum(-1).max()) == K                           # no candidate beyond the cap
    assert torch.equal((p2f >= 0).sum(-1), R.dense(soft, "ncand", 0))
    alpha = P.sigmoid_alpha_blend(p2f, dists, c["sigma"])
    got = R.dense(soft, "alpha", 0.0)
    assert ((got - alpha.detach()).abs() <= 1e-12 * alpha.detach().abs()).all()
    g = torch.rand(B, S, S, generator=torch.Generator().manual_seed(3), dtype=F64) - 0.3
    want_g, = torch.autograd.grad((alpha * g).sum(), leaf)
    st = R.silhouette_gradient(soft, g)
    assert want_g.abs().max() > 0 and (st["ref"][..., 2] == 0).all()
    assert (st["ref"] - want_g).abs().max() <= 1e-12 * want_g.abs().max()
    # the per-pair shares add up to the gradient, and N / A / M describe them
    assert (st["A"] + 1e-300 >= st["ref"].abs() * (1 - 1e-9)).all() and st["M"] <= st["A"].max() and (st["N"][st["A"].sum(-1) > 0] >= 1).all()


@pytest.mark.parametrize("name", C.CASES + C.WORKLOAD)
def test_case_conditions_on_the_reference(name, refs):
    c, hard, soft = refs(name)
    C.conditions(c, hard, soft)
    # float32 evaluation: same nearest face and same candidates on the decided pixels
    h32 = R.rasterize(c["ndc"], c["faces"], c["S"], dtype=torch.float32)
    S, B = c["S"], c["B"]
    und = torch.zeros(B * S * S, dtype=torch.bool)
    und[hard["pix"][hard["undecided"]]] = True
    und[hard["undecided_uncovered"]] = True
    a = torch.full((B * S * S,), -1, dtype=torch.long)
    b = a.clone()
    a[hard["pix"]] = hard["face_id"]
    b[h32["pix"]] = h32["face_id"]
    assert torch.equal(a[~und], b[~und])
