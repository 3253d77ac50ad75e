"""tests/_fragment_ref.py (what tests/test_gpu_fragment_paths.py builds its bounds from) anchored on the oracle, and the cases of that GPU
test checked on the reference alone — no GPU.

Anchor: gradient() — P._pair_eval on the gathered face vertices of the oracle's pix_to_face — gives the autograd gradient through
oracle/p3d_like.rasterize_meshes itself to 1e-12 relative, for each cotangent alone and all three; its per-pair shares add up to it.
Conditions, on every case: the path the case is for is reached, at most 2 % of its covered pixels are undecided for every (K, blur) it runs
with (and the undecided mask does flag an edge through pixel centres, a band edge on them and a near-tie in depth, but not duplicates), and the float32 evaluation of the oracle picks the same face in every slot of every decided pixel (so E32 is defined on all of them)."""
import pytest
import torch

from tests import _fragment_cases as C
from tests import _fragment_ref as Fr

F64 = torch.float64


@pytest.fixture(scope="module")
def built():
    cases = {}

    def get(name):
        if name not in cases:
            cases[name] = C.build(name)
        return cases[name]
    yield get
    cases.clear()


@pytest.mark.parametrize("name", C.CASES)
def test_case_conditions_on_the_reference(name, built):
    c = built(name)
    C.conditions(c)
    for K, blur in C.runs(c):
        e = Fr.e32(c, K, blur)
        print(f"[{name} K={K} blur={blur:.3g}] E32 zbuf {e['zbuf']:.2e} bary {e['bary']:.2e} dists {e['dists']:.2e}")
        assert e["same_faces"], (name, K, blur)
        ref = Fr.reference(c, K, blur)
        filled = ref["p2f"] >= 0
        assert (filled[..., 1:] <= filled[..., :-1]).all()                # filled slots first
        for k in Fr.OUTPUTS:
            assert (ref[k][~filled] == -1).all()


@pytest.mark.parametrize("name,K,which", [("band", 4, 0), ("band", 1, 1), ("ties", 4, 0), ("nearplane", 2, 1), ("culled", 2, 0)])
def test_gradient_matches_autograd_through_the_oracle(name, K, which, built):
    from oracle import p3d_like as P
    c = built(name)
    blur = c["blurs"][which]
    ref = Fr.reference(c, K, blur)
    leaf = c["ndc"].double().requires_grad_()
    p2f, z, b, d = P.rasterize_meshes(leaf, c["faces"], c["S"], blur, K)
    g = torch.Generator().manual_seed(7)
    cots = dict(g_zbuf=torch.randn(z.shape, generator=g, dtype=F64), g_bary=torch.randn(b.shape, generator=g, dtype=F64),
                g_dists=torch.randn(d.shape, generator=g, dtype=F64))
    m = (p2f >= 0).double()
    terms = dict(g_zbuf=(z * cots["g_zbuf"] * m).sum(), g_bary=(b * cots["g_bary"] * m[..., None]).sum(), g_dists=(d * cots["g_dists"] * m).sum())
    for keys in (("g_zbuf",), ("g_bary",), ("g_dists",), ("g_zbuf", "g_bary", "g_dists")):
        want, = torch.autograd.grad(sum(terms[k] for k in keys), leaf, retain_graph=True)
        st = Fr.gradient(c, ref["p2f"], blur, **{k: cots[k] for k in keys})
        assert want.abs().max() > 0
        assert (st["ref"] - want).abs().max() <= 1e-12 * want.abs().max(), keys
        assert (st["A"] + 1e-300 >= st["ref"].abs() * (1 - 1e-9)).all() and st["M"] <= st["A"].max() and (st["N"][st["A"].sum(-1) > 0] >= 1).all()
    none = Fr.gradient(c, ref["p2f"], blur)
    assert none["M"] == 0.0 and (none["ref"] == 0).all()


def test_undecided_flags_what_it_should():
    S = 8
    yc = 1.0 - 7.0 / S                                                    # the centres of pixel row 3: exact in float32
    tri = [[-0.71, yc, 1.5], [0.73, yc, 1.6], [0.03, 0.93, 1.7]]
    far = [[x, y, z * (1.0 + 2.0 ** -22)] for x, y, z in tri]
    mk = lambda tris: dict(name="probe", S=S, B=1, ndc=torch.tensor(tris, dtype=F64).reshape(1, -1, 3).float(), faces=torch.arange(3 * len(tris)).reshape(-1, 3))
    one = mk([tri])
    und = Fr.undecided(one, 1, 0.0)
    assert und[0, 3].any() and not und[0, :3].any() and not und[0, 4:].any()        # the edge through the row's centres
    r = 2.0 / S                                                           # a band that ends exactly on the centres of row 4
    und = Fr.undecided(one, 1, Fr.f32(r * r))
    assert und[0, 4].any() and not und[0, 3].any()
    dup, near = mk([tri, tri]), mk([tri, far])
    inside = Fr.pairs(one, 0.0)["inside"][0, 0] & ~Fr.undecided(one, 1, 0.0)[0]
    assert inside.any()
    assert not Fr.undecided(dup, 1, 0.0)[0][inside].any() and Fr.undecided(near, 1, 0.0)[0][inside].all()
    assert not Fr.undecided(near, 1, 0.0)[0][~Fr.covered(near, 0.0)[0] & ~Fr.undecided(one, 1, 0.0)[0]].any()
