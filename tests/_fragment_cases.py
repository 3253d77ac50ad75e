"""TEST INFRASTRUCTURE ONLY — the synthetic meshes of tests/test_gpu_fragment_paths.py (given directly as NDC vertices, one per path of
csrc/fragments.hip) and, per case, the conditions that make it force its path, asserted on the float64 reference alone:
tests/test_fragment_ref_cpu.py runs them without a GPU, the GPU tests run them again on the reference they compare with.

  stack      80 quads over one another at distinct depths, face order a different permutation of depth order per frame: the sorted
             insertion with a binding cap (front / middle insertion into a full list, eviction, rejection), K = 64 = the array bound
  ties       six coincident copies of a quad between nearer and farther layers: exact depth ties, the cap inside the tied group
  band       a dozen triangles under a 2.5-pixel blur band (and the workload's): clamp + renormalise, positive dists, vertex regions
  nearplane  z ~ 4e-5: the perspective denominator is clamped at kEps
  needle     an edge shorter than 1e-4 NDC: the degenerate branch of the point-segment distance
  culled     faces behind / straddling the camera plane / collinear among live ones; a frame in which no face survives

Vertex coordinates are decimals that are no multiple of the pixel pitch, so that (nearly) no pixel centre sits within 2^-20 of an edge."""
import numpy as np
import torch

from tests import _fragment_ref as Fr

K_EPS = 1e-8
CASES = ("stack", "ties", "band", "nearplane", "needle", "culled")


def band_blur(S):
    """a band sqrt(blur) of 2.5 pixels"""
    return Fr.f32((2.5 * 2.0 / S) ** 2)


def quad_faces(v0):
    """the two triangles of the quad with vertex rows v0 .. v0 + 3 (counter-clockwise corners)"""
    return [[v0, v0 + 2, v0 + 1], [v0, v0 + 3, v0 + 2]]


def quad(x0, x1, y0, y1, z, tx=0.0, ty=0.0, skew=0.0):
    xy = np.array([[x0, y0 + skew], [x1, y0 - skew], [x1 - skew, y1], [x0 + skew, y1 + skew]])
    return np.concatenate([xy, (z + tx * xy[:, :1] + ty * xy[:, 1:])], 1)


def build(name):
    """dict(name, S, B, ndc (B,V,3) float32, faces (F,3) int64, Ks, blurs [, case-specific entries])"""
    from harp_amd import ops
    extra = {}
    if name == "stack":
        S, nq = 40, 80
        q = np.arange(nq)
        size = np.random.RandomState(11).permutation(nq)
        half = 0.4813 + 0.4391 * size / (nq - 1)                           # 0.48 .. 0.92: 80 candidates at the centre, a few at the rim
        frames = []
        for b, seed in enumerate((3, 4)):
            rank = np.random.RandomState(seed).permutation(nq)             # depth order of the quads: face order is a permutation of it
            cx, cy = 0.0313 * np.sin(1.7 * q + 0.3 + b), 0.0271 * np.cos(2.3 * q + 0.9 - b)
            vs = [quad(cx[i] - half[i], cx[i] + half[i], cy[i] - 0.97 * half[i], cy[i] + 1.03 * half[i], 1.2 + 0.02 * rank[i],
                       0.003 * np.sin(q[i] + 0.5), 0.003 * np.cos(1.3 * q[i]), 0.0173 * np.sin(0.7 * q[i] + b)) for i in range(nq)]
            frames.append(np.concatenate(vs, 0))
        v = np.stack(frames)
        f = np.array([t for i in range(nq) for t in quad_faces(4 * i)])
        Ks, blurs = (1, 5, 64), (0.0,)
    elif name == "ties":
        S = 40
        tied = quad(-0.6317, 0.6689, -0.5923, 0.7117, 1.6, 0.031, -0.023, 0.0137)
        layers = [("near0", quad(-0.8317, 0.3521, -0.7713, 0.8129, 1.1, 0.02, 0.01, 0.011)),
                  ("near1", quad(-0.7131, 0.7919, -0.8537, 0.2311, 1.3, -0.015, 0.02, -0.009)),
                  ("tied_a", tied), ("tied_b", tied.copy()), ("tied_c", tied.copy()),       # three vertex sets with equal coordinates
                  ("far0", quad(-0.9013, 0.9117, -0.8931, 0.9071, 1.9, 0.01, 0.01, 0.007)),
                  ("far1", quad(-0.8719, 0.8833, -0.9127, 0.8891, 2.2, -0.01, 0.02, -0.013)),
                  ("far2", quad(-0.9231, 0.8617, -0.8713, 0.9211, 2.5, 0.02, -0.01, 0.005))]
        v = np.concatenate([m for _, m in layers], 0)[None]
        first = {n: 4 * i for i, (n, _) in enumerate(layers)}
        # quads as face rows: every layer once, and the tied quad six times — tied_a three times (duplicate rows), tied_b twice, tied_c once
        rows = ["near0", "near1", "far0", "far1", "far2", "tied_a", "tied_a", "tied_a", "tied_b", "tied_b", "tied_c"]
        tris = [(n, t) for n in rows for t in quad_faces(first[n])]
        order = np.random.RandomState(5).permutation(len(tris))           # scattered face indices
        f = np.array([tris[i][1] for i in order])
        extra = dict(tied=torch.tensor([k for k, i in enumerate(order) if tris[i][0].startswith("tied")]))
        Ks, blurs = (1, 3, 4, 8), (0.0,)
    elif name == "band":
        S = 72
        yrow = 1.0 - 21.0 / S + 4.1e-4                                     # 4.1e-4 NDC above the centres of pixel row 10 (workload band 9.6e-4)
        tris = [[[-0.5213, -0.4731, 1.8], [0.4917, -0.3829, 2.0], [-0.0317, 0.5123, 1.9]],            # half the image
                [[0.1031, 0.0523, 1.4], [0.3017, 0.4519, 1.5], [0.5531, 0.1213, 1.45]],               # over it, the other winding
                [[0.7219, 0.5817, 1.3], [1.3117, 0.7123, 1.35], [0.8831, 1.1219, 1.4]],               # past +1 in x and y
                [[-0.3013, -0.8017, 1.6], [0.1021, -1.2031, 1.7], [0.2519, -0.7523, 1.65]],           # past -1 in y, across the super-tile row
                [[-0.6217, 0.2013, 1.5], [-0.9519, 0.3521, 1.55], [-0.8523, -0.1017, 1.6]],           # across the 64-pixel super-tile column
                [[0.4424, -0.3909, 1.2], [0.4484, -0.3899, 1.21], [0.4444, -0.3849, 1.22]],           # sub-pixel, around a pixel corner
                [[-0.5298, 0.6647, 1.3], [-0.5238, 0.6657, 1.31], [-0.5258, 0.6707, 1.32]],           # sub-pixel, alone
                [[-0.2013, 0.8017, 1.7], [-0.1619, 0.8313, 1.72], [-0.2117, 0.8521, 1.71]],           # a pixel and a half
                [[-0.3517, -0.3013, 1.2], [-0.2019, 0.1017, 1.25], [-0.1013, -0.3521, 1.22]],         # nearer than the first, the other winding
                [[0.6013, -0.2017, 1.5], [0.9521, -0.6013, 1.6], [0.6219, -0.2313, 1.55]],            # one pixel wide
                [[0.0513, yrow, 1.45], [0.4519, yrow, 1.5], [0.2517, 0.9317, 1.48]],                  # a horizontal edge just above a pixel row
                [[-0.9017, -0.5013, 1.35], [-0.5519, -0.4517, 1.4], [-0.6013, -0.9021, 1.3]]]         # both super-tile edges
        v0 = np.array(tris).reshape(-1, 3)
        v = np.stack([v0, v0 + np.array([0.0371, -0.0293, 0.1])])
        f = np.arange(v0.shape[0]).reshape(-1, 3)
        extra = dict(sub_pixel=(5, 6))
        Ks, blurs = (1, 4), (band_blur(S), Fr.f32(ops.SIL_BLUR))
    elif name == "nearplane":
        S = 40
        tris = [[[-0.7013, -0.6017, 2.1e-5], [0.6519, -0.5013, 5.7e-5], [0.0517, 0.7019, 3.3e-5]],
                [[-0.5017, 0.5013, 4.4e-5], [0.0013, -0.6517, 5.1e-5], [0.5519, 0.6017, 2.6e-5]],
                [[0.2013, -0.1017, 3.0e-5], [0.8017, 0.1013, 3.9e-5], [0.5013, 0.8019, 2.2e-5]]]
        v = np.array(tris).reshape(1, -1, 3)
        f = np.arange(9).reshape(-1, 3)
        Ks, blurs = (2,), (0.0, band_blur(S))
    elif name == "needle":
        S = 40
        tris = [[[-0.6013, 0.3003, 1.5], [-0.60126, 0.30035, 1.5], [0.5517, -0.2013, 1.6]],           # edge 0-1: 6.4e-5 long
                [[0.6019, 0.7013, 1.4], [-0.4517, 0.5519, 1.45], [-0.45173, 0.55194, 1.45]],          # edge 1-2: 5e-5 long, the other winding
                [[-0.3013, -0.4017, 1.7], [0.4019, -0.3013, 1.75], [0.0517, 0.6519, 1.8]]]            # an ordinary face behind both
        v = np.array(tris).reshape(1, -1, 3)
        f = np.arange(9).reshape(-1, 3)
        extra = dict(short=((0, 0, 1), (1, 1, 2)))                          # (face, vertex, vertex) of the short edges
        Ks, blurs = (2,), (band_blur(S),)
    elif name == "culled":
        S = 40
        live = [[[-0.7013, -0.6017, 1.5], [0.3519, -0.5013, 1.6], [-0.2517, 0.4019, 1.55]],
                [[-0.1017, -0.2013, 1.3], [0.7519, -0.0517, 1.35], [0.3013, 0.7019, 1.4]],
                [[-0.8013, 0.1017, 1.7], [-0.1519, 0.2013, 1.75], [-0.5017, 0.8519, 1.8]],
                [[0.1013, -0.8017, 1.2], [0.8519, -0.7013, 1.25], [0.5017, -0.1519, 1.22]]]
        dead = dict(behind=[[-0.3113, 0.2217, -1.0], [0.4319, 0.1113, -1.5], [0.0717, -0.5213, -0.7]],
                    straddling=[[-0.4113, -0.3217, 1.2], [0.3319, -0.2113, -0.3], [0.1217, 0.4713, 1.4]],
                    collinear=[[-0.25, -0.25, 1.1], [0.0, 0.0, 1.15], [0.5, 0.5, 1.2]])
        tris = [live[0], dead["behind"], live[1], dead["straddling"], live[2], dead["collinear"], live[3]]
        v0 = np.array(tris).reshape(-1, 3)
        v1 = v0.copy()
        v1[:, 2] = -1.3                                                    # frame 1: everything behind the camera (or collinear)
        v = np.stack([v0, v1, v0 + np.array([-0.0171, 0.0233, 0.05])])
        f = np.arange(v0.shape[0]).reshape(-1, 3)
        extra = dict(dead=(1, 3, 5))
        Ks, blurs = (2,), (band_blur(S),)
    else:
        raise KeyError(name)
    return dict(name=name, S=S, B=v.shape[0], ndc=torch.from_numpy(np.asarray(v)).float().contiguous(), faces=torch.from_numpy(np.asarray(f)).long(),
                Ks=Ks, blurs=tuple(Fr.f32(x) for x in blurs), **extra)


def runs(c):
    """the (K, blur) combinations of a case"""
    return [(K, blur) for blur in c["blurs"] for K in c["Ks"]]


def undecided_share(c, K, blur):
    und, cov = Fr.undecided(c, K, blur), Fr.covered(c, blur)
    return int(und.sum()), int(cov.sum())


def conditions(c):
    """the case forces its path: asserted on the reference's data.  Returns what it found (printed, recorded in docs/NOTEBOOK.md)."""
    name, S, B, Fn = c["name"], c["S"], c["B"], c["faces"].shape[0]
    info = {}
    for K, blur in runs(c):                                               # the cap on undecided pixels: move the vertices, not the cap
        n_und, n_cov = undecided_share(c, K, blur)
        info[f"undecided K={K} blur={blur:.3g}"] = f"{n_und}/{n_cov}"
        assert n_und <= 0.02 * n_cov, info
    for blur in c["blurs"]:
        if blur > 0.0:                                                    # with a band the clamp masks of the backward flip on the edge lines
            p = Fr.pairs(c, blur)
            assert not (p["cand"] & (p["smin"].abs() < Fr.TOL)).any(), (name, blur)
    blur = c["blurs"][0]
    p = Fr.pairs(c, blur)
    ncand = p["cand"].sum(1)                                              # (B,S,S)
    info["max_candidates"] = int(ncand.max())
    if name == "stack":
        assert Fn == 160 and B == 2
        assert ncand.max() >= 65 and ((ncand >= 1) & (ncand <= 63)).any(), info
        for K in (5, 64):
            ref = Fr.reference(c, K, blur)["p2f"]
            filled = ref >= 0
            up = ((ref[..., 1:] > ref[..., :-1]) | ~filled[..., 1:]).all(-1)
            down = ((ref[..., 1:] < ref[..., :-1]) | ~filled[..., 1:]).all(-1)
            cov = filled[..., 0]
            info[f"K={K} pixels whose kept ids are not monotone in depth"] = f"{int((cov & ~up & ~down).sum())}/{int(cov.sum())}"
            assert (cov & ~up & ~down).sum() >= 0.5 * cov.sum(), info
        # K = 64: a candidate that was evicted or rejected has a lower index than a kept one
        ref = Fr.reference(c, 64, blur)["p2f"]
        kept = torch.zeros(B, S, S, Fn, dtype=torch.long).scatter_add_(3, ref.clamp(min=0), (ref >= 0).long()) > 0
        lost = p["cand"].permute(0, 2, 3, 1) & ~kept
        ids = torch.arange(Fn)
        lowest_lost = torch.where(lost, ids, torch.full_like(ids, Fn)).amin(-1)
        info["K=64 pixels that lost a lower index than one they kept"] = int((lowest_lost < ref.amax(-1)).sum())
        assert info["K=64 pixels that lost a lower index than one they kept"] > 0, info
        assert not torch.equal(Fr.reference(c, 1, blur)["p2f"][0], Fr.reference(c, 1, blur)["p2f"][1])      # another permutation per frame
    if name == "ties":
        tied = c["tied"]
        assert tied.numel() == 12 and (tied[1:] - tied[:-1] > 1).any()     # scattered indices
        rows = c["faces"][tied]
        assert torch.unique(rows, dim=0).shape[0] == 6                      # duplicate rows AND distinct vertices of equal coordinates
        assert torch.unique(c["ndc"][0][rows].reshape(12, 9), dim=0).shape[0] == 2
        for K in c["Ks"]:
            ref = Fr.reference(c, K + 1, blur)["p2f"]
            inside_group = torch.isin(ref[..., K - 1], tied) & torch.isin(ref[..., K], tied)
            info[f"K={K} pixels with the cap inside the tied group"] = int(inside_group.sum())
            z = Fr.reference(c, K + 1, blur)["zbuf"]
            assert (z[..., K - 1] == z[..., K])[inside_group].all() and (ref[..., K - 1] < ref[..., K])[inside_group].all()
        assert info["K=4 pixels with the cap inside the tied group"] >= 100, info
        assert info["K=1 pixels with the cap inside the tied group"] > 0 and info["K=3 pixels with the cap inside the tied group"] > 0, info
    if name == "band":
        for blur in c["blurs"]:
            ref = Fr.reference(c, 4, blur)
            filled = ref["p2f"] >= 0
            outside = filled & (ref["dists"] > 0)
            zeros = (ref["bary"] == 0).sum(-1)
            n = dict(inside=int((filled & (ref["dists"] < 0)).sum()), one_clamped=int((outside & (zeros == 1)).sum()), two_clamped=int((outside & (zeros == 2)).sum()))
            info[f"blur={blur:.3g} slots"] = n
            if blur == c["blurs"][0]:
                assert n["inside"] >= 100 and n["one_clamped"] >= 20 and n["two_clamped"] >= 20, info
                for f in c["sub_pixel"]:                                   # kept by some pixel through the band only
                    pf = Fr.pairs(c, blur)
                    assert not pf["inside"][0, f].any() and (ref["p2f"][0] == f).any(), f
            else:                                                         # the workload's band (0.035 pixel): the row under the horizontal edge
                assert n["inside"] >= 100 and n["one_clamped"] >= 10, info
        x = c["ndc"][..., 0]
        assert x.max() > 1.0 and c["ndc"][..., 1].min() < -1.0 and S > 64 and S % 16 != 0
        cov = Fr.covered(c, c["blurs"][0])
        assert cov[:, :64, 64:].any() and cov[:, 64:, :64].any() and cov[:, :64, :64].any()          # three of the four super-tiles
        area = Fr.P._edge_fn(*[c["ndc"][0][c["faces"]][:, k, j].double() for k in (0, 1, 2) for j in (0, 1)])
        assert (area > 0).any() and (area < 0).any()                        # both windings
    if name == "nearplane":
        for blur in c["blurs"]:
            pf = Fr.pairs(c, blur)
            worst = pf["den"][pf["cand"]].max().item()
            info[f"blur={blur:.3g} largest denominator sum / kEps"] = worst / K_EPS
            assert worst < 0.5 * K_EPS and pf["cand"].any() and pf["live"].all(), info
            assert (pf["cand"].sum(1) >= 2).any()
    if name == "needle":
        fv = c["ndc"][0][c["faces"]].double()
        for f, i, j in c["short"]:
            l2 = ((fv[f, i, :2] - fv[f, j, :2]) ** 2).sum().item()
            area = Fr.P._edge_fn(fv[f, 0, 0], fv[f, 0, 1], fv[f, 1, 0], fv[f, 1, 1], fv[f, 2, 0], fv[f, 2, 1]).abs().item()
            n = int((Fr.reference(c, 2, blur)["p2f"] == f).sum())
            info[f"face {f}"] = dict(l2=l2, area=area, slots=n)
            assert 0 < l2 <= 0.5 * K_EPS and area > 100 * K_EPS and n > 0 and p["live"][0, f], info
    if name == "culled":
        ref = Fr.reference(c, 2, blur)["p2f"]
        assert not torch.isin(ref, torch.tensor(c["dead"])).any() and (ref[1] == -1).all() and not p["live"][1].any()
        assert (ref[0] >= 0).any() and (ref[2] >= 0).any() and not p["live"][:, list(c["dead"])].any()
        assert p["live"][0].sum() == Fn - 3
        z = c["ndc"][0][c["faces"]][..., 2]
        assert (z[1] < 0).all() and (z[3] < 0).any() and (z[3] > 0).any()
    print(f"[{name}] conditions: {info}")
    return info
