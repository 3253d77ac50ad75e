"""The K-fragment rasteriser's paths (csrc/fragments.hip: harp_rasterize_fragments_fwd / _bwd) against float64 on synthetic meshes, through
the raw C ABI.  The one scene tests/test_gpu_fragments.py rasterises never reaches: a full sorted list (eviction, insertion at its front and
middle, K = 64), exact depth ties, a blur band wide enough for the clamp-and-renormalise code and its backward to matter, a clamped
perspective denominator, a degenerate edge, culled faces, an empty frame, S off the 16- and 64-pixel grids.  tests/_fragment_cases.py builds
a mesh per path and asserts on the reference that the path is reached; the reference is oracle/p3d_like.rasterize_meshes in float64 on the
float32-rounded vertices, tests/_fragment_ref.py adds the bounds' ingredients (anchored by tests/test_fragment_ref_cpu.py).

Bounds, per element, none of them measured on the kernel:
  pix_to_face   equal in all K slots of every DECIDED pixel (undecided: a membership test flips when the centre moves by 2^-20 NDC, or two
                consecutive depths among the K + 1 nearest differ by less than 2^-20 relative without being duplicates; at most 2 % of a
                case's covered pixels, asserted on the reference); empty slots hold exactly -1 in all four outputs; depths ascend
  zbuf, bary, dists   |got - ref64| <= 4 E32 + 2^-22 |ref64| on the decided pixels, E32 = |ref32 - ref64|_inf of the oracle run in float32,
                per case, K, blur and output (4 x: the factor of tests/test_gpu_raster_paths.py; this kernel divides exactly)
  g_ndc (float atomics, += into a preset G0)   |got - G0 - ref| <= N_i M 2^-24 + 4 E32_g + 2^-22 A_i + 2 2^-24 |G0_i|, from the reference's
                per-pair shares (N_i of them on element i, the largest M, their magnitudes' sum A_i)
Measured err / bound per case, K and output: docs/NOTEBOOK.md."""
import pytest
import torch

from tests import _fragment_cases as C
from tests import _fragment_ref as Fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1
SENT_F, SENT_Z, SENT_B, SENT_D = -7, 7.0, 0.5, 0.25
NAN, INF = float("nan"), float("inf")


def _api():
    from harp_amd import _lib
    return _lib.lib(), _lib.ptr, _lib.stream


# ----------------------------------------------------------------------------------------------------------------------
# reference side (once per case, shared, never modified)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    built = {}
    yield built
    built.clear()


def get_case(cases, name):
    if name not in cases:
        c = C.build(name)
        c["info"] = C.conditions(c)
        c.update(V=c["ndc"].shape[1], F=c["faces"].shape[0], d_ndc=c["ndc"].to(DEV), d_faces=c["faces"].int().to(DEV).contiguous(), und={}, e32={})
        cases[name] = c
    return cases[name]


def bounds_of(c, K, blur):
    """(undecided (B,S,S), E32 per output) of a run"""
    key = (K, blur)
    if key not in c["und"]:
        c["und"][key] = Fr.undecided(c, K, blur)
        c["e32"][key] = Fr.e32(c, K, blur, c["und"][key])
        assert c["e32"][key]["same_faces"]
    return c["und"][key], c["e32"][key]


RUNS = [(n, K, i) for n in C.CASES for K, i in {"stack": [(1, 0), (5, 0), (64, 0)], "ties": [(1, 0), (3, 0), (4, 0), (8, 0)],
                                                "band": [(1, 0), (4, 0), (1, 1), (4, 1)], "nearplane": [(2, 0), (2, 1)], "needle": [(2, 0)],
                                                "culled": [(2, 0)]}[n]]
BWD_RUNS = [(n, K, i) for n, K, i in RUNS if K in {"stack": (1, 64), "ties": (1, 8), "band": (1, 4)}.get(n, (2,))] + \
           [("nearplane", 1, 0), ("nearplane", 1, 1), ("needle", 1, 0), ("culled", 1, 0)]


def test_the_runs_are_the_cases_runs(cases):
    for name in C.CASES:
        c = get_case(cases, name)
        assert sorted((K, c["blurs"][i]) for n, K, i in RUNS if n == name) == sorted(C.runs(c))


# ----------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------
def outputs(c, K):
    B, S = c["B"], c["S"]
    return (torch.full((B, S, S, K), SENT_F, dtype=torch.int32, device=DEV), torch.full((B, S, S, K), SENT_Z, device=DEV),
            torch.full((B, S, S, K, 3), SENT_B, device=DEV), torch.full((B, S, S, K), SENT_D, device=DEV))


def fwd(c, K, blur):
    from harp_amd import ops
    L, p, st = _api()
    ws = ops.rasterize_workspace(c["B"], c["F"], c["S"], DEV)
    p2f, z, b, d = outputs(c, K)
    rc = L.harp_rasterize_fragments_fwd(p(c["d_ndc"]), p(c["d_faces"]), c["B"], c["V"], c["F"], c["S"], blur, K, p(ws), p(p2f), p(z), p(b), p(d), st())
    assert rc == 0
    torch.cuda.synchronize()
    return dict(p2f=p2f, zbuf=z, bary=b, dists=d)


def bwd(c, K, blur, p2f, g0, g_zbuf=None, g_bary=None, g_dists=None):
    """g_ndc preset to g0; the cotangents are CPU tensors or None (NULL)"""
    L, p, st = _api()
    dev = lambda t: None if t is None else t.float().contiguous().to(DEV)
    gz, gb, gd = dev(g_zbuf), dev(g_bary), dev(g_dists)
    d_p2f = p2f.int().contiguous().to(DEV)
    assert d_p2f.shape == (c["B"], c["S"], c["S"], K) and int(d_p2f.max()) < c["F"] and int(d_p2f.min()) >= -1
    g_ndc = g0.clone().to(DEV)
    rc = L.harp_rasterize_fragments_bwd(p(c["d_ndc"]), p(c["d_faces"]), p(d_p2f), p(gz), p(gb), p(gd), c["B"], c["V"], c["F"], c["S"], blur, K, p(g_ndc), st())
    assert rc == 0
    torch.cuda.synchronize()
    return g_ndc.cpu()


def ratio_of(err, bound):
    return torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max().item() if err.numel() else 0.0


def check_forward(c, K, blur, out, tag=""):
    ref = Fr.reference(c, K, blur)
    und, e32 = bounds_of(c, K, blur)
    dec = ~und
    got = out["p2f"].cpu().long()
    assert torch.equal(got[dec], ref["p2f"][dec]), (c["name"], K, blur, int((got[dec] != ref["p2f"][dec]).sum()))
    assert ((got >= -1) & (got < c["F"])).all()                           # the undecided pixels too hold a possible value; no sentinel is left
    empty = got < 0
    z, b, d = out["zbuf"].cpu(), out["bary"].cpu(), out["dists"].cpu()
    assert (z[empty] == -1).all() and (d[empty] == -1).all() and (b[empty] == -1).all()
    assert (~empty[..., 1:] <= ~empty[..., :-1]).all()                    # filled slots first ...
    zz = torch.where(empty, torch.full_like(z, INF), z)
    assert (zz[..., 1:] >= zz[..., :-1]).all() and (z[~empty] >= 0).all()  # ... in ascending depth
    m = dec[..., None] & (ref["p2f"] >= 0)
    res = {}
    for k, g in (("zbuf", z), ("bary", b), ("dists", d)):
        r = ref[k]
        assert torch.isfinite(g).all()
        err, bound = (g.double() - r).abs(), 4.0 * e32[k] + 2.0 ** -22 * r.abs()
        mm = m[..., None].expand_as(r) if k == "bary" else m
        res[k] = ratio_of(err[mm], bound[mm])
    print(f"[{c['name']} K={K} blur={blur:.3g}{tag}] err / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in res.items()) +
          "  (E32 " + " ".join(f"{e32[k]:.2e}" for k in Fr.OUTPUTS) + f"; {int(m.sum())} slots, {int(und.sum())} undecided pixels)")
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, (c["name"], K, blur, bad)
    return res


def cotangents(c, K, blur, seed=0):
    """random float32 cotangents, zero on the undecided pixels"""
    und, _ = bounds_of(c, K, blur)
    B, S = c["B"], c["S"]
    g = torch.Generator().manual_seed(1000 * seed + 10 * K + sum(map(ord, c["name"])))
    keep = (~und)[..., None].float()
    gz, gd = torch.randn(B, S, S, K, generator=g) * keep, torch.randn(B, S, S, K, generator=g) * keep
    gb = torch.randn(B, S, S, K, 3, generator=g) * keep[..., None]
    if c["name"] == "needle":
        gd = torch.zeros_like(gd)       # past the short end two near-equal edge distances send the same gradient to different vertices
    g0 = torch.randn(B, c["V"], 3, generator=g)
    return dict(g_zbuf=gz, g_bary=gb, g_dists=gd), g0


def gradient_reference(c, K, blur, cots):
    p2f = Fr.reference(c, K, blur)["p2f"]
    st = Fr.gradient(c, p2f, blur, **cots)
    g32 = Fr.gradient(c, p2f, blur, dtype=torch.float32, stats=False, **cots)
    st["e32"] = (g32.double() - st["ref"]).abs().max().item()
    return st


def check_gradient(c, tag, got, g0, st, must_flow=True):
    assert torch.isfinite(got).all(), (c["name"], tag)
    assert not must_flow or st["ref"].abs().max() > 0
    err = (got.double() - g0.double() - st["ref"]).abs()
    bound = st["N"] * st["M"] * 2.0 ** -24 + 4.0 * st["e32"] + 2.0 ** -22 * st["A"] + 2.0 * 2.0 ** -24 * g0.double().abs()
    ratio = ratio_of(err, bound)
    print(f"[{c['name']} {tag}] g_ndc err / bound {ratio:.3f} (max |g| {st['ref'].abs().max().item():.3e}, E32_g {st['e32']:.2e}, largest N {int(st['N'].max())})")
    assert ratio <= 1.0, (c["name"], tag, ratio)
    return ratio


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,which", RUNS)
def test_forward_every_slot(name, K, which, cases):
    c = get_case(cases, name)
    blur = c["blurs"][which]
    out = fwd(c, K, blur)
    check_forward(c, K, blur, out)
    again = fwd(c, K, blur)                                               # no atomics: bit-identical
    for k in out:
        assert torch.equal(out[k], again[k]), k
    if name == "culled":                                                  # a frame in which no face survives
        assert (out["p2f"][1] == -1).all() and (out["zbuf"][1] == -1).all()


@pytest.mark.parametrize("name,K,which", BWD_RUNS)
def test_backward_every_element(name, K, which, cases):
    c = get_case(cases, name)
    blur = c["blurs"][which]
    cots, g0 = cotangents(c, K, blur)
    p2f = Fr.reference(c, K, blur)["p2f"]
    st = gradient_reference(c, K, blur, cots)
    got = bwd(c, K, blur, p2f, g0, **cots)
    check_gradient(c, f"K={K} blur={blur:.3g}", got, g0, st)
    if name == "culled":
        assert torch.equal(got[1], g0[1])                                 # nothing flows into the frame without a face
    if name == "stack" and K == 64:                                       # the kernel's own pix_to_face gives the same gradient
        own = fwd(c, K, blur)["p2f"].cpu()
        check_gradient(c, f"K={K} own pix_to_face", bwd(c, K, blur, own, g0, **cots), g0, st)


CONTRACT = [("band", 4, 0), ("band", 4, 1), ("ties", 8, 0), ("nearplane", 2, 1), ("culled", 2, 0)]


@pytest.mark.parametrize("name,K,which", CONTRACT)
def test_backward_contract(name, K, which, cases):
    """each cotangent alone (the other two NULL); all three NULL; NaN cotangents on the empty slots"""
    c = get_case(cases, name)
    blur = c["blurs"][which]
    cots, g0 = cotangents(c, K, blur, seed=1)
    p2f = Fr.reference(c, K, blur)["p2f"]
    for k in cots:
        one = {k: cots[k]}
        got = bwd(c, K, blur, p2f, g0, **one)
        check_gradient(c, f"K={K} blur={blur:.3g} {k} alone", got, g0, gradient_reference(c, K, blur, one))
    assert torch.equal(bwd(c, K, blur, p2f, g0), g0)
    empty = p2f < 0
    assert empty.any()
    poisoned = {k: torch.where(empty[..., None] if k == "g_bary" else empty, torch.full_like(v, NAN), v) for k, v in cots.items()}
    got = bwd(c, K, blur, p2f, g0, **poisoned)
    check_gradient(c, f"K={K} blur={blur:.3g} NaN on empty slots", got, g0, gradient_reference(c, K, blur, cots))
    if name == "culled":
        assert torch.equal(got[1], g0[1])


def test_python_op_packs_the_ids(cases):
    from harp_amd import ops
    c = get_case(cases, "culled")
    K, blur, F = 2, c["blurs"][0], c["F"]
    raw = fwd(c, K, blur)
    p2f, z, b, d = ops.rasterize_fragments(c["d_ndc"], c["d_faces"], c["S"], blur, K, packed=True)
    assert p2f.dtype == torch.int64 and p2f.shape == (c["B"], c["S"], c["S"], K)
    for f in range(c["B"]):
        ids = p2f[f]
        assert bool(((ids == -1) | ((ids >= f * F) & (ids < (f + 1) * F))).all())
    local = torch.where(p2f >= 0, p2f - (torch.arange(c["B"], device=DEV) * F).view(-1, 1, 1, 1), p2f)
    assert torch.equal(local.int(), raw["p2f"]) and torch.equal(z, raw["zbuf"]) and torch.equal(b, raw["bary"]) and torch.equal(d, raw["dists"])
    assert bool((p2f[1] == -1).all()) and bool((p2f[0] >= 0).any()) and bool((p2f[2] >= 2 * F).any())
    unpacked = ops.rasterize_fragments(c["d_ndc"], c["d_faces"], c["S"], blur, K, packed=False)[0]
    assert torch.equal(unpacked.int(), raw["p2f"])


def test_argument_checks_refuse_without_a_launch(cases):
    """HARP_ERR_ARG, every buffer correctly sized and valid, no output touched"""
    from harp_amd import ops
    L, p, st = _api()
    c = get_case(cases, "culled")
    B, V, F, S, K, blur = c["B"], c["V"], c["F"], c["S"], 2, c["blurs"][0]
    ws = ops.rasterize_workspace(B, F, S, DEV)
    ws0 = ws.clone()
    p2f, z, b, d = outputs(c, 64)                                         # (sized for the largest K any call below could use)
    good = [p(c["d_ndc"]), p(c["d_faces"]), B, V, F, S, blur, K, p(ws), p(p2f), p(z), p(b), p(d), st()]
    changes = [(k, None) for k in (0, 1, 8, 9, 10, 11, 12)] + [(7, 0), (7, 65), (7, -1), (2, 0), (4, 0), (5, 0), (3, 0), (2, -1), (5, -1),
                                                                (6, -1.0), (6, -1e-30), (6, NAN), (6, INF), (6, -INF)]
    for k, v in changes:
        bad = list(good)
        bad[k] = v
        assert L.harp_rasterize_fragments_fwd(*bad) == ERR_ARG, (k, v)
    ref = Fr.reference(c, K, blur)["p2f"].int().contiguous().to(DEV)
    gz, gb, gd = torch.ones(B, S, S, K, device=DEV), torch.ones(B, S, S, K, 3, device=DEV), torch.ones(B, S, S, K, device=DEV)
    g_ndc = torch.full((B, V, 3), SENT_D, device=DEV)
    good = [p(c["d_ndc"]), p(c["d_faces"]), p(ref), p(gz), p(gb), p(gd), B, V, F, S, blur, K, p(g_ndc), st()]
    changes = [(k, None) for k in (0, 1, 2, 12)] + [(11, 0), (11, 65), (11, -1), (6, 0), (9, 0), (7, 0), (6, -1), (9, -1),
                                                    (10, -1.0), (10, -1e-30), (10, NAN), (10, -INF)]
    for k, v in changes:
        bad = list(good)
        bad[k] = v
        assert L.harp_rasterize_fragments_bwd(*bad) == ERR_ARG, (k, v)
    torch.cuda.synchronize()
    assert bool((p2f == SENT_F).all()) and bool((z == SENT_Z).all()) and bool((b == SENT_B).all()) and bool((d == SENT_D).all())
    assert bool((g_ndc == SENT_D).all()) and torch.equal(ws, ws0)
    assert L.harp_rasterize_fragments_fwd(*[p(c["d_ndc"]), p(c["d_faces"]), B, V, F, S, blur, K, p(ws), p(p2f), p(z), p(b), p(d), st()]) == 0      # the valid call goes through
    torch.cuda.synchronize()
