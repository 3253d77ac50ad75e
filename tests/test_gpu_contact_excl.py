"""-m gpu: ops.mesh_contact(..., exclude=) (csrc/contact.hip: harp_mesh_contact_excl) against the float64 brute force of its contract
(tests/_contact_ref.py with the masked minimum of tests/_contact_excl_ref.py) over tests/_contact_ref.py's grid: B in {1, 3}; 1, 63, 64, 65
and 130 query vertices around the 64-lane tile; targets of 127, 128 and 129 faces around the 128-face chunk and the ends of the table's
16-byte words, 960 faces for two chunks per wave; both flips of each side; max_dist in {0, 0.004, 0.02, inf}.  Per case six masks
(_contact_excl_ref.masks): nothing (bit for bit the call without `exclude`), Bernoulli(0.3), every vertex's nearest face (the runner-up
wins), every face for the odd vertices, whole chunks, everything but the last face; and once per target mesh a face duplicated at the end
of the list, one of the tied pair excluded.

Bounds: tests/test_gpu_contact.py's own, derived there — distance within 32 * 2^-24 * M of float64's masked minimum; the reported face
counts and its float64 distance is within the same bound of that minimum; the winding number, which is NOT masked, within 1e-4 of the sum
over all faces; the near set equal outside the undecided vertices; the inside flag equal outside the band; at most 2 % of a case in
either (tests/test_contact_excl_cpu.py counts both on the reference alone).  The test prints the largest errors it saw."""
import itertools

import numpy as np
import pytest
import torch

from tests import _contact_excl_ref as XR
from tests import _contact_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _side(ops, d):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    return ops.ContactMesh(t(d["verts"]), t(d["cam_R"]), t(d["cam_T"]), t(d.get("faces")), d.get("flip", False))


def _table(mask):
    return torch.from_numpy(XR.pack(mask).view(np.int32)).to(DEV)


def _check(got, ref, mask, max_dist, what, stats):
    """one call's three outputs against the MASKED reference at this max_dist; stats collects the largest errors"""
    dist, face, wind = (x.cpu().numpy() for x in got)
    assert dist.dtype == np.float32 and face.dtype == np.int32 and wind.dtype == np.float32
    assert not np.isnan(dist).any() and not np.isnan(wind).any(), what
    bound = CR.dist_bound(ref["M"])
    maybe = CR.undecided(ref, max_dist)
    want_near = np.isfinite(ref["d_min"]) & (ref["d_min"] <= max_dist)      # (+inf: a non-finite query vertex, or no valid face that counts)
    near = np.isfinite(dist)
    assert np.array_equal(near[~maybe], want_near[~maybe]), ("which vertices are within max_dist", what)
    assert (dist[near] <= max_dist).all(), what
    assert ((face >= 0) == near).all() and (face[near] < ref["D"].shape[-1]).all() and (face[~near] == -1).all() and (wind[~near] == 0).all(), what
    assert np.array_equal(near & np.isfinite(ref["d_min"]), near), what
    b, i = np.nonzero(near)
    assert not mask[i, face[b, i]].any(), ("an excluded face is never reported", what)
    err = np.abs(dist[near].astype(np.float64) - ref["d_min"][near])
    stats["dist"] = max(stats["dist"], float((err / ref["M"]).max()) if err.size else 0.0)
    assert (err <= bound).all(), ("distance", what, err.max(), bound)
    excess = ref["D"][b, i, face[b, i]] - ref["d_min"][b, i]                # the float64 distance to the face the kernel reports (inf if masked)
    assert (excess <= bound).all(), ("the reported face attains the masked minimum", what, excess.max() if excess.size else 0, bound)
    werr = np.abs(wind[near].astype(np.float64) - ref["wind_all"][near])
    stats["wind"] = max(stats["wind"], float(werr.max()) if werr.size else 0.0)
    assert (werr <= CR.WIND_TOL).all(), ("winding number, over ALL faces", what, werr.max())
    clear = near & (np.abs(ref["wind_all"] - 0.5) >= CR.INSIDE_BAND)
    assert np.array_equal(wind[clear] > 0.5, ref["wind_all"][clear] > 0.5), ("inside flag", what)
    assert (~clear & near).sum() <= 0.02 * near.size and maybe.sum() <= 0.02 * near.size, what
    stats["n"] += int(near.sum())


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _tie(ops, name, q, t, ref, plain):
    """face f0, the one the kernel reports for (frame 0, vertex 0), once more at the end of the list: the pair ties exactly.  With f0 excluded its copy
    wins where f0 did, at the same bits; with the copy excluded nothing changes.  plain: the call without `exclude` on the list as it was
    -> the vertices at which the copy won"""
    Vq, F = ref["D"].shape[1:]
    f0 = int(plain.face[0, 0])
    assert f0 >= 0
    dq, dt2 = _side(ops, q), _side(ops, XR.with_duplicate(t, f0))
    both = ops.mesh_contact(dq, dt2, want=("dist", "face"))
    assert torch.equal(both.dist, plain.dist) and torch.equal(both.face, plain.face), ("the lower of a tied pair wins", name)
    was = plain.face == f0
    assert was[0, 0]
    for hide in (f0, F):
        mask = np.zeros((Vq, F + 1), bool)
        mask[:, hide] = True
        got = ops.mesh_contact(dq, dt2, want=("dist", "face"), exclude=_table(mask))
        assert torch.equal(got.dist, plain.dist), ("a tied pair has the same distance bits", name, hide)
        assert torch.equal(got.face[~was], plain.face[~was]), (name, hide)
        if hide == F:                                                       # f0 counts and still wins every tie it won
            assert torch.equal(got.face, plain.face), (name, hide)
        else:                                                               # its copy wins, unless a face between the two ties with them:
            g = got.face[was]                                               # (a shared corner or edge can be the nearest point of both)
            assert ((g == F) | ((g > f0) & (g < F))).all(), ("the lowest of the faces that count", name, hide)
            copies = int((g == F).sum())
    return copies


@pytest.mark.parametrize("Vq", CR.QUERY_V)
@pytest.mark.parametrize("B", [1, 3])
def test_masked_contact_against_float64(B, Vq):
    from harp_amd import ops
    stats = dict(dist=0.0, wind=0.0, n=0)
    forced = copies = 0
    for k, (name, q, t) in enumerate(CR.grid_cases(B, Vq)):
        ref = CR.mesh_contact(q, t)
        dq, dt = _side(ops, q), _side(ops, t)
        plain = {md: ops.mesh_contact(dq, dt, md) for md in CR.MAX_DISTS}
        for tag, mask in XR.masks(ref, 7 * k + Vq):
            ref_m = XR.masked(ref, mask)
            table = _table(mask)
            if tag == "nearest":
                moved = np.isfinite(ref_m["d_min"])
                assert (ref_m["d_min"][moved] >= ref["d_min"][moved]).all() and (ref_m["face"][moved] != ref["face"][moved]).all()
                forced += int(moved.sum())
            for md in CR.MAX_DISTS:
                got = ops.mesh_contact(dq, dt, md, exclude=table)
                if tag == "zero":
                    assert _same(got, plain[md]), ("no bit set: the call without exclude, bit for bit", name, md)
                    continue
                if tag == "odd":
                    assert torch.isinf(got.dist[:, 1::2]).all() and (got.face[:, 1::2] == -1).all() and (got.wind[:, 1::2] == 0).all(), (name, md)
                    assert _same([x[:, 0::2] for x in got], [x[:, 0::2] for x in plain[md]]), ("the even vertices are unchanged", name, md)
                    continue
                _check(got, ref_m, mask, md, (name, tag, md), stats)
                if k % 4 == 0 and tag == "bernoulli":                       # once per target mesh
                    assert _same(got, ops.mesh_contact(dq, dt, md, exclude=table)), ("a repeated call is bit-identical", name, md)
                    for drop in range(3):                                   # one output missing: the others unchanged
                        want = tuple(w for i, w in enumerate(("dist", "face", "wind")) if i != drop)
                        part = ops.mesh_contact(dq, dt, md, want=want, exclude=table)
                        assert part[drop] is None and _same([x for i, x in enumerate(part) if i != drop], [x for i, x in enumerate(got) if i != drop]), (name, md, drop)
        if k % 4 == 0:
            copies += _tie(ops, name, q, t, ref, plain[np.inf])
    assert forced > 0 and copies > 0
    print(f"[mesh_contact exclude] B={B} Vq={Vq}: {stats['n']} finite vertices, largest |dist - dist64| = {stats['dist'] / CR.EPS32:.2f} * 2^-24 M "
          f"(bound {CR.DIST_FACTOR:g}), largest |wind - wind64| = {stats['wind']:.2e} (bound {CR.WIND_TOL:g}); {forced} runner-ups forced, "
          f"{copies} ties won by the copy")


@pytest.mark.parametrize("B", [1, 3])
def test_degenerate_inputs_under_a_mask(B):
    from harp_amd import ops
    stats = dict(dist=0.0, wind=0.0, n=0)
    for qf, tf in itertools.product((False, True), repeat=2):
        q, t = CR.degenerate_case(B, qf, tf)
        ref = CR.mesh_contact(q, t)
        tag, mask = list(XR.masks(ref, 11))[1]
        assert tag == "bernoulli"
        ref_m = XR.masked(ref, mask)
        for md in CR.MAX_DISTS:
            got = ops.mesh_contact(_side(ops, q), _side(ops, t), md, exclude=_table(mask))
            _check(got, ref_m, mask, md, ("degenerate", B, qf, tf, md), stats)
            bad = ~np.isfinite(q["verts"]).all(-1)
            assert torch.isinf(got.dist)[torch.from_numpy(bad)].all() and (got.face.cpu().numpy()[bad] == -1).all() and (got.wind.cpu().numpy()[bad] == 0).all()


def test_host_validation_of_exclude():
    from harp_amd import ops
    q, t = CR.make_pair(1, 1, 4, "multi129")
    dq, dt = _side(ops, q), _side(ops, t)
    good = torch.zeros(2, 4, 4, dtype=torch.int32, device=DEV)
    assert _same(ops.mesh_contact(dq, dt, exclude=good), ops.mesh_contact(dq, dt))
    assert _same(ops.mesh_contact(dq, dt, exclude=good.view(torch.uint32)), ops.mesh_contact(dq, dt))
    for bad in (good.long(), good.float(), good.bool(), good.cpu().numpy()):
        with pytest.raises(TypeError, match="exclude"):
            ops.mesh_contact(dq, dt, exclude=bad)
    for bad in (good[:1], good[:, :3], good[..., :3], good.reshape(-1), torch.zeros(3, 4, 4, dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="exclude"):
            ops.mesh_contact(dq, dt, exclude=bad)
    with pytest.raises(ValueError, match="exclude"):
        ops.mesh_contact(dq, dt, exclude=good.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        ops.mesh_contact(dq, dt, exclude=torch.zeros(2, 4, 8, dtype=torch.int32, device=DEV)[..., ::2])
