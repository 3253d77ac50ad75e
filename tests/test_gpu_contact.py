"""-m gpu: ops.mesh_contact (csrc/contact.hip: harp_mesh_contact) against the float64 brute force of its contract (tests/_contact_ref.py)
over the cases that file makes: B in {1, 3}, 1 to 130 query vertices, targets of 1 to 320 faces around the kernel's chunk of 128, both
flips of each side, max_dist in {0, 0.004, 0.02, inf}; a pair 0.5 m apart, a coincident pair, degenerate inputs.

Bounds (each derived, none measured): distance within 32 * 2^-24 * M of float64's, M the case's largest absolute view coordinate — the
inputs are exact float32 and each coordinate difference and the norm round within a few units of 2^-24 M; a vertex whose float64
distance lies within that bound of max_dist may be finite or +inf; the reported face's float64 distance within the same bound of the
minimum; winding number within 1e-4 (320 terms of a float32 atan2, about 1e-5, times 10 for the device's atan2); the inside flag
wind > 0.5 equal wherever |wind64 - 0.5| >= 0.05.  The test prints the largest errors it saw."""
import itertools

import numpy as np
import pytest
import torch

from tests import _contact_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _side(ops, d):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    return ops.ContactMesh(t(d["verts"]), t(d["cam_R"]), t(d["cam_T"]), t(d.get("faces")), d.get("flip", False))


def _check(got, ref, max_dist, what, stats):
    """one call's three outputs against the reference at this max_dist; stats collects the largest errors"""
    dist, face, wind = (x.cpu().numpy() for x in got)
    assert dist.dtype == np.float32 and face.dtype == np.int32 and wind.dtype == np.float32
    assert not np.isnan(dist).any() and not np.isnan(wind).any(), what
    bound = CR.dist_bound(ref["M"])
    maybe = CR.undecided(ref, max_dist)
    want_near = np.isfinite(ref["d_min"]) & (ref["d_min"] <= max_dist)      # (+inf: a non-finite query vertex, or no valid face)
    near = np.isfinite(dist)
    assert np.array_equal(near[~maybe], want_near[~maybe]), ("which vertices are within max_dist", what)
    assert (dist[near] <= max_dist).all(), what
    assert ((face >= 0) == near).all() and (face[near] < ref["D"].shape[-1]).all() and (face[~near] == -1).all() and (wind[~near] == 0).all(), what
    both = near & np.isfinite(ref["d_min"])
    assert np.array_equal(both, near), what
    err = np.abs(dist[near].astype(np.float64) - ref["d_min"][near])
    stats["dist"] = max(stats["dist"], float((err / ref["M"]).max()) if err.size else 0.0)
    assert (err <= bound).all(), ("distance", what, err.max(), bound)
    b, i = np.nonzero(near)
    excess = ref["D"][b, i, face[b, i]] - ref["d_min"][b, i]                # the float64 distance to the face the kernel reports
    assert (excess <= bound).all(), ("the reported face attains the minimum", what, excess.max() if excess.size else 0, bound)
    werr = np.abs(wind[near].astype(np.float64) - ref["wind_all"][near])
    stats["wind"] = max(stats["wind"], float(werr.max()) if werr.size else 0.0)
    assert (werr <= CR.WIND_TOL).all(), ("winding number", what, werr.max())
    clear = near & (np.abs(ref["wind_all"] - 0.5) >= CR.INSIDE_BAND)
    assert np.array_equal(wind[clear] > 0.5, ref["wind_all"][clear] > 0.5), ("inside flag", what)
    assert (~clear & near).sum() <= 0.02 * near.size and maybe.sum() <= 0.02 * near.size, what
    stats["n"] += int(near.sum())


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("Vq", CR.QUERY_V)
@pytest.mark.parametrize("B", [1, 3])
def test_mesh_contact_against_float64(B, Vq):
    from harp_amd import ops
    stats = dict(dist=0.0, wind=0.0, n=0)
    for k, (name, q, t) in enumerate(CR.grid_cases(B, Vq)):
        ref = CR.mesh_contact(q, t)
        dq, dt = _side(ops, q), _side(ops, t)
        for md in CR.MAX_DISTS:
            got = ops.mesh_contact(dq, dt, md)
            _check(got, ref, md, (name, md), stats)
            if k % 4 == 0:                                                  # once per target mesh
                assert _same(got, ops.mesh_contact(dq, dt, md)), ("a repeated call is bit-identical", name, md)
                for drop in range(3):                                       # one output missing: the others unchanged
                    want = tuple(w for i, w in enumerate(("dist", "face", "wind")) if i != drop)
                    part = ops.mesh_contact(dq, dt, md, want=want)
                    assert part[drop] is None and _same([x for i, x in enumerate(part) if i != drop], [x for i, x in enumerate(got) if i != drop]), (name, md, drop)
    print(f"[mesh_contact] B={B} Vq={Vq}: {stats['n']} finite vertices, largest |dist - dist64| = {stats['dist'] / CR.EPS32:.2f} * 2^-24 M "
          f"(bound {CR.DIST_FACTOR:g}), largest |wind - wind64| = {stats['wind']:.2e} (bound {CR.WIND_TOL:g})")


def test_apart_everything_is_culled():
    from harp_amd import ops
    q, t = CR.apart_case()
    ref = CR.mesh_contact(q, t)
    assert ref["d_min"].min() > 0.3
    dist, face, wind = ops.mesh_contact(_side(ops, q), _side(ops, t), 0.02)
    assert torch.isinf(dist).all() and (dist > 0).all() and (face == -1).all() and (wind == 0).all()
    _check(ops.mesh_contact(_side(ops, q), _side(ops, t)), ref, np.inf, "apart, no limit", dict(dist=0.0, wind=0.0, n=0))


def test_coincident_pair_has_distance_zero():
    from harp_amd import ops
    for qf, tf in ((False, False), (True, True)):
        q, t = CR.coincident_case()
        q["flip"], t["flip"] = qf, tf
        ref = CR.mesh_contact(q, t)
        assert (ref["d_min"] == 0).all()
        for md in CR.MAX_DISTS:
            got = ops.mesh_contact(_side(ops, q), _side(ops, t), md)
            assert (got.dist.cpu().numpy() <= CR.dist_bound(ref["M"])).all(), (qf, tf, md)
            assert (got.face >= 0).all() and not torch.isnan(got.wind).any()
            # every vertex lies on the surface it is tested against: its winding number is the reference's where that is decided by the
            # faces that do not touch it (those that do add exactly 0 on both sides)
            assert np.abs(got.wind.cpu().numpy() - ref["wind_all"]).max() <= CR.WIND_TOL, (qf, tf, md)


@pytest.mark.parametrize("B", [1, 3])
def test_degenerate_inputs(B):
    from harp_amd import ops
    stats = dict(dist=0.0, wind=0.0, n=0)
    for qf, tf in itertools.product((False, True), repeat=2):
        q, t = CR.degenerate_case(B, qf, tf)
        ref = CR.mesh_contact(q, t)
        for md in CR.MAX_DISTS:
            got = ops.mesh_contact(_side(ops, q), _side(ops, t), md)
            _check(got, ref, md, ("degenerate", B, qf, tf, md), stats)
            bad = ~np.isfinite(q["verts"]).all(-1)
            assert torch.isinf(got.dist)[torch.from_numpy(bad)].all() and (got.face.cpu().numpy()[bad] == -1).all() and (got.wind.cpu().numpy()[bad] == 0).all()
    # a target without one valid face: nothing to be near to, whatever max_dist
    q, t = CR.degenerate_case(B, False, False)
    t["verts"][:] = np.nan
    for md in (0.02, np.inf):
        got = ops.mesh_contact(_side(ops, q), _side(ops, t), md)
        assert torch.isinf(got.dist).all() and (got.face == -1).all() and (got.wind == 0).all()


def test_host_validation():
    from harp_amd import ops
    q, t = CR.make_pair(1, 1, 4, "ico0")
    dq, dt = _side(ops, q), _side(ops, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mesh_contact(ops.ContactMesh(*(torch.from_numpy(q[k]) for k in ("verts", "cam_R", "cam_T"))), dt)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dist"):
            ops.mesh_contact(dq, dt, bad)
    with pytest.raises(ValueError, match="want"):
        ops.mesh_contact(dq, dt, want=())
    with pytest.raises(TypeError, match="faces"):
        ops.mesh_contact(dq, dt._replace(faces=None))
    with pytest.raises(ValueError, match="cam_R"):
        ops.mesh_contact(dq, dt._replace(cam_R=dt.cam_R.repeat(2, 1)))
    with pytest.raises(RuntimeError, match="forward only|grad"):
        ops.mesh_contact(dq._replace(verts=dq.verts.clone().requires_grad_()), dt)
