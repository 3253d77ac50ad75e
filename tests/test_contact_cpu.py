"""The float64 restatement of harp_mesh_contact's contract (tests/_contact_ref.py) against known geometry: hand-computed point-triangle
distances in each Voronoi region, a sphere against an icosphere within the mesh's sagitta, winding numbers of closed and open meshes, the
mirror rules, the skip rules — and the share of vertices that the cases of tests/test_gpu_contact.py leave undecided.  No device."""
import numpy as np
import pytest

from tests import _contact_ref as CR

EYE = np.eye(3).reshape(1, 9)
ZERO = np.zeros((1, 3))


def _side(verts, faces=None, flip=False, R=EYE, T=ZERO):
    v = np.asarray(verts, float)[None]
    return dict(verts=v, cam_R=np.repeat(R, 1, 0), cam_T=np.repeat(T, 1, 0), faces=faces, flip=flip)


def test_point_against_a_triangle_in_each_voronoi_region():
    # a = (0,0,0), b = (4,0,0), c = (0,3,0); the hypotenuse bc has length 5 and lies on 3x + 4y = 12
    tri = _side([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.array([[0, 1, 2]]))
    pts = {"face": ([1, 1, 2], 2.0),                                       # above the interior: the height
           "vertex a": ([-3, -4, 0], 5.0), "vertex b": ([7, -4, 0], 5.0), "vertex c": ([-3, 7, 0], 5.0),
           "edge ab": ([2, -2, 0], 2.0), "edge ac": ([-2, 1, 0], 2.0),
           "edge bc": ([4, 3, 0], 12.0 / 5.0),                             # (3*4 + 4*3 - 12) / 5, its foot (2.56, 1.08) lies on the edge
           "edge ab, above": ([2, -3, 4], 5.0), "vertex a, above": ([-2, -2, 1], 3.0)}
    ref = CR.mesh_contact(_side([p for p, _ in pts.values()]), tri)
    for k, (name, (_, want)) in enumerate(pts.items()):
        assert abs(ref["dist"][0, k] - want) < 1e-12, (name, ref["dist"][0, k], want)
    assert (ref["face"] == 0).all()


@pytest.mark.parametrize("sub", [0, 1, 2])
def test_sphere_against_icosphere_within_the_sagitta(sub):
    v, f = CR.icosphere(sub)
    r = 0.05
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    depth = ((n / np.linalg.norm(n, axis=1, keepdims=True)) * v[f[:, 0]]).sum(1)      # each face plane's distance from the centre
    assert (depth > 0).all(), "the faces are oriented outwards"
    sagitta = r * (1.0 - depth.min())
    rng = np.random.default_rng(sub)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for radius in (0.3 * r * depth.min(), 0.9 * r * depth.min(), 1.1 * r, 3.0 * r):       # inside the inscribed ball, outside the sphere
        ref = CR.mesh_contact(_side(radius * d), _side(r * v, f))
        err = ref["dist"][0] - abs(radius - r)
        lo, hi = (-sagitta, 0.0) if radius < r else (0.0, sagitta)
        assert (err >= lo - 1e-12).all() and (err <= hi + 1e-12).all(), (sub, radius, err.min(), err.max(), sagitta)


def test_winding_number_of_closed_and_open_meshes():
    v, f = CR.icosphere(2)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(100, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = CR.mesh_contact(_side(0.04 * d * rng.uniform(0, 1, (100, 1))), _side(0.05 * v, f))["wind"]
    outside = CR.mesh_contact(_side(d * rng.uniform(0.06, 1.0, (100, 1))), _side(0.05 * v, f))["wind"]
    assert np.abs(inside - 1.0).max() < 1e-12 and np.abs(outside).max() < 1e-12, (inside, outside)
    # the open mesh, seen from its centre: what is left of the sphere, by the spherical areas of the removed faces (Girard)
    vo, kept, removed = CR.open_icosphere(2)
    assert kept.shape[0] == 276 and removed.shape[0] == 44
    gone = sum(CR.spherical_area(*vo[t]) for t in removed)
    got = CR.mesh_contact(_side([[0.0, 0.0, 0.0]]), _side(0.05 * vo, kept))["wind"][0, 0]
    assert abs(got - (1.0 - gone / (4.0 * np.pi))) < 1e-12, (got, gone)
    assert 0.8 < got < 0.95                                                  # fractional: the mesh is open


def test_mirror_rules():
    rng = np.random.default_rng(4)
    q, t = CR.make_pair(40, 3, 65, "open2")
    base = CR.mesh_contact(q, t)
    both = CR.mesh_contact(dict(q, flip=True), dict(t, flip=True))
    for k in ("dist", "face", "wind"):                                       # mirroring both sides changes nothing
        assert np.array_equal(base[k], both[k]), k
    # the target alone, by its flag = its view-space vertices mirrored beforehand: an identity camera makes model space view space
    ident = dict(cam_R=np.repeat(EYE, 3, 0).astype(np.float32), cam_T=np.zeros((3, 3), np.float32))
    qi, ti = dict(q, **ident), dict(t, **ident)
    flagged = CR.mesh_contact(qi, dict(ti, flip=True))
    mirrored = CR.mesh_contact(qi, dict(ti, verts=ti["verts"] * np.array([-1, 1, 1], np.float32)))
    assert np.array_equal(flagged["dist"], mirrored["dist"]) and np.array_equal(flagged["face"], mirrored["face"])
    # the mirrored vertices keep the face order, so their orientation is reversed: the flag's negation undoes exactly that
    assert np.array_equal(flagged["wind"], -mirrored["wind"])
    v, f = CR.icosphere(1)
    centre = CR.mesh_contact(_side([[0.0, 0.0, 0.0]]), _side(0.05 * v, f, flip=True))["wind"][0, 0]
    assert abs(centre - 1.0) < 1e-12, "a mirrored closed mesh still has its inside inside"
    del rng


def test_skip_rules():
    for B in (1, 3):
        q, t = CR.degenerate_case(B, False, False)
        ref = CR.mesh_contact(q, t)
        assert not any(np.isnan(ref[k]).any() for k in ("dist", "wind", "D"))
        # the faces on the NaN vertex, the two with an index out of range: skipped; the segment and the point: measured
        bad = (t["faces"] == 5).any(1) | (np.arange(80) == 11) | (np.arange(80) == 12)
        assert np.isinf(ref["D"][:, :, bad]).all() and np.isfinite(ref["D"][:, 0][:, ~bad]).all()
        assert np.isinf(ref["dist"][:, 2]).all() and (ref["face"][:, 2] == -1).all() and (ref["wind"][:, 2] == 0).all()
        assert np.isinf(ref["dist"][0, 9]) and np.isfinite(ref["dist"][1:, 9]).all()
        # the point face's distance is the distance to its vertex; the same mesh without the two zero-area faces has the same winding number
        tv = CR.view_space(t["verts"], t["cam_R"], t["cam_T"], False)
        qv = CR.view_space(q["verts"], q["cam_R"], q["cam_T"], False)
        want = np.linalg.norm(qv[:, 0] - tv[:, t["faces"][7, 0]], axis=-1)
        assert np.allclose(ref["D"][:, 0, 7], want, rtol=0, atol=1e-15)
        seg = CR._segment(qv[:, 0], tv[:, t["faces"][3, 0]], tv[:, t["faces"][3, 2]] - tv[:, t["faces"][3, 0]])
        assert np.allclose(ref["D"][:, 0, 3], seg, rtol=0, atol=1e-15)
        keep = np.ones(80, bool)
        keep[[3, 7]] = False
        assert np.allclose(CR.mesh_contact(q, dict(t, faces=t["faces"][keep]))["wind"], ref["wind"], rtol=0, atol=1e-14)      # (78 terms or 80)
    # max_dist: beyond it (+inf, -1, 0), within it untouched
    q, t = CR.make_pair(41, 1, 130, "ico2")
    full, cut = CR.mesh_contact(q, t), CR.mesh_contact(q, t, 0.02)
    near = full["dist"] <= 0.02
    assert 0 < near.sum() < near.size
    assert np.isinf(cut["dist"][~near]).all() and (cut["face"][~near] == -1).all() and (cut["wind"][~near] == 0).all()
    assert all(np.array_equal(cut[k][near], full[k][near]) for k in ("dist", "face", "wind"))


def test_the_gpu_cases_leave_few_vertices_undecided():
    """tests/test_gpu_contact.py lets a vertex within the distance bound of max_dist be finite or +inf, and compares the inside flag
    only where |wind64 - 0.5| >= 0.05: both exclusions stay under 2 % of the vertices of every case"""
    worst_d = worst_w = 0.0
    for B in (1, 3):
        for Vq in CR.QUERY_V:
            for name, q, t in CR.grid_cases(B, Vq):
                ref = CR.mesh_contact(q, t)
                n = ref["d_min"].size
                for md in CR.MAX_DISTS:
                    u = int(CR.undecided(ref, md).sum())
                    assert u <= 0.02 * n, (name, md, u, n)
                    worst_d = max(worst_d, u / n)
                band = int((np.abs(ref["wind_all"] - 0.5) < CR.INSIDE_BAND).sum())
                assert band <= 0.02 * n, (name, band, n)
                worst_w = max(worst_w, band / n)
    print(f"[contact cases] largest undecided share {worst_d:.2%} (distance), {worst_w:.2%} (inside flag)")


def test_compose_contact_with_meshes_of_different_sizes():
    """playback.player.compose_contact on CPU tensors (pure torch): three players whose meshes have 5, 40 and 9 faces — every part table
    is indexed by its own player's faces only —, the lower player wins a tie, a pair beyond max_dist never wins, the sign is the winner's
    winding number's, and no returned tensor is a view of the pairwise buffers"""
    import torch
    from harp_amd.playback.player import compose_contact
    rng = np.random.default_rng(5)
    F, V, n = (5, 40, 9), (7, 6, 4), 2
    tabs = [torch.from_numpy(rng.integers(1, 17, size=f).astype(np.uint8)) for f in F]
    pairs = []
    for k in range(3):
        mine = {}
        for j in range(3):
            if j != k:
                d = rng.uniform(0.0, 0.02, size=(n, V[k])).astype(np.float32)
                f = rng.integers(0, F[j], size=(n, V[k])).astype(np.int32)
                f[0, 0] = F[j] - 1                                              # the last face of every mesh occurs
                w = rng.uniform(-0.2, 1.2, size=(n, V[k])).astype(np.float32)
                far = rng.uniform(size=d.shape) < 0.3
                d[far], f[far], w[far] = np.inf, -1, 0.0
                mine[j] = [d, f, w]
        a, b = sorted(mine)
        mine[b][0][1, 1], mine[b][1][1, 1] = mine[a][0][1, 1], 0                # a tie between the two others: the lower player wins
        mine[a][0][1, 2], mine[a][1][1, 2], mine[a][2][1, 2] = np.inf, -1, 0.0  # none at all
        mine[b][0][1, 2], mine[b][1][1, 2], mine[b][2][1, 2] = np.inf, -1, 0.0
        pairs.append({j: tuple(torch.from_numpy(x) for x in v) for j, v in mine.items()})
    kept = [{j: tuple(x.clone() for x in v) for j, v in mine.items()} for mine in pairs]
    c = compose_contact(pairs, tabs)
    for k in range(3):
        a, b = sorted(pairs[k])
        for r in range(n):
            for i in range(V[k]):
                cand = [(float(pairs[k][j][0][r, i]), j) for j in (a, b)]
                dmin, j = min(cand)                                             # (of equal distances the lower player)
                if np.isinf(dmin):
                    want = (np.inf, 0, -1, 0, 0.0)
                else:
                    fj, wj = int(pairs[k][j][1][r, i]), float(pairs[k][j][2][r, i])
                    want = (-dmin if wj > 0.5 else dmin, j + 1, fj, int(tabs[j][fj]), wj)
                got = (float(c.dist[k][r, i]), int(c.other[k][r, i]), int(c.face[k][r, i]), int(c.part[k][r, i]), float(c.wind[k][r, i]))
                assert got == want, (k, r, i, got, want)
        assert c.dist[k].dtype == torch.float32 and c.other[k].dtype == torch.uint8 and c.face[k].dtype == torch.int32
        assert c.part[k].dtype == torch.uint8 and c.wind[k].dtype == torch.float32
    alld = torch.cat(c.dist, 1)
    assert torch.equal(c.min_dist, alld.amin(1)) and torch.equal(c.max_penetration, (-alld).clamp(min=0).amax(1).where(torch.cat(c.wind, 1).gt(0.5).any(1), torch.zeros(n)))
    # two players: the result owns its tensors
    two = [{1: pairs[0][1]}, {0: pairs[1][0]}]
    c2 = compose_contact(two, tabs[:2])
    before = [t.clone() for t in (c2.face[0], c2.wind[0])]
    two[0][1][1].fill_(3)
    two[0][1][2].fill_(9.0)
    assert torch.equal(c2.face[0], before[0]) and torch.equal(c2.wind[0], before[1])
    assert all(torch.equal(x, y) for mine, old in zip(pairs[1:], kept[1:]) for j in mine for x, y in zip(mine[j], old[j])), "the inputs are not written"
