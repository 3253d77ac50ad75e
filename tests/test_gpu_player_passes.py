"""-m gpu: the two things the players' passes rest on ("What the base owns").

(a) The labels and the flow pass are written once over a player's layers, so an AvatarPlayer must be exactly a ScenePlayer of that one
player, unflipped and without a scene depth: every field of annotate(uv=True) and of flow is compared bit for bit, the avatar's bare bbox /
uvz / vis against the scene's [:, 0] / [0].  (It held before the two were written once, too: the file passes on that tree.)

(b) Every kind of pass keeps its output buffers by one rule: made on first use, dropped — with every graph — when a longer call grows the
player.  On one graph scene the four kinds are called at 3 rows, again, at 5 rows (the capacity grows from 4 to 6 padded rows) and at the
first 3 rows once more; each result is read by an in-stream clone and must equal that of a fresh eager scene that makes only that call.
The views returned by the first round are kept as well: neither a later pass's first allocation nor the growth may change them."""
import numpy as np
import pytest
import torch

from tests.test_gpu_scene_player import BATCH, T, _players, _two_hands

pytestmark = pytest.mark.gpu
KINDS = ("render", "annotate", "flow", "contact")
REACH = 1.0                                              # metres: contact's max_dist here, so that the hand behind is within reach of every vertex


def _clone(x):
    """a copy made in stream order, of (nested, named) tuples of tensors and Nones"""
    if x is None or torch.is_tensor(x):
        return x if x is None else x.clone()
    return type(x)(*map(_clone, x)) if hasattr(x, "_fields") else tuple(map(_clone, x))


def _same(a, b):
    """equal over (nested tuples of) tensors and Nones; float32 by its int32 view, so that +inf, NaN and the sign of zero count too"""
    if a is None or b is None:
        return a is None and b is None
    if not torch.is_tensor(a):
        return not torch.is_tensor(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def _differing(got, want):
    """the fields of two namedtuples that are not the same bits"""
    return [k for k in want._fields if not _same(getattr(got, k), getattr(want, k))]


@pytest.mark.parametrize("ss", [1, 2])
def test_an_avatar_is_a_scene_of_one_layer(tmp_path_factory, ss):
    from harp_amd.playback import ScenePlayer
    hand = _two_hands(tmp_path_factory)[0]
    avatar, alone = _players((hand, hand), ss, True)
    avatar.load_motion(hand[3])
    scene = ScenePlayer([alone])
    scene.load_motions([hand[3]])
    rows = np.arange(T)
    to = (rows + 2) % T
    a, s = avatar.annotate(rows, uv=True), scene.annotate(rows, uv=True)
    assert tuple(a.bbox.shape) == (T, 4) and tuple(s.bbox.shape) == (T, 1, 4) and torch.is_tensor(a.uvz) and len(s.uvz) == len(s.vis) == 1
    assert bool(a.owner.any()) and bool((a.vis[..., 0] == 2).any())
    assert _differing(a, s._replace(bbox=s.bbox[:, 0], uvz=s.uvz[0], vis=s.vis[0])) == []
    fa, fs = avatar.flow(rows, to), scene.flow(rows, to)
    assert bool((fa.status[..., 0] == 4).any()) and bool((fa.flow != 0).any())
    assert _differing(fa, fs) == []


def _scene(hands, use_graph):
    from harp_amd.playback import ScenePlayer
    scene = ScenePlayer(_players(hands, 1, True, use_graph=use_graph), flip=[False, True])
    scene.load_motions([h[3] for h in hands])
    return scene


def _call(scene, kind, rows, to):
    if kind == "render":
        return scene.render(rows, owner=True)
    if kind == "annotate":
        return scene.annotate(rows)
    if kind == "flow":
        return scene.flow(rows, to)
    return scene.contact(rows, REACH)


def test_pass_buffers_across_passes_and_growth(tmp_path_factory):
    hA, hB, _ = _two_hands(tmp_path_factory)
    short, longer = (np.array([0, 2, 4]), np.array([1, 3, 0])), (np.array([4, 3, 2, 1, 0]), np.array([0, 4, 3, 2, 1]))
    assert BATCH == 2                                      # 3 rows are padded to 4, 5 rows to 6: the second length grows the scene
    scene = _scene((hA, hB), True)
    got, views = {}, {}
    for k in KINDS:                                        # every pass's first use, behind the results of those before it
        views[k] = _call(scene, k, *short)
        got["first", k] = _clone(views[k])
    assert len(scene._graphs) == 4
    for k in KINDS:
        got["again", k] = _clone(_call(scene, k, *short))
    assert len(scene._graphs) == 4
    for i, k in enumerate(KINDS):                          # the first of these grows the scene: the four graphs go, and every pass's buffers
        got["longer", k] = _clone(_call(scene, k, *longer))
        assert len(scene._graphs) == i + 1
    for i, k in enumerate(KINDS):
        got["back", k] = _clone(_call(scene, k, *short))
        assert len(scene._graphs) == 5 + i
    torch.cuda.synchronize()
    for k in KINDS:
        want = {n: _clone(_call(_scene((hA, hB), False), k, *rows)) for n, rows in (("short", short), ("longer", longer))}
        torch.cuda.synchronize()
        for step in ("first", "again", "back"):
            assert _same(got[step, k], want["short"]), (step, k)
        assert _same(got["longer", k], want["longer"]), k
        assert _same(views[k], got["first", k]), f"the first {k}'s own tensors were changed by a later pass or by the growth"
    c = got["first", "contact"]
    assert all(bool(torch.isfinite(d).any()) for d in c.dist) and bool((got["first", "flow"].status[..., 0] == 4).any())
