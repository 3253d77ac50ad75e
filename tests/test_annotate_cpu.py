"""CPU checks of labelled playback (harp_amd/playback/labels.py, csrc/annotate.hip): the part tables on the real hand and
arm templates, the float64 yardstick tests/_annotate_ref.py against what it restates — its projection against project_pixels, its owner
against tests/_layers_ref.py's, its vote rules on hand-written blocks —, the seeded keypoint inputs of tests/test_gpu_annotate.py within
the cap on undecidable joints, the command line's switches, and the two entry points' argument errors, which return before any launch."""
import ctypes
import os

import numpy as np
import pytest

from tests import _annotate_ref as AR
from tests import _layers_ref as LR

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "harp_amd", "assets")
UNDECIDABLE_CAP = 0.02                                 # the share of joints test_gpu_annotate.py may skip


@pytest.mark.parametrize("name,V0,NJ", [("hand_template", 778, 16), ("arm_template", 1026, 55)])
def test_part_tables_on_the_templates(name, V0, NJ):
    from harp_amd.playback.labels import face_part_labels, vertex_part_labels
    from harp_amd.topology import subdivide_topology
    faces0 = np.load(os.path.join(ASSETS, name + ".npz"))["faces0"]
    assert faces0.max() == V0 - 1
    rng = np.random.default_rng(11)
    w = rng.uniform(size=(V0, NJ)) ** 8                    # peaked, as skinning weights are
    w[rng.integers(0, V0, size=50)] = 0.0                  # all-equal rows: the tie goes to joint 0
    rows = rng.integers(0, V0, size=50)
    w[rows, 5], w[rows, 9] = 2.0, 2.0                      # an exact tie of two joints: the lower one
    tab = face_part_labels(w, faces0, V0)
    F0 = faces0.shape[0]
    assert tab.dtype == np.uint8 and tab.shape == (4 * F0,) == (subdivide_topology(faces0, V0)[1].shape[0],)
    assert tab.min() >= 1 and tab.max() <= NJ
    vp = vertex_part_labels(w)
    assert (vp[rows] == 6).all() and np.array_equal(vp, 1 + np.array([int(np.flatnonzero(r == r.max())[0]) for r in w]))
    for k in range(3):                                     # sub-face i + k F0 has base corner k as its first vertex, and that corner's part
        assert np.array_equal(subdivide_topology(faces0, V0)[1][k * F0:(k + 1) * F0, 0], faces0[:, k])
        assert np.array_equal(tab[k * F0:(k + 1) * F0], vp[faces0[:, k]])
    c = vp[faces0]
    for i in rng.integers(0, F0, size=200):
        vals, counts = np.unique(c[i], return_counts=True)
        assert tab[3 * F0 + i] == (vals[np.argmax(counts)] if counts.max() > 1 else c[i, 0])


def test_centre_rule_by_hand():
    from harp_amd.playback.labels import face_part_labels, joint_part_names
    eye = np.eye(4)
    f = np.array([[0, 1, 2]])
    assert face_part_labels(eye[[2, 0, 3]], f, 3).tolist() == [3, 1, 4, 3]          # three different parts: corner 0's
    assert face_part_labels(eye[[2, 0, 0]], f, 3).tolist() == [3, 1, 1, 1]          # 2 : 1 against corner 0
    assert face_part_labels(eye[[2, 0, 2]], f, 3).tolist() == [3, 1, 3, 3]
    assert face_part_labels(eye[[2, 2, 0]], f, 3).tolist() == [3, 3, 1, 3]
    with pytest.raises(ValueError):
        face_part_labels(eye[:3], np.array([[0, 1, 3]]), 3)
    assert len(joint_part_names(16)) == 17 and joint_part_names(16)[1] == "wrist" and joint_part_names(55)[22] == "right_wrist"
    assert len(joint_part_names(55)) == 56 and joint_part_names(7) == ["background"] + [f"joint{j}" for j in range(7)]


def test_reference_projection_is_project_pixels():
    from harp_amd.playback.keypoints import camera_tz, project_pixels
    rng = np.random.default_rng(5)
    B, S, focal = 6, 64, 110.0
    j = rng.uniform(-0.1, 0.1, size=(B, 21, 3)).astype(np.float32)
    cam = np.concatenate([rng.uniform(3.0, 6.0, size=(B, 1)), rng.uniform(-0.03, 0.03, size=(B, 2))], 1)
    R = np.tile(np.array([-1, 0, 0, 0, -1, 0, 0, 0, 1], np.float64), (B, 1))
    T = np.stack([-cam[:, 1], -cam[:, 2], camera_tz(cam, focal, S)], 1)
    # float64 camera rows straight into the formula (project() rounds its inputs to float32, which the comparison must not see)
    view = np.einsum("bji,bik->bjk", j.astype(np.float64), R.reshape(B, 3, 3)) + T[:, None]
    uvz = np.stack([S / 2.0 - focal * view[..., 0] / view[..., 2], S / 2.0 - focal * view[..., 1] / view[..., 2], view[..., 2]], -1)
    want = project_pixels(j, cam, focal, S)
    assert np.abs(uvz[..., :2] - want[..., :2]).max() < 1e-12
    assert np.abs((uvz[..., 2] - uvz[:, :1, 2]) - want[..., 2]).max() < 1e-12
    # and project() itself is that formula on float32-representable inputs
    T32 = T.astype(np.float32)
    got = AR.project(j, R, T32, focal, S)
    view = np.einsum("bji,bik->bjk", j.astype(np.float64), R.reshape(B, 3, 3)) + T32.astype(np.float64)[:, None]
    assert np.abs(got[..., 0] - (S / 2.0 - focal * view[..., 0] / view[..., 2])).max() < 1e-12 and np.array_equal(got[..., 2], view[..., 2])


@pytest.mark.parametrize("ss", [1, 2])
def test_seeded_keypoint_inputs_are_decidable_and_cover_the_cases(ss):
    c = AR.keypoint_case(ss)
    seen = set()
    for self_layer in (0, 1):
        r = AR.keypoint_visibility(c["joints"], c["R"], c["T"], AR.KP_FOCAL, AR.KP_S, ss, self_layer, c["zs"], AR.KP_FLIPS, c["scene_z"], None, 0.02)
        share = float((~r["decidable"]).mean())
        print(f"[keypoints] ss={ss} self_layer={self_layer}: {share:.2%} of the joints undecidable in float32")
        assert share <= UNDECIDABLE_CAP
        vis = r["vis"]
        seen |= {(int(a), int(b) if b in (0, 255) else ("self" if b == 1 + self_layer else "other")) for a, b in vis.reshape(-1, 2)}
        assert (vis[:, 3] == 0).all() and (vis[:, 7] == 0).all() and (r["uvz"][:, 7] == 0).all() and (r["uvz"][:, 3, 2] > 0.4).all()
        if AR.KP_FLIPS[self_layer]:                        # the flipped player's joints are mirrored in u
            plain = AR.project(c["joints"], c["R"], c["T"], AR.KP_FOCAL, AR.KP_S)
            keep = np.arange(AR.KP_NJ) != 7
            assert np.allclose(r["uvz"][:, keep, 0], AR.KP_S - plain[:, keep, 0], rtol=0, atol=1e-12)
    assert seen >= {(0, 0), (2, 0), (1, "self"), (1, "other"), (1, 255)}, seen


def test_reference_owner_is_the_composite_reference():
    rng = np.random.default_rng(77)
    for ss, L, kind in [(1, 1, "none"), (2, 2, "one"), (3, 4, "rows"), (4, 3, "per_row")]:
        B, S = 2, 5
        lay = AR.label_case(rng, L, B, S, ss)
        flips = [bool(f) for f in rng.integers(0, 2, size=L)]
        for l, f in zip(lay, flips):
            l["flip"] = f
        sz, rows = AR.scene_case(rng, kind, B, S)
        got = AR.annotate_layers(lay, ss, sz, rows)
        rgb = np.zeros((B, S * ss, S * ss, 3), np.float32)
        ref = LR.composite_layers([(rgb, l["zbuf"], l["flip"]) for l in lay], ss, sz, rows)
        assert np.array_equal(got["owner"], ref["owner"]), (ss, L, kind)
        assert ((got["part"] > 0) <= (got["owner"] > 0)).all() and ((got["face"] >= 0) <= (got["owner"] > 0)).all()


def test_vote_rules_by_hand():
    n = (-1, 0, 0.0, -1)                                    # a sub-sample without a winner
    # 2 x 2, an owner tie 2 : 2 -> the lower layer; its two labels tie 1 : 1 -> the lower label; the representative is that sample
    assert AR.vote([(1, 3, 0.5, 10), (0, 7, 0.9, 11), (1, 3, 0.4, 12), (0, 5, 0.8, 13)]) == (1, 5, 3)
    # layer 1 has more samples; label 4 twice against label 2 once; of the two the nearer
    assert AR.vote([(1, 4, 0.6, 1), (1, 2, 0.1, 2), (1, 4, 0.5, 3), (0, 9, 0.2, 4)]) == (2, 4, 2)
    # a z tie among the label's samples: the first in row-major order
    assert AR.vote([n, (0, 2, 0.5, 8), (0, 2, 0.5, 9), n]) == (1, 2, 1)
    assert AR.vote([n, n, n, n]) == (0, 0, -1)
    # 4 x 4: layer 2 wins 6, layers 0 and 1 five each; labels 1 and 2 three each -> label 1; depths 0.3, 0.2, 0.2 -> the first 0.2
    block = [(2, 2, 0.1, 0), (0, 1, 0.1, 1), (2, 1, 0.3, 2), (1, 1, 0.1, 3),
             (2, 2, 0.1, 4), (0, 1, 0.1, 5), (2, 1, 0.2, 6), (1, 1, 0.1, 7),
             (2, 2, 0.1, 8), (0, 1, 0.1, 9), (2, 1, 0.2, 10), (1, 1, 0.1, 11),
             (0, 1, 0.1, 12), (0, 1, 0.1, 13), (1, 1, 0.1, 14), (1, 1, 0.1, 15)]
    assert AR.vote(block) == (3, 1, 6)
    # the same rules through annotate_layers: one pixel at ss = 2, two layers, the second flipped
    z0 = np.array([[[0.5, -1.0], [0.5, 0.7]]], np.float32)
    z1 = np.array([[[0.4, 0.6], [-1.0, 0.3]]], np.float32)      # read mirrored: [[0.6, 0.4], [0.3, -1]]
    f0 = np.array([[[0, -1], [1, 2]]], np.int32)
    f1 = np.array([[[3, 4], [-1, 5]]], np.int32)                # mirrored: [[4, 3], [5, -1]]
    lab = np.array([1, 2, 2, 9, 9, 8], np.uint8)
    r = AR.annotate_layers([dict(zbuf=z0, face_id=f0, face_label=lab, flip=False), dict(zbuf=z1, face_id=f1, face_label=lab, flip=True)], 2)
    # winners: (0,0) layer 0 at 0.5 (0.6 is farther); (0,1) layer 1 at 0.4, face 3; (1,0) layer 1 at 0.3, face 5; (1,1) layer 0 at 0.7, face 2
    # 2 : 2 -> layer 0; its labels 1 and 2 tie -> 1; face 0 at 0.5
    assert (r["owner"][0, 0, 0], r["part"][0, 0, 0], r["face"][0, 0, 0], r["depth"][0, 0, 0]) == (1, 1, 0, 0.5)
    assert r["bbox"].tolist() == [[[0, 0, 0, 0], [-1, -1, -1, -1]]]


def test_command_line_switches():
    from harp_amd.playback import cli
    base = ["--config", "c.yaml", "--motion", "m.npz", "--out", "o"]
    a = cli.parse_args(base)
    assert a.labels is False and a.label_tol == 0.02
    a = cli.parse_args(base + ["--labels", "--label-tol", "0.01"])
    assert a.labels is True and a.label_tol == 0.01
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--labels", "--label-tol", "-1"])


def test_entry_points_refuse_bad_arguments_without_launch():
    """every HARP_ERR_ARG exit of the two entries on fake pointers: a legal call would launch (no device here: a status >= 2), each broken
    argument returns 1 before that"""
    import torch
    from harp_amd import _lib, build
    if torch.cuda.is_available():
        pytest.skip("fake pointers: an entry point that lost a check would launch on them")
    build.build(force=False, verbose=False)
    L, f = _lib.lib(), 1 << 20
    full = lambda **kw: _lib.LabelLayer(**dict(dict(face_id=f, zbuf=f, face_label=f, ndc=f, faces=f, verts_uvs=f, faces_uvs=f, V=9, F=8, Vt=12,      # noqa: E731
                                                    flip_x=0, reserved=0), **kw))
    arr = lambda *ls: (_lib.LabelLayer * len(ls))(*ls)      # noqa: E731

    def annotate(layers=None, n=1, B=2, S=8, ss=2, scene=(None, 0, None), outs=(f, f, f, f, f, f)):
        return L.harp_annotate_layers(arr(full()) if layers is None else layers, n, B, S, ss, *scene, *outs, None)

    assert annotate() >= 2
    assert annotate(outs=(f, None, None, None, None, None)) >= 2
    bad = [dict(n=0), dict(n=5), dict(B=0), dict(S=0), dict(ss=0), dict(ss=5), dict(S=20000, ss=4), dict(outs=(None,) * 6),
           dict(scene=(f, 0, None)), dict(scene=(f, 3, None)), dict(layers=arr(full(face_id=None))), dict(layers=arr(full(zbuf=None))),
           dict(layers=arr(full(face_label=None))), dict(layers=arr(full(F=0))), dict(layers=arr(full(reserved=1))),
           dict(layers=arr(full(ndc=None))), dict(layers=arr(full(faces=None))), dict(layers=arr(full(verts_uvs=None))),
           dict(layers=arr(full(faces_uvs=None))), dict(layers=arr(full(V=0))), dict(layers=arr(full(Vt=0))),
           dict(layers=arr(full(), full(zbuf=None)), n=2)]
    for kw in bad:
        assert annotate(**kw) == 1, kw
    assert L.harp_annotate_layers(None, 1, 2, 8, 2, None, 0, None, f, f, f, f, f, f, None) == 1
    # the uv tables may be NULL without the uv output
    assert annotate(layers=arr(full(ndc=None, faces=None, verts_uvs=None, faces_uvs=None, V=0, Vt=0)), outs=(f, f, f, f, None, f)) >= 2

    def keypoints(j=f, R=f, T=f, B=2, NJ=21, focal=100.0, S=8, ss=2, self_layer=0, layers=None, n=1, scene=(None, 0, None), tol=0.02, uvz=f, vis=f):
        return L.harp_keypoint_visibility(j, R, T, B, NJ, focal, S, ss, self_layer, arr(full()) if layers is None else layers, n, *scene, tol, uvz, vis, None)

    assert keypoints() >= 2
    assert keypoints(layers=arr(full(face_id=None, face_label=None, F=0))) >= 2         # only zbuf and flip_x are read
    bad = [dict(j=None), dict(R=None), dict(T=None), dict(uvz=None), dict(vis=None), dict(B=0), dict(NJ=0), dict(S=0), dict(ss=0), dict(ss=5),
           dict(S=20000, ss=4), dict(n=0), dict(n=5), dict(self_layer=-1), dict(self_layer=1), dict(focal=0.0), dict(focal=float("nan")),
           dict(tol=-0.01), dict(tol=float("nan")), dict(scene=(f, 3, None)), dict(layers=arr(full(zbuf=None))), dict(layers=arr(full(reserved=2)))]
    for kw in bad:
        assert keypoints(**kw) == 1, kw
    assert L.harp_keypoint_visibility(f, f, f, 2, 21, 100.0, 8, 2, 0, None, 1, None, 0, None, 0.02, f, f, None) == 1


def test_label_layer_struct_matches_c(tmp_path):
    import subprocess
    from harp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(harp_label_layer),'
                   'offsetof(harp_label_layer, faces_uvs), offsetof(harp_label_layer, V), offsetof(harp_label_layer, flip_x),'
                   'offsetof(harp_label_layer, reserved)); return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "layout")]).split()]
    LL = _lib.LabelLayer
    assert got == [ctypes.sizeof(LL), LL.faces_uvs.offset, LL.V.offset, LL.flip_x.offset, LL.reserved.offset]
