"""Motion labels without a device: the float64 restatement of harp_flow_layers (tests/_flow_ref.py) against cases whose
answer is known in closed form, the seeded cases' coverage and their undecidable share, the .flo files, the struct's layout and the
binding's refusal of CPU tensors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _annotate_ref as AR
from tests import _flow_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDECIDABLE_CAP = 0.02


def _quad(B, z=0.5, half=0.5):
    """a fronto-parallel square of two triangles at constant depth"""
    xy = np.array([[-half, -half], [half, -half], [half, half], [-half, half]])
    ndc = np.concatenate([np.tile(xy, (B, 1, 1)), np.full((B, 4, 1), z)], -1).astype(np.float32)
    return ndc, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _layer(ndc, faces, Sh, flip=False):
    fid, zbuf = FR.rasterize(ndc, faces, Sh)
    return dict(face_id=fid, zbuf=zbuf, face_label=np.ones(faces.shape[0], np.uint8), flip=flip, ndc=ndc, faces=faces)


@pytest.mark.parametrize("ss", [1, 2, 3])
def test_identity(ss):
    rng = np.random.default_rng(50 + ss)
    c = FR.flow_case(rng, 2, 2, 8, ss, "none", corrupt=False)
    to = [dict(ndc=l["ndc"], zbuf=l["zbuf"]) for l in c["layers"]]
    r = FR.flow_layers(c["layers"], to, ss)
    own = AR.annotate_layers(c["layers"], ss)["owner"] > 0
    assert own.sum() > 50 and np.array_equal(r["status"][..., 0] > 0, own)
    assert np.abs(r["flow"]).max() <= 1e-12 and np.abs(r["dz"]).max() <= 1e-6
    assert (r["status"][own] == (4, 0)).all() and not r["status"][~own].any()


@pytest.mark.parametrize("ss,k", [(1, 2), (2, 3), (4, -5)])
def test_known_shift_and_sign(ss, k):
    S, B = 8, 1
    Sh = S * ss
    ndc, faces = _quad(B)
    moved = ndc.copy()
    moved[..., 0] -= 2.0 * k / Sh                          # k sub-pixels towards +X: x_ndc falls as the column grows
    for flip in (False, True):
        src = _layer(ndc, faces, Sh, flip)
        r = FR.flow_layers([src], [dict(ndc=moved, zbuf=FR.rasterize(moved, faces, Sh)[1])], ss)
        own = r["status"][..., 0] > 0
        assert own.sum() >= 9
        # the layer's own image moves by k sub-pixels; shown mirrored, it moves the other way
        assert np.abs(r["flow"][own][:, 0] - (-k if flip else k) / ss).max() <= 1e-12 and np.abs(r["flow"][own][:, 1]).max() <= 1e-12
        assert np.abs(r["dz"][own]).max() <= 1e-7
        assert set(np.unique(r["status"][own][:, 0]).tolist()) <= {2, 4}


def test_occluders():
    S, B, ss = 8, 1, 2
    Sh = S * ss
    far, faces = _quad(B, z=0.8)
    near, _ = _quad(B, z=0.4, half=0.9)
    l0, l1 = _layer(far, faces, Sh), _layer(near, faces, Sh)
    l1["zbuf"][:] = -1.0                                   # the near layer is absent in the source frame: layer 0 owns its pixels
    to = [dict(ndc=far, zbuf=l0["zbuf"]), dict(ndc=near, zbuf=FR.rasterize(near, faces, Sh)[1])]
    r = FR.flow_layers([l0, l1], to, ss)
    own = r["status"][..., 0] > 0
    assert own.sum() >= 9 and (r["status"][own] == (3, 2)).all()       # hidden by layer 1
    scene = np.full((1, S, S), 0.3, np.float32)
    r = FR.flow_layers([l0], to[:1], ss, scene_z_to=scene)
    assert (r["status"][own] == (3, 255)).all()                          # hidden by the target frames' scene depth
    r = FR.flow_layers([l0], to[:1], ss, scene_z=scene)
    assert not r["status"].any()                                         # in front of the SOURCE frame: nothing is owned
    pushed = dict(ndc=far, zbuf=np.where(l0["zbuf"] > 0, l0["zbuf"] - np.float32(0.02), l0["zbuf"]))
    r = FR.flow_layers([l0], [pushed], ss)
    assert (r["status"][own] == (3, 1)).all()                            # its own layer, nearer than the point by more than tol
    r = FR.flow_layers([l0], [pushed], ss, tol=0.03)
    assert (r["status"][own] == (4, 0)).all()


def test_seeded_cases_cover_every_status_within_the_undecidable_cap():
    seen, by = set(), set()
    for ss in (1, 2, 3, 4):
        skipped = owned = 0
        for L, kind, c, r in FR.seeded_cases(ss):
            own = AR.annotate_layers(c["layers"], ss, *c["scene"])["owner"] > 0
            assert np.array_equal(r["status"][..., 0] > 0, own), (ss, L, kind)
            low = r["status"][..., 0] <= 1
            assert not r["flow"][low].any() and not r["dz"][low].any()
            seen |= set(np.unique(r["status"][..., 0]).tolist())
            by |= set(np.unique(r["status"][..., 1]).tolist())
            skipped, owned = skipped + int((~r["decidable"] & own).sum()), owned + int(own.sum())
        print(f"[flow cpu] ss={ss}: {skipped} of {owned} owned pixels undecidable ({skipped / owned:.2%}; cap {UNDECIDABLE_CAP:.0%})")
        assert owned > 500 and skipped <= UNDECIDABLE_CAP * owned
    assert seen == {0, 1, 2, 3, 4} and {0, 1, 2, 255} <= by


def test_flo_round_trip(tmp_path):
    from harp_amd.io import FLO_MAGIC, FLO_UNKNOWN, load_flo, save_flo
    rng = np.random.default_rng(7)
    f = rng.normal(size=(5, 7, 2)).astype(np.float32)
    known = rng.uniform(size=(5, 7)) < 0.7
    save_flo(tmp_path / "a.flo", f, known)
    raw = open(tmp_path / "a.flo", "rb").read()
    assert raw[:4] == b"PIEH" and len(raw) == 12 + 5 * 7 * 8 and np.frombuffer(raw[4:12], "<i4").tolist() == [7, 5]
    assert np.frombuffer(raw[:4], "<f4")[0] == np.float32(FLO_MAGIC)
    g, k = load_flo(tmp_path / "a.flo")
    assert g.dtype == np.float32 and np.array_equal(k, known) and np.array_equal(g[known], f[known]) and (g[~known] == np.float32(FLO_UNKNOWN)).all()
    save_flo(tmp_path / "b.flo", f)
    g, k = load_flo(tmp_path / "b.flo")
    assert k.all() and np.array_equal(g, f)
    with pytest.raises(ValueError):
        save_flo(tmp_path / "c.flo", f[..., 0])
    (tmp_path / "d.flo").write_bytes(raw[:-4])
    with pytest.raises(ValueError):
        load_flo(tmp_path / "d.flo")
    (tmp_path / "e.flo").write_bytes(b"\0" * 20)
    with pytest.raises(ValueError):
        load_flo(tmp_path / "e.flo")


def test_flow_layer_layout_matches_c(tmp_path):
    """tests/test_abi.py test_struct_layouts_match_c for harp_flow_layer"""
    from harp_amd import _lib
    names = ("face_id", "zbuf", "face_label", "ndc", "faces", "ndc_to", "zbuf_to", "V", "F", "flip_x", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu' + " %zu" * len(names) + '\\n", sizeof(harp_flow_layer)' +
                   "".join(f", offsetof(harp_flow_layer, {n})" for n in names) + ");return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.FlowLayer)] + [getattr(_lib.FlowLayer, n).offset for n in names], got
    assert "harp_flow_layers" in _lib.SIGNATURES and len(_lib.SIGNATURES["harp_flow_layers"][1]) == 16


def test_no_cpu_path_and_cli_switches():
    from harp_amd import ops, playback
    from harp_amd.playback.cli import parse_args
    assert ops.FLOW_TOL == 0.005 and playback.FLOW_TOL == ops.FLOW_TOL
    lay = dict(face_id=torch.zeros(1, 4, 4, dtype=torch.int32), zbuf=torch.zeros(1, 4, 4), face_label=torch.ones(2, dtype=torch.uint8), flip=False,
               ndc=torch.zeros(1, 3, 3), faces=torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.flow_layers([lay], [dict(ndc=torch.zeros(1, 3, 3), zbuf=torch.zeros(1, 4, 4))], 2)
    base = ["--config", "c.yaml", "--motion", "m.npz", "--out", "o"]
    a = parse_args(base)
    assert a.flow is None and a.flow_tol == ops.FLOW_TOL
    a = parse_args(base + ["--flow", "both", "--flow-tol", "0.01"])
    assert a.flow == "both" and a.flow_tol == 0.01
    for bad in (["--flow-tol", "-1"], ["--flow-tol", "nan"], ["--flow-tol", "inf"], ["--flow", "sideways"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
