"""CPU checks of the UV bake (csrc/bake.hip): the float64 restatement tests/_bake_ref.py against closed forms, the undecidable caps on
the committed cases, the ABI's argument checks (no launch), the ctypes mirror of harp_bake_args, the dilation workspace arithmetic and
the argument errors of the fit's `texture_init`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _bake_cases as C
from tests import _bake_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


# ---- the reference against closed forms
def _bake_quad(sc, y_true, **kw):
    tf, tb, _ = R.texel_map(sc["verts_uvs"], sc["faces_uvs"], sc["Ht"], sc["Wt"])
    acc = R.new_accumulators(sc["Ht"], sc["Wt"])
    B = sc["ndc"].shape[0]
    info = R.accumulate(acc, tf, tb, sc["faces"], sc["ndc"], sc["face_id"], sc["zbuf"], y_true, np.ones(y_true.shape[:3], dtype=np.float32),
                        np.arange(B, dtype=np.int32), **kw)
    return tf, acc, info


@pytest.mark.parametrize("flip", [False, True])
def test_reference_resamples_a_fronto_parallel_quad(flip):
    """The whole atlas on a quad facing the camera; the image is linear in the pixel coordinates, so its bilinear resampling is exact:
    texel (tx, ty) = (u, v) = (tx / (Wt - 1), 1 - ty / (Ht - 1)) sits at x_ndc = -e + 2 e u (mirrored with flip), y_ndc = -e + 2 e v, i.e.
    at the continuous pixel (1 - x_ndc) S / 2 - 0.5, and must read a + b px + c py there.  A flipped axis anywhere in the chain fails."""
    S, Ht, Wt, e = 32, 17, 33, 0.5
    sc = R.textured_quad_scene(S=S, Ht=Ht, Wt=Wt, extent=e, flip=flip)
    py, px = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    coef = np.array([[0.2, 0.010, 0.004], [0.7, -0.008, 0.002], [0.4, 0.003, -0.006]])
    y_true = np.stack([a + b * px + c * py for a, b, c in coef], -1)[None].astype(np.float32)
    tf, acc, info = _bake_quad(sc, y_true)
    # (the outermost texels sit on the quad's silhouette, i.e. on a pixel boundary: the pixel beyond it is empty)
    inner = np.zeros((Ht, Wt), dtype=bool)
    inner[1:-1, 1:-1] = True
    assert (tf >= 0).all() and info["observed"][0].reshape(Ht, Wt)[inner].all()
    ty, tx = np.meshgrid(np.arange(Ht, dtype=np.float64), np.arange(Wt, dtype=np.float64), indexing="ij")
    u, v = tx / (Wt - 1), 1.0 - ty / (Ht - 1)
    xn, yn = (-e + 2 * e * u) * (-1.0 if flip else 1.0), -e + 2 * e * v
    cx, cy = (1.0 - xn) * S / 2 - 0.5, (1.0 - yn) * S / 2 - 0.5
    want = np.stack([a + b * cx + c * cy for a, b, c in coef], -1)
    mean, var, seen = R.finish(acc)
    assert seen[inner].all() and (acc["count"][inner] == 1).all() and (acc["sum_w"][inner] == 1.0).all()
    assert np.abs(mean - want)[inner].max() < 2e-6, np.abs(mean - want)[inner].max()       # float32 image values, float32 result
    assert var.max() < 1e-6


def test_reference_never_observes_a_quad_behind_another():
    """two quads over the same pixels, each with half of the atlas: the hard pass saw the front one, the texels of the other stay empty"""
    S, Ht, Wt = 32, 17, 33
    verts_uvs = np.array([[0, 0], [0.5, 0], [0.5, 1], [0, 1], [0.5, 0], [1, 0], [1, 1], [0.5, 1]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int32)
    sq = lambda z: [[-0.5, -0.5, z], [0.5, -0.5, z], [0.5, 0.5, z], [-0.5, 0.5, z]]      # noqa: E731
    ndc = np.array([sq(2.0) + sq(2.5)], dtype=np.float32)
    c = -1.0 + (2.0 * (S - 1 - np.arange(S)) + 1.0) / S
    inside = (np.abs(c)[None, :] <= 0.6) & (np.abs(c)[:, None] <= 0.6)         # (a pixel wider than the quads: their rims are covered too)
    sc = dict(verts_uvs=verts_uvs, faces_uvs=faces, faces=faces, ndc=ndc, Ht=Ht, Wt=Wt, face_id=np.where(inside, 0, -1).astype(np.int32)[None],
              zbuf=np.where(inside, 2.0, -1.0).astype(np.float32)[None])
    tf, acc, info = _bake_quad(sc, np.full((1, S, S, 3), 0.5, dtype=np.float32))
    front, back = (tf == 0) | (tf == 1), (tf == 2) | (tf == 3)
    assert front.sum() > 100 and back.sum() > 100
    assert (acc["count"][front] == 1).all() and (acc["count"][back & ~front] == 0).all()
    assert info["reasons"]["occluded"] == int(back.sum()) and R.finish(acc)[2][back].sum() == 0


def test_reference_dilate_closed_form():
    tex = np.zeros((5, 7, 1), dtype=np.float32)
    tex[2, 3] = 4.0
    valid = np.zeros((5, 7), dtype=np.uint8)
    valid[2, 3] = 1
    out, v = R.dilate(tex, valid, 1)
    assert v.sum() == 9 and (out[1:4, 2:5] == 4.0).all() and out.sum() == 36.0
    out, v = R.dilate(tex, valid, 2)
    assert v.sum() == 25 and (out[0:5, 1:6] == 4.0).all()                       # means of equal values
    out0, v0 = R.dilate(tex, valid, 0)
    assert (out0 == tex).all() and (v0 == valid).all()


# ---- the caps on the undecidable items of the committed cases (conditions of the GPU comparisons)
@pytest.mark.parametrize("Ht,Wt", C.HAND_ATLASES)
def test_texel_map_undecidable_cap(Ht, Wt):
    face, _, und = C.hand_texel_map(Ht, Wt)
    covered = face >= 0
    share = (und & covered).sum() / covered.sum()
    print(f"[bake] hand template {Ht} x {Wt}: {covered.sum()} covered texels, {und.sum()} undecidable")
    assert covered.sum() > 0.2 * Ht * Wt and share <= 0.005


@pytest.mark.parametrize("name", list(C.ACCUM_CASES))
def test_accumulate_cases_hit_their_branches_under_the_cap(name):
    case = C.accum_case(name)
    acc, info = C.accum_reference(name)
    seen_any = info["observed"].any(0)
    share = (info["undecided"] & seen_any).sum() / max(1, seen_any.sum())
    print(f"[bake] case {name}: {seen_any.sum()} texels observed, {info['undecided'].sum()} undecidable, rejected {info['reasons']}")
    assert seen_any.sum() >= 50
    assert share <= 0.02
    for reason in case["expect"]:
        assert info["reasons"][reason] > 0, reason
    n_tri = case["faces"].shape[0]
    assert 2 <= n_tri <= 8 and case["S"] in (32, 48) and case["B"] in (1, 3, 6)


def test_uv_cases_are_exact_in_float32():
    for name in C.UV_CASES:
        vu, _ = C.uv_case(name)
        for Ht, Wt in C.UV_ATLASES:
            P = R.texel_coords(vu, Ht, Wt)
            assert (P * 2 == np.round(P * 2)).all(), name                       # half-integers at most: products of differences are exact


# ---- ABI
def test_entry_points_refuse_bad_arguments_without_launch(lib):
    """HARP_ERR_ARG (1) before any launch.  Where a device is visible, fake pointers are only passed together with sizes whose grid would
    be empty (a failed launch, status >= 2) if the check were missing, so no kernel can ever reach them (tests/test_abi.py:71-75).  The
    NULL-pointer and parameter cases prove something only with legal sizes: they get them where no device is visible (a lost check then
    shows as a failed launch, a status other than 1, and nothing can run) and the empty sizes elsewhere.  The parameter refusals whose
    grid is not empty are checked once more on real buffers in tests/test_gpu_bake.py."""
    import torch
    from harp_amd import _lib
    f = 1 << 20
    legal = not torch.cuda.is_available()
    # texel map: grid = (Ht * Wt + 255) / 256 is empty for Ht = 0 / Wt = 0
    for Ht, Wt in [(0, 17), (17, 0)]:
        assert lib.harp_uv_texel_map(f, f, 2, 4, Ht, Wt, f, f, None) == 1
    for args in [(None, f, f, f), (f, None, f, f), (f, f, None, f), (f, f, f, None)]:
        assert lib.harp_uv_texel_map(args[0], args[1], 2, 4, 17 if legal else 0, 17 if legal else 0, args[2], args[3], None) == 1
    # finish / dilate: empty atlas
    for Ht, Wt in [(0, 5), (5, 0), (-1, 5)]:
        assert lib.harp_texture_bake_finish(f, f, f, f, Ht, Wt, 1, f, f, f, None) == 1
        assert lib.harp_texture_dilate(f, f, None, Ht, Wt, 3, 1, f, None, f, None) == 1
    # ... their NULL pointers and parameters (var, allow and valid_out may be NULL); with a device only together with the empty atlas
    H = 5 if legal else 0
    if legal:                                                                       # legal: as far as the launch (no device here)
        assert lib.harp_texture_bake_finish(f, f, f, f, H, 5, 1, f, None, f, None) >= 2
        assert lib.harp_texture_dilate(f, f, None, H, 5, 3, 1, f, None, f, None) >= 2
    for k in (0, 1, 2, 3, 7, 9):                                                    # sum_w, sum_wc, sum_wc2, count, mean, seen
        a = [f, f, f, f, H, 5, 1, f, f, f, None]
        a[k] = None
        assert lib.harp_texture_bake_finish(*a) == 1, k
    for k in (0, 1, 7):                                                             # tex, valid, out
        a = [f, f, f, H, 5, 3, 1, f, f, f, None]
        a[k] = None
        assert lib.harp_texture_dilate(*a) == 1, k
    assert lib.harp_texture_dilate(f, f, f, H, 5, 3, 1, f, f, None, None) == 1      # n_pass > 0 without a workspace
    for Cn, n_pass in [(0, 1), (5, 1), (-1, 1), (3, -1)]:
        assert lib.harp_texture_dilate(f, f, f, H, 5, Cn, n_pass, f, f, f, None) == 1, (Cn, n_pass)
    # accumulate: n = 0 gives an empty grid
    def args(**kw):
        a = _lib.BakeArgs(**{n: f for n, t in _lib.BakeArgs._fields_ if t is ctypes.c_void_p})
        a.n, a.Ht, a.Wt, a.F, a.V, a.B, a.S, a.N = (64 if legal else 0), 8, 8, 2, 4, 1, 16, 1
        a.depth_tol, a.cos_min, a.cos_power, a.shade_floor = 4e-3, 0.2, 2.0, 0.1
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.harp_texture_bake_accum(ctypes.byref(args(n=0)), None) == 1
    if legal:
        assert lib.harp_texture_bake_accum(ctypes.byref(args()), None) >= 2         # legal: it gets as far as the launch (no device here)
    assert lib.harp_texture_bake_accum(None, None) == 1
    for name in ("texel_face", "texel_bary", "faces", "ndc", "face_id", "zbuf", "y_true", "y_mask", "rows", "sum_w", "sum_wc", "sum_wc2",
                 "count", "best_cos"):
        assert lib.harp_texture_bake_accum(ctypes.byref(args(**{name: None})), None) == 1, name
    for kw in (dict(verts=None), dict(cam_pos=None), dict(colors=None), dict(verts=None, vnormals=None, cam_pos=None),
               dict(depth_tol=-1.0), dict(shade_floor=0.0), dict(cos_power=-1.0), dict(cos_min=float("nan")), dict(B=0), dict(S=0), dict(Ht=1)):
        assert lib.harp_texture_bake_accum(ctypes.byref(args(**kw)), None) == 1, kw


def test_ops_have_no_cpu_path(lib):
    import torch
    from harp_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.uv_texel_map(torch.zeros(3, 2), torch.zeros(1, 3, dtype=torch.int32), 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.texture_dilate(torch.zeros(4, 4, 3), torch.zeros(4, 4, dtype=torch.uint8), 1)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.texture_dilate(torch.zeros(4, 4, 3, requires_grad=True), torch.zeros(4, 4, dtype=torch.uint8), 1)


def test_bake_args_layout_matches_c(tmp_path):
    from harp_amd import _lib
    fields = [n for n, _ in _lib.BakeArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu", sizeof(harp_bake_args));\n' +
                   "".join(f'printf(" %zu", offsetof(harp_bake_args, {n}));\n' for n in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(_lib.BakeArgs)] + [getattr(_lib.BakeArgs, n).offset for n in fields]
    assert got == want, (got, want)


def test_dilate_ws_bytes(lib):
    r = lambda n: (n + 255) // 256 * 256      # noqa: E731
    for Ht, Wt, Cn in [(17, 17, 1), (33, 17, 3), (512, 512, 3), (512, 512, 4), (1, 1, 1)]:
        assert lib.harp_texture_dilate_ws_bytes(Ht, Wt, Cn) == 2 * r(4 * Cn * Ht * Wt) + 2 * r(Ht * Wt), (Ht, Wt, Cn)
    for Ht, Wt, Cn in [(0, 5, 3), (5, 0, 3), (5, 5, 0), (5, 5, 5), (-1, 5, 3)]:
        assert lib.harp_texture_dilate_ws_bytes(Ht, Wt, Cn) == 0, (Ht, Wt, Cn)


# ---- argument errors of the fit
def test_texture_init_with_known_appearance_is_refused():
    from harp_amd.optimize_sequence import optimize_hand_sequence
    cfg = {"model_type": "harp", "known_appearance": True}
    with pytest.raises(ValueError, match="texture_init"):
        optimize_hand_sequence(cfg, None, None, None, None, None, texture_init="bake")
    with pytest.raises(ValueError, match="texture_init"):
        optimize_hand_sequence(dict(cfg, texture_init="bake"), None, None, None, None, None)
    with pytest.raises(ValueError, match="texture_init"):
        optimize_hand_sequence(dict(cfg, known_appearance=False), None, None, None, None, None, texture_init="projective")
