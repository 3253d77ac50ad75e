"""CPU checks of scene playback (csrc/composite.hip, harp_amd/playback/player.py ScenePlayer): the float64 yardstick tests/_layers_ref.py agrees
with the yardstick of harp_resolve_u8 where the two contracts coincide and has the properties the contract promises; the entry point
refuses bad arguments before any launch; the ctypes mirror of harp_layer matches the C struct."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _layers_ref as LR
from tests import _playback_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(rng, B, Sh, hole=0.4):
    rgb = rng.uniform(-0.1, 1.1, size=(B, Sh, Sh, 3)).astype(np.float32)
    rgb.reshape(-1)[rng.integers(0, rgb.size, size=max(1, rgb.size // 50))] = np.nan
    z = rng.uniform(0.2, 1.0, size=(B, Sh, Sh)).astype(np.float32)
    z[rng.uniform(size=z.shape) < hole] = -1.0
    return rgb, z


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_yardstick_equals_the_resolve_yardstick_for_one_layer(ss):
    rng = np.random.default_rng(10 + ss)
    for S, B, channels in ((7, 3, 3), (16, 1, 4), (5, 2, 4)):
        Sh = S * ss
        rgb, _ = _layer(rng, B, Sh)
        fid = np.where(rng.uniform(size=(B, Sh, Sh)) < 0.6, rng.integers(0, 5000, size=(B, Sh, Sh)), -1).astype(np.int32)
        z = np.where(fid >= 0, 1.0, -1.0).astype(np.float32)
        bg = rng.integers(0, 256, size=(4, S, S, 3)).astype(np.uint8)
        rows = rng.integers(-1, 5, size=B).astype(np.int32)
        color = rng.uniform(0, 1, size=3).astype(np.float32)
        for kw in (dict(), dict(bg=bg, bg_rows=rows), dict(bg=bg[:1]), dict(bg=bg[:B])):
            a = LR.composite_layers([(rgb, z, False)], ss, bg_color=color, channels=channels, **kw)
            b = R.resolve_u8(rgb, fid, ss, kw.get("bg"), kw.get("bg_rows"), color, channels)
            assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["n"], b["n"]) and np.array_equal(a["v255"], b["v255"])
            assert np.array_equal(a["owner"], (b["n"] > 0).astype(np.uint8))


@pytest.mark.parametrize("ss", [1, 2, 3])
def test_yardstick_properties(ss):
    rng = np.random.default_rng(20 + ss)
    B, S = 2, 9
    Sh = S * ss
    (c0, z0), (c1, z1) = _layer(rng, B, Sh), _layer(rng, B, Sh)
    bg = rng.integers(0, 256, size=(B, S, S, 3)).astype(np.uint8)
    mir = lambda a: np.ascontiguousarray(a[:, :, ::-1])
    # flipping a layer = mirroring its arrays
    a = LR.composite_layers([(c0, z0, False), (c1, z1, True)], ss, bg=bg, channels=4)
    b = LR.composite_layers([(c0, z0, False), (mir(c1), mir(z1), False)], ss, bg=bg, channels=4)
    for k in ("out", "v255", "n", "owner"):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["out"], LR.composite_layers([(c0, z0, False), (c1, z1, False)], ss, bg=bg, channels=4)["out"])
    # equal depths everywhere: layer 0 is shown
    t = LR.composite_layers([(c0, z0, False), (c1, z0, False)], ss, bg=bg, channels=4)
    one = LR.composite_layers([(c0, z0, False)], ss, bg=bg, channels=4)
    assert np.array_equal(t["out"], one["out"]) and set(np.unique(t["owner"])) <= {0, 1} and (t["owner"] == 1).any()
    # a scene depth in front of everything: the pure background, nothing owned
    front = np.full((1, S, S), 0.1, np.float32)
    f = LR.composite_layers([(c0, z0, False), (c1, z1, True)], ss, scene_z=front, bg=bg, channels=4)
    assert np.array_equal(f["out"][..., :3], bg) and not f["out"][..., 3].any() and not f["owner"].any() and not f["n"].any()
    # ... and 0 / NaN / a row out of range are no depth at all
    for sz, rows in ((np.zeros((1, S, S), np.float32), None), (np.full((1, S, S), np.nan, np.float32), None), (front, np.full(B, 1, np.int32))):
        g = LR.composite_layers([(c0, z0, False), (c1, z1, True)], ss, scene_z=sz, scene_rows=rows, bg=bg, channels=4)
        assert np.array_equal(g["out"], a["out"]) and np.array_equal(g["owner"], a["owner"])
    # swapping two layers: the same colours unless their depths tie (they do not: independent uniform draws), owner relabelled
    assert not ((z0 == z1) & (z0 > 0)).any()
    x = LR.composite_layers([(c0, z0, False), (c1, z1, False)], ss, bg=bg, channels=4)
    y = LR.composite_layers([(c1, z1, False), (c0, z0, False)], ss, bg=bg, channels=4)
    assert np.array_equal(x["out"], y["out"]) and np.array_equal(x["n"], y["n"])
    relabel = np.array([0, 2, 1], np.uint8)
    if ss == 1:                                            # (at ss > 1 a tie of the COUNTS goes to the lower index on both sides)
        assert np.array_equal(relabel[x["owner"]], y["owner"])
    else:
        win = np.where((z0 > 0) & ((z1 <= 0) | (z0 < z1)), 0, np.where(z1 > 0, 1, -1))
        c = np.stack([(win == l).reshape(B, S, ss, S, ss).sum((2, 4)) for l in (0, 1)])
        untied = c[0] != c[1]
        assert untied.any() and np.array_equal(relabel[x["owner"]][untied], y["owner"][untied])
        assert (x["owner"][~untied] == y["owner"][~untied]).all()
    assert {1, 2} <= set(np.unique(x["owner"]))


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def test_entry_point_refuses_bad_arguments_without_launch(lib):
    """HARP_ERR_ARG (1) before any launch; `f` is a fake device pointer that no kernel may reach"""
    from harp_amd import _lib
    f = 1 << 20
    mk = lambda n=1, **kw: (_lib.Layer * max(n, 1))(*[_lib.Layer(**dict(dict(rgb=f, zbuf=f, flip_x=0, reserved=0), **kw)) for _ in range(max(n, 1))])
    ok = dict(layers=mk(), n_layers=1, B=3, S=4, ss=2, scene_z=None, n_scene=0, scene_rows=None, bg=None, n_bg=0, bg_rows=None, bg_color=f, channels=3,
              out=f, owner=None)
    order = ("layers", "n_layers", "B", "S", "ss", "scene_z", "n_scene", "scene_rows", "bg", "n_bg", "bg_rows", "bg_color", "channels", "out", "owner")
    for bad in (dict(layers=None), dict(n_layers=0), dict(layers=mk(5), n_layers=5), dict(n_layers=-1), dict(layers=mk(zbuf=None)),
                dict(layers=mk(rgb=None)), dict(layers=mk(reserved=1)), dict(layers=mk(2, reserved=7), n_layers=2), dict(ss=0), dict(ss=5),
                dict(channels=2), dict(channels=5), dict(bg=f, n_bg=2), dict(scene_z=f, n_scene=2), dict(bg=f, n_bg=0), dict(scene_z=f, n_scene=0),
                dict(scene_z=f, n_scene=-1), dict(B=0), dict(B=-1), dict(S=0), dict(S=-1), dict(out=None), dict(bg_color=None), dict(S=46341, ss=1),
                dict(S=12000, ss=4)):
        a = dict(ok, **bad)
        assert lib.harp_composite_layers_u8(*[a[k] for k in order], None) == 1, bad


def test_layer_struct_layout_matches_c(tmp_path):
    from harp_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(harp_layer), '
                   'offsetof(harp_layer, zbuf), offsetof(harp_layer, flip_x), offsetof(harp_layer, reserved)); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.Layer), _lib.Layer.zbuf.offset, _lib.Layer.flip_x.offset, _lib.Layer.reserved.offset], got
    assert got == [24, 8, 16, 20]


def test_scene_player_is_importable_without_the_library(tmp_path):
    import sys
    env = dict(os.environ, HARP_LIB_PATH=str(tmp_path / "no_such_library.so"))
    code = ("import sys; sys.path.insert(0, %r); import harp_amd.playback as P; "
            "assert callable(P.ScenePlayer) and callable(P.load_scene_depth) and P.load_scene_depth(None, 8, 'cpu') is None" % ROOT)
    subprocess.check_call([sys.executable, "-c", code], env=env)
