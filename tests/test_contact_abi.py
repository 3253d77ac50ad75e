"""CPU checks of harp_mesh_contact's boundary (include/harp_hip.h), after the pattern of tests/test_abi.py: every argument error returns
HARP_ERR_ARG before any launch (fake pointers, never dereferenced: no device is touched), the workspace size is the documented host
arithmetic, and the ctypes mirror matches the C struct."""
import ctypes
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20                                                 # a fake device pointer, 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def _mesh(**over):
    from harp_amd import _lib
    m = dict(verts=FAKE, cam_R=FAKE, cam_T=FAKE, faces=FAKE, V=5, F=7, flip_x=0, reserved=0)
    m.update(over)
    return _lib.ContactMesh(**m)


def _call(lib, q, t, B=2, max_dist=0.02, ws=FAKE, dist=FAKE, face=FAKE, wind=FAKE):
    ref = lambda m: None if m is None else ctypes.byref(m)      # noqa: E731
    return lib.harp_mesh_contact(ref(q), ref(t), B, max_dist, ws, dist, face, wind, None)


def test_argument_errors_return_before_any_launch(lib):
    ok = _mesh()
    assert _call(lib, None, ok) == 1 and _call(lib, ok, None) == 1
    assert _call(lib, ok, ok, ws=None) == 1
    for field in ("verts", "cam_R", "cam_T"):
        assert _call(lib, _mesh(**{field: None}), ok) == 1, ("query", field)
        assert _call(lib, ok, _mesh(**{field: None})) == 1, ("target", field)
    assert _call(lib, ok, _mesh(faces=None)) == 1
    for bad in (0, -1):
        assert _call(lib, _mesh(V=bad), ok) == 1 and _call(lib, ok, _mesh(V=bad)) == 1 and _call(lib, ok, _mesh(F=bad)) == 1
        assert _call(lib, ok, ok, B=bad) == 1
    assert _call(lib, _mesh(reserved=1), ok) == 1 and _call(lib, ok, _mesh(reserved=-3)) == 1
    for bad in (-0.001, -math.inf, math.nan):
        assert _call(lib, ok, ok, max_dist=bad) == 1, bad
    assert _call(lib, ok, ok, dist=None, face=None, wind=None) == 1
    assert _call(lib, ok, ok, ws=FAKE + 4) == 1                               # not 16-byte aligned


def test_workspace_size_is_host_arithmetic(lib):
    f = lib.harp_mesh_contact_ws_floats
    assert f(0, 10) == 0 and f(2, 0) == 0 and f(-1, -1) == 0
    for B, F in ((1, 1), (3, 128), (2, 129), (32, 6152)):
        assert f(B, F) == B * (8 * -(-F // 128) + 12 * F), (B, F)             # a box per chunk of 128 faces, 12 floats per face


def test_struct_layout_matches_c(tmp_path):
    from harp_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",'
                   'sizeof(harp_contact_mesh), offsetof(harp_contact_mesh, faces), offsetof(harp_contact_mesh, V),'
                   'offsetof(harp_contact_mesh, flip_x), offsetof(harp_contact_mesh, reserved)); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    M = _lib.ContactMesh
    assert got == [ctypes.sizeof(M), M.faces.offset, M.V.offset, M.flip_x.offset, M.reserved.offset], got
