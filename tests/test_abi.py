"""CPU checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol include/harp_hip.h
declares (no compute calls without a GPU); the ctypes mirrors match the C structs; the product has no CPU fallback."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def test_header_symbols_exported(lib):
    from harp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "harp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t)\s+(harp_\w+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 30
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in harp_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)


def test_struct_layouts_match_c(tmp_path):
    """compile a tiny C program against the header and compare sizeof/offsetof with the ctypes mirrors"""
    import subprocess
    from harp_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(harp_shade_args), offsetof(harp_shade_args, B), offsetof(harp_shade_args, rgb), sizeof(harp_mano_model),'
                   'sizeof(harp_frame_tables), sizeof(harp_adam_hyper), offsetof(harp_frame_tables, share_light), sizeof(harp_mesh_chain),'
                   'sizeof(harp_hand_front), offsetof(harp_hand_front, step), sizeof(harp_step_frame), offsetof(harp_step_frame, draw_counter),'
                   'sizeof(harp_tree_model), sizeof(harp_arm_front), offsetof(harp_arm_front, weights_T), offsetof(harp_arm_front, step));'
                   'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(_lib.ShadeArgs), _lib.ShadeArgs.B.offset, _lib.ShadeArgs.rgb.offset, ctypes.sizeof(_lib.ManoModel),
            ctypes.sizeof(_lib.FrameTables), 32, _lib.FrameTables.share_light.offset, ctypes.sizeof(_lib.MeshChain),
            ctypes.sizeof(_lib.HandFront), _lib.HandFront.step.offset, ctypes.sizeof(_lib.StepFrame), _lib.StepFrame.draw_counter.offset,
            ctypes.sizeof(_lib.TreeModel), ctypes.sizeof(_lib.ArmFront), _lib.ArmFront.weights_T.offset, _lib.ArmFront.step.offset]
    assert got == want, (got, want)


def test_no_cpu_fallback(lib):
    from harp_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rasterize_fwd(torch.zeros(1, 3, 3), torch.zeros(1, 3, dtype=torch.int32), 8)
    # records | bboxes | lists | counts, order, nact (256 B each) | hit bitmaps (one 64-bit word per frame, super-tile and 64 faces)
    assert lib.harp_rasterize_ws_bytes(2, 10, 64) == 2 * 10 * 64 + 2 * 10 * 16 + 2 * 1 * 10 * 4 + 3 * 256 + 2 * 1 * 1 * 8      # pure host arithmetic
    assert lib.harp_rasterize_fwd(None, None, 1, 1, 1, 8, 0, 0.0, 1.0, None, None, None, None, None) == 1   # HARP_ERR_ARG, no launch


def test_product_does_not_import_oracle():
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r); import harp_amd, harp_amd.engine, harp_amd.ops, harp_amd.synth, "
            "harp_amd.manopth.manolayer; assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules), 'oracle imported'" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])
    for dirpath, _, files in os.walk(os.path.join(ROOT, "harp_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "oracle" not in open(os.path.join(dirpath, f)).read().replace("# oracle", ""), f


def test_building_blocks_refuse_empty_sizes_without_launch(lib):
    """The stand-alone entry points return HARP_ERR_ARG (1) for empty sizes before any launch (include/harp_hip.h).  Only sizes 0 and -1
    and B = 0 are used: for each of them an entry point WITHOUT the check would compute an empty grid and fail its launch (status 2 + the
    HIP error), so no kernel can reach the fake pointers.  The cases whose grid would not be empty (centroid with V = 0, displace with
    B = 0, close-to-z with W = 0, ...) are checked with real buffers in tests/test_gpu_building_blocks.py."""
    f = 1 << 20                                                # a fake device pointer, never dereferenced
    for B, V0, E0 in [(0, 4, 2), (1, 0, 0), (1, -1, 0), (1, 0, -1)]:
        assert lib.harp_subdivide_fwd(f, f, B, V0, E0, 1.0, f, None) == 1, (B, V0, E0)
    for B, V0 in [(0, 4), (1, 0), (1, -1)]:
        assert lib.harp_subdivide_bwd(f, f, f, B, V0, 6, 1.0, f, None) == 1, (B, V0)
    for B, V in [(0, 4), (1, 0), (1, -1)]:
        assert lib.harp_vertex_normals_fwd(f, f, f, f, B, V, f, f, None, None, None) == 1, (B, V)
        assert lib.harp_vertex_normals_fwd(f, f, f, f, B, V, f, f, f, f, None) == 1, (B, V)
        assert lib.harp_vertex_normals_bwd(f, f, f, f, B, V, f, f, f, f, f, None) == 1, (B, V)
        assert lib.harp_project_fwd(f, f, f, B, V, 500.0, 128.0, 128.0, 256, f, None) == 1, (B, V)
        assert lib.harp_project_bwd(f, f, f, f, B, V, 500.0, 256, f, f, f, None) == 1, (B, V)
    for V in (0, -1):
        assert lib.harp_displace_bwd(f, f, f, 1, V, f, f, None) == 1, V
    assert lib.harp_centroid(f, 0, 4, f, None) == 1
    for n in (0, -1):
        assert lib.harp_scale(f, 2.0, n, f, None) == 1, n
        assert lib.harp_sum_squares(f, n, f, f, f, None) == 1, n
        assert lib.harp_mse(f, f, n, f, f, None) == 1, n
        assert lib.harp_normalize3_fwd(f, n, f, None) == 1, n
        assert lib.harp_normalize3_bwd(f, f, n, f, None) == 1, n
        assert lib.harp_image_l1(f, f, None, None, 1, n, 3, f, f, f, None) == 1, n
    for H, W in [(0, 5), (5, 0), (-1, 5), (5, -1)]:
        assert lib.harp_texture_smooth_reg(f, f, None, H, W, f, f, f, None) == 1, (H, W)
    assert lib.harp_close_to_z_reg(f, 0, 5, 1.0, f, f, f, None) == 1
    assert lib.harp_adam_step(f, f, f, f, 0, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None) == 1
    assert lib.harp_kps_loss(f, None, f, 0, 21, f, f, f, None) == 1
    assert lib.harp_image_l1(f, f, None, None, 0, 12, 3, f, f, f, None) == 1
    # mesh regularisers: B = 0 (grid y), V = 0 or V = -1 (grid x = (V + 511) / 512 or (V + 255) / 256 = 0); P < 0 / E < 0 would launch
    for B, V in [(0, 4), (1, 0), (1, -1)]:
        assert lib.harp_mesh_regularizers(f, f, f, f, f, f, f, B, V, 2, 5, f, f, f, None) == 1, (B, V)
        assert lib.harp_mesh_kps_terms(f, f, f, f, f, f, f, B, V, 2, 5, f, f, f, f, None, f, 21, f, f, f, None) == 1, (B, V)
    # skinning backward calls, B = 0 only (B = -1 gives a non-empty dim3(B)); the model struct is read on the host: a real one holding
    # fake device pointers
    from harp_amd import _lib
    mano = _lib.ManoModel(*([f] * len(_lib.ManoModel._fields_)))
    assert lib.harp_lbs_mano_bwd(ctypes.byref(mano), f, f, f, 0, f, f, f, f, f, f, None) == 1
    tree = _lib.TreeModel(NV=1026, NJ=55, NB=20, n_pose_in=17, center_joint=21, n_joints_out=22,
                          **{n: f for n, t in _lib.TreeModel._fields_ if t is ctypes.c_void_p})
    assert lib.harp_lbs_tree_bwd(ctypes.byref(tree), f, f, f, 0, f, f, f, f, f, f, None) == 1
    # per-frame glue: B <= 0 is refused on the host.  As above only the sizes whose launch would be empty WITHOUT the check are tried with
    # fake pointers: B = 0 and B = -1 for the 64-lane grids, B = 0 for harp_frame_setup_bwd, whose grid is dim3(B) (its B = -1 is refused
    # with real buffers in tests/test_gpu_frame_glue.py)
    tables = _lib.FrameTables(n_betas_out=10, **{n: f for n, t in _lib.FrameTables._fields_ if t is ctypes.c_void_p})
    for B in (0, -1):
        assert lib.harp_frame_setup_fwd(ctypes.byref(tables), f, B, 64, 500.0, 1, f, f, f, f, f, f, f, None) == 1, B
        assert lib.harp_light_setup_fwd(f, f, B, f, f, None) == 1, B
        assert lib.harp_light_setup_bwd(f, f, f, f, B, 4, f, f, None, None) == 1, B
    assert lib.harp_frame_setup_bwd(ctypes.byref(tables), f, 0, 64, 500.0, 1, f, f, f, f, f, f, None) == 1
