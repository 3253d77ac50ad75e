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


_F = 1 << 20                                                   # a fake device pointer, never dereferenced


def _ptr_fields(cls):
    return [n for n, t in cls._fields_ if t is ctypes.c_void_p]


def _full_chain(V0, E0, NJ):
    from harp_amd import _lib
    return _lib.MeshChain(B=3, V0=V0, E0=E0, NJ=NJ, S=128, focal=500.0, shadow=1, has_normal_grad=1, light_only=0,
                          **{n: _F for n in _ptr_fields(_lib.MeshChain)})


def _full_step():
    from harp_amd import _lib
    return _lib.StepFrame(n_rows=4, target_offset=0, clear_mesh_grads=1, n_loss=8, **{n: _F for n in _ptr_fields(_lib.StepFrame)})


def _full_hand():
    from harp_amd import _lib
    tables = _lib.FrameTables(n_betas_out=10, **{n: _F for n in _ptr_fields(_lib.FrameTables) if "wrist" not in n})
    return _lib.HandFront(chain=_full_chain(778, 2328, 21), mano=_lib.ManoModel(*([_F] * len(_lib.ManoModel._fields_))), tables=tables,
                          self_shadow=1, step=_full_step(), **{n: _F for n in _ptr_fields(_lib.HandFront)})


def _full_arm():
    from harp_amd import _lib
    tables = _lib.FrameTables(n_betas_out=20, **{n: _F for n in _ptr_fields(_lib.FrameTables)})
    tree = _lib.TreeModel(NV=1026, NJ=55, NB=20, n_pose_in=17, center_joint=21, n_joints_out=22, **{n: _F for n in _ptr_fields(_lib.TreeModel)})
    return _lib.ArmFront(chain=_full_chain(1026, 3000, 22), tree=tree, tables=tables, self_shadow=1, step=_full_step(),
                         **{n: _F for n in _ptr_fields(_lib.ArmFront)})


def _mutated(make, path, value):
    h = make()
    obj, names = h, path.split(".")
    for n in names[:-1]:
        obj = getattr(obj, n)
    setattr(obj, names[-1], value)
    return h


_CHAIN_IN = ["chain.edges0", "chain.vf_off", "chain.vf_tri", "chain.disp"]
_CHAIN_FWD = ["chain." + n for n in ("verts_mm", "joints_mm", "joints_m", "vs", "n1", "il1", "vd", "n2", "il2", "ndc_c")]
_CHAIN_FWD_SHADOW = ["chain." + n for n in ("centroid", "light_R", "light_T", "ndc_l")]
_CHAIN_BWD = ["chain." + n for n in ("sub_off", "sub_idx", "vd", "vs", "n1", "il1", "cam_R", "cam_T", "g_vd", "g_ndc_c", "g_joints_m", "g_joints_mm",
                                     "g_v0", "g_cam_T", "g_disp", "n2", "il2", "g_n2",                      # (has_normal_grad is set)
                                     "light_pos", "centroid", "light_R", "light_T", "g_ndc_l", "g_light_R", "g_light_T", "g_light_pos")]
_HAND_ROWS = ["fid", "pose48", "betas", "trans_b", "cam_R", "cam_T", "light_pos", "colors", "lbs_ws"]
_ARM_OK = (_CHAIN_IN + ["tree." + n for n in ("v_template", "shapedirs_T", "posedirs_T", "posedirs", "J_template", "J_dirs", "weights", "pose_mean",
                                               "parents", "pose_src", "joint_src")] +
           ["weights_T", "fid", "pose_in", "betas", "trans_b", "cam_R", "cam_T", "light_pos", "colors", "lbs_ws", "tables.wrist_pose"])
_CLEAR = ["chain.g_vd", "chain.g_joints_m"]                    # (step.clear_mesh_grads is set)
_ARM_SIZES = [("tree.NJ", 0), ("tree.NJ", 65), ("tree.NB", 9), ("tree.NB", 33), ("tree.n_pose_in", 16), ("tables.n_betas_out", 10)]

# entry point -> (struct, number of trailing scratch pointers, required pointers, further (path, value) mutations)
_FUSED = {
    "harp_hand_front_fwd": (_full_hand, 0, _CHAIN_IN + _CHAIN_FWD + _CHAIN_FWD_SHADOW + _HAND_ROWS + _CLEAR, [("chain.E0", 4097 - 778)]),
    "harp_hand_front_wide_fwd": (_full_hand, 1, _CHAIN_IN + _CHAIN_FWD + _CHAIN_FWD_SHADOW + _HAND_ROWS + _CLEAR, [("chain.E0", 4097 - 778)]),
    # the hybrid front leaves the mesh inputs, the chain outputs and the size limit to harp_mesh_chain_fwd, its second launch
    "harp_hand_front_hybrid_fwd": (_full_hand, 0, ["chain.verts_mm", "chain.joints_mm"] + _HAND_ROWS + _CLEAR, []),
    "harp_hand_back_bwd": (_full_hand, 2, _CHAIN_IN + _CHAIN_BWD + ["fid", "pose48", "lbs_ws"], [("chain.E0", 4097 - 778), ("step.n_loss", 65)]),
    "harp_hand_back_wide_bwd": (_full_hand, 3, _CHAIN_IN[1:] + _CHAIN_BWD + ["fid", "pose48", "lbs_ws"],
                                [("chain.E0", 4097 - 778), ("step.n_loss", 65)]),
    "harp_arm_front_fwd": (_full_arm, 0, _ARM_OK + _CHAIN_FWD + _CHAIN_FWD_SHADOW + _CLEAR, [("chain.E0", 4097 - 1026)] + _ARM_SIZES),
    "harp_arm_front_wide_fwd": (_full_arm, 1, _ARM_OK + _CHAIN_FWD + _CHAIN_FWD_SHADOW + _CLEAR + ["chain.cam_R", "chain.cam_T", "chain.light_pos"],
                                [("chain.E0", 4097 - 1026)] + _ARM_SIZES),
    "harp_arm_back_bwd": (_full_arm, 3, _ARM_OK + _CHAIN_BWD, [("chain.E0", 4097 - 1026), ("step.n_loss", 65)] + _ARM_SIZES),
    "harp_arm_back_wide_bwd": (_full_arm, 4, _ARM_OK + _CHAIN_BWD, [("chain.E0", 4097 - 1026), ("step.n_loss", 65)] + _ARM_SIZES),
}


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: an entry point that lost a check would launch on them")
def test_fused_entry_points_refuse_bad_arguments(lib):
    """The nine fused front / back entry points return HARP_ERR_ARG (1) for every single broken argument: a fully populated struct of fake
    pointers with legal sizes, then ONE mutation per case — B = 0, V0 != NV, a wrong NJ, V0 + E0 over the limit of that form, every required
    pointer nulled on its own, wrist_pose set on the hand path / missing on the arm path, a schedule without its row counter or with
    n_rows = 0, n_loss = 65, clear_mesh_grads without g_vd, shadow without the light rows.
    Skipped when a GPU is visible: most of these cases have a non-empty grid, so an entry point that lost a check would launch its kernel on
    the fake pointers; on a machine without a device such a call fails in the runtime instead (a status other than 1, so the test fails
    without touching memory).  For the same reason the unmutated struct is checked on the front launchers only (they reach their launch:
    status >= 2).  The back launchers return 1 for the unmutated struct as well on a CPU-only machine, from the call that raises the
    kernel's LDS limit: for them this test proves "still rejected" and cannot prove "not rejected more"."""
    for name, (make, n_scratch, pointers, more) in _FUSED.items():
        fn = getattr(lib, name)
        is_arm, is_back, is_wide = "_arm_" in name, "_back_" in name, "_wide_" in name
        scratch = [_F] * n_scratch

        def call(h, scratch=scratch):
            return fn(ctypes.byref(h), *scratch, None)

        if not is_back:
            assert call(make()) >= 2, name                     # legal: it gets as far as the launch (no device here)
        cases = [("chain.B", 0), ("chain.V0", 777 if not is_arm else 1025), ("chain.NJ", 20 if not is_arm else 21), ("chain.E0", -1)]
        cases += [(p, None) for p in pointers] + more
        cases += [("tables.wrist_pose", _F)] if not is_arm else []                       # (missing on the arm path: in `pointers`)
        cases += [("step.sched_row", None), ("step.n_rows", 0)]
        for path, value in cases:
            assert call(_mutated(make, path, value)) == 1, (name, path, value)
        if is_arm and is_wide:                                 # a quarter of the arm's vertices per 320-thread workgroup
            h = make()
            h.chain.V0 = h.tree.NV = 1284; h.chain.E0 = 100
            assert call(h) == 1, (name, "NV over 4 x 320")
        # the scratch pointers of the call itself; a null struct
        for k in range(n_scratch):
            if is_back and k == 0:
                continue                                       # g_colors may be NULL (no appearance gradient)
            args = list(scratch); args[k] = None
            assert fn(ctypes.byref(make()), *args, None) == 1, (name, "scratch", k)
        assert fn(None, *scratch, None) == 1, name
