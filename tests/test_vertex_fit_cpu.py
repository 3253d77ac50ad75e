"""The batched MANO vertex fit without a device: the yardstick of tests/_vertex_fit_ref.py converges from the rigid start as the
issue's float64 prototype did; the rigid start itself (harp_amd.playback.vertex_start) at its edges; the new signatures, the command line
and harp_mano_vertex_fit's argument errors, which return before any launch."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import _ik_ref
from tests import _vertex_fit_ref as R


# ---- (a) the yardstick converges ----------------------------------------------------------------------------------------------------
def test_yardstick_converges_from_the_rigid_start():
    sc = R.scene(T=3, seed=0)
    x0 = R.rigid_x0(sc)
    res = R.lm(sc["model"], x0, sc["targets"], iters=8)
    assert bool(res["ok"][:5].all()), res["ok"]
    rms = R.rms_mm(sc["model"], res["x"], sc["targets"])
    print(f"[vertex_fit] yardstick rms after 8 iterations {rms.tolist()} mm; start {R.rms_mm(sc['model'], x0, sc['targets']).tolist()}")
    assert float(rms.max()) < 1e-6
    # float32, the error model, gets to its own floor as well: far below a tenth of a millimetre
    res32 = R.lm(sc["model"], x0, sc["targets"], iters=8, dtype=torch.float32)
    assert float(R.rms_mm(sc["model"], res32["x"], sc["targets"]).max()) < 1e-2


def test_yardstick_stops_at_the_noise_floor():
    sc = R.scene(T=3, seed=0, noise=0.002)
    res = R.lm(sc["model"], R.rigid_x0(sc), sc["targets"], iters=8)
    c6, c8 = res["cost"][6], res["cost"][8]
    print(f"[vertex_fit] yardstick noise floor rms {((c8 / 778).sqrt() * 1000).tolist()} mm; relative change 6 -> 8 {((c6 - c8) / c8).tolist()}")
    assert float(((c6 - c8) / c8).abs().max()) <= 1e-6
    assert 3.0 < float((c8 / 778).sqrt().mean() * 1000) < 3.6          # 2 mm per coordinate = 3.46 mm per vertex, less the 61 fitted unknowns


def test_yardstick_freezes_the_shape():
    sc = R.scene(T=2, seed=3)
    x0 = R.rigid_x0(sc)
    n = R.normal(sc["model"], x0, sc["targets"], solve_shape=False)
    A, g = n["A"], n["g"]
    assert bool((A[:, 48:58, :48] == 0).all() and (A[:, :48, 48:58] == 0).all() and (A[:, 58:, 48:58] == 0).all() and (g[:, 48:58] == 0).all())
    assert bool((torch.diagonal(A, dim1=1, dim2=2)[:, 48:58] == 1).all())
    res = R.lm(sc["model"], x0, sc["targets"], solve_shape=False, iters=3)
    assert torch.equal(res["x"][:, 48:58], x0[:, 48:58]) and bool((res["cost"][3] < res["cost"][0]).all())


# ---- (b) vertex_start -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rest():
    sc = R.scene(T=1, seed=0)
    v, j = R.rest(sc["model"], torch.zeros(1, 10, dtype=torch.float64))
    return v[0], j[0]


def _moved(rest, angles, rng):
    from harp_amd.playback import vertex_start  # noqa: F401  (the feature under test)
    v, j0 = rest
    Rs, tg, tr = [], [], []
    for th in angles:
        u = rng.normal(size=3)
        Rm = _ik_ref.axis_angle_to_matrix(th * u / np.linalg.norm(u))
        t = rng.uniform(-0.3, 0.3, size=3)
        Rs.append(Rm); tr.append(t); tg.append((v - j0) @ Rm.T + j0 + t)
    return np.stack(Rs), np.stack(tg), np.stack(tr)


def test_vertex_start_recovers_rigid_motions(rest):
    from harp_amd.playback import vertex_start
    angles = [0.0, 1e-7, 1.0, np.pi - 1e-6, np.pi]
    Rs, tg, tr = _moved(rest, angles, np.random.default_rng(5))
    rot, trans = vertex_start(tg, np.ones((5, 778), bool), rest[0], rest[1])
    assert rot.shape == (5, 3) and trans.shape == (5, 3) and rot.dtype == np.float64 and np.isfinite(rot).all()
    for k, th in enumerate(angles):
        err = np.abs(_ik_ref.axis_angle_to_matrix(rot[k]) - Rs[k]).max()
        print(f"[vertex_fit] vertex_start angle {th!r}: rotation error {err:.2e}, trans error {np.abs(trans[k] - tr[k]).max():.2e}, |rot| {np.linalg.norm(rot[k])!r}")
        assert err < 1e-9 and np.abs(trans[k] - tr[k]).max() < 1e-9
        assert abs(np.linalg.norm(rot[k]) - th) < 1e-7
    # weights: a vertex with weight 0 may lie anywhere; per-frame rest vertices and root joints are taken as well
    w = np.ones((5, 778))
    w[:, ::7] = 0.0
    bad = tg.copy()
    bad[:, ::7] = 1e3
    rot2, trans2 = vertex_start(bad, w, np.broadcast_to(rest[0], (5, 778, 3)), np.broadcast_to(rest[1], (5, 3)))
    assert np.abs(trans2 - trans).max() < 1e-9            # (at the angle pi the axis-angle's sign is free: the matrices are compared)
    assert max(np.abs(_ik_ref.axis_angle_to_matrix(rot2[k]) - Rs[k]).max() for k in range(5)) < 1e-9
    # a mirrored target gets a proper rotation
    rot3, _ = vertex_start(tg[2:3] * np.array([-1.0, 1.0, 1.0]), np.ones((1, 778), bool), rest[0], rest[1])
    assert abs(np.linalg.det(_ik_ref.axis_angle_to_matrix(rot3[0])) - 1.0) < 1e-12


def test_vertex_start_frames_that_cannot_be_aligned(rest):
    from harp_amd.playback import vertex_start
    Rs, tg, tr = _moved(rest, [0.5, 1.0, 1.5, 2.0], np.random.default_rng(6))
    tg[0] = np.nan                                         # none before it: zeros
    tg[2] = np.nan                                         # takes frame 1's
    used = np.ones((4, 778), bool)
    used[3, 2:] = False                                    # two used vertices: takes frame 1's too
    rot, trans = vertex_start(tg, used, rest[0], rest[1])
    assert np.isfinite(rot).all() and np.isfinite(trans).all()
    assert (rot[0] == 0).all() and (trans[0] == 0).all()
    assert (rot[2] == rot[1]).all() and (trans[2] == trans[1]).all() and (rot[3] == rot[1]).all() and (trans[3] == trans[1]).all()
    assert np.abs(_ik_ref.axis_angle_to_matrix(rot[1]) - Rs[1]).max() < 1e-9
    # a few NaN vertices in an otherwise good frame are left out
    tg2 = _moved(rest, [1.0], np.random.default_rng(7))
    t = tg2[1].copy()
    t[0, 5:9] = np.nan
    r2, _ = vertex_start(t, np.ones((1, 778), bool), rest[0], rest[1])
    assert np.abs(_ik_ref.axis_angle_to_matrix(r2[0]) - tg2[0][0]).max() < 1e-9


def test_vertex_start_is_vectorised(rest, monkeypatch):
    """T = 0 .. 3 frames through ONE SVD call each time: the frames are a batch dimension, not a loop"""
    from harp_amd.playback import keypoints, vertex_start
    calls = []
    svd = np.linalg.svd
    monkeypatch.setattr(keypoints.np.linalg, "svd", lambda a, *k, **kw: (calls.append(np.shape(a)), svd(a, *k, **kw))[1])
    for T in range(4):
        _, tg, _ = _moved(rest, [0.3 * (k + 1) for k in range(T)], np.random.default_rng(8)) if T else (None, np.zeros((0, 778, 3)), None)
        rot, trans = vertex_start(tg, np.ones((T, 778), bool), rest[0], rest[1])
        assert rot.shape == (T, 3) and trans.shape == (T, 3)
    assert calls == [(T, 3, 3) for T in range(4)]


# ---- (c) signatures, command line, argument errors ------------------------------------------------------------------------------------
def test_optimize_for_mano_param_takes_a_method():
    from harp_amd.metro_modifications import hand_utils
    p = inspect.signature(hand_utils.optimize_for_mano_param).parameters
    assert p["method"].default == "adam"
    assert list(p)[:5] == ["pred_vertices", "mano_layer", "idx", "vert_rgb", "use_graph"]

    class Never:                                           # touching the layer (or a device) before the check would raise AttributeError
        def __getattr__(self, name):
            raise AttributeError(name)
    with pytest.raises(ValueError, match="method"):
        hand_utils.optimize_for_mano_param(torch.zeros(1, 778, 3), Never(), method="newton")


def test_command_line_takes_vertices():
    from harp_amd.playback import cli
    common = ["--config", "c.yaml", "--out", "o"]
    args = cli.parse_args(common + ["--vertices", "v.npz"])
    assert args.vertices == "v.npz" and args.motion is None and args.keypoints is None
    assert cli.parse_args(common + ["--motion", "m.npz"]).vertices is None
    for other in ("--motion", "--keypoints"):
        with pytest.raises(SystemExit):
            cli.parse_args(common + ["--vertices", "v.npz", other, "m.npz"])
    with pytest.raises(SystemExit):
        cli.parse_args(common)


def test_from_vertices_signature_and_arm():
    from harp_amd.playback import Motion
    p = inspect.signature(Motion.from_vertices).parameters
    assert [k for k in p] == ["vertices", "params", "hand_layer", "cam", "weights", "iters", "pose_prior_weight", "init", "device"]
    assert p["iters"].default == 10 and p["pose_prior_weight"].default == 0.0
    with pytest.raises(NotImplementedError):
        Motion.from_vertices(np.zeros((1, 778, 3)), {}, _ik_ref._Layer({"pose_mean": np.zeros(165)}))


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def test_vertex_fit_argument_errors_without_a_launch(lib):
    from harp_amd import _lib
    f = 1 << 20                                            # a fake device pointer, never dereferenced
    mano = _lib.ManoModel(*([f] * len(_lib.ManoModel._fields_)))
    good = dict(m=ctypes.byref(mano), targets=f, weights=None, prior=None, T=2, pose48=f, betas=f, trans=f, cost=f, status=f)

    def call(opt=None, **kw):
        a = dict(good, **kw)
        o = ctypes.byref(_lib.VertexFitOptions(10, 1e-3, 0.0, 0.0, 1, 0)) if opt is None else opt
        return lib.harp_mano_vertex_fit(a["m"], a["targets"], a["weights"], a["prior"], a["T"], o, a["pose48"], a["betas"], a["trans"], a["cost"],
                                        a["status"], None, None, None, None, None)

    for name in ("m", "targets", "pose48", "betas", "trans", "cost", "status"):
        assert call(**{name: None}) == 1, name
    assert call(opt=ctypes.POINTER(_lib.VertexFitOptions)()) == 1
    assert call(T=0) == 1 and call(T=-1) == 1
    nan, inf = float("nan"), float("inf")
    for bad in [(-1, 1e-3, 0.0, 0.0), (10, -1.0, 0.0, 0.0), (10, nan, 0.0, 0.0), (10, inf, 0.0, 0.0), (10, 1e-3, -1.0, 0.0), (10, 1e-3, nan, 0.0),
                (10, 1e-3, inf, 0.0), (10, 1e-3, 0.0, -1.0), (10, 1e-3, 0.0, nan), (10, 1e-3, 0.0, inf)]:
        assert call(opt=ctypes.byref(_lib.VertexFitOptions(*bad, 1, 0))) == 1, bad
    assert ctypes.sizeof(_lib.VertexFitOptions) == 24 and lib.harp_mano_vertex_fit_frames_per_block() >= 1


def test_vertex_fit_options_layout_matches_c(tmp_path):
    import os
    import subprocess
    from harp_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [n for n, _ in _lib.VertexFitOptions._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "harp_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) +
                   '\\n", sizeof(harp_vertex_fit_options),' + ",".join(f"offsetof(harp_vertex_fit_options, {n})" for n in fields) + "); return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_lib.VertexFitOptions)] + [getattr(_lib.VertexFitOptions, n).offset for n in fields]


def test_ops_refuses_host_tensors():
    from harp_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mano_vertex_fit(None, torch.zeros(1, 778, 3), torch.zeros(1, 48), torch.zeros(1, 10), torch.zeros(1, 3))
