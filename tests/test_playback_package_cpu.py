"""CPU checks of the parts that harp_amd/playback/ is made of, none of which needs a device: the index table of a render
call (player.stage_table), the one packed table of a motion's rows (motion.RowLayout) and what Motion.resample makes of it, the host side
of the keypoint solve (keypoints.ik_inputs), and the command line as a module."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _ik_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stage_loop(rows, n_pad, inputs):
    """stage_table restated frame by frame"""
    n = len(rows)
    tab = np.zeros((1 + 2 * len(inputs), n_pad), np.int32)
    for i in range(n_pad):
        j = min(i, n - 1)                                # the padding repeats the last frame
        tab[0, i] = rows[j]
        for k, (rr, N) in enumerate(inputs):
            if rr is not None:
                inside = 0 <= rr[j] < N
                tab[1 + 2 * k, i] = j if inside else -1
                tab[2 + 2 * k, i] = rr[j] if inside else 0
    return tab


@pytest.mark.parametrize("n,B", [(1, 1), (5, 2), (4, 4)])
@pytest.mark.parametrize("last", ["inside", "outside"])
def test_stage_table_against_a_loop(n, B, last):
    from harp_amd.playback.player import stage_table
    n_pad = -(-n // B) * B
    rows = np.arange(n, dtype=np.int64)[::-1] + 3          # the motion's rows in descending order
    N = 4
    a = np.array([2, -1, N, 0, 3][:n], np.int64)           # a row below 0 and a row >= N
    b = np.array([N + 5, 1, 1, -7, 0][:n], np.int64)
    a[-1], b[-1] = (N - 1, 0) if last == "inside" else (N, -1)
    for inputs in ([], [(a, N)], [(a, N), (b, N)], [(None, 0), (b, N)], [(a, N), (None, 0)]):
        got = stage_table(rows, n_pad, inputs)
        assert got.dtype == np.int32 and got.shape == (1 + 2 * len(inputs), n_pad)
        assert np.array_equal(got, _stage_loop(rows, n_pad, inputs)), inputs
    got = stage_table(rows, n_pad, [(a, N), (b, N)])
    assert np.array_equal(got[0, n:], np.full(n_pad - n, rows[-1]))
    for k, rr in ((0, a), (1, b)):                           # the padding: the last frame's slot and source, or -1 / 0
        want = (n - 1, rr[-1]) if last == "inside" else (-1, 0)
        assert all((got[1 + 2 * k, i], got[2 + 2 * k, i]) == want for i in range(n - 1, n_pad))
    if n == 5:
        assert list(got[1]) == ([0, -1, -1, 3] + [4, 4] if last == "inside" else [0, -1, -1, 3, -1, -1])
        assert list(got[2]) == ([2, 0, 0, 0] + [N - 1, N - 1] if last == "inside" else [2, 0, 0, 0, 0, 0])


def _motion(arm, light, T=6, seed=2):
    """distinct values per field: field f holds 100 f + a small seeded number"""
    from harp_amd.playback import Motion
    rng = np.random.default_rng(seed)
    r = lambda f, w: (100.0 * f + rng.uniform(0.0, 1.0, size=(T, w))).astype(np.float32)      # noqa: E731
    return Motion(r(1, 45), r(2, 3), r(3, 3), r(4, 3), wrist_pose=r(5, 3) if arm else None, light_positions=r(6, 3) if light else None)


def _order(arm, light):
    return ["rot"] + ["wrist_pose"] * arm + ["pose", "trans"] + ["light_positions"] * light + ["cam"]


@pytest.mark.parametrize("arm", [False, True])
@pytest.mark.parametrize("light", [False, True])
def test_row_layout_round_trip(arm, light):
    from harp_amd.playback import Motion
    from harp_amd.playback.motion import RowLayout
    m = _motion(arm, light)
    lay = RowLayout(m)
    assert [k for k, _, _ in lay.fields] == _order(arm, light)
    assert [(w, kind) for _, w, kind in lay.fields] == [(45 if k == "pose" else 3, dict(rot="rot", wrist_pose="rot", pose="rot", trans="vec",
                                                                                        light_positions="vec", cam="scalar")[k]) for k in _order(arm, light)]
    assert (lay.n_rot, lay.n_vec) == (16 + arm, 1 + light) and lay.widths == [w for _, w, _ in lay.fields]
    table = lay.pack("cpu")
    assert table.dtype == torch.float32 and table.is_contiguous() and tuple(table.shape) == (len(m), 3 * lay.n_rot + 3 * lay.n_vec + 3)
    assert torch.equal(table, torch.cat([getattr(m, k) for k in _order(arm, light)], 1))
    back = lay.unpack(table)
    assert set(back) == set(Motion.FIELDS)
    for k in Motion.FIELDS:
        if getattr(m, k) is None:
            assert back[k] is None, k
        else:
            assert torch.equal(back[k], getattr(m, k)), k
    assert lay.trim(0.5, 0.1) == [0.5] * lay.n_rot + [0.1] * lay.n_vec + [0.0] * 3
    assert lay.trim(None, 0.1) == [0.0] * lay.n_rot + [0.1] * lay.n_vec + [0.0] * 3


class _Layer:
    def __init__(self, arm):
        rng = np.random.default_rng(3)
        self._model_np = dict(pose_mean=rng.normal(size=165) * 0.2) if arm else dict(hands_mean=rng.normal(size=45) * 0.2)


@pytest.mark.parametrize("arm", [False, True])
@pytest.mark.parametrize("light", [False, True])
def test_motion_resample_assembles_the_table(monkeypatch, arm, light):
    from harp_amd import ops, playback
    calls = []

    def motion_resample(keys, times, n_rot, rot_offset=None):
        """the gather of `keys` at the rounded times; records what it was given"""
        calls.append(dict(keys=keys.clone(), times=times.clone(), n_rot=n_rot, rot_offset=rot_offset.clone()))
        return keys[times.round().long()]

    monkeypatch.setattr(ops, "motion_resample", motion_resample)
    m = _motion(arm, light)
    layer = _Layer(arm)
    times = np.array([0.0, 2.2, 4.9, 1.0])
    out = m.resample(times, layer, device="cpu")
    c = calls[-1]
    assert torch.equal(c["keys"], torch.cat([getattr(m, k) for k in _order(arm, light)], 1)) and c["keys"].is_contiguous()
    assert c["n_rot"] == 16 + arm and np.array_equal(c["rot_offset"].numpy(), playback.pose_mean_rows(layer, arm))
    assert c["rot_offset"].dtype == torch.float32 and np.array_equal(c["times"].numpy(), times.astype(np.float32))
    at = [0, 2, 5, 1]
    assert len(out) == 4
    for k in playback.Motion.FIELDS:                         # each field from its own columns: a swapped pair would show in the hundreds
        if getattr(m, k) is None:
            assert getattr(out, k) is None, k
        else:
            assert torch.equal(getattr(out, k), getattr(m, k)[at]), k


def test_ik_inputs_prepares_the_start_and_refuses_bad_input():
    from harp_amd import playback
    from harp_amd.playback import keypoints as K
    sc = R.scene(T=3, seed=0)
    model, T = sc["model_np"], 3
    params = dict(shape=sc["betas"].float(), cam=torch.tensor([[1.5, 0.1, -0.2]] * 4))
    tg = sc["targets"].numpy()
    big = tg[:, :1] + 1.25 * (tg - tg[:, :1])                # someone else's, larger hand
    a = K.ik_inputs(big, None, None, None, params, model)
    shape = params["shape"].numpy().astype(np.float64)
    rest = playback.rest_chain_joints(model, shape)
    used = np.ones((T, 21), bool)
    scaled = big[:, :1] + playback.bone_length_scale(big, used, rest) * (big - big[:, :1])
    rot, trans = playback.palm_start(scaled, used, rest)
    assert np.array_equal(a["keypoints"], scaled) and np.abs(a["keypoints"] - tg).max() < 1e-6      # (float32 betas: the model's bones to ~1e-8)
    assert np.array_equal(a["pose48"][:, :3], rot) and np.array_equal(a["trans"], trans) and not a["pose48"][:, 3:].any()
    assert a["pose48"].shape == (T, 48) and np.array_equal(a["shape"], shape) and a["weights"] is None
    assert a["cam"].dtype == np.float32 and np.array_equal(a["cam"], np.tile(np.float32([1.5, 0.1, -0.2]), (T, 1)))
    # the switch, the weights and a warm start
    off = K.ik_inputs(big, np.ones((T, 21)), np.zeros((T, 3)), None, params, model, match_bone_lengths=False)
    assert np.array_equal(off["keypoints"], big) and off["weights"].dtype == np.float64 and off["cam"].shape == (T, 3)
    init = playback.Motion(np.full((T, 45), 0.25), np.full((T, 3), 0.5), np.full((T, 3), 0.75), np.zeros((T, 3)))
    warm = K.ik_inputs(tg, None, None, init, params, model)
    assert np.array_equal(warm["pose48"], np.concatenate([np.full((T, 3), 0.5), np.full((T, 45), 0.25)], 1)) and (warm["trans"] == 0.75).all()
    # what Motion.from_keypoints refuses
    for bad in (tg[:, :20], tg[0]):
        with pytest.raises(ValueError, match="keypoints"):
            K.ik_inputs(bad, None, None, None, params, model)
    with pytest.raises(TypeError, match="keypoints"):
        K.ik_inputs(np.zeros((T, 21, 3), np.int64), None, None, None, params, model)
    with pytest.raises(ValueError, match="weights"):
        K.ik_inputs(tg, np.ones((T, 20)), None, None, params, model)
    with pytest.raises(TypeError, match="weights"):
        K.ik_inputs(tg, np.ones((T, 21), np.int32), None, None, params, model)
    with pytest.raises(ValueError, match="init"):
        K.ik_inputs(tg, None, None, playback.Motion(np.zeros((2, 45)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3))), params, model)
    with pytest.raises(ValueError, match="init"):
        K.ik_inputs(tg, None, None, "a motion", params, model)
    with pytest.raises(ValueError, match="cam"):
        K.ik_inputs(tg, None, np.zeros((2, 3)), None, params, model)


def test_command_line_as_a_module_without_the_library(tmp_path):
    env = dict(os.environ, HARP_LIB_PATH=str(tmp_path / "no_such_library.so"), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "harp_amd.playback", "--help"], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert "--motion" in r.stdout and "--smooth-keypoints" in r.stdout
