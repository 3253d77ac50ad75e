"""The pure parts of the post-fit evaluation (harp_amd/evaluate.py): the 64-frame chunk averaging, the result file, the host path of the
frame batches, the re-exports of optimize_sequence, and the import without the built library.  No GPU, no library."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 70, 128, 130)                            # one short chunk; one frame under, at and over a chunk; two chunks and two over


def _chunks(n):
    return [slice(c, min(n, c + 64)) for c in range(0, n, 64)]


@pytest.mark.parametrize("n", SIZES)
def test_chunk_mean_against_float64_numpy(n):
    """the reference's "mean of the 64-frame chunk means" restated in numpy.  Random values: both sides are float64 and differ only in the
    order of at most 64 additions per chunk and one division, so by n * 2^-53 relative at the very most — 1e-13 leaves a factor of 7 at
    n = 130.  Integer-valued inputs: every sum is exact in any order, so the result is the restatement's to the bit — for the L1 form that
    pins its arithmetic, ONE division of the chunk's sum by (frames * values per frame)."""
    from harp_amd.evaluate import EVAL_CHUNK, chunk_mean
    assert EVAL_CHUNK == 64
    g = np.random.default_rng(n)
    per_pixel = float(176 * 176 * 3)
    v = g.random(n)
    sums = g.random(n) * per_pixel                               # L1 arrives as per-frame sums of |y_true - y_pred|
    want = np.mean([v[c].mean() for c in _chunks(n)])
    want_l1 = np.mean([sums[c].sum() / ((c.stop - c.start) * per_pixel) for c in _chunks(n)])
    got, got_l1 = chunk_mean(torch.from_numpy(v), n), chunk_mean(torch.from_numpy(sums), n, per_frame=per_pixel)
    assert isinstance(got, float) and isinstance(got_l1, float)
    assert abs(got - want) <= 1e-13 * abs(want) and abs(got_l1 - want_l1) <= 1e-13 * abs(want_l1), (got, want, got_l1, want_l1)
    k = g.integers(0, 1 << 30, n).astype(np.float64)
    assert chunk_mean(torch.from_numpy(k), n) == float(np.mean([k[c].sum() / (c.stop - c.start) for c in _chunks(n)]))
    assert chunk_mean(torch.from_numpy(k), n, per_frame=per_pixel) == float(np.mean([k[c].sum() / ((c.stop - c.start) * per_pixel) for c in _chunks(n)]))


def test_chunk_mean_weighs_chunks_not_frames():
    """65 frames: the single frame of the second chunk counts as much as the 64 of the first (the reference's np.mean over image_eval's results)"""
    from harp_amd.evaluate import chunk_mean
    v = torch.cat([torch.zeros(64, dtype=torch.float64), torch.ones(1, dtype=torch.float64)])
    assert chunk_mean(v, 65) == 0.5 and chunk_mean(v * 10.0, 65, per_frame=10.0) == 0.5


def test_write_stats(tmp_path, capsys):
    from harp_amd.evaluate import write_stats
    keys = ["Silhouette IoU", "L1", "LPIPS", "MS_SSIM", "Procrustes-aligned joint error (mm)", "Joint AUC 0-50 mm",
            "Procrustes-aligned vertex error (mm)", "Vertex AUC 0-50 mm", "F@5mm", "F@15mm", "Texel coverage"]
    stats = {k: (-1.0) ** i * (i + 1) / 7.0 for i, k in enumerate(keys)}
    write_stats(stats, tmp_path / "eval_results.txt")
    text = open(tmp_path / "eval_results.txt").read()
    assert text == "".join(" %s: %.5f\n" % (k, stats[k]) for k in keys)
    lines = text.splitlines()
    assert [ln.split(":")[0][1:] for ln in lines] == keys
    for ln in lines:
        assert re.fullmatch(r" [A-Za-z0-9_ ()@-]+: -?\d+\.\d{5}", ln), ln
    assert capsys.readouterr().out == "  -- Evaluation --\n" + text
    write_stats({"L1": 0.25}, tmp_path / "eval_results.txt")                 # rewritten, not appended to
    assert open(tmp_path / "eval_results.txt").read() == " L1: 0.25000\n"


def test_frame_batches_from_a_list():
    from harp_amd.evaluate import frame_batches
    g = torch.Generator().manual_seed(5)
    ds = [(10 + i, torch.rand(8, 8, 3, generator=g, dtype=torch.float64), torch.rand(8, 8, 1, generator=g), torch.zeros(8, 8, 1)) for i in range(7)]
    got = list(frame_batches(ds, 3, 8, device="cpu"))
    assert [b.fid.tolist() for b in got] == [[10, 11, 12], [13, 14, 15], [16]]
    lo = 0
    for b in got:
        fid, y_true, y_sil_true = b                                          # a plain 3-tuple as well
        B = fid.shape[0]
        assert fid.dtype == torch.long and y_true.dtype == y_sil_true.dtype == torch.float32
        assert y_true.shape == (B, 8, 8, 3) and y_sil_true.shape == (B, 8, 8)
        assert torch.equal(y_true, torch.stack([d[1] for d in ds[lo:lo + B]]).float())
        assert torch.equal(y_sil_true, torch.stack([d[2][..., 0] for d in ds[lo:lo + B]]))
        lo += B
    ids = [(i, ds[i][1], ds[i][2], ds[i][3]) for i in range(7)]
    assert [b.fid.tolist() for b in frame_batches(ids, 3, 8, device="cpu")] == [[0, 1, 2], [3, 4, 5], [6]]
    assert [b.fid.tolist() for b in frame_batches(ids, 32, 8, device="cpu")] == [list(range(7))]


def test_frame_batches_refuses_device_ingest_without_paths():
    """the ValueError comes from the call itself, not from the first next(): nothing has been rendered or written by then"""
    from harp_amd.evaluate import frame_batches
    ds = [(i, torch.zeros(8, 8, 3), torch.zeros(8, 8, 1), torch.zeros(8, 8, 1)) for i in range(2)]
    with pytest.raises(ValueError, match="image_paths"):
        frame_batches(ds, 3, 8, device="cpu", device_ingest=True)


def test_optimize_sequence_reexports():
    import inspect
    from harp_amd import bake, evaluate, monitor, optimize_sequence
    from harp_amd.utils import visualize
    assert optimize_sequence.evaluate_sequence is evaluate.evaluate_sequence
    assert optimize_sequence.mirror_render is evaluate.mirror_render is monitor.mirror_render
    assert optimize_sequence.EVAL_CHUNK is evaluate.EVAL_CHUNK
    assert optimize_sequence.get_mesh_subdivider is visualize.get_mesh_subdivider is bake.get_mesh_subdivider is monitor.get_mesh_subdivider
    sig = inspect.signature(evaluate.evaluate_sequence)
    assert [(p.name, p.default) for p in sig.parameters.values()][4:] == [
        ("device", "cuda"), ("batch_size", 32), ("uv_mask", None), ("lpips_fn", None), ("panels", False), ("turntable", False), ("panel_hook", None),
        ("export_mesh", False), ("pose_eval", None), ("device_ingest", False), ("coverage", False), ("pad_texture", 0)]
    assert list(sig.parameters)[:4] == ["configs", "params", "images_dataset", "hand_layer"]


def test_params_on():
    from harp_amd.utils.visualize import params_on
    w = torch.nn.Parameter(torch.ones(2, 3))
    faces = [[0, 1, 2]]
    out = params_on({"pose": w, "mesh_faces": faces, "verts_uvs": None}, "cpu")
    assert list(out) == ["pose", "mesh_faces", "verts_uvs"] and out["mesh_faces"] is faces and out["verts_uvs"] is None
    assert not out["pose"].requires_grad and torch.equal(out["pose"], w.detach()) and w.requires_grad


def test_import_without_the_built_library(tmp_path):
    """a fresh interpreter whose library path names no file imports the evaluation and the fit's module; the library is loaded by no import"""
    code = ("import sys; sys.path.insert(0, %r); import harp_amd.evaluate, harp_amd.optimize_sequence, harp_amd._lib as L; "
            "import os; assert not os.path.exists(L.LIB_PATH) and L._lib is None" % ROOT)
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, HARP_LIB_PATH=str(tmp_path / "no_such_library.so")))
