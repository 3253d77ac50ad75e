"""No GPU: the device-side target ingest (csrc/ingest.hip, utils/data_util.decode_u8) as far as it goes on the host.  The numpy
restatement tests/_ingest_ref.py — the reference of tests/test_gpu_ingest.py — equals the existing host path (load_img through
torch.Tensor) bit for bit for every size and subsampling factor of the GPU test; the float32 division equals the float64 route for all
256 codes; decode_u8 is deterministic over its thread count and refuses what it cannot stack; harp_targets_from_u8 refuses its bad
arguments before any launch."""
import numpy as np
import pytest
import torch

from tests import _ingest_ref as R


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("H0,W0", R.SIZES)
def test_restatement_equals_host_path(tmp_path, H0, W0):
    from harp_amd.utils.data_util import load_img
    rgb, mask = R.make_frames(2, H0, W0, seed=H0 * 1000 + W0)
    ips, mps = R.write_files(tmp_path, rgb, mask)
    for d in R.FACTORS:
        y_true, y_sil, y_col = R.targets(rgb, mask, d)
        for i in range(2):
            assert torch.equal(load_img(ips[i], downsample_factor=d, torch_tensor=True), torch.from_numpy(y_true[i])), (d, i)
            assert torch.equal(load_img(mps[i], downsample_factor=d, torch_tensor=True, load_mask=True)[..., 0], torch.from_numpy(y_sil[i])), (d, i)
            assert torch.equal(load_img(mps[i], downsample_factor=d, torch_tensor=True, load_mask=True, erode=True),
                               torch.from_numpy(y_col[i])), (d, i)


def test_float32_division_equals_float64_route():
    u = np.arange(256, dtype=np.uint8)
    want = R.unit(u)
    assert np.array_equal(u.astype(np.float32) / np.float32(255), want)
    assert torch.equal(torch.from_numpy(u).float() / 255.0, torch.from_numpy(want))
    assert not np.array_equal(u.astype(np.float32) * np.float32(1 / 255), want)        # why the kernel divides


def test_decode_u8_is_deterministic_over_workers(tmp_path):
    from harp_amd.utils.data_util import ImagesDataset, decode_u8, default_workers
    rgb, mask = R.make_frames(7, 19, 67, seed=5)
    ds = ImagesDataset(*R.write_files(tmp_path, rgb, mask), downsample_factor=2)
    order = [4, 0, 6, 6, 1]
    a = decode_u8(ds, order, workers=1)
    b = decode_u8(ds, order, workers=4)
    for x, y, src in zip(a, b, (rgb, mask)):
        assert x.dtype == np.uint8 and x.tobytes() == y.tobytes() and np.array_equal(x, src[order])      # full size: d belongs to the kernel
    out = (np.zeros((5, 19, 67, 3), np.uint8), np.zeros((5, 19, 67), np.uint8))
    got = decode_u8(ds, order, out=out)
    assert got[0] is out[0] and got[1] is out[1] and np.array_equal(out[0], a[0]) and np.array_equal(out[1], a[1])
    assert 1 <= default_workers() <= 16


def test_decode_u8_refuses_what_it_cannot_stack(tmp_path):
    from harp_amd.utils.data_util import ImagesDataset, ResidentTargets, decode_u8
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    ips, mps = R.write_files(tmp_path / "a", *R.make_frames(3, 8, 12, seed=1))
    ips2, mps2 = R.write_files(tmp_path / "b", *R.make_frames(1, 8, 13, seed=2))
    with pytest.raises(ValueError, match="0000.png"):                                    # a frame of another size, named
        decode_u8(ImagesDataset(ips + ips2, mps + mps2, 1), range(4), workers=2)
    with pytest.raises(ValueError, match="0000_mask.png"):                               # a mask that does not fit its image, named
        decode_u8(ImagesDataset(ips, [mps2[0]] + mps[1:], 1), range(3), workers=2)
    frames = [(i, torch.zeros(8, 12, 3), torch.zeros(8, 12, 1), torch.zeros(8, 12)) for i in range(3)]
    with pytest.raises(ValueError, match="image_paths"):                                 # an in-memory dataset: nothing to decode
        decode_u8(frames, range(3))
    with pytest.raises(ValueError, match="image_paths"):
        ResidentTargets(frames, device="cuda", ingest="device")
    with pytest.raises(ValueError, match="HIP device"):
        ResidentTargets(ImagesDataset(ips, mps, 1), device="cpu", ingest="device")
    with pytest.raises(ValueError):
        ResidentTargets(ImagesDataset(ips, mps, 1), ingest="gpu")


def test_symbol_is_declared_and_bound(lib):
    """fails without csrc/ingest.hip: the library has no such symbol"""
    import ctypes
    from harp_amd import _lib
    assert "harp_targets_from_u8" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "harp_targets_from_u8")
    # the one refusal that needs no pointer at all: nothing is NULL-checked after it, nothing could launch on NULL buffers before it
    assert lib.harp_targets_from_u8(None, None, 0, 0, 0, 0, None, None, None, None) == 1


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: an entry point that lost a check would launch on them "
                                                      "(tests/test_gpu_ingest.py runs the same calls on real buffers)")
def test_entry_point_refuses_bad_arguments_without_launch(lib):
    """HARP_ERR_ARG (1) for every bad argument include/harp_hip.h lists, in the style of tests/test_abi.py: fake device pointers that are
    never dereferenced.  Most of these calls have a non-empty grid, hence the skip where a GPU is visible."""
    f = 1 << 20
    for what, status in R.bad_argument_calls(lib.harp_targets_from_u8, f, f, f, f, f):
        assert status == 1, what
    for what, status in R.bad_argument_calls(lib.harp_targets_from_u8, f, f, f, f, None):       # ... and without the eroded output
        assert status == 1, what
