"""-m gpu: the device-side target ingest — ops.targets_from_u8 (csrc/ingest.hip) against the numpy restatement tests/_ingest_ref.py, which
tests/test_ingest_cpu.py pins to the host path; ResidentTargets(ingest="device") against ResidentTargets (the host path) from files;
optimize_hand_sequence / evaluate_sequence with device_ingest=True.  Every comparison is torch.equal: the feature's claim is bit identity.
Tile of the kernel: 16 rows x 64 columns with a halo of 2 — tests/_ingest_ref.SIZES puts its edges at every offset from the image's."""
import numpy as np
import pytest
import torch

from tests import _ingest_ref as R
from tests._scene import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = -7.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(rgb, mask, d, what):
    from harp_amd import ops
    got = ops.targets_from_u8(_dev(rgb), _dev(mask), d=d)
    for name, g, w in zip(("y_true", "y_sil", "y_sil_col"), got, R.targets(rgb, mask, d)):
        assert g.dtype == torch.float32 and torch.equal(g.cpu(), torch.from_numpy(w)), (what, d, name)


@pytest.mark.parametrize("H0,W0", R.SIZES)
def test_resident_targets_from_files(tmp_path, H0, W0):
    """ingest="device" == the host path, for d in 1..3, N in 1, 3 and chunks that reuse a staging buffer (1), end short (2) and hold all (32)"""
    from harp_amd.utils.data_util import ImagesDataset, ResidentTargets
    ips, mps = R.write_files(tmp_path, *R.make_frames(3, H0, W0, seed=H0 * 1000 + W0))
    for d in R.FACTORS:
        ds = ImagesDataset(ips, mps, downsample_factor=d)
        host = ResidentTargets(ds, frames=[2, 0, 1])
        for frames in ([2], [2, 0, 1]):
            n = len(frames)
            for chunk in (1, 2, 32):
                rt = ResidentTargets(ds, frames=frames, device=DEV, ingest="device", chunk=chunk, workers=2)
                assert torch.equal(rt.fid, host.fid[:n]) and rt.fid.dtype == host.fid.dtype and len(rt) == n
                for name, g, w in zip(("y_true", "y_sil", "y_sil_col"), rt.tensors(), host.tensors()):
                    assert g.is_cuda and g.shape == w[:n].shape and torch.equal(g.cpu(), w[:n]), (d, n, chunk, name)
                assert rt.ingest_stats()["chunks"] == -(-n // min(chunk, n))
    rt = ResidentTargets(ds, device=DEV, ingest="device", eroded=False)
    assert rt.y_sil_col is None and torch.equal(rt.y_sil.cpu(), ResidentTargets(ds).y_sil)


def test_every_code():
    """an RGB ramp and a mask that hold all 256 codes: the division is the float64 route's for each of them"""
    ramp = (np.arange(4 * 64 * 3) % 256).astype(np.uint8).reshape(1, 4, 64, 3)
    mask = np.arange(256, dtype=np.uint8).reshape(1, 4, 64)
    assert len(np.unique(ramp)) == 256
    _check(ramp, mask, 1, "ramp")
    _check(np.ascontiguousarray(ramp[:, :, ::-1]), np.ascontiguousarray(mask[:, ::-1, ::-1]), 1, "ramp reversed")


@pytest.mark.parametrize("H0,W0", R.SIZES + [(40, 200)])
def test_random_and_constant_masks(H0, W0):
    g = np.random.default_rng(H0 * 77 + W0)
    rgb = g.integers(0, 256, (2, H0, W0, 3), dtype=np.uint8)
    for d in R.FACTORS:
        _check(rgb, g.integers(0, 256, (2, H0, W0), dtype=np.uint8), d, "random")
        _check(rgb, np.full((2, H0, W0), 255, np.uint8), d, "all 255")


@pytest.mark.parametrize("H0,W0", [(5, 5), (19, 67), (33, 130)])
def test_single_zero(H0, W0):
    """one 0 in a mask of 255 at each corner, at each edge midpoint and at (2, 2): the eroded mask is 0 on the clipped 5 x 5 block around it"""
    ys, xs = (0, H0 // 2, H0 - 1), (0, W0 // 2, W0 - 1)
    spots = [(y, x) for y in ys for x in xs if (y, x) != (H0 // 2, W0 // 2)] + [(2, 2)]
    mask = np.full((len(spots), H0, W0), 255, np.uint8)
    for k, (y, x) in enumerate(spots):
        mask[k, y, x] = 0
    rgb = np.zeros((len(spots), H0, W0, 3), np.uint8)
    _check(rgb, mask, 1, "single zero")
    from harp_amd import ops
    col = ops.targets_from_u8(_dev(rgb), _dev(mask))[2].cpu()
    for k, (y, x) in enumerate(spots):
        want = torch.ones(H0, W0)
        want[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = 0
        assert torch.equal(col[k], want), (y, x)


@pytest.mark.parametrize("H0,W0,d", [(16, 64, 1), (17, 65, 1), (19, 67, 2)])
def test_out_slices_and_eroded_false(H0, W0, d):
    """out = slices of larger buffers: the neighbouring frames keep their poison (at 17 x 65 the slices start off every 16-byte boundary);
    eroded=False returns None and leaves out[2] as it was"""
    from harp_amd import ops
    rgb, mask = R.make_frames(2, H0, W0, seed=9)
    want = [torch.from_numpy(w) for w in R.targets(rgb, mask, d)]
    H, W = want[1].shape[1:]
    bufs = [torch.full((5, H, W, 3), POISON, device=DEV), torch.full((5, H, W), POISON, device=DEV), torch.full((5, H, W), POISON, device=DEV)]
    for eroded in (True, False):
        for b in bufs:
            b.fill_(POISON)
        got = ops.targets_from_u8(_dev(rgb), _dev(mask), d=d, eroded=eroded, out=tuple(b[2:4] for b in bufs))
        assert (got[2] is None) == (not eroded)
        for k, (b, w) in enumerate(zip(bufs, want)):
            b = b.cpu()
            assert bool((b[:2] == POISON).all()) and bool((b[4:] == POISON).all()), (eroded, k)
            if k == 2 and not eroded:
                assert bool((b == POISON).all())
            else:
                assert got[k].data_ptr() == bufs[k][2:4].data_ptr() and torch.equal(b[2:4], w), (eroded, k)


def test_refusals():
    """the C entry point's HARP_ERR_ARG exits on real buffers (nothing is written), and the wrapper's own errors"""
    from harp_amd import _lib, ops
    rgb, mask = _dev(np.zeros((1, 4, 4, 3), np.uint8)), _dev(np.zeros((1, 4, 4), np.uint8))
    outs = [torch.full((1, 4, 4, 3), POISON, device=DEV), torch.full((1, 4, 4), POISON, device=DEV), torch.full((1, 4, 4), POISON, device=DEV)]
    p = [t.data_ptr() for t in (rgb, mask, *outs)]
    for y_col in (p[4], None):
        for what, status in R.bad_argument_calls(_lib.lib().harp_targets_from_u8, p[0], p[1], p[2], p[3], y_col):
            assert status == 1, what
    torch.cuda.synchronize()
    assert all(bool((t == POISON).all()) for t in outs)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.targets_from_u8(rgb.cpu(), mask.cpu())
    with pytest.raises(TypeError):
        ops.targets_from_u8(rgb.float(), mask)
    with pytest.raises(ValueError):
        ops.targets_from_u8(rgb, mask, d=9)
    with pytest.raises(ValueError):
        ops.targets_from_u8(rgb, mask[:, :3])
    with pytest.raises(ValueError):
        ops.targets_from_u8(rgb, mask, out=(outs[0], outs[1], outs[2][:, :3]))


# ---- the fit and the evaluation from files ----------------------------------------------------------------------------------------------
T, S = 4, 64


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.utils.data_util import ImagesDataset
    sc = make_scene(T=T, S=S, seed=11)
    g = np.random.default_rng(11)
    rgb = g.integers(0, 256, (T, S, S, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:S, :S]
    mask = np.stack([np.where((yy - 30 - t) ** 2 + (xx - 33) ** 2 < 18 ** 2, 255 - 3 * t, 2 * t) for t in range(T)]).astype(np.uint8)
    ds = ImagesDataset(*R.write_files(tmp_path_factory.mktemp("frames"), rgb, mask), downsample_factor=1)
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=sc["model_np"], device=DEV)
    uvs = (torch.from_numpy(sc["tpl"]["verts_uvs"])[None], torch.from_numpy(sc["tpl"]["faces_uvs"])[None])
    return sc, ds, layer, uvs


def _config(sc, out, **kw):
    from harp_amd.utils.config_utils import get_config
    return get_config(write_yaml=False, use_arm=False, img_size=S, focal_length=sc["focal"], base_output_dir=str(out) + "/", **kw)


def test_fit_from_files(scene, tmp_path, monkeypatch):
    """optimize_hand_sequence(device_ingest=True): the engine holds the targets of a device_ingest=False run bit for bit, the monitor's
    validation frames come the same way, ImagesDataset.__getitem__ is never called, the loss is finite.  (The fitted parameters are not
    compared: the step's float atomics are not run-to-run deterministic.)"""
    import os
    from harp_amd.optimize_sequence import optimize_hand_sequence
    from harp_amd.utils.data_util import ImagesDataset
    sc, ds, layer, uvs = scene
    kept = {}

    def fit(name, **kw):
        out = tmp_path / name
        out.mkdir()
        seen = []

        def log(epoch, loss, eng):
            seen.append(loss)
            kept[name] = [t.clone() for t in (eng.y_true, eng.y_sil, eng.y_sil_col)]
        optimize_hand_sequence(_config(sc, out, total_epoch=2, training_stage=[1, 1, 0]), sc["seq"], ds, kw.pop("val", None), kw.pop("val_ds", None),
                               layer, *uvs, device=DEV, uv_mask=sc["uv_mask"], batch_size=2, log_fn=log, **kw)
        assert len(seen) == 2 and all(np.isfinite(seen)), seen
        return out

    fit("host")
    with monkeypatch.context() as mp:
        def never(self, ix):
            raise AssertionError("ImagesDataset.__getitem__ called with device_ingest=True")
        mp.setattr(ImagesDataset, "__getitem__", never)
        val = {k: sc["seq"][k].float() for k in ("cam", "trans", "rot")}
        out = fit("device", device_ingest=True, monitor=True, val=val, val_ds=ds)
    assert os.path.exists(out / "val_0000.jpg")
    for name, a, b in zip(("y_true", "y_sil", "y_sil_col"), kept["host"], kept["device"]):
        assert a.shape == b.shape == ((T, S, S, 3) if name == "y_true" else (T, S, S)) and torch.equal(a, b), name
    lists = [(i, torch.zeros(S, S, 3), torch.zeros(S, S, 1), torch.zeros(S, S)) for i in range(T)]
    with pytest.raises(ValueError, match="image_paths"):                       # no silent fall-back for a dataset without files
        optimize_hand_sequence(_config(sc, tmp_path, total_epoch=1, training_stage=[1, 0, 0]), sc["seq"], lists, None, None, layer, *uvs, device=DEV,
                               uv_mask=sc["uv_mask"], batch_size=2, device_ingest=True)


@pytest.mark.filterwarnings("ignore:MS_SSIM left out")
def test_evaluate_from_files(scene, tmp_path, monkeypatch):
    """evaluate_sequence(device_ingest=True) writes the lines of device_ingest=False byte for byte: same inputs, deterministic kernels"""
    from harp_amd.optimize_sequence import evaluate_sequence, init_params
    from harp_amd.utils.data_util import ImagesDataset
    sc, ds, layer, uvs = scene
    text = {}
    for name, flag in (("host", False), ("device", True)):
        out = tmp_path / name
        out.mkdir()
        cfg = _config(sc, out)
        params = init_params(sc["seq"], True, True, None, layer.th_faces, False, *uvs, configs=cfg, device=DEV, uv_mask=sc["uv_mask"])
        with monkeypatch.context() as mp:
            if flag:
                mp.setattr(ImagesDataset, "__getitem__", lambda self, ix: (_ for _ in ()).throw(AssertionError("__getitem__ called")))
            stats = evaluate_sequence(cfg, params, ds, layer, device=DEV, batch_size=3, device_ingest=flag)
        assert all(np.isfinite(v) for v in stats.values()), stats
        text[name] = open(out / "eval_results.txt", "rb").read()
    assert text["host"] == text["device"] and text["host"].count(b"\n") == 2, text
    lists = [(i, torch.zeros(S, S, 3), torch.zeros(S, S, 1), torch.zeros(S, S)) for i in range(T)]
    with pytest.raises(ValueError, match="image_paths"):
        evaluate_sequence(_config(sc, tmp_path), params, lists, layer, device=DEV, device_ingest=True)
