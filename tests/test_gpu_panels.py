"""-m gpu: ops.panels_u8 / harp_panels_u8 (csrc/present.hip) bit-equal to the reference's numpy statement (optimize_sequence.py:744-755),
written out here: colour panels uint8(clip(x, 0, 1) * 255) with the product in float32, the overlay panel uint8(m * 225) with the product
in float64 (np.zeros is float64), concatenated along the width.  Both sides perform the same IEEE operations: no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def numpy_panels(images, mask_true=None, mask_pred=None):
    """the statement of optimize_sequence.py:744-755 per frame; images: (N,H,W,3) float32 arrays"""
    out = []
    for n in range(images[0].shape[0] if images else mask_true.shape[0]):
        cols = [im[n].clip(0, 1) * 255 for im in images]
        if mask_true is not None:
            overlay = np.zeros([*mask_true[n].shape[:2], 3])
            overlay[:, :, 0] = mask_true[n]
            overlay[:, :, 2] = mask_pred[n]
            cols.append(overlay * 225)
        out.append(np.concatenate(cols, axis=1).astype(np.uint8))
    return np.stack(out)


def special_values():
    f = np.float32
    k255 = (np.arange(256, dtype=np.float64) / 255).astype(f)
    k225 = (np.arange(226, dtype=np.float64) / 225).astype(f)
    base = np.concatenate([k255, k225, (np.arange(256, dtype=f) / f(255)), (np.arange(226, dtype=f) / f(225))])
    vals = np.concatenate([base, np.nextafter(base, f(2)), np.nextafter(base, f(-1)), np.array([0.99999994, 0.0, 1.0, -0.0, 1.0000001, -1e-8, 0.5], f)])
    return vals.astype(f)


def images_with_specials(N, S, n_img, seed):
    rng = np.random.default_rng(seed)
    sp = special_values()
    out = []
    for k in range(n_img):
        im = rng.uniform(-0.5, 1.5, size=(N, S, S, 3)).astype(np.float32)
        flat = im.reshape(-1)
        idx = rng.permutation(flat.size)[:min(flat.size // 2, 4 * sp.size)]
        flat[idx] = np.resize(sp, idx.size)
        out.append(im)
    return out


def masks_with_specials(N, S, seed):
    rng = np.random.default_rng(seed + 100)
    sp = special_values()
    sp = sp[(sp >= 0) & (sp <= 1)]
    ms = []
    for k in range(2):
        m = rng.uniform(0, 1, size=(N, S, S)).astype(np.float32)
        flat = m.reshape(-1)
        idx = rng.permutation(flat.size)[:min(flat.size // 2, 2 * sp.size)]
        flat[idx] = np.resize(sp, idx.size)
        if k == 1:
            m = (m > 0.5).astype(np.float32) if S > 100 else m          # a hard silhouette as the dataset's, at the large size
        ms.append(m)
    return ms


@pytest.mark.parametrize("S,N", [(31, 3), (512, 2)])
@pytest.mark.parametrize("n_img,masks", [(1, False), (3, True), (3, False), (2, True), (0, True)])
def test_panels_bit_equal_to_numpy(S, N, n_img, masks):
    from harp_amd import ops
    imgs = images_with_specials(N, S, n_img, seed=S + n_img)
    mt, mp = masks_with_specials(N, S, seed=S) if masks else (None, None)
    want = numpy_panels(imgs, mt, mp)
    P = n_img + int(masks)
    assert want.shape == (N, S, P * S, 3) and want.dtype == np.uint8
    d = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    got = ops.panels_u8([d(im) for im in imgs], d(mt), d(mp))
    assert got.dtype == torch.uint8 and got.shape == want.shape and got.is_cuda
    g = got.cpu().numpy()
    assert np.array_equal(g, want), (int((g != want).sum()), np.argwhere(g != want)[:5])
    if masks:
        got1 = ops.panels_u8([d(im) for im in imgs], d(mt)[..., None], d(mp)[..., None])      # the dataset's (N,S,S,1) masks
        assert torch.equal(got1, got)


@pytest.mark.parametrize("S", [31, 512])
def test_strided_inputs(S):
    """the first three channels of a 4-channel normal image and an NCHW view, read in place"""
    from harp_amd import ops
    N = 2
    a, b = images_with_specials(N, S, 2, seed=7)
    want = numpy_panels([a, b])
    rgba = torch.cat([torch.from_numpy(a), torch.full((N, S, S, 1), 7.0)], -1).to(DEV)
    nchw = torch.from_numpy(b).permute(0, 3, 1, 2).contiguous().to(DEV)
    got = ops.panels_u8([rgba[..., 0:3], nchw.permute(0, 2, 3, 1)])
    assert np.array_equal(got.cpu().numpy(), want)
    got2 = ops.panels_u8([nchw], channels_last=False)
    assert np.array_equal(got2.cpu().numpy(), numpy_panels([b]))
    assert np.array_equal(ops.panels_u8(rgba).cpu().numpy(), numpy_panels([a]))                    # 4 channels: the first three


def test_panels_refuse_bad_arguments():
    from harp_amd import _lib, ops
    import ctypes
    L = _lib.lib()
    f = 1 << 20
    one = (ctypes.c_void_p * 1)(f)
    st = (ctypes.c_longlong * 4)(48, 12, 3, 1)
    assert L.harp_panels_u8(one, st, 1, None, None, 1, 4, 4, None, None) == 1
    assert L.harp_panels_u8(one, st, 4, None, None, 1, 4, 4, f, None) == 1
    assert L.harp_panels_u8(one, st, 1, f, None, 1, 4, 4, f, None) == 1
    assert L.harp_panels_u8(None, None, 0, None, None, 1, 4, 4, f, None) == 1
    assert L.harp_panels_u8(one, st, 1, None, None, 0, 4, 4, f, None) == 1
    assert L.harp_panels_u8(one, (ctypes.c_longlong * 4)(48, -12, 3, 1), 1, None, None, 1, 4, 4, f, None) == 1
    x = torch.zeros(1, 4, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.panels_u8(x)
    with pytest.raises(ValueError):
        ops.panels_u8([x.to(DEV)] * 4)
    with pytest.raises(ValueError):
        ops.panels_u8(x.to(DEV), mask_true=torch.zeros(1, 4, 4, device=DEV))
