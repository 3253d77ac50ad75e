"""No GPU: the host-side playback helpers of harp_amd.utils.visualize — change_pose (utils/visualize.py:111-142), save_gif (:349-355) and
concat_image_in_dir (:322-345)."""
import os

import numpy as np
import torch
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "change_pose.npz")


def test_change_pose_sets_the_demo_pose_of_frame_0_only():
    from harp_amd.utils.visualize import change_pose
    want = np.load(GOLDEN)["pose"]
    assert want.shape == (45,)
    g = torch.Generator().manual_seed(0)
    params = {"pose": torch.randn(4, 45, generator=g), "rot": torch.randn(4, 3, generator=g), "shape": torch.randn(10, generator=g)}
    before = {k: v.clone() for k, v in params.items()}
    out = change_pose(params, 7)
    assert out is params
    assert np.array_equal(params["pose"][0].numpy(), want.astype(np.float32))
    assert torch.equal(params["pose"][1:], before["pose"][1:])
    assert torch.equal(params["rot"], before["rot"]) and torch.equal(params["shape"], before["shape"])
    wide = {"pose": torch.randn(2, 48, generator=g)}                       # only columns 0..44 are written
    keep = wide["pose"].clone()
    change_pose(wide, 0)
    assert torch.equal(wide["pose"][0, 45:], keep[0, 45:]) and torch.equal(wide["pose"][1], keep[1])
    leaf = {"pose": torch.zeros(2, 45, requires_grad=True)}                # fitted parameters are leaves
    change_pose(leaf, 0)
    assert np.array_equal(leaf["pose"][0].detach().numpy(), want.astype(np.float32))


def _jpg(path, value, size=(12, 8)):
    a = np.zeros((size[1], size[0], 3), np.uint8)
    a[..., 0], a[..., 1], a[: size[1] // 2, :, 2] = value, 255 - value, value
    Image.fromarray(a).save(path)


def test_save_gif_takes_the_sorted_jpgs(tmp_path):
    from harp_amd.utils.visualize import save_gif
    d = tmp_path / "frames"
    d.mkdir()
    for name, v in (("h_0000.jpg", 250), ("0001.jpg", 90), ("0000.jpg", 10), ("0002.jpg", 170)):
        _jpg(str(d / name), v)
    Image.fromarray(np.zeros((8, 12, 3), np.uint8)).save(str(d / "ignored.png"))       # *.jpg only, as the reference globs
    n = save_gif(str(d), str(d / "out.gif"))
    assert n == 4
    gif = Image.open(str(d / "out.gif"))
    assert gif.n_frames == 4 and gif.size == (12, 8)
    reds = []
    for k in range(4):
        gif.seek(k)
        assert gif.info["duration"] == 100
        reds.append(int(np.asarray(gif.convert("RGB"))[0, 0, 0]))
    assert reds[0] < reds[1] < reds[2] < reds[3], reds                       # 0000, 0001, 0002, h_0000: sorted by name


def test_concat_image_in_dir(tmp_path):
    from harp_amd.utils.visualize import concat_image_in_dir
    d1, d2, out = tmp_path / "a", tmp_path / "b", tmp_path / "combined"
    d1.mkdir(); d2.mkdir()
    for name, v in (("0001.jpg", 200), ("0000.jpg", 20), ("0002.jpg", 120)):
        _jpg(str(d1 / name), v)
    Image.fromarray(np.full((8, 12, 3), 33, np.uint8)).save(str(d2 / "0000.png"))      # .png and .jpg are both picked up
    _jpg(str(d2 / "0001.jpg"), 240)
    (d2 / "notes.txt").write_text("not an image")
    strips = concat_image_in_dir(str(d1), str(d2), str(out))
    assert len(strips) == 2                                                   # the longer directory's surplus (a/0002.jpg) is ignored
    assert sorted(os.listdir(str(out))) == ["0000.jpg", "0001.jpg", "out.gif"]
    for k in range(2):
        im = Image.open(str(out / ("%04d.jpg" % k)))
        assert im.size == (24, 8)
        assert strips[k].shape == (8, 24, 3) and strips[k].dtype == np.uint8
    # a/0000.jpg | b/0000.png, a/0001.jpg | b/0001.jpg (JPEG is lossy: the files' red levels 20 / 200 / 240 are 60 or more apart, so
    # 16 levels tell them apart; the PNG is exact)
    assert abs(int(strips[0][0, 0, 0]) - 20) <= 16 and np.all(strips[0][:, 12:] == 33)
    assert abs(int(strips[1][0, 0, 0]) - 200) <= 16 and abs(int(strips[1][0, 12, 0]) - 240) <= 16
    assert Image.open(str(out / "out.gif")).n_frames == 2
