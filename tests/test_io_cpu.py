"""No GPU: harp_amd.io.save_obj (the mirror of pytorch3d.io.save_obj as optimize_sequence.py:785-791 calls it) on small CPU tensors, read
back by the few-line parser below: what went in comes out."""
import io
import os

import numpy as np
import pytest
import torch


def read_obj(path):
    """v / vt / f lines of a Wavefront OBJ -> dict of lists (face indices as written, 1-based)"""
    out = dict(v=[], vt=[], f=[], ft=[], mtllib=[], usemtl=[])
    for ln in open(path).read().splitlines():
        k, *rest = ln.split()
        if k in ("v", "vt"):
            out[k].append([float(x) for x in rest])
        elif k == "f":
            c = [x.split("/") for x in rest]
            out["f"].append([int(x[0]) for x in c])
            if len(c[0]) > 1:
                out["ft"].append([int(x[1]) for x in c])
        else:
            out[k].append(rest[0])
    return out


def _mesh(seed=0, V=7, F=5, VT=9):
    g = torch.Generator().manual_seed(seed)
    verts = torch.randn(V, 3, generator=g) * 0.1 + torch.tensor([0.02, -0.01, 0.45])
    faces = torch.randint(0, V, (F, 3), generator=g)
    faces[0] = torch.tensor([V - 1, 0, 1])                       # the last vertex is used
    verts_uvs = torch.rand(VT, 2, generator=g)
    faces_uvs = torch.randint(0, VT, (F, 3), generator=g)
    faces_uvs[0] = torch.tensor([VT - 1, 0, 2])
    tex = torch.rand(6, 4, 3, generator=g)                       # H != W: a transposed or flipped image would show
    tex[0, 0], tex[5, 3] = torch.tensor([1.0, 0.0, 0.999]), torch.tensor([0.0, 1.0, 0.5])
    return verts, faces, verts_uvs, faces_uvs, tex


def test_textured_round_trip(tmp_path):
    from PIL import Image
    from harp_amd.io import save_obj
    verts, faces, verts_uvs, faces_uvs, tex = _mesh()
    p = tmp_path / "0007.obj"
    save_obj(str(p), verts=verts, faces=faces, verts_uvs=verts_uvs, faces_uvs=faces_uvs, texture_map=tex)
    assert sorted(os.listdir(tmp_path)) == ["0007.mtl", "0007.obj", "0007.png"]
    o = read_obj(p)
    assert o["mtllib"] == ["0007.mtl"] and o["usemtl"] == ["mesh"]
    assert open(p).read().splitlines()[:2] == ["mtllib 0007.mtl", "usemtl mesh"]
    assert (len(o["v"]), len(o["vt"]), len(o["f"]), len(o["ft"])) == (7, 9, 5, 5)
    assert (torch.tensor(o["f"]) - 1).equal(faces) and (torch.tensor(o["ft"]) - 1).equal(faces_uvs)        # 1-based in the file
    assert (torch.tensor(o["v"], dtype=torch.float64) - verts.double()).abs().max() <= 5e-7                # '%f': six decimals
    assert (torch.tensor(o["vt"], dtype=torch.float64) - verts_uvs.double()).abs().max() <= 5e-7
    for ln in open(p).read().splitlines():
        if ln.startswith("v "):
            assert all(len(x.split(".")[1]) == 6 for x in ln.split()[1:]), ln
    mtl = open(tmp_path / "0007.mtl").read().split()
    assert mtl[mtl.index("newmtl") + 1] == "mesh" and mtl[mtl.index("map_Kd") + 1] == "0007.png"
    im = Image.open(tmp_path / "0007.png")
    assert im.mode == "RGB" and im.size == (4, 6)
    want = (tex * 255.0).to(torch.uint8).numpy()                 # truncated, rows as given
    assert np.array_equal(np.asarray(im), want)
    assert want[0, 0].tolist() == [255, 0, 254] and want[5, 3].tolist() == [0, 255, 127]


@pytest.mark.parametrize("places", [2, 8])
def test_decimal_places(tmp_path, places):
    from harp_amd.io import save_obj
    verts, faces, verts_uvs, faces_uvs, _ = _mesh(1)
    p = tmp_path / "m.obj"
    save_obj(p, verts.double(), faces, decimal_places=places, verts_uvs=verts_uvs, faces_uvs=faces_uvs)      # a PathLike, float64, no texture
    assert os.listdir(tmp_path) == ["m.obj"]
    o = read_obj(p)
    assert not o["mtllib"] and not o["usemtl"] and len(o["vt"]) == 9 and (torch.tensor(o["ft"]) - 1).equal(faces_uvs)
    assert (torch.tensor(o["v"], dtype=torch.float64) - verts.double()).abs().max() <= 0.5 * 10.0 ** -places + 1e-15
    for ln in open(p).read().splitlines():
        if ln[0] == "v":
            assert all(len(x.split(".")[1]) == places for x in ln.split()[1:]), ln


def test_plain_mesh_has_no_side_files(tmp_path):
    from harp_amd.io import save_obj
    verts, faces, _, _, _ = _mesh(2)
    p = tmp_path / "plain.obj"
    save_obj(str(p), verts, faces)
    assert os.listdir(tmp_path) == ["plain.obj"]
    lines = open(p).read().splitlines()
    assert len(lines) == 7 + 5 and all(ln.startswith("v ") for ln in lines[:7]) and all(ln.startswith("f ") and "/" not in ln for ln in lines[7:])
    o = read_obj(p)
    assert (torch.tensor(o["f"]) - 1).equal(faces) and not o["vt"] and not o["ft"]


def test_pre_encoded_png_is_written_verbatim(tmp_path):
    from PIL import Image
    from harp_amd.io import encode_png, save_obj
    verts, faces, verts_uvs, faces_uvs, tex = _mesh(3)
    png = encode_png(tex)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(png))), (tex * 255.0).to(torch.uint8).numpy())
    marked = png + b"trailing bytes no encoder would write"
    for name in ("a", "b"):
        save_obj(str(tmp_path / f"{name}.obj"), verts, faces, verts_uvs=verts_uvs, faces_uvs=faces_uvs, texture_png=marked)
        assert open(tmp_path / f"{name}.png", "rb").read() == marked
        assert f"map_Kd {name}.png" in open(tmp_path / f"{name}.mtl").read()


def test_refuses_what_it_cannot_write(tmp_path):
    from harp_amd.io import save_obj
    verts, faces, verts_uvs, faces_uvs, tex = _mesh(4)
    p = str(tmp_path / "x.obj")
    with pytest.raises(ValueError, match="together"):
        save_obj(p, verts, faces, verts_uvs=verts_uvs)
    with pytest.raises(ValueError, match="texture needs"):
        save_obj(p, verts, faces, texture_map=tex)
    with pytest.raises(ValueError, match="index"):
        save_obj(p, verts, faces + 7)
    with pytest.raises(ValueError, match="index"):
        save_obj(p, verts, faces, verts_uvs=verts_uvs, faces_uvs=faces_uvs + 9)
    with pytest.raises(ValueError, match="must match"):
        save_obj(p, verts, faces, verts_uvs=verts_uvs, faces_uvs=faces_uvs[:3])
    assert os.listdir(tmp_path) == []
