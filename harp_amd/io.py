"""Mirror of `pytorch3d.io.save_obj` as the reference calls it when it exports the fitted meshes (optimize_sequence.py:781-791):
import swap `from pytorch3d.io import save_obj` -> `from harp_amd.io import save_obj`.

Own code, written from the Wavefront OBJ / MTL formats: what is pinned is that the files read back to the tensors that went in
(tests/test_io_cpu.py), not byte identity with PyTorch3D's writer."""
import io
import os

import numpy as np
import torch


def encode_png(texture_map):
    """PNG bytes of a (H,W,3) float texture in [0, 1] (the caller clamps, as the reference does): uint8(texture_map * 255), truncated,
    rows as given (no flip).  For a texture shared by many meshes: encode once, hand the bytes to save_obj(texture_png=)."""
    from PIL import Image
    t = torch.as_tensor(texture_map).detach().cpu()
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"texture_map must be (H,W,3), got {tuple(t.shape)}")
    buf = io.BytesIO()
    Image.fromarray((t.float() * 255.0).to(torch.uint8).numpy()).save(buf, format="PNG")
    return buf.getvalue()


def _rows(prefix, a, fmt):
    """one '<prefix> x y ...' line per row of the 2-D array a"""
    if a.shape[0] == 0:
        return ""
    line = prefix + (" " + fmt) * a.shape[1] + "\n"
    return (line * a.shape[0]) % tuple(a.reshape(-1).tolist())


def save_obj(f, verts, faces, decimal_places=None, *, verts_uvs=None, faces_uvs=None, texture_map=None, texture_png=None):
    """Write a mesh as `<name>.obj`; with UVs and a texture also `<name>.mtl` and `<name>.png` next to it.

    f: path of the .obj.  verts (V,3) float, faces (F,3) int, 0-based.  decimal_places: None -> '%f', n -> '%.<n>f'.
    verts_uvs (VT,2) + faces_uvs (F,3): `vt u v` lines and `f a/ta b/tb c/tc` faces (both or neither).
    texture_map (H,W,3) in [0, 1], or texture_png = the bytes encode_png gave for it (written verbatim): the .obj then opens with
    `mtllib <name>.mtl` / `usemtl mesh`, the .mtl names `<name>.png`.  Without UVs and texture: plain `v` / `f` lines, no side files.
    Indices in the file are 1-based."""
    path = os.fspath(f)
    v = torch.as_tensor(verts).detach().cpu()
    fa = torch.as_tensor(faces).detach().cpu()
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"verts must be (V,3), got {tuple(v.shape)}")
    if fa.numel() and (fa.dim() != 2 or fa.shape[1] != 3):
        raise ValueError(f"faces must be (F,3), got {tuple(fa.shape)}")
    fa = fa.reshape(-1, 3).to(torch.int64)
    if fa.numel() and (int(fa.min()) < 0 or int(fa.max()) >= v.shape[0]):
        raise ValueError(f"faces index {v.shape[0]} vertices: found indices in [{int(fa.min())}, {int(fa.max())}]")
    if (verts_uvs is None) != (faces_uvs is None):
        raise ValueError("pass verts_uvs and faces_uvs together")
    has_uv = verts_uvs is not None
    has_tex = texture_map is not None or texture_png is not None
    if has_tex and not has_uv:
        raise ValueError("a texture needs verts_uvs and faces_uvs")
    fmt = "%f" if decimal_places is None else "%%.%df" % int(decimal_places)
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    parts = []
    if has_tex:
        parts.append(f"mtllib {name}.mtl\nusemtl mesh\n")
    parts.append(_rows("v", v.double().numpy(), fmt))
    if has_uv:
        vt = torch.as_tensor(verts_uvs).detach().cpu()
        ft = torch.as_tensor(faces_uvs).detach().cpu().reshape(-1, 3).to(torch.int64)
        if vt.dim() != 2 or vt.shape[1] != 2:
            raise ValueError(f"verts_uvs must be (VT,2), got {tuple(vt.shape)}")
        if ft.shape != fa.shape:
            raise ValueError(f"faces_uvs {tuple(ft.shape)} must match faces {tuple(fa.shape)}")
        if ft.numel() and (int(ft.min()) < 0 or int(ft.max()) >= vt.shape[0]):
            raise ValueError(f"faces_uvs index {vt.shape[0]} uv rows: found indices in [{int(ft.min())}, {int(ft.max())}]")
        parts.append(_rows("vt", vt.double().numpy(), fmt))
        both = torch.stack([fa + 1, ft + 1], 2).reshape(-1, 6).numpy()         # a ta b tb c tc
        if both.shape[0]:
            parts.append(("f %d/%d %d/%d %d/%d\n" * both.shape[0]) % tuple(both.reshape(-1).tolist()))
    else:
        parts.append(_rows("f", (fa + 1).numpy(), "%d"))
    with open(path, "w") as out:
        out.write("".join(parts))
    if has_tex:
        with open(stem + ".mtl", "w") as out:
            out.write(f"newmtl mesh\nmap_Kd {name}.png\n")
        with open(stem + ".png", "wb") as out:
            out.write(texture_png if texture_png is not None else encode_png(texture_map))


FLO_MAGIC = 202021.25                                  # the Middlebury .flo tag, the float32 whose bytes read "PIEH"
FLO_UNKNOWN = 1e9                                      # that format's value for a pixel without flow, in both channels


def save_flo(path, flow, known=None):
    """Optical flow (H,W,2) in pixels as a Middlebury .flo file: float32 FLO_MAGIC, int32 width, int32 height, then (H,W,2) float32 (u, v),
    little endian.  known: None or (H,W) bool; a pixel where it is False is written as FLO_UNKNOWN in both channels."""
    f = np.array(flow, dtype="<f4")
    if f.ndim != 3 or f.shape[2] != 2:
        raise ValueError(f"flow must be (H, W, 2), got {f.shape}")
    if known is not None:
        known = np.asarray(known, bool)
        if known.shape != f.shape[:2]:
            raise ValueError(f"known must be {f.shape[:2]}, got {known.shape}")
        f[~known] = FLO_UNKNOWN
    with open(path, "wb") as fh:
        fh.write(np.array(FLO_MAGIC, "<f4").tobytes() + np.array([f.shape[1], f.shape[0]], "<i4").tobytes() + f.tobytes())


def load_flo(path):
    """A Middlebury .flo file -> (flow (H,W,2) float32 as stored, known (H,W) bool: False where a channel's magnitude is FLO_UNKNOWN or
    more, which is what save_flo writes for a pixel without flow)"""
    with open(path, "rb") as fh:
        raw = fh.read()
    if len(raw) < 12 or np.frombuffer(raw[:4], "<f4")[0] != np.float32(FLO_MAGIC):
        raise ValueError(f"{path} is not a .flo file")
    w, h = (int(v) for v in np.frombuffer(raw[4:12], "<i4"))
    if w < 1 or h < 1 or len(raw) != 12 + 8 * w * h:
        raise ValueError(f"{path}: {len(raw)} bytes for {w} x {h} pixels")
    f = np.frombuffer(raw[12:], "<f4").reshape(h, w, 2).copy()
    return f, ~(np.abs(f) >= np.float32(FLO_UNKNOWN)).any(-1)
