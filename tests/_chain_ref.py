"""Plain float64, differentiable torch reference of the per-frame mesh chain (include/harp_hip.h: harp_mesh_chain): metres, SubdivideMeshes,
vertex normals, displacement, second normals, centroid, light camera and both projections, assembled from the pieces the oracle already
has (oracle/p3d_like.verts_normals / world_to_ndc, oracle/harp_ref.process_info_for_shadow) with a GENERAL camera rotation.  The stages
are exposed one by one so that a test can evaluate each on a kernel's own float32 output of the stage before it."""
import torch

from oracle import harp_ref as H
from oracle import p3d_like as P

FWD_KEYS = ("joints_m", "vs", "n1", "il1", "vd", "n2", "il2", "ndc_c", "centroid", "light_R", "light_T", "ndc_l")


def subdivide(verts_mm, edges0, mm=1e-3):
    """(B,V0,3) millimetres -> (B,V0+E0,3) metres: the vertices, then the midpoint of every base edge (SubdivideMeshes)"""
    v0 = verts_mm * mm
    return torch.cat([v0, v0[:, edges0].mean(2)], 1) if edges0.shape[0] else v0


def normals(verts, faces):
    """unit area-weighted vertex normals n = N / max(|N|, 1e-6) and il = 1 / |N|, 0 where the clamp holds (what the kernels save)"""
    n = P.verts_normals(verts, faces)
    with torch.no_grad():
        fv = verts[:, faces]
        fn = torch.cross(fv[:, :, 2] - fv[:, :, 1], fv[:, :, 0] - fv[:, :, 1], dim=-1)
        N = torch.zeros_like(verts)
        for k in range(3):
            N = N.index_add(1, faces[:, k], fn)
        ln = N.norm(dim=-1)
        il = torch.where(ln > 1e-6, 1.0 / ln.clamp_min(1e-6), torch.zeros_like(ln))
    return n, il


def displace(vs, n1, disp):
    return vs + n1 * disp[None, :, None]


def project(verts, R, T, S, focal):
    """MeshRasterizer.transform with the principal point at the image centre; R (B,3,3) any rotation, applied as verts @ R"""
    return P.world_to_ndc(verts, R, T, focal, (S / 2.0, S / 2.0), S)[1]


def light_camera(centroid, light_pos, S, focal):
    """process_info_for_shadow: the light camera 1.5 m from the centroid towards the light -> light_R (B,3,3), light_T (B,3)"""
    cam = torch.ones_like(centroid)                      # only feeds the camera convention, which this chain takes as an input instead
    light_R, light_T, _, _ = H.process_info_for_shadow(cam, light_pos, centroid, S, focal)
    return light_R, light_T


def chain(verts_mm, joints_mm, cam_R, cam_T, light_pos, disp, edges0, faces, S, focal, mm=1e-3, centroid_value=None):
    """verts_mm (B,V0,3), joints_mm (B,NJ,3), cam_R (B,3,3), cam_T (B,3), light_pos (B,3), disp (V,), edges0 (E0,2) long, faces (F,3) long
    of the subdivided mesh -> dict of every forward output of harp_mesh_chain (FWD_KEYS; light_R as (B,3,3)).
    mm: the millimetre -> metre factor (a test against float32 code passes the float32 value of 1e-3).
    centroid_value (B,3), optional: the light camera is evaluated AT this value while the gradient still flows through the mean of the
    displaced vertices.  The light camera is discontinuous where the light stands on the vertical through the centroid (look_at_rotation's
    replacement branch), so a comparison with a float32 backward there has to use the centroid that backward read."""
    out = {"joints_m": joints_mm * mm}
    out["vs"] = subdivide(verts_mm, edges0, mm)
    out["n1"], out["il1"] = normals(out["vs"], faces)
    out["vd"] = displace(out["vs"], out["n1"], disp)
    out["n2"], out["il2"] = normals(out["vd"], faces)
    out["ndc_c"] = project(out["vd"], cam_R, cam_T, S, focal)
    c = out["vd"].mean(1)
    if centroid_value is not None:
        c = centroid_value + (c - c.detach())
    out["centroid"] = c
    out["light_R"], out["light_T"] = light_camera(c, light_pos, S, focal)
    out["ndc_l"] = project(out["vd"], out["light_R"], out["light_T"], S, focal)
    return out
