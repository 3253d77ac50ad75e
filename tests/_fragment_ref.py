"""TEST INFRASTRUCTURE ONLY — what tests/test_gpu_fragment_paths.py needs around its reference.  The reference of the fragment rasteriser
(csrc/fragments.hip) is oracle/p3d_like.rasterize_meshes itself, in float64 on the float32-rounded NDC vertices with the blur radius rounded
to float32 (what the C ABI receives); this module only adds what the bounds are made of:

  reference   the oracle's outputs for (case, K, blur), face ids frame-local as the ABI has them; cached in the case, never modified
  pairs       every (frame, face, pixel) pair of a case evaluated densely in float64 (the cases are small): candidates, inside, depth, d2
  undecided   (B,S,S) bool.  A pixel is undecided if for some live face
                a membership test of the pair flips when the pixel centre moves by 2^-20 NDC: the three edge lines (blur = 0),
                |sqrt(d2) - r| (blur > 0, centre outside the face), the edges of the dilated box (pairs that pass the other tests); or
                two consecutive depths among its K + 1 nearest candidates differ by less than 2^-20 relative — unless the two faces have
                identical vertex coordinates: duplicates give bit-equal depths in any arithmetic, the tie rule decides them, they are compared
  e32         |ref32 - ref64|_inf per float output over the filled slots of the decided pixels, ref32 = the same oracle on a float32 ndc
  gradient    d (sum g_zbuf zbuf + g_bary bary + g_dists dists) / d ndc from the oracle's pix_to_face: the kept pairs' face vertices gathered
              as a leaf (P,3,3), P._pair_eval on it, autograd; with N (non-zero shares per element), A (their magnitudes' sum), M (the largest)
              — the quantities of tests/_raster_ref.silhouette_gradient

Anchored on autograd through the oracle by tests/test_fragment_ref_cpu.py."""
import math

import torch

from oracle import p3d_like as P
from tests import _raster_ref as R

F64 = torch.float64
TOL = R.TOL
f32 = R.f32
OUTPUTS = ("zbuf", "bary", "dists")


def reference(c, K, blur, dtype=F64):
    """dict(p2f (B,S,S,K) int64 frame-local, zbuf, bary (B,S,S,K,3), dists) of the oracle; float64 results are cached in the case"""
    key = (int(K), f32(blur), dtype)
    cache = c.setdefault("_refs", {})
    if key not in cache:
        Fn = c["faces"].shape[0]
        with torch.no_grad():
            p2f, z, b, d = P.rasterize_meshes(c["ndc"].float().to(dtype), c["faces"], c["S"], f32(blur), int(K))
        cache[key] = dict(p2f=torch.where(p2f >= 0, p2f % Fn, p2f), zbuf=z, bary=b, dists=d)
    return cache[key]


def _smin(fv, px, py):
    """smallest signed distance to the three edge LINES, positive on the face's side (inside <=> positive)"""
    x0, y0, x1, y1, x2, y2 = fv[:, 0, 0], fv[:, 0, 1], fv[:, 1, 0], fv[:, 1, 1], fv[:, 2, 0], fv[:, 2, 1]
    sg = torch.sign(P._edge_fn(x2, y2, x0, y0, x1, y1) + P.K_EPS)
    tiny = torch.finfo(fv.dtype).tiny
    out = None
    for ax, ay, bx, by in ((x1, y1, x2, y2), (x2, y2, x0, y0), (x0, y0, x1, y1)):
        s = P._edge_fn(px, py, ax, ay, bx, by) * sg / ((bx - ax) ** 2 + (by - ay) ** 2).clamp(min=tiny).sqrt()
        out = s if out is None else torch.minimum(out, s)
    return out


def pairs(c, blur):
    """all (B,F,S,S) pairs in float64: dict(live (B,F), cand, inside, pz, d2, smin, den (the perspective denominator's sum), unstable)"""
    key = ("pairs", f32(blur))
    cache = c.setdefault("_refs", {})
    if key in cache:
        return cache[key]
    blur = f32(blur)
    r = math.sqrt(blur)
    B, S, Fn = c["B"], c["S"], c["faces"].shape[0]
    fv = c["ndc"].float().double()[:, c["faces"]]                          # (B,F,3,3)
    live = ~R.cull(fv)
    pc = P.pixel_centers(S, F64)
    shp = (B, Fn, S, S)
    fvp = fv[:, :, None, None].expand(*shp, 3, 3).reshape(-1, 3, 3)
    px, py = pc[None, None, None, :].expand(shp).reshape(-1), pc[None, None, :, None].expand(shp).reshape(-1)
    _, pz, d2, inside = P._pair_eval(fvp, px, py, True, blur > 0.0)
    z0, z1, z2 = fvp[:, 0, 2], fvp[:, 1, 2], fvp[:, 2, 2]
    w, _, _, _ = P._pair_eval(fvp, px, py, False, False)
    den = w[:, 0] * z1 * z2 + z0 * w[:, 1] * z2 + z0 * z1 * w[:, 2]
    smin = _smin(fvp, px, py)
    box = R._bbox(fv, r)[:, :, None, None].expand(*shp, 4).reshape(-1, 4)
    inbox = ~((px > box[:, 1]) | (px < box[:, 0]) | (py > box[:, 3]) | (py < box[:, 2]))
    lv = live[:, :, None, None].expand(shp).reshape(-1)
    nobox = lv & (pz >= 0) & (inside | (d2 < blur))
    edge = torch.stack([(px - box[:, 0]).abs(), (px - box[:, 1]).abs(), (py - box[:, 2]).abs(), (py - box[:, 3]).abs()], 0).min(0).values
    member = (~inside & ((d2.sqrt() - r).abs() < TOL)) if blur > 0.0 else (smin.abs() < TOL)
    unstable = lv & (member | (nobox & (edge < TOL)))
    v = lambda t: t.view(shp)
    out = dict(live=live, cand=v(nobox & inbox), inside=v(inside), pz=v(pz), d2=v(d2), smin=v(smin), den=v(den), unstable=v(unstable), fv=fv)
    cache[key] = out
    return out


def undecided(c, K, blur):
    """(B,S,S) bool"""
    p = pairs(c, blur)
    B, S, Fn = c["B"], c["S"], c["faces"].shape[0]
    und = p["unstable"].any(1)
    z = torch.where(p["cand"], p["pz"], torch.full_like(p["pz"], float("inf"))).permute(0, 2, 3, 1)          # (B,S,S,F)
    zs, idx = torch.sort(z, dim=-1, stable=True)
    n = min(int(K) + 1, Fn)
    zs, idx = zs[..., :n], idx[..., :n]
    if n > 1:
        fv = p["fv"]
        same = (fv[:, :, None] == fv[:, None, :]).reshape(B, Fn, Fn, 9).all(-1)                             # (B,F,F)
        b = torch.arange(B)[:, None, None, None]
        dup = same[b, idx[..., :-1], idx[..., 1:]]
        close = torch.isfinite(zs[..., 1:]) & ((zs[..., 1:] - zs[..., :-1]) < TOL * zs[..., :-1].abs()) & ~dup
        und = und | close.any(-1)
    return und


def covered(c, blur):
    """(B,S,S) bool: pixels with at least one candidate"""
    return pairs(c, blur)["cand"].any(1)


def e32(c, K, blur, und=None):
    """dict(zbuf, bary, dists: |ref32 - ref64|_inf on the decided pixels' filled slots; same_faces: the float32 oracle picked the same face
    in every slot of every decided pixel)"""
    und = undecided(c, K, blur) if und is None else und
    a, b = reference(c, K, blur), reference(c, K, blur, torch.float32)
    dec = ~und
    same = torch.equal(a["p2f"][dec], b["p2f"][dec])
    m = (dec[..., None] & (a["p2f"] >= 0) & (a["p2f"] == b["p2f"]))
    out = dict(same_faces=same)
    for k in OUTPUTS:
        d = (b[k].double() - a[k]).abs()
        d = d.amax(-1) if k == "bary" else d
        out[k] = d[m].max().item() if m.any() else 0.0
    return out


def gradient(c, p2f, blur, g_zbuf=None, g_bary=None, g_dists=None, dtype=F64, stats=True):
    """p2f (B,S,S,K) frame-local; cotangents (B,S,S,K[,3]) or None, read on the filled slots only.  (B,V,3) gradient, or with stats
    dict(ref, N, A, M)"""
    B, S, V = c["B"], c["S"], c["ndc"].shape[1]
    faces = c["faces"].long()
    K = p2f.shape[-1]
    flat = p2f.reshape(-1)
    slot = torch.nonzero(flat >= 0)[:, 0]
    f, pix = flat[slot], slot // K
    b, rem = pix // (S * S), pix % (S * S)
    ndc = c["ndc"].float().to(dtype)
    leaf = ndc[b[:, None], faces[f]].clone().requires_grad_()                                               # (P,3,3)
    pc = P.pixel_centers(S, dtype)
    bary, pz, d2, inside = P._pair_eval(leaf, pc[rem % S], pc[rem // S], True, f32(blur) > 0.0)
    sd = torch.where(inside, -d2, d2)
    loss = leaf.sum() * 0.0
    if g_zbuf is not None:
        loss = loss + (pz * g_zbuf.reshape(-1)[slot].to(dtype)).sum()
    if g_bary is not None:
        loss = loss + (bary * g_bary.reshape(-1, 3)[slot].to(dtype)).sum()
    if g_dists is not None:
        loss = loss + (sd * g_dists.reshape(-1)[slot].to(dtype)).sum()
    g, = torch.autograd.grad(loss, leaf)
    vid = (b[:, None] * V + faces[f]).reshape(-1)
    ref = torch.zeros(B * V, 3, dtype=dtype).index_add_(0, vid, g.reshape(-1, 3)).view(B, V, 3)
    if not stats:
        return ref
    s = g.abs().reshape(-1, 3)
    A = torch.zeros(B * V, 3, dtype=dtype).index_add_(0, vid, s).view(B, V, 3)
    N = torch.zeros(B * V, dtype=dtype).index_add_(0, vid, (s != 0).any(-1).to(dtype)).view(B, V, 1).expand(B, V, 3)
    return dict(ref=ref, N=N, A=A, M=s.max().item() if s.numel() else 0.0)
