"""TEST INFRASTRUCTURE ONLY — the tile rasteriser (csrc/raster.hip, csrc/raster_body.h) restated in plain torch, vectorised over the
(pixel, face) pairs of every face's blur-dilated bounding box, evaluated in chunks.  SURVEY.md Appendix A.2 / A.3 as the FUSED kernel
implements them:

  culling      face_rec: zmax < 0, zmin < kEps, |area| <= kEps, NaN area  ->  the face exists for no pixel
  candidates   pixel centre inside the dilated bbox, and inside the face or closer than sqrt(blur) to one of its edges
  depth        perspective-correct barycentrics (never clipped: only faces that CONTAIN the pixel centre compete for the nearest face)
  nearest      smallest depth, ties to the lower face id
  alpha        1 - prod_f (1 - sigmoid(-d_f / sigma)) over ALL candidate faces of the pixel (the kernel has no K = 50 cap)
  fused L1     mean |alpha - y[fid]| and w * d/d alpha

float64 by default; dtype=torch.float32 evaluates the same code in float32 (E32 of the bounds).  blur and sigma are rounded to float32
first, ndc is float32 data: what the C ABI receives.  Anchored on oracle/p3d_like.py by tests/test_raster_ref_cpu.py."""
import math

import numpy as np
import torch

K_EPS = 1e-8
TILE, SUPER = 16, 64
TOL = 2.0 ** -20          # a pixel is UNDECIDED if a test of it flips within this distance (NDC) / this relative depth difference
CHUNK = 1 << 20


def f32(x):
    return float(np.float32(x))


def pixel_centers(S, dtype):
    """pix_to_ndc: -1 + (2 (S - 1 - i) + 1) / S"""
    i = torch.arange(S, dtype=dtype)
    return -1.0 + (2.0 * (S - 1 - i) + 1.0) / S


def _edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def _seg(px, py, ax, ay, bx, by):
    """squared distance to the segment (a, b); a degenerate edge gives the distance to b"""
    bax, bay = bx - ax, by - ay
    l2 = bax * bax + bay * bay
    deg = l2 <= K_EPS
    t = ((bax * (px - ax) + bay * (py - ay)) / torch.where(deg, torch.ones_like(l2), l2)).clamp(0.0, 1.0)
    qx, qy = ax + t * bax, ay + t * bay
    return torch.where(deg, (px - bx) ** 2 + (py - by) ** 2, (px - qx) ** 2 + (py - qy) ** 2)


def cull(fv):
    """face_rec's rules on (..., 3, 3) face vertices -> bool (fmaxf / fminf skip a NaN operand, so does torch.fmax / fmin)"""
    x, y, z = fv[..., 0], fv[..., 1], fv[..., 2]
    area = _edge(x[..., 0], y[..., 0], x[..., 1], y[..., 1], x[..., 2], y[..., 2])
    zmax = torch.fmax(z[..., 0], torch.fmax(z[..., 1], z[..., 2]))
    zmin = torch.fmin(z[..., 0], torch.fmin(z[..., 1], z[..., 2]))
    return (zmax < 0) | ((area <= K_EPS) & (area >= -K_EPS)) | (zmin < K_EPS) | torch.isnan(area)


def _bbox(fv, r):
    x, y = fv[..., 0], fv[..., 1]
    return torch.stack([x.min(-1).values - r, x.max(-1).values + r, y.min(-1).values - r, y.max(-1).values + r], -1)


def _pair(fv, px, py, blur):
    """everything about (face, pixel centre) pairs: fv (P,3,3), px / py (P,)"""
    x0, y0, z0 = fv[:, 0, 0], fv[:, 0, 1], fv[:, 0, 2]
    x1, y1, z1 = fv[:, 1, 0], fv[:, 1, 1], fv[:, 1, 2]
    x2, y2, z2 = fv[:, 2, 0], fv[:, 2, 1], fv[:, 2, 2]
    area = _edge(x2, y2, x0, y0, x1, y1) + K_EPS
    sg = torch.sign(area)
    e0, e1, e2 = _edge(px, py, x1, y1, x2, y2), _edge(px, py, x2, y2, x0, y0), _edge(px, py, x0, y0, x1, y1)
    inside = (e0 * sg > 0) & (e1 * sg > 0) & (e2 * sg > 0)
    w0, w1, w2 = e0 / area, e1 / area, e2 / area
    t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
    den = (t0 + t1 + t2).clamp(min=K_EPS)
    pz = (t0 / den) * z0 + (t1 / den) * z1 + (t2 / den) * z2
    d2 = torch.minimum(torch.minimum(_seg(px, py, x0, y0, x1, y1), _seg(px, py, x0, y0, x2, y2)), _seg(px, py, x1, y1, x2, y2))
    # signed distance to the three edge LINES (positive on the face's side): inside <=> the smallest is positive
    l12, l20, l01 = (x2 - x1) ** 2 + (y2 - y1) ** 2, (x0 - x2) ** 2 + (y0 - y2) ** 2, (x1 - x0) ** 2 + (y1 - y0) ** 2
    tiny = torch.finfo(fv.dtype).tiny
    s = torch.stack([e0 * sg / l12.clamp(min=tiny).sqrt(), e1 * sg / l20.clamp(min=tiny).sqrt(), e2 * sg / l01.clamp(min=tiny).sqrt()], 0).min(0).values
    return dict(inside=inside, pz=pz, d2=d2, smin=s, sd=torch.where(inside, -d2, d2))


def rasterize(ndc, faces, S, blur=0.0, sigma=1.0, dtype=torch.float64, grad=False):
    """ndc (B,V,3) float32, faces (F,3) -> dict, everything per COVERED pixel (one that has a nearest face or a soft candidate), sorted by
    `pix` = (b S + y) S + x; `dense(ref, key, fill)` spreads an entry over (B,S,S):
      face_id (-1: no face contains the centre), z, alpha (blur > 0; differentiable with grad=True), ncand (soft candidates of the pixel),
      undecided (+ unstable_b / unstable_f: the (frame, face) pairs whose test is the unstable one), and per tile / super-tile (B,nt,nt) / (B,nsx,nsx): tile_count, super_count = live faces whose dilated bbox reaches it
    grad=True keeps the graph: `leaf` (B,V,3) and `fvs` (the candidate pairs' gathered face vertices, (P,3,3), rows `pair_b`, `pair_f`)."""
    B, V, _ = ndc.shape
    F = faces.shape[0]
    faces = faces.long()
    blur, sigma = f32(blur), f32(sigma)
    soft = blur > 0.0
    r = math.sqrt(blur) if dtype == torch.float64 else float(np.sqrt(np.float32(blur)))
    leaf = ndc.detach().float().to(dtype).requires_grad_(grad)
    pc = pixel_centers(S, dtype)
    with torch.no_grad():
        fv = leaf.detach()[:, faces]                                      # (B,F,3,3)
        live = ~cull(fv)
        bb = _bbox(fv, r)                                                 # (B,F,4)
        # ---- per tile / super-tile: live faces whose box reaches its pixel centres (the staging filter / the binning pass)
        counts = {}
        for name, side in (("tile_count", TILE), ("super_count", SUPER)):
            n = (S + side - 1) // side
            hi = pc[torch.arange(n) * side]
            lo = pc[(torch.arange(n) * side + side).clamp(max=S) - 1]
            ox = (~((lo[None, None] > bb[..., 1, None]) | (hi[None, None] < bb[..., 0, None])) & live[..., None]).to(torch.float64)      # (B,F,n)
            oy = (~((lo[None, None] > bb[..., 3, None]) | (hi[None, None] < bb[..., 2, None])) & live[..., None]).to(torch.float64)
            counts[name] = torch.einsum("bfy,bfx->byx", oy, ox).round().long()
        # ---- the pairs: every pixel of every live face's box, with a margin (the exact comparisons follow)
        lf = torch.nonzero(live.reshape(-1))[:, 0]                        # packed b F + f
        q = bb.reshape(-1, 4)[lf].double()

        def rng(lo, hi):
            a = (torch.floor((S * (1.0 - hi) - 1.0) / 2.0) - 1).clamp(0, S - 1).long()
            b = (torch.ceil((S * (1.0 - lo) - 1.0) / 2.0) + 1).clamp(0, S - 1).long()
            return a, b
        ax, bx = rng(q[:, 0], q[:, 1])
        ay, by = rng(q[:, 2], q[:, 3])
        w = (bx - ax + 1).clamp(min=0)
        cnt = w * (by - ay + 1).clamp(min=0)
        row = torch.repeat_interleave(torch.arange(lf.numel()), cnt)
        local = torch.arange(int(cnt.sum())) - (torch.cumsum(cnt, 0) - cnt)[row]
        xi, yi = ax[row] + local % w[row], ay[row] + local // w[row]
        bf = lf[row]
        keep_c, keep_h, pz_all, unst = [], [], [], []
        fvp_all = fv.reshape(-1, 3, 3)
        bbp_all = bb.reshape(-1, 4)
        for s in range(0, bf.numel(), CHUNK):
            sl = slice(s, s + CHUNK)
            px, py, box = pc[xi[sl]], pc[yi[sl]], bbp_all[bf[sl]]
            p = _pair(fvp_all[bf[sl]], px, py, blur)
            inbox = ~((px > box[:, 1]) | (px < box[:, 0]) | (py > box[:, 3]) | (py < box[:, 2]))
            c = inbox & (p["inside"] | (p["d2"] < blur))
            keep_c.append(c)
            keep_h.append(inbox & p["inside"] & (p["pz"] >= 0) & (p["pz"] < 3.0e38))
            pz_all.append(p["pz"])
            edge = torch.stack([(px - box[:, 0]).abs(), (px - box[:, 1]).abs(), (py - box[:, 2]).abs(), (py - box[:, 3]).abs()], 0).min(0).values
            u = (p["smin"].abs() < TOL) | (~p["inside"] & ((p["d2"].sqrt() - r).abs() < TOL) & soft) | (c & (edge < TOL))
            unst.append(u)
        cat = lambda xs, dt: torch.cat(xs) if xs else torch.zeros(0, dtype=dt)
        c, h, pz, u = cat(keep_c, torch.bool), cat(keep_h, torch.bool), cat(pz_all, dtype), cat(unst, torch.bool)
        g = (bf // F) * (S * S) + yi * S + xi                             # global pixel
        fid = bf % F
        # ---- nearest face per pixel among the faces that contain it; near-ties
        gh, fh, zh = g[h], fid[h], pz[h]
        o = torch.from_numpy(np.lexsort((fh.numpy(), zh.numpy(), gh.numpy()))).long()
        gh, fh, zh = gh[o], fh[o], zh[o]
        first = torch.ones_like(gh, dtype=torch.bool)
        first[1:] = gh[1:] != gh[:-1]
        start = torch.cummax(torch.where(first, torch.arange(gh.numel()), torch.zeros_like(gh)), 0).values
        near_pix, near_f, near_z = gh[first], fh[first], zh[first]
        z0 = zh[start]
        nxt = torch.zeros_like(first)
        if gh.numel() > 1:
            same = gh[1:] == gh[:-1]
            dz = zh[1:] - zh[:-1]
            nxt[:-1] = same & (zh[:-1] == z0[:-1]) & (dz > 0) & (dz < TOL * zh[:-1].abs())
        tie_pix = gh[nxt]
        # ---- soft candidates, in (pixel, face id) order
        if soft:
            gc, fc, bc = g[c], fid[c], (bf // F)[c]
            o = torch.from_numpy(np.lexsort((fc.numpy(), gc.numpy()))).long()
            gc, fc, bc = gc[o], fc[o], bc[o]
        else:
            gc = fc = bc = torch.zeros(0, dtype=torch.long)
        pix = torch.unique(torch.cat([near_pix, gc]))                      # sorted
        n = pix.numel()
        at = lambda gg: torch.searchsorted(pix, gg)
        face_id = torch.full((n,), -1, dtype=torch.long)
        face_id[at(near_pix)] = near_f
        z = torch.full((n,), -1.0, dtype=dtype)
        z[at(near_pix)] = near_z
        und = torch.zeros(n, dtype=torch.bool)
        gu = g[u]
        gu = gu[torch.isin(gu, pix)]
        und[at(gu)] = True
        und[at(tie_pix)] = True
        # an unstable pair of a pixel that is not covered at all: it may become covered
        extra = torch.unique(g[u][~torch.isin(g[u], pix)])
        ncand = torch.zeros(n, dtype=torch.long)
        if soft:
            ncand.index_add_(0, at(gc), torch.ones_like(gc))
    out = dict(B=B, S=S, F=F, V=V, blur=blur, sigma=sigma, pix=pix, face_id=face_id, z=z, undecided=und, undecided_uncovered=extra, ncand=ncand,
               pair_b=bc, pair_f=fc, pair_pix=gc, unstable_b=(bf // F)[u], unstable_f=fid[u], leaf=leaf, faces=faces, live=live, **counts)
    if soft:
        # ---- differentiable: the candidates' signed distances -> per pixel product, padded to the largest candidate count
        rem = gc % (S * S)
        fvs = leaf[bc[:, None], faces[fc]]                                        # (P,3,3)
        p = _pair(fvs, pc[rem % S], pc[rem // S], blur)
        slot_pix = at(gc)
        firstc = torch.ones_like(gc, dtype=torch.bool)
        firstc[1:] = gc[1:] != gc[:-1]
        startc = torch.cummax(torch.where(firstc, torch.arange(gc.numel()), torch.zeros_like(gc)), 0).values
        rank = torch.arange(gc.numel()) - startc
        K = int(rank.max()) + 1 if gc.numel() else 1
        slot = slot_pix * K + rank
        sd = torch.zeros(n * K, dtype=dtype).index_put((slot,), p["sd"]).view(n, K)
        mask = torch.zeros(n * K, dtype=dtype).index_put((slot,), torch.ones_like(p["sd"])).view(n, K)
        prob = torch.sigmoid(-sd / sigma) * mask
        alpha = 1.0 - torch.prod(1.0 - prob, dim=-1)
        if not grad:
            alpha, fvs = alpha.detach(), fvs.detach()
        # rim: 0 < alpha < 1 in this dtype; rim_wide: with a margin that survives float32 (1 - 1e-11 is a rim pixel in float64 only)
        ad = alpha.detach()
        out.update(alpha=alpha, fvs=fvs, rim=(ad > 0) & (ad < 1), rim_wide=(ad > 1e-3) & (ad < 1 - 1e-3))
    return out


def dense(ref, key, fill):
    """(B,S,S) image of a per-covered-pixel entry"""
    v = ref[key].detach()
    img = torch.full((ref["B"] * ref["S"] * ref["S"],), fill, dtype=v.dtype)
    img[ref["pix"]] = v
    return img.view(ref["B"], ref["S"], ref["S"])


def undecided_image(ref):
    img = dense(ref, "undecided", False).reshape(-1)
    img[ref["undecided_uncovered"]] = True
    return img.view(ref["B"], ref["S"], ref["S"])


def per_pixel(count, side, S):
    """a per-tile / per-super-tile count spread over the pixels"""
    return count.repeat_interleave(side, 1).repeat_interleave(side, 2)[:, :S, :S]


def tile_pairs(ref):
    """(B,nt,nt): soft (pixel, face) candidate pairs per 16x16 tile"""
    S, B = ref["S"], ref["B"]
    nt = (S + TILE - 1) // TILE
    g = ref["pair_pix"]
    b, rem = g // (S * S), g % (S * S)
    t = (b * nt + (rem // S) // TILE) * nt + (rem % S) // TILE
    return torch.bincount(t, minlength=B * nt * nt).view(B, nt, nt)


def silhouette_gradient(ref, g_alpha, stats=True):
    """(g_alpha: a (B,S,S) image, or one value per covered pixel in the order of ref["pix"])
    d (sum g_alpha * alpha) / d ndc of a grad=True rasterisation: (B,V,3) (z components exactly 0), and — stats — what the bound of an
    atomically summed output needs per element: N contributions (one per candidate pair and vertex with a non-zero share), A the sum of
    their magnitudes, M the largest single one"""
    cot = (g_alpha if g_alpha.numel() == ref["pix"].numel() and g_alpha.dim() == 1 else g_alpha.reshape(-1)[ref["pix"]]).to(ref["alpha"].dtype)
    loss = (ref["alpha"] * cot).sum()
    g_leaf, g_fvs = torch.autograd.grad(loss, [ref["leaf"], ref["fvs"]], retain_graph=True, allow_unused=True)
    g_leaf = torch.zeros_like(ref["leaf"]) if g_leaf is None else g_leaf
    if not stats:
        return g_leaf
    B, V = ref["B"], ref["V"]
    c = torch.zeros_like(ref["fvs"]) if g_fvs is None else g_fvs.abs()     # (P,3,3)
    vid = (ref["pair_b"][:, None] * V + ref["faces"][ref["pair_f"]]).reshape(-1)          # (P*3,)
    A = torch.zeros(B * V, 3, dtype=c.dtype).index_add_(0, vid, c.reshape(-1, 3)).view(B, V, 3)
    N = torch.zeros(B * V, dtype=c.dtype).index_add_(0, vid, (c.reshape(-1, 3) != 0).any(-1).to(c.dtype)).view(B, V, 1).expand(B, V, 3)
    return dict(ref=g_leaf, N=N, A=A, M=c.max().item() if c.numel() else 0.0)


def l1(alpha_img, y, rows, w):
    """fused L1 of the camera view: mean |alpha - y[rows]| (float64), and the float32 image w * (1 / (B S S)) * sign(alpha - y) the kernel
    writes (its factors are float32 numbers: the product is formed as the kernel forms it), plus the per-pixel terms of the mean"""
    B, S, _ = alpha_img.shape
    d = alpha_img.double() - y[rows.long()].double()
    inv = np.float32(1.0) / (np.float32(B) * np.float32(S) * np.float32(S))
    scale = float(np.float32(w) * inv)
    terms = d.abs() * float(inv)
    return terms.sum().item(), (torch.sign(d) * scale).float(), d, terms
