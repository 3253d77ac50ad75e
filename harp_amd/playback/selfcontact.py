"""Which faces of a mesh do not count for which of its own vertices when the mesh is tested for contact with ITSELF: a
vertex lies at distance 0 from the faces that meet at it and within a few millimetres of its neighbourhood, so self-contact needs a
geodesic exclusion.  `geodesic_exclusion` makes the (V, F) mask from a radius, `pack_exclusion` the bit table that harp_mesh_contact_excl
reads (include/harp_hip.h).  Torch on whatever device the inputs live on, no kernel: the table belongs to a topology and a rest shape,
is made once per (player, radius) and is the same for every frame."""
import torch

EXCL_FACES = 128                                       # HARP_CONTACT_EXCL_FACES: the faces one 16-byte word of four uint32 covers
_SWEEP_BYTES = 200 << 20                               # the (rows, E) float64 temporary of a sweep stays under this (< 256 MB at V = 4083)


def directed_edges(faces):
    """faces (F,3) integer -> (src, dst) int64: every edge of every face once in each direction"""
    f = torch.as_tensor(faces).long()
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError(f"faces must be (F, 3), got {tuple(f.shape)}")
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = torch.unique(torch.cat([e, e.flip(1)]), dim=0)
    return e[:, 0].contiguous(), e[:, 1].contiguous()


def geodesic_exclusion(verts, faces, radius):
    """verts (V,3) float, faces (F,3) integer, radius >= 0 (inf allowed) -> (V,F) bool on verts' device: face f is excluded for vertex i
    iff some corner of f lies within `radius` of i in edge-path length, the shortest path along mesh edges with the Euclidean edge
    lengths of `verts`.  The faces that meet at i are always excluded (distance 0), also at radius 0; with radius inf, i's whole
    connected component.  Bellman-Ford from all sources at once in float64: a sweep relaxes every directed edge (scatter_reduce "amin")
    and drops candidates above the radius, until nothing changes — as many sweeps as the longest shortest path within the radius has
    edges.  The source rows are taken in chunks that keep the (rows, E) temporary under 200 MB."""
    v = torch.as_tensor(verts)
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < 1 or not v.is_floating_point():
        raise ValueError(f"verts must be a float (V, 3), got {v.dtype} {tuple(v.shape)}")
    radius = float(radius)
    if not radius >= 0:
        raise ValueError(f"radius must not be negative or NaN, got {radius}")
    V, dev = v.shape[0], v.device
    f = torch.as_tensor(faces).long().to(dev)
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] < 1 or int(f.min()) < 0 or int(f.max()) >= V:
        raise ValueError(f"faces must be (F, 3) indices in [0, {V}), got {tuple(f.shape)}")
    v = v.detach().double()
    src, dst = directed_edges(f)
    length = (v[src] - v[dst]).norm(dim=1)
    rows = max(1, _SWEEP_BYTES // (8 * src.shape[0]))
    inf = float("inf")
    out = torch.empty(V, f.shape[0], dtype=torch.bool, device=dev)
    for lo in range(0, V, rows):
        n = min(rows, V - lo)
        d = torch.full((n, V), inf, dtype=torch.float64, device=dev)
        d[torch.arange(n, device=dev), torch.arange(lo, lo + n, device=dev)] = 0.0
        idx = dst.expand(n, -1)
        while True:
            cand = d[:, src] + length
            cand.masked_fill_(cand > radius, inf)
            new = d.scatter_reduce(1, idx, cand, "amin", include_self=True)
            if torch.equal(new, d):
                break
            d = new
        out[lo:lo + n] = torch.isfinite(d)[:, f].any(-1)       # (what is kept is within the radius: the rest was dropped)
    return out


def pack_exclusion(mask):
    """(V,F) bool -> (ceil(F / 128), V, 4) int32, contiguous, on mask's device: bit k & 31 of [c, i, k >> 5] is mask[i, 128 c + k]; the
    bits past F are 0.  int32 holds the 32 bits as they are (bit 31 is the sign)."""
    m = torch.as_tensor(mask)
    if m.dtype != torch.bool or m.dim() != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"mask must be a bool (V, F), got {m.dtype} {tuple(m.shape)}")
    V, F = m.shape
    C = -(-F // EXCL_FACES)
    bits = torch.zeros(V, C * EXCL_FACES, dtype=torch.int64, device=m.device)
    bits[:, :F] = m
    word = (bits.view(V, C, 4, 32) << torch.arange(32, dtype=torch.int64, device=m.device)).sum(-1)      # 0 .. 2^32 - 1
    word = torch.where(word >= 1 << 31, word - (1 << 32), word).to(torch.int32)
    return word.permute(1, 0, 2).contiguous()


def unpack_exclusion(table, F):
    """pack_exclusion's table and the number of faces -> the (V,F) bool mask"""
    t = torch.as_tensor(table)
    if t.dtype not in (torch.int32, torch.uint32) or t.dim() != 3 or t.shape[2] != 4 or not 0 < int(F) <= t.shape[0] * EXCL_FACES:
        raise ValueError(f"table must be int32 or uint32 (chunks, V, 4) with room for {F} faces, got {t.dtype} {tuple(t.shape)}")
    C, V = t.shape[0], t.shape[1]
    w = t.view(torch.int32).long().permute(1, 0, 2)                                                         # (V, C, 4)
    bits = (w[..., None] >> torch.arange(32, dtype=torch.int64, device=t.device)) & 1
    return bits.reshape(V, C * EXCL_FACES)[:, :int(F)].bool()
