"""The tile rasteriser's paths (csrc/raster.hip, csrc/raster_body.h) against float64 on synthetic meshes, through the raw C ABI.  The hand and
bench scenes the rest of the suite rasterises never reach: the second trip of expand_bits_body (F > 8 192) and of order_tiles
(B nst > 8 192), several staging rounds of a tile (> 256 faces; > 128 in the backward), culled faces, exact depth ties, a frame without a
face (nact % 8 != 0 under the striding grid's background table), a super-tile that empties between two harp_rasterize_fwd_keep calls, and —
at small S with the workload's sigma — hardly any soft pixel.  tests/_raster_cases.py builds a mesh per path and asserts on the reference
that the path is reached; tests/_raster_ref.py is the reference (anchored on the oracle by tests/test_raster_ref_cpu.py).

Bounds, per element, none of them measured on the kernel:
  face ids   equal on the DECIDED pixels (undecided: two nearest depths within 2^-20 relative, or an inside / band / box test that flips when
             the centre moves by 2^-20 NDC; at most 2 % of a case's covered pixels, asserted on the reference)
  z, alpha   |got - ref64| <= 4 E32 + 2^-22 |ref64| on the decided pixels, E32 = |ref32 - ref64|_inf of the restatement in float32 (4 x: the
             kernel's approximate reciprocals and exponential); exactly -1 / 0 where the reference has no face / no candidate.  (An undecided
             pixel may hold another face, so its depth and coverage are not compared; its cotangent is zero.)
  g_ndc, loss (float atomics)   N_i M 2^-24 + 4 E32_g + 2^-22 A_i, from the reference's per-pair shares (N_i of them on element i, the largest M,
             their magnitudes' sum A_i); z components exactly 0
  records / fused backward against the staged walk: relative L2 difference < 1e-5 (tests/test_gpu_sil_records.py)
Measured err / bound per case and output: docs/NOTEBOOK.md."""
import pytest
import torch

from tests import _raster_cases as C
from tests import _raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = 1
SENT_F, SENT_Z, SENT_A, SENT_G = -7, 7.0, 0.5, 0.25


def _api():
    from harp_amd import _lib
    return _lib.lib(), _lib.ptr, _lib.stream


# ----------------------------------------------------------------------------------------------------------------------
# reference side (once per case, shared, never modified)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    built = {}
    yield built
    built.clear()


def get_case(cases, name, grad=True):
    if name in cases:
        return cases[name]
    c = C.build(name)
    hard, soft = C.references(c, grad=grad)
    c["info"] = C.conditions(c, hard, soft)
    h32 = R.rasterize(c["ndc"], c["faces"], c["S"], dtype=torch.float32)
    s32 = R.rasterize(c["ndc"], c["faces"], c["S"], c["blur"], c["sigma"], dtype=torch.float32, grad=grad)
    B, S = c["B"], c["S"]
    c.update(hard=hard, soft=soft, h32=h32, s32=s32, d_ndc=c["ndc"].to(DEV), d_faces=c["faces"].int().to(DEV).contiguous(),
             V=c["ndc"].shape[1], F=c["faces"].shape[0])
    if B * S * S <= (1 << 22):
        und = R.undecided_image(hard) | R.undecided_image(soft)
        c["und"] = und
        zv = c["ndc"][:, c["faces"]][..., 2].double().reshape(B, -1)                       # depth range of each frame's live faces
        lv = hard["live"][..., None].expand(-1, -1, 3).reshape(B, -1)
        c["zrange"] = (zv.masked_fill(~lv, float("inf")).amin(1), zv.masked_fill(~lv, float("-inf")).amax(1))
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        c["y"] = torch.rand(4, S, S, generator=g) * 0.9 + 0.05
        c["y"][0, : S // 3] = 0.0                          # ... with stretches of exact 0 and 1, as a silhouette mask has
        c["y"][1, S // 2:] = 1.0
        c["rows"] = (torch.arange(B, dtype=torch.int32) * 3 + 1) % 4
        c["cot"] = ((torch.rand(B, S, S, generator=g) * 0.8 + 0.2) * torch.where(torch.rand(B, S, S, generator=g) < 0.3, -1.0, 1.0) * (~und)).float()
    cases[name] = c
    return c


def e32_of(c, kind, key, fill):
    """|ref32 - ref64|_inf of a per-pixel output on the decided pixels"""
    a, b = R.dense(c[kind], key, fill), R.dense(c["h32" if kind == "hard" else "s32"], key, fill)
    return (a - b.double())[~c["und"]].abs().max().item()


def check_pixels(c, tag, face_id=None, z=None, alpha=None, where=None, soft_ids=False):
    """face ids / depth / alpha of a forward call against the reference on `where` (default: everywhere); returns err / bound"""
    dec = ~c["und"]
    sel = dec if where is None else dec & where
    hard = c["hard"]
    out = {}
    rf = R.dense(hard, "face_id", -1)
    if face_id is not None:
        got = face_id.cpu().long()
        assert torch.equal(got[sel], rf[sel]), (c["name"], tag, int((got[sel] != rf[sel]).sum()))
    if z is not None:
        got, rz = z.cpu().double(), R.dense(hard, "z", -1.0)
        assert (got[sel & (rf < 0)] == -1.0).all(), (c["name"], tag)
        m = sel & (rf >= 0)
        lim = 4.0 * e32_of(c, "hard", "z", -1.0) + 2.0 ** -22 * rz.abs()
        out["z"] = ((got - rz).abs() / lim)[m].max().item()
    if alpha is not None:
        got, ra = alpha.cpu().double(), R.dense(c["soft"], "alpha", 0.0)
        nc = R.dense(c["soft"], "ncand", 0)
        assert (got[sel & (nc == 0)] == 0.0).all(), (c["name"], tag)
        lim = 4.0 * e32_of(c, "soft", "alpha", 0.0) + 2.0 ** -22 * ra.abs()
        m = sel & (nc > 0)
        out["alpha"] = ((got - ra).abs() / lim)[m].max().item() if m.any() else 0.0
    # the undecided pixels: which face they hold is open, that they hold a possible value is not
    u = c["und"] if where is None else c["und"] & where
    if u.any():
        zlo, zhi = (v[:, None, None].expand_as(rf) for v in c["zrange"])
        if face_id is not None:
            got = face_id.cpu().long()[u]
            assert ((got >= -1) & (got < c["F"])).all(), (c["name"], tag)
        if z is not None:
            got = z.cpu().double()
            assert ((got == -1.0) | ((got >= zlo * (1 - 1e-6)) & (got <= zhi * (1 + 1e-6))))[u].all(), (c["name"], tag)
        if alpha is not None:
            got = alpha.cpu()[u]
            assert ((got >= 0.0) & (got <= 1.0)).all(), (c["name"], tag)
    print(f"[{c['name']} {tag}] err / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in out.items()))
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, (c["name"], tag, bad)
    return out


def gradient_reference(c, cot):
    """float64 gradient of sum(cot * alpha) with its bound terms, and E32_g"""
    st = R.silhouette_gradient(c["soft"], cot.double())
    g32 = R.silhouette_gradient(c["s32"], cot.float(), stats=False)
    st["e32"] = (g32.double() - st["ref"]).abs().max().item()
    return st


def undecided_vertices(c):
    """(B,V) bool: vertices of a face that is a candidate of an undecided pixel, or whose own test on a pixel is the unstable one"""
    soft, V = c["soft"], c["V"]
    und = c["und"].reshape(-1)
    out = torch.zeros(c["B"] * V, dtype=torch.bool)
    hit = und[soft["pair_pix"]]
    for b, f in ((soft["pair_b"][hit], soft["pair_f"][hit]), (soft["unstable_b"], soft["unstable_f"])):
        out[(b[:, None] * V + soft["faces"][f]).reshape(-1)] = True
    return out.view(c["B"], V)


def check_gradient(c, tag, g_ndc, st, skip=None):
    """skip (B,V) bool: vertices left out of the comparison with the reference (still: z exactly 0, finite)"""
    got = g_ndc.cpu().double()
    assert st["ref"].abs().max() > 0 and (got[..., 2] == 0).all() and torch.isfinite(got).all(), (c["name"], tag)
    err = (got - st["ref"]).abs()
    if skip is not None:
        err = err.masked_fill(skip[..., None], 0.0)
    bound = st["N"] * st["M"] * 2.0 ** -24 + 4.0 * st["e32"] + 2.0 ** -22 * st["A"]
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max().item()
    print(f"[{c['name']} {tag}] g_ndc err / bound {ratio:.3f} (max |g| {st['ref'].abs().max().item():.3e}, E32 {st['e32']:.2e}, largest N {int(st['N'].max())})")
    assert ratio <= 1.0, (c["name"], tag, ratio)
    return ratio


def check_loss(c, tag, loss, alpha_ref=None, w=1.0):
    """the fused L1's loss against mean |alpha64 - y| : per-pixel terms summed with float atomics"""
    a64 = R.dense(c["soft"], "alpha", 0.0) if alpha_ref is None else alpha_ref
    want, _, _, terms = R.l1(a64, c["y"], c["rows"], w)
    a32 = R.dense(c["s32"], "alpha", 0.0)
    e32 = abs(R.l1(a32, c["y"], c["rows"], w)[0] - want)
    bound = float((terms != 0).sum()) * terms.max().item() * 2.0 ** -24 + 4.0 * e32 + 2.0 ** -22 * want
    ratio = abs(loss.item() - want) / bound
    print(f"[{c['name']} {tag}] loss err / bound {ratio:.3f} (loss {want:.6f})")
    assert ratio <= 1.0, (c["name"], tag, loss.item(), want, bound)
    return ratio


def check_l1_grad(c, tag, l1_grad, w, where=None):
    """sign image: exact wherever |alpha64 - y| exceeds alpha's own bound"""
    a64 = R.dense(c["soft"], "alpha", 0.0)
    _, want, d, _ = R.l1(a64, c["y"], c["rows"], w)
    lim = 4.0 * e32_of(c, "soft", "alpha", 0.0) + 2.0 ** -22 * a64.abs()
    sel = ~c["und"] & (d.abs() > lim)
    if where is not None:
        sel &= where
    got = l1_grad.cpu()
    assert torch.equal(got[sel], want[sel]), (c["name"], tag, int((got[sel] != want[sel]).sum()))
    rest = ~sel if where is None else ~sel & where
    assert (got[rest].abs() <= want.abs().max()).all()


# ----------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------
def workspace(c):
    from harp_amd import ops
    return ops.rasterize_workspace(c["B"], c["F"], c["S"], DEV)


def outputs(c):
    B, S = c["B"], c["S"]
    return (torch.full((B, S, S), SENT_F, dtype=torch.int32, device=DEV), torch.full((B, S, S), SENT_Z, device=DEV), torch.full((B, S, S), SENT_A, device=DEV))


def fwd(c, soft, ws=None, face_ids=True, want_z=True):
    L, p, st = _api()
    ws = workspace(c) if ws is None else ws
    fid, z, a = outputs(c)
    rc = L.harp_rasterize_fwd(p(c["d_ndc"]), p(c["d_faces"]), c["B"], c["V"], c["F"], c["S"], soft, c["blur"] if soft & 1 else 0.0, c["sigma"] if soft & 1 else 1.0,
                              p(ws), p(fid) if face_ids else None, p(z) if want_z else None, p(a) if soft & 1 else None, st())
    assert rc == 0
    torch.cuda.synchronize()
    return fid, z, a, ws


def l1_fwd(c, soft=1, ws=None, face_ids=True, bg=None, w=7.0, g_ndc=None):
    """harp_rasterize_l1_fwd, or (g_ndc given) harp_rasterize_l1_fwd_bwd"""
    L, p, st = _api()
    ws = workspace(c) if ws is None else ws
    fid, z, a = outputs(c)
    g = torch.full_like(a, SENT_G)
    loss = torch.zeros(1, device=DEV)
    y, rows, wt = c["y"].to(DEV), c["rows"].to(DEV), torch.tensor([w], device=DEV)
    head = (p(c["d_ndc"]), p(c["d_faces"]), c["B"], c["V"], c["F"], c["S"], soft, c["blur"], c["sigma"], p(ws), p(fid) if face_ids else None)
    if g_ndc is None:
        rc = L.harp_rasterize_l1_fwd(*head, p(z) if face_ids else None, p(a), p(y), p(rows), p(wt), p(loss), p(g), p(bg) if bg is not None else None, st())
    else:
        rc = L.harp_rasterize_l1_fwd_bwd(*head, p(a), p(y), p(rows), p(wt), p(loss), p(g), p(bg) if bg is not None else None, p(g_ndc), st())
    assert rc == 0
    torch.cuda.synchronize()
    return dict(face_id=fid, z=z, alpha=a, l1_grad=g, loss=loss, ws=ws)


def sil_bwd(c, ws, alpha, g_alpha):
    L, p, st = _api()
    g_ndc = torch.zeros(c["B"], c["V"], 3, device=DEV)
    rc = L.harp_silhouette_bwd(p(c["d_faces"]), c["B"], c["V"], c["F"], c["S"], c["blur"], c["sigma"], p(ws), p(alpha), p(g_alpha), p(g_ndc), st())
    assert rc == 0
    torch.cuda.synchronize()
    return g_ndc


def occupied(c, kind="soft"):
    """(B,S,S) bool: pixels of the super-tiles that hold a face"""
    return R.per_pixel(c[kind]["super_count"] > 0, R.SUPER, c["S"])


def bg_table(c):
    """l1_bg_sums: per target frame and super-tile the sum of |0 - y|, in float64"""
    S = c["S"]
    nsx = (S + R.SUPER - 1) // R.SUPER
    pad = torch.zeros(4, nsx * R.SUPER, nsx * R.SUPER, dtype=torch.float64)
    pad[:, :S, :S] = c["y"].double().abs()
    return pad.view(4, nsx, R.SUPER, nsx, R.SUPER).sum((2, 4)).reshape(4, nsx * nsx).float().contiguous().to(DEV)


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


SMALL = ("one_face", "fan", "many_faces", "layers", "culled", "empty_frame", "one_face_w", "fan_w")
LOOPED = ("fan", "empty_frame", "one_face")
FWD = [(n, 0) for n in SMALL] + [(n, 8) for n in LOOPED]


def set_loop(monkeypatch, loop):
    if loop:
        monkeypatch.setenv("HARP_RASTER_LOOP", str(loop))
    else:
        monkeypatch.delenv("HARP_RASTER_LOOP", raising=False)


@pytest.mark.parametrize("name,loop", FWD)
def test_forward_hard_and_soft(name, loop, cases, monkeypatch):
    """harp_rasterize_fwd: K = 1 pass (face ids, depth) and soft pass (face ids, depth, alpha); every pixel is written"""
    set_loop(monkeypatch, loop)
    c = get_case(cases, name)
    fid, z, _, ws = fwd(c, 0)
    check_pixels(c, f"hard loop={loop}", fid, z)
    assert int((fid == SENT_F).sum()) == 0 and int((z == SENT_Z).sum()) == 0
    if name == "empty_frame":
        from harp_amd import ops
        assert ops.rasterize_ws_nact(ws, c["B"], c["F"], c["S"]) == c["info"]["nact"]
    fid, z, a, _ = fwd(c, 1)
    check_pixels(c, f"soft loop={loop}", fid, z, a)
    assert int((fid == SENT_F).sum()) == 0 and int((a == SENT_A).sum()) == 0
    _, _, a2, _ = fwd(c, 1, face_ids=False, want_z=False)
    assert torch.equal(a2, a)
    # sparse outputs: untouched where a super-tile holds no face, the depth map complete
    fid, z, a, _ = fwd(c, 3)
    occ = occupied(c)
    check_pixels(c, f"soft sparse loop={loop}", fid, z, a, where=occ)
    assert (fid.cpu()[~occ] == SENT_F).all() and (a.cpu()[~occ] == SENT_A).all() and (z.cpu()[~occ] == -1.0).all()


@pytest.mark.parametrize("name,loop", FWD)
def test_fused_l1_forward(name, loop, cases, monkeypatch):
    """harp_rasterize_l1_fwd: loss and l1_grad with a target; without face ids; sparse with the background table built in float64"""
    set_loop(monkeypatch, loop)
    c = get_case(cases, name)
    w = 7.0
    r = l1_fwd(c, w=w)
    check_pixels(c, f"l1 loop={loop}", r["face_id"], r["z"], r["alpha"])
    check_loss(c, f"l1 loop={loop}", r["loss"])
    check_l1_grad(c, "l1", r["l1_grad"], w)
    r2 = l1_fwd(c, w=w, face_ids=False)
    assert torch.equal(r2["alpha"], r["alpha"]) and torch.equal(r2["l1_grad"], r["l1_grad"])
    check_loss(c, f"l1 no ids loop={loop}", r2["loss"])
    occ = occupied(c)
    r3 = l1_fwd(c, soft=3, w=w, bg=bg_table(c))
    check_pixels(c, f"l1 sparse+table loop={loop}", r3["face_id"], r3["z"], r3["alpha"], where=occ)
    check_loss(c, f"l1 sparse+table loop={loop}", r3["loss"])
    check_l1_grad(c, "l1 sparse", r3["l1_grad"], w, where=occ)
    assert (r3["l1_grad"].cpu()[~occ] == SENT_G).all() and (r3["alpha"].cpu()[~occ] == SENT_A).all()
    r4 = l1_fwd(c, soft=3, w=w)                                       # sparse without a table: the background's terms are summed from the target
    check_loss(c, f"l1 sparse loop={loop}", r4["loss"])


@pytest.mark.parametrize("name", ["layers", "empty_frame", "many_faces"])
def test_setup_pair_gives_the_single_setups_outputs(name, cases):
    """harp_raster_setup_pair with two different blur radii, then calls with bit 2 set: bit for bit what the calls give that set up themselves"""
    L, p, st = _api()
    c = get_case(cases, name)
    ws_a, ws_b = workspace(c), workspace(c)
    other = c["d_ndc"].flip(0).contiguous() if c["B"] > 1 else (c["d_ndc"] * torch.tensor([0.9, 0.9, 1.0], device=DEV)).contiguous()
    assert L.harp_raster_setup_pair(p(c["d_ndc"]), c["blur"], p(ws_a), p(other), 0.0, p(ws_b), p(c["d_faces"]), c["B"], c["V"], c["F"], c["S"], st()) == 0
    w = 3.0
    a = l1_fwd(c, soft=1 | 4, ws=ws_a, w=w)
    ref = l1_fwd(c, soft=1, w=w)
    for k in ("face_id", "z", "alpha", "l1_grad"):
        assert torch.equal(a[k], ref[k]), k
    assert abs(a["loss"].item() - ref["loss"].item()) <= 1e-6 * ref["loss"].item()
    c2 = dict(c, d_ndc=other)
    fid, z, _, _ = fwd(c2, 4, ws=ws_b)
    fid0, z0, _, _ = fwd(c2, 0)
    assert torch.equal(fid, fid0) and torch.equal(z, z0)
    # and the backward on the pair's workspace
    g = sil_bwd(c, ws_a, a["alpha"], a["l1_grad"])
    g0 = sil_bwd(c, ref["ws"], ref["alpha"], ref["l1_grad"])
    assert g0.abs().max().item() > 0 and rel(g, g0) < 1e-5


BWD = [(n, 0) for n in SMALL] + [(n, 8) for n in LOOPED]


@pytest.mark.parametrize("name,loop", BWD)
def test_silhouette_backward_in_all_forms(name, loop, cases, monkeypatch):
    """staged walk, records (capacity 0, one below the fullest tile's count, ample) and the fused forward + backward: every element of g_ndc"""
    L, p, st = _api()
    set_loop(monkeypatch, loop)
    c = get_case(cases, name)
    B, S, F = c["B"], c["S"], c["F"]
    cot = c["cot"].to(DEV)
    ref = gradient_reference(c, c["cot"])
    ws = workspace(c)
    _, _, alpha, _ = fwd(c, 1, ws=ws)
    g_staged = sil_bwd(c, ws, alpha, cot)
    check_gradient(c, f"staged loop={loop}", g_staged, ref)
    ample = int(R.tile_pairs(c["soft"]).max()) + 64
    fullest = None
    for cap in (ample, "below", 0):
        if cap == "below":
            cap = max(fullest - 1, 0)
        rec = torch.full((L.harp_sil_records_bytes(B, S, cap),), 0xFF, dtype=torch.uint8, device=DEV)
        assert L.harp_sil_records_bind(p(ws), p(rec), cap, B, F, S) == 0
        try:
            fid, z, a, _ = fwd(c, 1, ws=ws)
            assert torch.equal(a, alpha)                                   # the forward's outputs do not depend on the records
            g_rec = sil_bwd(c, ws, a, cot)
        finally:
            assert L.harp_sil_records_bind(p(ws), None, 0, B, F, S) == 0
        counts = rec[:L.harp_sil_records_bytes(B, S, 0)].view(torch.int32)      # (capacity 0: the count area alone)
        if fullest is None:
            fullest = int(counts.max().item())
            assert 0 < fullest <= ample                                    # no more pairs recorded than the reference has candidates (+ 64 for undecided ones)
        else:
            assert int(counts.max().item()) == fullest > cap               # the fullest tile takes the staged walk
        check_gradient(c, f"records cap={cap} loop={loop}", g_rec, ref)
        assert rel(g_rec, g_staged) < 1e-5
    # fused: the cotangent is the fused L1's own gradient image (checked in test_fused_l1_forward); the reference differentiates with it
    g_fused = torch.zeros(B, c["V"], 3, device=DEV)
    r = l1_fwd(c, w=5.0, g_ndc=g_fused)
    check_pixels(c, f"fused loop={loop}", r["face_id"], None, r["alpha"])
    check_loss(c, f"fused loop={loop}", r["loss"])
    check_l1_grad(c, "fused", r["l1_grad"], 5.0)
    # ... which leaves the undecided pixels their cotangent (the target cannot zero it without being built from the output): the vertices of
    # every face that is a candidate of such a pixel are compared with the two-launch form below only, not with the reference
    ref_f = gradient_reference(c, r["l1_grad"].cpu())
    skip = undecided_vertices(c)
    print(f"[{name} fused] {int(skip.sum())} of {skip.numel()} vertices touched by an undecided pixel")
    assert skip.sum() <= 0.1 * skip.numel()
    check_gradient(c, f"fused loop={loop}", g_fused, ref_f, skip=skip)
    g_two = sil_bwd(c, ws, r["alpha"], r["l1_grad"])
    assert rel(g_fused, g_two) < 1e-5


def test_culled_faces_leave_no_trace(cases):
    """the visible faces alone (the sheet and the face crossing the border) give bit for bit what they give among the culled faces"""
    c = get_case(cases, "culled")
    keep = torch.tensor(c["alone"])
    alone = dict(c, d_faces=c["d_faces"][keep.to(DEV)].contiguous(), F=int(keep.numel()))
    remap = torch.full((c["F"] + 1,), -1, dtype=torch.int32)
    remap[keep] = torch.arange(keep.numel(), dtype=torch.int32)
    for soft in (0, 1):
        fid, z, a, _ = fwd(c, soft)
        fid1, z1, a1, _ = fwd(alone, soft)
        assert torch.equal(remap[fid.cpu().long()], fid1.cpu()) and torch.equal(z, z1) and (soft == 0 or torch.equal(a, a1))
        assert int((fid1 >= 0).sum()) > 0


def test_moves_on_a_kept_depth_map(cases):
    """harp_rasterize_fwd_keep, sparse 0 and 1: the mesh leaves one super-tile for another between two calls on one workspace, one kept depth
    map and one st_state; after each call the WHOLE map is the reference's and st_state is 1 exactly on the empty super-tiles"""
    L, p, st = _api()
    a, b = get_case(cases, "moves_a"), get_case(cases, "moves_b")
    B, S, V, F = a["B"], a["S"], a["V"], a["F"]
    nst = ((S + R.SUPER - 1) // R.SUPER) ** 2
    for sparse in (0, 1):
        ws = workspace(a)
        z = torch.full((B, S, S), SENT_Z, device=DEV)
        state = torch.zeros(B * nst, dtype=torch.int32, device=DEV)
        for step, c in enumerate((a, b, b, a)):
            fid = torch.full((B, S, S), SENT_F, dtype=torch.int32, device=DEV)
            assert L.harp_rasterize_fwd_keep(p(c["d_ndc"]), p(c["d_faces"]), B, V, F, S, sparse, p(ws), p(fid), p(z), p(state), st()) == 0
            torch.cuda.synchronize()
            occ = occupied(c, "hard")
            assert int((z == SENT_Z).sum()) == 0
            check_pixels(c, f"keep sparse={sparse} call {step}", fid, z, where=None if not sparse else occ)
            if sparse:
                assert (fid.cpu()[~occ] == SENT_F).all() and (z.cpu()[~occ] == -1.0).all()
            assert torch.equal(state.cpu().view(B, -1) == 1, c["hard"]["super_count"].reshape(B, -1) == 0)
            assert bool(((state == 0) | (state == 1)).all())


def test_order_tiles_second_trip(cases):
    """B nst = 8 320 launch-order entries: one small quad per frame, each in its own super-tile; the reference lives on the quads' windows"""
    from harp_amd import ops
    c = get_case(cases, "order")
    B, S = c["B"], c["S"]
    n = B * S * S

    def at(ref, key, fill, pix):
        img = torch.full((n,), fill, dtype=torch.float64)
        img[ref["pix"]] = ref[key].detach().double()
        return img[pix]

    def image_of(ref):
        m = torch.zeros(n, dtype=torch.bool, device=DEV)
        m[ref["pix"].to(DEV)] = True
        m[ref["undecided_uncovered"].to(DEV)] = True
        return m
    hard, sref = c["hard"], c["soft"]
    for soft in (0, 1):
        fid, z, a, ws = fwd(c, soft)
        assert ops.rasterize_ws_nact(ws, B, c["F"], S) == c["info"]["nact"] == B
        hp, ok = hard["pix"], ~hard["undecided"]
        assert torch.equal(fid.view(-1)[hp.to(DEV)].cpu().long()[ok], hard["face_id"][ok])
        outside = ~image_of(hard)
        assert bool((fid.view(-1)[outside] == -1).all()) and bool((z.view(-1)[outside] == -1.0).all())
        near = ok & (hard["face_id"] >= 0)
        e32 = (at(c["h32"], "z", -1.0, hp) - hard["z"])[near].abs().max().item()
        ratio = ((z.view(-1)[hp.to(DEV)].cpu().double() - hard["z"]).abs() / (4.0 * e32 + 2.0 ** -22 * hard["z"].abs()))[near].max().item()
        print(f"[order soft={soft}] z err / bound {ratio:.3f}")
        assert ratio <= 1.0
        if soft:
            assert bool((a.view(-1)[~image_of(sref)] == 0.0).all())
            sp, ok = sref["pix"], ~sref["undecided"]
            ra = sref["alpha"]
            e32 = (at(c["s32"], "alpha", 0.0, sp) - ra)[ok].abs().max().item()
            ratio = ((a.view(-1)[sp.to(DEV)].cpu().double() - ra).abs() / (4.0 * e32 + 2.0 ** -22 * ra.abs()))[ok].max().item()
            print(f"[order soft=1] alpha err / bound {ratio:.3f}")
            assert ratio <= 1.0
            # the silhouette backward reads the same order / nact tables: one staged walk, the cotangent (zero on the undecided pixels) built
            # per covered pixel and spread on the device, only g_ndc copied back
            g = torch.Generator().manual_seed(11)
            cs = ((torch.rand(sp.numel(), generator=g) * 0.8 + 0.2) * torch.where(torch.rand(sp.numel(), generator=g) < 0.3, -1.0, 1.0) * ok).float()
            cot = torch.zeros(n, device=DEV)
            cot[sp.to(DEV)] = cs.to(DEV)
            g_ndc = sil_bwd(c, ws, a, cot.view(B, S, S))
            stt = R.silhouette_gradient(sref, cs.double())
            s32 = c["s32"]
            in64 = torch.isin(s32["pix"], sp)
            c32 = torch.zeros(s32["pix"].numel())
            c32[in64] = cs[torch.searchsorted(sp, s32["pix"][in64])]
            stt["e32"] = (R.silhouette_gradient(s32, c32, stats=False).double() - stt["ref"]).abs().max().item()
            check_gradient(c, "staged", g_ndc, stt)


def test_argument_checks_refuse_without_a_launch(cases):
    """the HARP_ERR_ARG exits of the rasteriser's entry points that tests/test_abi.py does not reach, with real buffers: no output is touched"""
    L, p, st = _api()
    c = get_case(cases, "one_face")
    B, V, F, S = c["B"], c["V"], c["F"], c["S"]
    ws = workspace(c)
    fid, z, a = outputs(c)
    g = torch.full_like(a, SENT_G)
    loss = torch.zeros(1, device=DEV)
    g_ndc = torch.zeros(B, V, 3, device=DEV)
    y, rows, wt = c["y"].to(DEV), c["rows"].to(DEV), torch.tensor([1.0], device=DEV)
    n, f = p(c["d_ndc"]), p(c["d_faces"])
    bl, sg = c["blur"], c["sigma"]
    E = ERR_ARG
    assert L.harp_rasterize_fwd(n, f, B, V, F, S, 0, 0.0, 1.0, p(ws), None, p(z), None, st()) == E            # K = 1 pass without face ids
    assert L.harp_rasterize_fwd(n, f, B, V, F, S, 1, bl, sg, p(ws), None, p(z), p(a), st()) == E               # silhouette only, but a depth map
    assert L.harp_rasterize_fwd(n, f, B, V, F, S, 1, bl, sg, p(ws), p(fid), p(z), None, st()) == E             # soft without alpha
    assert L.harp_rasterize_fwd(n, f, B, V, F, S, 1, bl, sg, None, p(fid), p(z), p(a), st()) == E
    for b_, f_, s_ in ((0, F, S), (-1, F, S), (B, 0, S), (B, F, 0), (B, F, -1)):
        assert L.harp_rasterize_fwd(n, f, b_, V, f_, s_, 1, bl, sg, p(ws), p(fid), p(z), p(a), st()) == E
    full = [n, f, B, V, F, S, 1, bl, sg, p(ws), p(fid), p(z), p(a), p(y), p(rows), p(wt), p(loss), p(g), None, st()]
    for k in (14, 15, 16, 17):                                            # a target without its rows / weight / loss / gradient image
        bad = list(full)
        bad[k] = None
        assert L.harp_rasterize_l1_fwd(*bad) == E, k
    bad = list(full)
    bad[6] = 0                                                            # a target on a hard pass
    assert L.harp_rasterize_l1_fwd(*bad) == E
    fb = [n, f, B, V, F, S, 1, bl, sg, p(ws), p(fid), p(a), p(y), p(rows), p(wt), p(loss), p(g), None, p(g_ndc), st()]
    for k, v in ((18, None), (12, None), (6, 0), (6, 2)):                 # no g_ndc, no target, soft bit clear
        bad = list(fb)
        bad[k] = v
        assert L.harp_rasterize_l1_fwd_bwd(*bad) == E, k
    state = torch.zeros(B * 4, dtype=torch.int32, device=DEV)
    assert L.harp_rasterize_fwd_keep(n, f, B, V, F, S, 0, p(ws), p(fid), None, p(state), st()) == E
    assert L.harp_rasterize_fwd_keep(n, f, B, V, F, S, 0, p(ws), p(fid), p(z), None, st()) == E
    assert L.harp_rasterize_fwd_keep(n, f, B, V, F, S, 0, p(ws), None, p(z), p(state), st()) == E
    sb = [f, B, V, F, S, bl, sg, p(ws), p(a), p(g), p(g_ndc), st()]
    for k in (0, 7, 8, 9, 10):
        bad = list(sb)
        bad[k] = None
        assert L.harp_silhouette_bwd(*bad) == E, k
    pair = [n, bl, p(ws), n, 0.0, p(ws), f, B, V, F, S, st()]
    for k, v in ((0, None), (2, None), (3, None), (5, None), (6, None), (1, -1.0), (4, -1.0), (7, 0), (8, 0), (9, 0), (10, 0)):
        bad = list(pair)
        bad[k] = v
        assert L.harp_raster_setup_pair(*bad) == E, k
    # a record buffer bound for fewer frames / a smaller image than the call's
    rec = torch.full((L.harp_sil_records_bytes(B, S, 16),), 0xFF, dtype=torch.uint8, device=DEV)
    assert L.harp_sil_records_bind(None, p(rec), 16, B, F, S) == E and L.harp_sil_records_bind(p(ws), p(rec), -1, B, F, S) == E
    assert L.harp_sil_records_bind(p(ws), p(rec), 16, 0, F, S) == E and L.harp_sil_records_bind(p(ws), p(rec), 16, B, (1 << 24) + 1, S) == E
    for b_, s_ in ((B - 1, S), (B, 64)):                                  # one frame fewer; one super-tile a side instead of two
        assert L.harp_sil_records_bytes(b_, s_, 16) < L.harp_sil_records_bytes(B, S, 16)
        assert L.harp_sil_records_bind(p(ws), p(rec), 16, b_, F, s_) == 0
        try:
            assert L.harp_rasterize_fwd(n, f, B, V, F, S, 1, bl, sg, p(ws), p(fid), p(z), p(a), st()) == E
            assert L.harp_rasterize_l1_fwd(*full) == E
            assert L.harp_silhouette_bwd(*sb) == E
        finally:
            assert L.harp_sil_records_bind(p(ws), None, 0, B, F, S) == 0
    torch.cuda.synchronize()
    assert bool((fid == SENT_F).all()) and bool((z == SENT_Z).all()) and bool((a == SENT_A).all()) and bool((g == SENT_G).all())
    assert loss.item() == 0 and g_ndc.abs().max().item() == 0 and int(state.abs().max()) == 0
    assert bool((rec == 0xFF).all())
