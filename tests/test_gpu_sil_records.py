"""Silhouette records (harp_sil_records_bind): the camera raster's soft pass stores its (pixel, face)
pairs per 16x16 tile and the silhouette backward walks them instead of finding them again.  Against the staged walk of
harp_silhouette_bwd on the same workspace: the forward outputs are bit-identical with records on and off, d loss / d ndc agrees up to
the order of float sums — at the bench's sizes, off the tile grid, on the striding grid, with sparse outputs, without face ids, with a
capacity so small that most tiles take the staged walk, and after a larger scene left its records in the same buffers."""
import pytest
import torch

from tests._scene import make_fit_case, make_scene, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def sc():
    return make_scene(T=3, S=128, seed=0)


def _scene_ndc(sc, S, shrink=1.0, B=3):
    from oracle import harp_ref as H, p3d_like as P
    f_S = sc["focal"] * S / sc["S"]
    params = dict(pose=sc["seq"]["pose"], rot=sc["seq"]["rot"], trans=sc["seq"]["trans"], shape=sc["seq"]["shape"].mean(0),
                  verts_disps=torch.zeros(3093, 1))
    fid = torch.arange(B) % 3
    with torch.no_grad():
        _, v = H.prepare_mesh(params, fid, sc["model"], sc["topo"])
        R, T = H.camera_RT(sc["seq"]["cam"][fid], S, f_S)
        _, ndc = P.world_to_ndc(v, R, T, f_S * shrink, (S / 2, S / 2), S)
    return ndc.float().to(DEV).contiguous(), sc["topo"]["faces"].int().to(DEV).contiguous()


def _engine_ndc(kind, S, B):
    """camera-view NDC vertices of a fitting step of the engine (the bench's scenes: realistic poses, framing and mesh density)"""
    case = make_fit_case(kind, T=min(B, 4), S=S, B=B, seed=2, device=DEV)
    eng = case["eng"]
    eng.keep_image = False
    eng.set_schedule((torch.arange(B) % min(B, 4)).reshape(1, B).int())
    eng.step(None, True, False, use_graph=False)
    torch.cuda.synchronize()
    return eng.s["ndc_c"][:B].clone(), eng.topo.faces


def _run(ndc, faces, S, sparse=False, face_ids=True, cap=256, rec=None, ws=None):
    """forward without and with records, both backward forms on the forward's outputs.  Returns (outputs off, outputs on, g_ndc staged,
    g_ndc records, largest record count of a tile)"""
    from harp_amd import _lib, ops
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream
    B, V, F = ndc.shape[0], ndc.shape[1], faces.shape[0]
    g = torch.Generator().manual_seed(5)
    y_sil = (torch.rand(4, S, S, generator=g) > 0.5).float().to(DEV)
    rows = (torch.arange(B, dtype=torch.int32) % 4).to(DEV)
    w = torch.tensor([7.0], device=DEV)
    ws = ops.rasterize_workspace(B, F, S, DEV) if ws is None else ws
    if rec is None:
        rec = torch.empty(L.harp_sil_records_bytes(B, S, cap), dtype=torch.uint8, device=DEV)
        rec.fill_(0xFF)                                   # (garbage: every count the backward reads must be written by the forward)
    soft = 1 | (2 if sparse else 0)
    bind = lambda on: _lib.check(L.harp_sil_records_bind(p(ws), p(rec) if on else None, cap, B, F, S), "bind")
    outs = []
    g_st, g_rec = torch.zeros(B, V, 3, device=DEV), torch.zeros(B, V, 3, device=DEV)
    try:
        for on in (False, True):
            bind(on)
            face_id = torch.full((B, S, S), -7, dtype=torch.int32, device=DEV) if face_ids else None
            alpha, g_alpha = torch.full((B, S, S), 0.5, device=DEV), torch.full((B, S, S), 0.25, device=DEV)
            loss = torch.zeros(1, device=DEV)
            args = (p(ndc), p(faces), B, V, F, S, soft, ops.SIL_BLUR, ops.SIL_SIGMA, p(ws), p(face_id) if face_ids else None, None, p(alpha),
                    p(y_sil), p(rows), p(w), p(loss), p(g_alpha), None)
            _lib.check(L.harp_rasterize_l1_fwd(*args, st()), "fwd")
            outs.append((face_id, alpha, g_alpha, loss))
        face_id, alpha, g_alpha, loss = outs[1]
        for on, g_ndc in ((False, g_st), (True, g_rec)):
            bind(on)
            _lib.check(L.harp_silhouette_bwd(p(faces), B, V, F, S, ops.SIL_BLUR, ops.SIL_SIGMA, p(ws), p(alpha), p(g_alpha), p(g_ndc), st()), "bwd")
        torch.cuda.synchronize()
    finally:
        bind(False)
    nsx = (S + 63) // 64
    counts = rec[:B * nsx * nsx * 16 * 4].view(torch.int32)
    return outs[0], outs[1], g_st, g_rec, int(counts.max().item())


def _check(r, min_records=1):
    off, on, g_st, g_rec, mx = r
    for a, b in zip(off[:3], on[:3]):
        if a is not None:
            assert torch.equal(a, b)                      # face ids, alpha, g_alpha: bit-identical with records on
    assert abs(on[3].item() - off[3].item()) <= 1e-6 * abs(off[3].item())      # (the loss: a float atomic sum over the tiles)
    assert g_st.abs().max().item() > 0 and (g_rec[..., 2] == 0).all()
    assert rel(g_rec.double(), g_st.double()) < 1e-5, rel(g_rec.double(), g_st.double())
    assert mx >= min_records
    return mx


@pytest.mark.parametrize("S,loop,sparse,face_ids", [(128, 0, False, True), (128, 0, True, True), (128, 0, True, False), (128, 16, False, True),
                                                    (128, 16, True, False), (300, 0, False, True), (301, 0, True, True), (301, 16, False, True)])
def test_records_backward_matches_the_staged_walk(sc, S, loop, sparse, face_ids, monkeypatch):
    if loop:
        monkeypatch.setenv("HARP_RASTER_LOOP", str(loop))
    ndc, faces = _scene_ndc(sc, S)
    _check(_run(ndc, faces, S, sparse=sparse, face_ids=face_ids))


@pytest.mark.parametrize("cap", [0, 1, 8])
def test_records_over_capacity_take_the_staged_walk(sc, cap):
    """a capacity far below a rim tile's pairs: (almost) every tile takes the staged walk, tiles at or under it the records"""
    ndc, faces = _scene_ndc(sc, 128)
    _check(_run(ndc, faces, 128, cap=cap))


def test_no_stale_records(sc):
    """a full-size scene, then the same hand shrunk to a few tiles on the same workspace and record buffer: the second backward reads
    only what the second forward wrote (tiles the first scene filled and the second leaves empty or sparse hold stale counts / records)"""
    from harp_amd import _lib, ops
    S = 128
    ndc_a, faces = _scene_ndc(sc, S)
    ndc_b, _ = _scene_ndc(sc, S, shrink=0.3)
    B, F = ndc_a.shape[0], faces.shape[0]
    ws = ops.rasterize_workspace(B, F, S, DEV)
    rec = torch.full((_lib.lib().harp_sil_records_bytes(B, S, 256),), 0xFF, dtype=torch.uint8, device=DEV)
    _check(_run(ndc_a, faces, S, rec=rec, ws=ws))
    _check(_run(ndc_b, faces, S, rec=rec, ws=ws, sparse=True))
    _check(_run(ndc_a, faces, S, rec=rec, ws=ws))


@pytest.mark.parametrize("kind,S,B", [("hand", 512, 32), ("arm", 1024, 1), ("arm", 1024, 8)])
def test_records_backward_at_the_bench_sizes(kind, S, B):
    ndc, faces = _engine_ndc(kind, S, B)
    _check(_run(ndc, faces, S, sparse=True, face_ids=(kind == "arm")), min_records=8)


@pytest.mark.parametrize("stage", ["both", "geometry"])
def test_engine_sil_records_switch(stage):
    """FitEngine with sil_records on (default) and off: losses and the whole gradient arena agree up to the order of float atomics,
    eagerly and graph-replayed (the pattern of test_schedule_switches_give_the_default_schedules_result); geometry: the stage without
    the shader backward, whose camera raster forms no face ids"""
    case = make_fit_case("hand", T=3, S=128, B=3, seed=4, device=DEV)
    eng = case["eng"]
    eng.keep_image = False
    eng.auto_draw = False
    eng.draw_texture_offsets()
    eng.set_lr(0.0, 0.0)
    eng.set_schedule(torch.arange(3).reshape(1, 3).int())
    app = stage == "both"
    assert eng.sil_records

    def run(graph):
        for _ in range(3 if graph else 1):
            eng.step(None, True, app, use_graph=graph)
        torch.cuda.synchronize()
        return eng.g_buf.double().clone(), eng.loss_vec[:9].double().clone()
    ref = {g: run(g) for g in (False, True)}
    eng.sil_records = False
    try:
        for graph in (False, True):
            g, l = run(graph)
            assert g.abs().max().item() > 0
            assert rel(g, ref[graph][0]) < 1e-5, (graph, rel(g, ref[graph][0]))
            assert ((l - ref[graph][1]).abs() <= 1e-5 * ref[graph][1].abs() + 1e-9).all(), (graph, l, ref[graph][1])
    finally:
        eng.sil_records = True
    for graph in (False, True):
        g, l = run(graph)
        assert rel(g, ref[graph][0]) < 1e-5, ("back on", graph, rel(g, ref[graph][0]))
