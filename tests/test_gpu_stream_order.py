"""Ordering between the step's streams, tested by delay injection (tests/_delay.py).

The step runs on the main stream, the second stream (silhouette backward, then harp_texel_reduce, harp_texel_finish and the maps' split
Adam), the extra streams of the mesh terms and the VGG parts.  Every other GPU test synchronises before it reads, which hides a reader
that runs ahead of its writer.  Here one side of every fork is made ~300 us late per launch, and results are read WITHOUT a synchronise in
between: gradients per arena segment and the loss vector must equal the undelayed reference of the same configuration (lr = 0, fixed
texture offsets, a one-row schedule: every step starts from the same state).  Two positive controls show that the detector catches the
races it is meant to catch.

Measured on MI355X: torch.cuda._sleep counts clock64 at 0.42 ns per cycle (2.4 GHz), ~710 k cycles for the 300 us delay.  The per-segment
bounds are tests/_scene.REPLAY_SPREAD x 10 (capped at 1e-4); the delayed steps of every configuration below stayed within 1.5 x the
undelayed replay spread of each segment.  With the join deferred (the behaviour before forward_backward() joined the maps' branch) the
texture gradient read right after the return was off by rel-L2 0.77 and the normal map's by 0.44."""
import numpy as np
import pytest
import torch

from tests._delay import calibrate, delayed
from tests._scene import assert_blocks, block_errors, make_fit_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
LW = [1, 1 / 16, 1 / 8, 1 / 4, 1]


def _fit_case(kind):
    case = make_fit_case(kind, T=3, S=128, B=3, seed=4, device=DEV)
    eng = case["eng"]
    eng.keep_image = False
    eng.auto_draw = False
    eng.draw_texture_offsets()
    eng.set_lr(0.0, 0.0)
    eng.set_schedule(torch.arange(3).reshape(1, 3).int())
    return case


@pytest.fixture(scope="module")
def hand():
    calibrate()
    return _fit_case("hand")


def _losses_match(l, ref):
    return bool(((l - ref).abs() <= 1e-5 * ref.abs() + 1e-9).all())


def _fb_frames(eng):
    fid = torch.arange(3, dtype=torch.int32, device=DEV)
    eng.fid.copy_(fid)
    eng.tfid.copy_(fid)
    eng.set_stage(True, True)


def test_delay_is_calibrated():
    _, n, us = calibrate()
    assert 100.0 <= us <= 2000.0 and n > 0


def test_gradients_are_final_when_forward_backward_returns(hand):
    """A caller that reads eng.g_buf on the current stream right after forward_backward(), and back-to-back forward_backward() calls
    (the target loops of bench.py and tests/_scene.py), with every second-stream launch late: the maps' branch (texel reduce -> finish,
    a non-atomic += into the texture / normal-map gradients) must be joined before forward_backward() returns."""
    eng = hand["eng"]
    _fb_frames(eng)
    eng.forward_backward(True, True)
    torch.cuda.synchronize()
    g0, l0 = eng.g_buf.clone(), eng.loss_vec[:10].clone()
    for calls in (1, 2):
        with delayed(eng, "side"):
            for _ in range(calls):
                eng.forward_backward(True, True)
            g, l = eng.g_buf.clone(), eng.loss_vec[:10].clone()         # (enqueued on the current stream, no synchronise in between)
        torch.cuda.synchronize()
        print(f"[eager read, {calls} call(s)] per-segment rel-L2", {k: float("%.1e" % e) for k, e in block_errors(eng, g, g0).items()})
        assert_blocks(eng, g, g0, tag=("forward_backward x%d" % calls))
        assert _losses_match(l, l0), (calls, l, l0)
        assert eng._maps_pending is None


def test_detector_sees_a_deferred_join(hand):
    """Positive control: the pre-fix behaviour (the maps' branch left open on return, `_defer_maps_join=True`) under the same delays
    leaves the texture gradient without what harp_texel_finish adds."""
    eng = hand["eng"]
    _fb_frames(eng)
    eng.forward_backward(True, True)
    torch.cuda.synchronize()
    g0 = eng.g_buf.clone()
    with delayed(eng, "side"):
        eng.forward_backward(True, True, _defer_maps_join=True)
        assert eng._maps_pending is not None
        g = eng.g_buf.clone()
    torch.cuda.synchronize()
    eng._join_maps()
    errs = block_errors(eng, g, g0)
    print("[deferred join] per-segment rel-L2", {k: float("%.1e" % e) for k, e in errs.items()})
    assert errs["texture"] > 0.5, errs


B1, B2 = np.float32(0.9), np.float32(0.999)


def adam_mismatches(eng):
    """Check the optimiser state after ONE Adam update from m = v = 0 (grad_scale 1) against the final gradient arena: inside the two
    optimiser spans m = float32((1 - beta1) g) bit for bit (the kernel's m + (g - m)(1 - beta1) with m = 0) and v = float32((1 - beta2) g^2)
    within 1 ulp (fma contraction); outside them m = v = 0 exactly.  Returns {segment: number of elements that fail}."""
    g, m, v = (t.cpu().numpy() for t in (eng.g_buf, eng.m_buf, eng.v_buf))
    inside = np.zeros(g.shape, bool)
    for o, n in (eng.coarse_span, eng.app_span):
        inside[o:o + n] = True
    gd = g.astype(np.float64)
    m_ref = (gd * float(np.float32(1) - B1)).astype(np.float32)           # (an exact product of two floats, rounded once)
    v_ref = (gd * float(np.float32(1) - B2) * gd).astype(np.float32)
    ulp = np.spacing(np.abs(v_ref)) + np.finfo(np.float32).tiny
    bad = np.where(inside, (m != m_ref) | (np.abs(v.astype(np.float64) - v_ref) > ulp), (m != 0) | (v != 0))
    out = {}
    for k in eng.grads:
        o, n, _ = eng.arena.offsets[k]
        out[k] = int(bad[o:o + n].sum())
    out["(padding)"] = int(bad.sum()) - sum(out.values())
    return out


def _run_steps(eng, graph, steps=3):
    """`steps` steps from the same state; m and v are zeroed in place before the last one.  Returns (g_buf, loss_vec[:10])."""
    for i in range(steps):
        if i == steps - 1:
            eng.m_buf.zero_()
            eng.v_buf.zero_()
        eng.step(None, True, True, use_graph=graph)
    g, l = eng.g_buf.clone(), eng.loss_vec[:10].clone()
    torch.cuda.synchronize()
    return g, l


SWITCHES = [dict(), dict(tail_side=True), dict(mesh_third=True), dict(fused_sil_bwd=True), dict(sil_late=True), dict(mesh_terms_late=True),
            dict(graph_order=False), dict(camera_first=False), dict(split_adam=False), dict(texel_records=False), "arm", "perceptual"]


@pytest.mark.parametrize("config", SWITCHES, ids=lambda c: c if isinstance(c, str) else ("-".join(f"{k}={v}" for k, v in c.items()) or "default"))
def test_step_under_delays(hand, config):
    """Eager and graph-replayed step() with every second-stream launch late, then with every main-stream launch late: per-segment
    gradients and the loss vector of the undelayed step of the same configuration, and an Adam update that read the FINAL gradients
    (with lr = 0 the parameters alone could not show a split Adam that ran ahead of harp_texel_finish)."""
    from harp_amd.model.vgg import Vgg16Features
    case = _fit_case("arm") if config == "arm" else hand
    eng = case["eng"]
    switches = config if isinstance(config, dict) else {}
    defaults = {k: getattr(eng, k) for k in switches}
    for k, v in switches.items():
        setattr(eng, k, v)
    if config == "perceptual":
        eng.set_perceptual(Vgg16Features(layers_weights=LW, weights="random", seed=2), precision=2)
        eng.vgg_streams = 2
    try:
        ref = {graph: _run_steps(eng, graph) for graph in (False, True)}
        assert sum(adam_mismatches(eng).values()) == 0, adam_mismatches(eng)         # (undelayed, graph-replayed)
        for where in ("side", "main"):
            for graph in (False, True):
                with delayed(eng, where):
                    g, l = _run_steps(eng, graph)
                tag = (config, where, "graph" if graph else "eager")
                errs = assert_blocks(eng, g, ref[graph][0], tag=tag)
                print(f"[{tag}] per-segment rel-L2", {k: float("%.1e" % e) for k, e in errs.items()})
                assert _losses_match(l, ref[graph][1]), (tag, l, ref[graph][1])
                bad = adam_mismatches(eng)
                assert sum(bad.values()) == 0, (tag, bad)
    finally:
        for k, v in defaults.items():
            setattr(eng, k, v)
        if config == "perceptual":
            eng.set_perceptual(None)
        eng._graphs = {}


def test_detector_sees_adam_ahead_of_texel_finish(hand, monkeypatch):
    """Positive control of the Adam check: eager step() with the maps' update in the step's last launch (split_adam off) and the join of
    the maps' branch removed, under the side delays — Adam then reads the texture gradient before harp_texel_finish has added to it."""
    eng = hand["eng"]
    monkeypatch.setattr(eng, "split_adam", False)
    _run_steps(eng, False, steps=1)
    assert sum(adam_mismatches(eng).values()) == 0, adam_mismatches(eng)
    monkeypatch.setattr(eng, "_join_maps", lambda: None)
    with delayed(eng, "side"):
        _run_steps(eng, False, steps=1)
    torch.cuda.synchronize()
    eng._maps_pending = None
    bad = adam_mismatches(eng)
    print("[Adam ahead of texel_finish] mismatching elements per segment", bad)
    assert bad["texture"] > 0, bad
