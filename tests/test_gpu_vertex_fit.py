"""-m gpu: harp_mano_vertex_fit (csrc/vertex_fit.hip), optimize_for_mano_param(method="lm") and Motion.from_vertices against the yardstick of
tests/_vertex_fit_ref.py.

No bound here is a number fixed in advance.  Each is computed in the test from the yardstick itself:

    bound = 8 x the float32 yardstick's error against the float64 yardstick on the same inputs            (R.FACTOR)

— the same code in float32 (forward, J^T W J, Cholesky of the Jacobi-scaled system) is the error model of a correct float32 solver, and the
factor covers what the kernel does differently: 2334-term and 135-term dots summed in another order, and the device's sinf / cosf.  A
quantity that is ONE number per frame (a cost) has a float32 error that can come out tiny by luck on a single frame, so both sides of every
comparison are the worst over all the frames that the test runs, never one frame's.  Measured errors and bounds are recorded side by side in
profiles/vertex_fit_errors.txt and DESIGN.md §27.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from tests import _ik_ref
from tests import _vertex_fit_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
# vertices whose weight is zero in the weighted cases: both sides of the kernel's 64-vertex tile boundaries, of the 256-vertex rounds of
# its forward, and inside the last, partial tile (768 .. 777)
W_ZERO = [0, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 511, 512, 575, 576, 767, 768, 769, 776, 777]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _f32(t):
    return None if t is None else t.to(torch.float32).to(DEV).contiguous()


def _all_bits(out):
    return [_bits(t) for t in out if t is not None]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_all_bits(a), _all_bits(b)))


def _x(out):
    b = out.betas if out.betas.dim() == 2 else out.betas[None].expand(out.pose48.shape[0], 10)
    return torch.cat([out.pose48, b, out.trans], 1).cpu().double()


@pytest.fixture(scope="module")
def dm():
    from harp_amd import synth
    from harp_amd.manopth.manolayer import ManoDeviceModel
    return ManoDeviceModel(synth.make_mano_model(), torch.device(DEV))


def _solve(dm, x0, targets, betas=None, **kw):
    """x0 (T,61) holds the start; betas: None = x0's own (T,10), else what is passed for a frozen shape"""
    from harp_amd import ops
    b = x0[:, 48:58] if betas is None else betas
    return ops.mano_vertex_fit(dm, _f32(targets), _f32(x0[:, :48]), _f32(b), _f32(x0[:, 58:]), **kw)


def _scene32(T, seed, noise=0.0, **kw):
    """the seeded scene as the kernel sees it: float32 targets and a float32 rigid start; the yardstick runs from exactly those numbers"""
    s = R.scene(T=T, seed=seed, noise=noise, **kw)
    s["targets32"] = s["targets"].float()
    s["x0_32"] = R.rigid_x0(s, targets=s["targets32"]).float()
    return s


@pytest.fixture(scope="module")
def exact():
    s = _scene32(8, 0)
    kw = dict(iters=10)
    s["y64"] = R.lm(s["model"], s["x0_32"].double(), s["targets32"].double(), **kw)
    s["y32"] = R.lm(s["model"], s["x0_32"], s["targets32"], dtype=torch.float32, **kw)
    return s


@pytest.fixture(scope="module")
def noisy():
    s = _scene32(8, 1, noise=0.002)
    s["y64"] = R.lm(s["model"], s["x0_32"].double(), s["targets32"].double(), iters=20)
    s["y32"] = R.lm(s["model"], s["x0_32"], s["targets32"], iters=10, dtype=torch.float32)
    return s


# ---- 1. iters = 0 at the input ----------------------------------------------------------------------------------------------------------
def _poses(kind, T, hands_mean, rng):
    x = np.zeros((T, 61), np.float32)
    if kind == "aa_zero":                                 # stored pose = -hands_mean: every joint's axis-angle is exactly 0
        x[:, 3:48] = -hands_mean
    elif kind == "tiny":
        x[:, :48] = 1e-6
    elif kind == "random":
        x[:, :48] = rng.normal(size=(T, 48)) * 0.3
    elif kind == "near_pi":
        x[:, 3:48] = rng.normal(size=(T, 45)) * 0.3
        u = rng.normal(size=(T, 3))
        x[:, :3] = (np.pi - 1e-3) * u / np.linalg.norm(u, axis=1, keepdims=True)
    return x


def _rel(got, ref):
    """per frame: the largest deviation relative to the frame's largest entry of the quantity"""
    T = ref.shape[0]
    d, m = (got.double() - ref.double()).abs().reshape(T, -1).amax(1), ref.double().abs().reshape(T, -1).amax(1)
    return float((d / m).max())


# (betas, solve_shape, betas given as, trans, weights)
_CASES = [("zero", True, "per_frame", False, False), ("random", True, "per_frame", True, True),
          ("random", False, "shared", True, False), ("random", False, "per_frame", False, True)]


@pytest.mark.parametrize("kind", ["zero", "aa_zero", "tiny", "random", "near_pi"])
def test_everything_at_the_input(dm, kind):
    """iters = 0 evaluates at the input: verts, jac, A, g and cost[:, 0] against float64, each relative to the frame's largest entry of
    that quantity; the in/out rows come back bit for bit; the frozen columns of A and g are exactly the contract's.  T = 1, 2, F, F + 1
    for F frames per workgroup; betas zero / random, solved / frozen as (10,) / frozen as (T,10); trans zero / not; weights None / a
    pattern of zeros across the tile boundaries with a NaN target under a weight of 1."""
    from harp_amd import ops, synth
    F = ops.mano_vertex_fit_frames_per_block()
    model = _ik_ref.model64(synth.make_mano_model())
    hm = model["hands_mean"].numpy().astype(np.float32)
    rng = np.random.default_rng(11)
    names = ("verts", "jac", "A", "g", "cost")
    worst, worst32 = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0)
    for T in sorted({1, 2, F, F + 1}):
        for beta_kind, solve_shape, given, with_trans, with_w in _CASES:
            x = _poses(kind, T, hm, rng)
            if beta_kind == "random":
                x[:, 48:58] = rng.normal(size=10 if given == "shared" else (T, 10)) * 0.5
            if with_trans:
                x[:, 58:] = rng.uniform(-0.3, 0.3, size=(T, 3))
            x = torch.as_tensor(x)
            targets = torch.as_tensor(rng.uniform(-0.3, 0.3, size=(T, 778, 3)), dtype=torch.float32)
            w = None
            if with_w:
                w = torch.as_tensor(rng.uniform(0.5, 1.5, size=(T, 778)), dtype=torch.float32)
                w[:, W_ZERO] = 0.0
                targets[:, 300] = float("nan")            # unused although its weight is positive
            betas = x[0, 48:58].clone() if given == "shared" else x[:, 48:58].clone()
            kw = dict(pose_prior_weight=1e-3, shape_prior_weight=2e-3)
            out = _solve(dm, x, targets, betas=betas, weights=_f32(w), solve_shape=solve_shape, iters=0, verts=True, jac=True, normal=True, **kw)
            assert torch.equal(_bits(out.pose48), _bits(x[:, :48])) and torch.equal(_bits(out.trans), _bits(x[:, 58:]))
            assert torch.equal(_bits(out.betas), _bits(betas)) and out.status.tolist() == [0] * T
            assert torch.equal(_bits(out.cost[:, 0]), _bits(out.cost[:, 1]))
            A, g = out.A.cpu(), out.g.cpu()
            if not solve_shape:
                off = A.clone()
                off[:, range(48, 58), range(48, 58)] -= 1.0
                assert bool((off[:, 48:58, :] == 0).all() and (off[:, :, 48:58] == 0).all() and (g[:, 48:58] == 0).all())
            assert torch.equal(A, A.transpose(1, 2))
            n64 = R.normal(model, x.double(), targets, weights=w, solve_shape=solve_shape, **kw)
            n32 = R.normal(model, x, targets, weights=w, solve_shape=solve_shape, dtype=torch.float32, **kw)
            with torch.no_grad():
                v64, v32 = R.verts(model, x.double()), R.verts(model, x, torch.float32)
            got = dict(verts=out.verts.cpu() / 1000.0, jac=out.jac.cpu(), A=A, g=g, cost=out.cost[:, :1].cpu())
            ref = dict(verts=v64, jac=n64["J"], A=n64["A"], g=n64["g"], cost=n64["C"][:, None])
            f32 = dict(verts=v32, jac=n32["J"], A=n32["A"], g=n32["g"], cost=n32["C"][:, None])
            for k in names:
                worst[k], worst32[k] = max(worst[k], _rel(got[k], ref[k])), max(worst32[k], _rel(f32[k], ref[k]))
    print(f"[vertex_fit] input[{kind}] " + " ".join(f"{k} {worst[k]:.3e} (bound {R.FACTOR * worst32[k]:.3e})" for k in names))
    for k in names:
        assert worst[k] <= R.FACTOR * worst32[k], k


# ---- 2. one step from the rigid start -----------------------------------------------------------------------------------------------------
def test_one_step_from_the_rigid_start(dm, exact):
    sc = exact
    x0 = sc["x0_32"].double()
    y1 = R.lm(sc["model"], x0, sc["targets32"].double(), iters=1)
    y1_32 = R.lm(sc["model"], sc["x0_32"], sc["targets32"], iters=1, dtype=torch.float32)
    c0, c1 = y1["cost"][0], y1["cost"][1]
    counted = (c0 - c1) / c0 > 1e-3                       # a float32 accept / reject cannot be expected to agree on a tie
    assert int((~counted).sum()) <= 0.1 * counted.numel()
    assert bool(counted.all())                            # (8 frames: the yardstick leaves out none, verified on the CPU)
    out = _solve(dm, sc["x0_32"], sc["targets32"], iters=1)
    step = (y1["x"] - x0).abs().amax(1)
    dx = float((((_x(out) - y1["x"]).abs().amax(1) / step)[counted]).max())
    dx32 = float((((y1_32["x"].double() - y1["x"]).abs().amax(1) / step)[counted]).max())
    dc = float((((out.cost[:, 1].cpu().double() - c1).abs() / c1)[counted]).max())
    dc32 = float((((y1_32["cost"][1].double() - c1).abs() / c1)[counted]).max())
    print(f"[vertex_fit] one_step x {dx:.3e} (bound {R.FACTOR * dx32:.3e}) cost1 {dc:.3e} (bound {R.FACTOR * dc32:.3e}) "
          f"counted {int(counted.sum())} of {counted.numel()}")
    assert out.status.cpu()[counted].tolist() == [1] * int(counted.sum())
    assert dx <= R.FACTOR * dx32
    assert dc <= R.FACTOR * dc32


# ---- 3. convergence -------------------------------------------------------------------------------------------------------------------
def test_convergence_on_exact_frames(dm, exact):
    sc = exact
    out = _solve(dm, sc["x0_32"], sc["targets32"], iters=10, verts=True)
    rms = float((out.verts.cpu().double() / 1000.0 - sc["targets32"].double()).pow(2).sum(-1).mean(1).sqrt().max() * 1000.0)
    rms32 = float(R.rms_mm(sc["model"], sc["y32"]["x"], sc["targets32"], torch.float32).max())
    rms64 = float(R.rms_mm(sc["model"], sc["y64"]["x"], sc["targets32"]).max())
    print(f"[vertex_fit] convergence exact rms {rms:.3e} mm (bound {R.FACTOR * rms32:.3e}; float64 yardstick {rms64:.3e}) status {out.status.tolist()}")
    assert int(out.status.min()) >= 1                     # (float32 stops accepting where its cost stops falling: 4 .. 8 of 10, §27)
    assert rms <= R.FACTOR * rms32


def test_convergence_on_noisy_frames(dm, noisy):
    sc = noisy
    out = _solve(dm, sc["x0_32"], sc["targets32"], iters=10)
    c20 = sc["y64"]["cost"][20]
    m = float((out.cost[:, 1].cpu().double() / c20 - 1.0).max())
    m32 = float((sc["y32"]["cost"][10].double() / c20 - 1.0).abs().max())
    print(f"[vertex_fit] convergence noisy cost/yardstick - 1 {m:.3e} (bound {R.FACTOR * m32:.3e}) rms {float((c20 / 778).sqrt().mean() * 1000):.3f} mm")
    assert m <= R.FACTOR * m32


# ---- 4. unused vertices never enter ---------------------------------------------------------------------------------------------------
def test_unused_vertices_never_enter(dm, exact):
    sc = exact
    T = 3
    x0, tg = sc["x0_32"][:T], sc["targets32"][:T]
    w = torch.ones(T, 778)
    w[:, W_ZERO] = 0.0
    kw = dict(iters=4, verts=True, jac=True, normal=True)
    outs = []
    for fill in (1e30, float("nan"), 0.0):
        t = tg.clone()
        t[:, W_ZERO] = fill
        outs.append(_solve(dm, x0, t, weights=_f32(w), **kw))
    assert _same(outs[0], outs[2]) and _same(outs[1], outs[2])
    t = tg.clone()                                        # a NaN target with weight 1 is unused
    t[:, W_ZERO] = float("nan")
    assert _same(_solve(dm, x0, t, **kw), outs[2])
    assert int(outs[2].status.min()) >= 1

    for n_used, solved in ((20, False), (21, True)):      # the middle frame; its neighbours do not notice
        w = torch.ones(T, 778)
        w[1] = 0.0
        w[1, 37 * torch.arange(n_used)] = 1.0
        out = _solve(dm, x0, tg, weights=_f32(w), **kw)
        st = out.status.tolist()
        assert (st[1] >= 0) == solved and (solved or st[1] == -1) and min(st[0], st[2]) >= 1
        if not solved:
            assert torch.equal(_bits(_x(out)[1].float()), _bits(x0[1])) and torch.equal(_bits(out.cost[1, 0]), _bits(out.cost[1, 1]))
        else:
            assert float(out.cost[1, 1]) <= float(out.cost[1, 0]) and bool(torch.isfinite(_x(out)).all())
        for f in (0, 2):
            alone = _solve(dm, x0[f:f + 1], tg[f:f + 1], weights=_f32(w[f:f + 1]), **kw)
            assert all(torch.equal(_bits(a[f]), _bits(b[0])) for a, b in zip(out, alone) if a is not None), (n_used, f)
    # 21 used vertices whose weight is the smallest float32: a derivative with respect to a rotation is a lever arm, below 0.5 m, so w J
    # rounds to zero and A's rotation diagonals ARE zero — a non-positive diagonal, every step is rejected, and the frame is still "solved"
    w = torch.zeros(1, 778)
    w[0, 37 * torch.arange(21)] = 1.4e-45
    out = _solve(dm, x0[:1], tg[:1], weights=_f32(w), **kw)
    assert out.status.tolist() == [0] and torch.equal(_bits(_x(out).float()), _bits(x0[:1]))
    assert torch.equal(_bits(out.cost[:, 0]), _bits(out.cost[:, 1]))


# ---- 5. a fixed shape on someone else's hand --------------------------------------------------------------------------------------------
def test_fixed_shape_on_another_hand(dm, exact):
    sc = exact
    avatar = torch.as_tensor(np.random.default_rng(3).normal(size=10) * 0.5, dtype=torch.float32)
    x0 = R.rigid_x0(sc, targets=sc["targets32"], betas=avatar.double()[None]).float()
    kw = dict(solve_shape=False)
    y64 = R.lm(sc["model"], x0.double(), sc["targets32"].double(), iters=20, **kw)
    y32 = R.lm(sc["model"], x0, sc["targets32"], iters=10, dtype=torch.float32, **kw)
    for betas in (avatar, avatar[None].expand(8, 10).contiguous()):
        out = _solve(dm, x0, sc["targets32"], betas=betas, iters=10, **kw)
        assert torch.equal(_bits(out.betas), _bits(betas))
        c20 = y64["cost"][20]
        m = float((out.cost[:, 1].cpu().double() / c20 - 1.0).abs().max())
        m32 = float((y32["cost"][10].double() / c20 - 1.0).abs().max())
        print(f"[vertex_fit] fixed shape {tuple(betas.shape)} cost/yardstick - 1 {m:.3e} (bound {R.FACTOR * m32:.3e}) "
              f"rms {float((c20 / 778).sqrt().mean() * 1000):.3f} mm")
        assert float(out.cost[:, 1].min()) > 0.0
        assert m <= R.FACTOR * m32


# ---- 6. rejected steps never raise the cost ---------------------------------------------------------------------------------------------
def test_rejected_steps_never_raise_the_cost(dm):
    """from zero (no rigid start) on targets rotated by 3 rad the first steps overshoot.  The kernel is deterministic, so the run with k
    iterations is the prefix of the run with k + 1: the cost after every iteration is read from 12 calls, and the status must be the
    number of strict decreases in that history."""
    iters = 12
    s = R.scene(T=6, seed=1, root_lo=3.0, root_hi=3.0)
    x0, tg = torch.zeros(6, 61), s["targets"].float()
    hist = [_solve(dm, x0, tg, iters=0).cost[:, 0].cpu()]
    for k in range(1, iters + 1):
        out = _solve(dm, x0, tg, iters=k)
        assert torch.equal(_bits(out.cost[:, 0]), _bits(hist[0]))
        hist.append(out.cost[:, 1].cpu())
    hist = torch.stack(hist)
    falls = (hist[1:] < hist[:-1]).sum(0)
    print(f"[vertex_fit] rejected status {out.status.tolist()} strict decreases {falls.tolist()} cost {out.cost.cpu().tolist()}")
    assert bool((hist[1:] <= hist[:-1]).all()) and bool((out.cost[:, 1] <= out.cost[:, 0]).all())
    assert out.status.cpu().tolist() == falls.tolist()
    assert bool(torch.isfinite(_x(out)).all())


# ---- 7. repeatable and capturable -------------------------------------------------------------------------------------------------------
def test_repeatable_and_capturable(dm, exact):
    from harp_amd import ops
    sc = exact
    kw = dict(iters=6, verts=True, jac=True, normal=True)
    a = _solve(dm, sc["x0_32"], sc["targets32"], **kw)
    b = _solve(dm, sc["x0_32"], sc["targets32"], **kw)
    assert _same(a, b)
    # one captured call through out=, replayed on fresh inputs
    targets, pose48, betas, trans = (_f32(t).clone() for t in (sc["targets32"], sc["x0_32"][:, :48], sc["x0_32"][:, 48:58], sc["x0_32"][:, 58:]))
    out = ops.mano_vertex_fit(dm, targets, pose48, betas, trans, **kw)           # warm-up outside the capture; its tensors are reused
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mano_vertex_fit(dm, targets, pose48, betas, trans, out=out, **kw)
    half = slice(0, 4)
    flipped = torch.arange(7, -1, -1)
    for order in (torch.arange(8), flipped):                                     # fresh inputs: the frames in another order
        targets.copy_(_f32(sc["targets32"][order])); pose48.copy_(_f32(sc["x0_32"][order, :48]))
        betas.copy_(_f32(sc["x0_32"][order, 48:58])); trans.copy_(_f32(sc["x0_32"][order, 58:]))
        for t in out:
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(x[order]), _bits(y)) for x, y in zip(a, out)), order[half]


# ---- 8. the preprocessing layer ---------------------------------------------------------------------------------------------------------
def test_preprocessing_lm_against_adam(capsys):
    from harp_amd.manopth.manolayer import ManoLayer
    from harp_amd.metro_modifications import hand_utils as hu
    from tests._scene import make_scene
    from tests.test_metro_fit import _targets
    sc = make_scene(T=2, S=32, seed=2)
    layer = ManoLayer(flat_hand_mean=False, use_pca=False, model=sc["model_np"], device=DEV)
    pred = _targets(sc, 4, seed=5)
    adam = hu.optimize_for_mano_param(pred, layer)
    capsys.readouterr()
    lm = hu.optimize_for_mano_param(pred, layer, method="lm")
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("After coarse alignment: ") and lines[1].startswith("After fine alignment: ") and len(lines) == 2
    assert sorted(lm) == sorted(adam)
    for k in adam:
        assert lm[k].shape == adam[k].shape and lm[k].dtype == adam[k].dtype, k
    rms = lambda o: float(np.sqrt(((o["verts"].astype(np.float64) - pred.numpy().astype(np.float64) * 1000.0) ** 2).sum(-1).mean()))
    print(f"[vertex_fit] preprocessing rms lm {rms(lm):.3e} mm adam {rms(adam):.3e} mm; printed {lines}")
    assert rms(lm) <= rms(adam)
    assert abs(float(lines[1].split(":")[1]) - rms(lm) ** 2 / 3.0) <= 1e-5 + 0.05 * rms(lm) ** 2


# ---- 9. playback --------------------------------------------------------------------------------------------------------------------------
def _playback_scene(tmp_path, T=5, S=32):
    from harp_amd.playback import Motion
    from tests.test_gpu_evaluate import _setup
    _, cfg, layer, params, _ = _setup(T, S, 3, tmp_path)
    true = Motion.from_params(params)
    betas = params["shape"].detach().reshape(1, 10).expand(T, 10).contiguous()

    def forward(m):
        with torch.no_grad():
            return layer(torch.cat([m.rot, m.pose], 1).to(DEV), betas, m.trans.to(DEV))[0]

    return cfg, layer, params, true, forward


def test_motion_from_vertices_drives_the_player(tmp_path, exact):
    from harp_amd.playback import AvatarPlayer, Motion
    T = 5
    cfg, layer, params, true, forward = _playback_scene(tmp_path, T)
    v = forward(true) / 1000.0
    rec = Motion.from_vertices(v, params, layer)
    assert len(rec) == T and rec.light_positions is None and torch.equal(rec.cam.cpu(), params["cam"][0].detach().cpu().expand(T, 3))
    rms = float((forward(rec) / 1000.0 - v).double().pow(2).sum(-1).mean(1).sqrt().max() * 1000.0)
    bound = R.FACTOR * float(R.rms_mm(exact["model"], exact["y32"]["x"], exact["targets32"], torch.float32).max())
    print(f"[vertex_fit] layer rms {rms:.3e} mm (bound {bound:.3e}, test 3's)")
    assert rms <= bound
    with pytest.raises(NotImplementedError):
        Motion.from_vertices(v, params, _ik_ref._Layer(dict(layer._model_np, pose_mean=np.zeros(165))))
    warm = Motion.from_vertices(v, params, layer, init=rec, iters=1)
    assert float((warm.pose - rec.pose).abs().max()) < 1e-3
    player = AvatarPlayer(cfg, params, layer, batch_size=T, ss=1, device=DEV)
    white = lambda fr: int((fr.cpu() != 255).any(-1).sum())
    player.load_motion(true)
    n_true = white(player.render(np.arange(T)))
    player.load_motion(Motion(rec.pose, rec.rot, rec.trans, true.cam))      # the true motion's per-frame cam: the two renders are comparable
    n_rec = white(player.render(np.arange(T)))
    print(f"[vertex_fit] layer covered pixels true {n_true} recovered {n_rec}")
    assert n_true > 0 and abs(n_rec - n_true) <= 0.01 * n_true


def test_command_line_takes_vertices(tmp_path, monkeypatch):
    """python -m harp_amd.playback's main() with --vertices (the two loaders of licensed / fitted files replaced by the synthetic scene, as
    tests/test_gpu_avatar_player.py does): vertices, weights and cam in, frames out"""
    import os
    import yaml
    from PIL import Image
    from harp_amd import playback
    from harp_amd.utils import file_utils, hand_model_utils
    T, S = 5, 32
    cfg, layer, params, true, forward = _playback_scene(tmp_path, T, S)
    monkeypatch.setattr(hand_model_utils, "load_hand_model", lambda c: (layer, params["verts_uvs"], params["faces_uvs"], None))
    monkeypatch.setattr(file_utils, "load_result", lambda base, device="cuda", test=False: dict(params))
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump({k: cfg[k] for k in ("use_arm", "img_size", "focal_length", "self_shadow", "share_light_position", "base_output_dir")}, f)
    np.savez(tmp_path / "v.npz", vertices=(forward(true) / 1000.0).cpu().numpy(), weights=np.ones((T, 778), np.float32), cam=true.cam.cpu().numpy())
    out = tmp_path / "frames"
    paths = playback.main(["--config", str(tmp_path / "cfg.yaml"), "--out", str(out), "--vertices", str(tmp_path / "v.npz"), "--batch-size", "4"])
    assert sorted(os.listdir(out)) == ["%04d.jpg" % i for i in range(T)] and len(paths) == T
    assert Image.open(paths[0]).size == (S, S)
