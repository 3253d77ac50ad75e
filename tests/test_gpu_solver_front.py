"""GPU: the Python front of the five batched LM solvers (harp_amd/ops.py: mano_ik, mano_reproj_ik, mano_vertex_fit, arm_ik, arm_vertex_fit;
DESIGN.md §34) with real buffers, on the synthetic hand and the synthetic arm at T = 2 and iters = 0: the plain call, every refusal that
the wrappers share — what tests/test_gpu_arm_ik.py::test_refusals_with_real_buffers holds for one of them — and out=."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 2
CAM, FOCAL, S = (8.9, 0.01, -0.02), 2000.0, 448
SOLVERS = ("mano_ik", "mano_reproj_ik", "mano_vertex_fit", "arm_ik", "arm_vertex_fit")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def models():
    import harp_amd
    from harp_amd import synth
    from harp_amd.hand_models_harp.body_models import SMPLXARM
    from harp_amd.manopth.manolayer import ManoLayer
    hand = ManoLayer(flat_hand_mean=False, use_pca=False, model=synth.make_mano_model(), device=DEV).device_model
    m = synth.make_smplx_arm_model(seed=0)
    corr = np.load(os.path.join(os.path.dirname(os.path.abspath(harp_amd.__file__)), "assets", "arm_corr.npz"))
    return dict(hand=hand, arm=SMPLXARM(m, m["faces"], corr["mano_vert_from_arm"], device=DEV).device_model)


def _case(name, models):
    """dict(dm, args: the tensors by name in the wrapper's positional order, tail: what follows them, start: the name of the start rows and
    a tensor of a wrong shape for them, opt: the switch of an optional output = its field, weight: one of the solver's weights)"""
    rng = np.random.default_rng(5)
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=DEV)      # noqa: E731
    r = lambda *s: up(rng.normal(size=s) * 0.05)      # noqa: E731
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    if name in ("mano_ik", "mano_reproj_ik", "mano_vertex_fit"):
        dm, start, bad = models["hand"], "pose48", z(T, 51)
        rows = dict(pose48=r(T, 48), trans=r(T, 3))
    else:
        dm, start, bad = models["arm"], "in_pose", z(T, 51)
        rows = dict(in_pose=r(T, 17, 3), trans=r(T, 3))
    (k0, v0), (k1, v1) = rows.items()
    if name == "mano_ik":
        return dict(dm=dm, args={"betas": r(10), "targets": r(T, 21, 3), k0: v0, k1: v1}, tail=(), start=(start, bad), opt="joints",
                    weight="prior_weight")
    if name == "mano_reproj_ik":
        px = up(np.concatenate([S / 2 + rng.normal(size=(T, 21, 2)) * 20.0, rng.normal(size=(T, 21, 1)) * 0.02], -1))
        return dict(dm=dm, args={"betas": r(10), "targets": px, k0: v0, k1: v1, "cam": up(CAM)}, tail=(FOCAL, S), start=(start, bad), opt="proj",
                    weight="pose_prior_weight")
    if name == "arm_ik":
        n = int(dm.struct.n_joints_out)
        return dict(dm=dm, args={"betas": r(10), "targets": r(T, n, 3), k0: v0, k1: v1}, tail=(), start=(start, bad), opt="joints",
                    weight="wrist_prior_weight")
    nv = 778 if name == "mano_vertex_fit" else int(dm.NV)
    return dict(dm=dm, args={"targets": r(T, nv, 3), k0: v0, "betas": r(T, 10), k1: v1}, tail=(), start=(start, bad), opt="verts",
                weight="pose_prior_weight")


@pytest.mark.parametrize("name", SOLVERS)
def test_plain_call_refusals_and_out(name, models):
    from harp_amd import ops
    c = _case(name, models)
    fn, dm, args, tail = getattr(ops, name), c["dm"], c["args"], c["tail"]
    call = lambda kw=None, **changed: fn(dm, *dict(args, **changed).values(), *tail, iters=0, **(kw or {}))      # noqa: E731
    kept = {k: v.clone() for k, v in args.items()}

    first = call()
    assert first.status.tolist() == [0, 0]
    assert getattr(first, c["opt"]) is None
    assert all(torch.equal(_bits(args[k]), _bits(kept[k])) for k in args)            # the start is left untouched

    # the refusals of test_refusals_with_real_buffers, in its exception types, with the field named
    with pytest.raises(ValueError, match="targets"):
        call(targets=args["targets"][:, :-1].contiguous())
    start, bad = c["start"]
    with pytest.raises(ValueError, match=start):
        call(**{start: bad})
    with pytest.raises(ValueError, match="betas"):
        call(betas=torch.zeros(3, 10, device=DEV))
    with pytest.raises(ValueError, match=c["weight"]):
        call({c["weight"]: -1.0})
    with pytest.raises(TypeError, match="targets"):
        call(targets=args["targets"].double())
    with pytest.raises(RuntimeError, match="forward-only"):
        call(**{start: args[start].clone().requires_grad_()})
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(trans=args["trans"].cpu())
    with pytest.raises(ValueError, match=f"out.{c['opt']}"):
        call({c["opt"]: True, "out": first})

    # out=: the same tensor objects are written, and they hold the first call's bits
    want = call({c["opt"]: True})
    out = call({c["opt"]: True})
    assert out is not want and getattr(out, c["opt"]) is not None
    for t in out:
        if t is not None:
            t.fill_(7)
    again = call({c["opt"]: True, "out": out})
    assert all(a is b for a, b in zip(again, out))
    for f, a, b in zip(want._fields, again, want):
        assert (a is None) == (b is None), f
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), f
    for f in first._fields:                                                           # and the optional output changes nothing else
        if getattr(first, f) is not None:
            assert torch.equal(_bits(getattr(first, f)), _bits(getattr(want, f))), f
