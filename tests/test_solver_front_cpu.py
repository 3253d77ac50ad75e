"""CPU checks of the front that the five batched LM solvers' wrappers share (harp_amd/ops.py: _lm_float32, _lm_shapes, _lm_scalars,
_lm_result, _lm_start, _lm_input).  The device and forward-only check is a step of its own (_playback_input), so these are
plain Python on CPU tensors."""
import collections

import pytest
import torch

from harp_amd import ops

T = 2
Result = collections.namedtuple("Result", "rows cost status extra")
WANT = ((T, 48), (T, 2), (T,), None)
CPU = torch.device("cpu")


def test_a_float64_field_is_named():
    ok = dict(betas=torch.zeros(10), targets=torch.zeros(T, 21, 3), weights=None)
    ops._lm_float32("mano_ik", **ok)
    for name in ("betas", "targets"):
        with pytest.raises(TypeError, match=f"mano_ik takes float32 tensors, {name} is torch.float64"):
            ops._lm_float32("mano_ik", **dict(ok, **{name: ok[name].double()}))
    with pytest.raises(TypeError, match="weights"):
        ops._lm_float32("mano_ik", **dict(ok, weights=torch.zeros(T, 21, dtype=torch.int32)))


def test_a_wrong_shape_is_named_with_both_shapes():
    ops._lm_shapes(("pose48", torch.zeros(T, 48), (T, 48)), ("prior", None, (T, 45)))
    with pytest.raises(ValueError, match=r"pose48 must be \(2, 48\), got \(2, 51\)"):
        ops._lm_shapes(("trans", torch.zeros(T, 3), (T, 3)), ("pose48", torch.zeros(T, 51), (T, 48)))
    with pytest.raises(ValueError, match=r"z_prior must be \(2,\), got \(2, 1\)"):
        ops._lm_shapes(("z_prior", torch.zeros(T, 1), (T,)))


def test_one_of_two_shapes():
    for name, w in (("betas", 10), ("cam", 3)):
        for good in ((w,), (T, w)):
            ops._lm_shapes((name, torch.zeros(good), [(w,), (T, w)]))
        with pytest.raises(ValueError, match=rf"{name} must be \({w},\) or \(2, {w}\), got \(3, {w}\)"):
            ops._lm_shapes((name, torch.zeros(3, w), [(w,), (T, w)]))
    with pytest.raises(ValueError, match=r"betas must be \(2, 10\), got \(10,\)"):      # a solved shape is per frame
        ops._lm_shapes(("betas", torch.zeros(10), [(T, 10)]))


@pytest.mark.parametrize("bad", [-1.0, float("inf"), float("-inf"), float("nan")])
def test_a_weight_must_be_finite_and_not_negative(bad):
    ops._lm_scalars(0, lambda0=0.0, pose_prior_weight=1e-4)
    for name in ("lambda0", "pose_prior_weight"):
        with pytest.raises(ValueError, match="iters >= 0 and finite lambda0, pose_prior_weight >= 0, got 3, "):
            ops._lm_scalars(3, **dict(dict(lambda0=1e-3, pose_prior_weight=0.0), **{name: bad}))


def test_iters_must_not_be_negative():
    with pytest.raises(ValueError, match="got -1, 0.001"):
        ops._lm_scalars(-1, lambda0=1e-3)


def _fitting():
    return Result(torch.zeros(T, 48), torch.zeros(T, 2), torch.zeros(T, dtype=torch.int32), None)


def test_a_new_result_has_the_wanted_fields():
    r = ops._lm_result(Result, WANT, None, CPU)
    assert isinstance(r, Result) and r.extra is None
    assert [tuple(t.shape) for t in r[:3]] == list(WANT[:3])
    assert [t.dtype for t in r[:3]] == [torch.float32, torch.float32, torch.int32]
    assert ops._lm_result(Result, WANT[:3] + ((T, 21, 3),), None, CPU).extra.shape == (T, 21, 3)


def test_a_fitting_out_is_returned_as_it_is():
    out = _fitting()
    got = ops._lm_result(Result, WANT, out, CPU)
    assert got is out and all(a is b for a, b in zip(got, out))
    ops._lm_start(got, rows=torch.ones(T, 48, requires_grad=True))
    assert got.rows is out.rows and bool((out.rows == 1).all()) and not out.rows.requires_grad


@pytest.mark.parametrize("field,change,want", [
    ("extra", lambda t: torch.zeros(T, 21, 3), WANT),                                   # present but not wanted
    ("extra", lambda t: None, WANT[:3] + ((T, 21, 3),)),                                # wanted but None
    ("rows", lambda t: None, WANT),
    ("rows", lambda t: torch.zeros(T, 51), WANT),                                       # the wrong shape
    ("cost", lambda t: torch.zeros(T + 1, 2), WANT),
    ("rows", lambda t: torch.zeros(48, T).t(), WANT),                                   # the right shape, not contiguous
    ("status", lambda t: torch.zeros(T), WANT),                                         # status is the int32 field
    ("rows", lambda t: t.to(torch.int32), WANT),                                        # and the only one
    ("cost", lambda t: t.double(), WANT),
])
def test_an_out_that_does_not_fit_is_refused(field, change, want):
    out = _fitting()
    out = out._replace(**{field: change(getattr(out, field))})
    with pytest.raises(ValueError, match=f"out.{field} does not fit this call"):
        ops._lm_result(Result, want, out, CPU)


def test_an_out_on_another_device_is_refused():
    with pytest.raises(ValueError, match="out.rows does not fit this call"):
        ops._lm_result(Result, WANT, _fitting(), torch.device("meta"))


def test_a_contiguous_input_is_passed_on_without_a_copy():
    t = torch.zeros(T, 21, 3)
    assert ops._lm_input(t) is t and ops._lm_input(None) is None
    v = torch.zeros(3, 21, T).permute(2, 1, 0)
    c = ops._lm_input(v.requires_grad_())
    assert c.is_contiguous() and not c.requires_grad and c.data_ptr() != v.data_ptr()


def test_the_model_and_the_targets_share_a_device():
    Model = collections.namedtuple("Model", "v_template")
    ops._lm_model_device(Model(torch.zeros(3)), torch.zeros(T, 21, 3))
    with pytest.raises(ValueError, match="the model is on meta, the targets on cpu"):
        ops._lm_model_device(Model(torch.zeros(3, device="meta")), torch.zeros(T, 21, 3))
