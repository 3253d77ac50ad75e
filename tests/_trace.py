"""Enqueue trace of the fitting step (a test helper in the style of tests/_delay.py, not a conftest).

Capture order is behaviour: of the kernels that depend on one node, hipGraph keeps the first-captured one on that node's stream
(DESIGN.md §2), so a step that enqueues the same launches in another order replays slower with identical numbers.  `traced()` records
what the engine enqueues, in order, in a form that is the same from process to process (no addresses, no handles):

  [name, stream, arg, ...]         a C-ABI call that takes a stream (tests/_delay.stream_entry_points()): ordinal of the current stream,
                                   then every argument — integers and floats by value, pointers as 0 (null) / 1, a `byref(struct)` as
                                   the list of its fields (nested structs and arrays as nested lists), the stream argument as "s<ordinal>"
  ["wait_stream", stream, other]   Stream.wait_stream
  ["wait_event", stream, event]    Stream.wait_event   (events are numbered in record order; -1: recorded outside the trace)
  ["record_event", stream, event]  Stream.record_event
  ["zero_", stream, numel]         Tensor.zero_ of a device tensor (the engine's own clears: gs_zero, gs_mesh, gs_zero_late, ...)

Streams are numbered in order of first appearance; the stream current on entry is 0.

`configurations()` lists what tests/golden/step_traces.json holds (written by tests/golden/make_step_traces.py at the commit whose
schedule is the reference, replayed by tests/test_gpu_step_trace.py)."""
import contextlib
import ctypes
import json
import os

import torch

from harp_amd import _lib
from tests._delay import stream_entry_points

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_traces.json")
LW = [1, 1 / 16, 1 / 8, 1 / 4, 1]
_POINTERS = (ctypes.c_void_p, ctypes.c_char_p)


def _value(v):
    """one ctypes field / element in the trace's form"""
    if isinstance(v, ctypes.Structure):
        return [_value(getattr(v, name)) for name, _ in v._fields_]
    if isinstance(v, ctypes.Array):
        return [_value(x) for x in v]
    return v


def _struct(obj):
    out = []
    for name, ctype in obj._fields_:
        v = getattr(obj, name)
        if issubclass(ctype, _POINTERS):
            out.append(int(bool(v)))
        elif issubclass(ctype, ctypes.Array) and issubclass(ctype._type_, _POINTERS):
            out.append([int(bool(x)) for x in v])
        elif issubclass(ctype, ctypes.Structure):
            out.append(_struct(v))
        else:
            out.append(_value(v))
    return out


def _arg(a, ctype):
    if hasattr(a, "_obj"):                              # ctypes.byref(struct)
        return _struct(a._obj)
    if ctype is not None and issubclass(ctype, _POINTERS + (ctypes._Pointer,)):
        return int(bool(a))
    if a is None:
        return 0
    return float(a) if isinstance(a, float) else int(a)


@contextlib.contextmanager
def traced():
    """Inside the context, everything enqueued through the C ABI, the stream ordering calls and the device-tensor clears are appended
    to the list the context yields."""
    L = _lib.lib()
    entries, streams, events, keep = [], {}, {}, []
    depth = [0]

    def ordinal(handle):
        return streams.setdefault(int(handle or 0), len(streams))

    cur = lambda: ordinal(torch.cuda.current_stream().cuda_stream)
    cur()                                               # the main stream is 0

    def wrap(name, fn):
        types = list(fn.argtypes)

        def call(*args):
            e = [name, cur()] + [_arg(a, t) for a, t in zip(args[:-1], types)] + ["s%d" % ordinal(args[-1])]
            entries.append(e)
            return fn(*args)
        return call

    saved = {name: getattr(L, name) for name in stream_entry_points()}
    S = torch.cuda.Stream
    wait_stream, wait_event, record_event, zero_ = S.wait_stream, S.wait_event, S.record_event, torch.Tensor.zero_

    def nested(fn, *args):                               # (torch's wait_stream is record_event + wait_event: one entry, not three)
        depth[0] += 1
        try:
            return fn(*args)
        finally:
            depth[0] -= 1

    def t_wait_stream(self, other):
        if not depth[0]:
            entries.append(["wait_stream", ordinal(self.cuda_stream), ordinal(other.cuda_stream)])
        return nested(wait_stream, self, other)

    def t_wait_event(self, event):
        if not depth[0]:
            entries.append(["wait_event", ordinal(self.cuda_stream), events.get(id(event), -1)])
        return nested(wait_event, self, event)

    def t_record_event(self, event=None):
        ev = nested(record_event, self, event)
        if not depth[0]:
            keep.append(ev)                              # (alive until the context ends: id() stays unique)
            events[id(ev)] = len(keep) - 1
            entries.append(["record_event", ordinal(self.cuda_stream), events[id(ev)]])
        return ev

    def t_zero_(self):
        if self.is_cuda and not depth[0]:
            entries.append(["zero_", cur(), self.numel()])
        return zero_(self)

    own_zero = "zero_" in torch.Tensor.__dict__
    for name, fn in saved.items():
        setattr(L, name, wrap(name, fn))
    S.wait_stream, S.wait_event, S.record_event, torch.Tensor.zero_ = t_wait_stream, t_wait_event, t_record_event, t_zero_
    try:
        yield entries
    finally:
        S.wait_stream, S.wait_event, S.record_event = wait_stream, wait_event, record_event
        if own_zero:
            torch.Tensor.zero_ = zero_
        else:
            del torch.Tensor.zero_
        for name, fn in saved.items():
            setattr(L, name, fn)


# ----------------------------------------------------------------------------------------------------------------------
# the configurations of the golden file
# ----------------------------------------------------------------------------------------------------------------------
STAGES = {"TT": (True, True), "TF": (True, False), "FT": (False, True)}
KNOWN_APPEARANCE_OFF = ("kps_anchor", "vert_disp_reg", "laplacian", "normal", "arap")       # optimize_sequence.py, known_appearance


def _tag(d):
    return ",".join(f"{k}={'+'.join(v) if isinstance(v, (list, tuple)) else v}" for k, v in d.items()) or "default"


def configurations():
    """{name: spec}; spec = dict(kind, stage, fid (explicit frame ids instead of the schedule), attrs (set on the engine), disabled (terms),
    vgg (perceptual term on, in this precision))"""
    from tests._scene import SCHEDULE_SWITCHES
    from tests.test_gpu_stream_order import SWITCHES
    out = {}

    def add(kind, stage, attrs=None, fid=False, **special):
        attrs = dict(attrs or {})
        name = "/".join([kind, stage, "fid" if fid else "sched", _tag({**attrs, **special})])
        out.setdefault(name, dict(kind=kind, stage=stage, fid=fid, attrs=attrs, **special))

    lists = [dict()] + list(SCHEDULE_SWITCHES) + [c for c in SWITCHES if isinstance(c, dict)]
    for sw in lists:
        add("hand", "TT", sw)
    for sw in lists:                                     # the default and every single-switch flip at the other stages and unfolded
        if len(sw) <= 1:
            add("hand", "TF", sw)
            add("hand", "FT", sw)
            add("hand", "TT", sw, fid=True)
    for stage in STAGES:
        for sw in (dict(), dict(wide_front=False), dict(wide_back=False), dict(fused_front=False)):
            add("arm", stage, sw)
    for sw in (dict(fused_chain=False), dict(fused_back=False), dict(keep_image=True), dict(auto_draw=True),
               dict(frozen=("texture", "normal_map")), dict(force_allreduce=True), dict(force_allreduce=True, texel_records=False),
               dict(accumulate_loss=True)):
        add("hand", "TT", sw)
    add("hand", "FT", dict(lean_app_stage=True))
    add("hand", "TT", disabled=list(KNOWN_APPEARANCE_OFF))
    for stage in ("TT", "FT"):
        for n in (1, 2):
            add("hand", stage, dict(vgg_streams=n), vgg="f32")
    add("hand", "TT", dict(vgg_streams=2), vgg="f16")       # ("perceptual" of tests/test_gpu_stream_order.SWITCHES; "arm" is arm/TT above)
    return out


def fit_case(kind):
    """the scene of the switch tests (tests/test_gpu_parity.py, tests/test_gpu_stream_order.py): 2x2 super-tiles, 8x8 tiles, lr = 0 and a
    one-row schedule, so every step starts from the same state"""
    from tests._scene import make_fit_case
    case = make_fit_case(kind, T=3, S=128, B=3, seed=4, device="cuda")
    eng = case["eng"]
    eng.keep_image = False
    eng.auto_draw = False
    eng.draw_texture_offsets()
    eng.set_lr(0.0, 0.0)
    eng.set_schedule(torch.arange(3).reshape(1, 3).int())
    return case


_vgg = []


def trace_configuration(eng, spec):
    """the entries of one eager step (forward_backward, allreduce, adam) of `eng` under `spec`; one untraced step runs first and absorbs
    the lazy work (stream creation, record buffers, the silhouette records' re-bind, the shadow state after a consume_gzl / keep_depth
    flip).  The engine is left as it was."""
    attrs = spec["attrs"]
    defaults = {k: getattr(eng, k) for k in attrs}
    coarse, app = STAGES[spec["stage"]]
    fid = torch.arange(3) if spec["fid"] else None
    try:
        for k, v in attrs.items():
            setattr(eng, k, tuple(v) if isinstance(v, (list, tuple)) else v)
        if spec.get("disabled"):
            eng.set_disabled_terms(spec["disabled"])
        if spec.get("vgg"):
            from harp_amd.model.vgg import Vgg16Features
            if not _vgg:
                _vgg.append(Vgg16Features(layers_weights=LW, weights="random", seed=2))
            eng.set_perceptual(_vgg[0], precision={"f32": 0, "f16": 2}[spec["vgg"]])
        eng.step(fid, coarse, app, use_graph=False)
        torch.cuda.synchronize()
        with traced() as entries:
            eng.step(fid, coarse, app, use_graph=False)
        torch.cuda.synchronize()
        return json.loads(json.dumps(entries))           # (what the golden file holds: lists, ints, floats, strings)
    finally:
        for k, v in defaults.items():
            setattr(eng, k, v)
        if spec.get("disabled"):
            eng.set_disabled_terms(())
        if spec.get("vgg"):
            eng.set_perceptual(None)
        eng._graphs = {}


def first_difference(got, ref):
    """None, or a readable report of the first entry that differs, with its two neighbours"""
    for i in range(max(len(got), len(ref))):
        a, b = (got[i] if i < len(got) else None), (ref[i] if i < len(ref) else None)
        if a != b:
            lines = [f"entry {i} of {len(got)} (golden: {len(ref)})"]
            for j in range(max(0, i - 1), i + 2):
                for tag, t in (("golden", ref), ("now   ", got)):
                    lines.append(f"  [{j}] {tag} {json.dumps(t[j]) if j < len(t) else '(none)'}")
            return "\n".join(lines)
    return None
