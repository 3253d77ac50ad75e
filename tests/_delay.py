"""Deterministic delay injection for the stream-ordering tests (a test helper, not a conftest).

Every GPU test synchronises before it reads a result, which hides a reader that runs ahead of its writer on another stream.  `delayed()`
makes one side of the step's fork late on purpose: in front of every `harp_*` launch that takes a stream, it enqueues a calibrated busy
wait (`torch.cuda._sleep`) on that launch's stream.  A missing edge between two streams then shows on every run instead of when the
hardware happens to interleave them badly."""
import contextlib
import os
import re
import sys
import threading

import torch

from harp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET_US = 300.0                                   # well above any single kernel of the step at S = 128, B = 3
_cal = {}


def stream_entry_points():
    """names of the C-ABI functions whose declaration in include/harp_hip.h ends in `hipStream_t stream`"""
    with open(os.path.join(ROOT, "include", "harp_hip.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    names = [n for n, args in re.findall(r"\b(harp_\w+)\s*\(([^;{]*?)\)\s*;", src) if re.search(r"hipStream_t\s+stream$", args.strip())]
    assert len(names) > 50, names                     # (the parser still finds the header's launches)
    return names


def _time_us(fn, reps=5):
    """median wall time of fn() on the current stream, CUDA events"""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[len(ts) // 2]


def _sleep_fn():
    """(n -> enqueue a busy wait of n units on the current stream, what the unit is): torch's clock64 spin kernel, or — where that is
    unusable — a chain of n dependent element-wise kernels on a scratch tensor"""
    try:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        return torch.cuda._sleep, "clock64 cycles"
    except Exception:
        scratch = torch.zeros(1 << 16, device="cuda")

        def chain(n):
            for _ in range(int(n)):
                scratch.mul_(1.0)
        return chain, "element-wise launches"


def calibrate():
    """(sleep function, n, measured µs): n units of the busy wait take about TARGET_US.  How clock64 maps to wall time on the device is
    measured here, not assumed (once per process)."""
    if not _cal:
        sleep, unit = _sleep_fn()
        n1 = 20000 if unit.startswith("clock") else 4
        _time_us(lambda: sleep(n1), 2)                  # (first launch: code-object load)
        t1, t2 = _time_us(lambda: sleep(n1)), _time_us(lambda: sleep(2 * n1))
        per = max(t2 - t1, 1e-3) / n1
        n = max(1, int(round(TARGET_US / per)))
        us = _time_us(lambda: sleep(n))
        print(f"[delay] {n} {unit} -> {us:.0f} us ({per * 1e3:.3f} ns per unit)")
        assert 100.0 <= us <= 2000.0, (n, unit, us)
        _cal.update(sleep=sleep, n=n, us=us, unit=unit)
    return _cal["sleep"], _cal["n"], _cal["us"]


@contextlib.contextmanager
def delayed(eng, where):
    """Inside the context, every stream launch of the C ABI that runs on the step's second (and further) streams — where="side" — or on
    its main stream — where="main" — waits the calibrated delay first.  The main stream is the stream current when `eng.forward_backward`
    was last entered (under capture: torch's capture stream).  "side" makes every side-branch producer late: it catches a main-stream
    reader without a join.  "main" makes the main-stream producers late: it catches a side-stream reader without a wait.  Captured graphs
    do not contain the delays: the engine's graph cache is emptied on entry and on exit."""
    assert where in ("side", "main"), where
    sleep, n, _ = calibrate()
    L = _lib.lib()
    state = {"main": None}
    side = where == "side"

    def wrap(fn):
        def call(*args):
            m = state["main"]
            if m is not None and (torch.cuda.current_stream().cuda_stream != m) == side:
                sleep(n)
            return fn(*args)
        return call

    saved = {name: getattr(L, name) for name in stream_entry_points()}
    fb = eng.forward_backward

    def forward_backward(*args, **kw):
        state["main"] = torch.cuda.current_stream().cuda_stream
        return fb(*args, **kw)

    for name, fn in saved.items():
        setattr(L, name, wrap(fn))
    eng.forward_backward = forward_backward
    eng._graphs = {}
    try:
        yield
    finally:
        del eng.forward_backward                     # (the instance attribute: the class's method shows again)
        for name, fn in saved.items():
            setattr(L, name, fn)
        eng._graphs = {}


# ---- host / device hand-offs (tests/test_gpu_handoffs.py) ------------------------------------------------------------------------------
# Where the HOST can run ahead of the device — a pinned buffer rewritten before its copy has run, a pinned buffer read before its copy
# has landed — the device is made late by whole milliseconds, and the host-side waits are watched: a run proves something only if one
# of its waits really found its event incomplete.
_EVENT_BASE = torch._C._CudaEventBase                   # the methods under torch.cuda.Event's wrappers: what the spies call through to
_waits_checked = {}


def busy_wait(ms):
    """Enqueue a busy wait of about `ms` milliseconds on the current stream: calibrate()'s busy wait, scaled by the time per unit it
    measured.  The first call per process and length times one such wait with events (and waits for it) and asserts that it took
    between 0.5 x and 2 x the request; every call then enqueues the wait and returns at once."""
    sleep, n, us = calibrate()
    units = max(1, int(round(n * (float(ms) * 1e3 / us))))
    if units not in _waits_checked:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sleep(units)
        e1.record()
        _EVENT_BASE.synchronize(e1)                      # (not through torch.cuda.Event.synchronize: a wait_spy may have it)
        took = e0.elapsed_time(e1)
        print(f"[delay] busy_wait({ms:.1f} ms): {units} {_cal['unit']} took {took:.1f} ms")
        assert 0.5 * ms <= took <= 2.0 * ms, (ms, units, took)
        _waits_checked[units] = took
    sleep(units)


@contextlib.contextmanager
def late_calls(obj, name, ms):
    """Inside the context every call of the Python attribute `obj.name` (a function of a module, a method of an instance) first enqueues
    busy_wait(ms) on the stream current at that moment: the device work of every such call starts `ms` late.  The attribute is restored
    on exit (an instance's own attribute that hid its class's method is deleted again)."""
    own = name in vars(obj)
    fn = getattr(obj, name)

    def call(*args, **kw):
        busy_wait(ms)
        return fn(*args, **kw)

    setattr(obj, name, call)
    try:
        yield
    finally:
        if own:
            setattr(obj, name, fn)
        else:
            delattr(obj, name)


@contextlib.contextmanager
def wait_spy(bypass=False, method="synchronize"):
    """Wrap torch.cuda.Event.synchronize (or, with method="query", torch.cuda.Event.query) and yield the list of records, one dict per
    call: `complete` — for synchronize: self.query() as it was on entry; for query: what it returned — `thread`, the calling thread's
    name, and `where`, the name of the calling function.  synchronize calls through unless `bypass` is true (the positive controls: the
    host then does not wait).  The method is restored on exit.  A record with complete == False is the proof that the host reached a
    wait before the device had got there: without one a delayed run has not opened the window it claims to test."""
    assert method in ("synchronize", "query") and not (bypass and method == "query"), (method, bypass)
    records = []
    saved = getattr(torch.cuda.Event, method)

    def spy(self):
        rec = dict(complete=None, thread=threading.current_thread().name, where=sys._getframe(1).f_code.co_name)
        if method == "query":
            rec["complete"] = bool(saved(self))
            records.append(rec)
            return rec["complete"]
        rec["complete"] = bool(_EVENT_BASE.query(self))
        records.append(rec)
        if not bypass:
            saved(self)

    setattr(torch.cuda.Event, method, spy)
    try:
        yield records
    finally:
        setattr(torch.cuda.Event, method, saved)


def incomplete(records, where=None, thread=None):
    """how many of wait_spy's records found their event incomplete, of those made in function `where` / on thread `thread`"""
    return sum(1 for r in records if not r["complete"] and where in (None, r["where"]) and thread in (None, r["thread"]))
